"""Writer of `Wiscombe` and `HanrahanKrueger` object streams, for the byte-level tests of integration/streamparse.h
(tests/test_stream_parsers_snow.py).  Test infrastructure, next to tests/mts_stream_writer_mask.py.

Wiscombe::serialize (src/bsdfs/wiscombe.cpp:172-179): BSDF::serialize (the parent reference and the name), then m_g, m_depth,
m_w0 and m_sigmaT.  HanrahanKrueger::serialize (src/bsdfs/hanrahan-krueger.cpp:225-230): BSDF::serialize, then m_sizeMultiplier,
m_sigmaA and m_sigmaS -- and nothing of g, the two indices, the two factors and the flag."""
import mts_stream_writer as W


def wiscombe(key, g=0.874, depth=1.0, w0=(0.99, 0.99, 0.99), sigma_t=(16.4967, 6.0957, 4.6547), name=""):
    """a nested-instance writer: callable (s)"""
    def write(s):
        def body(s):
            W.configurable(s); s.string(name)
            s.float(g); s.float(depth)
            s.spectrum(w0); s.spectrum(sigma_t)
        s.ref(key, "Wiscombe", body)
    return write


def hanrahan_krueger(key, size_multiplier=1.0, sigma_a=(0.0014, 0.0025, 0.0142), sigma_s=(0.7, 1.22, 1.9), name=""):
    def write(s):
        def body(s):
            W.configurable(s); s.string(name)
            s.float(size_multiplier)
            s.spectrum(sigma_a); s.spectrum(sigma_s)
        s.ref(key, "HanrahanKrueger", body)
    return write
