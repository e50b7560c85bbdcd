"""Writer of `IrawanClothBRDF` object streams, for the byte-level tests of integration/streamparse.h
(tests/test_stream_parsers_cloth.py).  Test infrastructure, next to tests/mts_stream_writer_snow.py.

IrawanClothBRDF::serialize (src/bsdfs/irawan.cpp:265-273): BSDF::serialize (the parent reference and the name), then
WeavePattern::serialize (irawan.h:191-211) -- the name, alpha, beta, ss, hWidth, warpArea, weftArea, tileWidth and tileHeight as
uints, the four d*UmaxOverD*, fineness, period, the pattern as an array of uints, the yarn count as a size, and per yarn
(irawan.h:88-99) the type as an int, psi, umax, kappa, width, length, centerU, centerV and the two Spectrums -- then repeatU,
repeatV, kdMultiplier and ksMultiplier."""
import struct

import mts_stream_writer as W


def irawan(key, weave, name="", yarn_count=None, pattern=None):
    """a nested-instance writer: callable (s).  weave: a scenes.Weave; yarn_count / pattern override what is written"""
    def write(s):
        def body(s):
            W.configurable(s); s.string(name)
            s.string(weave.name)
            for n in ("alpha", "beta", "ss", "hWidth", "warpArea", "weftArea"):
                s.float(getattr(weave, n))
            s.uint(weave.tileWidth); s.uint(weave.tileHeight)
            for n in ("dWarpUmaxOverDWarp", "dWarpUmaxOverDWeft", "dWeftUmaxOverDWarp", "dWeftUmaxOverDWeft", "fineness", "period"):
                s.float(getattr(weave, n))
            for p in (weave.pattern if pattern is None else pattern):
                s.uint(p)
            s.b += struct.pack("<Q", len(weave.yarns) if yarn_count is None else yarn_count)
            for y in weave.yarns:
                s.int(int(y.type))
                for n in ("psi", "umax", "kappa", "width", "length", "centerU", "centerV"):
                    s.float(getattr(y, n))
                s.spectrum(y.kd); s.spectrum(y.ks)
            for n in ("repeatU", "repeatV", "kdMultiplier", "ksMultiplier"):
                s.float(getattr(weave, n))
        s.ref(key, "IrawanClothBRDF", body)
    return write
