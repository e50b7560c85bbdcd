"""Writer of `Mask` object streams, for the byte-level tests of integration/streamparse.h (tests/test_stream_parsers_mask.py).
Test infrastructure, next to tests/mts_stream_writer_bmp.py, whose texture writer serves every opacity texture.

Mask::serialize (src/bsdfs/mask.cpp:47-52): BSDF::serialize (the parent reference and the name), the opacity texture instance,
then the nested BSDF instance."""
import mts_stream_writer as W
import mts_stream_writer_bmp as WB
import mts_stream_writer_vcol as WV
import mts_stream_writer_ward as WW

VERTEX_COLORS = "vertexcolors"


def mask(s, key, opacity, nested, name="", tex_parent=False):
    """opacity: an RGB triple (a ConstantSpectrumTexture), a texture object (a Checkerboard, GridTexture or WB.Ldr), VERTEX_COLORS,
    or None (a NULL reference); nested: a callable (s) that writes the nested BSDF instance, or None for a NULL reference"""
    tp = key if tex_parent else None

    def body(s):
        W.configurable(s); s.string(name)
        if opacity is None:
            s.ref(None)
        elif opacity is VERTEX_COLORS:
            WV.vertex_colors(s, (key, "opacity"), tp)
        elif hasattr(opacity, "kind"):
            WB.uv_texture(s, (key, "opacity"), opacity, tp)
        else:
            W.const_spectrum_texture(s, (key, "opacity"), opacity, tp)
        if nested is None:
            s.ref(None)
        else:
            nested(s)
    s.ref(key, "Mask", body)


def twosided(s, key, nested, name=""):
    """TwoSidedBRDF::serialize (src/bsdfs/twosided.cpp:52-56) around whatever `nested` writes"""
    def body(s):
        W.configurable(s); s.string(name)
        nested(s)
    s.ref(key, "TwoSidedBRDF", body)


def any_bsdf(key, btype, P):
    """a nested-instance writer for table type `btype` (with the twosided flag: wrapped in a TwoSidedBRDF)"""
    return lambda s: WW.any_bsdf(s, key, btype, P)


def composite(key, weights, children):
    """a nested-instance writer for a Composite (src/bsdfs/composite.cpp:81-89) whose children are nested-instance writers"""
    def write(s):
        def body(s):
            W.configurable(s); s.string("")
            WW.size(s, len(children))
            for w, child in zip(weights, children):
                s.float(w); child(s)
        s.ref(key, "Composite", body)
    return write
