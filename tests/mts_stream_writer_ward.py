"""Writers for the object streams of the Ward and Composite BSDFs of Mitsuba 0.2.1, next to tests/mts_stream_writer.py (whose
Stream, textures and writers of the other classes they use): each follows the serialize() of the class it is named after.
Test infrastructure; nothing here is used by the product."""
import mts_stream_writer as W


def ward(s, key, P, name="", tex_parent=False, share_textures=False):
    """Ward::serialize (src/bsdfs/ward.cpp:299-311) behind BSDF::serialize (src/librender/bsdf.cpp:50-53): model type (uint),
    the two textures, alphaX, alphaY, kd, ks, specular and diffuse sampling weight.  P: the block of include/mtsgpu.h"""
    tp = key if tex_parent else None
    def body(s):
        W.configurable(s); s.string(name)
        s.uint(int(P[0]))
        W.const_spectrum_texture(s, (key, "tex") if share_textures else (key, "diffuseReflectance"), P[7:10], tp)
        W.const_spectrum_texture(s, (key, "tex") if share_textures else (key, "specularReflectance"), P[10:13], tp)
        for k in range(1, 7):
            s.float(P[k])
    s.ref(key, "Ward", body)


def any_bsdf(s, key, btype, P, name=""):
    """one non-composite instance of table type `btype` (with the twosided flag: wrapped in a TwoSidedBRDF, twosided.cpp:52-56)"""
    two = bool(btype & 0x100)
    base = btype & 0xFF
    if base != 8:
        W.bsdf(s, key, base, P, twosided=two, name=name)
    elif two:
        def body(s):
            W.configurable(s); s.string(name)
            ward(s, (key, "nested"), P, name)
        s.ref(key, "TwoSidedBRDF", body)
    else:
        ward(s, key, P, name)


def size(s, v):
    """Stream::writeSize (include/mitsuba/core/stream.h:180): 64 bits"""
    s.b += int(v).to_bytes(8, "little")


def composite(s, key, weights, children, name="", twosided=False):
    """Composite::serialize (src/bsdfs/composite.cpp:81-89): the count, then weight and nested instance per child.
    children: (key, table type, block) -- a key seen before is written as a bare id, as InstanceManager does"""
    def body(s):
        W.configurable(s); s.string(name)
        size(s, len(children))
        for w, (ckey, ctype, cP) in zip(weights, children):
            s.float(w)
            if ckey is None:
                s.ref(None)
            elif ctype == 9:
                composite(s, ckey, *cP)
            else:
                any_bsdf(s, ckey, ctype, cP)
    if twosided:
        def outer(s):
            W.configurable(s); s.string(name)
            s.ref((key, "nested"), "Composite", body)
        s.ref(key, "TwoSidedBRDF", outer)
    else:
        s.ref(key, "Composite", body)
