"""Writer of BSDF object streams whose texture slots may hold a `VertexColors` texture, for the byte-level tests of
integration/streamparse.h (tests/test_stream_parsers_vcol.py).  Test infrastructure, next to tests/mts_stream_writer.py: every
function follows the serialize() of the class it is named after (paths relative to /root/reference).

VertexColors::serialize (src/textures/vertexcolors.cpp:37-39) calls Texture::serialize (src/librender/texture.cpp:39-41),
which calls ConfigurableObject::serialize (the parent reference) and writes nothing else."""
import mts_stream_writer as W

CLASS = {0: "Lambertian", 1: "Dielectric", 2: "RoughMetal", 3: "Microfacet", 5: "Phong", 6: "RoughGlass", 7: "DiffuseTransmitter", 8: "Ward"}


def vertex_colors(s, key, parent_key=None, cls="VertexColors"):
    s.ref(key, cls, lambda s: W.configurable(s, parent_key))


def bsdf(s, key, btype, P, mask=0, twosided=False, name="", tex_parent=False, share=False, alpha_colors=False, other_class=None):
    """BSDF::serialize (src/librender/bsdf.cpp:50-53) + the plugin's own fields, the texture of slot k a VertexColors when bit k
    of `mask` is set and a ConstantSpectrumTexture of the block's values otherwise.  share: both slots hold ONE VertexColors
    object (the second reference is its bare id); alpha_colors: roughglass' alpha is a VertexColors; other_class: the class
    name written for the coloured slots instead (a texture that is not on the path)."""
    if twosided:                                   # TwoSidedBRDF::serialize (src/bsdfs/twosided.cpp:52-56)
        def body(s):
            W.configurable(s); s.string(name)
            bsdf(s, (key, "nested"), btype, P, mask, False, name, tex_parent, share, alpha_colors, other_class)
        s.ref(key, "TwoSidedBRDF", body)
        return
    tp = key if tex_parent else None

    def tex(slot, rgb):
        if mask >> slot & 1:
            vertex_colors(s, (key, "vc") if share else (key, "vc", slot), tp, other_class or "VertexColors")
        else:
            W.const_spectrum_texture(s, (key, "const", slot), rgb, tp)

    def body(s):
        W.configurable(s); s.string(name)
        if btype == 0:                             # lambertian.cpp:137-141
            tex(0, P[0:3])
        elif btype == 1:                           # dielectric.cpp:88-95
            s.float(P[0]); s.float(P[1]); tex(0, P[2:5]); tex(1, P[5:8])
        elif btype == 2:                           # roughmetal.cpp:169-176
            tex(0, P[7:10]); s.float(P[0]); s.spectrum(P[1:4]); s.spectrum(P[4:7])
        elif btype in (3, 5):                      # microfacet.cpp:283-293, phong.cpp:246-256
            tex(0, P[5:8]); tex(1, P[8:11])
            for k in range(5): s.float(P[k])
        elif btype == 6:                           # roughglass.cpp:735-744
            s.int(int(P[0]))
            if alpha_colors: vertex_colors(s, (key, "alpha"), tp)
            else: W.const_float_texture(s, (key, "alpha"), P[1], tp)
            tex(0, P[4:7]); tex(1, P[7:10]); s.float(P[2]); s.float(P[3])
        elif btype == 7:                           # difftrans.cpp:142-146
            tex(0, P[0:3])
        elif btype == 8:                           # ward.cpp:299-311
            s.uint(int(P[0])); tex(0, P[7:10]); tex(1, P[10:13])
            for k in range(1, 7): s.float(P[k])
    s.ref(key, CLASS[btype], body)


def composite(s, key, weights, children, name=""):
    """Composite::serialize (src/bsdfs/composite.cpp:81-89): children = [(key, btype, P, mask)]"""
    def body(s):
        W.configurable(s); s.string(name)
        s.b += len(weights).to_bytes(8, "little")             # size_t (stream.h:180)
        for w, (k, t, P, mask) in zip(weights, children):
            s.float(w); bsdf(s, k, t, P, mask)
    s.ref(key, "Composite", body)
