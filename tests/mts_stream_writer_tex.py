"""Writer of BSDF object streams whose texture slots may hold a `Checkerboard` or `GridTexture`, for the byte-level tests of
integration/streamparse.h (tests/test_stream_parsers_tex.py).  Test infrastructure, next to tests/mts_stream_writer_vcol.py:
every function follows the serialize() of the class it is named after (paths relative to the reference's tree).

Checkerboard::serialize (src/textures/checkerboard.cpp:42-46) and GridTexture::serialize (src/textures/gridtexture.cpp:44-49)
call Texture2D::serialize (src/librender/texture.cpp:67-71): Texture::serialize (the parent reference), m_uvOffset (Point2),
m_uvScale (Vector2); then brightColor, darkColor and, the grid only, lineWidth."""
import mts_stream_writer as W
import mts_stream_writer_vcol as WV

CLASS_OF_KIND = {0: "Checkerboard", 1: "GridTexture"}


def uv_texture(s, key, t, parent_key=None):
    """t: an object with kind, uoffset, voffset, uscale, vscale, bright, dark, line_width (scenes.Checkerboard / GridTexture)"""
    def body(s):
        W.configurable(s, parent_key)
        s.float(t.uoffset); s.float(t.voffset); s.float(t.uscale); s.float(t.vscale)
        s.spectrum(t.bright); s.spectrum(t.dark)
        if t.kind == 1:
            s.float(t.line_width)
    s.ref(key, CLASS_OF_KIND[t.kind], body)


def bsdf(s, key, btype, P, slot_tex=(None, None), colour_mask=0, twosided=False, name="", tex_parent=False, share=False, alpha_tex=None):
    """BSDF::serialize + the plugin's own fields; slot k holds slot_tex[k] (a texture object), a VertexColors when bit k of
    colour_mask is set, and a ConstantSpectrumTexture of the block's values otherwise.  share: both slots hold ONE texture
    object (the second reference is its bare id); alpha_tex: roughglass' alpha is that uv texture."""
    if twosided:                                   # TwoSidedBRDF::serialize (src/bsdfs/twosided.cpp:52-56)
        def body(s):
            W.configurable(s); s.string(name)
            bsdf(s, (key, "nested"), btype, P, slot_tex, colour_mask, False, name, tex_parent, share, alpha_tex)
        s.ref(key, "TwoSidedBRDF", body)
        return
    tp = key if tex_parent else None

    def tex(slot, rgb):
        if slot_tex[slot] is not None:
            uv_texture(s, (key, "uv") if share else (key, "uv", slot), slot_tex[slot], tp)
        elif colour_mask >> slot & 1:
            WV.vertex_colors(s, (key, "vc", slot), tp)
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
            if alpha_tex is not None: uv_texture(s, (key, "alpha"), alpha_tex, tp)
            else: W.const_float_texture(s, (key, "alpha"), P[1], tp)
            tex(0, P[4:7]); tex(1, P[7:10]); s.float(P[2]); s.float(P[3])
        elif btype == 7:                           # difftrans.cpp:142-146
            tex(0, P[0:3])
        elif btype == 8:                           # ward.cpp:299-311
            s.uint(int(P[0])); tex(0, P[7:10]); tex(1, P[10:13])
            for k in range(1, 7): s.float(P[k])
    s.ref(key, WV.CLASS[btype], body)


def composite(s, key, weights, children, name=""):
    """Composite::serialize (src/bsdfs/composite.cpp:81-89): children = [(key, btype, P, slot_tex)]"""
    def body(s):
        W.configurable(s); s.string(name)
        s.b += len(weights).to_bytes(8, "little")             # size_t (stream.h:180)
        for w, (k, t, P, slot_tex) in zip(weights, children):
            s.float(w); bsdf(s, k, t, P, slot_tex)
    s.ref(key, "Composite", body)
