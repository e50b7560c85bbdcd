"""SpotLuminaire::serialize (src/luminaires/spot.cpp:63-70) with any texture instance behind Luminaire::serialize, written the way
tests/mts_stream_writer.py writes the constant one: for tests/test_stream_parsers_spot.py.  The texture is a child added through
addChild (spot.cpp:163-169), so its parent is the luminaire, whose id the stream already knows.  Test infrastructure."""
import mts_stream_writer as W
import mts_stream_writer_bmp as WB


class Proc:
    """what a Checkerboard (kind 0) or a GridTexture (kind 1) serializes"""

    def __init__(self, kind, uoffset=0.0, voffset=0.0, uscale=1.0, vscale=1.0, bright=(0.4, 0.4, 0.4), dark=(0.2, 0.2, 0.2), line_width=0.01):
        self.kind, self.uoffset, self.voffset, self.uscale, self.vscale = kind, uoffset, voffset, uscale, vscale
        self.bright, self.dark, self.line_width = bright, dark, line_width


def texture(s, key, t, parent_key):
    """the texture instance: a Proc, a WB.Ldr, ("constant", rgb) or ("other", class name)"""
    if isinstance(t, tuple) and t[0] == "constant":
        return W.const_spectrum_texture(s, key, t[1], parent_key)
    if isinstance(t, tuple):
        def body(s):
            W.configurable(s, parent_key)
        return s.ref(key, t[1], body)
    if t.kind == 2:
        return WB.uv_texture(s, key, t, parent_key)

    def body(s):
        W.configurable(s, parent_key)
        s.float(t.uoffset); s.float(t.voffset); s.float(t.uscale); s.float(t.vscale)      # Texture2D::serialize (texture.cpp:67-71)
        s.spectrum(t.bright); s.spectrum(t.dark)                                            # checkerboard.cpp:42-46
        if t.kind == 1:
            s.float(t.line_width)                                                           # gridtexture.cpp:44-49
    s.ref(key, "GridTexture" if t.kind == 1 else "Checkerboard", body)


def spot(s, key, w2l, l2w, intensity, beam_width, cutoff_angle, tex):
    def body(s):
        W.luminaire_base(s, w2l, l2w, ltype=2)
        texture(s, (key, "texture"), tex, key)
        s.spectrum(intensity); s.float(beam_width); s.float(cutoff_angle)
    s.ref(key, "SpotLuminaire", body)
