"""Writer of BSDF object streams whose texture slots may hold an `LDRTexture`, for the byte-level tests of
integration/streamparse.h (tests/test_stream_parsers_bmp.py).  Test infrastructure, next to tests/mts_stream_writer_tex.py, whose
BSDF and composite writers it reuses with its own texture writer in place.

LDRTexture::serialize (src/textures/ldrtexture.cpp:210-228): Texture2D::serialize (src/librender/texture.cpp:67-71: the parent
reference, m_uvOffset, m_uvScale), the file name (string), m_gamma (Float), m_format (int), m_filterType (int), m_wrapMode
(uint), m_maxAnisotropy (Float), the size of the encoded file (uint) and its bytes."""
import mts_stream_writer as W
import mts_stream_writer_tex as WT

EWA, TRILINEAR, NONE = 0, 1, 2                       # MIPMap::EFilterType (mipmap.h:39-46)
REPEAT, BLACK, WHITE, CLAMP = 0, 1, 2, 3             # MIPMap::EWrapMode (mipmap.h:32-37)
PNG, JPEG = 1, 3                                     # two of Bitmap::EFileFormat; the parser passes the number on


class Ldr:
    """what an LDRTexture instance serializes"""
    kind = 2

    def __init__(self, payload, filename="textures/wood.png", gamma=-1.0, fmt=PNG, filter_type=NONE, wrap=REPEAT, max_anisotropy=8.0,
                 uoffset=0.0, voffset=0.0, uscale=1.0, vscale=1.0, declared_size=None):
        self.payload, self.filename, self.gamma, self.fmt, self.filter_type, self.wrap = bytes(payload), filename, gamma, fmt, filter_type, wrap
        self.max_anisotropy, self.uoffset, self.voffset, self.uscale, self.vscale = max_anisotropy, uoffset, voffset, uscale, vscale
        self.declared_size = len(self.payload) if declared_size is None else declared_size


def uv_texture(s, key, t, parent_key=None):
    """WT.uv_texture for every kind: an Ldr writes itself, the procedural textures go to the writer they had"""
    if t.kind != 2:
        return _tex_uv_texture(s, key, t, parent_key)

    def body(s):
        W.configurable(s, parent_key)
        s.float(t.uoffset); s.float(t.voffset); s.float(t.uscale); s.float(t.vscale)
        s.string(t.filename); s.float(t.gamma); s.int(t.fmt); s.int(t.filter_type); s.uint(t.wrap); s.float(t.max_anisotropy)
        s.uint(t.declared_size)
        t.offset = len(s.b)                          # where the encoded file starts in the stream
        s.b += t.payload
    s.ref(key, "LDRTexture", body)


_tex_uv_texture = WT.uv_texture


def _with_our_texture_writer(fn, *a, **k):
    WT.uv_texture = uv_texture
    try:
        return fn(*a, **k)
    finally:
        WT.uv_texture = _tex_uv_texture


def bsdf(s, *a, **k):
    """WT.bsdf, whose slots may hold an Ldr"""
    return _with_our_texture_writer(WT.bsdf, s, *a, **k)


def composite(s, *a, **k):
    return _with_our_texture_writer(WT.composite, s, *a, **k)
