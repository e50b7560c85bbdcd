"""The unfiltered bitmap texture (`ldrtexture`, filterType = "none"), restated from the reference's lines (not from the kernels):

    Texture2D::getValue(its)    texture.cpp:73-82         uv' = (uv.x * uscale, uv.y * vscale) + (uoffset, voffset)
    MIPMap::triangle, ENone     mipmap.cpp:228-231        xPos = floorToInt(x * width), yPos = floorToInt(y * height)
    MIPMap::getTexel            mipmap.cpp:203-225        if (x <= 0 || y < 0 || x >= w || y >= h): repeat -> modulo, clamp ->
                                                          clamp(., 0, size - 1), black -> 0, white -> 1;  pyramid[0][x + w * y]
    modulo / clamp              util.cpp:424-427, util.h:314-320
    LDRTexture::initializeFrom  ldrtexture.cpp:116-202    the 256-entry gamma table
    LDRTexture average/maximum  ldrtexture.cpp:206-207, mipmap.cpp:137-154

its.uv itself is tests/ref64_tex.py's.  `lookup` takes `dtype`: numpy.float32 is the mirror (the reference's Float expressions,
one rounding per operation, no contraction), numpy.float64 the restatement, which starts from the same binary32 inputs.  The
result is the discrete decision `cell`: the flat index y * w + x of the texel, BLACK or WHITE.  Everything after the two floors
is integer arithmetic, so the two precisions can only part at a floor: a query whose cells differ is FRAGILE -- it sits on a
texel edge closer than binary32 resolves -- and is reported, not compared.

`mutation` swaps one line for a plausible mistake (MUTATIONS); tests/test_bmp.py shows that each one is reported.  A mutated
index that leaves the bitmap is wrapped into it, so that the mutation has a value at all.  Test infrastructure."""
import numpy as np

F = np.float32
REPEAT, CLAMP, BLACK_MODE, WHITE_MODE = 0, 1, 2, 3      # MTSGPU_WRAP_*
WRAP_NAMES = ("repeat", "clamp", "black", "white")
BLACK, WHITE = -1, -2                                   # cells that are no texel
MUTATIONS = ("col0_inside", "trunc", "round", "swap_wh", "xy_storage", "clamp_w", "c_remainder", "flip_v")
U24 = 2.0 ** -24


class Bmp:
    """a bitmap texture: texels [height][width][3] float32, a wrap mode, Texture2D's transform"""

    def __init__(self, texels, wrap=REPEAT, uoffset=0.0, voffset=0.0, uscale=1.0, vscale=1.0):
        self.texels = np.ascontiguousarray(texels, dtype=np.float32)
        self.height, self.width = self.texels.shape[:2]
        self.wrap = int(wrap)
        self.uoffset, self.voffset, self.uscale, self.vscale = F(uoffset), F(voffset), F(uscale), F(vscale)


def transform(t, uvx, uvy, dtype):
    us, vs, uo, vo = dtype(t.uscale), dtype(t.vscale), dtype(t.uoffset), dtype(t.voffset)
    return uvx * us + uo, uvy * vs + vo


def _floor_to_int(x, mutation):
    f = np.trunc(x) if mutation == "trunc" else np.rint(x) if mutation == "round" else np.floor(x)
    return f.astype(np.int64)      # the values stay inside the int range: mtsgpu_set_uv_bitmap_textures checks it


def _modulo(a, b, mutation):
    if mutation == "c_remainder":
        return np.fmod(a, b)       # C's %: the sign of the dividend
    r = a - (np.trunc(a / b)).astype(np.int64) * b
    return np.where(r < 0, r + b, r)


def cell_at(t, x, y, dtype, mutation=None):
    """the decision at the transformed coordinates (x, y)"""
    w, h = t.width, t.height
    if mutation == "flip_v":
        y = dtype(1) - y
    sw, sh = (h, w) if mutation == "swap_wh" else (w, h)
    xp = _floor_to_int(x * dtype(F(sw)), mutation)
    yp = _floor_to_int(y * dtype(F(sh)), mutation)
    outside = ((xp < 0) if mutation == "col0_inside" else (xp <= 0)) | (yp < 0) | (xp >= sw) | (yp >= sh)
    if t.wrap == REPEAT:
        xq, yq = _modulo(xp, sw, mutation), _modulo(yp, sh, mutation)
    elif t.wrap == CLAMP:
        hi = 0 if mutation == "clamp_w" else 1
        xq, yq = np.clip(xp, 0, sw - hi), np.clip(yp, 0, sh - hi)
    else:
        xq, yq = np.zeros_like(xp), np.zeros_like(yp)
    xi, yi = np.where(outside, xq, xp), np.where(outside, yq, yp)
    flat = (xi * h + yi) if mutation == "xy_storage" else (xi + sw * yi)
    if mutation is not None:
        flat = np.mod(flat, w * h)
    if t.wrap in (BLACK_MODE, WHITE_MODE):
        flat = np.where(outside, BLACK if t.wrap == BLACK_MODE else WHITE, flat)
    return flat


def lookup(t, uvx, uvy, dtype, mutation=None):
    x, y = transform(t, np.asarray(uvx).astype(dtype), np.asarray(uvy).astype(dtype), dtype)
    return cell_at(t, x, y, dtype, mutation)


def value(t, cell):
    """the float32 colours of a decision array -> [n][3]"""
    cell = np.asarray(cell)
    table = np.concatenate([t.texels.reshape(-1, 3), np.ones((1, 3), np.float32), np.zeros((1, 3), np.float32)])      # [-2] white, [-1] black
    return table[cell].astype(np.float32)


def average(t):
    """m_average = triangle(levels - 1, 0, 0) with one level: the lookup at uv' = (0, 0)"""
    z = np.zeros(1)
    return value(t, cell_at(t, z, z, np.float64))[0]


def maximum(t):
    m = t.texels.reshape(-1, 3).max(axis=0)
    return np.maximum(m, F(1)) if t.wrap == WHITE_MODE else m


class Decision:
    """uv in both precisions, the cell in both, `fragile` = the two disagree, value32 = the mirror's colours.  With a mutation,
    cell64 is the mutated restatement's; `fragile` stays that of the unmutated one."""

    def __init__(self, t, uv32, uv64, mutation=None):
        self.uv32 = np.stack(uv32, axis=1).astype(np.float32)
        self.uv64 = np.stack(uv64, axis=1)
        self.cell32 = lookup(t, uv32[0], uv32[1], np.float32)
        self.cell64 = lookup(t, uv64[0], uv64[1], np.float64, mutation)
        # the binary64 lookup with both floors also taken in binary32: the two disagree on a texel edge
        x64, y64 = transform(t, np.asarray(uv64[0], dtype=np.float64), np.asarray(uv64[1], dtype=np.float64), np.float64)
        plain = cell_at(t, x64, y64, np.float64)
        self.fragile = (self.cell32 != plain) | (plain != cell_at(t, x64.astype(np.float32), y64.astype(np.float32), np.float32))
        self.value32 = value(t, self.cell32)
        self.value64 = value(t, self.cell64)


def decide_triangles(t, texcoords, tri, prim, u, v, mutation=None):
    import ref64_tex as RT
    return Decision(t, RT.triangle_uv(texcoords, tri, prim, u, v, np.float32), RT.triangle_uv(texcoords, tri, prim, u, v, np.float64), mutation)


def decide_sphere(t, center, radius, world_to_object, p, mutation=None):
    import ref64_tex as RT
    return Decision(t, RT.sphere_uv(center, radius, world_to_object, p, np.float32), RT.sphere_uv(center, radius, world_to_object, p, np.float64),
                    mutation)


# --- the gamma table (ldrtexture.cpp:116-133) ------------------------------------------------------------------------------
def gamma_table(gamma):
    """(table [256] binary64, bound [256]): the table of LDRTexture::initializeFrom evaluated in binary64 with the reference's
    binary32 constants, and a first-order bound on what the binary32 evaluation may differ from it by.  With u = 2^-24, one
    rounding to nearest moves a value by a relative u at the most:
      v = i / 255                             one rounding                                       u
      gamma != -1:  powf(v, gamma)            the error of v amplified by |gamma|, then powf:  (|gamma| + 2) u
      sRGB, v <= 0.04045:  v / 12.92          v's and the quotient's                             2 u
      sRGB otherwise:  a = v + 0.055 carries v's error (v < a) and its own rounding: 2 u;  b = a / 1.055 one more: 3 u;
                       powf(b, 2.4) amplifies by 2.4 and adds its own:                           (2.4 * 3 + 2) u
    powf is within 1 ulp (glibc's documented bound), and an ulp is at most 2^-23 = 2 u of the value.  Entry 0 is exactly 0."""
    i = np.arange(256, dtype=np.float64)
    v = i / 255.0
    g = float(F(gamma))
    if g == -1.0:
        lo = v / float(F(12.92))
        hi = ((v + float(F(0.055))) / float(F(1.0 + 0.055))) ** float(F(2.4))
        low = (i / 255.0).astype(np.float32) <= F(0.04045)
        # no entry sits where the two precisions could take different branches
        assert np.array_equal(low, v <= float(F(0.04045))) and np.abs(v - 0.04045).min() > 1e-3
        table = np.where(low, lo, hi)
        rel = np.where(low, 2.0, 2.4 * 3 + 2) * U24
    else:
        with np.errstate(divide="ignore"):
            table = v ** g
        rel = (abs(g) + 2) * U24 * np.ones(256)
    table = np.maximum(table, 0.0)      # clampNegative
    return table, np.abs(table) * rel


def ldr_indices(bpp, width, height, data):
    """per pixel the table entries of r, g, b (ldrtexture.cpp:135-202) -> [height][width][3] int"""
    d = np.asarray(data, dtype=np.uint8).reshape(-1)
    n = width * height
    if bpp in (24, 32):
        px = d[:n * (bpp // 8)].reshape(n, bpp // 8)[:, :3]
    elif bpp == 16:
        px = np.repeat(d[:2 * n].reshape(n, 2)[:, :1], 3, axis=1)
    elif bpp == 8:
        px = np.repeat(d[:n].reshape(n, 1), 3, axis=1)
    elif bpp == 1:
        pos = np.arange(n)
        bit = (d[pos // 8] >> (pos % 8)) & 1
        px = np.repeat(np.where(bit, 255, 0).reshape(n, 1), 3, axis=1)
    else:
        raise ValueError("%i bpp images are currently not supported!" % bpp)
    return px.astype(np.int64).reshape(height, width, 3)
