"""Texture coordinates and the two procedural uv textures, restated from the reference's lines (not from shade.hip):

    its.uv on a triangle mesh   skdtree.h:364,408-415     b = ((1 - u) - v, u, v);  uv = (t0 * b.x + t1 * b.y) + t2 * b.z
    its.uv on a sphere          sphere.cpp:136-145        local = worldToObject(p - center);  theta = acos(clamp(local.z / r));
                                                          phi = atan2(local.y, local.x) (+ 2 pi if negative);
                                                          uv = (phi * (0.5f * INV_PI), theta * INV_PI)
    Texture2D::getValue(its)    texture.cpp:73-82         uv' = (uv.x * uscale, uv.y * vscale) + (uoffset, voffset)
    Checkerboard::getValue      checkerboard.cpp:48-56    x = 2 * modulo((int) (uv'.x * 2), 2) - 1, y alike; bright iff x * y == 1
    GridTexture::getValue       gridtexture.cpp:51-64     x = uv'.x - (int) uv'.x; if (x > .5) x -= 1; y alike;
                                                          dark iff |x| < lineWidth || |y| < lineWidth

Every function takes `dtype`: numpy.float32 gives the mirror (the reference's Float expressions, one rounding per operation,
no contraction), numpy.float64 the restatement, which starts from the same binary32 inputs.  A texture's value is one of two
colours, so the restatement's result is the discrete decision `bright`; `decide` takes it in both precisions, and a query on
which they disagree is FRAGILE: it sits on a cell boundary closer than binary32 resolves, is reported, and is not compared.

`mutation` swaps one line for a plausible mistake (MUTATIONS); tests/test_tex.py shows that each one is reported.  Test
infrastructure, not product code."""
import numpy as np

F = np.float32
CHECKERBOARD, GRID = 0, 1
MUTATIONS = ("floor", "offset_first", "invert", "ge_half", "le_width", "swap_uv", "b_order")
M_PI32, INV_PI32 = F(3.14159265358979323846), F(0.31830988618379067154)      # constants.h:46-47, single precision


class Tex:
    """the eight parameters of a texture, from a scenes.Checkerboard / GridTexture or from keywords"""

    def __init__(self, kind, uoffset=0.0, voffset=0.0, uscale=1.0, vscale=1.0, bright=0.4, dark=0.2, line_width=0.01):
        self.kind = int(kind)
        self.uoffset, self.voffset, self.uscale, self.vscale, self.line_width = F(uoffset), F(voffset), F(uscale), F(vscale), F(line_width)
        self.bright = np.broadcast_to(np.asarray(bright, dtype=np.float32), (3,)).copy()
        self.dark = np.broadcast_to(np.asarray(dark, dtype=np.float32), (3,)).copy()

    @classmethod
    def of(cls, t):
        return cls(t.kind, t.uoffset, t.voffset, t.uscale, t.vscale, t.bright, t.dark, t.line_width)


def triangle_uv(texcoords, tri, prim, u, v, dtype, mutation=None):
    """its.uv of records (prim, u, v): texcoords [n_verts][2] float32, tri [n_tris][3]"""
    T = np.asarray(texcoords, dtype=np.float32).astype(dtype)
    idx = np.asarray(tri)[np.asarray(prim)].astype(np.int64)
    u, v = np.asarray(u, dtype=np.float32).astype(dtype), np.asarray(v, dtype=np.float32).astype(dtype)
    one = dtype(1)
    bx, by, bz = (one - u) - v, u, v
    if mutation == "b_order":
        bx, by, bz = by, bz, bx
    t0, t1, t2 = T[idx[:, 0]], T[idx[:, 1]], T[idx[:, 2]]
    uv = (t0 * bx[:, None] + t1 * by[:, None]) + t2 * bz[:, None]
    return uv[:, 0], uv[:, 1]


def sphere_uv(center, radius, world_to_object, p, dtype):
    """its.uv of world-space hit points p [n][3] (binary32) on a sphere; world_to_object: the 3x3 linear part, row major"""
    c = np.asarray(center, dtype=np.float32).astype(dtype)
    W = np.asarray(world_to_object, dtype=np.float32).astype(dtype).reshape(3, 3)
    r = dtype(F(radius))
    pc = np.asarray(p, dtype=np.float32).astype(dtype) - c
    local = [(W[k, 0] * pc[:, 0] + W[k, 1] * pc[:, 1]) + W[k, 2] * pc[:, 2] for k in range(3)]
    cos_theta = np.minimum(np.maximum(local[2] / r, dtype(-1)), dtype(1))
    # std::acos / std::atan2 of a Float: the correctly rounded binary32 value of the binary64 function
    theta = np.arccos(cos_theta.astype(np.float64)).astype(dtype)
    phi = np.arctan2(local[1].astype(np.float64), local[0].astype(np.float64)).astype(dtype)
    two_pi = dtype(F(2) * M_PI32)
    phi = np.where(phi < 0, phi + two_pi, phi)
    return phi * dtype(F(0.5) * INV_PI32), theta * dtype(INV_PI32)


def transform(tex, uvx, uvy, dtype, mutation=None):
    us, vs, uo, vo = dtype(tex.uscale), dtype(tex.vscale), dtype(tex.uoffset), dtype(tex.voffset)
    if mutation == "swap_uv":
        uvx, uvy = uvy, uvx
    if mutation == "offset_first":
        return (uvx + uo) * us, (uvy + vo) * vs
    return uvx * us + uo, uvy * vs + vo


def _to_int(x, mutation):
    """(int) x: truncation towards zero (the values stay far inside the int range: mtsgpu_set_uv_textures checks it)"""
    return (np.floor(x) if mutation == "floor" else np.trunc(x)).astype(np.int64)


def grid_fraction(x, y, dtype, mutation=None):
    """GridTexture's wrapped fractions: x - (int) x, less 1 when above .5 (gridtexture.cpp:52-58)"""
    fx, fy = x - _to_int(x, mutation).astype(dtype), y - _to_int(y, mutation).astype(dtype)
    half = dtype(0.5)
    if mutation == "ge_half":
        return np.where(fx >= half, fx - dtype(1), fx), np.where(fy >= half, fy - dtype(1), fy)
    return np.where(fx > half, fx - dtype(1), fx), np.where(fy > half, fy - dtype(1), fy)


def bright(tex, x, y, dtype, mutation=None):
    """the decision at the transformed coordinates (x, y): True = brightColor"""
    if tex.kind == CHECKERBOARD:
        two = dtype(2)
        cx = 2 * np.mod(_to_int(x * two, mutation), 2) - 1          # numpy's mod is the non-negative remainder
        cy = 2 * np.mod(_to_int(y * two, mutation), 2) - 1
        out = cx * cy == 1
        return ~out if mutation == "invert" else out
    fx, fy = grid_fraction(x, y, dtype, mutation)
    lw = dtype(tex.line_width)
    if mutation == "le_width":
        dark = (np.abs(fx) <= lw) | (np.abs(fy) <= lw)
    else:
        dark = (np.abs(fx) < lw) | (np.abs(fy) < lw)
    return dark if mutation == "invert" else ~dark


def at_uv(tex, uvx, uvy, dtype, mutation=None):
    x, y = transform(tex, np.asarray(uvx).astype(dtype), np.asarray(uvy).astype(dtype), dtype, mutation)
    return bright(tex, x, y, dtype, mutation)


def value(tex, is_bright):
    """the float32 colours of a decision array -> [n][3]"""
    return np.where(np.asarray(is_bright)[:, None], tex.bright[None, :], tex.dark[None, :]).astype(np.float32)


class Decision:
    """uv (binary32 mirror and binary64), the decision in both precisions, and `fragile` = the two disagree.  With a
    mutation, bright64 (and uv64, frac64) are the mutated restatement's; `fragile` stays that of the unmutated one.
    frac32 / frac64: the grid's wrapped fractions [n][2], None for the checkerboard"""

    def __init__(self, tex, uv32, uv64, uv64_mutated=None, mutation=None):
        m = uv64 if uv64_mutated is None else uv64_mutated
        self.uv32 = np.stack(uv32, axis=1).astype(np.float32)
        self.uv64 = np.stack(m, axis=1)
        self.bright32 = at_uv(tex, uv32[0], uv32[1], np.float32)
        self.bright64 = at_uv(tex, m[0], m[1], np.float64, mutation)
        self.fragile = self.bright32 != at_uv(tex, uv64[0], uv64[1], np.float64)
        self.value32 = value(tex, self.bright32)
        self.frac32 = self.frac64 = None
        if tex.kind == GRID:
            self.frac32 = np.stack(grid_fraction(*transform(tex, uv32[0], uv32[1], np.float32), np.float32), axis=1)
            self.frac64 = np.stack(grid_fraction(*transform(tex, m[0], m[1], np.float64, mutation), np.float64, mutation), axis=1)
            # a fraction that wraps in one precision only is as undecided as a colour
            plain = np.stack(grid_fraction(*transform(tex, uv64[0], uv64[1], np.float64), np.float64), axis=1)
            self.fragile = self.fragile | (np.abs(self.frac32 - plain) > 1e-5).any(axis=1)


def decide_triangles(tex, texcoords, tri, prim, u, v, mutation=None):
    return Decision(tex, triangle_uv(texcoords, tri, prim, u, v, np.float32), triangle_uv(texcoords, tri, prim, u, v, np.float64),
                    triangle_uv(texcoords, tri, prim, u, v, np.float64, mutation), mutation)


def decide_sphere(tex, center, radius, world_to_object, p, mutation=None):
    return Decision(tex, sphere_uv(center, radius, world_to_object, p, np.float32),
                    sphere_uv(center, radius, world_to_object, p, np.float64), None, mutation)
