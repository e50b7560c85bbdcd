"""The spot luminaire with a projection texture, restated from the reference's lines (not from the kernels):

    SpotLuminaire::configure     spot.cpp:55-61            cosBeamWidth, cosCutoffAngle, uvFactor = tan(cutoffAngle), invTransitionWidth
    SpotLuminaire::falloffCurve  spot.cpp:87-108           result = intensity; localDir = worldToLuminaire(d); 0 if cosTheta <= cosCutoff;
                                                           uv = 0.5 + 0.5 * localDir.xy / (localDir.z * uvFactor); result *= texture(uv);
                                                           result if cosTheta >= cosBeamWidth; else result * ((cutoff - acos(cosTheta)) * invTW)
    SpotLuminaire::sample        spot.cpp:116-124          lumToP = p - position; invDist = 1 / |lumToP|; d = lumToP * invDist;
                                                           value = falloffCurve(d) * (invDist * invDist)
    Texture2D::getValue(its)     texture.cpp:73-82         no uv partials (spot.cpp:97): getValue(uv'), uv' = uv * scale + offset
    checkerboard / gridtexture   tests/ref64_tex.py        the decision `bright`
    ldrtexture, filterType none  tests/ref64_bmp.py        the decision `cell`
    ldrtexture, trilinear / ewa  ldrtexture.cpp:230-232    MIPMap::triangle(0, u, v)
    MIPMap::triangle             mipmap.cpp:233-241        x = x * w - 0.5; xPos = floorToInt(x); dx = x - xPos; four getTexel taps,
                                                           T00 (1-dx)(1-dy) + T01 (1-dx) dy + T10 dx (1-dy) + T11 dx dy
    MIPMap::getTexel             mipmap.cpp:203-225        the `x <= 0` column quirk and the wrap mode, per tap

`sample(spot, tex, p, dtype)` runs those lines in `dtype`: numpy.float32 is the mirror (the reference's Float expressions, one
rounding per operation, no contraction), numpy.float64 the restatement, which starts from the same binary32 inputs (the points, the
luminaire's block as the flattener leaves it, the texture) and derives uvFactor itself.  std::tan and std::acos of a Float are the
correctly rounded binary32 values of the binary64 functions unless `fn` supplies the library's (devmath.h's
specification, held to libm by tests/test_oracle_kats.py); the device test passes the library's, the CPU tests the default.

`restate` adds a first-order error bound per value (derivation at `_bound`) and marks a record FRAGILE where a discrete decision --
the two cone thresholds, every cast and floor, the checker parity, the grid's line test, the wrap branch of every tap -- comes out
differently in the two precisions, or would within the restatement's own uncertainty of uv': such a record sits on an edge closer
than binary32 resolves and is reported, not compared.

`mutation` swaps one line for a plausible mistake (MUTATIONS); tests/test_spot.py shows that each one is reported.  Test infrastructure."""
import numpy as np

import ref64_bmp as B
import ref64_tex as T

F = np.float32
U = 2.0 ** -24
CONSTANT, CHECKERBOARD, GRID, BITMAP = -1, 0, 1, 2
MUTATIONS = ("no_half_offset", "swap_xy", "uvfactor_beam", "texture_after_falloff", "no_bilinear_shift", "swap_dxdy", "col0_inside",
             "wrap_coordinate", "nearest_for_bilinear", "recip_division", "no_perspective_divide", "ramp_in_cosine")
# the mutations that change roundings only: they are seen by the mirror bit for bit, not by the bound
ROUNDING_MUTATIONS = ("texture_after_falloff", "recip_division")


class Spot:
    """a spot luminaire from its parameter block (include/mtsgpu.h: MTSGPU_LUM_SPOT) as the flattener leaves it"""

    def __init__(self, block):
        P = np.asarray(block, dtype=np.float32)
        self.block = P.copy()
        self.intensity, self.position = P[0:3].copy(), P[3:6].copy()
        self.cos_beam, self.cos_cutoff, self.cutoff, self.inv_tw, self.beam = P[6], P[7], P[8], P[9], P[19]
        self.w2l = P[10:19].reshape(3, 3).copy()


class SpotTex:
    """a projection texture: ref64_tex.Tex (checkerboard, grid) or ref64_bmp.Bmp (bitmap) with the filter flag"""

    def __init__(self, tex, bilinear=False):
        self.tex = tex
        self.kind = BITMAP if isinstance(tex, B.Bmp) else int(tex.kind)
        self.bilinear = bool(bilinear) and self.kind == BITMAP


def uv_factor(spot, dtype, fn=None, mutation=None):
    """configure(): m_uvFactor = std::tan(m_cutoffAngle)"""
    a = spot.beam if mutation == "uvfactor_beam" else spot.cutoff
    if dtype is np.float64:
        return np.tan(np.float64(a))
    return F(fn["tan"](a)) if fn else F(np.tan(np.float64(a)))


def _acos(c, dtype, fn):
    if dtype is np.float64:
        return np.arccos(np.clip(c, -1.0, 1.0))
    return np.asarray(fn["acos"](c), dtype=np.float32) if fn else np.arccos(np.clip(c.astype(np.float64), -1.0, 1.0)).astype(np.float32)


def _tap_cell(t, tx, ty, mutation):
    """MIPMap::getTexel(0, tx, ty): the flat index of the texel, B.BLACK or B.WHITE"""
    w, h = t.width, t.height
    outside = ((tx < 0) if mutation == "col0_inside" else (tx <= 0)) | (ty < 0) | (tx >= w) | (ty >= h)
    if t.wrap == B.REPEAT:
        qx, qy = np.mod(tx, w), np.mod(ty, h)          # the non-negative remainder (util.cpp:424-427)
    elif t.wrap == B.CLAMP:
        qx, qy = np.clip(tx, 0, w - 1), np.clip(ty, 0, h - 1)
    else:
        qx, qy = np.zeros_like(tx), np.zeros_like(ty)
    xi, yi = np.where(outside, qx, tx), np.where(outside, qy, ty)
    flat = xi + w * yi
    if t.wrap in (B.BLACK_MODE, B.WHITE_MODE):
        flat = np.where(outside, B.BLACK if t.wrap == B.BLACK_MODE else B.WHITE, flat)
    return flat


def triangle_cells(t, x, y, dtype, mutation=None):
    """MIPMap::triangle(0, x, y) up to its weights: (cells [4][n] in the order T00 T01 T10 T11, dx, dy)"""
    w, h = dtype(F(t.width)), dtype(F(t.height))
    half = dtype(0.0 if mutation == "no_bilinear_shift" else 0.5)
    x, y = x * w - half, y * h - half
    xp, yp = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    dx, dy = x - xp.astype(dtype), y - yp.astype(dtype)
    if mutation == "wrap_coordinate":
        # the wrap applied once, to the base texel; the other taps sit beside it, held inside the bitmap
        base = _tap_cell(t, xp, yp, None)
        const = base < 0
        bx, by = np.where(const, 0, base % t.width), np.where(const, 0, base // t.width)
        cells = []
        for ox, oy in ((0, 0), (0, 1), (1, 0), (1, 1)):
            c = np.minimum(bx + ox, t.width - 1) + t.width * np.minimum(by + oy, t.height - 1)
            cells.append(np.where(const, base, c))
        return np.stack(cells), dx, dy
    cells = np.stack([_tap_cell(t, xp + ox, yp + oy, mutation) for ox, oy in ((0, 0), (0, 1), (1, 0), (1, 1))])
    return cells, dx, dy


def triangle_value(t, cells, dx, dy, dtype, mutation=None):
    """the weighted sum of the four taps, per channel, left to right -> [n][3]"""
    if mutation == "swap_dxdy":
        dx, dy = dy, dx
    one = dtype(1)
    tx = [B.value(t, c).astype(dtype) for c in cells]
    wa, wb = [one - dx, one - dx, dx, dx], [one - dy, dy, one - dy, dy]
    acc = None
    for k in range(4):
        term = (tx[k] * wa[k][:, None]) * wb[k][:, None]
        acc = term if acc is None else acc + term
    return acc


def texture_value(st, uvx, uvy, dtype, mutation=None):
    """Texture2D::getValue(its) without partials -> (value [n][3] in dtype, decision: an integer array [k][n] that names every
    discrete outcome, transformed coordinates x, y)"""
    t = st.tex
    if st.kind == BITMAP:
        x, y = B.transform(t, uvx, uvy, dtype)
        if st.bilinear and mutation != "nearest_for_bilinear":
            cells, dx, dy = triangle_cells(t, x, y, dtype, mutation)
            return triangle_value(t, cells, dx, dy, dtype, mutation), cells, x, y
        cell = B.cell_at(t, x, y, dtype, "col0_inside" if mutation == "col0_inside" else None)
        return B.value(t, cell).astype(dtype), cell[None, :], x, y
    x, y = T.transform(t, uvx, uvy, dtype)
    br = T.bright(t, x, y, dtype)
    return T.value(t, br).astype(dtype), br.astype(np.int64)[None, :], x, y


class Sample:
    pass


def sample(spot, st, p, dtype, mutation=None, fn=None):
    """SpotLuminaire::sample(p) for points p [n][3] (binary32) in `dtype`; st = None: the constant texture.  Returns a Sample:
    d [n][3], uv [n][2] (0 outside the cone), value [n][3], inside / in_beam [n] (the two thresholds), decision [k][n], and the
    intermediate quantities the bound needs"""
    with np.errstate(invalid="ignore", divide="ignore"):      # (beam = cutoff: invTransitionWidth is infinite, and never used)
        return _sample(spot, st, p, dtype, mutation, fn)


def _sample(spot, st, p, dtype, mutation, fn):
    r = Sample()
    # (binary32 points; the restatement also takes binary64 ones: the exact hit points of the end-to-end tests)
    p = (np.asarray(p, dtype=np.float64) if dtype is np.float64 and np.asarray(p).dtype == np.float64 else np.asarray(p, dtype=np.float32).astype(dtype)).reshape(-1, 3)
    pos, W, I = spot.position.astype(dtype), spot.w2l.astype(dtype), spot.intensity.astype(dtype)
    one, half = dtype(1), dtype(0.5)
    l = p - pos
    length = np.sqrt((l[:, 0] * l[:, 0] + l[:, 1] * l[:, 1]) + l[:, 2] * l[:, 2])
    inv = one / length
    d = l * inv[:, None]
    loc = [(W[k, 0] * d[:, 0] + W[k, 1] * d[:, 1]) + W[k, 2] * d[:, 2] for k in range(3)]
    cos_theta = loc[2]
    r.d, r.inv, r.loc, r.cos_theta = d, inv, loc, cos_theta
    r.inside = ~(cos_theta <= dtype(spot.cos_cutoff))
    r.in_beam = cos_theta >= dtype(spot.cos_beam)
    n = p.shape[0]
    safe_z = np.where(r.inside, loc[2], one)          # (outside the cone nothing below is evaluated)
    result = np.broadcast_to(I, (n, 3)).astype(dtype)
    r.uv = np.zeros((n, 2), dtype=dtype)
    r.decision = np.zeros((1, n), dtype=np.int64)
    r.tex = np.ones((n, 3), dtype=dtype)
    r.x = r.y = np.zeros(n, dtype=dtype)
    if st is not None:
        f = uv_factor(spot, dtype, fn, mutation)
        lx, ly = (loc[1], loc[0]) if mutation == "swap_xy" else (loc[0], loc[1])
        den = f if mutation == "no_perspective_divide" else safe_z * f
        if mutation == "recip_division":
            rcp = one / den
            qx, qy = (half * lx) * rcp, (half * ly) * rcp
        else:
            qx, qy = (half * lx) / den, (half * ly) / den
        off = dtype(0.0 if mutation == "no_half_offset" else 0.5)
        uvx, uvy = off + qx, off + qy
        r.den, r.f = den, f
        r.uv = np.where(r.inside[:, None], np.stack([uvx, uvy], axis=1), dtype(0))
        tv, dec, r.x, r.y = texture_value(st, np.where(r.inside, uvx, dtype(0.5)), np.where(r.inside, uvy, dtype(0.5)), dtype, mutation)
        r.tex, r.decision = tv, np.where(r.inside[None, :], dec, 0)
    if mutation == "ramp_in_cosine":
        ramp = (cos_theta - dtype(spot.cos_cutoff)) / (dtype(spot.cos_beam) - dtype(spot.cos_cutoff))
    else:
        r.acos = _acos(np.where(r.inside, cos_theta, one), dtype, fn)
        ramp = (dtype(spot.cutoff) - r.acos) * dtype(spot.inv_tw)
    r.ramp = ramp
    if mutation == "texture_after_falloff":
        flat = result * r.tex
        ramped = (result * ramp[:, None]) * r.tex
    else:
        flat = result * r.tex
        ramped = flat * ramp[:, None]
    result = np.where(r.in_beam[:, None], flat, ramped)
    result = np.where(r.inside[:, None], result, dtype(0))
    r.value = result * (inv * inv)[:, None]
    return r


def mirror(spot, st, p, mutation=None, fn=None):
    return sample(spot, st, p, np.float32, mutation, fn)


class Restated:
    """value64 [n][3] and its bound [n][3], uv64 [n][2] and its bound [n], d64, the decisions, fragile [n]"""


def _bound(spot, st, r):
    """First-order bounds on what the binary32 evaluation may differ from the binary64 one by, u = 2^-24 per rounding:
      lumToP = p - position        exact inputs, one rounding per component:               rel u
      |lumToP|^2                   squares 2u + u, two sums of non-negative terms 2u:      rel 5u;  sqrt: 3.5u;  invDist: 4.5u
      d = lumToP * invDist         u + 4.5u + u:                                           abs 6.5u |d_i|
      localDir_k = W_k . d         products 7.5u, two sums 2u, of S_k = sum |W_kj d_j|:     abs e_k = 9.5u S_k
      den = localDir.z * uvFactor  uvFactor within 1 ulp of tan (2u), the product u:        rel e_z / z + 3u
      q = (0.5 lx) / den           abs e_x * 0.5 / |den| + |q| (rel den + u);  uv = 0.5 + q:  abs e_q + u |uv|
      uv' = uv * scale + offset    abs e_uv |scale| + u |uv scale| + u |uv'|
    checkerboard, grid, nearest texel: a decision and a stored value: no further error.  Bilinear:
      xs = uv' * w - 0.5           abs e_uv' w + u |uv' w| + u |xs|;   dx = xs - xPos: e_xs + u;   1 - dx: e_dx + u
      term = T a b                 abs T (e_a b + e_b a + 2u a b);  the sum of four: the terms' + 3u |sum|
      result = intensity * tex     abs I e_tex + u I tex
      acos(cosTheta)               abs e_z / sqrt(1 - c^2) (capped by 2 sqrt(e_z)) + 2u acos;  cutoff - acos: + u |.|
      ramp = (.) * invTW           invTW 2u, the product u: abs e_sub |invTW| + 3u |ramp|;  result * ramp: rel sum + u
      value = result * invDist^2   invDist^2: 10u; the product u
    The bound is doubled: first order only."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return _bound_of(spot, st, r)


def _bound_of(spot, st, r):
    n = r.d.shape[0]
    absd = np.abs(r.d)
    W = np.abs(spot.w2l.astype(np.float64))
    e_loc = [9.5 * U * (W[k, 0] * absd[:, 0] + W[k, 1] * absd[:, 1] + W[k, 2] * absd[:, 2]) for k in range(3)]
    e_z = e_loc[2]
    e_tex = np.zeros((n, 3))
    e_uvp = np.zeros((n, 2))
    e_uv = np.zeros(n)
    if st is not None:
        z = np.where(r.inside, r.loc[2], 1.0)
        rel_den = e_z / np.abs(z) + 3 * U
        q = r.uv - 0.5
        e_q = [e_loc[k] * 0.5 / np.abs(r.den) + np.abs(q[:, k]) * (rel_den + U) for k in range(2)]
        e_uvk = [e_q[k] + U * np.abs(r.uv[:, k]) for k in range(2)]
        e_uv = np.maximum(e_uvk[0], e_uvk[1])
        t = st.tex
        sc = [abs(float(t.uscale)), abs(float(t.vscale))]
        xy = [r.x, r.y]
        for k in range(2):
            e_uvp[:, k] = e_uvk[k] * sc[k] + U * np.abs(r.uv[:, k]) * sc[k] + U * np.abs(xy[k])
        if st.bilinear:
            size = [float(t.width), float(t.height)]
            e_w = []
            for k in range(2):
                xs = xy[k] * size[k] - 0.5
                e_xs = e_uvp[:, k] * size[k] + U * np.abs(xy[k] * size[k]) + U * np.abs(xs)
                e_w.append(e_xs + 2 * U)
            cells, dx, dy = triangle_cells(t, r.x, r.y, np.float64)
            a, b = [1 - dx, 1 - dx, dx, dx], [1 - dy, dy, 1 - dy, dy]
            for k in range(4):
                tv = B.value(t, cells[k]).astype(np.float64)
                e_tex += tv * (e_w[0] * np.abs(b[k]) + e_w[1] * np.abs(a[k]) + 2 * U * np.abs(a[k] * b[k]))[:, None]
            e_tex += 3 * U * np.abs(r.tex)
    I = np.abs(spot.intensity.astype(np.float64))[None, :]
    e_res = I * e_tex + U * I * np.abs(r.tex)
    res = I * np.abs(r.tex)
    c = np.clip(r.cos_theta, -1.0, 1.0)
    e_acos = np.minimum(e_z / np.sqrt(np.maximum(1 - c * c, 1e-300)), 2 * np.sqrt(e_z)) + 2 * U * np.abs(r.acos)
    sub = np.abs(float(spot.cutoff) - r.acos)
    e_ramp = (e_acos + U * sub) * abs(float(spot.inv_tw)) + 3 * U * np.abs(r.ramp)
    ramped = e_res * np.abs(r.ramp)[:, None] + res * e_ramp[:, None] + U * res * np.abs(r.ramp)[:, None]
    e = np.where(r.in_beam[:, None], e_res, ramped)
    inv2 = (r.inv * r.inv)[:, None]
    val = np.abs(r.value)
    e = e * inv2 + 11 * U * val
    e = np.where(r.inside[:, None], e, 0.0)
    return 2 * e, 2 * e_uv, 2 * e_uvp, 2 * e_z


def decide_near(spot, st, p64, reach):
    """the restatement at binary64 points p64 [n][3] and whether anything discrete -- the two thresholds, the texture's decision --
    changes on the corners of the box p64 +- reach: (Sample, unstable [n])"""
    base = sample(spot, st, p64, np.float64)
    unstable = np.zeros(len(p64), dtype=bool)
    for sx in (-1.0, 1.0):
        for sy in (-1.0, 1.0):
            for sz in (-1.0, 1.0):
                r = sample(spot, st, p64 + reach * np.array([sx, sy, sz]), np.float64)
                unstable |= (r.inside != base.inside) | (r.in_beam != base.in_beam) | (r.decision != base.decision).any(axis=0)
    return base, unstable


def restate(spot, st, p, mutation=None):
    """the binary64 restatement with its bound, and the records on which a decision is ambiguous"""
    r64 = sample(spot, st, p, np.float64, mutation)
    r32 = sample(spot, st, p, np.float32)
    plain = r64 if mutation is None else sample(spot, st, p, np.float64)
    out = Restated()
    out.value64, out.uv64, out.d64 = r64.value, r64.uv, r64.d
    out.bound, out.uv_bound, e_uvp, e_z = _bound(spot, st, plain)
    out.inside, out.in_beam, out.decision = plain.inside, plain.in_beam, plain.decision
    fragile = (r32.inside != plain.inside) | (r32.in_beam != plain.in_beam) | (r32.decision != plain.decision).any(axis=0)
    # ... or would differ within the restatement's own uncertainty of cosTheta and of uv'
    c = plain.cos_theta
    for thr in (float(spot.cos_cutoff), float(spot.cos_beam)):
        fragile |= np.abs(c - thr) <= e_z
    if st is not None:
        for sx in (-1.0, 1.0):
            for sy in (-1.0, 1.0):
                x, y = plain.x + sx * e_uvp[:, 0], plain.y + sy * e_uvp[:, 1]
                if st.kind == BITMAP and st.bilinear:
                    dec = triangle_cells(st.tex, x, y, np.float64)[0]
                elif st.kind == BITMAP:
                    dec = B.cell_at(st.tex, x, y, np.float64)[None, :]
                else:
                    dec = T.bright(st.tex, x, y, np.float64).astype(np.int64)[None, :]
                fragile |= plain.inside & (dec != plain.decision).any(axis=0)
    out.fragile = fragile
    return out
