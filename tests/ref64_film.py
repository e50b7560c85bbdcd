"""A binary64 restatement of the film stage: the five reconstruction-filter plugins behind TabulatedFilter, and
ImageBlock::putSample per bordered block followed by Film::putImageBlock.  Written from the reference's sources --
src/rfilters/{box,gaussian,mitchell,catmullrom,wsinc}.cpp, src/libcore/util.cpp:664-674 (lanczosSinc),
src/librender/rfilter.cpp:40-69, include/mitsuba/render/rfilter.h:65-102, include/mitsuba/render/imageblock.h:80-138,
src/librender/renderproc.cpp:143-153, src/librender/imageproc.cpp:28-52, src/films/mfilm.cpp:118-143 -- not from csrc/ or
oracle/.  Test infrastructure.

Filter tables (tabulate).  Every quantity is a pair (value, err) of ref64_sky.E: the value in binary64, err a first-order
bound, in units of 2^-23, on the absolute error of a binary32 evaluation in the reference's operation order (a rounded
operation adds half a unit of its result, sums and products carry their operands' errors on by the derivatives).  A libm
call (exp, sin) is taken to be within one ulp of the true value, not correctly rounded, and adds a whole unit.  The
sequential sum over the 256 entries adds half a unit of every partial sum.  Where the Mitchell polynomial's branch (|x| < 1,
< 2) is within reach of the argument's own error, the bound also covers the other branch.  The bound of an entry is what the
test allows; there is no factor on top.

Reconstruction (reconstruct).  Order-free: per film pixel and channel (r, g, b, alpha, weight) the sum T of weight * value
over all taps in binary64, S = sum |weight * value|, and the number n of taps with a non-zero weight.  The weights are the
binary32 table entries the kernels read, so the table's own error is no part of this comparison.

Discrete decisions.  xStart / xEnd / yStart / yEnd and the two table indices are evaluated twice: as the reference's Float
expressions in numpy float32 -- sample.x - 0.5f, then - (offset.x - border), then -/+ filterSize, ceil / floor; x - sample.x,
abs, times factor (= FILTER_RESOLUTION / size, one division), truncation: one operation and one rounding per step, so binary32
leaves no freedom -- and in binary64 from the same binary32 inputs.  Where both give the same tap (in range or not, same table
cell) the tap is firm.  Where they differ the tap is fragile: the pixel's value may be either, so the tap contributes the
interval [min, max] of its two outcomes (lo, hi below) and is counted; tests cap the count at 1 in 1000 taps.

Tolerance (derived, not fitted).  A binary32 implementation forms each term with one rounded product and adds the n terms of
a pixel in some order: sequentially inside a block (n - 1 additions), then Film::putImageBlock adds at most 4 blocks that
overlap a pixel (the block and the borders of three neighbours: 2 * border <= block size).  A term therefore passes through
at most 1 + (n - 1) + 4 roundings, each of relative size at most u = 2^-24; with two more for slack,
    k = n + 6,   gamma = k u / (1 - k u),   |film - T| <= gamma * S        (Higham, Accuracy and Stability, section 4.2),
whatever the order.  A pixel passes if it lies in [lo - B, hi + B], B = gamma * S.  Films the test itself adds in binary32
(tile parts, group members) pass `extra` = the number of those additions, which joins k.  Channels whose terms are all
exact (weight 1, alpha 0 / 1) get the same bound; it is merely not needed there.

Mutations.  `mutate` alters the restatement in one place; tests show that each altered restatement disagrees with the films
beyond B, which is what shows that B discriminates.  Two of them need a remark.  The border ceil(size - 0.5) is by
construction the smallest that holds every tap of a tile's own samples (a sample at s < offset + width reaches at most
pixel floor(s - 0.5 + size) <= offset + width + border - 1), so the clamp to the bordered block (imageblock.h:98-99) never
binds and a LARGER border, ceil(size), leaves every film value as it is: what it changes is the rectangle rendered with
highQualityEdges (Geometry.size), and that is where "border_ceil" is caught.  For the same reason "a sample splatting outside
its own block" cannot be stated as a wider clamp; "foreign_samples" states the misreading that has an effect: a bordered
block receiving the samples of neighbouring tiles that reach it, which counts the overlaps twice."""
import numpy as np

from ref64_sky import E, PI32

U = 2.0 ** -24
FILTER_RESOLUTION = 15            # rfilter.h:65
REACH = 4.0
KINDS = ("box", "gaussian", "mitchell", "catmullrom", "wsinc")
_F = np.float32


# --- the filter plugins -------------------------------------------------------------------------------------------------
def _lib(v, e):
    return E(v, e + np.abs(v))                    # a libm result: within one ulp


def _exp(a):
    v = np.exp(a.v); return _lib(v, v * a.e)


def _sin(a):
    return _lib(np.sin(a.v), np.abs(np.cos(a.v)) * a.e)


def _abs(a):
    return E(np.abs(a.v), a.e)


def _max0(a):
    return E(np.maximum(a.v, 0.0), a.e)           # |max(0, a) - max(0, b)| <= |a - b|


def _select(x, thr, below, above):
    """below where x < thr else above; where x is within reach of thr the bound covers both"""
    near = np.abs(x.v - thr) <= REACH * x.e * 2.0 ** -23
    v = np.where(x.v < thr, below.v, above.v)
    e = np.where(x.v < thr, below.e, above.e)
    return E(v, np.where(near, np.maximum(below.e, above.e) + np.abs(below.v - above.v) * 2.0 ** 23, e))


def _mitchell(x, B, C):
    """mitchellNetravali (mitchell.cpp:62-75, catmullrom.cpp:58-71)"""
    x = _abs(x)
    x2 = x * x; x3 = x2 * x
    sixth = E(1.0) / 6.0                                                         # 1.0f/6.0f
    inner = sixth * (((12 - 9 * B - 6 * C) * x3 + (-18 + 12 * B + 6 * C) * x2) + (6 - 2 * B))
    outer = sixth * ((((-B - 6 * C) * x3 + (6 * B + 30 * C) * x2) + (-12 * B - 48 * C) * x) + (8 * B + 24 * C))
    return _select(x, 1.0, inner, _select(x, 2.0, outer, E(np.zeros_like(x.v))))


def _lanczos(t, tau):
    """lanczosSinc (util.cpp:664-674); Epsilon = 1e-4f (constants.h)"""
    t = _abs(t)
    reach = REACH * t.e * 2.0 ** -23
    if (np.abs(t.v - 1e-4) <= reach).any() or (np.abs(t.v - 1.0) <= reach).any():
        raise ValueError("lanczosSinc argument within reach of a threshold: not restated")
    tp = t * PI32
    a = tp * tau
    val = (_sin(a) / a) * (_sin(tp) / tp)
    v = np.where(t.v < 1e-4, 1.0, np.where(t.v > 1.0, 0.0, val.v))
    return E(v, np.where((t.v < 1e-4) | (t.v > 1.0), 0.0, val.e))


def _f32(v):
    return float(_F(v))


def tabulate(kind, half_size=None, p0=None, p1=None, mutate=None):
    """TabulatedFilter::TabulatedFilter (rfilter.cpp:40-69) of plugin `kind` with its constructor's defaults (None) or the given
    binary32 parameters: gaussian p0 = stddev; mitchell p0 = B, p1 = C; wsinc p0 = cycles.  Returns (size_x, size_y, values
    [16][16] float64, bound [16][16]: the first-order absolute error bound of a binary32 evaluation).  mutate == "radial":
    the filter function times 1 + 0.05 r, r the distance from the centre, before normalisation."""
    R = FILTER_RESOLUTION
    if kind == "box":
        size = 0.5                                                               # box.cpp:30
    elif kind == "wsinc":
        size = _f32(3.0 if half_size is None else half_size)                     # wsinc.cpp:32
    else:
        size = _f32(2.0 if half_size is None else half_size)                     # gaussian.cpp:33, mitchell.cpp:34, catmullrom.cpp:33
    sz = E(size)
    pos = E(np.arange(R) + 0.5) / float(R) * sz                                  # (x + 0.5f) / FILTER_RESOLUTION * m_size.x
    if kind == "box":
        f = E(np.ones(R))                                                        # box.cpp:42-44
    elif kind == "gaussian":
        stddev = E(_f32(0.5 if p0 is None else p0))                              # gaussian.cpp:35
        alpha = 1 / (2 * stddev * stddev)                                        # :38
        const = _exp(-alpha * sz * sz)                                           # :42
        f = _max0(_exp(-alpha * pos * pos) - const)                              # :64-65
    elif kind in ("mitchell", "catmullrom"):
        third = _F(1.0) / _F(3.0)                                                # 1.0f / 3.0f (mitchell.cpp:37,39)
        B = E(0.0 if kind == "catmullrom" else _f32(third if p0 is None else p0))
        C = E(0.5 if kind == "catmullrom" else _f32(third if p1 is None else p1))      # catmullrom.cpp:35
        f = _mitchell(2.0 * pos / sz, B, C)                                      # mitchell.cpp:58-59
    elif kind == "wsinc":
        f = _lanczos(pos / sz, E(_f32(3.0 if p0 is None else p0)))               # wsinc.cpp:34,52-53
    else:
        raise ValueError(kind)
    # evaluate(x, y) = f(x) * f(y), one rounded product
    v = np.abs(f.v[None, :]) * 0 + f.v[None, :] * f.v[:, None]
    e = np.abs(f.v[None, :]) * f.e[:, None] + np.abs(f.v[:, None]) * f.e[None, :] + 0.5 * np.abs(v)
    if kind == "box":
        e = np.zeros_like(v)                                                     # return 1.0f
    if mutate == "radial":
        r = np.hypot(pos.v[None, :], pos.v[:, None])
        v = v * (1 + 0.05 * r); e = e * (1 + 0.05 * r)
    elif mutate is not None:
        raise ValueError(mutate)
    full = np.zeros((R + 1, R + 1)); full[:R, :R] = v                            # the zero 16th row and column
    efull = np.zeros((R + 1, R + 1)); efull[:R, :R] = e
    # sum += m_values[y][x], row by row, in binary32
    partial = np.cumsum(full.ravel())
    total = E(partial[-1], efull.sum() + 0.5 * np.abs(partial).sum())
    total = total * (4 * sz * sz / float(R * R))                                 # rfilter.cpp:62-63
    out = E(full, efull) / total                                                 # :64-68
    bound = np.where(full == 0, 0.0, out.e * 2.0 ** -23)                         # 0 / sum is exact
    return size, size, out.v, bound


# --- the blocks -----------------------------------------------------------------------------------------------------------
def border_of(size_x, size_y, mutate=None):
    """renderproc.cpp:143-144, in Float"""
    m = _F(max(_F(size_x), _F(size_y)))
    return int(np.ceil(m)) if mutate == "border_ceil" else int(np.ceil(_F(m - _F(0.5))))


class Geometry:
    """the film (crop window inside a full film), the block size and what renderproc.cpp:146-153 makes of them"""

    def __init__(self, crop_size, crop_offset=(0, 0), film_size=None, block_size=32, hq_edges=False, border=0):
        self.crop_size = tuple(int(v) for v in crop_size)
        self.crop_offset = tuple(int(v) for v in crop_offset)
        self.film_size = self.crop_size if film_size is None else tuple(int(v) for v in film_size)
        self.block_size, self.hq_edges, self.border = int(block_size), bool(hq_edges), int(border)
        grow = self.border if self.hq_edges else 0
        self.offset = (self.crop_offset[0] - grow, self.crop_offset[1] - grow)          # the rendered rectangle
        self.size = (self.crop_size[0] + 2 * grow, self.crop_size[1] + 2 * grow)
        bs = self.block_size
        self.n_blocks = (-(-self.size[0] // bs), -(-self.size[1] // bs))                # imageproc.cpp:32-34

    def rendered_pixels(self):
        """raster pixels (x, y) of the rendered rectangle, [n][2]"""
        ys, xs = np.mgrid[self.offset[1]:self.offset[1] + self.size[1], self.offset[0]:self.offset[0] + self.size[0]]
        return np.stack([xs.ravel(), ys.ravel()], axis=1)

    def tile_of(self, pix):
        """tile indices (tx, ty) of raster pixels [n][2]"""
        pix = np.asarray(pix, dtype=np.int64)
        return np.stack([(pix[:, 0] - self.offset[0]) // self.block_size, (pix[:, 1] - self.offset[1]) // self.block_size], axis=1)

    def tile_rect(self, tile):
        """rect.setOffset / setSize of imageproc.cpp:47-51 for tiles [n][2]: offsets [n][2], sizes [n][2]"""
        tile = np.asarray(tile, dtype=np.int64)
        pos = tile * self.block_size
        off = pos + np.array(self.offset)
        size = np.minimum(np.array(self.size) - pos, self.block_size)
        return off, size

    def key_to_pixel(self, key):
        """the library's pixel key (include/mtsgpu.h, mtsgpu_pass_samples) -> raster pixel"""
        grow = self.border if self.hq_edges else 0
        kw = self.film_size[0] + 2 * grow
        key = np.asarray(key, dtype=np.int64)
        return np.stack([key % kw - grow, key // kw - grow], axis=1)


def morton(tx, ty):
    """bits of tx and ty interleaved, tx lowest: the part a tile belongs to is morton % n_parts (include/mtsgpu.h)"""
    tx = np.asarray(tx, dtype=np.int64); ty = np.asarray(ty, dtype=np.int64)
    out = np.zeros_like(tx)
    for b in range(16):
        out |= ((tx >> b) & 1) << (2 * b) | ((ty >> b) & 1) << (2 * b + 1)
    return out


def _axis(s, off, full, size, border, mutate):
    """one axis of putSample (imageblock.h:91-114) for samples s (float32), their blocks' offsets and full sizes: candidate
    block-local pixels pos [n][m], and for both evaluations whether the pixel is in [start, end] and its table index"""
    half = 0.0 if mutate == "no_half" else 0.5
    res = 16.0 if mutate == "factor16" else float(FILTER_RESOLUTION)
    o = off - border
    s32 = ((s - _F(half)).astype(_F) - o.astype(_F)).astype(_F)
    s64 = s.astype(np.float64) - half - o
    z = _F(size)
    st32 = np.ceil((s32 - z).astype(_F)).astype(np.int64); en32 = np.floor((s32 + z).astype(_F)).astype(np.int64)
    st64 = np.ceil(s64 - float(z)).astype(np.int64); en64 = np.floor(s64 + float(z)).astype(np.int64)
    st32 = np.maximum(0, st32); st64 = np.maximum(0, st64)                      # imageblock.h:98-99
    en32 = np.minimum(en32, full - 1); en64 = np.minimum(en64, full - 1)
    K = int(np.ceil(float(z))) + 2
    pos = np.floor(s64).astype(np.int64)[:, None] + np.arange(-K, K + 1)[None, :]
    in32 = (pos >= st32[:, None]) & (pos <= en32[:, None])
    in64 = (pos >= st64[:, None]) & (pos <= en64[:, None])
    fac32 = _F(_F(res) / z); fac64 = res / float(z)                              # rfilter.cpp:43-45
    t32 = (fac32 * np.abs((pos.astype(_F) - s32[:, None]).astype(_F))).astype(_F)
    t64 = fac64 * np.abs(pos - s64[:, None])
    if mutate == "round_index":
        i32 = np.rint(t32).astype(np.int64); i64 = np.rint(t64).astype(np.int64)
    else:
        i32 = t32.astype(np.int64); i64 = t64.astype(np.int64)                   # (int) trafoX
    return pos, in32, np.minimum(i32, FILTER_RESOLUTION), in64, np.minimum(i64, FILTER_RESOLUTION)


class Result:
    def __init__(self, H, W):
        self.T = np.zeros((H, W, 5)); self.lo = np.zeros((H, W, 5)); self.hi = np.zeros((H, W, 5))
        self.S = np.zeros((H, W, 5)); self.n = np.zeros((H, W), dtype=np.int64)
        self.taps = 0; self.fragile = 0

    def bound(self, extra=0):
        k = (self.n + 6 + extra)[..., None] * U
        return k / (1 - k) * self.S

    def ratio(self, film, extra=0):
        """per pixel and channel: distance of the film value from [lo, hi], over B (0 inside; inf outside where B = 0)"""
        f = np.asarray(film, dtype=np.float64)
        err = np.maximum(np.maximum(self.lo - f, f - self.hi), 0.0)
        B = self.bound(extra)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(err == 0, 0.0, np.where(B > 0, err / np.where(B > 0, B, 1), np.inf))

    def __add__(self, o):
        """the restatement of the sum of two films (disjoint sample sets)"""
        r = Result(*self.n.shape)
        for a in ("T", "lo", "hi", "S", "n", "taps", "fragile"):
            setattr(r, a, getattr(self, a) + getattr(o, a))
        return r


def reconstruct(xy, L, alpha, valid, tile, geom, size_x, size_y, values, mutate=None, chunk=4096):
    """xy [n][2] float32 raster positions, L [n][3] float32, alpha [n], valid [n] (Spectrum::isValid, spectrum.h:285-290),
    tile [n][2]: the tile of the sample's pixel (Geometry.tile_of); values [16][16] float32: the table; -> Result"""
    if mutate == "foreign_samples":
        # a bordered block also receives the samples of its eight neighbours that reach it (instead of its own tile's only)
        tile = np.asarray(tile, dtype=np.int64)
        res = reconstruct(xy, L, alpha, valid, tile, geom, size_x, size_y, values)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                t2 = tile + np.array([dx, dy])
                ok = (t2[:, 0] >= 0) & (t2[:, 0] < geom.n_blocks[0]) & (t2[:, 1] >= 0) & (t2[:, 1] < geom.n_blocks[1])
                if (dx or dy) and ok.any():
                    res = res + reconstruct(np.asarray(xy)[ok], np.asarray(L)[ok], np.asarray(alpha)[ok], np.asarray(valid)[ok], t2[ok],
                                            geom, size_x, size_y, values)
        return res
    xy = np.ascontiguousarray(xy, dtype=_F); L = np.asarray(L, dtype=_F).astype(np.float64)
    alpha = np.asarray(alpha, dtype=_F).astype(np.float64)
    tab = np.asarray(values, dtype=_F).astype(np.float64).reshape(16, 16)
    if mutate == "transposed":
        tab = tab.T
    border = geom.border
    W, H = geom.crop_size
    res = Result(H, W)
    keep = np.nonzero(np.asarray(valid, dtype=bool))[0]                          # imageblock.h:85-88
    off, bsize = geom.tile_rect(np.asarray(tile)[keep])
    full = bsize + 2 * border                                                    # fullSize
    one = np.ones(len(keep))
    if mutate == "weight_needs_alpha":
        one = (alpha[keep] != 0).astype(np.float64)
    val = np.concatenate([L[keep], alpha[keep, None], one[:, None]], axis=1)     # pixels, alpha, weights (:122-124)
    flat = {a: [np.zeros(W * H) for _ in range(5)] for a in ("T", "lo", "hi", "S")}
    nflat = np.zeros(W * H, dtype=np.int64)
    for c0 in range(0, len(keep), chunk):
        sl = slice(c0, c0 + chunk); k = keep[sl]
        px, x32, ix32, x64, ix64 = _axis(xy[k, 0], off[sl, 0], full[sl, 0], size_x, border, mutate)
        py, y32, iy32, y64, iy64 = _axis(xy[k, 1], off[sl, 1], full[sl, 1], size_y, border, mutate)
        in32 = y32[:, :, None] & x32[:, None, :]; in64 = y64[:, :, None] & x64[:, None, :]
        c32 = np.where(in32, iy32[:, :, None] * 16 + ix32[:, None, :], -1)       # lookup(idxX, idxY) = m_values[y][x]
        c64 = np.where(in64, iy64[:, :, None] * 16 + ix64[:, None, :], -1)
        w32 = np.where(in32, tab.ravel()[np.maximum(c32, 0)], 0.0)
        w64 = np.where(in64, tab.ravel()[np.maximum(c64, 0)], 0.0)
        # Film::putImageBlock (mfilm.cpp:118-143): block-local pixel -> film pixel, kept inside the crop window
        X = px + (off[sl, 0] - border - geom.crop_offset[0])[:, None]
        Y = py + (off[sl, 1] - border - geom.crop_offset[1])[:, None]
        inside = ((Y >= 0) & (Y < H))[:, :, None] & ((X >= 0) & (X < W))[:, None, :] & (in32 | in64)
        firm = c32 == c64
        res.taps += int(inside.sum()); res.fragile += int((inside & ~firm).sum())
        idx = (Y[:, :, None] * W + X[:, None, :])[inside]
        a32 = w32[inside]; a64 = w64[inside]; fm = firm[inside]
        si = np.broadcast_to(np.arange(len(k))[:, None, None], inside.shape)[inside]
        nflat += np.bincount(idx, weights=((a32 != 0) | (a64 != 0)).astype(np.float64), minlength=W * H).astype(np.int64)
        for c in range(5):
            v = val[sl][si, c]
            t32 = a32 * v; t64 = a64 * v
            flat["T"][c] += np.bincount(idx, weights=np.where(fm, t32, 0.0), minlength=W * H)
            flat["lo"][c] += np.bincount(idx, weights=np.where(fm, t32, np.minimum(t32, t64)), minlength=W * H)
            flat["hi"][c] += np.bincount(idx, weights=np.where(fm, t32, np.maximum(t32, t64)), minlength=W * H)
            flat["S"][c] += np.bincount(idx, weights=np.maximum(np.abs(t32), np.abs(t64)), minlength=W * H)
    for a in ("T", "lo", "hi", "S"):
        getattr(res, a)[...] = np.stack(flat[a], axis=1).reshape(H, W, 5)
    res.n[...] = nflat.reshape(H, W)
    return res


def is_valid(L):
    """Spectrum::isValid (spectrum.h:285-290): no channel NaN or negative"""
    L = np.asarray(L)
    with np.errstate(invalid="ignore"):
        return ~(np.isnan(L) | (L < 0)).any(axis=1)
