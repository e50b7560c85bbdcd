"""The film configurations tests/test_film_truth.py (oracle, CPU) and tests/test_gpu_film_truth.py (device) share: one small
scene with misses (alpha 0) and a wide radiance range -- scenes.envlit() at maxDepth 3 -- and the filters, block sizes, crop
windows and samplers of the cases.  Seeds are chosen so that the oracle's own samples meet the cap on fragile taps."""
import numpy as np

MAX_DEPTH = 3
FILM, CROP = (64, 48), (5, 3, 42, 28)           # the crop cases: offset (5, 3) of a 64 x 48 film
MAX_FRAGILE = 1e-3                              # fragile taps / all taps

# name -> filter (kind, half size, p0, p1 | "table"), width, height, spp, sampler, block size, highQualityEdges, crop, integrator
CASES = {
    "box_independent": dict(filter=("box",), W=40, H=28, spp=4, sampler="independent"),
    "box_halton": dict(filter=("box",), W=40, H=28, spp=4, sampler="halton"),
    "box_wave": dict(filter=("box",), W=12, H=10, spp=300, sampler="independent"),
    "box_crop": dict(filter=("box",), W=42, H=28, spp=4, sampler="independent", crop=True),
    "gaussian_bs8": dict(filter=("gaussian",), W=42, H=28, spp=4, sampler="independent", bs=8),
    "mitchell_bs8": dict(filter=("mitchell",), W=42, H=28, spp=4, sampler="independent", bs=8),
    "catmullrom_bs8": dict(filter=("catmullrom",), W=42, H=28, spp=4, sampler="independent", bs=8),
    "wsinc_bs8": dict(filter=("wsinc",), W=42, H=28, spp=4, sampler="independent", bs=8),
    "gaussian_bs16": dict(filter=("gaussian",), W=42, H=28, spp=4, sampler="independent", bs=16),
    "gaussian_hq": dict(filter=("gaussian",), W=42, H=28, spp=4, sampler="independent", bs=8, hq=True),
    "gaussian_crop": dict(filter=("gaussian",), W=42, H=28, spp=4, sampler="independent", bs=8, crop=True),
    "gaussian_crop_hq": dict(filter=("gaussian",), W=42, H=28, spp=4, sampler="independent", bs=8, crop=True, hq=True),
    "asymmetric": dict(filter=("table",), W=42, H=28, spp=4, sampler="independent", bs=8),
    "direct_hq": dict(filter=("gaussian",), W=42, H=28, spp=4, sampler="independent", bs=8, hq=True, integrator="direct"),
    "thin_lens": dict(filter=("box",), W=40, H=28, spp=4, sampler="independent", scene="next_rows"),
}
SEED = 0x5EED


def case(name):
    c = dict(bs=32, hq=False, crop=False, integrator="path", scene="envlit")
    c.update(CASES[name]); c["name"] = name
    return c


def asymmetric_table():
    """size_x = 1.25, size_y = 2.5 and 225 distinct positive values, not symmetric in (ix, iy), with the zero 16th row and
    column of a TabulatedFilter; scaled so that a pixel collects a weight of the order of spp"""
    iy, ix = np.mgrid[0:16, 0:16]
    v = (1.0 + 0.37 * ix + 0.0113 * iy * iy + 0.0031 * ix * iy + 0.00071 * iy) / 60.0
    v[15, :] = 0; v[:, 15] = 0
    v = v.astype(np.float32)
    assert len(np.unique(v[:15, :15])) == 225 and not np.array_equal(v, v.T)
    return np.float32(1.25), np.float32(2.5), v


def scene_of(mts, c):
    return getattr(mts.scenes, c["scene"])()


def filter_table(mts, c):
    """(size_x, size_y, values [16][16] float32) of the case's filter, as the library tabulates it on the host"""
    f = c["filter"]
    if f[0] == "table":
        return asymmetric_table()
    kind = ("box", "gaussian", "mitchell", "catmullrom", "wsinc").index(f[0])
    args = [(-1.0 if v is None else float(v)) for v in (list(f[1:]) + [None] * 3)[:3]]
    size = np.zeros(2, dtype=np.float32); values = np.zeros(256, dtype=np.float32)
    assert mts.lib().mtsgpu_tabulate_filter(kind, args[0], args[1], args[2], mts.abi.ptr(size, mts.abi.f32p), mts.abi.ptr(values, mts.abi.f32p)) == 0
    return size[0], size[1], values.reshape(16, 16)


def geometry(rf, c, size_x, size_y, mutate=None):
    border = rf.border_of(size_x, size_y, mutate)
    if c["crop"]:
        return rf.Geometry((c["W"], c["H"]), CROP[:2], FILM, c["bs"], c["hq"], border)
    return rf.Geometry((c["W"], c["H"]), (0, 0), None, c["bs"], c["hq"], border)


def restate(rf, geom, table, rec, pix, mutate=None, valid=None):
    """the restatement over sample records [n][8] (Li rgb, alpha, raster x, y, ...) whose pixels are pix [n][2]"""
    rec = np.asarray(rec, dtype=np.float32)
    ok = rf.is_valid(rec[:, :3]) if valid is None else valid
    return rf.reconstruct(rec[:, 4:6], rec[:, :3], rec[:, 3], ok, geom.tile_of(pix), geom, table[0], table[1], table[2], mutate=mutate)


def worst(res, film, extra=0):
    """the worst error / B over all pixels and channels"""
    return float(res.ratio(film, extra).max())
