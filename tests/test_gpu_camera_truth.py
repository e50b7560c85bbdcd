"""k_generate on the device against the binary64 restatement of the camera (tests/ref64_camera.py), through the read-out of
the camera records (mtsgpu_camera_rays): the kernel's own launch, no copy of its arithmetic, no oracle between the rows and
the truth.  Every row goes through the check the oracle's rows go through in tests/test_camera_truth.py -- worst |error| /
bound <= 1 with the restatement's first-order bound, the geometric properties, the float32 mirror bit for bit -- and its
raster position must be its pixel plus the sampler's own draw, the lens sample drawn first (mtsgpu_sampler_values).  The
figures are printed and kept in LABNOTES.md (device: the oracle's, value for value, since both equal the mirror)."""
import ctypes as C

import numpy as np
import pytest

import camera_cases as cc
import ref64_camera as rc
import ref64_film as rf

pytestmark = pytest.mark.gpu
ESTATE, EINVAL = -5, -1
_TRUTH = {}


def _truth(c):
    if c["name"] not in _TRUTH:
        _TRUTH[c["name"]] = cc.truth(c)
    return _TRUTH[c["name"]]


def _tracer(mts, c, sampler="independent", spp=1, maxDepth=3):
    sd = mts.scenes.cornell_c1()
    scene = mts.Scene(sd)
    it = mts.MIPathTracer(maxDepth=maxDepth)
    it.preprocess(scene, cc.product_camera(mts, c), sampler=sampler, sampleCount=spp, seed=cc.SEED)
    it._scene_keep = scene
    _configure(mts, it, c, sampler, spp)
    return it


@pytest.fixture(scope="module")
def tracer(gpu_lib, mts):
    """one context for the explicit-mode tests: each sets its camera, sampler, filter and edges"""
    it = _tracer(mts, cc.cases("perspective")[0])
    yield it
    it.close()


def _configure(mts, it, c, sampler="independent", spp=1):
    cam = cc.product_camera(mts, c)
    L = mts.lib()
    it.camera = cam
    it._chk(L.mtsgpu_set_camera(it._ctx, C.byref(cam.c)), "set_camera")
    kind = {"independent": 0, "ldsampler": 1, "halton": 2, "hammersley": 3, "stratified": 4}[sampler]
    it._chk(L.mtsgpu_set_sampler(it._ctx, kind, spp, 3, cc.SEED), "set_sampler")
    it.set_rfilter("gaussian" if c["border"] else "box")
    it.set_film_edges(c["border"] > 0)
    return cam


def _draws(it, keys, js):
    """the first and the second next2D() of every (key, sample index), from the device's sampler"""
    return np.stack([it.sampler_values(int(k), int(j), 2, two_d=True) for k, j in zip(keys, js)]).astype(np.float32)


def _check_rows(orc, it, cam, c, rows, pix, js, label=None):
    """every row against the truth for the request (pixel of the crop window, sample index) it answers"""
    T = _truth(c)
    keys = cc.key_of(c, pix)
    assert np.array_equal(rows[:, 12].copy().view(np.uint32), keys), label
    assert np.array_equal(rows[:, 13].copy().view(np.uint32), np.asarray(js, dtype=np.uint32)), label
    raster, lens = cc.samples_of(c, pix, _draws(it, keys, js))
    mrows, branches = rc.mirror(cam.c, raster, lens, cc.sincos_of(orc))
    assert cc.same_bits(rows[:, :8], mrows), label                          # bit for bit against the float32 mirror
    w, differ = rc.check(T, rows, branches, raster, lens)                   # the raster positions bit for bit, the rays in bound
    val, bnd, _ = rc.generate(T, branches, raster, lens)
    p = rc.properties(T, rows, bnd, raster, lens)
    assert w <= 1.0 and p <= 1.0, (label, w, p)
    return w, p, differ


# --- explicit mode -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", cc.FAMILIES)
def test_explicit_rays(tracer, mts, orc, family):
    """every camera of camera_cases: the corners of its window (of its border with highQualityEdges: negative pixels) and
    arbitrary pixels"""
    worst, worst_prop, differ, total = 0.0, 0.0, 0, 0
    for c in cc.cases(family):
        cam = _configure(mts, tracer, c)
        pix = cc.pixels_of(c, 24)
        js = np.zeros(len(pix), dtype=np.int64)
        rows = tracer.camera_rays(np.concatenate([pix, js[:, None]], axis=1))
        w, p, k = _check_rows(orc, tracer, cam, c, rows, pix, js, c["name"])
        worst, worst_prop, differ, total = max(worst, w), max(worst_prop, p), differ + k, total + len(pix)
        if c["border"]:
            assert rows[:, 8].min() < cc.offset(c)[0] and pix.min() == -c["border"]
    print("device rays, %s: worst error / bound %.3f, properties %.3f, %d of %d samples with a differing branch, 0 excluded"
          % (family, worst, worst_prop, differ, total))


_COUNTERS = {"independent": lambda k: (0, 0), "ldsampler": lambda k: (0, k), "halton": lambda k: (2 * k, 0),
             "hammersley": lambda k: (2 * k, 0), "stratified": lambda k: (0, k)}


@pytest.mark.parametrize("sampler", cc.SAMPLERS)
def test_samplers_and_counters(tracer, mts, orc, sampler):
    """all five samplers at 1 and 16 samples per pixel, with and without a lens sample.  After generation the independent
    sampler has no counter, ldsampler and stratified have drawn k of their 2D tables (k = 2 with a lens sample, the lens
    first; depth 3), Halton and Hammersley are 2 k dimensions into their sequence (integrator.cpp:156-161)"""
    for c in (cc.cases("thinlens")[0], cc.cases("perspective")[1]):
        for spp in (1, 16):
            cam = _configure(mts, tracer, c, sampler, spp)
            pix = np.repeat(cc.pixels_of(c, 8 if spp == 16 else 24), spp, axis=0)
            js = np.tile(np.arange(spp), len(pix) // spp)
            rows = tracer.camera_rays(np.concatenate([pix, js[:, None]], axis=1))
            _check_rows(orc, tracer, cam, c, rows, pix, js, (sampler, spp, c["name"]))
            d = rows[:, 10:12].copy().view(np.uint32)
            assert (d == np.array(_COUNTERS[sampler](2 if cc.thin(c) else 1), dtype=np.uint32)).all(), (sampler, spp, c["name"])


@pytest.mark.parametrize("n", cc.RECORD_COUNTS)
def test_record_counts(tracer, mts, orc, n):
    """a lone lane, a ragged wave, a ragged block of the write-out through LDS: EVERY record compared, so a record stored to a
    neighbour's slot -- or one of its eight 16-byte pieces -- fails"""
    c = cc.cases("thinlens")[0]
    spp = 4
    cam = _configure(mts, tracer, c, "independent", spp)
    w, h = cc.size(c)
    i = np.arange(n)
    assert np.gcd(11, w * h) == 1 and n <= w * h
    slot = (i * 11) % (w * h)                                            # distinct pixels in no particular order
    pix = np.stack([slot % w, slot // w], axis=1)
    js = i % spp
    rows = tracer.camera_rays(np.concatenate([pix, js[:, None]], axis=1))
    assert rows.shape == (n, 14)
    _check_rows(orc, tracer, cam, c, rows, pix, js, n)
    assert len(np.unique(rows[:, :8].copy().view(np.uint32), axis=0)) == n    # no two records alike: a misplaced one cannot hide


def test_refusals(gpu_lib, mts):
    c = cc.cases("border")[0]
    it = _tracer(mts, c, spp=4)
    L, a = mts.lib(), mts.abi
    out = np.zeros((4, 14), dtype=np.float32)
    po = a.ptr(out, a.f32p)

    def explicit(rows, first=0, o=po):
        ps = np.ascontiguousarray(rows, dtype=np.int32)
        return L.mtsgpu_camera_rays(it._ctx, a.ptr(ps, a.i32p), first, len(ps), o)

    W, H = cc.size(c)
    b = c["border"]
    assert L.mtsgpu_camera_rays(it._ctx, None, 0, 4, po) == ESTATE                      # nothing rendered
    assert explicit([(-b, -b, 0), (W + b - 1, H + b - 1, 3)]) == 0
    for bad in ((-b - 1, 0, 0), (0, -b - 1, 0), (W + b, 0, 0), (0, H + b, 0), (0, 0, 4), (0, 0, -1)):
        assert explicit([(0, 0, 0), bad]) == EINVAL, bad
    assert explicit([(0, 0, 0)], first=1) == EINVAL and explicit([(0, 0, 0)], o=None) == EINVAL
    it.set_film_edges(False)                                                            # no border: its pixels are out of range
    assert explicit([(-1, 0, 0)]) == EINVAL and explicit([(W, 0, 0)]) == EINVAL and explicit([(W - 1, H - 1, 0)]) == 0
    it.set_options(max_paths=1 << 20)
    assert it.render()
    n = it.stats()["camera_samples"]
    assert n == W * H * 4
    assert L.mtsgpu_camera_rays(it._ctx, None, n - 3, 4, po) == EINVAL                  # past the end: the pass stays valid
    assert L.mtsgpu_camera_rays(it._ctx, None, 0xFFFFFFFF, 4, po) == EINVAL
    assert L.mtsgpu_camera_rays(it._ctx, None, 0, 4, None) == EINVAL
    assert L.mtsgpu_camera_rays(it._ctx, None, 0, (1 << 24) + 1, po) == EINVAL
    assert L.mtsgpu_camera_rays(it._ctx, None, n - 4, 4, po) == 0
    assert L.mtsgpu_camera_rays(it._ctx, None, n - 4, 4, po) == ESTATE                  # the records no longer hold that pass
    assert L.mtsgpu_pass_samples(it._ctx, 0, 4, a.ptr(np.zeros((4, 8), dtype=np.float32), a.f32p)) == ESTATE
    assert it.render()
    assert explicit([(0, 0, 0)]) == 0
    assert L.mtsgpu_camera_rays(it._ctx, None, 0, 4, po) == ESTATE                      # the explicit mode took the records too
    it.close()


# --- last-pass mode ------------------------------------------------------------------------------------------------------------------
def _last_pass_pixels(c, bs, part, n_parts, slots_per_pass):
    """pixels of the crop window [n][2] of the pass mtsgpu_render renders last: the part's tiles in row-major tile order
    (imageproc.cpp:43-78), whole tiles to a pass while they fit, row-major inside a tile"""
    (w, h), b = cc.size(c), c["border"]
    W, H = w + 2 * b, h + 2 * b
    tiles = [(tx, ty) for ty in range(-(-H // bs)) for tx in range(-(-W // bs)) if int(rf.morton(tx, ty)) % n_parts == part]
    passes, acc = [[]], 0
    for tx, ty in tiles:
        tw, th = min(bs, W - tx * bs), min(bs, H - ty * bs)
        if acc and acc + tw * th > slots_per_pass:
            passes.append([]); acc = 0
        passes[-1] += [(tx * bs + x - b, ty * bs + y - b) for y in range(th) for x in range(tw)]
        acc += tw * th
    return np.array(passes[-1]), len(passes)


@pytest.mark.parametrize("tiles_per_pass", [3, 5])
def test_last_pass(gpu_lib, mts, orc, tiles_per_pass):
    """42 x 28 at (5, 3) of 64 x 48, the gaussian border of 2, tiles of 8, part 1 of 3, a thin lens, ldsampler tables, passes of
    at most 3 (5) tiles: the last pass is shorter than the others and ends in tiles narrower than 8.  Its records, generated
    once more, come in tile order with the keys and raster positions mtsgpu_pass_samples reported, and their rays are the
    truth's"""
    c = cc.cases("border")[2]
    assert c["crop"] == (5, 3, 42, 28) and c["border"] == 2 and cc.thin(c)
    spp, bs = 4, 8
    it = _tracer(mts, c, "ldsampler", spp)
    cam = it.camera
    it.set_tiles(bs, 1, 3)
    it.set_options(max_paths=tiles_per_pass * bs * bs * spp)
    assert it.render()
    pix, n_passes = _last_pass_pixels(c, bs, 1, 3, tiles_per_pass * bs * bs)
    n = len(pix) * spp
    assert n_passes >= 2 and len(pix) % (bs * bs) != 0                     # several passes, and a ragged last one
    L, a = mts.lib(), mts.abi
    probe = np.zeros((1, 8), dtype=np.float32)
    assert L.mtsgpu_pass_samples(it._ctx, n, 1, a.ptr(probe, a.f32p)) == EINVAL       # the pass has exactly n records
    rec = it.pass_samples(0, n)
    rows = it.camera_rays(None, 0, n)
    pix, js = np.repeat(pix, spp, axis=0), np.tile(np.arange(spp), len(pix))
    assert cc.same_bits(rows[:, 12], rec[:, 7]) and cc.same_bits(rows[:, 8:10], rec[:, 4:6])
    assert (rows[:, 10:12].copy().view(np.uint32) == np.array([0, 2], dtype=np.uint32)).all()
    w, p, _ = _check_rows(orc, it, cam, c, rows, pix, js, "last pass")    # keys and sample indices in tile order, rays in bound
    print("device rays, last pass of %d tiles: worst error / bound %.3f, properties %.3f over %d records" % (tiles_per_pass, w, p, n))
    # a window of the pass: records first .. first + n
    it.clear_film()
    assert it.render()
    part = it.camera_rays(None, 37, 65)
    assert cc.same_bits(part, rows[37:102])
    it.close()


# --- frames that must not change -------------------------------------------------------------------------------------------------
def test_frames_unchanged_by_the_hook(gpu_lib, mts):
    c = cc.cases("thinlens")[0]
    it = _tracer(mts, c, "ldsampler", 4)
    it.set_options(max_paths=300 * 4)
    assert it.render()
    film = it.film().copy()
    assert film[..., :3].max() > 0
    pix = cc.pixels_of(c, 50)
    it.camera_rays(np.concatenate([pix, np.ones((len(pix), 1), dtype=np.int64)], axis=1))
    it.clear_film()
    assert it.render()
    assert np.array_equal(it.film().view(np.uint32), film.view(np.uint32))
    it.camera_rays(None, 0, 16)                                              # the last-pass mode likewise
    it.clear_film()
    assert it.render()
    assert np.array_equal(it.film().view(np.uint32), film.view(np.uint32))
    it.close()
