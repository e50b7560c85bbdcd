"""The film kernels on the device -- k_accumulate, k_accumulate_wave, k_splat_blocks + k_add_blocks, the tile and pass logic
of mtsgpu_render -- against the binary64 restatement of ImageBlock::putSample (tests/ref64_film.py), fed with the very
records the kernels read (mtsgpu_pass_samples).  Every case renders its frame in one pass, reads the records, and requires
every film value inside [lo - B, hi + B], B = gamma_(n+6) * S.  The worst error / B of each case is printed and kept in
LABNOTES.md; the bound does not follow from those figures (observed: 0.04 for the wave form to 0.25 for one tile part of three;
no fragile tap in any case).

Not covered: Spectrum::isValid failing on the device in a way the film could show.  The Halton case does produce NaN
radiance (sample 0 of every pixel draws zeros everywhere), and those records are flagged invalid here, but they sit on the
pixel corner where every weight is 0; tests/test_film_truth.py covers the rule on a synthetic list."""
import ctypes as C

import numpy as np
import pytest

import film_cases as fc
import ref64_film as rf

pytestmark = pytest.mark.gpu
ONE_PASS = 1 << 20


def _set_filter(mts, ctx, c):
    table = fc.filter_table(mts, c)
    if c["filter"][0] != "box":
        v = np.ascontiguousarray(table[2], dtype=np.float32)
        assert mts.lib().mtsgpu_set_rfilter(ctx, float(table[0]), float(table[1]), mts.abi.ptr(v, mts.abi.f32p)) == 0
    return table


def _camera(mts, sd, c):
    if c["crop"]:
        return mts.PerspectiveCamera.cropped(sd, fc.FILM[0], fc.FILM[1], fc.CROP)
    return mts.PerspectiveCamera.for_description(sd, c["W"], c["H"])


def _tracer(mts, name, **over):
    c = dict(fc.case(name), **over)
    sd = fc.scene_of(mts, c)
    scene = mts.Scene(sd)
    it = mts.MIDirectIntegrator(2, 2) if c["integrator"] == "direct" else mts.MIPathTracer(maxDepth=fc.MAX_DEPTH)
    it.preprocess(scene, _camera(mts, sd, c), sampler=c["sampler"], sampleCount=c["spp"], seed=fc.SEED)
    table = _set_filter(mts, it._ctx, c)
    it.set_tiles(c["bs"], 0, 1); it.set_film_edges(c["hq"]); it.set_options(max_paths=ONE_PASS)
    it._scene_keep = scene
    return c, table, it, fc.geometry(rf, c, table[0], table[1])


def _expected_pixels(geom, part=0, n_parts=1):
    pix = geom.rendered_pixels()
    t = geom.tile_of(pix)
    return pix[rf.morton(t[:, 0], t[:, 1]) % n_parts == part]


def _records(rec, geom, spp, part=0, n_parts=1):
    """the pixels of the records, checked against the rectangle the restatement says is rendered (renderproc.cpp:146-153)"""
    pix = geom.key_to_pixel(rec[:, 7].copy().view(np.uint32))
    exp = _expected_pixels(geom, part, n_parts)
    assert len(rec) == len(exp) * spp
    assert np.array_equal(pix[::spp], pix.reshape(-1, spp, 2)[:, -1])                    # spp consecutive records per pixel
    key = lambda p: sorted(map(tuple, p))
    assert key(pix[::spp]) == key(exp)
    # every sample lies in the pixel of its key (the corner included: Halton's sample 0; pixel + u may round up to the far edge)
    assert ((rec[:, 4:6] >= pix) & (rec[:, 4:6] <= pix + 1)).all()
    return pix


def _render_and_check(it, c, table, geom, label, part=0, n_parts=1):
    assert it.render()
    film = it.film()
    rec = it.pass_samples()
    pix = _records(rec, geom, c["spp"], part, n_parts)
    res = fc.restate(rf, geom, table, rec, pix)
    w = fc.worst(res, film)
    print("%s: worst error / B %.3f, %d fragile of %d taps, %d invalid records" % (label, w, res.fragile, res.taps, (~rf.is_valid(rec[:, :3])).sum()))
    assert res.fragile <= fc.MAX_FRAGILE * res.taps
    assert w <= 1.0, label
    assert (rec[:, 3] == 0).any() and (rec[:, 3] == 1).any()
    return film, rec, pix, res


def _raster_positions(it, c, rec, pix, lens, count=300):
    """raster x, y of a record == its key's pixel + the matching next2D() of (key, sample index), bit for bit
    (integrator.cpp:154-166: with a thin lens the lens sample is drawn first)"""
    keys = rec[:, 7].copy().view(np.uint32)
    sel = np.unique(np.concatenate([np.arange(min(count // 2, len(rec))), np.linspace(0, len(rec) - 1, count // 2).astype(int)]))
    for i in sel:
        v = it.sampler_values(int(keys[i]), int(i % c["spp"]), 2, two_d=True)[1 if lens else 0]
        exp = (pix[i].astype(np.float32) + v).astype(np.float32)
        assert np.array_equal(exp.view(np.uint32), rec[i, 4:6].view(np.uint32)), (i, pix[i], v, rec[i, 4:6])
    return len(sel)


# --- box filter ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["box_independent", "box_halton", "box_crop"])
def test_box_lane_form(gpu_lib, mts, name):
    """k_accumulate: 4 spp.  Halton's sample 0 sits exactly on the pixel corner and adds weight 0"""
    c, table, it, geom = _tracer(mts, name)
    film, rec, pix, _ = _render_and_check(it, c, table, geom, name)
    if name == "box_halton":
        assert np.array_equal(film[..., 4], np.full((c["H"], c["W"]), c["spp"] - 1, dtype=np.float32))
        assert (rec[::c["spp"], 4:6] == pix[::c["spp"]]).all()
    if name == "box_independent":
        assert _raster_positions(it, c, rec, pix, lens=False) > 200


def test_box_wave_form(gpu_lib, mts):
    """k_accumulate_wave: 120 slots at 300 spp (>= 256 spp, <= 2^15 slots: the wave form by launch_accumulate's rule); 300 is
    no multiple of 64, so the last chunk has idle lanes.  The same frame in passes of 16 pixels equals it bit for bit"""
    c, table, it, geom = _tracer(mts, "box_wave")
    film, _, _, _ = _render_and_check(it, c, table, geom, "box_wave")
    it.set_options(max_paths=16 * c["spp"]); it.clear_film()
    assert it.render()
    assert np.array_equal(it.film().view(np.uint32), film.view(np.uint32))


def test_thin_lens_raster_positions(gpu_lib, mts):
    c, table, it, geom = _tracer(mts, "thin_lens")
    assert it.render()
    rec = it.pass_samples()
    pix = _records(rec, geom, c["spp"])
    assert _raster_positions(it, c, rec, pix, lens=True) > 200


# --- filters wider than a pixel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gaussian_bs8", "mitchell_bs8", "catmullrom_bs8", "wsinc_bs8", "gaussian_bs16", "gaussian_hq",
                                  "gaussian_crop", "gaussian_crop_hq", "asymmetric", "direct_hq"])
def test_wide_filters(gpu_lib, mts, name):
    """k_splat_blocks + k_add_blocks: 42 x 28 with blocks of 8 (neither a multiple; wsinc's border 3 makes 8 the tightest
    block), 16, highQualityEdges (border pixels at negative raster coordinates), a crop window at (5, 3) of 64 x 48, the
    asymmetric 1.25 x 2.5 table (nothing else sees a transposed lookup or swapped sizes), the direct integrator"""
    c, table, it, geom = _tracer(mts, name)
    film, rec, pix, _ = _render_and_check(it, c, table, geom, name)
    if c["hq"]:
        assert pix.min() == (0 if not c["crop"] else min(fc.CROP[:2])) - geom.border
    if name == "gaussian_hq":
        assert pix[:, 0].min() == -2 and rec[:, 4].min() < 0
        assert _raster_positions(it, c, rec, pix, lens=False) > 200


def test_wide_filter_passes(gpu_lib, mts):
    """the gaussian frame in passes of three tiles equals the one-pass film bit for bit"""
    c, table, it, geom = _tracer(mts, "gaussian_bs8")
    assert it.render()
    film = it.film()
    it.set_options(max_paths=3 * 64 * c["spp"]); it.clear_film()
    assert it.render()
    assert np.array_equal(it.film().view(np.uint32), film.view(np.uint32))


def test_wide_filter_tile_parts(gpu_lib, mts):
    """three tile parts: each part's film against the restatement of that part's samples, and the binary32 sum of the parts
    against the restatement of all samples (two more additions in k)"""
    c, table, it, geom = _tracer(mts, "gaussian_bs8")
    acc = np.zeros((c["H"], c["W"], 5), dtype=np.float32)
    total = None
    for part in range(3):
        it.set_tiles(c["bs"], part, 3); it.clear_film()
        film, _, _, res = _render_and_check(it, c, table, geom, "gaussian_bs8 part %d of 3" % part, part, 3)
        acc += film
        total = res if total is None else total + res
    w = fc.worst(total, acc, extra=2)
    print("gaussian_bs8, three parts summed: worst error / B %.3f" % w)
    assert w <= 1.0


def test_device_group(gpu_lib, mts):
    """a two-member group on one GPU, gaussian with highQualityEdges: the group's film against the restatement of both
    members' samples.  The members' passes are read through mtsgpu_group_ctx (the group has no read-out of its own)"""
    c = fc.case("gaussian_hq")
    sd = fc.scene_of(mts, c); scene = mts.Scene(sd)
    g = mts.DeviceGroup([0, 0], maxDepth=fc.MAX_DEPTH)
    g.preprocess(scene, _camera(mts, sd, c), sampler=c["sampler"], sampleCount=c["spp"], seed=fc.SEED)
    g.set_rfilter("gaussian")
    table = fc.filter_table(mts, c)
    geom = fc.geometry(rf, c, table[0], table[1])
    for i in range(2):
        assert mts.lib().mtsgpu_set_film_edges(g.member(i), 1) == 0
        assert mts.lib().mtsgpu_set_options(g.member(i), ONE_PASS, 0, 0) == 0
    assert g.render(block_size=c["bs"], ordered_reduce=True)
    film = g.film()
    total = None
    for i in range(2):
        rec = g.member_pass_samples(i)
        pix = _records(rec, geom, c["spp"], i, 2)
        res = fc.restate(rf, geom, table, rec, pix)
        total = res if total is None else total + res
    w = fc.worst(total, film, extra=1)
    print("group of two, gaussian_hq: worst error / B %.3f, %d fragile of %d taps" % (w, total.fragile, total.taps))
    assert w <= 1.0 and total.fragile <= fc.MAX_FRAGILE * total.taps
    g.close()


# --- the hook ----------------------------------------------------------------------------------------------------------------------
def test_pass_samples_refusals(gpu_lib, mts):
    c, table, it, geom = _tracer(mts, "box_independent")
    L = mts.lib()
    out = np.zeros((4, 8), dtype=np.float32)
    ESTATE, EINVAL = -5, -1
    assert L.mtsgpu_pass_samples(it._ctx, 0, 4, mts.abi.ptr(out, mts.abi.f32p)) == ESTATE            # before any render
    assert it.render()
    n = c["W"] * c["H"] * c["spp"]
    assert L.mtsgpu_pass_samples(it._ctx, n - 4, 4, mts.abi.ptr(out, mts.abi.f32p)) == 0
    assert L.mtsgpu_pass_samples(it._ctx, n - 3, 4, mts.abi.ptr(out, mts.abi.f32p)) == EINVAL        # past the end
    assert L.mtsgpu_pass_samples(it._ctx, 0xFFFFFFFF, 4, mts.abi.ptr(out, mts.abi.f32p)) == EINVAL
    assert L.mtsgpu_pass_samples(it._ctx, 0, 4, None) == EINVAL
    # the records are those of li_samples for the same (pixel, sample)
    rec = it.pass_samples(0, 8)
    pix = geom.key_to_pixel(rec[:, 7].copy().view(np.uint32))
    ps = np.concatenate([pix, (np.arange(8) % c["spp"])[:, None]], axis=1).astype(np.uint32)
    li = it.li_samples(ps)
    assert np.array_equal(li[:, :7].view(np.uint32), rec[:, :7].view(np.uint32))
    assert L.mtsgpu_pass_samples(it._ctx, 0, 4, mts.abi.ptr(out, mts.abi.f32p)) == ESTATE            # li_samples took the records
