"""Test-case mode on the device: the per-pixel variance film (k_variance / k_variance_wave of csrc/film.hip) against the
recurrence of SampleIntegrator::renderBlock (integrator.cpp:171-202) restated in numpy binary32 over mtsgpu_li_samples, bit
for bit.  12-triangle cornell_c1, maxDepth 5."""
import numpy as np
import pytest

from test_testmode import E2E, knuth_variance, oracle_reference_file, reject_bound

pytestmark = pytest.mark.gpu

F = np.float32
W, H = 37, 29                  # neither a multiple of 64 nor of the block size
MAX_DEPTH = 5
SEED = 0x5EED


def _tracer(mts, w=W, h=H, sampler="independent", spp=64, stats=True, camera=None, cls=None, seed=SEED):
    sd = mts.scenes.cornell_c1()
    it = cls() if cls else mts.MIPathTracer(maxDepth=MAX_DEPTH)
    cam = camera(sd) if camera else mts.PerspectiveCamera.for_description(sd, w, h)
    it.preprocess(mts.Scene(sd), cam, sampler=sampler, sampleCount=spp, seed=seed)
    if stats:
        it.set_film_statistics(True)
    return it


_expected = {}


def expected(mts, sampler, spp, w=W, h=H, cls=None, seed=SEED):
    """(variance [h][w][3], Li [h][w][spp][3]) from li_samples for every (x, y, j), computed once per configuration"""
    key = (sampler, spp, w, h, cls, seed)
    if key not in _expected:
        it = _tracer(mts, w, h, sampler, spp, stats=False, cls=cls, seed=seed)
        ys, xs, js = np.meshgrid(np.arange(h), np.arange(w), np.arange(spp), indexing="ij")
        li = it.li_samples(np.stack([xs, ys, js], -1).reshape(-1, 3)).reshape(h, w, spp, 8)[..., :3]
        it.close()
        var = knuth_variance(li)
        var.setflags(write=False); li.setflags(write=False)
        _expected[key] = (var, li)
    return _expected[key]


def same_bits(a, b):
    """equal bit for bit, NaNs in the same places (a NaN's payload is the processor's business)"""
    a = np.asarray(a, dtype=F); b = np.asarray(b, dtype=F)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32))


def render_stats(it, form=None):
    if form is not None:
        it.set_tuning(stats_wave=form)
    assert it.render()
    return it.film_statistics()


# --- 1. film sizes and sample counts, both forms -------------------------------------------------------------------------
@pytest.mark.parametrize("sampler,spp", [("independent", 1), ("independent", 2), ("independent", 3), ("independent", 64),
                                         ("independent", 65), ("independent", 130), ("ldsampler", 64)])
def test_variance_matches_the_recurrence(gpu_lib, mts, sampler, spp):
    var_e, li = expected(mts, sampler, spp)
    it = _tracer(mts, sampler=sampler, spp=spp)
    got = {}
    for form in (0, 1):
        var, n = render_stats(it, form)
        assert it.film_statistics_form() == ("lane", "wave")[form]
        assert (n == spp).all()
        assert same_bits(var, var_e), "form %d: %d of %d values differ" % (form, (var.view(np.uint32) != var_e.view(np.uint32)).sum(), var.size)
        got[form] = var
        it.clear_film()
    assert same_bits(got[0], got[1])
    if spp == 1:
        assert np.isnan(var_e).all() and np.isnan(got[0]).all()          # 0 * (1 / 0): the reference stores that too
    else:
        assert np.isfinite(var_e).all() and (var_e > 0).any() and (li.std(axis=2) > 0).any()
    it.close()


# --- 2. passes of 7 pixels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", [0, 1])
def test_pass_splitting_changes_nothing(gpu_lib, mts, form):
    spp = 65
    var_e, _ = expected(mts, "independent", spp)
    it = _tracer(mts, spp=spp)
    it.set_options(max_paths=7 * spp)
    var, n = render_stats(it, form)
    assert (n == spp).all() and same_bits(var, var_e)
    it.close()


# --- 3. tiles and crop window ---------------------------------------------------------------------------------------------
def _morton(tx, ty):
    m = 0
    for b in range(16):
        m |= ((tx >> b) & 1) << (2 * b) | ((ty >> b) & 1) << (2 * b + 1)
    return m


def test_tile_parts_leave_other_pixels_alone(gpu_lib, mts):
    spp = 3
    var_e, _ = expected(mts, "independent", spp)
    ys, xs = np.mgrid[0:H, 0:W]
    part = np.vectorize(lambda x, y: _morton(x // 8, y // 8) % 3)(xs, ys)
    seen = np.zeros((H, W), dtype=np.uint32)
    for p in range(3):
        it = _tracer(mts, spp=spp)
        it.set_tiles(8, p, 3)
        var, n = render_stats(it)
        own = part == p
        assert own.any() and np.array_equal(n, np.where(own, spp, 0).astype(np.uint32)), p
        assert same_bits(var[own], var_e[own]) and not var[~own].view(np.uint32).any(), p
        seen += n
        it.close()
    assert (seen == spp).all()


def test_crop_window(gpu_lib, mts):
    spp = 3
    var_e, _ = expected(mts, "independent", spp)
    x0, y0, cw, ch = 5, 3, 20, 17
    it = _tracer(mts, spp=spp, camera=lambda sd: mts.PerspectiveCamera.cropped(sd, W, H, (x0, y0, cw, ch)))
    for form in (0, 1):
        var, n = render_stats(it, form)
        assert var.shape == (ch, cw, 3) and (n == spp).all()
        assert same_bits(var, var_e[y0:y0 + ch, x0:x0 + cw]), form          # a cropped render is that rectangle of the full one
    it.close()


# --- 4. few pixels, many samples: the rule picks the wave form -----------------------------------------------------------
def test_rule_picks_the_wave_form_for_few_pixels_with_many_samples(gpu_lib, mts):
    w, h, spp = 5, 3, 4096
    var_e, _ = expected(mts, "independent", spp, w, h)
    it = _tracer(mts, w, h, spp=spp)
    var, n = render_stats(it)
    assert it.film_statistics_form() == "wave"
    assert (n == spp).all() and same_bits(var, var_e)
    it.close()
    it = _tracer(mts, spp=64)
    render_stats(it)
    assert it.film_statistics_form() == "lane"
    it.close()


# --- 5. the film does not change ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["independent", "ldsampler"])
def test_film_keeps_its_bits(gpu_lib, mts, sampler):
    off = _tracer(mts, sampler=sampler, spp=64, stats=False)
    assert off.render() and off.film_statistics_form() is None
    ref = off.film()
    off.close()
    on = _tracer(mts, sampler=sampler, spp=64)
    for form in (0, 1):
        render_stats(on, form)
        assert np.array_equal(on.film().view(np.uint32), ref.view(np.uint32)), form
        on.clear_film()
    on.set_film_statistics(False)
    assert on.render() and np.array_equal(on.film().view(np.uint32), ref.view(np.uint32))
    on.close()


# --- 6. clearing ----------------------------------------------------------------------------------------------------------
def test_clear_film_clears_the_statistics(gpu_lib, mts):
    it = _tracer(mts, spp=3)
    var, n = render_stats(it)
    assert (n == 3).all() and var.view(np.uint32).any()
    it.clear_film()
    var, n = it.film_statistics()
    assert not n.any() and not var.view(np.uint32).any() and not it.film().view(np.uint32).any()
    it.close()


# --- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_refusals(gpu_lib, mts):
    spp = 3
    var_e, _ = expected(mts, "independent", spp)
    it = _tracer(mts, spp=spp)
    it.set_rfilter("gaussian")
    with pytest.raises(mts.MtsGpuError, match=r"box filter.*\(code -1\)"):                 # MTSGPU_EINVAL
        it.render()
    it.set_rfilter("box")                                                                  # the context is still usable
    var, n = render_stats(it)
    assert (n == spp).all() and same_bits(var, var_e)
    it.set_film_statistics(False)
    with pytest.raises(mts.MtsGpuError, match=r"\(code -5\)"):                             # MTSGPU_ESTATE
        it.film_statistics()
    it.set_rfilter("gaussian")
    assert it.render()                                                                     # mode off: wide filters render
    it.close()


# --- 8. device group: two members on one device ---------------------------------------------------------------------------
@pytest.mark.parametrize("ordered", [False, True])
def test_group_merges_the_statistics_on_member_0(gpu_lib, mts, ordered):
    spp = 3
    var_e, _ = expected(mts, "independent", spp)
    single = _tracer(mts, spp=spp, stats=False)
    assert single.render()
    film = single.film()
    single.close()
    sd = mts.scenes.cornell_c1()
    g = mts.DeviceGroup([0, 0], maxDepth=MAX_DEPTH)
    g.preprocess(mts.Scene(sd), mts.PerspectiveCamera.for_description(sd, W, H), sampler="independent", sampleCount=spp, seed=SEED)
    g.set_film_statistics(True)
    assert g.render(block_size=8, ordered_reduce=ordered)
    var, n = g.film_statistics()
    assert (n == spp).all() and same_bits(var, var_e)
    assert np.array_equal(g.film().view(np.uint32), film.view(np.uint32))
    g.set_film_statistics(False)
    with pytest.raises(mts.MtsGpuError, match=r"\(code -5\)"):
        g.film_statistics()
    g.close()


# --- 9. the direct integrator inherits the mode ---------------------------------------------------------------------------
def test_direct_integrator(gpu_lib, mts):
    w = h = 16; spp = 4
    var_e, _ = expected(mts, "independent", spp, w, h, cls=mts.MIDirectIntegrator)
    it = _tracer(mts, w, h, spp=spp, cls=mts.MIDirectIntegrator)
    for form in (0, 1):
        var, n = render_stats(it, form)
        assert (n == spp).all() and same_bits(var, var_e) and (var_e > 0).any()
    it.close()


# --- 10. the t-test on the device's own film ------------------------------------------------------------------------------
def test_t_test_end_to_end_on_the_device(gpu_lib, mts, orc, tmp_path):
    """test_testmode.test_t_test_end_to_end_on_the_oracle with the device's .m file in place of the oracle's, against the same
    .ref and the same bound; film and variance are also the oracle-derived ones bit for bit"""
    n, spp = E2E["size"], E2E["spp"]
    it = _tracer(mts, n, n, spp=spp, seed=E2E["seed"])
    var, ns = render_stats(it)
    film = it.film()
    it.close()
    sd = mts.scenes.cornell_c1()
    osc = orc.FlatScene(sd); ocam = orc.make_camera(sd, n, n)
    op = orc.render_params(MAX_DEPTH, spp=spp, seed=E2E["seed"])
    ys, xs, js = np.meshgrid(np.arange(n), np.arange(n), np.arange(spp), indexing="ij")
    oli = orc.li_samples(osc.scene, ocam, op, np.stack([xs, ys, js], -1).reshape(-1, 3)).reshape(n, n, spp, 8)
    ofilm, _ = orc.render(osc.scene, ocam, op)
    assert np.array_equal(film.view(np.uint32), ofilm.view(np.uint32))
    assert same_bits(var, knuth_variance(oli[..., :3])) and (ns == spp).all()
    m, ref = str(tmp_path / "cornell.m"), str(tmp_path / "cornell.ref")
    mts.write_mfile(m, film, stats=(var, ns))
    oracle_reference_file(mts, orc, ref)
    r = mts.analyze(m, ref, "t-test", E2E["thresh"])
    print("rejecting pixels: %d of %d (bound %d); %s" % (r.rejects, n * n, reject_bound(), r.message))
    assert r.rejects < reject_bound()
