"""A path whose ray leaves a scene without a background luminaire ends in the closest-hit kernel: its record already describes
the finished path (DConfig::miss_settled), so the ray goes to no material queue and nothing shades it.  The "miss_shaded" knob
at 1 sends it through the terminal queue and k_shade<10> as before.  Every film and every per-sample (Li, alpha, depth) is
compared bit for bit with the oracle's, in the four combinations of miss_shaded x sync_free (host-driven / device-driven
bounces) and once with nee_parked = 0; mtsgpu_bin_entries shows where the rays went.

The scenes are 32 x 32 pixels at 4 spp, put together from the pieces scenes.py builds its Cornell boxes from:

  floor     a floor quad under an area light, no walls, the camera tilted up so that its upper rows look past the far edge of the
            floor.  The light's quad is grey, not black as in the Cornell boxes, so that a path which reaches it goes on: then,
            below the depth limit and below rrDepth, a path of this scene ends only when a ray leaves it (nothing is hit from
            behind, no BSDF sample is zero), and the oracle's per-sample depths count the misses: rendered with maxDepth K + 1,
            the samples of final depth <= K are the paths that a miss ended within K rays (a miss at ray d leaves depth d).
            Every point of the floor sees the whole light, so every bounce miss follows an unoccluded light sample whose term is
            still parked in the record when the path ends (checked below with the oracle's any-hit rays: 0 of 2000 occluded).
  occluder  the same with a plate that shadows part of the floor: occluded light samples (cancelled terms) before a miss.
  apron     the same with a quad WITHOUT a BSDF below floor level behind the far edge and a black light: only camera rays reach
            the quad (the floor reflects upwards, a path that reaches the light ends there), their paths end on it
            (path.cpp:72-77) with alpha 1 and depth 1, and its hits are what the terminal queue still holds.
  sky       the floor under a constant background: a miss adds radiance, the frame keeps the shaded route whatever the knob says.

Shares measured on the CPU (oracle, ldsampler, seed 7; asserted below against 10 %): floor, 4096 samples: 56.5 % camera misses;
42.9 % / 43.4 % / 43.5 % of the samples end by a bounce miss at depth >= 2 with maxDepth 2 / 3 / 16, every one of them with a
light sample that came through (Li > 0); apron: 17.8 % of the samples end on the shape without a BSDF."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = H = 32
SPP = 4
SEED = 7
RR = 10
# (miss_shaded, sync_free, nee_parked): the four combinations, and the settled route once with the term travelling with the ray
MODES = [(ms, sf, 1) for ms in (0, 1) for sf in (1, 0)] + [(0, 1, 0)]


def _build(s, name, occluder=False, apron=False, sky=False):
    sd = s.SceneDescription(name)
    grey = sd.lambertian(0.5)
    pos, tri = s._quad((-1, 0, -1), (2, 0, 0), (0, 0, 2), (0, 1, 0))
    sd.add_mesh(pos, tri, bsdf=grey, face_normals=True, name="floor")
    lum = sd.add_lum(s.abi.LUM_AREA, [15.0] * 3)
    pos, tri = s._quad((-0.25, 1.99, -0.25), (0.5, 0, 0), (0, 0, 0.5), (0, -1, 0))
    # apron: a black light as in the Cornell boxes, where a path ends (its BSDF sample is zero) instead of going on downwards
    sd.add_mesh(pos, tri, bsdf=sd.lambertian(0.0) if apron else grey, lum=lum, face_normals=True, name="light")
    if occluder:
        pos, tri = s._quad((-0.9, 1.0, -0.3), (0.6, 0, 0), (0, 0, 0.6), (0, -1, 0))
        sd.add_mesh(pos, tri, bsdf=sd.twosided(grey), face_normals=True, name="plate")
    if apron:
        pos, tri = s._quad((-4, -0.5, -5), (8, 0, 0), (0, 0, 4), (0, 1, 0))
        sd.add_mesh(pos, tri, bsdf=-1, face_normals=True, name="apron")
    if sky:
        sd.add_lum(s.abi.LUM_CONSTANT, [0.5, 0.6, 0.7])
    sd.camera = dict(origin=(0.0, 1.0, 1.8), target=(0.0, 0.45, 0.0), up=(0.0, 1.0, 0.0), fov=39.3)
    return sd


CASES = {"floor": dict(), "occluder": dict(occluder=True), "apron": dict(apron=True), "sky": dict(sky=True)}
_cache = {}


def _scene(mts, orc, case):
    """description, product scene, oracle scene and the two cameras of a case: built once, shared, never changed"""
    if case not in _cache:
        sd = _build(mts.scenes, "miss_" + case, **CASES[case])
        _cache[case] = dict(sd=sd, scene=mts.Scene(sd), oscene=orc.FlatScene(sd), cam=mts.PerspectiveCamera.for_description(sd, W, H),
                            ocam=orc.make_camera(sd, W, H), ref={})
    return _cache[case]


def _all_samples():
    y, x, j = np.meshgrid(np.arange(H), np.arange(W), np.arange(SPP), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), j.ravel()], axis=1).astype(np.uint32)


def _params(mts, orc, sampler, max_depth, **kw):
    kind = {"independent": mts.abi.SAMPLER_INDEPENDENT_KEYED, "ldsampler": mts.abi.SAMPLER_LD_KEYED}[sampler]
    return orc.render_params(max_depth, rr_depth=RR, sampler=kind, spp=SPP, seed=SEED, **kw)


def _reference(orc, c, key, op):
    """the oracle's film, statistics and per-sample (Li, alpha, raster position, depth) of every sample, computed once per setting"""
    if key not in c["ref"]:
        film, st = orc.render(c["oscene"].scene, c["ocam"], op)
        c["ref"][key] = (film, st, orc.li_samples(c["oscene"].scene, c["ocam"], op, _all_samples()))
    return c["ref"][key]


def _ended_early(mts, orc, c, sampler, max_depth):
    """per sample: the path ended within max_depth rays by something other than the depth limit or Russian roulette -- read from
    the oracle's depths of the frame with one more ray allowed (see the module docstring); needs max_depth + 1 <= rrDepth"""
    assert max_depth + 1 <= RR
    _, _, li = _reference(orc, c, ("path", sampler, max_depth + 1), _params(mts, orc, sampler, max_depth + 1))
    return li[:, 6] <= max_depth, li


def _check_modes(mts, it, film_ref, li_ref, what, modes=MODES):
    """renders the frame in every mode, compares film and samples with the oracle's, returns {mode: (stats, bin entries)}"""
    ps = _all_samples()
    out = {}
    for ms, sf, nee in modes:
        it.set_tuning(miss_shaded=ms, sync_free=sf, nee_parked=nee)
        it.clear_film()
        assert it.render()
        film, st, bins = it.film(), it.stats(), it.bin_entries()
        tag = "%s, miss_shaded=%d sync_free=%d nee_parked=%d" % (what, ms, sf, nee)
        differ = int((film.view(np.uint32) != film_ref.view(np.uint32)).sum())
        assert differ == 0, "%s: film differs from the oracle's in %d values" % (tag, differ)
        # the records the film kernels read: same radiance, alpha and depth
        rec = it.pass_samples()
        assert rec.shape[0] == W * H * SPP
        got = it.li_samples(ps)
        bad = (got.view(np.uint32) != li_ref.view(np.uint32)).any(axis=1)
        assert not bad.any(), "%s: %d of %d samples differ (Li, alpha, position or depth)" % (tag, bad.sum(), len(ps))
        # one 32 x 32 tile: the records of the pass lie in the order of _all_samples()
        bad = (rec[:, :7].view(np.uint32) != li_ref[:, :7].view(np.uint32)).any(axis=1)
        assert not bad.any(), "%s: %d of %d records of the rendered pass differ" % (tag, bad.sum(), len(ps))
        out[(ms, sf, nee)] = (st, bins)
    return out


def _check_queues(res, ost, n_terminal_shaded, n_terminal_settled, what, path=True, shadows=True):
    """where the rays went: every finished ray is in exactly one queue when misses are shaded; the settled route leaves the
    misses out of the terminal queue and changes no other queue"""
    shaded = res[(1, 0, 1)][1]
    for (ms, sf, nee), (st, bins) in res.items():
        tag = "%s, miss_shaded=%d sync_free=%d nee_parked=%d" % (what, ms, sf, nee)
        assert st["rays_closest"] == ost.rays_closest, tag      # a dropped miss is still a ray that was traced
        assert (0 if shadows else -1) < st["rays_shadow"] == res[(1, 0, 1)][0]["rays_shadow"] <= ost.rays_shadow, tag
        if path:
            assert st["path_length_sum"] == ost.path_length_sum, tag
        assert bins[:-1] == shaded[:-1], tag
        assert bins[-1] == (n_terminal_shaded if ms else n_terminal_settled), tag
        if ms:
            assert sum(bins) == ost.rays_closest, tag


@pytest.mark.parametrize("sampler", ["ldsampler", "independent"])
@pytest.mark.parametrize("max_depth", [1, 2, 3, 16])
def test_camera_and_bounce_misses(gpu_lib, mts, orc, sampler, max_depth):
    c = _scene(mts, orc, "floor")
    film_ref, ost, li_ref = _reference(orc, c, ("path", sampler, max_depth), _params(mts, orc, sampler, max_depth))
    n = len(li_ref)
    # what the case is about, from the oracle alone
    camera_miss = li_ref[:, 3] == 0
    assert camera_miss.sum() >= 0.10 * n and (li_ref[camera_miss, 6] == 1).all() and (li_ref[camera_miss, :3] == 0).all()
    if max_depth <= 3:
        early, _ = _ended_early(mts, orc, c, sampler, max_depth)
    else:
        early = li_ref[:, 6] < min(max_depth, RR)           # below both limits in the frame itself: a lower bound of the misses
    bounce_miss = early & ~camera_miss
    assert (early & camera_miss).sum() == camera_miss.sum()
    if max_depth >= 2:
        assert bounce_miss.sum() >= 0.10 * n and (li_ref[bounce_miss, 6] >= 2).all()
        # each of them follows an unoccluded light sample from the floor or the light: its term is parked when the path ends
        assert (li_ref[bounce_miss, :3].sum(axis=1) > 0).all()
    else:
        assert bounce_miss.sum() == 0
    seg = _floor_to_light_segments()
    assert orc.trace_rays(c["oscene"].scene, seg, shadow=True)[:, 3].sum() == 0
    it = mts.MIPathTracer(maxDepth=max_depth, rrDepth=RR)
    it.preprocess(c["scene"], c["cam"], sampler=sampler, sampleCount=SPP, seed=SEED)
    res = _check_modes(mts, it, film_ref, li_ref, "floor maxDepth %d %s" % (max_depth, sampler))
    shaded = res[(1, 0, 1)][1]
    if max_depth <= 3:
        assert shaded[-1] == early.sum()                    # the oracle's miss count
    else:
        assert shaded[-1] >= early.sum()
    _check_queues(res, ost, shaded[-1], 0, "floor", shadows=max_depth >= 2)
    assert (film_ref[..., :3].max() > 0) == (max_depth >= 2)      # maxDepth 1: the camera hit is where the path ends, unlit


def _floor_to_light_segments(n=2000):
    """shadow segments from points of the floor to points of the light, as Scene::isOccluded takes them"""
    rng = np.random.RandomState(9)
    p1 = np.stack([rng.uniform(-0.99, 0.99, n), np.zeros(n), rng.uniform(-0.99, 0.99, n)], axis=1)
    p2 = np.stack([rng.uniform(-0.24, 0.24, n), np.full(n, 1.99), rng.uniform(-0.24, 0.24, n)], axis=1)
    seg = np.zeros((n, 8), dtype=np.float32)
    seg[:, 0:3] = p1; seg[:, 3] = 1e-3; seg[:, 4:7] = p2 - p1; seg[:, 7] = 1 - 1e-3
    return seg


def test_occluded_light_sample_before_a_miss(gpu_lib, mts, orc):
    c = _scene(mts, orc, "occluder")
    K = 3
    film_ref, ost, li_ref = _reference(orc, c, ("path", "ldsampler", K), _params(mts, orc, "ldsampler", K))
    occluded = orc.trace_rays(c["oscene"].scene, _floor_to_light_segments(), shadow=True)[:, 3]
    assert 0.05 * len(occluded) <= occluded.sum() <= 0.5 * len(occluded)          # part of the floor lies in the plate's shadow
    it = mts.MIPathTracer(maxDepth=K, rrDepth=RR)
    it.preprocess(c["scene"], c["cam"], sampler="ldsampler", sampleCount=SPP, seed=SEED)
    res = _check_modes(mts, it, film_ref, li_ref, "occluder")
    _check_queues(res, ost, res[(1, 0, 1)][1][-1], 0, "occluder")
    assert res[(1, 0, 1)][1][-1] >= 0.10 * len(li_ref)
    # samples whose camera hit is in shadow and whose bounce ray left the scene: nothing but zeros was ever added
    assert ((li_ref[:, 3] == 1) & (li_ref[:, 6] == 2) & (li_ref[:, :3].sum(axis=1) == 0)).sum() > 0


def test_shape_without_bsdf_keeps_the_terminal_queue(gpu_lib, mts, orc):
    c = _scene(mts, orc, "apron")
    K = 3
    film_ref, ost, li_ref = _reference(orc, c, ("path", "ldsampler", K), _params(mts, orc, "ldsampler", K))
    # camera rays that hit the shape without a BSDF: the only samples of alpha 1 that end at depth 1 when maxDepth > 1
    on_apron = (li_ref[:, 3] == 1) & (li_ref[:, 6] == 1)
    camera_miss = li_ref[:, 3] == 0
    assert on_apron.sum() >= 0.10 * len(li_ref) and camera_miss.sum() >= 0.10 * len(li_ref)
    it = mts.MIPathTracer(maxDepth=K, rrDepth=RR)
    it.preprocess(c["scene"], c["cam"], sampler="ldsampler", sampleCount=SPP, seed=SEED)
    res = _check_modes(mts, it, film_ref, li_ref, "apron")
    shaded = res[(1, 0, 1)][1]
    # shaded: the hits on the quad and every miss (here paths also end on the light, so the depths do not count the misses:
    # _check_queues holds the sum of the queues to the oracle's rays instead); settled: the hits on the quad alone
    assert shaded[-1] >= on_apron.sum() + camera_miss.sum() + 0.10 * len(li_ref)
    _check_queues(res, ost, shaded[-1], int(on_apron.sum()), "apron")


def test_background_scene_keeps_the_shaded_route(gpu_lib, mts, orc):
    c = _scene(mts, orc, "sky")
    K = 3
    film_ref, ost, li_ref = _reference(orc, c, ("path", "ldsampler", K), _params(mts, orc, "ldsampler", K))
    # a ray that reaches the background is a luminaire hit to the reference: no depth++ (path.cpp:147-170), so a miss at ray
    # d >= 2 leaves depth d - 1 here, and the misses within K rays are the samples of depth <= K - 1 of the frame with K + 1
    _, li_next = _ended_early(mts, orc, c, "ldsampler", K)
    early = li_next[:, 6] <= K - 1
    camera_miss = li_ref[:, 3] == 0
    assert camera_miss.sum() >= 0.10 * len(li_ref) and (li_ref[camera_miss, :3] == np.float32([0.5, 0.6, 0.7])).all()
    assert early.sum() > camera_miss.sum()
    it = mts.MIPathTracer(maxDepth=K, rrDepth=RR)
    it.preprocess(c["scene"], c["cam"], sampler="ldsampler", sampleCount=SPP, seed=SEED)
    res = _check_modes(mts, it, film_ref, li_ref, "sky")
    # the knob changes nothing here: every miss is shaded, it adds the background
    _check_queues(res, ost, int(early.sum()), int(early.sum()), "sky")


@pytest.mark.parametrize("nb", [1, 0])
def test_one_sample_direct_integrator(gpu_lib, mts, orc, nb):
    """direct has no depth to settle (no depth++ on a miss): the ray of its BSDF sample is dropped all the same"""
    c = _scene(mts, orc, "floor")
    op = _params(mts, orc, "ldsampler", -1, integrator="direct", luminaire_samples=1, bsdf_samples=nb)
    film_ref, ost, li_ref = _reference(orc, c, ("direct", 1, nb), op)
    it = mts.MIDirectIntegrator(luminaireSamples=1, bsdfSamples=nb)
    it.preprocess(c["scene"], c["cam"], sampler="ldsampler", sampleCount=SPP, seed=SEED)
    res = _check_modes(mts, it, film_ref, li_ref, "floor direct 1/%d" % nb)
    shaded = res[(1, 0, 1)][1]
    camera_miss = int((li_ref[:, 3] == 0).sum())
    assert shaded[-1] >= camera_miss and (shaded[-1] > camera_miss) == (nb == 1)
    _check_queues(res, ost, shaded[-1], 0, "floor direct", path=False)


def test_frames_without_the_material_sort_in_the_same_context(gpu_lib, mts, orc):
    """The launches of k_trace without the material sort are those of the direct integrator's rounds (the rays of its BSDF
    samples, shaded with their misses by k_shade<10> over the ray queue) and of mtsgpu_trace_rays.  They keep the shaded route,
    also right after and right before frames that settle their misses in the same context: the flag is the frame's."""
    c = _scene(mts, orc, "floor")
    op1 = _params(mts, orc, "ldsampler", -1, integrator="direct", luminaire_samples=1, bsdf_samples=1)
    op3 = _params(mts, orc, "ldsampler", -1, integrator="direct", luminaire_samples=2, bsdf_samples=3)
    film1, ost1, li1 = _reference(orc, c, ("direct", 1, 1), op1)
    film3, ost3, li3 = _reference(orc, c, ("direct", 2, 3), op3)
    it = mts.MIDirectIntegrator(luminaireSamples=1, bsdfSamples=1)
    it.preprocess(c["scene"], c["cam"], sampler="ldsampler", sampleCount=SPP, seed=SEED)
    one = [(0, 1, 1)]
    settled = _check_modes(mts, it, film1, li1, "direct 1/1", one)[one[0]][1]
    assert settled[-1] == 0
    it.luminaireSamples, it.bsdfSamples = 2, 3
    it.preprocess(c["scene"], c["cam"], sampler="ldsampler", sampleCount=SPP, seed=SEED)
    rounds = _check_modes(mts, it, film3, li3, "direct 2/3", one)[one[0]]
    assert rounds[1][-1] == int((li3[:, 3] == 0).sum())      # the camera misses, in the terminal queue: the rounds shade them
    assert rounds[0]["rays_closest"] == ost3.rays_closest
    # closest-hit rays through the test hook: hits in the records, no queue
    rays = np.zeros((256, 8), dtype=np.float32)
    rays[:, 0:3] = (0.0, 1.0, 1.8); rays[:, 3] = 1e-4; rays[:, 7] = np.inf
    rng = np.random.RandomState(3)
    d = np.stack([rng.uniform(-0.4, 0.4, 256), rng.uniform(-0.7, 0.2, 256), -np.ones(256)], axis=1)
    rays[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)
    hits, ohits = it.trace_rays(rays), orc.trace_rays(c["oscene"].scene, rays)
    assert np.array_equal(hits, ohits) and 0 < (hits[:, 3] == 0xFFFFFFFF).sum() < 256
    it.luminaireSamples, it.bsdfSamples = 1, 1
    it.preprocess(c["scene"], c["cam"], sampler="ldsampler", sampleCount=SPP, seed=SEED)
    again = _check_modes(mts, it, film1, li1, "direct 1/1 again", one)[one[0]][1]
    assert again == settled


def test_the_knob_is_range_checked(gpu_lib, mts):
    it = mts.MIPathTracer(maxDepth=2)
    it.set_tuning(miss_shaded=0); it.set_tuning(miss_shaded=1)
    for v in (-1, 2):
        with pytest.raises(mts.MtsGpuError):
            it.set_tuning(miss_shaded=v)
