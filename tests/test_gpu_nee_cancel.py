"""The pending direct-light term of a shadow ray: parked in the path record by the shading, cancelled by the any-hit kernel
when the ray is occluded (DQueues::nee_parked = 1), against the term travelling with the ray (nee_parked = 0), in the
host-driven and the device-driven bounce loop (sync_free = 0 / 1).  Every film is compared bit for bit with the oracle's,
so the films of the four modes are equal to each other as well.

The scenes are 32 x 32 pixels at 4 spp.  `open` and `covered` are put together from the pieces scenes.py builds its Cornell
boxes from (no ready-made scene has no or only occluded shadow rays); `mixed` is cornell_c5."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W = H = 32
SPP = 4
SEED = 7
MODES = [(nee, sf) for nee in (1, 0) for sf in (1, 0)]        # (nee_parked, sync_free)


def _floor_and_light(s, name, covered):
    sd = s.SceneDescription(name)
    grey = sd.lambertian(0.5)
    pos, tri = s._quad((-1, 0, -1), (2, 0, 0), (0, 0, 2), (0, 1, 0))
    sd.add_mesh(pos, tri, bsdf=grey, face_normals=True, name="floor")
    if covered:
        # a plate right under the light, wide enough to hide it from the whole floor and from the camera
        pos, tri = s._quad((-1, 1.9, -1), (2, 0, 0), (0, 0, 2), (0, -1, 0))
        sd.add_mesh(pos, tri, bsdf=grey, face_normals=True, name="plate")
    s._add_light(sd)
    sd.camera = dict(origin=(0.0, 1.0, 1.8), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=39.3)
    sd.max_depth = 4
    return sd


def _mixed(s):
    sd = s.cornell_c5(sphere_subdiv=2)
    sd.max_depth = 2          # the term of the camera hit is settled by the path's last shading or, if that never comes, by the film kernels
    return sd


CASES = {"open": lambda s: _floor_and_light(s, "nee_open", False),
         "covered": lambda s: _floor_and_light(s, "nee_covered", True),
         "mixed": _mixed}

_cache = {}


def _scene(mts, orc, case):
    """description, product scene, oracle scene and the two cameras of a case: built once, shared, never changed"""
    if case not in _cache:
        sd = CASES[case](mts.scenes)
        _cache[case] = dict(sd=sd, scene=mts.Scene(sd), oscene=orc.FlatScene(sd), cam=mts.PerspectiveCamera.for_description(sd, W, H),
                            ocam=orc.make_camera(sd, W, H), ref={})
    return _cache[case]


def _reference(mts, orc, c, key, op, ps):
    """the oracle's film and per-sample radiance for one integrator setting of a case, computed once"""
    if key not in c["ref"]:
        film, st = orc.render(c["oscene"].scene, c["ocam"], op)
        c["ref"][key] = (film, st, orc.li_samples(c["oscene"].scene, c["ocam"], op, ps))
    return c["ref"][key]


def _samples():
    rng = np.random.RandomState(5)
    return np.stack([rng.randint(0, W, 600), rng.randint(0, H, 600), rng.randint(0, SPP, 600)], axis=1).astype(np.uint32)


def _floor_to_light_segments(n=2000):
    """shadow segments from points of the floor to points of the light, as Scene::isOccluded takes them"""
    rng = np.random.RandomState(9)
    p1 = np.stack([rng.uniform(-0.99, 0.99, n), np.zeros(n), rng.uniform(-0.99, 0.99, n)], axis=1)
    p2 = np.stack([rng.uniform(-0.24, 0.24, n), np.full(n, 1.99), rng.uniform(-0.24, 0.24, n)], axis=1)
    seg = np.zeros((n, 8), dtype=np.float32)
    seg[:, 0:3] = p1; seg[:, 3] = 1e-3; seg[:, 4:7] = p2 - p1; seg[:, 7] = 1 - 1e-3
    return seg


def _check_all_modes(mts, it, c, film_ref, li_ref, ps, what):
    for nee, sf in MODES:
        it.set_tuning(nee_parked=nee, sync_free=sf)
        it.clear_film()
        assert it.render()
        film, st = it.film(), it.stats()
        assert np.array_equal(film.view(np.uint32), film_ref.view(np.uint32)), \
            "%s, nee_parked=%d sync_free=%d: film differs from the oracle's in %d values" \
            % (what, nee, sf, int((film.view(np.uint32) != film_ref.view(np.uint32)).sum()))
        # the read-out hook settles what is still parked in the records the way the film kernels do
        got = it.li_samples(ps)
        bad = (got.view(np.uint32) != li_ref.view(np.uint32)).any(axis=1)
        assert not bad.any(), "%s, nee_parked=%d sync_free=%d: %d of %d samples differ" % (what, nee, sf, bad.sum(), len(ps))
    return film, st


@pytest.mark.parametrize("case", list(CASES))
def test_path_films_equal_the_oracle_in_every_mode(gpu_lib, mts, orc, case):
    c = _scene(mts, orc, case)
    sd = c["sd"]
    ps = _samples()
    op = orc.render_params(sd.max_depth, sampler=mts.abi.SAMPLER_LD_KEYED, spp=SPP, seed=SEED)
    film_ref, ost, li_ref = _reference(mts, orc, c, "path", op, ps)
    it = mts.MIPathTracer(maxDepth=sd.max_depth)
    it.preprocess(c["scene"], c["cam"], sampler="ldsampler", sampleCount=SPP, seed=SEED)
    if case in ("open", "covered"):
        # what the case is about: no / every segment between the floor and the light is occluded
        occluded = it.trace_rays(_floor_to_light_segments(), shadow=True)[:, 3]
        assert occluded.sum() == (len(occluded) if case == "covered" else 0)
    film, st = _check_all_modes(mts, it, c, film_ref, li_ref, ps, case)
    assert st["rays_shadow"] > 0 and st["rays_closest"] == ost.rays_closest
    if case == "covered":
        assert film_ref[..., :3].max() == 0 and film[..., :3].max() == 0      # the direct term is exactly absent
    else:
        assert film_ref[..., :3].max() > 0


@pytest.mark.parametrize("case,nb", [("mixed", 1), ("mixed", 0), ("covered", 0)])
def test_one_sample_direct_integrator(gpu_lib, mts, orc, case, nb):
    """MIDirectIntegrator with one luminaire sample runs the bounce loops of the path tracer; without a BSDF sample every
    path ends in the shading that issued its shadow ray, and only the film kernels (or the read-out hook) see its term"""
    c = _scene(mts, orc, case)
    ps = _samples()
    op = orc.render_params(-1, sampler=mts.abi.SAMPLER_LD_KEYED, spp=SPP, seed=SEED, integrator="direct", luminaire_samples=1, bsdf_samples=nb)
    film_ref, ost, li_ref = _reference(mts, orc, c, ("direct", 1, nb), op, ps)
    it = mts.MIDirectIntegrator(luminaireSamples=1, bsdfSamples=nb)
    it.preprocess(c["scene"], c["cam"], sampler="ldsampler", sampleCount=SPP, seed=SEED)
    film, st = _check_all_modes(mts, it, c, film_ref, li_ref, ps, "%s direct 1/%d" % (case, nb))
    assert st["rays_shadow"] > 0 and st["rays_closest"] == ost.rays_closest
    if case == "covered":
        assert film[..., :3].max() == 0
    else:
        assert film_ref[..., :3].max() > 0


def test_direct_rounds_allocate_their_term_queue(gpu_lib, mts, orc):
    """several luminaire samples: the rounds add their terms to Li one after the other (nothing is parked), in a context
    that has not run such a frame before, and again after a frame that parked its terms"""
    c = _scene(mts, orc, "mixed")
    ps = _samples()
    op = orc.render_params(-1, sampler=mts.abi.SAMPLER_LD_KEYED, spp=SPP, seed=SEED, integrator="direct", luminaire_samples=3, bsdf_samples=1)
    film_ref, ost, li_ref = _reference(mts, orc, c, ("direct", 3, 1), op, ps)
    it = mts.MIDirectIntegrator(luminaireSamples=3, bsdfSamples=1)
    it.preprocess(c["scene"], c["cam"], sampler="ldsampler", sampleCount=SPP, seed=SEED)
    assert it.render()
    assert np.array_equal(it.film().view(np.uint32), film_ref.view(np.uint32))
    assert film_ref[..., :3].max() > 0 and it.stats()["rays_shadow"] > 0
    assert np.array_equal(it.li_samples(ps).view(np.uint32), li_ref.view(np.uint32))
    # a larger frame of the one-sample kind in between (new path buffers, terms parked), then the rounds again
    big = mts.PerspectiveCamera.for_description(c["sd"], 2 * W, 2 * H)
    it.luminaireSamples = 1
    it.preprocess(c["scene"], big, sampler="ldsampler", sampleCount=SPP, seed=SEED)
    it.clear_film(); assert it.render()
    op1 = orc.render_params(-1, sampler=mts.abi.SAMPLER_LD_KEYED, spp=SPP, seed=SEED, integrator="direct", luminaire_samples=1, bsdf_samples=1)
    obig, _ = orc.render(c["oscene"].scene, orc.make_camera(c["sd"], 2 * W, 2 * H), op1)
    assert np.array_equal(it.film().view(np.uint32), obig.view(np.uint32))
    it.luminaireSamples = 3
    it.preprocess(c["scene"], big, sampler="ldsampler", sampleCount=SPP, seed=SEED)
    it.clear_film(); assert it.render()
    obig3, _ = orc.render(c["oscene"].scene, orc.make_camera(c["sd"], 2 * W, 2 * H), op)
    assert np.array_equal(it.film().view(np.uint32), obig3.view(np.uint32))
