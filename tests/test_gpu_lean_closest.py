"""The closest-hit kernel without the mailbox (k_trace LEAN, tuning key "lean_closest") against the kernel with it and
against the oracle: hits, films and material queues are the same bits, and the rays on which two primitives tie in t --
the only ones the mailbox can decide -- are found, handed to the kernel with the mailbox and counted (rays_redone).

The knob is a mask of launch classes (render.cpp: traceAndBin): 1 = incoherent launches of at least plainBelow rays, 2 = the
coherent first launch, 4 = launches below plainBelow.  The launches of these tests are small, so "on" is 7 here, and
plain_below = 1 puts the same rays through the class of bit 1 (the loops with the early exits)."""
import os

import numpy as np
import pytest

import geom_cases as GC
from conftest import chord_rays

gpu = pytest.mark.gpu

F = np.float32
MISS = 0xFFFFFFFF
OFF = dict(lean_closest=0)
ON = [dict(lean_closest=7), dict(lean_closest=7, plain_below=1)]
_cache = {}


# ---------------------------------------------------------------------------------------------------------------------
# scenes and rays
# ---------------------------------------------------------------------------------------------------------------------
def _doubled(mts):
    """a mesh with every triangle twice (the second copy listed after the first), under a point light"""
    rng = np.random.RandomState(11)
    c = rng.rand(60, 1, 3) * 2 - 1
    tris = c + 0.5 * (rng.rand(60, 3, 3) * 2 - 1)
    tris[:, :, 1] += 1.0
    sd = mts.scenes.SceneDescription("doubled")
    pos = tris.reshape(-1, 3)
    idx = np.arange(180).reshape(-1, 3)
    sd.add_mesh(pos, np.concatenate([idx, idx]), bsdf=sd.lambertian(0.5), face_normals=True)
    sd.point_light((0.0, 5.0, 0.0), 1.0)
    return sd


GRID_N = 6


def _grid(mts):
    """a coarse GRID_N x GRID_N grid of quads in the plane z = 0.25, two triangles per quad, every coordinate a multiple of
    1/4: the triangles share edges and vertices, their TriAccel planes are the same numbers, and a ray through a lattice
    point meets up to six of them with the same t"""
    n = GRID_N
    xs = (np.arange(n + 1) - n / 2) * 0.25
    pos = np.array([[x, y + 1.0, 0.25] for y in xs for x in xs], dtype=np.float64)
    v = lambda i, j: j * (n + 1) + i
    idx = []
    for j in range(n):
        for i in range(n):
            idx += [[v(i, j), v(i + 1, j), v(i + 1, j + 1)], [v(i, j), v(i + 1, j + 1), v(i, j + 1)]]
    sd = mts.scenes.SceneDescription("grid")
    sd.add_mesh(pos, np.array(idx), bsdf=sd.lambertian(0.5), face_normals=True)
    sd.point_light((0.0, 5.0, 0.0), 1.0)
    return sd


def _grid_rays():
    """from a few origins with coordinates in multiples of 1/4, at every vertex of the grid, every edge midpoint (multiples
    of 1/8) and a few interior points; the differences are exact, so is the plane distance where the direction is kept
    unnormalised (a ray's direction need not be a unit vector, ray.h)"""
    n = GRID_N
    pts = []
    for j in range(2 * n + 1):
        for i in range(2 * n + 1):
            pts.append(((i - n) * 0.125, (j - n) * 0.125 + 1.0, 0.25))
    pts = np.array(pts, dtype=np.float64)
    rays = []
    for o in [(0.0, 1.0, 2.25), (0.5, 0.5, 1.25), (-0.25, 1.75, 4.25), (0.125, 1.125, 1.25)]:
        o = np.array(o)
        d = pts - o
        r = np.zeros((len(pts), 8), dtype=F)
        r[:, 0:3] = o; r[:, 3] = 1e-4; r[:, 4:7] = d; r[:, 7] = np.inf
        rays.append(r)
        r = r.copy(); r[:, 4:7] = d / np.linalg.norm(d, axis=1, keepdims=True)     # and normalised: mostly no ties, some
        rays.append(r)
    return np.concatenate(rays)


def _edge_case_scene(mts):
    """test_gpu_parity.test_edge_cases: degenerate and duplicated triangles next to the Cornell box"""
    sd = mts.scenes.cornell_c1()
    pos = np.array([[-0.3, 0.5, 0.0], [0.3, 0.5, 0.0], [0.0, 1.1, 0.0], [0.1, 0.1, 0.1]], dtype=F)
    tri = np.array([[0, 1, 2], [0, 1, 2], [3, 3, 3], [0, 1, 1], [2, 1, 0]], dtype=np.uint32)
    sd.add_mesh(pos, tri, bsdf=sd.lambertian(0.5), face_normals=True, name="degenerate")
    return sd


def _bunny(mts):
    import ply_io
    pos, tri = ply_io.read(os.path.join(os.path.dirname(__file__), "golden", "bunny.ply.gz"))
    sd = mts.scenes.SceneDescription("bunny")
    sd.add_mesh(pos, tri, bsdf=sd.lambertian(0.5), face_normals=False, name="bunny")
    sd.point_light((0.0, 0.5, 0.5), 1.0)
    return sd


def _box_rays(n, seed):
    rng = np.random.RandomState(seed)
    o = rng.uniform(-0.95, 0.95, (n, 3)); o[:, 1] = rng.uniform(0.05, 1.95, n)
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([o, np.full((n, 1), 1e-4), d, np.full((n, 1), np.inf)], axis=1).astype(F)


N = 4000
HIT_SCENES = {
    # name: (scene description, rays)
    "twins": lambda m, o: (GC.scene_description(m, "twins"), GC.case(m, "twins").rays),
    "degenerate": lambda m, o: (GC.scene_description(m, "degenerate"), GC.case(m, "degenerate").rays),
    "fan": lambda m, o: (GC.scene_description(m, "fan"), GC.case(m, "fan").rays),
    "geom_spheres": lambda m, o: (GC.scene_description(m, "spheres"), GC.case(m, "spheres").rays),
    "spheres": lambda m, o: (m.scenes.spheres(), chord_rays(N, (0, 1, 0), 2.2, seed=7)),
    "c3_small": lambda m, o: (m.scenes.cornell_c3(grid=24, sphere_subdiv=2), chord_rays(N, (0, 1, 0), 2.2, seed=7)),
    "edge_cases": lambda m, o: (_edge_case_scene(m), chord_rays(N, (0, 1, 0), 2.2, seed=5)),
    "fuzz3": lambda m, o: (m.scenes.fuzz(3), _box_rays(N, 3)),
    "bunny": lambda m, o: (_bunny(m), o.chord_rays((-0.016840, 0.110154, -0.001537), 0.2, N)),
    "doubled": lambda m, o: (_doubled(m), chord_rays(N, (0, 1, 0), 2.2, seed=9)),
    "grid": lambda m, o: (_grid(m), _grid_rays()),
}


TIE_FREE = ("degenerate", "bunny")


def _hit_case(mts, orc, name):
    """scene, rays and the oracle's hits: built once, shared, never changed"""
    if name not in _cache:
        sd, rays = HIT_SCENES[name](mts, orc)
        oscene = orc.FlatScene(sd)
        rays = np.ascontiguousarray(rays, dtype=F)
        _cache[name] = dict(sd=sd, scene=mts.Scene(sd), oscene=oscene, rays=rays, exp=orc.trace_rays(oscene.scene, rays))
    return _cache[name]


def _tracer(mts, c, **knobs):
    it = mts.MIPathTracer(maxDepth=2)
    it.preprocess(c["scene"], mts.PerspectiveCamera.for_description(c["sd"], 16, 16), sampler="independent", sampleCount=1)
    it.set_tuning(**knobs)
    return it


def _equal_t_candidates(c):
    """How many rays of the case have, by the oracle's own arrays, a second primitive that passes TriAccel::rayIntersect with
    the bits of the reported t: the test of triaccel.h:98-159 in binary32, one rounding per operation, over every triangle"""
    ta = c["oscene"].arrays()["triaccel"]
    k = ta[:, 0].astype(np.int64)
    f = ta[:, 1:10].view(F)
    n_u, n_v, n_d, a_u, a_v, b_nu, b_nv, c_nu, c_nv = (f[:, i] for i in range(9))
    rays, exp = c["rays"], c["exp"]
    found = np.nonzero(exp[:, 3] != MISS)[0]
    tied = 0
    ok = k < 3
    ku, kv = (k + 1) % 3, (k + 2) % 3
    with np.errstate(all="ignore"):
        for r in found:
            o, d = rays[r, 0:3], rays[r, 4:7]
            o_u, o_v, o_k = o[ku % 3], o[kv % 3], o[k % 3]
            d_u, d_v, d_k = d[ku % 3], d[kv % 3], d[k % 3]
            recip = F(1.0) / ((d_u * n_u + d_v * n_v) + d_k)
            t = (((n_d - o_u * n_u) - o_v * n_v) - o_k) * recip
            hu = (o_u + t * d_u) - a_u
            hv = (o_v + t * d_v) - a_v
            u = hv * b_nu + hu * b_nv
            v = hu * c_nu + hv * c_nv
            same = ok & (t.view(np.uint32) == exp[r, 0]) & (u >= 0) & (v >= 0) & (u + v <= F(1.0))
            if same.sum() >= 2:
                tied += 1
    return tied, len(found)


# ---------------------------------------------------------------------------------------------------------------------
# hits
# ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", list(HIT_SCENES))
def test_hits_equal_the_oracle_with_the_knob_on_and_off(gpu_lib, mts, orc, name):
    c = _hit_case(mts, orc, name)
    exp = c["exp"]
    assert (exp[:, 3] != MISS).sum() > 100, "the rays of %s hit too little" % name
    for knobs in [OFF] + ON:
        it = _tracer(mts, c, **knobs)
        got = it.trace_rays(c["rays"])
        st = it.stats()
        it.close()
        bad = (got != exp).any(axis=1)
        print(name, knobs, "redone", st["rays_redone"], "of", len(exp))
        assert not bad.any(), "%s %s: (t, u, v, prim) differs in %d rays, first %s got %s exp %s" % (
            name, knobs, bad.sum(), c["rays"][bad][:1], got[bad][:1], exp[bad][:1])
        assert st["rays_closest"] == len(exp)
        if not knobs["lean_closest"]:
            assert st["rays_redone"] == 0


def test_the_tie_scenes_have_equal_t_candidates(mts, orc):
    """Without a GPU: by the oracle's arrays, the duplicated mesh offers a second candidate with the reported t on every ray that
    hits it and the grid on the rays through its lattice points; the soup with degenerate triangles and the bunny offer none
    (the fan, with its shared edges and rays aimed at them, on 7 rays of 2 735)"""
    tied, found = _equal_t_candidates(_hit_case(mts, orc, "doubled"))
    assert found > 100 and tied == found, (tied, found)
    tied, found = _equal_t_candidates(_hit_case(mts, orc, "grid"))
    assert tied > 100, (tied, found)
    for name in TIE_FREE:
        tied, found = _equal_t_candidates(_hit_case(mts, orc, name))
        assert found > 100 and tied == 0, (name, tied, found)


@gpu
def test_the_redo_happens_where_primitives_tie_and_nowhere_else(gpu_lib, mts, orc):
    d, g = (_hit_case(mts, orc, n) for n in ("doubled", "grid"))
    tied_d, found_d = _equal_t_candidates(d)
    assert tied_d == found_d > 100
    for knobs in ON:
        it = _tracer(mts, d, **knobs)
        assert np.array_equal(it.trace_rays(d["rays"]), d["exp"])
        redone = it.stats()["rays_redone"]
        # every ray that hits the doubled mesh accepts the second copy with the t of the first
        assert redone == found_d, (redone, found_d)
        it.close()
        it = _tracer(mts, g, **knobs)
        assert np.array_equal(it.trace_rays(g["rays"]), g["exp"])
        assert it.stats()["rays_redone"] > 0
        it.close()
        # a ray is redone only if two primitives pass the test with the t it reports: none does where none can
        for name in TIE_FREE:
            f = _hit_case(mts, orc, name)
            assert _equal_t_candidates(f)[0] == 0
            it = _tracer(mts, f, **knobs)
            assert np.array_equal(it.trace_rays(f["rays"]), f["exp"])
            assert it.stats()["rays_redone"] == 0, name
            it.close()


# ---------------------------------------------------------------------------------------------------------------------
# films and material queues
# ---------------------------------------------------------------------------------------------------------------------
W = H = 32
SPP = 4
FILM_SCENES = {
    "fuzz1": lambda s: s.fuzz(1), "fuzz2": lambda s: s.fuzz(2), "fuzz3": lambda s: s.fuzz(3),
    "c3_grid8": lambda s: s.cornell_c3(grid=8, sphere_subdiv=2),
    "doubled": None,
}
# host-driven frames (device-driven frames keep the kernel with the mailbox: nothing of this change runs in them)
DRIVES = [dict(sync_free=0), dict(sync_free=0, plain_below=1), dict(sync_free=0, test_retry=1), dict(sync_free=0, max_paths=SPP * (W * H // 3 + 1))]


def _film_scene(mts, name):
    if ("film", name) not in _cache:
        if name == "doubled":
            sd = _doubled(mts)
            sd.camera = dict(origin=(0.0, 1.0, 4.0), target=(0.0, 1.0, 0.0), up=(0.0, 1.0, 0.0), fov=40.0)
        else:
            sd = FILM_SCENES[name](mts.scenes)
        _cache[("film", name)] = (sd, mts.Scene(sd), mts.PerspectiveCamera.for_description(sd, W, H))
    return _cache[("film", name)]


def _frame(mts, name, integrator, lean, drive):
    sd, scene, cam = _film_scene(mts, name)
    drive = dict(drive)
    max_paths = drive.pop("max_paths", 0)
    if integrator == "path":
        it = mts.MIPathTracer(maxDepth=6)
    else:
        it = mts.MIDirectIntegrator(luminaireSamples=integrator[1], bsdfSamples=integrator[2])
    it.preprocess(scene, cam, sampler="ldsampler", sampleCount=SPP, seed=0x5EED)
    it.set_tuning(lean_closest=lean, **drive)
    it.set_options(max_paths=max_paths)
    it.clear_film()
    assert it.render()
    out = it.film().copy(), it.bin_entries(), it.stats()
    it.close()
    return out


@gpu
@pytest.mark.parametrize("integrator", ["path", ("direct", 1, 1), ("direct", 2, 2)], ids=["path", "direct", "direct_rounds"])
@pytest.mark.parametrize("name", list(FILM_SCENES))
def test_films_and_bins_are_the_same_bytes(gpu_lib, mts, name, integrator):
    ref_film, ref_bins, ref_st = _frame(mts, name, integrator, 0, DRIVES[0])
    assert ref_film[..., :3].max() > 0 and sum(ref_bins) > 0 and ref_st["rays_redone"] == 0
    redone = []
    for drive in DRIVES:
        film, bins, st = _frame(mts, name, integrator, 7, drive)
        assert film.tobytes() == ref_film.tobytes(), (name, integrator, drive)
        assert bins == ref_bins, (name, integrator, drive)
        assert st["rays_closest"] == ref_st["rays_closest"] and st["rays_shadow"] == ref_st["rays_shadow"]
        if drive.get("test_retry"):
            assert st["bin_overflow_retries"] > 0
        redone.append(st["rays_redone"])
    print(name, integrator, "redone per drive", redone, "of", ref_st["rays_closest"])
    if name == "doubled":
        assert min(redone) > 0


@gpu
def test_the_knob_is_range_checked(gpu_lib, mts):
    it = mts.MIPathTracer(maxDepth=2)
    L = mts.lib()
    assert L.mtsgpu_set_tuning(it._ctx, b"lean_closest", 8) != 0
    assert L.mtsgpu_set_tuning(it._ctx, b"lean_closest", -1) != 0
    assert L.mtsgpu_set_tuning(it._ctx, b"lean_closest", 7) == 0
    it.close()
