"""The non-delta luminaires on the device: mtsgpu_scene_lum_eval -- sample_luminaire, pdf_luminaire and background_le as
k_shade calls them, on the tables mtsgpu_upload_scene packed -- against the binary64 restatement (tests/ref64_lum.py) through
the check the oracle goes through on the CPU (tests/lum_cases.py, tests/test_lum_truth.py); what the hook refuses; and three
Lambertian floors lit by a sphere, a constant background and an envmap, rendered with luminaire samples only, BSDF samples
only and both under MIS, against closed forms."""
import numpy as np
import pytest

import lum_cases
import ref64_lum as R

pytestmark = pytest.mark.gpu
N_SCENES = 9


@pytest.fixture(scope="module")
def scenes(mts):
    s = lum_cases.scenes(mts)
    assert len(s) == N_SCENES
    return s


def _upload(mts, sd):
    scene = mts.Scene(sd)
    it = mts.MIPathTracer(maxDepth=2)
    it.preprocess(scene, mts.PerspectiveCamera.for_description(sd, 8, 8), sampler="independent", sampleCount=1, seed=1)
    return scene, it


# --- 1. the read-out hook against binary64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(N_SCENES))
def test_device_luminaires_against_binary64(gpu_lib, mts, scenes, k):
    name, sd = scenes[k]
    scene, it = _upload(mts, sd)
    failures, report = lum_cases.check_scene(it.scene_lum_eval, scene.arrays(), 100 + k)
    print("%s\n%s" % (name, lum_cases.format_report(report)))
    assert not failures, name + "\n" + "\n".join(failures)


def test_hook_refusals(gpu_lib, mts, scenes):
    by_name = dict(scenes)
    q = np.zeros((2, 16), dtype=np.float32)
    q[:, 9:12] = (0, 1, 0)
    fresh = mts.MIPathTracer(maxDepth=2)
    for op in range(3):
        with pytest.raises(mts.MtsGpuError, match=r"before mtsgpu_upload_scene.*code -5"):
            fresh.scene_lum_eval(op, q)
    scene, it = _upload(mts, by_name["five: quad, spot, sphere, point, envmap"])
    for lum in (5, 1000, -1, 0.5, np.nan, np.inf):
        q[1, 12] = lum
        with pytest.raises(mts.MtsGpuError, match=r"record 1: luminaire index .* out of range.*code -1"):
            it.scene_lum_eval(1, q)
    for lum in (1, 3):                          # the spot and the point light
        q[1, 12] = lum
        with pytest.raises(mts.MtsGpuError, match=r"record 1: luminaire %d is a delta luminaire.*code -1" % lum):
            it.scene_lum_eval(1, q)
    q[:, 12] = 4
    out = it.scene_lum_eval(1, q)
    assert out.shape == (2, 16) and (out[:, 0] > 0).all() and (out[:, 1:] == 0).all()
    with pytest.raises(mts.MtsGpuError, match=r"operation.*code -1"):
        it.scene_lum_eval(3, q)
    assert it.scene_lum_eval(0, q[:0]).shape == (0, 16)
    # the count is refused before a record is read, so the two records' memory stands in for 2^24 + 1 of them
    A, out = mts.abi, np.zeros((2, 16), np.float32)
    for op in range(3):
        with pytest.raises(mts.MtsGpuError, match=r"at most 2\^24 query records per call.*code -1"):
            it._chk(mts.lib().mtsgpu_scene_lum_eval(it._ctx, op, (1 << 24) + 1, A.ptr(q, A.f32p), A.ptr(out, A.f32p)), "scene_lum_eval")
    scene, it = _upload(mts, by_name["quad"])
    with pytest.raises(mts.MtsGpuError, match=r"no background luminaire.*code -1"):
        it.scene_lum_eval(2, q)
    assert np.isfinite(it.scene_lum_eval(0, q)).all()


# --- 2. three floors against closed forms ----------------------------------------------------------------------------
# The harness of test_gpu_ward_composite.py::test_area_light_floor_against_quadrature: an 8 x 8 film under the box filter (every
# pixel the mean of its own samples), an orthographic camera that sees the floor only, the standard error measured over the
# seeds.  Its sample counts are kept: the precondition se < 0.1 E holds for all nine cases with them.
W = H = 8
SPP, SEEDS = 4096, 64
RHO = 0.5
SPHERE_C, SPHERE_R, SPHERE_LE = (-0.6, 1.5, -0.4), 0.3, 8.0
CONST_LE = (0.7, 0.8, 0.9)
STRATEGIES = ["direct, luminaire samples only", "direct, BSDF samples only", "path (MIS)"]


def small_env_bitmap():
    """16 x 8, dim and smooth but for one bright 3 x 2 block in the upper hemisphere"""
    y, x = np.mgrid[0:8, 0:16].astype(np.float64)
    img = np.stack([0.3 + 0.1 * np.cos(x / 16 * 2 * np.pi), 0.3 + 0.02 * y, 0.25 + 0.1 * np.sin(x / 16 * 2 * np.pi) ** 2], axis=-1)
    img[1:3, 5:8] = (6.0, 5.0, 4.0)
    return img.astype(np.float32)


def _floor_scene(mts, kind):
    sd = mts.scenes.SceneDescription("lum floor " + kind)
    pos, tri = mts.scenes._quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), (0, 1, 0))
    sd.add_mesh(pos, tri, bsdf=sd.lambertian(RHO), face_normals=True)
    if kind == "sphere":
        sd.add_sphere(SPHERE_C, SPHERE_R, bsdf=sd.lambertian(0.0), lum=sd.add_lum(mts.abi.LUM_AREA, [SPHERE_LE] * 3))
    elif kind == "constant":
        sd.add_lum(mts.abi.LUM_CONSTANT, list(CONST_LE))
    else:
        sd.envmap(small_env_bitmap(), 0.8, to_world=lum_cases._rot([0.2, 1.0, 0.1], 0.6))
    sd.camera = dict(origin=(1.2, 2.0, 0.9), target=(0.05, 0.0, -0.1), up=(0.0, 1.0, 0.0), ortho_scale=(0.4, 0.4))
    return sd


def _floor_points(cam, sub):
    """sub x sub midpoints of every pixel's footprint on the floor y = 0 -> [H][W][sub * sub][3], binary64"""
    r2c = np.array(list(cam.raster_to_camera), dtype=np.float64).reshape(4, 4)
    c2w = np.array(list(cam.camera_to_world), dtype=np.float64).reshape(4, 4)
    u = (np.arange(sub) + 0.5) / sub
    x = (np.arange(cam.width)[None, :, None, None] + u[None, None, :, None] + 0 * u[None, None, None, :])
    y = (np.arange(cam.height)[:, None, None, None] + 0 * u[None, None, :, None] + u[None, None, None, :])
    x, y = np.broadcast_arrays(x, y)
    ras = np.stack([x, y, 0 * x, 1 + 0 * x], axis=-1).reshape(-1, 4)
    pc = ras @ r2c.T; pc = pc[:, :3] / pc[:, 3:4]
    o = np.concatenate([pc, np.ones((len(pc), 1))], axis=1) @ c2w.T
    o = o[:, :3] / o[:, 3:4]
    d = c2w[:3, :3] @ np.array([0.0, 0.0, 1.0]); d /= np.linalg.norm(d)
    p = o + (-o[:, 1] / d[1])[:, None] * d
    return p.reshape(cam.height, cam.width, sub * sub, 3)


def _expected_sphere(cam, sub):
    """rho Le (R / d)^2 cos(theta): the radiance a Lambertian floor point reflects under a uniform sphere wholly above its
    horizon (its projected solid angle is pi (R / d)^2 cos(theta), theta the angle of the centre from the normal), averaged
    over the footprint"""
    p = _floor_points(cam, sub)
    v = np.asarray(SPHERE_C) - p
    d2 = (v * v).sum(axis=-1)
    assert (v[..., 1] > SPHERE_R * 1.01).all()                    # wholly above the horizon
    L = RHO * SPHERE_LE * SPHERE_R ** 2 / d2 * (v[..., 1] / np.sqrt(d2))
    return L.mean(axis=2)[..., None] * np.ones(3)


def _expected_envmap(A, n):
    """(rho / pi) times the integral of Le(w) cos(theta) over the upper hemisphere, midpoint rule on n x 4n cells of (theta,
    phi) in world space, Le from the restatement"""
    T = R.tables(A)
    th = (np.arange(n) + 0.5) / n * (np.pi / 2)
    ph = (np.arange(4 * n) + 0.5) / (4 * n) * 2 * np.pi
    th, ph = np.meshgrid(th, ph, indexing="ij")
    w = np.stack([np.sin(th) * np.cos(ph), np.cos(th), np.sin(th) * np.sin(ph)], axis=-1).reshape(-1, 3)      # normal +y
    le, _, _ = R.background_le(T, w.astype(np.float32))
    weight = (np.cos(th) * np.sin(th)).reshape(-1, 1) * (np.pi / 2 / n) * (2 * np.pi / (4 * n))
    return RHO / np.pi * (le * weight).sum(axis=0)


@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("kind", ["sphere", "constant", "envmap"])
def test_lit_floor_against_closed_form(gpu_lib, mts, kind, strategy):
    """One expected value for the three strategies: a luminaire whose sample(), pdf() or Le() is wrong in a way its own
    round trip hides (a density that does not integrate to 1, a value not matching the density) shifts one of them.
    Accepted within 4 measured standard errors plus the quadrature's own bounded error."""
    sd = _floor_scene(mts, kind)
    scene = mts.Scene(sd)
    cam = mts.PerspectiveCamera.for_description(sd, W, H)
    films = []
    for seed in range(SEEDS):
        it = {STRATEGIES[0]: lambda: mts.MIDirectIntegrator(1, 0), STRATEGIES[1]: lambda: mts.MIDirectIntegrator(0, 1),
              STRATEGIES[2]: lambda: mts.MIPathTracer(maxDepth=2)}[strategy]()
        it.preprocess(scene, cam, sampler="independent", sampleCount=SPP, seed=2000 + seed)
        assert it.render()
        films.append(mts.develop(it.film())[..., 0:3].astype(np.float64))
    films = np.stack(films)
    assert np.isfinite(films).all()
    mean, se = films.mean(axis=0), films.std(axis=0, ddof=1) / np.sqrt(SEEDS)
    if kind == "sphere":
        E = _expected_sphere(cam.c, 5)
        qerr = np.abs(E - _expected_sphere(cam.c, 9))
    elif kind == "constant":
        E = np.ones((H, W, 3)) * RHO * np.asarray(CONST_LE, dtype=np.float32).astype(np.float64)
        qerr = np.zeros_like(E)
    else:
        A = scene.arrays()
        e1, e2 = _expected_envmap(A, 96), _expected_envmap(A, 192)
        E = np.ones((H, W, 3)) * e2
        qerr = np.ones((H, W, 3)) * 2 * np.abs(e2 - e1)           # the midpoint rule's error falls with the step: twice the last change bounds it
    dev = np.abs(mean - E)
    print("%s, %s: expected %.4g..%.4g, standard error relative %.3g..%.3g, quadrature error <= %.3g, worst deviation %.3g = %.2f standard errors"
          % (kind, strategy, E.min(), E.max(), (se / E).min(), (se / E).max(), qerr.max(), dev.max(), (np.maximum(dev - qerr, 0) / se).max()))
    if kind == "constant" and strategy == STRATEGIES[1]:
        # Every BSDF sample escapes to the same radiance, f cos / pdf = rho: the estimator has no variance, there is no standard
        # error to measure, and what is left is binary32 rounding.  A sample's weight carries a few roundings (say 8 units of
        # 2^-24); a pixel's sum of SPP such terms, in whatever order the film adds them, is off by at most (SPP - 1) 2^-24 of
        # the sum (the sum of the weights, SPP ones, is exact); the division adds one more.
        assert (dev <= (SPP + 8) * 2.0 ** -24 * E).all(), float((dev / E).max())
        return
    assert (E > 0).all() and (se > 0).all() and (se < 0.1 * E).all(), "the error bars must be far smaller than the value they guard"
    bad = dev > 4 * se + qerr
    assert not bad.any(), (kind, strategy, np.argwhere(bad)[0], mean[bad][0], E[bad][0], se[bad][0])
