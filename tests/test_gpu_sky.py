"""The sky luminaire on the device: mtsgpu_lum_eval against the binary64 restatement (tests/ref64_sky.py), background pixels
and a sky-lit floor inside frames, one film across the bounce drivers, tile parts and a device group, and what only
mtsgpu_upload_scene can refuse.  The CPU side (case list, ambiguity cap, host configure) is tests/test_sky.py."""
import numpy as np
import pytest

import closed_forms as cf
import ref64_sky
import sky_cases

pytestmark = pytest.mark.gpu
F = np.float32
SKY = 7


@pytest.fixture(scope="module")
def device(gpu_lib, mts):
    return mts.MIPathTracer(maxDepth=2)


# --- 1. the read-out hook against binary64 ---------------------------------------------------------------------------
def check_le(name, P, dirs, classes, got):
    """failures of Le read-outs `got` [n][3] against the restatement, and the worst ratio seen"""
    failures = []
    val, cond, amb = ref64_sky.le(P, dirs)
    cf._non_finite(failures, "%s Le" % name, got, val)
    zero = (val == 0).all(axis=1) & ~amb
    bad = zero & (got != 0).any(axis=1)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        failures.append("%s: %d records not exactly black below the clipped horizon, e.g. %s -> %s" % (name, bad.sum(), dirs[i].tolist(), got[i].tolist()))
    report = {}
    sel = ~zero & ~amb
    r = cf._check_values(report, "Le", got, val, cond, sel)
    if (r > cf.K_VALUE).any():
        i = int(np.argmax(r))
        failures.append("%s: worst ratio %.3g > %g at %s: got %s ref %s cond %.3g" % (name, r[i], cf.K_VALUE, dirs[i].tolist(), got[i].tolist(), val[i].tolist(), cond[i]))
    # on the horizon of a clipped sky binary32 may take either branch: exactly black, or the value of the unclipped sky
    if P[2] != 0:
        P_open = np.array(P, dtype=np.float32); P_open[2] = 0
        v2, c2, a2 = ref64_sky.le(P_open, dirs)
        edge = amb & ~a2
        black = (got == 0).all(axis=1)
        r2 = cf._check_values({}, "Le", got, v2, c2, edge & ~black)
        if (r2 > cf.K_VALUE).any():
            i = int(np.argmax(r2))
            failures.append("%s: on the horizon neither black nor the sky's value at %s: got %s ref %s" % (name, dirs[i].tolist(), got[i].tolist(), v2[i].tolist()))
    return failures, report["Le"][0]


@pytest.mark.parametrize("k", range(12))
def test_device_sky_against_binary64(device, mts, k):
    name, P = sky_cases.parameter_sets(mts)[k]
    rng = np.random.RandomState(900 + k)
    dirs, classes = sky_cases.directions(P, rng)
    got = device.lum_eval(SKY, P, 0, dirs)
    failures, worst = check_le(name, P, dirs, classes, got[:, 0:3])
    # --- sample(p, s) and pdf ---
    s = cf.sample_inputs(rng, 4000)
    p = sky_cases.sample_points(rng, len(s))
    out = device.lum_eval(SKY, P, 1, p, s)
    r = ref64_sky.sample(P, p, s)
    gd, gpdf, gval, gend = out[:, 0:3], out[:, 3], out[:, 4:7], out[:, 8:11]
    if not np.isfinite(out).all():
        failures.append("%s sample: %d non-finite outputs" % (name, (~np.isfinite(out)).sum()))
    pdf32 = ref64_sky.pdf()
    if not (gpdf.view(np.uint32) == np.float32(pdf32).view(np.uint32)).all():
        failures.append("%s sample: pdf is not 1 / (4 pi) in binary32" % name)
    if not (device.lum_eval(SKY, P, 2, p[:64], gd[:64])[:, 0].view(np.uint32) == np.float32(pdf32).view(np.uint32)).all():
        failures.append("%s pdf: not 1 / (4 pi) in binary32" % name)
    ok = ~r.amb
    derr = np.where(ok, np.abs(gd - r.d).max(axis=1) / (cf.EPS * np.where(ok, r.dir_cond, 1)), 0.0)
    if (derr > cf.K_DIR).any():
        i = int(np.argmax(derr))
        failures.append("%s sample: direction off by %.3g x eps x cond at s %s: got %s ref %s" % (name, derr[i], s[i].tolist(), gd[i].tolist(), r.d[i].tolist()))
    # the end point p - d (2 r): d's allowance carried through, plus the roundings of the product and the difference
    end_tol = cf.EPS * (cf.K_DIR * r.dir_cond[:, None] * 2 * float(P[6]) + cf.K_VALUE * r.end_err)
    if (ok[:, None] & (np.abs(gend - r.end) > end_tol)).any():
        i = int(np.argmax((np.abs(gend - r.end) / end_tol).max(axis=1) * ok))
        failures.append("%s sample: shadow-ray end point %s, ref %s" % (name, gend[i].tolist(), r.end[i].tolist()))
    # value == Le(-d) of the hook, bit for bit, at the hook's own d
    again = device.lum_eval(SKY, P, 0, -gd)[:, 0:3]
    if not np.array_equal(again.view(np.uint32), gval.view(np.uint32)):
        failures.append("%s sample: value differs from Le(-d) on %d records" % (name, (again != gval).any(axis=1).sum()))
    print("%s: worst Le ratio %.3g of %g, worst direction %.3g of %g" % (name, worst, cf.K_VALUE, derr.max(), cf.K_DIR))
    assert not failures, "\n".join(failures)


def test_the_check_sees_a_nan(device, mts):
    """self-test: one NaN and one wrong value in otherwise good read-outs fail the check"""
    name, P = sky_cases.parameter_sets(mts)[3]
    dirs, classes = sky_cases.directions(P, np.random.RandomState(1))
    got = device.lum_eval(SKY, P, 0, dirs)[:, 0:3]
    assert not check_le(name, P, dirs, classes, got)[0]
    val, cond, amb = ref64_sky.le(P, dirs)
    i = int(np.nonzero(~amb & (val > 0).all(axis=1))[0][5])
    bad = got.copy(); bad[i, 1] = np.nan
    assert any("non-finite" in f for f in check_le(name, P, dirs, classes, bad)[0])
    bad = got.copy(); bad[i, 2] *= F(1.05)
    assert any("worst ratio" in f for f in check_le(name, P, dirs, classes, bad)[0])
    j = int(np.nonzero((val == 0).all(axis=1) & ~amb)[0][0])
    bad = got.copy(); bad[j, 0] = F(1e-30)
    assert any("not exactly black" in f for f in check_le(name, P, dirs, classes, bad)[0])


def test_hook_refusals(device, mts):
    name, P = sky_cases.parameter_sets(mts)[1]
    d = np.float32([[0, 1, 0]])
    for t in (0, 1, 2, 3, 4, 5, 6, 8):
        with pytest.raises(mts.MtsGpuError, match="not served"):
            device.lum_eval(t, P, 0, d)
    with pytest.raises(mts.MtsGpuError, match="operation"):
        device.lum_eval(SKY, P, 3, d)
    Q = P.copy(); Q[6] = 0
    with pytest.raises(mts.MtsGpuError, match="positive radius"):
        device.lum_eval(SKY, Q, 0, d)
    # the count is refused before a record is read, so one record's memory stands in for 2^24 + 1 of them
    A, block, q, out = mts.abi, np.zeros(mts.abi.LUM_NPARAMS, np.float32), np.zeros(6, np.float32), np.zeros(12, np.float32)
    block[:len(P)] = P
    with pytest.raises(mts.MtsGpuError, match=r"at most 2\^24 query records per call.*code -1"):
        device._chk(mts.lib().mtsgpu_lum_eval(device._ctx, SKY, A.ptr(block, A.f32p), 0, (1 << 24) + 1, A.ptr(q, A.f32p), A.ptr(out, A.f32p)), "lum_eval")


# --- 2. background pixels --------------------------------------------------------------------------------------------
BG_W, BG_H, BG_SPP, BG_SUB = 32, 24, 4, 9
OCC = ((-0.3, 0.8, -2.0), (0.6, 0, 0), (0, 0.5, 0))          # a small quad in front of the camera


def _bg_scene(mts, **kw):
    sd = mts.scenes.SceneDescription("sky background")
    pos, tri = mts.scenes._quad(OCC[0], OCC[1], OCC[2], (0, 0, 1))
    sd.add_mesh(pos, tri, bsdf=sd.lambertian(0.5), face_normals=True)
    sd.camera = dict(origin=(0.0, 1.0, 3.0), target=(0.2, 1.15, 0.0), up=(0.0, 1.0, 0.0), fov=60.0)
    l = sd.sky(**kw)
    return sd, l


def _pixel_directions(cam, sub):
    r2c = np.array(list(cam.raster_to_camera), dtype=np.float64).reshape(4, 4)
    c2w = np.array(list(cam.camera_to_world), dtype=np.float64).reshape(4, 4)
    u = np.linspace(0.0, 1.0, sub)
    x = (np.arange(cam.width)[None, :, None, None] + u[None, None, :, None] + 0 * u[None, None, None, :])
    y = (np.arange(cam.height)[:, None, None, None] + 0 * u[None, None, :, None] + u[None, None, None, :])
    x, y = np.broadcast_arrays(x, y)
    ras = np.stack([x, y, 0 * x, 1 + 0 * x], axis=-1).reshape(-1, 4)
    pc = ras @ r2c.T; pc = pc[:, :3] / pc[:, 3:4]
    d = pc @ c2w[:3, :3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d.reshape(cam.height, cam.width, sub * sub, 3), c2w[:3, 3]


@pytest.mark.parametrize("integ", ["path", "direct"])
@pytest.mark.parametrize("kw", [dict(sun_direction=(0.3, 0.2, 0.8), turbidity=3.0),
                                dict(sun_direction=(-0.6, 0.5, 0.15), turbidity=6.0, sky_scale=0.5),
                                dict(sun_direction=(0.1, 0.3, 0.5), turbidity=4.0, clip_below_horizon=False, to_world=sky_cases._rot((0.2, 0.1, 1.0), 25.0))])
def test_background_pixels(gpu_lib, mts, integ, kw):
    """a camera ray that leaves the scene returns Le(ray.d): every pixel whose footprint sees only sky lies within the
    restatement's range over the footprint (closed_forms' rule for the delta-light renders), pixels below a clipped horizon
    are exactly 0"""
    sd, l = _bg_scene(mts, **kw)
    scene = mts.Scene(sd)
    P = scene.arrays()["lum_params"][l]
    cam = mts.PerspectiveCamera.for_description(sd, BG_W, BG_H)
    it = mts.MIPathTracer(maxDepth=3) if integ == "path" else mts.MIDirectIntegrator(1, 1)
    it.preprocess(scene, cam, sampler="independent", sampleCount=BG_SPP, seed=5)
    it.set_rfilter("box")
    assert it.render()
    img = mts.develop(it.film()).astype(np.float64)
    d, o = _pixel_directions(cam.c, BG_SUB)
    # pixels that may see the occluder: any footprint direction that meets its plane z = -2 inside the quad grown by a margin
    t = (OCC[0][2] - o[2]) / d[..., 2]
    hx, hy = o[0] + t * d[..., 0], o[1] + t * d[..., 1]
    m = 0.05
    hits = (t > 0) & (hx > OCC[0][0] - m) & (hx < OCC[0][0] + OCC[1][0] + m) & (hy > OCC[0][1] - m) & (hy < OCC[0][1] + OCC[2][1] + m)
    sky_only = ~hits.any(axis=2)
    assert sky_only.sum() > 0.7 * BG_W * BG_H and (~sky_only).sum() >= 4
    val, cond, amb = ref64_sky.le(P, d.reshape(-1, 3).astype(np.float32))
    L = val.reshape(BG_H, BG_W, -1, 3)
    lo, hi = L.min(axis=2), L.max(axis=2)
    tol = cf.REL_TOL * np.maximum(hi, 1e-30) + cf.GRID_SLACK * (hi - lo)
    assert np.isfinite(img).all()
    bad = sky_only[..., None] & ~((img >= lo - tol) & (img <= hi + tol))
    assert not bad.any(), (np.argwhere(bad)[0], img[bad][0], lo[bad][0], hi[bad][0], int(bad.sum()))
    black = sky_only & (hi.max(axis=2) == 0)
    zz = black.copy()
    zz[1:] &= black[:-1]; zz[:-1] &= black[1:]
    if kw.get("clip_below_horizon", True):
        assert zz.sum() > 0.2 * BG_W * BG_H
    assert (img[zz] == 0).all()
    assert (img[sky_only & (lo.min(axis=2) > 0)] > 0).all()


# --- 3. a sky-lit Lambertian floor against quadrature ----------------------------------------------------------------
# 4 x 4 blocks, 64 seeds: 16 independent comparisons per render set (the channels move together), so that 4 standard errors of a
# deviation estimated from 64 seeds (Student's t, 63 degrees of freedom: 2e-4 per comparison) stay a rare event over the 96 of them
FL_W = FL_H = 4
FL_SPP, FL_SEEDS = 4096, 64
ALBEDO = 0.6
FLOOR_SKIES = [dict(sun_direction=(0.3, 0.2, 0.8), turbidity=3.0),
               dict(sun_direction=(-0.4, 0.5, 0.35), turbidity=5.0, sky_scale=0.5, to_world=sky_cases._rot((0.3, 0.1, 1.0), 35.0))]


def _irradiance(P, n):
    """binary64 midpoint quadrature of the integral of Le(w) cos(theta) dw over the hemisphere around the world's +y, n x 2n
    cells in (cos theta, phi): dw = d(cos theta) d(phi)"""
    mu = (np.arange(n) + 0.5) / n
    ph = (np.arange(2 * n) + 0.5) / (2 * n) * 2 * np.pi
    mu, ph = np.meshgrid(mu, ph, indexing="ij")
    st = np.sqrt(1 - mu * mu)
    w = np.stack([st * np.cos(ph), mu, st * np.sin(ph)], axis=-1).reshape(-1, 3)
    val, _, _ = ref64_sky.le(P, w.astype(np.float32))
    return (val * mu.reshape(-1, 1)).sum(axis=0) * (1.0 / n) * (2 * np.pi / (2 * n))


@pytest.mark.parametrize("strategy", ["direct, luminaire samples only", "direct, BSDF samples only", "path (MIS)"])
@pytest.mark.parametrize("k", range(2))
def test_sky_lit_floor_against_quadrature(gpu_lib, mts, k, strategy):
    """the procedure of test_area_light_floor_against_quadrature: one floor, three strategies, one expected value -- the
    outgoing radiance albedo / pi x the irradiance of the sky, the same at every point of a floor nothing shadows.  A block
    mean is accepted within 4 measured standard errors (over FL_SEEDS seeds) plus the quadrature's own error, bounded by
    doubling the grid; binary32 directions fed to the restatement add 2^-24 relative, far below both."""
    sd = mts.scenes.SceneDescription("sky floor")
    pos, tri = mts.scenes._quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), (0, 1, 0))
    sd.add_mesh(pos, tri, bsdf=sd.lambertian(ALBEDO), face_normals=True)
    sd.camera = dict(origin=(1.2, 2.0, 0.9), target=(0.05, 0.0, -0.1), up=(0.0, 1.0, 0.0), ortho_scale=(0.4, 0.4))
    l = sd.sky(**FLOOR_SKIES[k])
    scene = mts.Scene(sd)
    P = scene.arrays()["lum_params"][l]
    cam = mts.PerspectiveCamera.for_description(sd, FL_W, FL_H)
    films = []
    for seed in range(FL_SEEDS):
        it = {"direct, luminaire samples only": lambda: mts.MIDirectIntegrator(1, 0), "direct, BSDF samples only": lambda: mts.MIDirectIntegrator(0, 1),
              "path (MIS)": lambda: mts.MIPathTracer(maxDepth=2)}[strategy]()
        it.preprocess(scene, cam, sampler="independent", sampleCount=FL_SPP, seed=3000 + seed)
        assert it.render()
        films.append(mts.develop(it.film()).astype(np.float64))
    films = np.stack(films)
    assert np.isfinite(films).all()
    mean, se = films.mean(axis=0), films.std(axis=0, ddof=1) / np.sqrt(FL_SEEDS)
    E1, E2 = _irradiance(P, 192), _irradiance(P, 384)
    want = float(np.float32(ALBEDO)) / np.pi * E2
    qerr = float(np.float32(ALBEDO)) / np.pi * np.abs(E2 - E1) * 2
    dev = np.abs(mean - want)
    print("sky %d, %s: expected %s, standard error %.3g..%.3g, quadrature error <= %s, worst deviation %.3g = %.2f standard errors"
          % (k, strategy, want, se.min(), se.max(), qerr, dev.max(), (np.maximum(dev - qerr, 0) / se).max()))
    assert (want > 0).all() and (se > 0).all() and (se < 0.1 * want).all() and (qerr < 0.01 * want).all()
    bad = dev > 4 * se + qerr
    assert not bad.any(), (k, strategy, np.argwhere(bad)[0], mean[bad][0], se[bad][0])


# --- 4. one film -----------------------------------------------------------------------------------------------------
def _mixed_scene(mts):
    """an open box (no ceiling, no front) under a rotated sky: lambertian walls, a Ward floor, a glass and a rough-metal sphere,
    a quad emitter"""
    S = mts.scenes
    sd = S.SceneDescription("sky mixed")
    white = sd.lambertian(0.6)
    floor = sd.ward(0.15, 0.15, rd=(0.5, 0.4, 0.3), rs=0.4, kd=0.6, ks=0.4, model="ward-duer")
    for args, b in ((((-1, 0, -1), (2, 0, 0), (0, 0, 2), (0, 1, 0)), floor), (((-1, 0, -1), (2, 0, 0), (0, 2, 0), (0, 0, 1)), white),
                    (((-1, 0, -1), (0, 0, 2), (0, 1.2, 0), (1, 0, 0)), white)):
        pos, tri = S._quad(*args)
        sd.add_mesh(pos, tri, bsdf=b, face_normals=True)
    sd.add_sphere((-0.4, 0.35, -0.2), 0.35, bsdf=sd.roughmetal(0.2))
    sd.add_sphere((0.45, 0.3, 0.3), 0.3, bsdf=sd.dielectric())
    lum = sd.add_lum(mts.abi.LUM_AREA, [6.0, 5.5, 4.5])
    pos, tri = S._quad((-0.3, 1.6, -0.3), (0.6, 0, 0), (0, 0, 0.6), (0, -1, 0))
    sd.add_mesh(pos, tri, bsdf=sd.lambertian(0.0), lum=lum, face_normals=True)
    sd.sky(sun_direction=(0.5, 0.3, 0.4), turbidity=3.5, sky_scale=0.2, to_world=sky_cases._rot((0.0, 1.0, 0.0), 50.0))
    sd.camera = dict(origin=(0.3, 1.2, 3.4), target=(0.0, 0.8, 0.0), up=(0.0, 1.0, 0.0), fov=45.0)
    return sd


@pytest.mark.parametrize("integ", ["path", "direct"])
def test_drivers_tile_parts_and_group_give_one_film(gpu_lib, mts, integ):
    sd = _mixed_scene(mts)
    scene = mts.Scene(sd)
    Wd, Ht, spp = 96, 64, 8
    cam = mts.PerspectiveCamera.for_description(sd, Wd, Ht)

    def render(drive, part=0, n_parts=1):
        it = mts.MIPathTracer(maxDepth=6) if integ == "path" else mts.MIDirectIntegrator(1, 1)
        it.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=11)
        if drive == 1: it.set_tuning(sync_free=0)
        elif drive == 2: it.set_tuning(sync_free=0); it.set_options(max_paths=spp * (Wd * Ht // 3 + 1))
        elif drive == 3: it.set_tuning(sync_free=1, shade_fused=0)
        if n_parts > 1:
            it.set_tiles(32, part, n_parts)
        assert it.render()
        return it.film()
    base = render(0)
    img = mts.develop(base)
    assert np.isfinite(base).all() and (img > 0).any()
    assert (img[:8].min(axis=2) > 0).mean() > 0.5, "the top rows of the frame look at the sky"
    for drive in (1, 2, 3):
        other = render(drive)
        assert np.array_equal(base.view(np.uint32), other.view(np.uint32)), "drive %d differs from the device-driven frame" % drive
    for n_parts in (2, 5):
        total = sum(render(0, part, n_parts) for part in range(n_parts))
        assert np.array_equal(base.view(np.uint32), total.view(np.uint32)), "%d tile parts do not add up to the frame" % n_parts
    g = mts.DeviceGroup([0, 0], maxDepth=6)
    g.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=11)
    if integ == "direct":
        # the group has no call of its own for the direct integrator: it is set on every member, as the plugin does
        for i in range(len(g)):
            assert mts.lib().mtsgpu_set_direct_integrator(g.member(i), 1, 1) == 0
    assert g.render(block_size=32, ordered_reduce=True)
    assert np.array_equal(base.view(np.uint32), g.film().view(np.uint32)), "the two-member group's film differs"
    g.close()


# --- 5. what only mtsgpu_upload_scene can refuse ---------------------------------------------------------------------
def test_upload_rejections(gpu_lib, mts):
    def attempt(patch, background=None):
        sd = mts.scenes.SceneDescription("upload")
        pos, tri = mts.scenes._quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), (0, 1, 0))
        sd.add_mesh(pos, tri, bsdf=sd.lambertian(0.5), face_normals=True)
        l = sd.sky(sun_direction=(0.2, 0.1, 0.9), turbidity=0.0, b=0.0)
        scene = mts.Scene(sd)
        sc = scene.ptr.contents
        Pv = np.ctypeslib.as_array(sc.lum_params, shape=(sc.n_lums * 32,))
        for i, v in patch.items():
            Pv[32 * l + i] = v
        if background is not None:
            sc.background_lum = background
        it = mts.MIPathTracer(maxDepth=2)
        rc = mts.lib().mtsgpu_upload_scene(it._ctx, scene.ptr)
        msg = mts.lib().mtsgpu_last_error(it._ctx).decode()
        return rc, msg
    assert attempt({})[0] == 0
    a = F(1.0 / 1.46303)
    cand = [c for c in (a, np.nextafter(a, F(0)), np.nextafter(a, F(1))) if F(np.float64(-1.46303) * np.float64(c)) == F(-1)][0]
    for patch, bg, words in (({}, -1, "must be the background luminaire"), ({1: np.nan}, None, "non-finite"), ({12: np.inf}, None, "non-finite"),
                             ({6: 0.0}, None, "positive radius"), ({6: -1.0}, None, "positive radius"),
                             ({18: cand}, None, "Perez denominator of the sky is zero"), ({1: 1e20}, None, "non-finite derived")):
        rc, msg = attempt(patch, bg)
        assert rc == -1 and words in msg, (patch, rc, msg)
