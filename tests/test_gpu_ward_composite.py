"""Ward and Composite on the MI355X: the device's f / pdf / sample (the code k_shade runs, read out through
mtsgpu_bsdf_eval and mtsgpu_bsdf_eval_table) against tests/ref64_ward.py with the comparison and the bounds of
closed_forms.check_model, the reference's chi-square test, point-lit renders against closed forms (a floor for the isotropic
models, a sphere for the anisotropic one, whose tangent frame comes from dpdu / dpdv), the rejections only
mtsgpu_upload_scene makes, and the four ways of driving the bounces and tile sharding against each other."""
import numpy as np
import pytest

import chisquare_ref
import closed_forms as cf
import ref64
import ward_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device(gpu_lib, mts):
    return mts.MIPathTracer()


def _evaluate(device, sd, index):
    """the device read-out of table entry `index` in the layout chisquare_ref / closed_forms expect; a plain Ward also goes
    through the single-block call, which must agree bit for bit"""
    def evaluate(btype, params, op, wi, aux):
        out = device.bsdf_eval_table(sd.bsdf_type, np.stack(sd.bsdf_params), index, op, wi, aux)
        if (btype & 0xFF) != 9:
            one = device.bsdf_eval(btype, params, op, wi, aux)
            assert np.array_equal(one.view(np.uint32), out.view(np.uint32))
        return out
    return evaluate


# --- 1. f / pdf / sample against the binary64 restatement ------------------------------------------------------------
@pytest.mark.parametrize("k", range(14))
def test_device_ward_composite_against_binary64(device, mts, monkeypatch, k):
    cases, sd = ward_cases.models(mts)
    name, index = cases[k]
    monkeypatch.setattr(cf, "ref64", ward_cases.table_of(sd))          # check_model's comparison, held against this table
    failures, report = cf.check_model(_evaluate(device, sd, index), name, sd.bsdf_type[index], sd.bsdf_params[index],
                                      np.random.RandomState(500 + k))
    print(name, report)
    assert not failures, "\n".join(failures) + "\nworst ratios: %s" % report


def test_device_ward_at_the_singular_samples(device, mts):
    """What the reference yields where Ward::sampleSpecular (ward.cpp:222-246) leaves the smooth part of its map, in
    binary32 as the reference computes.
    sample.x = 0: -log(0) = +inf, the quotient and its root are +inf, atan(+inf) = pi/2, whose binary32 value 1.5707964 lies
    ABOVE pi/2: cos(thetaH) = -4.4e-8, H lies in (just under) the tangent plane and wo = 2 <wi,H> H - wi has
    wo.z = -wi.z - 8.7e-8 <wi,H> < 0, so :242 returns a zero spectrum: the sample fails, f = 0 and pdf = 0.
    sample.y = 1/4: 2 pi sample.y = 1.5707964 is likewise above pi/2, so tan() is -2.3e7, not +inf: phiH = atan(alphaY /
    alphaX * tan) = -pi/2 + 1.5e-8, no pi is added (:225), and H = (sin thetaH * 1.5e-8, -sin thetaH, cos thetaH): the half
    vector points along MINUS t.  sample.y = 3/4: 2 pi sample.y = 4.712389 is above 3 pi / 2, tan() is -8.4e7, phiH = -pi/2
    + pi: H points along PLUS t.  In exact arithmetic both poles would give the opposite sign; the restatement flags them,
    and here the device must do what binary32 does.  thetaH follows from cos^2 phiH = 0, sin^2 phiH = 1:
    tan^2 thetaH = -log(sample.x) alphaY^2."""
    sd = mts.scenes.SceneDescription("poles")
    b = sd.ward(0.1, 0.3, rd=1.0, rs=1.0, kd=0.5, ks=0.5)
    P = sd.bsdf_params[b]
    ssw = float(P[5])
    wi = cf._unit([[0.3, -0.2, 0.9], [0.0, 0.0, 1.0], [-0.5, 0.4, 0.6]])
    out = device.bsdf_eval(8, P, 2, wi, np.tile(np.float32([0.0, 0.3]), (3, 1)))
    assert (out[:, 3] == 0).all() and (out[:, 4:7] == 0).all()
    for sy, sign in ((0.25, -1.0), (0.75, 1.0)):
        sx = 0.3
        out = device.bsdf_eval(8, P, 2, wi, np.tile(np.float32([sx, sy]), (3, 1)))
        th = np.arctan(np.sqrt(-np.log(np.float64(np.float32(sx)) / np.float64(np.float32(ssw))) * float(P[2]) ** 2))
        H = np.array([0.0, sign * np.sin(th), np.cos(th)])
        w = wi.astype(np.float64)
        want = 2 * (w @ H)[:, None] * H[None, :] - w
        alive = want[:, 2] > 1e-4
        assert alive.any()
        assert np.abs(out[alive, 0:3] - want[alive]).max() < 2e-6, (sy, out[:, 0:3], want)
        assert (out[alive, 3] > 0).all() and (out[alive, 7].view(np.uint32) == ref64.GLOSSY_REFL).all()


def test_single_block_call_refuses_a_composite(device, mts):
    with pytest.raises(mts.MtsGpuError) as e:
        device.bsdf_eval(9, [1, 1.0, 0], 0, [0, 0, 1], [[0, 0, 1]])
    assert "mtsgpu_bsdf_eval_table" in str(e.value)
    with pytest.raises(mts.MtsGpuError) as e:
        device.bsdf_eval_table([0, 9], np.zeros((2, 16), dtype=np.float32), 1, 0, [0, 0, 1], [[0, 0, 1]])
    assert "between 1 and 7 children" in str(e.value)
    for btype, op in ((0x200, 0), (11, 0), (0, 3), (0, -1)):
        with pytest.raises(mts.MtsGpuError, match="bad BSDF type or operation"):
            device.bsdf_eval(btype, [0.5, 0.5, 0.5], op, [0, 0, 1], [[0, 0, 1]])


def test_both_calls_take_at_most_2_24_records(device, mts):
    """the count is refused before a record is read, so one record's memory stands in for 2^24 + 1 of them"""
    A, L, n = mts.abi, mts.lib(), (1 << 24) + 1
    P, q, out, types = np.full(16, 0.5, np.float32), np.zeros(6, np.float32), np.zeros(8, np.float32), np.zeros(1, np.uint32)
    with pytest.raises(mts.MtsGpuError, match=r"at most 2\^24 query records per call.*code -1"):
        device._chk(L.mtsgpu_bsdf_eval(device._ctx, 0, A.ptr(P, A.f32p), 0, n, A.ptr(q, A.f32p), A.ptr(out, A.f32p)), "bsdf_eval")
    with pytest.raises(mts.MtsGpuError, match=r"at most 2\^24 query records per call.*code -1"):
        device._chk(L.mtsgpu_bsdf_eval_table(device._ctx, 1, A.ptr(types, A.u32p), A.ptr(P, A.f32p), 0, 0, n, A.ptr(q, A.f32p),
                                             A.ptr(out, A.f32p)), "bsdf_eval_table")


# --- 2. the reference's chi-square test on the device ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["test_bsdf.xml ward", "test_bsdf.xml composite"])
def test_device_chi_square(device, mts, name):
    cases, sd = ward_cases.models(mts)
    index = dict(cases)[name]
    failures = chisquare_ref.chi_square(_evaluate(device, sd, index), sd.bsdf_type[index], sd.bsdf_params[index], False,
                                        np.random.RandomState(91))
    assert not failures, failures


# --- 3. renders against closed forms ---------------------------------------------------------------------------------
FLOORS = [
    ("ward floor, type ward", lambda sd: sd.ward(0.2, 0.2, rd=0.5, rs=0.5, kd=0.5, ks=0.5, model="ward")),
    ("ward floor, type ward-duer", lambda sd: sd.ward(0.2, 0.2, rd=0.5, rs=0.5, kd=0.5, ks=0.5, model="ward-duer")),
    ("ward floor, type balanced", lambda sd: sd.ward(0.2, 0.2, rd=0.5, rs=0.5, kd=0.5, ks=0.5, model="balanced")),
    ("composite floor", lambda sd: sd.composite([0.4, 0.6], [sd.lambertian(0.5), sd.ward(0.2, 0.2, rd=0.5, rs=0.5, kd=0.5, ks=0.5)])),
]


def _integrator(mts, integ):
    return mts.MIPathTracer(maxDepth=2) if integ == "path" else mts.MIDirectIntegrator(1, 1)


@pytest.mark.parametrize("integ", ["path", "direct"])
@pytest.mark.parametrize("k", range(4))
def test_point_lit_floor(gpu_lib, mts, monkeypatch, k, integ):
    name, make = FLOORS[k]
    sd = mts.scenes.SceneDescription(name)
    b = make(sd)
    pos, tri = mts.scenes._quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), (0, 1, 0))
    sd.add_mesh(pos, tri, bsdf=b, face_normals=True)
    sd.camera = dict(origin=(1.2, 2.0, 0.9), target=(0.05, 0.0, -0.1), up=(0.0, 1.0, 0.0), ortho_scale=(0.4, 0.4))
    lpos, I = (-0.6, 1.5, -0.4), 6.0
    sd.point_light(lpos, I)
    it = _integrator(mts, integ)
    cam = mts.PerspectiveCamera.for_description(sd, cf.W, cf.H)
    it.preprocess(mts.Scene(sd), cam, sampler="independent", sampleCount=cf.SPP, seed=7)
    assert it.render()
    img = mts.develop(it.film())
    monkeypatch.setattr(cf, "ref64", ward_cases.table_of(sd))
    failures, worst, n_zero, n_lit = cf.check_render(img, cam.c, sd.bsdf_type[b], sd.bsdf_params[b],
                                                     lambda p: ref64.point_light([I] * 3, lpos, p))
    assert not failures, (name, integ, failures, worst)
    assert n_lit > 0


def _sphere_footprints(cam):
    """world points [H][W][SUB*SUB][3] where the orthographic camera's rays through every pixel's sub-grid hit the unit
    sphere at the origin (None if a ray misses it), and the ray direction"""
    r2c = np.array(list(cam.raster_to_camera), dtype=np.float64).reshape(4, 4)
    c2w = np.array(list(cam.camera_to_world), dtype=np.float64).reshape(4, 4)
    u = np.linspace(0.0, 1.0, cf.SUB)
    x = (np.arange(cam.width)[None, :, None, None] + u[None, None, :, None] + 0 * u[None, None, None, :])
    y = (np.arange(cam.height)[:, None, None, None] + 0 * u[None, None, :, None] + u[None, None, None, :])
    x, y = np.broadcast_arrays(x, y)
    ras = np.stack([x, y, 0 * x, 1 + 0 * x], axis=-1).reshape(-1, 4)
    pc = ras @ r2c.T; pc = pc[:, :3] / pc[:, 3:4]
    o = np.concatenate([pc, np.ones((len(pc), 1))], axis=1) @ c2w.T
    o = o[:, :3] / o[:, 3:4]
    d = c2w[:3, :3] @ np.array([0.0, 0.0, 1.0]); d /= np.linalg.norm(d)
    bq = o @ d
    disc = bq * bq - ((o * o).sum(axis=1) - 1.0)
    assert (disc > 0.05).all(), "every footprint must lie on the sphere"
    t = -bq - np.sqrt(disc)
    p = o + t[:, None] * d
    return p.reshape(cam.height, cam.width, cf.SUB * cf.SUB, 3), d


def _sphere_frames(p):
    """Sphere::fillIntersectionRecord (src/shapes/sphere.cpp:136-178) for the unit sphere at the origin with the identity
    transform: s = normalize(dpdu), t = normalize(dpdv), n = p; rows of [n][3][3]"""
    phi = np.arctan2(p[:, 1], p[:, 0])
    theta = np.arccos(np.clip(p[:, 2], -1, 1))
    dpdu = np.stack([-p[:, 1], p[:, 0], 0 * phi], axis=1) * (2 * np.pi)
    dpdv = np.stack([p[:, 2] * np.cos(phi), p[:, 2] * np.sin(phi), -np.sin(theta)], axis=1) * np.pi
    s = dpdu / np.linalg.norm(dpdu, axis=1)[:, None]
    t = dpdv / np.linalg.norm(dpdv, axis=1)[:, None]
    return np.stack([s, t, p / np.linalg.norm(p, axis=1)[:, None]], axis=1)


def _outside(img, L):
    lo, hi = L.min(axis=2), L.max(axis=2)
    tol = cf.REL_TOL * np.maximum(hi, 1e-30) + cf.GRID_SLACK * (hi - lo)
    return ~((img >= lo - tol) & (img <= hi + tol))


@pytest.mark.parametrize("integ", ["path", "direct"])
def test_anisotropic_ward_sphere(gpu_lib, mts, integ):
    """a unit sphere with ward(0.1, 0.3) under a point light: every pixel inside the extremes of the closed form over its
    footprint, with the tangent frame of sphere.cpp:136-178; the closed form of ward(0.3, 0.1) -- the same lobe turned by a
    right angle -- must NOT contain the image, so the test sees which way the tangent points"""
    sd = mts.scenes.SceneDescription("anisotropic sphere")
    b = sd.ward(0.1, 0.3, rd=0.5, rs=0.5, kd=0.5, ks=0.5)
    swapped = sd.ward(0.3, 0.1, rd=0.5, rs=0.5, kd=0.5, ks=0.5)
    sd.add_sphere((0.0, 0.0, 0.0), 1.0, bsdf=b)
    sd.camera = dict(origin=(0.0, 0.0, 3.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), ortho_scale=(0.5, 0.5))
    lpos, I = (3.0, 4.0, 8.0), 60.0        # every footprint faces the light: <p, L> > 1 on |x|, |y| <= 0.5
    sd.point_light(lpos, I)
    it = _integrator(mts, integ)
    cam = mts.PerspectiveCamera.for_description(sd, cf.W, cf.H)
    it.preprocess(mts.Scene(sd), cam, sampler="independent", sampleCount=cf.SPP, seed=7)
    assert it.render()
    img = mts.develop(it.film())
    assert np.isfinite(img).all() and (img > 0).all()
    p, d = _sphere_footprints(cam.c)
    flat = p.reshape(-1, 3)
    ld, val = ref64.point_light([I] * 3, lpos, flat)
    table = ward_cases.table_of(sd)
    wi = np.broadcast_to(-d, flat.shape)
    frames = _sphere_frames(flat)
    L = table.direct_radiance(8, sd.bsdf_params[b], frames, wi, ld, val).reshape(p.shape[0], p.shape[1], -1, 3)
    bad = _outside(img, L)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[0], img[tuple(np.argwhere(bad)[0][:2])])
    Ls = table.direct_radiance(8, sd.bsdf_params[swapped], frames, wi, ld, val).reshape(p.shape[0], p.shape[1], -1, 3)
    assert _outside(img, Ls).any(), "the render does not depend on the tangent direction"


# --- what only mtsgpu_upload_scene can refuse (the flattener refuses the same tables first, so the scene is patched) --
def test_upload_rejections(gpu_lib, mts):
    def flat(make, sphere=False):
        sd = mts.scenes.SceneDescription("upload")
        b = make(sd)
        if sphere:
            sd.add_sphere((0.0, 0.0, 0.0), 1.0, bsdf=b)
        else:
            pos, tri = mts.scenes._quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), (0, 1, 0))
            sd.add_mesh(pos, tri, bsdf=b, face_normals=True)
        sd.point_light((0.0, 2.0, 0.0), 1.0)
        return mts.Scene(sd), b
    def upload_patched(scene, b, patch, slot_type=None):
        sc = scene.ptr.contents
        n = sc.n_bsdfs
        P = np.ctypeslib.as_array(sc.bsdf_params, shape=(n * 16,))
        T = np.ctypeslib.as_array(sc.bsdf_type, shape=(n,))
        for i, v in patch.items():
            P[16 * b + i] = v
        if slot_type is not None:
            T[slot_type[0]] = slot_type[1]
        it = mts.MIPathTracer(maxDepth=2)
        with pytest.raises(mts.MtsGpuError) as e:
            it._chk(mts.lib().mtsgpu_upload_scene(it._ctx, scene.ptr), "upload_scene")
        return str(e.value)
    good = lambda sd: sd.composite([0.4, 0.6], [sd.lambertian(0.5), sd.ward(0.2, 0.2)])
    scene, b = flat(good)
    assert "between 1 and 7 children" in upload_patched(scene, b, {0: 0.0})
    scene, b = flat(good)
    assert "between 1 and 7 children" in upload_patched(scene, b, {0: 8.0})
    scene, b = flat(good)
    assert "invalid BRDF weight" in upload_patched(scene, b, {2: -0.5})
    scene, b = flat(good)
    assert "index out of range" in upload_patched(scene, b, {4: 17.0})
    scene, b = flat(good)
    assert "nested composites" in upload_patched(scene, b, {4: float(b)})
    scene, b = flat(good)
    assert "delta BSDF" in upload_patched(scene, b, {}, slot_type=(0, 1))
    scene, b = flat(good)
    assert "delta BSDF" in upload_patched(scene, b, {}, slot_type=(0, 4))
    scene, b = flat(good)
    assert "unknown type" in upload_patched(scene, b, {}, slot_type=(b, 10))
    # an anisotropic Ward on a triangle mesh, alone and inside the composite
    scene, b = flat(good)
    msg = upload_patched(scene, 1, {1: 0.1, 2: 0.3})
    assert "texture coordinates are required to generate tangent vectors" in msg
    scene, b = flat(lambda sd: sd.ward(0.2, 0.2))
    assert "texture coordinates are required" in upload_patched(scene, b, {1: 0.05})


# --- 5. drivers and sharding -----------------------------------------------------------------------------------------
def _mixed_scene(mts):
    """lambertian walls, an isotropic Ward floor, a composite sphere whose Ward child is anisotropic, a glass sphere and a
    quad emitter"""
    S = mts.scenes
    sd = S.SceneDescription("mixed")
    white = sd.lambertian(0.6)
    floor = sd.ward(0.15, 0.15, rd=(0.5, 0.4, 0.3), rs=0.4, kd=0.6, ks=0.4, model="ward-duer")
    comp = sd.composite([0.4, 0.6], [sd.lambertian(0.7, 0.2, 0.2), sd.ward(0.1, 0.3, rd=0.5, rs=0.5, kd=0.5, ks=0.5)])
    glass = sd.dielectric()
    for args, b in ((((-1, 0, -1), (2, 0, 0), (0, 0, 2), (0, 1, 0)), floor), (((-1, 0, -1), (2, 0, 0), (0, 2, 0), (0, 0, 1)), white),
                    (((-1, 0, -1), (0, 0, 2), (0, 2, 0), (1, 0, 0)), white), (((1, 0, -1), (0, 0, 2), (0, 2, 0), (-1, 0, 0)), white)):
        pos, tri = S._quad(*args)
        sd.add_mesh(pos, tri, bsdf=b, face_normals=True)
    sd.add_sphere((-0.4, 0.35, -0.2), 0.35, bsdf=comp)
    sd.add_sphere((0.45, 0.3, 0.3), 0.3, bsdf=glass)
    lum = sd.add_lum(mts.abi.LUM_AREA, [12.0, 11.0, 9.0])
    pos, tri = S._quad((-0.3, 1.98, -0.3), (0.6, 0, 0), (0, 0, 0.6), (0, -1, 0))
    sd.add_mesh(pos, tri, bsdf=sd.lambertian(0.0), lum=lum, face_normals=True)
    sd.camera = dict(origin=(0.0, 1.0, 3.4), target=(0.0, 0.9, 0.0), up=(0.0, 1.0, 0.0), fov=39.3)
    return sd


def test_drivers_and_tile_parts_give_one_film(gpu_lib, mts):
    sd = _mixed_scene(mts)
    scene = mts.Scene(sd)
    Wd, Ht, spp = 96, 64, 8
    cam = mts.PerspectiveCamera.for_description(sd, Wd, Ht)
    def render(drive, part=0, n_parts=1):
        it = mts.MIPathTracer(maxDepth=6)
        it.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=11)
        if drive == 1: it.set_tuning(sync_free=0)
        elif drive == 2: it.set_tuning(sync_free=0); it.set_options(max_paths=spp * (Wd * Ht // 3 + 1))
        elif drive == 3: it.set_tuning(sync_free=1, shade_fused=0)
        if n_parts > 1:
            it.set_tiles(32, part, n_parts)
        assert it.render()
        return it.film()
    base = render(0)
    assert np.isfinite(base).all() and (base[..., :3] > 0).any()
    for drive in (1, 2, 3):
        other = render(drive)
        assert np.array_equal(base.view(np.uint32), other.view(np.uint32)), "drive %d differs from the device-driven frame" % drive
    for n_parts in (2, 5):
        total = sum(render(0, part, n_parts) for part in range(n_parts))
        assert np.array_equal(base.view(np.uint32), total.view(np.uint32)), "%d tile parts do not add up to the frame" % n_parts


# --- 4. pdf and sample inside a frame: a floor under a quad area light -----------------------------------------------
AREA_W = AREA_H = 8          # every pixel is one image block: the box filter makes it the mean of its own samples
# Samples per pixel and seed.  A standard error estimated from the seeds' block means is an error bar only if those means are
# close to normal.  Under BSDF sampling a sample contributes only when it hits the light, which subtends about 0.12 sr from the
# floor: about 3 % of the diffuse lobe's samples and fewer of the glossy lobe's.  At 128 samples a block mean is the sum of a
# handful of hits, a skewed, Poisson-like variable whose spread a few dozen seeds underestimate whenever the rare large terms are
# missing from all of them; at 4096 it sums over a hundred hits.
AREA_SPP, AREA_SEEDS = 4096, 64
AREA_SUB = 5                 # points per pixel side for the expected block mean (9 to bound its error)
LIGHT_P0, LIGHT_SIZE, LIGHT_Y, LIGHT_LE = (-0.9, -0.7), 0.6, 1.5, 8.0
AREA_FLOORS = [
    ("ward floor", lambda sd: sd.ward(0.2, 0.2, rd=0.5, rs=0.5, kd=0.5, ks=0.5)),
    ("composite floor", lambda sd: sd.composite([0.4, 0.6], [sd.lambertian(0.5), sd.ward(0.2, 0.2, rd=0.5, rs=0.5, kd=0.5, ks=0.5)])),
]


def _area_scene(mts, make):
    sd = mts.scenes.SceneDescription("area light")
    b = make(sd)
    pos, tri = mts.scenes._quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), (0, 1, 0))
    sd.add_mesh(pos, tri, bsdf=b, face_normals=True)
    lum = sd.add_lum(mts.abi.LUM_AREA, [LIGHT_LE] * 3)
    pos, tri = mts.scenes._quad((LIGHT_P0[0], LIGHT_Y, LIGHT_P0[1]), (LIGHT_SIZE, 0, 0), (0, 0, LIGHT_SIZE), (0, -1, 0))
    sd.add_mesh(pos, tri, bsdf=sd.lambertian(0.0), lum=lum, face_normals=True)
    sd.camera = dict(origin=(1.2, 2.0, 0.9), target=(0.05, 0.0, -0.1), up=(0.0, 1.0, 0.0), ortho_scale=(0.4, 0.4))
    return sd, b


def _expected_blocks(table, btype, P, cam, sub, G):
    """binary64 quadrature of the direct-lighting integral Lo(p) = integral over the light of Le f(wi, wo) cos_p cos_l / r^2
    dA (midpoint rule, G x G cells) at sub x sub points of every pixel's footprint, averaged per pixel.  The light is fully
    visible from the floor and faces it, and the camera sees the floor only."""
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
    p = o + (-o[:, 1] / d[1])[:, None] * d                                   # on the floor y = 0
    g = (np.arange(G) + 0.5) / G * LIGHT_SIZE
    lx, lz = np.meshgrid(LIGHT_P0[0] + g, LIGHT_P0[1] + g, indexing="ij")
    q = np.stack([lx.ravel(), np.full(G * G, LIGHT_Y), lz.ravel()], axis=1)
    dA = (LIGHT_SIZE / G) ** 2
    to_local = lambda v: np.stack([v[:, 2], v[:, 0], v[:, 1]], axis=1)       # frame s = +z, t = +x, n = +y (the BSDFs are isotropic)
    wi = to_local(np.broadcast_to(-d, (1, 3)))
    Lo = np.zeros(len(p))
    for i0 in range(0, len(p), 64):
        pp = p[i0:i0 + 64]
        v = q[None, :, :] - pp[:, None, :]
        r2 = (v * v).sum(axis=2)
        w = v / np.sqrt(r2)[:, :, None]
        cos_p, cos_l = w[:, :, 1], w[:, :, 1]                                # floor normal +y, light normal -y: both <w, +y>
        fv, _, _ = table.f(btype, P, np.broadcast_to(wi, (w.shape[0] * w.shape[1], 3)), to_local(w.reshape(-1, 3)))
        Lo[i0:i0 + 64] = (LIGHT_LE * fv[:, 0].reshape(r2.shape) * cos_p * cos_l / r2).sum(axis=1) * dA
    return Lo.reshape(cam.height, cam.width, sub * sub).mean(axis=2)


@pytest.mark.parametrize("strategy", ["direct, luminaire samples only", "direct, BSDF samples only", "path (MIS)"])
@pytest.mark.parametrize("k", range(2))
def test_area_light_floor_against_quadrature(gpu_lib, mts, k, strategy):
    """pdf() and sample() inside a frame (the point-light cases use neither): the same floor rendered with luminaire samples
    only, with BSDF samples only and with both under MIS has one expected value, the direct-lighting integral.  The error bar
    is statistical and measured: the standard error of every block's mean over AREA_SEEDS seeds; a block is accepted within
    4 of those plus the quadrature's own error, bounded by halving the light's grid step and by refining the footprint grid.
    More seeds than the 8 the check needs at least, so that 4 standard errors of an estimated deviation are a rare event over
    the 384 blocks compared here (Student's t with 63 degrees of freedom: 2e-4 per block)."""
    name, make = AREA_FLOORS[k]
    sd, b = _area_scene(mts, make)
    scene = mts.Scene(sd)
    cam = mts.PerspectiveCamera.for_description(sd, AREA_W, AREA_H)
    films = []
    for seed in range(AREA_SEEDS):
        it = {"direct, luminaire samples only": lambda: mts.MIDirectIntegrator(1, 0), "direct, BSDF samples only": lambda: mts.MIDirectIntegrator(0, 1),
              "path (MIS)": lambda: mts.MIPathTracer(maxDepth=2)}[strategy]()
        it.preprocess(scene, cam, sampler="independent", sampleCount=AREA_SPP, seed=1000 + seed)
        assert it.render()
        films.append(mts.develop(it.film())[..., 0].astype(np.float64))
    films = np.stack(films)
    assert np.isfinite(films).all()
    mean, se = films.mean(axis=0), films.std(axis=0, ddof=1) / np.sqrt(AREA_SEEDS)
    table = ward_cases.table_of(sd)
    t, P = sd.bsdf_type[b], sd.bsdf_params[b]
    E = _expected_blocks(table, t, P, cam.c, AREA_SUB, 32)
    qerr = np.abs(E - _expected_blocks(table, t, P, cam.c, AREA_SUB, 64)) + np.abs(E - _expected_blocks(table, t, P, cam.c, 9, 32))
    dev = np.abs(mean - E)
    print("%s, %s: expected %.4g..%.4g, standard error %.3g..%.3g (relative %.3g..%.3g), quadrature error <= %.3g, worst deviation %.3g = %.2f standard errors"
          % (name, strategy, E.min(), E.max(), se.min(), se.max(), (se / E).min(), (se / E).max(), qerr.max(), dev.max(),
             (np.maximum(dev - qerr, 0) / se).max()))
    assert (E > 0).all() and (se > 0).all() and (se < 0.1 * E).all(), "the error bars must be far smaller than the value they guard"
    bad = dev > 4 * se + qerr
    assert not bad.any(), (name, strategy, np.argwhere(bad)[0], mean[bad][0], E[bad][0], se[bad][0])
