"""Tangent frames on the MI355X: the shading frame the tangent kernels build (read out through mtsgpu_shading_frame_eval)
against the float32 mirror of tests/ref64_tan.py bit for bit, the refusals of mtsgpu_upload_scene_tangents, films and samples
that must not change, point-lit renders of an anisotropic Ward on meshes against closed forms whose frames come from the
binary64 restatement, and one film across every way of driving the bounces."""
import numpy as np
import pytest

import closed_forms as cf
import ref64
import ref64_tan as R
import tan_cases
import ward_cases

pytestmark = pytest.mark.gpu
F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits_or_nan(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def _first_prim(sd, s):
    return sum(1 if m.sphere is not None else len(m.triangles) for m in sd.meshes[:s])


# --- 1. the frame hook -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mirrors(mts):
    sd = tan_cases.hook_scene(mts)
    return sd, {s: R.tangents32(sd.meshes[s].positions, sd.meshes[s].normals, sd.meshes[s].texcoords, sd.meshes[s].triangles) for s in (0, 1, 2)}


@pytest.mark.parametrize("device_tree", [False, True])
def test_frame_hook_equals_the_mirror(gpu_lib, mts, mirrors, device_tree):
    sd, mirror = mirrors
    scene = mts.Scene(sd, gpu_binning=device_tree, gpu_exact=device_tree)
    twin = mts.Scene(tan_cases.hook_scene(mts, isotropic=True), gpu_binning=device_tree, gpu_exact=device_tree)
    assert scene.wants_tangents and not twin.wants_tangents
    cam = mts.PerspectiveCamera.for_description(sd, 8, 8)
    it = mts.MIPathTracer(maxDepth=2); it.preprocess(scene, cam, sampleCount=1)
    before = mts.MIPathTracer(maxDepth=2); before.preprocess(twin, cam, sampleCount=1)
    rng = np.random.RandomState(17)
    for s in (0, 1, 2):
        m = sd.meshes[s]
        tan32, nrm, _ = mirror[s]
        prim, u, v = tan_cases.records(rng, 0, len(m.triangles), 4096)
        want, _ = R.frame(tan32[:, :3], nrm, m.triangles, prim, u, v, np.float32)
        rec = np.stack([u, v, 0 * u], axis=1)
        got = it.shading_frame_eval(prim + _first_prim(sd, s), rec).reshape(-1, 3, 3)
        ok = same_bits_or_nan(got, want)
        assert ok.all(), (m.name, int((~ok).sum()), np.argwhere(~ok)[0], got[np.argwhere(~ok)[0][0]], want[np.argwhere(~ok)[0][0]])
        if s < 2:
            assert np.isfinite(got).all()
            # and it is not the frame the mesh had before
            old = before.shading_frame_eval(prim + _first_prim(sd, s), rec).reshape(-1, 3, 3)
            assert np.array_equal(bits(old[:, 2]), bits(got[:, 2])) and np.abs(old[:, 0] - got[:, 0]).max() > 0.1
    # shapes without tangents keep the frame they had: the isotropic mesh, the one without texcoords, the face-normal one
    for s in (3, 4, 6):
        m = sd.meshes[s]
        prim, u, v = tan_cases.records(rng, _first_prim(sd, s), len(m.triangles), 1024)
        rec = np.stack([u, v, 0 * u], axis=1)
        assert np.array_equal(bits(it.shading_frame_eval(prim, rec)), bits(before.shading_frame_eval(prim, rec))), m.name
    # the sphere: what it returned before tangents were set
    d = rng.normal(size=(2048, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = (np.float32(sd.meshes[5].sphere[0]) + F(sd.meshes[5].sphere[1]) * d.astype(np.float32)).astype(np.float32)
    prim = np.full(len(p), _first_prim(sd, 5), dtype=np.uint32)
    a, b = it.shading_frame_eval(prim, p), before.shading_frame_eval(prim, p)
    assert same_bits_or_nan(a, b).all() and np.isfinite(a).mean() > 0.99
    with pytest.raises(mts.MtsGpuError, match="out of range"):
        it.shading_frame_eval([scene.sc.n_tris], [[0, 0, 0]])
    # the count is refused before a record is read, so one record's memory stands in for 2^24 + 1 of them
    A, p1, f9 = mts.abi, np.zeros(1, np.uint32), np.zeros(9, np.float32)
    with pytest.raises(mts.MtsGpuError, match=r"at most 2\^24 query records per call.*code -1"):
        it._chk(mts.lib().mtsgpu_shading_frame_eval(it._ctx, (1 << 24) + 1, A.ptr(p1, A.u32p), A.ptr(f9, A.f32p), A.ptr(f9, A.f32p)), "shading_frame_eval")


# --- 2. the refusals of mtsgpu_upload_scene_tangents ----------------------------------------------------------------------
def test_upload_scene_tangents_refusals(gpu_lib, mts):
    sd = tan_cases.hook_scene(mts)
    scene = mts.Scene(sd)
    tan, has = scene.vertex_tangents()
    dpdu = np.ascontiguousarray(tan[:, :3])
    it = mts.MIPathTracer(maxDepth=2)
    it.upload_scene_tangents(scene, dpdu, has)                     # accepted
    with pytest.raises(mts.MtsGpuError, match="texture coordinates are required to generate tangent vectors"):
        it.upload_scene_tangents(scene, None, None)                # vertex normals, anisotropic, no tangents
    for drop in (0, 1, 2):
        fewer = has.copy(); fewer[drop] = 0
        with pytest.raises(mts.MtsGpuError, match="texture coordinates are required"):
            it.upload_scene_tangents(scene, dpdu, fewer)
    with pytest.raises(mts.MtsGpuError, match="texture coordinates are required"):
        it._chk(mts.lib().mtsgpu_upload_scene(it._ctx, scene.ptr), "upload_scene")      # the old call, as before
    bad = dpdu.copy(); bad[3, 1] = np.inf
    with pytest.raises(mts.MtsGpuError, match="non-finite tangent"):
        it.upload_scene_tangents(scene, bad, has)
    bad = dpdu.copy(); bad[-1, 0] = np.nan                          # a row of a shape without tangents is ignored
    it.upload_scene_tangents(scene, bad, has)
    more = has.copy(); more[5] = 1
    with pytest.raises(mts.MtsGpuError, match="only a triangle mesh"):
        it.upload_scene_tangents(scene, dpdu, more)
    more = has.copy(); more[6] = 1
    with pytest.raises(mts.MtsGpuError, match="need vertex normals"):
        it.upload_scene_tangents(scene, dpdu, more)
    with pytest.raises(mts.MtsGpuError, match="both be given"):
        it.upload_scene_tangents(scene, dpdu, None)
    # a face-normal mesh with an anisotropic BSDF: accepted without tangents by the new call, refused by the old one
    one = mts.scenes.SceneDescription("face normals")
    pos, tri, nrm, uv = tan_cases.floor()
    one.add_mesh(pos, tri, bsdf=one.ward(**tan_cases.WARD_ANISO), face_normals=True, texcoords=uv)
    one.point_light((0, 2, 0), 1.0)
    flat = mts.Scene(one)
    assert flat.wants_tangents and flat.tangent_args() == (None, None)
    it.upload_scene_tangents(flat, None, None)
    with pytest.raises(mts.MtsGpuError, match="texture coordinates are required"):
        it._chk(mts.lib().mtsgpu_upload_scene(it._ctx, flat.ptr), "upload_scene")
    # colours and textures work after the new upload
    it.upload_scene_tangents(scene, dpdu, has)
    uvp, uvh = scene.vertex_texcoords()
    it.set_uv_textures(uvp, uvh, [mts.scenes.Checkerboard()], np.full((len(sd.bsdf_type), 2), -1, dtype=np.int32))
    it.set_vertex_colors()


# --- 3. frames that must not change ---------------------------------------------------------------------------------------
def _film(mts, sd, scene, res=(48, 32), spp=4, max_depth=6, seed=11, keep=False):
    cam = mts.PerspectiveCamera.for_description(sd, *res)
    it = mts.MIPathTracer(maxDepth=max_depth)
    it.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=seed)
    assert it.render()
    return (it.film(), it, cam) if keep else it.film()


def test_scene_without_tangents_renders_through_the_old_calls(gpu_lib, mts):
    """the mixed scene with every Ward isotropic has no tangents anywhere: Scene(sd) takes the calls it always took, and the
    film equals, bit for bit, the one of the explicit old calls and the one of the new upload with nothing to hand over"""
    sd = tan_cases.mixed_scene(mts, isotropic=True, extra="checkerboard")
    scene = mts.Scene(sd)
    assert not scene.wants_tangents and scene.tangent_args() is None
    base = _film(mts, sd, scene)
    assert np.isfinite(base).all() and (base[..., :3] > 0).any()
    cam = mts.PerspectiveCamera.for_description(sd, 48, 32)
    for new_upload in (False, True):
        it = mts.MIPathTracer(maxDepth=6)
        it.preprocess(scene, cam, sampler="independent", sampleCount=4, seed=11)
        if new_upload:
            it.upload_scene_tangents(scene, None, None)
        else:
            it._chk(mts.lib().mtsgpu_upload_scene(it._ctx, scene.ptr), "upload_scene")
        it._chk(mts.lib().mtsgpu_set_uv_textures(it._ctx, *scene.uv_texture_args()), "set_uv_textures")
        assert it.render()
        assert np.array_equal(bits(base), bits(it.film())), new_upload


def _primary_shape(sd, cam, raster):
    """the shape a camera ray through raster positions [n][2] hits first, in binary64: meshes by Moeller-Trumbore, spheres in
    closed form; -1 = none"""
    r2c = np.array(list(cam.raster_to_camera), dtype=np.float64).reshape(4, 4)
    c2w = np.array(list(cam.camera_to_world), dtype=np.float64).reshape(4, 4)
    ras = np.concatenate([raster, np.zeros((len(raster), 1)), np.ones((len(raster), 1))], axis=1)
    pc = ras @ r2c.T; pc = pc[:, :3] / pc[:, 3:4]
    d = pc @ c2w[:3, :3].T; d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = c2w[:3, 3]
    best_t, best_s = np.full(len(d), np.inf), np.full(len(d), -1)
    for s, m in enumerate(sd.meshes):
        if m.sphere is not None:
            c, r = np.asarray(m.sphere[0], dtype=np.float64), m.sphere[1]
            oc = o - c
            b = d @ oc
            disc = b * b - (oc @ oc - r * r)
            t = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0)), np.inf)
            t[t <= 0] = np.inf
        else:
            P = m.positions.astype(np.float64)[m.triangles.astype(np.int64)]
            e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
            pv = np.cross(d[:, None, :], e2[None, :, :])
            det = (pv * e1[None]).sum(axis=2)
            with np.errstate(divide="ignore", invalid="ignore"):
                inv = 1 / det
                tv = o - P[:, 0]
                uu = (pv * tv[None]).sum(axis=2) * inv
                qv = np.cross(tv, e1)
                vv = (d[:, None, :] * qv[None]).sum(axis=2) * inv
                tt = (qv * e2).sum(axis=1)[None] * inv
            hit = (np.abs(det) > 1e-12) & (uu >= 0) & (vv >= 0) & (uu + vv <= 1) & (tt > 0)
            t = np.where(hit, tt, np.inf).min(axis=1)
        closer = t < best_t
        best_t[closer] = t[closer]; best_s[closer] = s
    return best_s


@pytest.mark.parametrize("max_depth", [1, 2])
def test_isotropic_meshes_keep_their_samples(gpu_lib, mts, max_depth):
    """the mixed scene against its isotropic twin, sample by sample: a sample whose camera ray sees an isotropic mesh, a mesh
    without texcoords, the glass or nothing (at its position and a hundredth of a pixel around it) is the same bits in both;
    at maxDepth = 2 such a path ends before its second hit is shaded, so nothing of the tangent meshes enters it.  The samples
    on the tangent meshes do change at maxDepth = 2"""
    sd, twin = tan_cases.mixed_scene(mts), tan_cases.mixed_scene(mts, isotropic=True)
    a, ita, cam = _film(mts, sd, mts.Scene(sd), max_depth=max_depth, keep=True)
    b, itb, _ = _film(mts, twin, mts.Scene(twin), max_depth=max_depth, keep=True)
    sa, sb = ita.pass_samples(), itb.pass_samples()
    assert len(sa) == 48 * 32 * 4 and np.array_equal(bits(sa[:, 4:6]), bits(sb[:, 4:6]))
    raster = sa[:, 4:6].astype(np.float64)
    shapes = np.stack([_primary_shape(sd, cam.c, raster + off) for off in ((0, 0), (0.01, 0), (-0.01, 0), (0, 0.01), (0, -0.01))])
    tangent = np.isin(shapes, [0, 4, 6])              # the floor, the cylinder patch, the anisotropic sphere
    untouched = ~tangent.any(axis=0)
    assert untouched.sum() > 1000 and tangent.all(axis=0).sum() > 500
    assert np.array_equal(bits(sa[untouched, :4]), bits(sb[untouched, :4]))
    if max_depth == 1:
        assert np.array_equal(bits(a), bits(b))
    else:
        assert (bits(sa[tangent.all(axis=0), :3]) != bits(sb[tangent.all(axis=0), :3])).any(axis=1).mean() > 0.1


# --- 4. end to end: an anisotropic Ward on meshes under a point light -----------------------------------------------------
def _rays(cam):
    """origins [H * W * SUB * SUB][3] and the direction of an orthographic camera's rays through every pixel's sub-grid"""
    r2c = np.array(list(cam.raster_to_camera), dtype=np.float64).reshape(4, 4)
    c2w = np.array(list(cam.camera_to_world), dtype=np.float64).reshape(4, 4)
    u = np.linspace(0.0, 1.0, cf.SUB)
    x = (np.arange(cam.width)[None, :, None, None] + u[None, None, :, None] + 0 * u[None, None, None, :])
    y = (np.arange(cam.height)[:, None, None, None] + 0 * u[None, None, :, None] + u[None, None, None, :])
    x, y = np.broadcast_arrays(x, y)
    ras = np.stack([x, y, 0 * x, 1 + 0 * x], axis=-1).reshape(-1, 4)
    pc = ras @ r2c.T; pc = pc[:, :3] / pc[:, 3:4]
    o = np.concatenate([pc, np.ones((len(pc), 1))], axis=1) @ c2w.T
    d = c2w[:3, :3] @ np.array([0.0, 0.0, 1.0])
    return o[:, :3] / o[:, 3:4], d / np.linalg.norm(d)


def _mesh_hits(pos, tri, o, d):
    """(prim, u, v, p) of parallel rays against a mesh every ray hits exactly once (binary64; a hit on a shared edge goes to
    the first triangle that has it)"""
    P = pos.astype(np.float64)[tri.astype(np.int64)]
    prim = np.full(len(o), -1); uo = np.zeros(len(o)); vo = np.zeros(len(o)); to = np.zeros(len(o))
    for k in range(len(P)):
        e1, e2 = P[k, 1] - P[k, 0], P[k, 2] - P[k, 0]
        pv = np.cross(d, e2)
        det = pv @ e1
        if abs(det) < 1e-14:
            continue
        tv = o - P[k, 0]
        u = tv @ pv / det
        qv = np.cross(tv, e1)
        v = qv @ d / det
        t = qv @ e2 / det
        eps = 1e-9
        take = (prim < 0) & (u >= -eps) & (v >= -eps) & (u + v <= 1 + eps) & (t > 0)
        prim[take] = k; uo[take] = np.clip(u[take], 0, 1); vo[take] = np.clip(v[take], 0, 1); to[take] = t[take]
    assert (prim >= 0).all(), "every footprint must lie on the mesh"
    return prim, uo, vo, o + to[:, None] * d


def _outside(img, L):
    lo, hi = L.min(axis=2), L.max(axis=2)
    tol = cf.REL_TOL * np.maximum(hi, 1e-30) + cf.GRID_SLACK * (hi - lo)
    return ~((img >= lo - tol) & (img <= hi + tol))


E2E = {
    "floor": ("floor", lambda sd, kw: sd.ward(**kw)),
    "cylinder": ("cylinder", lambda sd, kw: sd.ward(**kw)),
    "composite": ("floor", lambda sd, kw: sd.composite([0.4, 0.6], [sd.lambertian(0.5), sd.ward(**kw)])),
    "twosided": ("floor", lambda sd, kw: sd.twosided(sd.ward(**kw))),
}


@pytest.mark.parametrize("integ", ["path", "direct"])
@pytest.mark.parametrize("case", sorted(E2E))
def test_anisotropic_ward_on_a_mesh(gpu_lib, mts, case, integ):
    """ward(0.1, 0.3) on the rotated-uv floor and on the cylinder patch, alone, inside a composite (bin 9) and inside a twosided:
    every pixel inside the extremes of the closed form over its footprint with the frames of the binary64 restatement; neither
    the closed form of ward(0.3, 0.1) nor the one with Frame(n) contains the image"""
    shape, make = E2E[case]
    sd = mts.scenes.SceneDescription("anisotropic " + case)
    b = make(sd, tan_cases.WARD_ANISO)
    swapped = make(sd, tan_cases.WARD_SWAPPED)
    if shape == "floor":
        pos, tri, nrm, uv = tan_cases.floor(4.0)
        sd.camera = dict(origin=(1.2, 2.0, 0.9), target=(0.05, 0.0, -0.1), up=(0.0, 1.0, 0.0), ortho_scale=(0.4, 0.4))
        lpos, I = (-0.6, 1.5, -0.4), 6.0
    else:
        pos, tri, nrm, uv = tan_cases.cylinder()
        sd.camera = dict(origin=(0.1, 3.0, 0.05), target=(0.1, 0.0, 0.05), up=(0.0, 0.0, -1.0), ortho_scale=(0.4, 0.4))
        lpos, I = (-0.6, 2.5, -0.4), 6.0
    sd.add_mesh(pos, tri, bsdf=b, face_normals=False, normals=nrm, texcoords=uv)
    sd.point_light(lpos, I)
    scene = mts.Scene(sd)
    assert scene.wants_tangents and scene.vertex_tangents()[1].tolist() == [1]
    it = mts.MIPathTracer(maxDepth=2) if integ == "path" else mts.MIDirectIntegrator(1, 1)
    cam = mts.PerspectiveCamera.for_description(sd, cf.W, cf.H)
    it.preprocess(scene, cam, sampler="independent", sampleCount=cf.SPP, seed=7)
    assert it.render()
    img = mts.develop(it.film())
    assert np.isfinite(img).all() and (img > 0).all()
    o, d = _rays(cam.c)
    prim, u, v, p = _mesh_hits(pos, tri, o, d)
    _, _, made = R.tangents32(pos, nrm, uv, tri)
    tan64, bound = R.tangents64(pos, nrm, uv, tri, made)
    frames, _ = R.frame(tan64[:, :3], nrm, tri, prim, u.astype(np.float32), v.astype(np.float32), np.float64, None, bound[:, :3])
    ld, val = ref64.point_light([I] * 3, lpos, p)
    table = ward_cases.table_of(sd)
    wi = np.broadcast_to(-d, p.shape)
    shape4 = (cf.H, cf.W, -1, 3)
    L = table.direct_radiance(sd.bsdf_type[b], sd.bsdf_params[b], frames, wi, ld, val).reshape(shape4)
    bad = _outside(img, L)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[0], img[tuple(np.argwhere(bad)[0][:2])])
    Ls = table.direct_radiance(sd.bsdf_type[swapped], sd.bsdf_params[swapped], frames, wi, ld, val).reshape(shape4)
    assert _outside(img, Ls).any(), "the render does not depend on which way the tangent points"
    Lp = table.direct_radiance(sd.bsdf_type[b], sd.bsdf_params[b], R.plain_frame(frames[:, 2]), wi, ld, val).reshape(shape4)
    assert _outside(img, Lp).any(), "the render does not use the tangent"


# --- 5. one film across drivers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sky, extra", [(False, None), (True, None), (False, "checkerboard"), (True, "vertexcolors")])
def test_drivers_tile_parts_group_and_direct_give_one_film(gpu_lib, mts, sky, extra):
    sd = tan_cases.mixed_scene(mts, sky=sky, extra=extra)
    scene = mts.Scene(sd)
    assert scene.wants_tangents and scene.vertex_tangents()[1].tolist() == tan_cases.MIXED_FLAGS
    assert (scene.bsdf_slot_texture is not None) == (extra == "checkerboard") and (scene.bsdf_color_slots is not None) == (extra == "vertexcolors")
    res, spp = 32, 4
    cam = mts.PerspectiveCamera.for_description(sd, res, res)

    def render(integ, drive, part=0, n_parts=1):
        it = mts.MIPathTracer(maxDepth=6) if integ == "path" else mts.MIDirectIntegrator(*integ)
        it.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=5)
        if drive == 1: it.set_tuning(sync_free=0)
        elif drive == 2: it.set_tuning(sync_free=0); it.set_options(max_paths=spp * (res * res // 3 + 1))
        elif drive == 3: it.set_tuning(sync_free=1, shade_fused=0)
        if n_parts > 1:
            it.set_tiles(16, part, n_parts)
        assert it.render()
        return it.film()
    for integ in ("path", (1, 1), (2, 3)):
        base = render(integ, 0)
        assert np.isfinite(base).all() and (base[..., :3] > 0).any()
        for drive in (1, 2, 3):
            assert np.array_equal(bits(base), bits(render(integ, drive))), (integ, "drive %d differs from the device-driven frame" % drive)
        total = sum(render(integ, 0, part, 2) for part in range(2))
        assert np.array_equal(bits(base), bits(total)), (integ, "two tile parts do not add up to the frame")
        if integ == (2, 3):
            continue
        g = mts.DeviceGroup([0, 0], maxDepth=6)
        g.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=5)
        if integ != "path":
            for i in range(len(g)):
                assert mts.lib().mtsgpu_set_direct_integrator(g.member(i), *integ) == 0
        assert g.render(block_size=16, ordered_reduce=True)
        assert np.array_equal(bits(base), bits(g.film())), (integ, "the two-member group's film differs")
        g.close()
    # the tangents matter in this frame: the isotropic twin renders another film
    twin = tan_cases.mixed_scene(mts, isotropic=True, sky=sky, extra=extra)
    it = mts.MIPathTracer(maxDepth=6)
    it.preprocess(mts.Scene(twin), cam, sampler="independent", sampleCount=spp, seed=5)
    assert it.render() and not np.array_equal(bits(it.film()), bits(render("path", 0)))
