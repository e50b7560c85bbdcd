"""The cylinder shape on the MI355X: the cylinder instantiations of k_trace against the tree-free brute force (binary64 inside
K_GEOM bounds, and the binary32 brute force bit for bit in every scene: the mirror for the cylinders, the oracle for the
triangles and the sphere), on the host tree and on the device-built ones, with and without the lean closest-hit kernel; device-built trees
against the host tree word for word; the clip in a kernel against the host's; the intersection record through the read-out
hooks against the mirror bit for bit and binary64; a tie between a cylinder and a triangle; the refusals of the uploads;
frames.  The CPU side is tests/test_cyl.py."""
import numpy as np
import pytest

import cyl_cases as CC
import geom_cases as GC
import ref64_cyl as R
from ref64 import EPS32
from test_gpu_tex import _all_samples, _prep

pytestmark = pytest.mark.gpu
F = np.float32
TREES = {"host": dict(), "device_exact": dict(gpu_exact=True), "device_both": dict(gpu_binning=True, gpu_exact=True)}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _scene(mts, name, tree):
    sd = CC.scene_description(mts, name)
    kp = CC.kd_params(mts, name)
    if tree == "device_both":
        kp.exact_prim_threshold = 4          # so that the binning phase has nodes to bin in scenes this small
    return sd, mts.Scene(sd, kd_params=kp, **TREES[tree])


_cases = {}


def _mirror(mts, orc, sd, scene, blocks, cyl, rays, shadow):
    """the binary32 answer of the whole scene -> (hit, t, prim, tied): the cylinders by the mirror's brute force (cyl_cases.brute32),
    the triangles and spheres by the oracle -- the reference's binary32 traversal -- on the scene without its cylinders, under the
    box of the scene with them, so that every ray starts from the interval the device gives it.  Each side leaves the other only a
    smaller maxt, and a primitive tested with a smaller maxt answers as before or not at all, so the scene's answer is the smaller
    of the two t; where they are equal the order of the leaf decides and the ray is tied"""
    import ctypes as C
    lo, hi = list(scene.sc.aabb_min), list(scene.sc.aabb_max)
    first = np.cumsum([0] + [1 if (m.sphere is not None or m.shape_type == mts.abi.SHAPE_CYLINDER) else len(m.triangles) for m in sd.meshes])
    hit, t, prim, tied = CC.brute32([blocks[s] for s in cyl], [int(first[s]) for s in cyl], lo, hi, rays, shadow=shadow)
    rest = [s for s in range(len(sd.meshes)) if s not in cyl]
    if not rest:
        return hit, t, prim, tied
    sd2 = CC.scene_description(mts, sd.name[4:])
    sd2.meshes = [sd2.meshes[s] for s in rest]
    other = mts.Scene(sd2)
    cp = mts.abi.Scene.from_buffer_copy(other.sc)
    for a in range(3):
        cp.aabb_min[a] = lo[a]; cp.aabb_max[a] = hi[a]
    oh = orc.trace_rays(C.pointer(cp), rays, shadow=shadow)
    if shadow:
        return hit | (oh[:, 3] != 0), None, None, tied
    # the oracle's primitive numbers are those of the scene without the cylinders
    ofirst = np.cumsum([0] + [1 if sd.meshes[s].sphere is not None else len(sd.meshes[s].triangles) for s in rest])
    ohit = oh[:, 3] != GC.MISS
    oprim = oh[:, 3].astype(np.int64)
    full = np.full(len(rays), -1, dtype=np.int64)
    for k, s in enumerate(rest):
        sel = ohit & (oprim >= ofirst[k]) & (oprim < ofirst[k + 1])
        full[sel] = oprim[sel] - ofirst[k] + first[s]
    ot = np.where(ohit, oh[:, 0].copy().view(np.float32), np.float32(np.inf)).astype(np.float32)
    tc = np.where(hit, t, np.float32(np.inf)).astype(np.float32)
    tied = tied | (hit & ohit & (ot == tc))
    take_o = ohit & (ot < tc)
    out_t = np.where(take_o, ot, tc).astype(np.float32)
    out_prim = np.where(take_o, full, prim)
    c = dict(u=np.where(take_o, oh[:, 1], 0).astype(np.uint32), v=np.where(take_o, oh[:, 2], 0).astype(np.uint32))
    return hit | ohit, out_t, out_prim, tied, c


def _case(mts, orc, name):
    """rays and the truths of a scene, computed once: a few thousand rays at every cylinder, the named rays, chords of the box"""
    if name in _cases:
        return _cases[name]
    sd, scene = _scene(mts, name, "host")
    blocks = scene.cylinder_blocks()
    cyl = [s for s, m in enumerate(sd.meshes) if m.shape_type == mts.abi.SHAPE_CYLINDER]
    rays = [CC.random_rays(blocks[s], 1500, seed=11 + s) for s in cyl]
    rays += [np.stack([r for r, _ in CC.named_rays(blocks[s]).values()]) for s in cyl]
    rng = np.random.RandomState(5)
    lo, hi = np.array(list(scene.sc.aabb_min)), np.array(list(scene.sc.aabb_max))
    o = lo + rng.rand(1000, 3) * (hi - lo); d = rng.normal(size=(1000, 3))
    rays.append(CC._rays(o, d / np.linalg.norm(d, axis=1, keepdims=True)))
    rays = np.concatenate(rays)
    geom = CC.Geometry(sd, list(scene.sc.aabb_min), list(scene.sc.aabb_max), blocks)
    assert geom.n_prims == scene.sc.n_tris
    c = dict(sd=sd, rays=rays, geom=geom, closest=CC.trace(geom, rays), shadow=CC.trace(geom, rays, shadow=True), blocks=blocks, cyl=cyl)
    c["mirror"] = _mirror(mts, orc, sd, scene, blocks, cyl, rays, False)
    c["mirror_shadow"] = _mirror(mts, orc, sd, scene, blocks, cyl, rays, True)
    _cases[name] = c
    return c


# --- 1. traversal ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", list(TREES))
@pytest.mark.parametrize("name", CC.SCENES)
def test_trace_rays_against_the_brute_force(gpu_lib, mts, orc, name, tree):
    c = _case(mts, orc, name)
    sd, scene = _scene(mts, name, tree)
    cam = mts.PerspectiveCamera.for_description(sd, 8, 8)
    it = mts.MIPathTracer(maxDepth=2); it.preprocess(scene, cam, sampleCount=1)
    amb = c["closest"].ambiguous.mean()
    print(name, tree, "rays", len(c["rays"]), "ambiguous %.3f %%" % (100 * amb), "hit %.1f %%" % (100 * c["closest"].hit.mean()))
    assert amb <= R.FRAGILE_CAP and c["shadow"].ambiguous.mean() <= R.FRAGILE_CAP
    block = GC.kernel_constants()["block"]
    for lean in (0, 7):
        it.set_tuning(lean_closest=lean)
        hits = it.trace_rays(c["rays"])
        assert it.stats()["rays_redone"] == 0, "no two primitives of these scenes tie"
        fails, worst = GC.check_closest(c["closest"], hits, "%s %s lean %d" % (name, tree, lean))
        print("lean", lean, "worst t %.3f bounds" % worst["t"][0])
        assert not fails, fails[:3]
        sh = it.trace_rays(c["rays"], shadow=True)
        fails = GC.check_shadow(c["shadow"], sh, "%s %s shadow" % (name, tree))
        assert not fails, fails[:3]
        on_cyl = np.isin(hits[:, 3], c["geom"].cyl_prim)
        assert on_cyl.sum() > 100 and (hits[on_cyl, 1] == 0).all() and (hits[on_cyl, 2] == 0).all(), "u = v = 0 on a cylinder"
        # the binary32 brute force of the whole scene, bit for bit: t and the primitive (and the oracle's u, v on a triangle)
        hit, t, prim, tied = c["mirror"][:4]
        assert tied.mean() <= R.FRAGILE_CAP
        ok = ~tied
        want = np.where(hit, prim, GC.MISS).astype(np.uint32)
        assert np.array_equal(hits[ok, 3], want[ok]), np.nonzero(ok & (hits[:, 3] != want))[0][:5]
        assert np.array_equal(hits[ok & hit, 0], bits(t[ok & hit])), "t equals the mirror's bit for bit"
        if len(c["mirror"]) > 4:
            assert np.array_equal(hits[ok & hit, 1], c["mirror"][4]["u"][ok & hit]) and np.array_equal(hits[ok & hit, 2], c["mirror"][4]["v"][ok & hit])
        assert np.array_equal(sh[:, 3] != 0, c["mirror_shadow"][0])
        # launches of 63, 64, 65 rays and a workgroup's worth plus one return what the long launch returned
        for n in (63, 64, 65, block + 1):
            assert np.array_equal(it.trace_rays(c["rays"][:n]), hits[:n]), n
            assert np.array_equal(it.trace_rays(c["rays"][:n], shadow=True), sh[:n]), n


@pytest.mark.parametrize("name", CC.SCENES)
def test_device_built_trees_equal_the_host_tree(gpu_lib, mts, name):
    host = CC.tree_words(_scene(mts, name, "host")[1])
    for tree in ("device_exact", "device_both"):
        sd, scene = _scene(mts, name, tree)
        kp = CC.kd_params(mts, name)
        if tree == "device_both":
            kp.exact_prim_threshold = 4
            host = CC.tree_words(mts.Scene(sd, kd_params=kp))
        dev = CC.tree_words(scene)
        assert np.array_equal(host[0], dev[0]) and np.array_equal(host[1], dev[1]), (name, tree)


def test_clip_in_a_kernel_equals_the_host(gpu_lib, mts):
    rng = np.random.RandomState(9)
    for name, p1, p2, r in CC.POSES:
        block = mts.cylinder_configure(mts.scenes.CylinderDesc(p1, p2, r))
        own = mts.cylinder_aabb(block)
        cells = list(CC.cells(block, own).values())
        lo = own[:3] - 0.2 + rng.rand(4000, 3) * (own[3:] - own[:3] + 0.4)
        hi = lo + rng.rand(4000, 3) * (own[3:] - own[:3] + 0.4) * rng.rand(4000, 1)
        boxes = np.concatenate([np.stack(cells), np.concatenate([lo, hi], axis=1).astype(np.float32)])
        a, va = mts.cylinder_clip(block, boxes)
        b, vb = mts.cylinder_clip(block, boxes, on_device=True)
        assert np.array_equal(va, vb) and np.array_equal(bits(a), bits(b)), name
        assert 0.1 < va.mean() < 0.95


# --- 2. the intersection record ---------------------------------------------------------------------------------------
def test_record_hook_equals_the_mirror_and_binary64(gpu_lib, mts):
    sd = mts.scenes.SceneDescription("cyl_record")
    grey = sd.lambertian(0.5)
    sd.add_cylinder((-0.4, 0.3, 0.1), (0.9, 1.2, -0.7), 0.25, bsdf=grey)
    sd.add_cylinder(to_world=CC.SHEARED, bsdf=grey)
    sd.add_cylinder((0.2, -0.1, 1.0), (0.2, -0.1, -1.5), 0.75, bsdf=grey)
    sd.add_lum(mts.abi.LUM_POINT, [1, 1, 1])
    it, scene = _prep(mts, sd)
    blocks = scene.cylinder_blocks()
    rng = np.random.RandomState(3)
    atan2 = lambda y, x: mts.devmath("atan2", y, x)
    tex = mts.scenes.Checkerboard(uscale=4.0, vscale=8.0).descriptor()
    worst = 0.0
    for s in range(3):
        D = blocks[s].astype(np.float64)
        M = D[0:12].reshape(3, 4)
        r, l = D[24], D[25]
        # around the seam phi = 0 (both sides, and on it), at both rims, anywhere
        phi = np.concatenate([rng.rand(3000) * 2 * np.pi, rng.normal(size=500) * 1e-3, -np.abs(rng.normal(size=500)) * 1e-6, np.zeros(8)])
        z = np.concatenate([rng.rand(3000) * l, rng.rand(1000) * l, np.linspace(0, l, 8)])
        z[3000:3200] = 0.0; z[3200:3400] = l
        loc = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
        p = (loc @ M[:, :3].T + M[:, 3]).astype(np.float32)
        prim = np.full(len(p), s, dtype=np.uint32)
        frame = it.shading_frame_eval(prim, p).reshape(-1, 3, 3)
        uv = it.uv_texture_eval(tex, prim, p)[:, :2]
        want = R.record32(blocks[s], p, atan2)
        for got, key in ((frame[:, 0], "s"), (frame[:, 1], "t"), (frame[:, 2], "n"), (uv, "uv")):
            ok = (bits(got) == bits(want[key])) | (np.isnan(got) & np.isnan(want[key]))
            assert ok.all(), (s, key, np.argwhere(~ok)[0], got[np.argwhere(~ok)[0][0]], want[key][np.argwhere(~ok)[0][0]])
        assert np.isfinite(frame).all() and (uv[:, 1] >= 0).all() and (uv[:, 1] <= 1).all()
        # mutations the comparison reports
        for mutation, key in (("uv_swapped", "uv"), ("phi_no_wrap", "uv"), ("normal_as_normal", "n"), ("frame_orthogonalised", "t")):
            if s != 1 and mutation in ("normal_as_normal", "frame_orthogonalised"):
                continue              # they differ from the record only where objectToWorld is not rigid: the sheared cylinder
            bad = R.record32(blocks[s], p, atan2, mutation)[key]
            got = {"uv": uv, "n": frame[:, 2], "t": frame[:, 1]}[key]
            assert (bits(got) != bits(bad)).any(), (s, mutation)
        # binary64: inside K_GEOM bounds, except the uv of points within reach of the seam (phi's sign decides the wrap)
        tr = R.record64(blocks[s], p)
        seam = np.abs(tr["phi"].v) <= 4 * EPS32 * tr["phi"].e
        seam |= np.abs(tr["phi"].v - 2 * np.pi) <= 1e-5
        for got, key in ((frame[:, 0], "s"), (frame[:, 1], "t"), (frame[:, 2], "n"), (uv, "uv")):
            for k in range(got.shape[1]):
                ratio = np.abs(got[:, k].astype(np.float64) - tr[key][k].v) / (EPS32 * tr[key][k].e + 1e-300)
                ratio = np.where((np.abs(got[:, k] - tr[key][k].v) == 0) | (seam & (key == "uv")), 0.0, ratio)
                worst = max(worst, ratio.max())
                assert ratio.max() <= GC.K_GEOM, (s, key, k, ratio.max(), int(np.argmax(ratio)))
        assert seam.mean() <= 0.2
    print("record: worst %.3f bounds" % worst)


# --- 3. a tie between a cylinder and a triangle ---------------------------------------------------------------------
def test_a_cylinder_and_a_tangent_triangle_tie(gpu_lib, mts):
    """the triangle lies in the plane x = 0.5, tangent to the cylinder of radius 0.5 about the z axis along the line x = 0.5,
    y = 0; rays along -x with y = 0 meet both at t = 2.5, exactly in binary32 (36 - 35 = 1 under the root)"""
    sd = mts.scenes.SceneDescription("cyl_tie")
    grey = sd.lambertian(0.5)
    sd.add_cylinder((0, 0, -1), (0, 0, 1), 0.5, bsdf=grey)
    sd.add_mesh([(0.5, -1, -1), (0.5, 1, -1), (0.5, 0, 2)], [(0, 1, 2)], bsdf=grey, face_normals=True)
    sd.add_lum(mts.abi.LUM_POINT, [1, 1, 1])
    it, scene = _prep(mts, sd)
    z = np.linspace(-0.9, 0.9, 256)
    rays = CC._rays(np.stack([np.full(256, 3.0), np.zeros(256), z], axis=1), np.tile([-1.0, 0.0, 0.0], (256, 1)))
    it.set_tuning(lean_closest=0)
    plain = it.trace_rays(rays)
    assert it.stats()["rays_redone"] == 0
    assert np.array_equal(plain[:, 0], bits(np.full(256, 2.5, dtype=np.float32))) and set(plain[:, 3]) <= {0, 1}
    it.set_tuning(lean_closest=7)
    lean = it.trace_rays(rays)
    assert np.array_equal(lean, plain), "the tied rays are redone with the mailbox"
    assert it.stats()["rays_redone"] > 0


# --- 4. refusals at the upload -----------------------------------------------------------------------------------------
def test_upload_refusals(gpu_lib, mts, orc):
    L, A = mts.lib(), mts.abi
    sd, scene = _scene(mts, "mixed", "host")
    cam = mts.PerspectiveCamera.for_description(sd, 8, 8)
    it = mts.MIPathTracer(maxDepth=2)
    blocks = scene.cylinder_blocks()
    err = lambda: L.mtsgpu_last_error(it._ctx).decode()
    assert L.mtsgpu_upload_scene(it._ctx, scene.ptr) != 0 and "mtsgpu_upload_scene_cylinders" in err()
    assert L.mtsgpu_upload_scene_tangents(it._ctx, scene.ptr, None, None) != 0 and "mtsgpu_upload_scene_cylinders" in err()
    assert L.mtsgpu_upload_scene_cylinders(it._ctx, scene.ptr, None, None, None) != 0 and "no cylinder blocks" in err()
    for k, v, why in ((24, 0.0, "radius > 0"), (25, -1.0, "length > 0"), (3, np.nan, "non-finite")):
        bad = blocks.copy(); bad[0, k] = v
        assert L.mtsgpu_upload_scene_cylinders(it._ctx, scene.ptr, None, None, A.ptr(bad, A.f32p)) != 0 and why in err(), why
    with pytest.raises(mts.MtsGpuError):
        it.trace_rays(np.zeros((1, 8), dtype=np.float32))          # nothing was uploaded
    it.preprocess(scene, cam, sampleCount=1)
    c = _case(mts, orc, "mixed")
    good = it.trace_rays(c["rays"][:512])
    # a refused upload after a good one leaves no scene behind; the good one again restores it
    assert L.mtsgpu_upload_scene(it._ctx, scene.ptr) != 0
    it.preprocess(scene, cam, sampleCount=1)
    assert np.array_equal(it.trace_rays(c["rays"][:512]), good)
    # a scene without a cylinder after one with: the plain kernels again, the same hits as a fresh context
    plain_sd = mts.scenes.cornell_c1()
    plain = mts.Scene(plain_sd)
    pcam = mts.PerspectiveCamera.for_description(plain_sd, 8, 8)
    rng = np.random.RandomState(1)
    o = rng.rand(777, 3) * 0.5 + 0.25; d = rng.normal(size=(777, 3))
    rays = CC._rays(o, d)
    it.preprocess(plain, pcam, sampleCount=1)
    fresh = mts.MIPathTracer(maxDepth=2); fresh.preprocess(plain, pcam, sampleCount=1)
    assert np.array_equal(it.trace_rays(rays), fresh.trace_rays(rays))


def test_families_not_served_on_a_cylinder_are_refused_by_name(gpu_lib, mts):
    """a cylinder takes a plain Lambertian; the mask, snow and cloth kernels do not build its record, so a scene with a cylinder
    refuses those calls, whichever shape the entry sits on"""
    S = mts.scenes

    def scene(make_bsdf, other=None):
        sd = S.SceneDescription("cyl_refused")
        sd.add_cylinder((0, 0, -1), (0, 0, 1), 0.5, bsdf=make_bsdf(sd))
        if other is not None:
            pos, tri, uv = S.tex_grid_mesh(2)
            sd.add_mesh(pos, tri, bsdf=other(sd), face_normals=True, texcoords=uv)
        sd.add_lum(mts.abi.LUM_POINT, [1, 1, 1])
        return sd
    grey = lambda sd: sd.lambertian(0.5)
    for make, why in ((lambda sd: sd.phong(30.0, 0.3, 0.5), "plain lambertian BSDF only; BSDF 0 is of type 5"),
                      (lambda sd: sd.twosided(sd.lambertian(0.5)), "under twosided"),
                      (lambda sd: sd.ward(0.1, 0.3), "plain lambertian BSDF only"),
                      (lambda sd: sd.dielectric(), "plain lambertian BSDF only")):
        with pytest.raises(mts.MtsGpuError, match=why):
            _prep(mts, scene(make))
    with pytest.raises(mts.MtsGpuError, match="mask BSDF is not served in a scene with a cylinder"):
        _prep(mts, scene(grey, lambda sd: sd.mask(sd.lambertian(0.5), 0.5)))
    with pytest.raises(mts.MtsGpuError, match="snow BRDFs are not served in a scene with a cylinder"):
        _prep(mts, scene(grey, lambda sd: sd.wiscombe()))
    import cloth_cases
    weave = cloth_cases.weaves(mts)[0][1]
    with pytest.raises(mts.MtsGpuError, match="cloth BRDF is not served in a scene with a cylinder"):
        _prep(mts, scene(grey, lambda sd: sd.irawan(weave)))
    with pytest.raises(mts.MtsGpuError, match="a cylinder without a BSDF"):
        _prep(mts, scene(lambda sd: -1))
    # the same entries in a scene with a sphere in the cylinder's place are served as ever: the refusals are the cylinder's

    def control(make_bsdf, other=None):
        sd = S.SceneDescription("sphere_served")
        sd.add_sphere((0, 0, 0), 0.5, bsdf=make_bsdf(sd))
        if other is not None:
            pos, tri, uv = S.tex_grid_mesh(2)
            sd.add_mesh(pos, tri, bsdf=other(sd), face_normals=True, texcoords=uv)
        sd.add_lum(mts.abi.LUM_POINT, [1, 1, 1])
        it, _ = _prep(mts, sd)
        assert it.render()
    control(lambda sd: sd.phong(30.0, 0.3, 0.5))
    control(lambda sd: sd.twosided(sd.lambertian(0.5)))
    control(grey, lambda sd: sd.mask(sd.lambertian(0.5), 0.5))
    control(grey, lambda sd: sd.wiscombe())
    control(grey, lambda sd: sd.irawan(weave))
    control(lambda sd: -1)


# --- 5. frames -------------------------------------------------------------------------------------------------------
def test_a_scene_without_cylinders_renders_the_same_bytes_through_the_cylinder_upload(gpu_lib, mts):
    L, A = mts.lib(), mts.abi
    sd = mts.scenes.cornell_c1()
    it, scene = _prep(mts, sd)
    assert it.render()
    base = it.film()
    it2, _ = _prep(mts, sd, scene=scene)
    it2._chk(L.mtsgpu_upload_scene_cylinders(it2._ctx, scene.ptr, None, None, None), "upload_scene_cylinders")
    it2.clear_film()
    assert it2.render()
    assert base[..., :3].max() > 0 and np.array_equal(bits(base), bits(it2.film()))


def _tube_scene(mts, reflectance, sky=False):
    """tex_scene with a cylinder lying under the orthographic camera: a path meets its outside once at most"""
    S = mts.scenes
    sd = S.SceneDescription("tex_cylinder")
    sd.add_cylinder((-0.7, -0.1, 0.1), (0.75, -0.05, -0.2), 0.45, bsdf=sd.lambertian(reflectance))
    sd.point_light((0.3, 1.5, -0.2), (5.0, 4.0, 3.0))
    sd.add_lum(mts.abi.LUM_CONSTANT, [0.25, 0.25, 0.25])
    sd.camera = dict(origin=(0.0, 2.0, 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), ortho_scale=1.0)
    sd.max_depth = 2
    return sd


@pytest.mark.parametrize("integrator", ["path", "direct"])
def test_checkerboard_on_a_cylinder_is_bright_or_dark_times_the_white_scene(gpu_lib, mts, integrator):
    """bright and dark are distinct powers of two, and a path meets the tube once at most: every sample is the white scene's
    times one of the two colours, bit for bit (a power of two commutes with every rounding), or the white scene's own (a miss).
    Which colour belongs where is the record's business: test_record_hook_equals_the_mirror_and_binary64."""
    S = mts.scenes
    tex = S.Checkerboard(bright=0.5, dark=0.125, uscale=3.0, vscale=8.0)
    res, spp = 32, 4
    samples = _all_samples(res, spp)
    make = (lambda: mts.MIDirectIntegrator()) if integrator == "direct" else (lambda: None)
    it, scene = _prep(mts, _tube_scene(mts, tex), res=res, spp=spp, integ=make())
    assert scene.has_cylinders and scene.bsdf_slot_texture is not None
    li = it.li_samples(samples)
    li_w = _prep(mts, _tube_scene(mts, 1.0), res=res, spp=spp, integ=make())[0].li_samples(samples)
    assert np.isfinite(li).all() and np.array_equal(bits(li[:, 3:6]), bits(li_w[:, 3:6]))
    W = li_w[:, :3]
    is_b = (bits(li[:, :3]) == bits(W * F(0.5))).all(axis=1)
    is_d = (bits(li[:, :3]) == bits(W * F(0.125))).all(axis=1)
    is_w = (bits(li[:, :3]) == bits(W)).all(axis=1)
    print(integrator, "bright", is_b.sum(), "dark", is_d.sum(), "miss", is_w.sum(), "neither", (~is_b & ~is_d & ~is_w).sum())
    assert (is_b | is_d | is_w).all()
    assert (is_b & ~is_d).sum() > 100 and (is_d & ~is_b).sum() > 100 and is_w.sum() > 100


@pytest.mark.parametrize("sky", [False, True])
def test_one_film_across_the_ways_of_driving_the_bounces(gpu_lib, mts, sky):
    """a cylinder next to a sphere and a textured mesh, under a constant environment or the sky, in both integrators: host- and device-driven
    bounces, ragged passes, the closest-hit kernel with the mailbox, two tile parts and a device group give the same bytes"""
    S = mts.scenes
    sd = S.tex_scene(S.Checkerboard(bright=0.5, dark=0.125, uscale=3.0, vscale=3.0), shape="grid", sky=sky)
    sd.add_cylinder((-0.6, 0.3, 0.2), (0.5, 0.45, -0.3), 0.2, bsdf=sd.lambertian(S.Checkerboard(bright=0.8, dark=0.1, uscale=2.0, vscale=6.0)))
    sd.add_sphere((0.4, 0.25, 0.45), 0.2, bsdf=sd.lambertian(0.6))
    sd.max_depth = 4
    scene = mts.Scene(sd)
    assert scene.has_cylinders
    res, spp = 32, 4
    cam = mts.PerspectiveCamera.for_description(sd, res, res)

    def render(integ, drive, part=0, n_parts=1):
        it = mts.MIPathTracer(maxDepth=sd.max_depth) if integ == "path" else mts.MIDirectIntegrator(*integ)
        it.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=5)
        if drive == 1: it.set_tuning(sync_free=0)
        elif drive == 2: it.set_tuning(sync_free=0); it.set_options(max_paths=spp * (res * res // 3 + 1))
        elif drive == 3: it.set_tuning(sync_free=1, shade_fused=0)
        elif drive == 4: it.set_tuning(lean_closest=0)
        if n_parts > 1:
            it.set_tiles(16, part, n_parts)
        assert it.render()
        return it.film()
    for integ in ("path", (1, 1)):
        base = render(integ, 0)
        assert np.isfinite(base).all() and (base[..., :3] > 0).any()
        for drive in (1, 2, 3, 4):
            assert np.array_equal(bits(base), bits(render(integ, drive))), (integ, "drive %d differs from the device-driven frame" % drive)
        total = sum(render(integ, 0, part, 2) for part in range(2))
        assert np.array_equal(bits(base), bits(total)), (integ, "two tile parts do not add up to the frame")
        g = mts.DeviceGroup([0, 0], maxDepth=sd.max_depth)
        g.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=5)
        if integ != "path":
            for i in range(len(g)):
                assert mts.lib().mtsgpu_set_direct_integrator(g.member(i), *integ) == 0
        assert g.render(block_size=16, ordered_reduce=True)
        assert np.array_equal(bits(base), bits(g.film())), (integ, "the two-member group's film differs")
        g.close()


def _lit_tube(mts, albedo, light_dir, intensity):
    sd = mts.scenes.SceneDescription("lit_cylinder")
    sd.add_cylinder((-0.7, -0.1, 0.1), (0.75, -0.05, -0.2), 0.45, bsdf=sd.lambertian(albedo))
    l = sd.directional_light(light_dir, intensity)
    sd.camera = dict(origin=(0.0, 2.0, 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), ortho_scale=1.0)
    sd.max_depth = 2
    return sd, np.asarray(sd.lum_params[l][3:6], dtype=np.float32)


def test_lambertian_cylinder_under_a_directional_light_in_direct(gpu_lib, mts):
    """every radiance sample of `direct` equals intensity x albedo / pi x cos at that sample's camera ray, the hit and the normal
    from the binary64 restatement.  The tolerance is derived, not chosen: K_GEOM first-order bounds of the value (the bounds of the
    record's normal through the dot product and the three factors), plus what the hit point's own error moves the normal by:
    |dp| <= K_GEOM x bound(t) x |d| + 3 x 2^-23 x |p| (t, the product t d, the sum), and the unit normal of a tube of radius r
    turns by |dp| / r at most.  The tube is convex from outside, so no lit point is shadowed, and nothing else emits."""
    from ref64_sky import E
    albedo, intensity = (0.5, 0.25, 0.75), (2.0, 3.0, 4.0)
    sd, ldir = _lit_tube(mts, albedo, (0.3, -1.0, 0.2), intensity)
    res, spp = 32, 4
    samples = _all_samples(res, spp)
    it, scene = _prep(mts, sd, res=res, spp=spp, integ=mts.MIDirectIntegrator())
    li = it.li_samples(samples)
    rays = _prep(mts, sd, res=res, spp=spp, integ=mts.MIDirectIntegrator())[0].camera_rays(samples.astype(np.int32))
    block = scene.cylinder_blocks()[0]
    r8 = np.ascontiguousarray(rays[:, :8])
    tr = R.intersect64(block, r8, r8[:, 3], r8[:, 7])
    hit = tr["hit"]
    o, d = r8[:, 0:3].astype(np.float64), r8[:, 4:7].astype(np.float64)
    p = o + tr["t"].v[:, None] * d
    rec = R.record64(block, np.where(hit[:, None], p, 0.0).astype(np.float32))
    L = -ldir.astype(np.float64)
    cos = rec["n"][0] * E(L[0]) + rec["n"][1] * E(L[1]) + rec["n"][2] * E(L[2])
    dp = GC.K_GEOM * EPS32 * tr["t"].e * np.linalg.norm(d, axis=1) + 3 * EPS32 * np.abs(p).max(axis=1)
    dcos = dp / float(block[24])
    fragile = tr["fragile"] | (hit & (np.abs(cos.v) <= 4 * EPS32 * cos.e + dcos))
    print("samples", len(li), "on the tube", int(hit.sum()), "lit", int((hit & (cos.v > 0)).sum()), "fragile", int(fragile.sum()))
    assert fragile.mean() <= R.FRAGILE_CAP
    assert np.isfinite(li).all()
    sure = ~fragile
    dark = sure & (~hit | (cos.v <= 0))
    assert (li[dark, :3] == 0).all(), "a miss and a point facing away from the light are black"
    assert np.array_equal(li[sure, 3] != 0, hit[sure]), "alpha is 1 on the tube and 0 beside it"
    lit = sure & hit & (cos.v > 0)
    assert lit.sum() > 1000
    worst = 0.0
    inv_pi = float(F(0.31830988618379067154))
    for ch in range(3):
        val = E(float(F(intensity[ch]))) * (E(float(F(albedo[ch]))) * E(inv_pi)) * cos
        tol = GC.K_GEOM * EPS32 * val.e + float(F(intensity[ch])) * float(F(albedo[ch])) * inv_pi * dcos
        ratio = np.abs(li[:, ch].astype(np.float64) - val.v)[lit] / tol[lit]
        worst = max(worst, ratio.max())
    print("worst ratio of |Li - I rho / pi cos| to the derived tolerance: %.3f" % worst)
    assert worst <= 1.0


def test_the_view_from_inside_the_tube(gpu_lib, mts):
    """a camera on the axis looking at the wall: every camera ray meets the tube with its FAR root (the binary64 restatement says
    so), alpha is 1, and the plain Lambertian, seen from behind (wi.z < 0 in the record's frame, whose normal points outward), is
    black although a point light and a constant environment are there"""
    sd = mts.scenes.SceneDescription("inside_cylinder")
    sd.add_cylinder((-2.0, 0.0, 0.0), (2.0, 0.1, 0.0), 0.5, bsdf=sd.lambertian(0.8))
    sd.point_light((0.3, 0.0, 0.1), (5.0, 4.0, 3.0))
    sd.add_lum(mts.abi.LUM_CONSTANT, [0.25, 0.25, 0.25])
    sd.camera = dict(origin=(0.0, 0.02, 0.0), target=(0.1, 0.6, 0.3), up=(1.0, 0.0, 0.0), fov=40.0)
    sd.max_depth = 3
    res, spp = 16, 4
    samples = _all_samples(res, spp)
    for integ in (None, mts.MIDirectIntegrator()):
        it, scene = _prep(mts, sd, res=res, spp=spp, integ=integ)
        li = it.li_samples(samples)
        rays = _prep(mts, sd, res=res, spp=spp)[0].camera_rays(samples.astype(np.int32))
        r8 = np.ascontiguousarray(rays[:, :8])
        tr = R.intersect64(scene.cylinder_blocks()[0], r8, r8[:, 3], r8[:, 7])
        assert not tr["fragile"].any() and tr["hit"].all() and not tr["first"].any(), "every ray takes the far root"
        assert (li[:, 3] == 1).all() and (li[:, :3] == 0).all()
    # the same tube from outside is lit: the black above is the side, not the scene
    sd.camera = dict(origin=(0.0, 3.0, 0.5), target=(0.0, 0.0, 0.0), up=(1.0, 0.0, 0.0), fov=40.0)
    sd.lum_params[0][3:6] = np.float32([0.3, 2.0, 0.1])
    li = _prep(mts, sd, res=res, spp=spp)[0].li_samples(samples)
    assert (li[:, :3] > 0).mean() > 0.2
