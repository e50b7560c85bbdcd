"""Per-vertex colours and the `vertexcolors` texture on the device: the interpolation hook against the float32 mirror and the
binary64 restatement (tests/ref64_vcol.py), the slot substitution against mtsgpu_bsdf_eval, what mtsgpu_set_vertex_colors
refuses, frames that must not change, an end-to-end check without the oracle, and one film across the drivers.  The CPU side
(loader, colour pool, ABI, exclusion cap) is tests/test_vcol.py."""
import ctypes as C

import numpy as np
import pytest

import ref64_vcol
import vcol_cases
from conftest import bits

pytestmark = pytest.mark.gpu
F = np.float32
TWOSIDED = 0x100


@pytest.fixture(scope="module")
def device(gpu_lib, mts):
    return mts.MIPathTracer(maxDepth=2)


def _prep(mts, sd, scene=None, res=32, spp=4, integ=None, **kw):
    scene = mts.Scene(sd, **kw) if scene is None else scene
    cam = mts.PerspectiveCamera.for_description(sd, res, res)
    it = mts.MIPathTracer(maxDepth=sd.max_depth) if integ is None else integ
    it.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=21)
    return it, scene


def _all_samples(res, spp):
    y, x, j = np.meshgrid(np.arange(res), np.arange(res), np.arange(spp), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), j.ravel()], axis=1).astype(np.uint32)


# --- 1. interpolation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", ["host", "gpu_binning", "gpu_exact"])
def test_interpolation_is_the_mirror_bit_for_bit(gpu_lib, mts, tree):
    """two coloured shared-vertex meshes (4 x 4 and 3 x 3 cells) around an uncoloured one: the hook returns the float32
    mirror of skdtree.h:364,417-421 bit for bit, within the restatement's bound of the binary64 value, 0 where a mesh has no
    colours -- on the host flattener's tree and on the trees the device builds"""
    S = mts.scenes
    sd = S.vcol_grid(4)
    plain = S.vcol_grid(2, colors=None).meshes[0]
    sd.add_mesh(plain.positions + F(4), plain.triangles, bsdf=sd.lambertian(0.5), face_normals=True)
    g = S.vcol_grid(3, seed=9).meshes[0]
    sd.add_mesh(g.positions - F(4), g.triangles, bsdf=sd.meshes[0].bsdf, face_normals=False, colors=g.colors)
    kp = mts.abi.KdParams()
    if tree != "host":
        kp.exact_prim_threshold = 16          # the 58 triangles go through the binning phase first
    it, scene = _prep(mts, sd, kd_params=kp, gpu_binning=tree != "host", gpu_exact=tree == "gpu_exact")
    A = scene.arrays()
    col, has = scene.vertex_colors()
    assert has.tolist() == [1, 0, 1]
    n_prims = sd.n_tris
    prim, u, v = vcol_cases.barycentric_records(np.random.RandomState(4), n_prims, 4096)
    got = it.vertex_color_eval(prim, np.stack([u, v], axis=1))
    want = ref64_vcol.color32(col, A["tri_idx"], prim, u, v)
    off = A["shape_tri_offset"]
    plain_prim = (prim >= off[1]) & (prim < off[2])
    assert plain_prim.sum() > 100 and not got[plain_prim].any()
    sel = ~plain_prim
    assert np.array_equal(bits(got[sel]), bits(want[sel])), "%d records differ from the float32 mirror" % (bits(got[sel]) != bits(want[sel])).any(axis=1).sum()
    val, bound = ref64_vcol.color64(col, A["tri_idx"], prim, u, v)
    ok = ref64_vcol.within_bound(got, val, bound)
    print("worst |device - binary64| / bound: %.3g" % (np.abs(got[sel] - val[sel]) / (bound[sel] * ref64_vcol.TOL32 + ref64_vcol.DENORM)).max())
    assert ok[sel].all()
    # the hook's own refusals
    with pytest.raises(mts.MtsGpuError, match="out of range"):
        it.vertex_color_eval([n_prims], [[0.1, 0.1]])
    # the count is refused before a record is read, so one record's memory stands in for 2^24 + 1 of them
    A, p1, f3 = mts.abi, np.zeros(1, np.uint32), np.zeros(3, np.float32)
    with pytest.raises(mts.MtsGpuError, match=r"at most 2\^24 query records per call.*code -1"):
        it._chk(mts.lib().mtsgpu_vertex_color_eval(it._ctx, (1 << 24) + 1, A.ptr(p1, A.u32p), A.ptr(f3, A.f32p), A.ptr(f3, A.f32p)), "vertex_color_eval")
    it.set_vertex_colors()
    with pytest.raises(mts.MtsGpuError, match="no vertex colours"):
        it.vertex_color_eval([0], [[0.1, 0.1]])


# --- 2. substitution ---------------------------------------------------------------------------------------------------
def _blocks(mts):
    """one parameter block per type 0..8, every float distinct so that a wrong offset shows"""
    sd = mts.scenes.SceneDescription("blocks")
    ids = [sd.lambertian(0.3, 0.5, 0.7), sd.dielectric(1.5, 1.0, refl=0.9, trans=0.8), sd.roughmetal(0.2, refl=0.85),
           sd.microfacet(0.2, 0.4, 0.5, rd=0.6, rs=0.7), sd.mirror(0.75), sd.phong(15.0, rd=0.35, rs=0.45, kd=0.7, ks=0.6),
           sd.roughglass(0.2, refl=0.9, trans=0.8), sd.difftrans(0.55), sd.ward(0.2, 0.2, rd=(0.3, 0.4, 0.5), rs=(0.25, 0.2, 0.15), kd=0.8, ks=0.9)]
    P = [sd.bsdf_params[i].copy() for i in ids]
    for t, p in enumerate(P):
        for o in mts.abi.BSDF_COLOR_SLOTS[t]:
            p[o:o + 3] = p[o] * np.float32([1.0, 0.9, 0.8])
    return P


@pytest.mark.parametrize("btype", range(9))
def test_coloured_slots_equal_overwritten_blocks(device, mts, btype):
    """mtsgpu_bsdf_eval_colored(P, slots, c) == mtsgpu_bsdf_eval(P with the slots overwritten by c), bit for bit: every slot
    combination, with and without the twosided adapter, f / pdf / sample; mask 0 == mtsgpu_bsdf_eval(P)"""
    P = _blocks(mts)[btype]
    offs = mts.abi.BSDF_COLOR_SLOTS[btype]
    rng = np.random.RandomState(50 + btype)
    n = 2048

    def dirs(k):
        d = rng.normal(size=(k, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        return d.astype(np.float32)
    wi, wo, s = dirs(n), dirs(n), rng.rand(n, 2).astype(np.float32)
    color = np.float32([0.21, 0.62, 0.93])
    nonzero = 0
    for two in (0, TWOSIDED):
        for mask in range(1 << len(offs)):
            Q = P.copy()
            for k, o in enumerate(offs):
                if mask >> k & 1:
                    Q[o:o + 3] = color
            for op in (0, 1, 2):
                aux = s if op == 2 else wo
                got = device.bsdf_eval_colored(btype | two, P, mask, color, op, wi, aux)
                want = device.bsdf_eval(btype | two, Q, op, wi, aux)
                assert np.array_equal(bits(got), bits(want)), (btype, two, mask, op, int((bits(got) != bits(want)).any(axis=1).sum()))
                nonzero += int((want[:, :7] != 0).any())
                if mask and op != 1:
                    # the colour arrives: the block with and without it give different values somewhere (f of the two
                    # delta BSDFs is zero whatever the block holds)
                    plain = device.bsdf_eval(btype | two, P, op, wi, aux)
                    if op == 2 or plain[:, :3].any():
                        assert not np.array_equal(bits(plain), bits(got)), (btype, two, mask, op)
                    else:
                        assert btype in (1, 4)
    assert nonzero > 0
    with pytest.raises(mts.MtsGpuError, match="beyond"):
        device.bsdf_eval_colored(btype, P, 1 << len(offs), color, 0, wi[:1], wo[:1])


def test_coloured_hook_refuses_the_composite(device, mts):
    with pytest.raises(mts.MtsGpuError, match="composite"):
        device.bsdf_eval_colored(9, np.zeros(16), 0, [1, 1, 1], 0, [[0, 0, 1]], [[0, 0, 1]])
    with pytest.raises(mts.MtsGpuError, match="bad BSDF type"):
        device.bsdf_eval_colored(0x200, np.zeros(16), 0, [1, 1, 1], 0, [[0, 0, 1]], [[0, 0, 1]])
    # the count is refused before a record is read, so one record's memory stands in for 2^24 + 1 of them
    A, P, q, out = mts.abi, np.full(16, 0.5, np.float32), np.zeros(6, np.float32), np.zeros(8, np.float32)
    with pytest.raises(mts.MtsGpuError, match=r"at most 2\^24 query records per call.*code -1"):
        device._chk(mts.lib().mtsgpu_bsdf_eval_colored(device._ctx, 0, A.ptr(P, A.f32p), 1, A.ptr(q, A.f32p), 0, (1 << 24) + 1, A.ptr(q, A.f32p),
                                                       A.ptr(out, A.f32p)), "bsdf_eval_colored")


# --- 3. refusals -------------------------------------------------------------------------------------------------------
def test_set_vertex_colors_refusals(gpu_lib, mts):
    S = mts.scenes
    sd = S.vcol_grid(4)                               # BSDF 0: coloured lambertian on mesh 0
    comp_child = sd.phong(10.0, rd=0.2, rs=0.3)       # BSDF 1
    comp = sd.composite([0.5, 0.5], [comp_child, comp_child])    # BSDF 2
    g = sd.meshes[0]
    sd.add_mesh(g.positions + F(3), g.triangles, bsdf=comp, face_normals=True)            # shape 1, no colours
    sd.add_sphere((0, 3, 0), 0.4, bsdf=sd.lambertian(0.5))                                # shape 2, BSDF 3
    it, scene = _prep(mts, sd)
    col, has = scene.vertex_colors()
    good = np.uint32([1, 0, 0, 0])

    def attempt(c=col, h=has, m=good):
        try:
            it.set_vertex_colors(c, h, m)
        except mts.MtsGpuError as e:
            assert "code -1" in str(e), e
            return str(e)
        return ""
    assert attempt() == ""
    assert "beyond the 1 texture slot" in attempt(m=np.uint32([2, 0, 0, 0]))
    assert "beyond the 0 texture slot" in attempt(m=np.uint32([1, 0, 1, 0]))          # the composite has no slot of its own
    msg = attempt(m=np.uint32([1, 2, 0, 0]))
    assert "BSDF 2" in msg and "composite child 0" in msg, msg
    msg = attempt(m=np.uint32([1, 0, 0, 1]))
    assert "shape 2" in msg and "sphere" in msg, msg
    msg = attempt(h=np.uint32([0, 0, 0]))
    assert "shape 0" in msg and "the mesh has none" in msg, msg
    for bad in (np.nan, np.inf):
        c = col.copy(); c[7, 1] = bad
        msg = attempt(c=c)
        assert "non-finite colour at vertex 7" in msg, msg
    # a non-finite row of a mesh WITHOUT colours is ignored, as the header says
    c = col.copy(); c[g.positions.shape[0] + 2] = np.nan
    assert attempt(c=c) == ""
    assert "both be given or both be NULL" in attempt(h=None)
    # a refused call leaves the colours switched off, and the context usable
    attempt(m=np.uint32([2, 0, 0, 0]))
    with pytest.raises(mts.MtsGpuError, match="no vertex colours"):
        it.vertex_color_eval([0], [[0.1, 0.1]])
    assert attempt() == "" and it.render()
    # before any scene
    fresh = mts.MIPathTracer(maxDepth=2)
    with pytest.raises(mts.MtsGpuError, match="before mtsgpu_upload_scene"):
        fresh.set_vertex_colors(col, has, good)
    # the Scene mirror passes a coloured slot on a mesh without colours on, and the library refuses it
    bad = S.vcol_grid(4, colors=None)
    with pytest.raises(mts.MtsGpuError, match="the mesh has none"):
        _prep(mts, bad)


# --- 4. no behaviour change --------------------------------------------------------------------------------------------
def _frame(it, res=32, spp=4):
    assert it.render()
    film = it.film()
    return film, it.li_samples(_all_samples(res, spp))


def test_unused_colours_and_black_colours_change_nothing(gpu_lib, mts):
    S = mts.scenes
    base_film, base_li = _frame(_prep(mts, S.vcol_grid(4, material="white", colors=None))[0])
    assert (base_film[..., :3] > 0).any()
    # colours on the mesh, no BSDF uses them
    it, scene = _prep(mts, S.vcol_grid(4, material="white"))
    assert scene.vertex_colors()[0] is not None and scene.bsdf_color_slots is None
    film, li = _frame(it)
    assert np.array_equal(bits(film), bits(base_film)) and np.array_equal(bits(li), bits(base_li))
    # a coloured scene after set_vertex_colors(NULL...) is the scene of its block: reflectance 1
    it, scene = _prep(mts, S.vcol_grid(4, material="lambertian"))
    coloured_film, _ = _frame(it)
    assert not np.array_equal(bits(coloured_film), bits(base_film))
    it.set_vertex_colors()
    it.clear_film()                                   # render() adds to the film of the frame before
    film, li = _frame(it)
    assert np.array_equal(bits(film), bits(base_film)) and np.array_equal(bits(li), bits(base_li))
    # all-zero colours under a coloured Lambertian: the constant-black scene
    black_film, black_li = _frame(_prep(mts, S.vcol_grid(4, material="black", colors=None))[0])
    film, li = _frame(_prep(mts, S.vcol_grid(4, material="lambertian", colors="zero"))[0])
    assert np.array_equal(bits(film), bits(black_film)) and np.array_equal(bits(li), bits(black_li))
    assert not black_film[..., :3].any()


# --- 5. end to end, without the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("material, white", [("lambertian", "white"), ("phong", "phong_white")])
def test_radiance_is_the_colour_times_the_white_scene(gpu_lib, mts, material, white):
    """Li(sample) = its.color (x) Li_white(sample) per channel, on the planar grid under one point light, path with
    maxDepth = 2: the only radiance a sample collects is the direct light at the camera hit (the light cannot be hit, and
    depth 2 ends the loop before a second luminaire sample, path.cpp:96-98), so with reflectance factor c

        Li = ((thr * value) * ((c * k) * cos)) * weight            (path.cpp:108-124; k = 1 / pi for the Lambertian,
                                                                    specRef for the Phong lobe over a black diffuse part)

    in which c moves through k = 4 rounded products (c * k, * cos, (thr * value) *, * weight); the white scene runs the same
    chain with c = 1, whose first product is exact: 3 roundings.  Both chains share every other factor bit for bit, so
    |Li - c Li_white| <= gamma(4 + 3) c Li_white, gamma(n) = n U / (1 - n U), U = 2^-24.  The colour itself: the device's
    value lies within ref64_vcol's bound of the binary64 value AT THE DEVICE'S (u, v), which lie within vcol_cases' reach
    of the exact barycentrics of the point below the raster position: times the colour gradient of the cell.  Samples within
    that reach of a cell edge are excluded (at most 1 %, checked on the CPU side too)."""
    geo = vcol_cases.GridGeometry(mts, material)
    res, spp = vcol_cases.E2E_RES, vcol_cases.E2E_SPP
    samples = _all_samples(res, spp)
    it, scene = _prep(mts, geo.sd, res=res, spp=spp)
    li = it.li_samples(samples)
    li_w = _prep(mts, mts.scenes.vcol_grid(vcol_cases.E2E_CELLS, material=white), res=res, spp=spp)[0].li_samples(samples)
    assert np.array_equal(bits(li[:, 3:6]), bits(li_w[:, 3:6])), "alpha and raster position are those of the white scene"
    hit = geo.locate(li[:, 4:6])
    assert hit.excluded.mean() <= vcol_cases.MAX_EXCLUDED
    keep = ~hit.excluded
    col = geo.mesh.colors
    val, bound = ref64_vcol.color64(col, geo.mesh.triangles, hit.prim, hit.u.astype(np.float32), hit.v.astype(np.float32))
    # (u, v) above were rounded to binary32 for the restatement's signature: that rounding is inside the reach too
    reach_u, reach_v = hit.du + vcol_cases.U24, hit.dv + vcol_cases.U24
    c_tol = bound * ref64_vcol.TOL32 + ref64_vcol.gradient_bound(col, geo.mesh.triangles, hit.prim, reach_u, reach_v)
    W = li_w[:, :3].astype(np.float64)
    assert (W[keep] > 0).all() and np.isfinite(li).all()
    n_round = 4 + 3
    gamma = n_round * vcol_cases.U24 / (1 - n_round * vcol_cases.U24)
    tol = W * c_tol + gamma * np.abs(val * W) + 2.0 ** -149
    err = np.abs(li[:, :3].astype(np.float64) - val * W)
    ratio = (err / tol)[keep]
    print("%s: %d of %d samples excluded, worst |Li - c Li_white| / tolerance %.3g, colour part %.3g of the tolerance"
          % (material, (~keep).sum(), len(keep), ratio.max(), (W * c_tol / tol)[keep].max()))
    assert ratio.max() <= 1.0, (material, int(np.argmax(ratio.max(axis=1))))
    # the check can fail: the neighbour cell's colours, or a swapped channel, are far outside
    wrong = val[:, [1, 2, 0]] * W
    assert (np.abs(li[:, :3] - wrong) > tol)[keep].mean() > 0.9


# --- 6. one film across drivers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sky", [False, True])
def test_drivers_tile_parts_group_and_direct_give_one_film(gpu_lib, mts, sky):
    sd = mts.scenes.cornell_vcol(sky=sky)
    scene = mts.Scene(sd)
    res, spp = 32, 4
    cam = mts.PerspectiveCamera.for_description(sd, res, res)

    def render(integ, drive, part=0, n_parts=1):
        it = mts.MIPathTracer(maxDepth=sd.max_depth) if integ == "path" else mts.MIDirectIntegrator(*integ)
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
        g = mts.DeviceGroup([0, 0], maxDepth=sd.max_depth)
        g.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=5)
        if integ != "path":
            for i in range(len(g)):
                assert mts.lib().mtsgpu_set_direct_integrator(g.member(i), *integ) == 0
        assert g.render(block_size=16, ordered_reduce=True)
        assert np.array_equal(bits(base), bits(g.film())), (integ, "the two-member group's film differs")
        g.close()
    # the colours matter in this frame: without them the same scene renders another film
    it = mts.MIPathTracer(maxDepth=sd.max_depth)
    it.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=5)
    it.set_vertex_colors()
    assert it.render() and not np.array_equal(bits(it.film()), bits(render("path", 0)))
