"""Texture coordinates and the checkerboard / grid textures on the device: the read-out hook against the float32 mirror of
tests/ref64_tex.py bit for bit, the generalised per-hit block builder against mtsgpu_bsdf_eval, what mtsgpu_set_uv_textures
refuses, frames that must not change, radiance with no tolerance, and one film across the drivers.  The CPU side (loader, uv
pool, ABI, restatement, mutations, cap) is tests/test_tex.py."""
import numpy as np
import pytest

import ref64_tex as R
import tex_cases
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


# --- 1. the read-out hook ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", ["host", "gpu_binning", "gpu_exact"])
def test_uv_and_texture_value_are_the_mirror_bit_for_bit(gpu_lib, mts, tree):
    """its.uv and the texture's value for random and boundary records on the floor, the boundary strip, a mesh without
    texcoords (uv = (0, 0)) and the sphere, every shared texture, on the host flattener's tree and on the device-built ones"""
    sd = tex_cases.hook_scene(mts)
    kp = mts.abi.KdParams()
    if tree != "host":
        kp.exact_prim_threshold = 16
    it, scene = _prep(mts, sd, kd_params=kp, gpu_binning=tree != "host", gpu_exact=tree == "gpu_exact")
    A = scene.arrays()
    pool, has = scene.vertex_texcoords()
    assert has.tolist() == [1, 1, 0, 0]
    # the scene has no textured slot, so the Scene mirror made no call: hand the texcoords over
    it.set_uv_textures(pool, has)
    off, tri = A["shape_tri_offset"], A["tri_idx"]
    rng = np.random.RandomState(4)
    prim, u, v = tex_cases.triangle_records(rng, off[0], off[1] - off[0], 3000)
    sprim = np.arange(off[1], off[2], dtype=np.uint32)
    nprim, nu, nv = tex_cases.triangle_records(rng, off[2], off[3] - off[2], 200)
    prim, u, v = np.concatenate([prim, sprim, nprim]), np.concatenate([u, np.zeros(len(sprim), F), nu]), np.concatenate([v, np.zeros(len(sprim), F), nv])
    rec = np.stack([u, v, np.zeros_like(u)], axis=1)
    strip = slice(3000, 3000 + len(sprim))
    SP = A["shape_params"][3]
    pts = tex_cases.sphere_points(rng, 2000, SP[0:3], SP[3])
    assert np.array_equal(SP[0:3], np.float32(tex_cases.SPHERE_CENTER)) and SP[3] == F(tex_cases.SPHERE_RADIUS)
    for name, tex in sorted(tex_cases.textures().items()):
        st = tex_cases.scene_texture(mts.scenes, tex)
        got = it.uv_texture_eval(st, prim, rec)
        d = R.decide_triangles(tex, pool, tri, prim, u, v)
        assert np.array_equal(bits(got[:, :2]), bits(d.uv32)), (name, int((bits(got[:, :2]) != bits(d.uv32)).any(axis=1).sum()))
        assert np.array_equal(bits(got[:, 2:]), bits(d.value32)), (name, int((bits(got[:, 2:]) != bits(d.value32)).any(axis=1).sum()))
        assert not got[-200:, :2].any(), "a mesh without texcoords gives uv = (0, 0)"
        keep = ~d.fragile
        assert np.array_equal(got[keep, 2:], R.value(tex, d.bright64)[keep]) and d.fragile.mean() <= tex_cases.MAX_FRAGILE
        if name.endswith("_id"):
            # b = (1, 0, 0): vertex 0's texcoord comes back as it is (but for the sign of a zero: -0 + 0 * t1 is +0)
            assert np.array_equal(got[strip, :2], pool[tri[sprim, 0]]), "vertex 0's texcoord, exactly"
        got = it.uv_texture_eval(st, np.full(len(pts), off[3], dtype=np.uint32), pts)
        d = R.decide_sphere(tex, SP[0:3], SP[3], SP[14:23], pts)
        same = (bits(got[:, :2]) == bits(d.uv32)).all(axis=1)
        print("%s / %s: %d of %d sphere records differ from the mirror" % (tree, name, (~same).sum(), len(same)))
        assert same.all(), (name, pts[~same][:4], got[~same][:4], d.uv32[~same][:4])
        assert np.array_equal(bits(got[:, 2:]), bits(d.value32))
        assert np.array_equal(got[~d.fragile, 2:], R.value(tex, d.bright64)[~d.fragile])
    # the hook's own refusals
    st = tex_cases.scene_texture(mts.scenes, tex_cases.textures()["checker"])
    with pytest.raises(mts.MtsGpuError, match="out of range"):
        it.uv_texture_eval(st, [off[4]], [[0.1, 0.1, 0]])
    bad = st.descriptor(); bad.kind = 2
    with pytest.raises(mts.MtsGpuError, match="unknown kind"):
        it.uv_texture_eval(bad, [0], [[0.1, 0.1, 0]])
    # the count is refused before a record is read, so one record's memory stands in for 2^24 + 1 of them
    A, p1, f5 = mts.abi, np.zeros(1, np.uint32), np.zeros(5, np.float32)
    with pytest.raises(mts.MtsGpuError, match=r"at most 2\^24 query records per call.*code -1"):
        it._chk(mts.lib().mtsgpu_uv_texture_eval(it._ctx, mts.uv_texture_array([st]), (1 << 24) + 1, A.ptr(p1, A.u32p), A.ptr(f5, A.f32p),
                                                 A.ptr(f5, A.f32p)), "uv_texture_eval")
    # without texcoords every mesh reads (0, 0); the sphere does not care
    it.set_uv_textures()
    got = it.uv_texture_eval(st, [0, off[3]], [[0.3, 0.3, 0], pts[20]])
    assert not got[0, :2].any() and got[1, :2].any()


# --- 2. the generalised block builder ----------------------------------------------------------------------------------
def _blocks(mts):
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
def test_slot_sources_equal_overwritten_blocks(device, mts, btype):
    """mtsgpu_bsdf_eval_slots(P, source, colour, values) == mtsgpu_bsdf_eval(P with slot s overwritten by the colour
    (source 1) or by values[s] (source 2)), bit for bit: every combination of sources, with and without the twosided adapter,
    f / pdf / sample"""
    P = _blocks(mts)[btype]
    offs = mts.abi.BSDF_COLOR_SLOTS[btype]
    rng = np.random.RandomState(70 + btype)
    n = 1024

    def dirs(k):
        d = rng.normal(size=(k, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
        return d.astype(np.float32)
    wi, wo, s = dirs(n), dirs(n), rng.rand(n, 2).astype(np.float32)
    color = np.float32([0.21, 0.62, 0.93])
    values = np.float32([[0.11, 0.52, 0.83], [0.74, 0.33, 0.46]])
    nonzero = 0
    for two in (0, TWOSIDED):
        for pick in range(3 ** len(offs)):
            src = [(pick // 3 ** k) % 3 if k < len(offs) else 0 for k in range(2)]
            Q = P.copy()
            for k, o in enumerate(offs):
                if src[k]:
                    Q[o:o + 3] = color if src[k] == 1 else values[k]
            for op in (0, 1, 2):
                aux = s if op == 2 else wo
                got = device.bsdf_eval_slots(btype | two, P, src, color, values, op, wi, aux)
                want = device.bsdf_eval(btype | two, Q, op, wi, aux)
                assert np.array_equal(bits(got), bits(want)), (btype, two, src, op, int((bits(got) != bits(want)).any(axis=1).sum()))
                nonzero += int((want[:, :7] != 0).any())
                if any(src) and op == 2:
                    assert not np.array_equal(bits(device.bsdf_eval(btype | two, P, op, wi, aux)), bits(got)), (btype, two, src)
    assert nonzero > 0
    if len(offs) < 2:
        with pytest.raises(mts.MtsGpuError, match="beyond the 1 texture slot"):
            device.bsdf_eval_slots(btype, P, [0, 2], color, values, 0, wi[:1], wo[:1])
    with pytest.raises(mts.MtsGpuError, match="unknown source"):
        device.bsdf_eval_slots(btype, P, [3, 0], color, values, 0, wi[:1], wo[:1])


def test_slot_hook_refuses_the_composite(device, mts):
    with pytest.raises(mts.MtsGpuError, match="composite"):
        device.bsdf_eval_slots(9, np.zeros(16), [0, 0], [1, 1, 1], np.zeros((2, 3)), 0, [[0, 0, 1]], [[0, 0, 1]])
    with pytest.raises(mts.MtsGpuError, match="bad BSDF type"):
        device.bsdf_eval_slots(0x200, np.zeros(16), [0, 0], [1, 1, 1], np.zeros((2, 3)), 0, [[0, 0, 1]], [[0, 0, 1]])
    # the count is refused before a record is read, so one record's memory stands in for 2^24 + 1 of them
    A, P, q, out, src = mts.abi, np.full(16, 0.5, np.float32), np.zeros(6, np.float32), np.zeros(8, np.float32), np.zeros(2, np.int32)
    with pytest.raises(mts.MtsGpuError, match=r"at most 2\^24 query records per call.*code -1"):
        device._chk(mts.lib().mtsgpu_bsdf_eval_slots(device._ctx, 0, A.ptr(P, A.f32p), A.ptr(src, A.i32p), A.ptr(q, A.f32p), A.ptr(q, A.f32p), 0,
                                                     (1 << 24) + 1, A.ptr(q, A.f32p), A.ptr(out, A.f32p)), "bsdf_eval_slots")


# --- 3. refusals -------------------------------------------------------------------------------------------------------
def test_set_uv_textures_refusals(gpu_lib, mts):
    S = mts.scenes
    check = S.Checkerboard(uscale=3.7)
    sd = S.tex_scene(check)                               # BSDF 0: textured lambertian on mesh 0 (shape 0)
    comp_child = sd.phong(10.0, rd=0.2, rs=0.3)           # BSDF 1
    comp = sd.composite([0.5, 0.5], [comp_child, comp_child])    # BSDF 2
    g = sd.meshes[0]
    sd.add_mesh(g.positions + F(3), g.triangles, bsdf=comp, face_normals=True)                       # shape 1, no texcoords
    sd.add_sphere((0, 3, 0), 0.4, bsdf=sd.lambertian(0.5))                                           # shape 2, BSDF 3
    vc = S.vcol_grid(2).meshes[0]
    sd.add_mesh(vc.positions - F(3), vc.triangles, bsdf=sd.lambertian(S.VERTEX_COLORS), colors=vc.colors)   # shape 3, BSDF 4
    it, scene = _prep(mts, sd)
    pool, has = scene.vertex_texcoords()
    texs = [check.descriptor(), S.GridTexture().descriptor()]
    good = np.int32([[0, -1], [-1, -1], [-1, -1], [-1, -1], [-1, -1]])

    def attempt(p=pool, h=has, t=texs, s=good):
        try:
            it.set_uv_textures(p, h, t, s)
        except mts.MtsGpuError as e:
            assert "code -1" in str(e), e
            return str(e)
        return ""

    def table(b, slot, k):
        s = good.copy(); s[b, slot] = k
        return s
    assert attempt() == ""
    assert "beyond the 1 texture slot" in attempt(s=table(0, 1, 0))
    assert "beyond the 0 texture slot" in attempt(s=table(2, 0, 0))                 # the composite has no slot of its own
    msg = attempt(s=table(1, 1, 1))
    assert "BSDF 2" in msg and "composite child 0" in msg, msg
    assert "names texture 2 of 2" in attempt(s=table(0, 0, 2)) and "names texture -2" in attempt(s=table(0, 0, -2))
    msg = attempt(s=table(4, 0, 1))
    assert "BSDF 4" in msg and "vertex colours as well" in msg, msg
    bad = check.descriptor(); bad.kind = 2
    assert "texture 1: unknown kind 2" in attempt(t=[texs[0], bad])
    for field in ("uoffset", "vscale", "line_width"):
        for value in (np.nan, np.inf):
            bad = S.GridTexture().descriptor(); setattr(bad, field, value)
            assert "texture 1: non-finite parameter" in attempt(t=[texs[0], bad]), field       # even though no slot uses it
    bad = check.descriptor(); bad.dark[1] = np.nan
    assert "texture 0: non-finite parameter" in attempt(t=[bad, texs[1]])
    for value in (np.nan, -np.inf):
        p = pool.copy(); p[7, 1] = value
        assert "non-finite texcoord at vertex 7" in attempt(p=p)
    # a non-finite row of a mesh WITHOUT texcoords is ignored, as the header says
    p = pool.copy(); p[g.positions.shape[0] + 2] = np.nan
    assert attempt(p=p) == ""
    # the (int) cast: 2 * (uv * scale + offset) must stay inside the int range for the shapes a texture is used on
    huge = check.descriptor(); huge.uscale = 2.0e9
    msg = attempt(t=[huge, texs[1]])
    assert "shape 0" in msg and "(int) cast" in msg, msg
    assert attempt(t=[texs[0], huge]) == "", "an unused texture's range is nobody's cast"
    huge = check.descriptor(); huge.voffset = -1.2e9
    assert "(int) cast" in attempt(t=[huge, texs[1]]) and "shape 2" in attempt(t=[texs[0], huge], s=table(3, 0, 1))    # the sphere too
    assert "both be given or both be NULL" in attempt(h=None)
    # accepted: a sphere, a mesh without texcoords (uv = (0, 0), as in the reference), no texcoords at all
    assert attempt(s=table(3, 0, 1)) == ""
    assert attempt(p=None, h=None) == ""
    # a refused call leaves the textures switched off and the context usable; the colour call refuses the clash from its side
    assert attempt(s=table(0, 1, 0)) != ""
    col, chas = scene.vertex_colors()
    assert it.render()
    assert attempt(s=table(0, 0, 0)) == ""
    with pytest.raises(mts.MtsGpuError, match="has a uv texture as well"):
        it.set_vertex_colors(col, chas, np.uint32([1, 0, 0, 0, 1]))
    assert attempt() == "" and it.render()
    fresh = mts.MIPathTracer(maxDepth=2)
    with pytest.raises(mts.MtsGpuError, match="before mtsgpu_upload_scene"):
        fresh.set_uv_textures(pool, has, texs, good)


# --- 4. no behaviour change --------------------------------------------------------------------------------------------
def _frame(it, res=32, spp=4):
    assert it.render()
    return it.film(), it.li_samples(_all_samples(res, spp))


@pytest.mark.parametrize("shape", ["grid", "sphere"])
def test_unused_textures_set_then_clear_and_equal_colours_change_nothing(gpu_lib, mts, shape):
    S = mts.scenes
    c = (0.5, 0.25, 0.75)
    it, scene = _prep(mts, S.tex_scene(c, shape=shape))
    base_film, base_li = _frame(it)
    assert (base_film[..., :3] > 0).any()
    # textures and texcoords handed over, no slot uses them: the same kernels, the same bits
    pool, has = scene.vertex_texcoords()
    it.set_uv_textures(pool, has, [S.Checkerboard().descriptor()], np.int32([[-1, -1]]))
    it.clear_film()
    film, li = _frame(it)
    assert np.array_equal(bits(film), bits(base_film)) and np.array_equal(bits(li), bits(base_li))
    # bright == dark == c: other kernels, the same arithmetic -- also against the block, which holds getAverage() != c
    for tex in (S.Checkerboard(bright=c, dark=c, uscale=3.7, vscale=-3.7, uoffset=0.3), S.GridTexture(bright=c, dark=c, uscale=-3.7, line_width=0.1)):
        it2, scene2 = _prep(mts, S.tex_scene(tex, shape=shape))
        assert scene2.bsdf_slot_texture is not None
        film, li = _frame(it2)
        assert np.array_equal(bits(film), bits(base_film)) and np.array_equal(bits(li), bits(base_li)), type(tex).__name__
    # a textured scene after set_uv_textures(NULL...) is the scene of its block
    tex = S.GridTexture(bright=c, dark=0.0, uscale=3.7, vscale=3.7, line_width=0.1)
    it3, _ = _prep(mts, S.tex_scene(tex, shape=shape))
    textured, _ = _frame(it3)
    assert not np.array_equal(bits(textured), bits(base_film))
    it3.set_uv_textures()
    it3.clear_film()
    film, li = _frame(it3)
    assert np.array_equal(bits(film), bits(base_film)) and np.array_equal(bits(li), bits(base_li))


# --- 5. radiance, with no tolerance ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, name", [("grid", "checker"), ("grid", "grid"), ("sphere", "checker")])
def test_radiance_is_bright_or_dark_times_the_white_scene(gpu_lib, mts, shape, name):
    """bright and dark are distinct powers of two per channel, and a path meets the floor (the sphere) once at most, so
    every sample is the white scene's sample times one of the two colours, bit for bit: a power of two commutes with every
    rounding of the chain.  Which one: the binary64 cell of the sample's hit, except for fragile samples, under the cap."""
    tex = tex_cases.textures()[name]
    geo = (tex_cases.FloorGeometry if shape == "grid" else tex_cases.SphereGeometry)(mts, tex)
    res, spp = tex_cases.E2E_RES, tex_cases.E2E_SPP
    samples = _all_samples(res, spp)
    assert geo.sd.max_depth < geo.sd.rr_depth
    it, _ = _prep(mts, geo.sd, res=res, spp=spp)
    li = it.li_samples(samples)
    li_w = _prep(mts, mts.scenes.tex_scene(1.0, shape=shape), res=res, spp=spp)[0].li_samples(samples)
    assert np.array_equal(bits(li[:, 3:6]), bits(li_w[:, 3:6])), "alpha and raster position are those of the white scene"
    hit = geo.locate(li[:, 4:6])
    W = li_w[:, :3]
    assert np.isfinite(li).all() and (W[hit.hit & ~hit.fragile] > 0).all()
    is_b = (bits(li[:, :3]) == bits(W * tex.bright)).all(axis=1)
    is_d = (bits(li[:, :3]) == bits(W * tex.dark)).all(axis=1)
    miss = ~hit.hit & ~hit.fragile
    assert np.array_equal(bits(li[miss, :3]), bits(W[miss])), "a ray that misses sees the environment of both scenes"
    on = hit.hit | hit.fragile
    print("%s / %s: %d samples, %d on the shape, %d bright, %d dark, %d neither, %d fragile"
          % (shape, name, len(li), on.sum(), (is_b & on).sum(), (is_d & on).sum(), (~is_b & ~is_d & hit.hit & ~hit.fragile).sum(), hit.fragile.sum()))
    sure = hit.hit & ~hit.fragile
    assert (is_b | is_d)[sure].all(), "every sample is bright x Li_white or dark x Li_white, bit for bit"
    assert (is_b & ~is_d)[sure].sum() > 100 and (is_d & ~is_b)[sure].sum() > 100, "both colours occur"
    assert hit.fragile.mean() <= tex_cases.MAX_FRAGILE
    assert np.array_equal(is_b[sure], hit.bright[sure]), "%d samples took the other cell's colour" % (is_b[sure] != hit.bright[sure]).sum()


# --- 6. one film across drivers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sky", [False, True])
def test_drivers_tile_parts_group_and_direct_give_one_film(gpu_lib, mts, sky):
    """cornell_tex: a checkerboard on a sphere and on a mesh without texcoords, a sheet whose Phong takes a grid texture in
    slot 0 and vertex colours in slot 1, an untextured metal"""
    sd = mts.scenes.cornell_tex(sky=sky)
    scene = mts.Scene(sd)
    assert scene.bsdf_slot_texture is not None and scene.bsdf_color_slots is not None
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
    # textures and colours both matter in this frame
    full = render("path", 0)
    for clear in ("set_uv_textures", "set_vertex_colors"):
        it = mts.MIPathTracer(maxDepth=sd.max_depth)
        it.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=5)
        getattr(it, clear)()
        assert it.render() and not np.array_equal(bits(it.film()), bits(full)), clear
