"""Unfiltered bitmap textures on the device: the read-out hook against the float32 mirror of tests/ref64_bmp.py bit for bit and
against its binary64 restatement but for fragile records, what mtsgpu_set_uv_bitmap_textures refuses, frames that must not change,
radiance with no tolerance on a palette of powers of two, one film across the drivers, and a bitmap next to a tangent mesh.
mtsgpu_bsdf_eval_slots needs nothing new: a bitmap's value reaches the block builder as any texture's does
(tests/test_gpu_tex.py).  The CPU side (gamma table, mirror, restatement, mutations, cap, ABI) is tests/test_bmp.py."""
import ctypes as C

import numpy as np
import pytest

import bmp_cases
import ref64_bmp as R
import tex_cases
from conftest import bits

pytestmark = pytest.mark.gpu
F = np.float32
N_SPECIAL = 12      # tex_cases.sphere_points puts the poles, the seam and the equator first: texel edges by construction


def _prep(mts, sd, scene=None, res=32, spp=4, integ=None, **kw):
    scene = mts.Scene(sd, **kw) if scene is None else scene
    cam = mts.PerspectiveCamera.for_description(sd, res, res)
    it = mts.MIPathTracer(maxDepth=sd.max_depth) if integ is None else integ
    it.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=21)
    return it, scene


def _all_samples(res, spp):
    y, x, j = np.meshgrid(np.arange(res), np.arange(res), np.arange(spp), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), j.ravel()], axis=1).astype(np.uint32)


# --- 1, 2. the read-out hook -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tree", ["host", "gpu_binning", "gpu_exact"])
def test_bitmap_value_is_the_mirror_bit_for_bit(gpu_lib, mts, tree):
    """every bitmap, wrap mode and transform on random records of the floor, the boundary strip, (identity transform) the strip
    just inside the cast limit, a mesh without texcoords and the sphere: the mirror's bits, and the binary64 cell but for
    fragile records, whose share stays under the cap"""
    sd = bmp_cases.hook_scene(mts)
    kp = mts.abi.KdParams()
    if tree != "host":
        kp.exact_prim_threshold = 16
    it, scene = _prep(mts, sd, kd_params=kp, gpu_binning=tree != "host", gpu_exact=tree == "gpu_exact")
    A = scene.arrays()
    pool, has = scene.vertex_texcoords()
    assert has.tolist() == [1, 1, 1, 0, 0]
    it.set_uv_textures(pool, has)          # no slot is textured, so the Scene mirror made no call: hand the texcoords over
    off, tri = A["shape_tri_offset"], A["tri_idx"]
    rng = np.random.RandomState(4)
    fprim, fu, fv = tex_cases.triangle_records(rng, off[0], off[1] - off[0], 3000)
    sprim = np.arange(off[1], off[2], dtype=np.uint32)
    hprim = np.arange(off[2], off[3], dtype=np.uint32)
    nprim, nu, nv = tex_cases.triangle_records(rng, off[3], off[4] - off[3], 200)
    SP = A["shape_params"][4]
    pts = tex_cases.sphere_points(rng, 2000, SP[0:3], SP[3])
    total = fragile = 0
    for name, t in sorted(bmp_cases.textures().items()):
        st = bmp_cases.scene_texture(mts.scenes, t)
        parts = [(fprim, fu, fv), (sprim, None, None), (nprim, nu, nv)] + ([(hprim, None, None)] if name.endswith("/id") else [])
        prim = np.concatenate([p[0] for p in parts])
        u = np.concatenate([np.zeros(len(p[0]), F) if p[1] is None else p[1] for p in parts])
        v = np.concatenate([np.zeros(len(p[0]), F) if p[2] is None else p[2] for p in parts])
        got = it.bitmap_texture_eval(st, prim, np.stack([u, v, np.zeros_like(u)], axis=1))
        d = R.decide_triangles(t, pool, tri, prim, u, v)
        assert np.array_equal(bits(got[:, :2]), bits(d.uv32)), name
        assert np.array_equal(bits(got[:, 2:]), bits(d.value32)), (name, int((bits(got[:, 2:]) != bits(d.value32)).any(axis=1).sum()))
        keep = ~d.fragile
        assert np.array_equal(bits(got[keep, 2:]), bits(d.value64[keep])), name
        assert d.fragile[:3000].mean() <= tex_cases.MAX_FRAGILE, name
        total += len(prim); fragile += int(d.fragile.sum())
        got = it.bitmap_texture_eval(st, np.full(len(pts), off[4], dtype=np.uint32), pts)
        d = R.decide_sphere(t, SP[0:3], SP[3], SP[14:23], pts)
        assert np.array_equal(bits(got[:, :2]), bits(d.uv32)), name
        assert np.array_equal(bits(got[:, 2:]), bits(d.value32)), name
        assert np.array_equal(bits(got[~d.fragile, 2:]), bits(d.value64[~d.fragile])) and d.fragile[N_SPECIAL:].mean() <= tex_cases.MAX_FRAGILE, name
    print("%s: %d triangle records, %d fragile" % (tree, total, fragile))
    # the hook's own refusals; the old hook keeps refusing the kind
    st = bmp_cases.scene_texture(mts.scenes, bmp_cases.textures()["5x3/repeat/id"])
    with pytest.raises(mts.MtsGpuError, match="out of range"):
        it.bitmap_texture_eval(st, [off[5]], [[0.1, 0.1, 0]])
    with pytest.raises(mts.MtsGpuError, match="unknown kind 2"):
        it.uv_texture_eval(st.descriptor(), [0], [[0.1, 0.1, 0]])
    with pytest.raises(mts.MtsGpuError, match="kind 0 is not a bitmap"):
        it.bitmap_texture_eval(mts.scenes.Checkerboard().descriptor(), [0], [[0.1, 0.1, 0]], bitmap=st.bitmap())
    bad = st.descriptor(); bad.vscale = np.nan
    with pytest.raises(mts.MtsGpuError, match="texture: non-finite parameter"):
        it.bitmap_texture_eval(bad, [0], [[0.1, 0.1, 0]], bitmap=st.bitmap())
    bad = st.bitmap(); bad.wrap_mode = 4
    with pytest.raises(mts.MtsGpuError, match="bitmap: unknown wrap mode 4"):
        it.bitmap_texture_eval(st.descriptor(), [0], [[0.1, 0.1, 0]], bitmap=bad)
    a, p1, f5 = mts.abi, np.zeros(1, np.uint32), np.zeros(5, np.float32)
    with pytest.raises(mts.MtsGpuError, match=r"at most 2\^24 query records per call.*code -1"):
        it._chk(mts.lib().mtsgpu_bitmap_texture_eval(it._ctx, mts.uv_texture_array([st]), mts.bitmap_array([st]), (1 << 24) + 1, a.ptr(p1, a.u32p),
                                                     a.ptr(f5, a.f32p), a.ptr(f5, a.f32p)), "bitmap_texture_eval")


# --- 4. refusals -------------------------------------------------------------------------------------------------------
def test_set_uv_bitmap_textures_refusals(gpu_lib, mts):
    S = mts.scenes
    tx = bmp_cases.texels("5x3")
    bmp = S.BitmapTexture(texels=tx, uscale=3.7)
    sd = S.tex_scene(bmp)                                 # BSDF 0: textured lambertian on mesh 0 (shape 0)
    sd.add_sphere((0, 3, 0), 0.4, bsdf=sd.lambertian(0.5))                                           # shape 1, BSDF 1
    it, scene = _prep(mts, sd)
    assert scene.uv_bitmap_texture_args() is not None
    pool, has = scene.vertex_texcoords()
    check = S.Checkerboard()
    texs = [bmp.descriptor(), check.descriptor()]
    maps = [bmp.bitmap()]
    good = np.int32([[0, -1], [-1, -1]])

    def attempt(p=pool, h=has, t=texs, s=good, b=maps, tb=(0, -1), old=False):
        try:
            if old:
                it.set_uv_textures(p, h, t, s)
            else:
                it.set_uv_bitmap_textures(p, h, t, s, b, np.int32(tb))
        except mts.MtsGpuError as e:
            assert "code -1" in str(e), e
            return str(e)
        return ""

    def bitmap(**kw):
        b = bmp.bitmap()
        for k, v in kw.items():
            setattr(b, k, v)
        return b
    assert attempt() == "" and it.render()
    assert "bitmap 0: zero dimension (0 x 3)" in attempt(b=[bitmap(width=0)]) and "bitmap 0: zero dimension (5 x 0)" in attempt(b=[bitmap(height=0)])
    assert "bitmap 1: unknown wrap mode 4" in attempt(b=[maps[0], bitmap(wrap_mode=4)])
    assert "bitmap 0: reserved word is not zero" in attempt(b=[bitmap(reserved=1)])
    assert "bitmap 0: no texels" in attempt(b=[bitmap(texels=C.cast(None, mts.abi.f32p))])
    for value in (np.nan, np.inf, -1e-30):
        bad = tx.copy(); bad[2, 3, 1] = value
        assert "bitmap 1: texel (3, 2) is negative or not finite" in attempt(b=[maps[0], bitmap(texels=mts.abi.ptr(bad, mts.abi.f32p))]), value
    # the total is refused before a texel is read: 15 texels stand in for 2^31 of them
    assert "bitmap 0: more than 2147483647 texels in all" in attempt(b=[bitmap(width=1 << 16, height=1 << 15)])
    assert "bitmap 1: more than 2147483647 texels in all" in attempt(b=[maps[0], bitmap(width=(1 << 31) - 15, height=1)])
    assert "bitmap 0: more than" in attempt(b=[bitmap(width=0xFFFFFFFF, height=0xFFFFFFFF)])
    assert "texture 0: bitmap index 1 out of range (1 bitmaps)" in attempt(tb=(1, -1)) and "texture 0: bitmap index -1 out of range" in attempt(tb=(-1, -1))
    assert "texture 1: bitmap index 3 out of range" in attempt(t=[texs[1], texs[0]], tb=(0, 3)), "even though no slot uses it"
    assert "texture 0: bitmap index 0 out of range (0 bitmaps)" in attempt(b=None, tb=(0, -1))
    # the checks of mtsgpu_set_uv_textures
    assert "beyond the 1 texture slot" in attempt(s=np.int32([[0, 0], [-1, -1]]))
    assert "names texture 2 of 2" in attempt(s=np.int32([[2, -1], [-1, -1]]))
    bad = bmp.descriptor(); bad.uoffset = np.inf
    assert "texture 0: non-finite parameter" in attempt(t=[bad, texs[1]])
    bad = bmp.descriptor(); bad.kind = 3
    assert "texture 0: unknown kind 3" in attempt(t=[bad, texs[1]])
    bad = bmp.descriptor(); bad.line_width = np.nan          # the seven words behind vscale are the library's
    assert attempt(t=[bad, texs[1]]) == ""
    p = pool.copy(); p[7, 1] = np.nan
    assert "non-finite texcoord at vertex 7" in attempt(p=p)
    assert "both be given or both be NULL" in attempt(h=None)
    # the (int) cast: uv' * (width, height) must stay inside the int range for the shapes the texture is used on
    huge = bmp.descriptor(); huge.uscale = 4.0e8           # |uv| reaches 1.4 on the floor: 5.6e8 * 5 texels
    msg = attempt(t=[huge, texs[1]])
    assert "shape 0" in msg and "(int) cast (|uv' * size|" in msg, msg
    huge.uscale = 1.0e8
    assert attempt(t=[huge, texs[1]]) == "", "5 * 1.4e8 is inside the range"
    huge = bmp.descriptor(); huge.voffset = -7.2e8         # * 3 texels
    assert "shape 1" in attempt(t=[huge, texs[1]], s=np.int32([[1, -1], [0, -1]])), "the sphere too"
    assert attempt(t=[texs[1], huge], s=np.int32([[0, -1], [-1, -1]]), tb=(-1, 0)) == "", "an unused texture's range is nobody's cast"
    # the old calls still do not know the kind
    assert "texture 0: unknown kind 2" in attempt(old=True)
    # a refused call leaves the textures switched off and the context usable; either call replaces what the other one set
    assert attempt(tb=(1, -1)) != ""
    it.clear_film(); assert it.render()
    off_film = it.film().copy()
    assert attempt() == ""
    it.clear_film(); assert it.render()
    on_film = it.film().copy()
    assert not np.array_equal(bits(on_film), bits(off_film))
    assert attempt(t=[texs[1]], s=good, old=True) == ""                       # the checkerboard through the old call
    it.clear_film(); assert it.render()
    assert not np.array_equal(bits(it.film()), bits(on_film)) and not np.array_equal(bits(it.film()), bits(off_film))
    it.set_uv_bitmap_textures()
    it.clear_film(); assert it.render()
    assert np.array_equal(bits(it.film()), bits(off_film))
    fresh = mts.MIPathTracer(maxDepth=2)
    with pytest.raises(mts.MtsGpuError, match="mtsgpu_set_uv_bitmap_textures before mtsgpu_upload_scene"):
        fresh.set_uv_bitmap_textures(pool, has, texs, good, maps, np.int32([0, -1]))


# --- 5. frames that must not change ------------------------------------------------------------------------------------
def _frame(it, res=32, spp=4):
    assert it.render()
    return it.film(), it.li_samples(_all_samples(res, spp))


def test_no_bitmaps_through_the_new_call_is_the_old_call(gpu_lib, mts):
    sd = mts.scenes.cornell_tex()
    it, scene = _prep(mts, sd)
    base_film, base_li = _frame(it)
    ut = scene.uv_texture_args()
    it._chk(mts.lib().mtsgpu_set_uv_bitmap_textures(it._ctx, *(ut + (0, None, None))), "set_uv_bitmap_textures")
    it.clear_film()
    film, li = _frame(it)
    assert (base_film[..., :3] > 0).any()
    assert np.array_equal(bits(film), bits(base_film)) and np.array_equal(bits(li), bits(base_li))


@pytest.mark.parametrize("shape", ["grid", "sphere"])
def test_one_texel_is_the_constant_and_set_then_clear_restores_the_film(gpu_lib, mts, shape):
    S = mts.scenes
    c = (0.5, 0.25, 0.75)
    it, scene = _prep(mts, S.tex_scene(c, shape=shape))
    base_film, base_li = _frame(it)
    assert (base_film[..., :3] > 0).any()
    one = np.float32([[c]])
    for wrap in ("repeat", "clamp"):
        tex = S.BitmapTexture(texels=one, wrap=wrap, uscale=3.7, vscale=-3.7, uoffset=0.3)
        it2, scene2 = _prep(mts, S.tex_scene(tex, shape=shape))
        assert scene2.uv_bitmap_texture_args() is not None and np.array_equal(scene2.description.bsdf_params[0][:3], np.float32(c))
        film, li = _frame(it2)
        assert np.array_equal(bits(film), bits(base_film)) and np.array_equal(bits(li), bits(base_li)), wrap
    # a textured scene after the call with everything NULL is the scene of its block: texel (0, 0) = c
    tx = bmp_cases.texels("5x3").copy(); tx[0, 0] = c
    it3, _ = _prep(mts, S.tex_scene(S.BitmapTexture(texels=tx, uscale=3.7, vscale=3.7), shape=shape))
    textured, _ = _frame(it3)
    assert not np.array_equal(bits(textured), bits(base_film))
    it3.set_uv_bitmap_textures()
    it3.clear_film()
    film, li = _frame(it3)
    assert np.array_equal(bits(film), bits(base_film)) and np.array_equal(bits(li), bits(base_li))


# --- 6. radiance, with no tolerance ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, wrap, transform", bmp_cases.E2E)
def test_radiance_is_one_palette_entry_times_the_white_scene(gpu_lib, mts, shape, wrap, transform):
    """the texels are drawn from a palette of distinct powers of two per channel, and a path meets the floor (the sphere) once at
    most, so every sample is the white scene's sample times exactly one palette entry (or the column-0 constant of black and
    white), bit for bit: a power of two commutes with every rounding of the chain.  Which one: the binary64 cell of the sample's
    hit, except for fragile samples, under the cap."""
    t, entry = bmp_cases.palette_bitmap(wrap, transform)
    pal = bmp_cases.palette()
    geo = (bmp_cases.FloorGeometry if shape == "grid" else bmp_cases.SphereGeometry)(mts, t)
    res, spp = tex_cases.E2E_RES, tex_cases.E2E_SPP
    samples = _all_samples(res, spp)
    assert geo.sd.max_depth < geo.sd.rr_depth
    it, scene = _prep(mts, geo.sd, res=res, spp=spp)
    assert scene.uv_bitmap_texture_args() is not None
    li = it.li_samples(samples)
    li_w = _prep(mts, mts.scenes.tex_scene(1.0, shape=shape), res=res, spp=spp)[0].li_samples(samples)
    assert np.array_equal(bits(li[:, 3:6]), bits(li_w[:, 3:6])), "alpha and raster position are those of the white scene"
    hit = geo.locate(li[:, 4:6])
    W = li_w[:, :3]
    sure = hit.hit & ~hit.fragile
    assert np.isfinite(li).all() and (W[sure] > 0).all()
    miss = ~hit.hit & ~hit.fragile
    assert np.array_equal(bits(li[miss, :3]), bits(W[miss])), "a ray that misses sees the environment of both scenes"
    # candidates: the palette, then black and white
    cand = np.concatenate([pal, np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32)])
    match = np.stack([(bits(li[:, :3]) == bits(W * c)).all(axis=1) for c in cand], axis=1)          # [n][PALETTE_N + 2]
    assert (match[sure].sum(axis=1) == 1).all(), "every sure sample is Li_white x exactly one entry, bit for bit"
    got = match.argmax(axis=1)
    cell = hit.cell
    want = np.where(cell == R.BLACK, len(pal), np.where(cell == R.WHITE, len(pal) + 1, entry.reshape(-1)[np.maximum(cell, 0)]))
    counts = np.bincount(got[sure], minlength=len(cand))
    print("%s / %s / %s: %d samples, %d sure, %d fragile; per entry %s" % (shape, R.WRAP_NAMES[wrap], transform, len(li), sure.sum(), hit.fragile.sum(),
                                                                          counts.tolist()))
    assert np.array_equal(got[sure], want[sure]), "%d samples took another cell's texel" % (got[sure] != want[sure]).sum()
    assert (counts[:len(pal)] > 100).sum() >= 8, "at least eight palette entries occur more than 100 times"
    assert hit.fragile.mean() <= tex_cases.MAX_FRAGILE
    if wrap == R.BLACK_MODE:
        assert counts[len(pal)] > 100 and counts[len(pal) + 1] == 0, "the column-0 constant is seen in the frame"
    elif wrap == R.WHITE_MODE:
        assert counts[len(pal) + 1] > 100 and counts[len(pal)] == 0, "the column-0 constant is seen in the frame"
    else:
        assert counts[len(pal):].sum() == 0


# --- 7. one film across drivers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sky", [False, True])
def test_drivers_tile_parts_group_and_direct_give_one_film(gpu_lib, mts, sky):
    """cornell_bmp: a bitmap on a sphere, a checkerboard on a mesh without texcoords, a sheet whose Phong takes a grid texture in
    slot 0 and vertex colours in slot 1, an untextured metal"""
    sd = mts.scenes.cornell_bmp(sky=sky)
    scene = mts.Scene(sd)
    assert scene.uv_bitmap_texture_args() is not None and scene.bsdf_color_slots is not None
    assert sorted(t.kind for t in scene.textures) == [0, 1, 2]
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
    for integ in ("path", (1, 1)):
        base = render(integ, 0)
        assert np.isfinite(base).all() and (base[..., :3] > 0).any()
        for drive in (1, 2, 3):
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
    # the bitmap matters in this frame: the sphere under its block's constant (texel (0, 0)) is another picture
    full = render("path", 0)
    it = mts.MIPathTracer(maxDepth=sd.max_depth)
    it.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=5)
    it.set_uv_bitmap_textures()
    assert it.render() and not np.array_equal(bits(it.film()), bits(full))
    # ... and so does its wrap mode: white turns column 0 into 1
    white = mts.Scene(mts.scenes.cornell_bmp(sky=sky, wrap="white"))
    it.preprocess(white, cam, sampler="independent", sampleCount=spp, seed=5)
    it.clear_film()
    assert it.render() and not np.array_equal(bits(it.film()), bits(full))


# --- 8. next to a tangent mesh -----------------------------------------------------------------------------------------
def test_bitmap_next_to_a_tangent_mesh(gpu_lib, mts):
    """an anisotropic Ward on a mesh with texcoords sends the scene to the tangent kernels, whose copy of the lookup then serves
    the floor's bitmap: the palette argument again, on the floor, with the Ward sheet out of the camera's sight"""
    S = mts.scenes
    t, entry = bmp_cases.palette_bitmap(R.WHITE_MODE, "id")
    pal = bmp_cases.palette()
    res, spp = tex_cases.E2E_RES, tex_cases.E2E_SPP
    samples = _all_samples(res, spp)

    def scene_of(reflectance):
        sd = S.tex_scene(reflectance, shape="grid", cells=tex_cases.CELLS)
        pos, tri, uv = S.tex_grid_mesh(2)
        sd.add_mesh((pos * F(0.1) + np.float32([30, 0, 30])).astype(np.float32), tri, bsdf=sd.ward(0.1, 0.3, rd=0.4, rs=0.2), face_normals=False,
                    name="ward sheet", texcoords=uv)
        return sd
    sd = scene_of(bmp_cases.scene_texture(S, t))
    it, scene = _prep(mts, sd, res=res, spp=spp)
    assert scene.wants_tangents and scene.uv_bitmap_texture_args() is not None
    li = it.li_samples(samples)
    it_w, scene_w = _prep(mts, scene_of(1.0), res=res, spp=spp)
    assert scene_w.wants_tangents
    W = it_w.li_samples(samples)[:, :3]
    geo = bmp_cases.FloorGeometry(mts, t)
    hit = geo.locate(li[:, 4:6])
    sure = hit.hit & ~hit.fragile
    cand = np.concatenate([pal, np.ones((1, 3), np.float32)])
    match = np.stack([(bits(li[:, :3]) == bits(W * c)).all(axis=1) for c in cand], axis=1)
    assert (W[sure] > 0).all() and (match[sure].sum(axis=1) == 1).all()
    want = np.where(hit.cell == R.WHITE, len(pal), entry.reshape(-1)[np.maximum(hit.cell, 0)])
    got = match.argmax(axis=1)
    counts = np.bincount(got[sure], minlength=len(cand))
    print("tangent family: %d sure, %d fragile; per entry %s" % (sure.sum(), hit.fragile.sum(), counts.tolist()))
    assert np.array_equal(got[sure], want[sure]) and (counts > 100).sum() >= 8 and counts[-1] > 100
    assert hit.fragile.mean() <= tex_cases.MAX_FRAGILE
