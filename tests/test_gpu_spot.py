"""Projection textures of the spot luminaire on the device: the read-out hook and the scene's sample_luminaire against the float32
mirror of tests/ref64_spot.py bit for bit and against its binary64 restatement inside the bound, the refusals through the context in
both call orders, frames that must not change, radiance with no tolerance on palettes of powers of two, the bilinear lookup end to
end against the restatement, and one film across the ways of driving the bounces.  The CPU side (mirror, restatement, mutations,
check, ABI) is tests/test_spot.py."""
import numpy as np
import pytest

import bmp_cases
import ref64_bmp as B
import ref64_spot as R
import ref64_tex as T
import spot_cases as SC
from conftest import bits

pytestmark = pytest.mark.gpu
F = np.float32
U = 2.0 ** -24
RES, SPP = 16, 4
MAX_FRAGILE = 0.01


def _prep(mts, sd, res=RES, spp=SPP, integ=None, scene=None):
    scene = mts.Scene(sd) if scene is None else scene
    cam = mts.PerspectiveCamera.for_description(sd, res, res)
    it = mts.MIPathTracer(maxDepth=sd.max_depth) if integ is None else integ
    it.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=21)
    return it, scene


def _all_samples(res=RES, spp=SPP):
    y, x, j = np.meshgrid(np.arange(res), np.arange(res), np.arange(spp), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), j.ravel()], axis=1).astype(np.uint32)


def _fn(mts):
    """the library's tangent and arc cosine for the mirror"""
    return dict(tan=lambda a: mts.devmath("tan", [a])[0], acos=lambda c: mts.devmath("acos", c))


# --- 1. the hook and the scene's sample_luminaire --------------------------------------------------------------------------------
def test_hook_is_the_mirror_bit_for_bit_and_inside_the_bound(gpu_lib, mts):
    it = mts.MIPathTracer()
    fn = _fn(mts)
    total = fragile = 0
    for i, (name, spot, st) in enumerate(SC.cases(mts)):
        p = SC.points(spot, st, seed=i)
        got = it.spot_eval(spot.block, SC.scene_texture(mts.scenes, st), p, bilinear=st.bilinear)
        m = R.mirror(spot, st, p, fn=fn)
        assert np.array_equal(bits(got[:, 0:3]), bits(m.d)), name
        assert np.array_equal(bits(got[:, 3:5]), bits(m.uv)), (name, int((bits(got[:, 3:5]) != bits(m.uv)).any(axis=1).sum()))
        assert np.array_equal(bits(got[:, 5:8]), bits(m.value)), (name, int((bits(got[:, 5:8]) != bits(m.value)).any(axis=1).sum()))
        r = R.restate(spot, st, p)
        ok = ~r.fragile
        assert (np.abs(got[ok, 5:8].astype(np.float64) - r.value64[ok]) <= r.bound[ok] + 1e-45).all(), name
        total += len(p); fragile += int(r.fragile.sum())
    print("%d records, %d fragile" % (total, fragile))
    assert fragile <= MAX_FRAGILE * total
    # the hook's refusals are the call's
    spot = SC.spots(mts)[0]
    odd = mts.scenes.BitmapTexture(texels=np.full((3, 5, 3), 0.5, np.float32))
    with pytest.raises(mts.MtsGpuError, match="power of two"):
        it.spot_eval(spot.block, odd, [[0, 0, 0]], bilinear=True)
    wide = spot.block.copy(); wide[8] = F(1.6)
    with pytest.raises(mts.MtsGpuError, match="cutoffAngle < 90"):
        it.spot_eval(wide, mts.scenes.Checkerboard(), [[0, 0, 0]])


def _three_lights(mts, texture=None, bilinear=False):
    S = mts.scenes
    sd = S.SceneDescription("spot_three")
    b = sd.lambertian(0.5)
    sd.add_mesh(np.float32([[-2, 0, -2], [2, 0, -2], [2, 0, 2], [-2, 0, 2]]), np.uint32([[0, 2, 1], [0, 3, 2]]), bsdf=b, face_normals=True, name="floor")
    sd.point_light((1.5, 1.0, -1.0), (0.5, 0.25, 0.125))
    sd.spot_light((-0.5, 2.0, 0.5), (0.0, 0.0, 0.0), (3.0, 2.0, 1.0), cutoff_deg=35.0, beam_deg=20.0)
    sd.spot_light((0.3, 2.2, -0.2), (0.1, 0.0, 0.2), (8.0, 6.0, 4.0), cutoff_deg=40.0, beam_deg=25.0, texture=texture, bilinear=bilinear)
    sd.camera = dict(origin=(0.0, 4.0, 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), fov=35.0)
    sd.max_depth = 2
    return sd


def test_scene_lum_eval_runs_the_textured_instantiation(gpu_lib, mts):
    """a point light, a plain spot and a textured spot: the selection and the two other luminaires are what they are without the
    texture, bit for bit; the textured spot's value is the mirror's"""
    rng = np.random.RandomState(3)
    q = np.zeros((3000, 16), dtype=np.float32)
    q[:, 0] = rng.uniform(-1.5, 1.5, len(q)); q[:, 2] = rng.uniform(-1.5, 1.5, len(q)); q[:, 1] = rng.uniform(0.0, 0.5, len(q))
    q[:, 3:5] = rng.uniform(0, 1, (len(q), 2))
    plain_it, _ = _prep(mts, _three_lights(mts))
    plain = plain_it.scene_lum_eval(0, q)
    fn = _fn(mts)
    for name in ("checker/scale4", "nearest/5x3/repeat/neg", "nearest/16x16/black/id", "bilinear/16x16/repeat/neg", "bilinear/2x2/white/id"):
        st = SC.textures()[name]
        it, scene = _prep(mts, _three_lights(mts, SC.scene_texture(mts.scenes, st), st.bilinear))
        assert scene.spot_texture_args() is not None
        got = it.scene_lum_eval(0, q)
        lum = got[:, 1].astype(int)
        assert np.array_equal(bits(got[:, :12]), bits(plain[:, :12])), name           # found, index, p, n, d, pdf
        other = lum != 2
        assert other.any() and (~other).any() and np.array_equal(bits(got[other]), bits(plain[other])), name
        spot = R.Spot(np.array(scene.arrays()["lum_params"]).reshape(-1, mts.abi.LUM_NPARAMS)[2])
        m = R.mirror(spot, st, q[~other, 0:3], fn=fn)
        sel_pdf = np.array(scene.arrays()["lum_sel_pdf"], dtype=np.float32)[2]
        assert np.array_equal(bits(got[~other, 8:11]), bits(m.d)), name
        want = m.value * (F(1) / (F(1) * sel_pdf))          # lRec.pdf *= lumPdf; lRec.value /= lRec.pdf: Spectrum / Float multiplies by 1 / f
        assert np.array_equal(bits(got[~other, 12:15]), bits(want)), (name, int((bits(got[~other, 12:15]) != bits(want)).any(axis=1).sum()))
        assert (m.value > 0).any() and (plain[~other, 12:15] != got[~other, 12:15]).any(), name


# --- 2. refusals through the context ---------------------------------------------------------------------------------------------
def test_both_call_orders_with_mask_snow_and_cloth_and_an_upload_clears(gpu_lib, mts):
    S = mts.scenes
    chk = S.Checkerboard(bright=1.0, dark=0.25)
    import cloth_cases
    weave = cloth_cases.weaves(mts)[0][1]

    def scene(other, texture=chk):
        sd = S.SceneDescription("spot_beside")
        pos, tri, uv = S.tex_grid_mesh(2)
        sd.add_mesh(pos, tri, bsdf=other(sd), face_normals=True, texcoords=uv)
        sd.spot_light((0.0, 2.0, 0.0), (0.0, 0.0, 0.0), 5.0, cutoff_deg=40.0, texture=texture)
        sd.camera = dict(origin=(0.0, 3.0, 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), fov=40.0)
        sd.max_depth = 2
        return sd
    makers = (("mask", lambda sd: sd.mask(sd.lambertian(0.5), 0.5)), ("snow", lambda sd: sd.wiscombe()), ("cloth", lambda sd: sd.irawan(weave)))
    # the family's call first (Scene's order), the spot call second: the spot call refuses
    for word, make in makers:
        with pytest.raises(mts.MtsGpuError, match="set_spot_textures.*" + word + ".*textured spot"):
            _prep(mts, scene(make))
        # ... and the same scene without the texture is served as ever
        it, _ = _prep(mts, scene(make, texture=None))
        assert it.render()
    # the spot call first: the family's call refuses
    for word, make in makers:
        sd = scene(make, texture=None)
        sc = mts.Scene(sd)
        it = mts.MIPathTracer(maxDepth=2)
        plain = mts.Scene(scene(lambda sd: sd.lambertian(0.5), texture=None))
        it.preprocess(plain, mts.PerspectiveCamera.for_description(sd, RES, RES), sampleCount=SPP, seed=21)
        it.set_spot_textures([chk], [0], [0])
        with pytest.raises(mts.MtsGpuError, match=word + ".*textured spot"):
            if word == "mask":
                it.set_uv_masked_textures(bsdf_mask=[(mts.abi.MASK_CONSTANT, -1, (0.5, 0.5, 0.5))])
            elif word == "snow":
                it.set_snow_bsdfs([sc.bsdf_snow[0]])
            else:
                it.set_cloth_bsdfs([weave], [0])
        # switched off, the family's call is taken again; and all-none tables are taken beside a textured spot
        it.set_snow_bsdfs([None]); it.set_cloth_bsdfs([], [-1]); it.set_uv_masked_textures(bsdf_mask=[(mts.abi.MASK_NONE, -1, (0, 0, 0))])
        it.set_spot_textures()
        if word == "snow":
            it.set_snow_bsdfs([sc.bsdf_snow[0]])
            assert it.render()
    # a new upload clears the table; switching off restores the plain film byte for byte
    sd_plain, sd_tex = SC.e2e_description(mts), SC.e2e_description(mts, texture=chk)
    it0, _ = _prep(mts, sd_plain)
    assert it0.render()
    base = it0.film()
    it, _ = _prep(mts, sd_tex)
    assert it.render()
    textured = it.film()
    assert (base[..., :3] > 0).any() and not np.array_equal(bits(textured), bits(base))
    it.set_spot_textures(); it.clear_film()
    assert it.render() and np.array_equal(bits(it.film()), bits(base))
    it.set_spot_textures([chk], [0], [0]); it.clear_film()
    assert it.render() and np.array_equal(bits(it.film()), bits(textured))
    it.preprocess(mts.Scene(sd_plain), mts.PerspectiveCamera.for_description(sd_plain, RES, RES), sampler="independent", sampleCount=SPP, seed=21)
    it.clear_film()
    assert it.render() and np.array_equal(bits(it.film()), bits(base))
    with pytest.raises(mts.MtsGpuError, match="texture index 1 out of range"):
        it.set_spot_textures([chk], [0], [1])


# --- 3. frames that must not change ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["next", "five"])
def test_constant_spots_through_the_new_call_render_the_same_bytes(gpu_lib, mts, name):
    """scenes with a constant spot, rendered after mtsgpu_set_spot_textures with every lum_texture = -1"""
    if name == "next":
        sd = mts.scenes.next_rows()
    else:
        import lum_cases
        sd = dict(lum_cases.scenes(mts))["five: quad, spot, sphere, point, envmap"]
    assert mts.abi.LUM_SPOT in sd.lum_type
    for integ in (None, mts.MIDirectIntegrator(2, 1)):
        it, scene = _prep(mts, sd, res=24, integ=integ)
        assert it.render()
        base = it.film()
        it.set_spot_textures([mts.scenes.Checkerboard()], [0], [-1] * len(sd.lum_type)); it.clear_film()
        assert it.render() and np.array_equal(bits(it.film()), bits(base)) and (base[..., :3] > 0).any()


# --- 4. radiance, with no tolerance -----------------------------------------------------------------------------------------------
# The reach of a binary32 hit point around the exact one: the hit is o + t d with t within a few roundings of the exact distance
# (<= 8 u relative, |t d| <= 4.5 in these scenes) and one rounding per coordinate of the sum: 16 u * 4.5 covers both.
REACH = 16 * U * 4.5


def _rays(it):
    r = it.camera_rays(_all_samples().astype(np.int32))
    return np.concatenate([r[:, 0:3], r[:, 4:7]], axis=1)      # o, d (mint and maxt dropped)


def _hit_points(it, shape):
    rays = _rays(it)
    p = SC.floor_hits(rays)
    unsure = np.zeros(len(p), dtype=bool)
    if shape == "sphere":
        hit, ps = SC.sphere_hits(rays)
        c = np.float32([0.1, 0.45, -0.05]).astype(np.float64)
        o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
        dn = d / np.linalg.norm(d, axis=1)[:, None]
        oc = c - o
        dist = np.linalg.norm(oc - dn * (oc * dn).sum(axis=1)[:, None], axis=1)       # the ray's distance from the centre
        unsure = np.abs(dist - float(F(0.45))) < 1e-4                                   # the silhouette: hit or miss is undecided
        p = np.where(hit[:, None], ps, p)
    return p, unsure


def _palette_textures():
    pal_tx, entry = bmp_cases.palette_bitmap(B.BLACK_MODE, "id")
    return {"checker": R.SpotTex(T.Tex(T.CHECKERBOARD, 0.1, 0.2, 3.0, 3.0, bright=1.0, dark=0.25)),
            "grid": R.SpotTex(T.Tex(T.GRID, 0.0, 0.0, 4.0, 4.0, bright=(0.5, 1.0, 0.25), dark=(0.125, 0.0625, 0.5), line_width=0.08)),
            "bitmap": R.SpotTex(B.Bmp(pal_tx.texels, B.BLACK_MODE, 0.0, 0.0, 1.0, 1.0), False)}


@pytest.mark.parametrize("integrator", ["direct", "path"])
@pytest.mark.parametrize("shape, tilted", [("floor", False), ("sphere", False), ("floor", True)])
def test_radiance_is_one_palette_entry_times_the_constant_spot(gpu_lib, mts, shape, tilted, integrator):
    """direct with one luminaire sample and no BSDF sample, path with maxDepth 2: only the camera hit's light sample contributes, so
    every radiance sample is the sample of the same scene with the constant spot times the texture's value at the hit, and that
    value is a power of two per channel: bit for bit, no tolerance.  Which value: the restatement at the binary64 hit point of the
    sample's camera ray; samples where a decision changes within the reach of the binary32 hit point are left out"""
    def integ():
        return mts.MIDirectIntegrator(1, 0) if integrator == "direct" else None
    samples = _all_samples()
    it_w, scene_w = _prep(mts, SC.e2e_description(mts, shape=shape, tilted=tilted), integ=integ())
    W = it_w.li_samples(samples)
    p64, unsure = _hit_points(it_w, shape)
    spot = R.Spot(np.array(scene_w.arrays()["lum_params"]).reshape(-1, mts.abi.LUM_NPARAMS)[0])
    for name, st in _palette_textures().items():
        it, scene = _prep(mts, SC.e2e_description(mts, SC.scene_texture(mts.scenes, st), shape=shape, tilted=tilted), integ=integ())
        assert scene.spot_texture_args() is not None
        li = it.li_samples(samples)
        assert np.array_equal(bits(li[:, 3:]), bits(W[:, 3:])), "alpha, raster position and depth are those of the constant spot"
        base, unstable = R.decide_near(spot, st, p64, REACH)
        fragile = unstable | unsure
        sure = ~fragile
        want = W[:, :3] * base.tex.astype(np.float32)
        lit = sure & (W[:, :3] > 0).any(axis=1)
        print("%s / %s / %s / %s: %d samples, %d lit and sure, %d fragile" % (shape, "tilted" if tilted else "down", integrator, name, len(li), lit.sum(), fragile.sum()))
        assert np.array_equal(bits(li[sure, :3]), bits(want[sure])), (name, int((bits(li[sure, :3]) != bits(want[sure])).any(axis=1).sum()))
        assert lit.sum() > 100 and fragile.mean() <= MAX_FRAGILE, name
        # both colours (several texels) occur among the lit samples, and the texture changes the frame
        assert len(np.unique(base.tex[lit], axis=0)) >= 2 and not np.array_equal(bits(li[:, :3]), bits(W[:, :3])), name


# --- 5. the bilinear lookup end to end ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["4x4", "16x16"])
@pytest.mark.parametrize("wrap", [B.REPEAT, B.CLAMP, B.BLACK_MODE, B.WHITE_MODE])
def test_bilinear_ratio_against_the_restatement(gpu_lib, mts, size, wrap):
    """Per sample and channel the ratio of the textured sample to the constant spot's is the texture's value: held against the
    restatement at the binary64 hit point.  The tolerance, derived:
      the ratio itself: from result = intensity * tex on, the two renders run the same operations on operands that differ by the
      factor tex up to rounding: tex *, ramp *, invDist^2 *, / lumPdf, thr * value * bsdf * weight (3), the sum into Li: 8 operations,
      one rounding in each render: 16 u relative;
      the value: the restatement's first-order bound of the lookup at the mirror's uv (ref64_spot._bound, the bilinear part), plus
      the texel gradient times the uv error of a binary32 hit point: |d tex / d uv'| <= (largest difference of two of the four taps) *
      (w |uscale| + h |vscale|), and d uv <= 0.5 / (z uvFactor) * (1 + tan theta) * REACH / dist per component.
    The largest observed fraction of the tolerance is printed (DESIGN.md section 6 records it); it is not tuned."""
    w = int(size.split("x")[0])
    tx = np.random.RandomState(40 + w).uniform(0.05, 1.0, (w, w, 3)).astype(np.float32)
    # uv' covers [-0.5, 1.5] x [1.25, -0.25]: the bitmap and what lies around it on every side
    st = R.SpotTex(B.Bmp(tx, wrap, -0.5, 1.25, 2.0, -1.5), True)
    samples = _all_samples()
    it_w, scene_w = _prep(mts, SC.e2e_description(mts))
    W = it_w.li_samples(samples)
    p64, _ = _hit_points(it_w, "floor")
    spot = R.Spot(np.array(scene_w.arrays()["lum_params"]).reshape(-1, mts.abi.LUM_NPARAMS)[0])
    it, _ = _prep(mts, SC.e2e_description(mts, SC.scene_texture(mts.scenes, st), bilinear=True))
    li = it.li_samples(samples)
    base, unstable = R.decide_near(spot, st, p64, REACH)
    lit = ~unstable & base.inside & (W[:, :3] > 0).all(axis=1)
    assert lit.sum() > 300 and unstable.mean() <= MAX_FRAGILE
    ratio = li[lit, :3].astype(np.float64) / W[lit, :3].astype(np.float64)
    tex = base.tex[lit]
    # the restatement's bound of the value at these points (it takes binary32 points: the nearest ones)
    r = R.restate(spot, st, p64[lit].astype(np.float32))
    I = spot.intensity.astype(np.float64)[None, :]
    inv2 = (base.inv[lit] ** 2)[:, None]
    ramp = np.where(base.in_beam[lit], 1.0, base.ramp[lit])[:, None]
    e_value = r.bound / np.maximum(I * inv2 * np.abs(ramp), 1e-300)          # the bound on value, as a bound on tex
    cells = R.triangle_cells(st.tex, base.x[lit], base.y[lit], np.float64)[0]
    taps = np.stack([B.value(st.tex, c).astype(np.float64) for c in cells])    # [4][n][3]
    spread = taps.max(axis=0) - taps.min(axis=0)
    grad = spread * (w * abs(float(st.tex.uscale)) + w * abs(float(st.tex.vscale)))
    z = base.loc[2][lit]
    tan_t = np.sqrt(np.maximum(1 - z * z, 0)) / z
    d_uv = 0.5 / (z * base.f) * (1 + tan_t) * REACH * base.inv[lit]
    tol = 16 * U * tex + e_value + grad * d_uv[:, None]
    err = np.abs(ratio - tex)
    frac = np.where(err == 0, 0.0, err / np.maximum(tol, 1e-300))          # (under `black` value, error and tolerance can all be zero)
    print("bilinear %s / %s: %d samples, largest error over tolerance %.3f" % (size, B.WRAP_NAMES[wrap], lit.sum(), frac.max()))
    assert (frac <= 1.0).all()
    assert np.abs(ratio - 1.0).max() > 0.1 and len(np.unique(np.round(tex, 3), axis=0)) > 50, "the texture is seen"


# --- 6. one film across the ways of driving the bounces ------------------------------------------------------------------------------
@pytest.mark.parametrize("sky", [False, True])
def test_one_film_across_the_ways_of_driving_the_bounces(gpu_lib, mts, sky):
    """a textured spot and a plain point light in a room with a tangent mesh, a textured mesh, a composite and two spheres, in both
    integrators: host- and device-driven bounces, ragged passes, the closest-hit kernel with the mailbox and the lean one, two tile
    parts and a device group give the same bytes"""
    import tan_cases
    S = mts.scenes
    sd = tan_cases.mixed_scene(mts, sky=sky, extra="checkerboard")
    tx = SC.bilinear_texels("16x16")
    sd.spot_light((0.2, 1.8, 0.8), (-0.2, 0.0, -0.2), (30.0, 25.0, 20.0), cutoff_deg=35.0, beam_deg=25.0,
                  texture=S.BitmapTexture(texels=tx, wrap="repeat", uscale=2.0, vscale=-2.0, uoffset=0.25), bilinear=True)
    sd.point_light((-0.6, 1.5, 0.5), (1.0, 1.5, 2.0))
    sd.max_depth = 4
    scene = mts.Scene(sd)
    assert scene.spot_texture_args() is not None and scene.wants_tangents and scene.uv_texture_args() is not None
    res, spp = 16, 4
    cam = mts.PerspectiveCamera.for_description(sd, res, res)

    def render(integ, drive, part=0, n_parts=1, sc=scene):
        it = mts.MIPathTracer(maxDepth=sd.max_depth) if integ == "path" else mts.MIDirectIntegrator(*integ)
        it.preprocess(sc, cam, sampler="independent", sampleCount=spp, seed=5)
        if drive == 1: it.set_tuning(sync_free=0)
        elif drive == 2: it.set_tuning(sync_free=0); it.set_options(max_paths=spp * (res * res // 3 + 1))
        elif drive == 3: it.set_tuning(sync_free=1, shade_fused=0)
        elif drive == 4: it.set_tuning(lean_closest=0)
        elif drive == 5: it.set_tuning(sync_free=1, shade_fused=1)
        if n_parts > 1:
            it.set_tiles(8, part, n_parts)
        assert it.render()
        return it
    for integ in ("path", (1, 1), (2, 2)):
        base = render(integ, 0).film()
        assert np.isfinite(base).all() and (base[..., :3] > 0).any()
        for drive in (1, 2, 3, 4, 5):
            assert np.array_equal(bits(base), bits(render(integ, drive).film())), (integ, "drive %d differs from the default frame" % drive)
        total = sum(render(integ, 0, part, 2).film() for part in range(2))
        assert np.array_equal(bits(base), bits(total)), (integ, "two tile parts do not add up to the frame")
        g = mts.DeviceGroup([0, 0], maxDepth=sd.max_depth)
        g.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=5)
        if integ != "path":
            for i in range(len(g)):
                assert mts.lib().mtsgpu_set_direct_integrator(g.member(i), *integ) == 0
        assert g.render(block_size=8, ordered_reduce=True)
        assert np.array_equal(bits(base), bits(g.film())), (integ, "the two-member group's film differs")
        g.close()
    # the texture matters in this frame, and without it the frame is the one the tangent kernels render
    it = render("path", 0)
    full = it.film()
    it.set_spot_textures(); it.clear_film()
    assert it.render()
    off = it.film()
    assert not np.array_equal(bits(off), bits(full))
    sd.spot_textures = {}
    plain = render("path", 0, sc=mts.Scene(sd)).film()
    assert np.array_equal(bits(off), bits(plain))
