"""The mask BSDF on the device: the adapter read out bit for bit against mtsgpu_bsdf_eval, opacity one through the mask kernels
against the films recorded long before them, the selection and the depth bookkeeping of the pass-through, exact scaling and
opaque shadows, a bitmap cutout, one film across drivers, and the refusals of mtsgpu_set_uv_masked_textures.  The host side is
tests/test_mask.py.

Selection scenes: black Lambertian quads that fill the view in front of a constant background L = 0.5.  A sample is then 0 (the
nested BSDF was chosen, or the depth ran out) or L times one factor b = x * (1 / x) per quad passed, x = (1 - p) |cosTheta|: the
value over the pdf of the pass-through, formed as shade_path forms it.  b lies in [1 - 2^-24, 1 + 2^-23], i.e. it is one of the
three binary32 values 1 - 2^-24, 1, 1 + 2^-23; L is a power of two and the MIS weight with lumPdf = 0 is exactly 1, so nothing
else is rounded.  Behind two quads the sample is L times the binary32 product of two such factors (the throughput is rounded
once per bounce): the square of that interval as the path forms it."""
import ctypes as C
import json

import numpy as np
import pytest

import mask_cases
import test_shade_matrix as M

pytestmark = pytest.mark.gpu

F = np.float32
L_BG = 0.5
B1 = sorted({float(F(1) - F(2.0 ** -24)), 1.0, float(F(1) + F(2.0 ** -23))})
B2 = sorted({float(F(a) * F(b)) for a in B1 for b in B1})
# miss_shaded x host- / device-driven loop
MODES = [(ms, sf) for ms in (0, 1) for sf in (1, 0)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _all_samples(res, spp):
    y, x, j = np.meshgrid(np.arange(res), np.arange(res), np.arange(spp), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), j.ravel()], axis=1).astype(np.uint32)


def _prep(mts, sd, res=32, spp=4, max_depth=None, rr_depth=10, seed=5):
    scene = mts.Scene(sd)
    cam = mts.PerspectiveCamera.for_description(sd, res, res)
    it = mts.MIPathTracer(maxDepth=sd.max_depth if max_depth is None else max_depth, rrDepth=rr_depth)
    it.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=seed)
    return it, scene


# --- 1. the hook, bit for bit ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device(gpu_lib, mts):
    return mts.MIPathTracer(maxDepth=2)


def test_hook_is_the_nested_read_out_through_the_mask_bit_for_bit(device, mts):
    ewi, ewo = mask_cases.eval_records()
    n_planted = n_nested = n_through = 0
    for name, btype, P in mask_cases.models(mts):
        plain_f, plain_pdf = device.bsdf_eval(btype, P, 0, ewi, ewo), device.bsdf_eval(btype, P, 1, ewi, ewo)
        for p in mask_cases.P_VALUES:
            p = F(p)
            tag = "%s, p = %g" % (name, p)
            got = device.bsdf_eval_masked(btype, P, [p, p, p], 0, ewi, ewo)
            assert np.array_equal(bits(got[:, :3]), bits(plain_f[:, :3] * p)), tag
            got = device.bsdf_eval_masked(btype, P, [p, p, p], 1, ewi, ewo)
            assert np.array_equal(bits(got[:, 0]), bits(plain_pdf[:, 0] * p)), tag
            wi, s = mask_cases.sample_records(p)
            got = device.bsdf_eval_masked(btype, P, [p, p, p], 2, wi, s)
            planted = mask_cases.planted_undefined(p, s)
            assert np.array_equal(planted, (p == 0) & (s[:, 0] == 0)) and planted.sum() == (2 * len(mask_cases.directions()) if p == 0 else 0)
            keep = ~planted
            nested = (s[:, 0] <= p) & keep
            with np.errstate(all="ignore"):
                q = s.copy(); q[:, 0] = np.where(nested, s[:, 0] / p, s[:, 0])
            plain = device.bsdf_eval(btype, P, 2, wi, q)
            want = np.zeros_like(got)
            want[:, 0:3] = np.where(nested[:, None], plain[:, 0:3], -wi)
            want[:, 3] = np.where(nested, plain[:, 3] * p, (F(1) - p) * np.abs(wi[:, 2]))
            want[:, 4:7] = np.where(nested[:, None], plain[:, 4:7] * p, (F(1) - p) * np.ones((1, 3), np.float32))
            want[:, 7] = np.where(nested, plain[:, 7], np.uint32([0x8]).view(np.float32)[0])
            bad = (bits(got) != bits(want)).any(axis=1) & keep
            assert not bad.any(), "%s: %d of %d sample records differ, first %s" % (tag, bad.sum(), keep.sum(), np.nonzero(bad)[0][:4])
            n_planted += int(planted.sum()); n_nested += int(nested.sum()); n_through += int((keep & ~nested).sum())
    print("%d nested, %d pass-through, %d planted undefined records" % (n_nested, n_through, n_planted))
    assert n_planted == 2 * len(mask_cases.directions()) * len(mask_cases.models(mts)) and n_nested > 1000 and n_through > 1000
    # the luminance is formed on the device: a colour acts as its luminance does
    for c in mask_cases.COLOURS:
        lum = (F(c[0]) * F(0.212671) + F(c[1]) * F(0.715160)) + F(c[2]) * F(0.072169)
        _, btype, P = mask_cases.models(mts)[0]
        got = device.bsdf_eval_masked(btype, P, c, 0, ewi, ewo)
        assert np.array_equal(bits(got[:, :3]), bits(device.bsdf_eval(btype, P, 0, ewi, ewo)[:, :3] * lum)), c


def test_hook_refusals(device, mts):
    one = [[0, 0, 1]]
    with pytest.raises(mts.MtsGpuError, match="a mask around a composite is not supported"):
        device.bsdf_eval_masked(9, np.zeros(16), [0.5] * 3, 0, one, one)
    with pytest.raises(mts.MtsGpuError, match="bad BSDF type or operation"):
        device.bsdf_eval_masked(0x200, np.zeros(16), [0.5] * 3, 0, one, one)
    with pytest.raises(mts.MtsGpuError, match="bad BSDF type or operation"):
        device.bsdf_eval_masked(0, np.zeros(16), [0.5] * 3, 3, one, one)
    A = mts.abi
    P = np.zeros(16, np.float32); q = np.zeros(6, np.float32); out = np.zeros(8, np.float32)
    L = mts.lib()
    assert L.mtsgpu_bsdf_eval_masked(device._ctx, 0, A.ptr(P, A.f32p), None, 0, 1, A.ptr(q, A.f32p), A.ptr(out, A.f32p)) == -1
    with pytest.raises(mts.MtsGpuError):
        device._chk(L.mtsgpu_bsdf_eval_masked(device._ctx, 0, A.ptr(P, A.f32p), A.ptr(q, A.f32p), 0, (1 << 24) + 1, A.ptr(q, A.f32p),
                                              A.ptr(out, A.f32p)), "bsdf_eval_masked")


# --- 2. opacity one changes nothing, through the mask kernels ----------------------------------------------------------
@pytest.mark.parametrize("family, sky", [(f, s) for f in ("plain", "tex", "tan") for s in (False, True)])
def test_opacity_one_is_the_recorded_film_through_the_mask_kernels(gpu_lib, mts, family, sky):
    """mask(1.0) on every non-composite BSDF of the launch-matrix scenes: s.x <= 1 always, and multiplying and dividing by 1 is
    exact, so every cell's film is the one tests/golden/shade_launch_matrix.json holds for the family -- through k_shade_msk<0..8>
    x ROUNDS x SKY and k_shade_all_msk, with the colour, texture-slot and tangent tables NULL where the family has none"""
    golden = json.load(open(M.GOLDEN))["films"]
    sd = M.scene_description(mts, family, sky)
    composite_children = set()
    for b, t in enumerate(sd.bsdf_type):
        if t & 0xFF == 9:
            n = int(sd.bsdf_params[b][0])
            composite_children |= {int(c) for c in sd.bsdf_params[b][1 + n:1 + 2 * n]}
    masked = [b for b, t in enumerate(sd.bsdf_type) if t & 0xFF != 9 and b not in composite_children]
    for b in masked:
        sd.mask(b, 1.0)
    # (a composite's children keep no mask: their own shapes go through the mask kernels with kind NONE)
    assert {sd.bsdf_type[b] & 0xFF for b in masked} >= set(range(1, 8)) and M.bins_of(sd) >= set(range(9)), "every bin of the mask family is filled"
    scene = mts.Scene(sd)
    # the masked launcher is the one taken: launch_shade / launch_shade_all look at the mask table first, and the context has one
    # exactly when the scene has (preprocess calls mtsgpu_set_uv_masked_textures then, and only then)
    assert scene.bsdf_mask is not None and scene.uv_masked_texture_args() is not None and M.family_of(scene) == family
    cam = mts.PerspectiveCamera.for_description(sd, M.RES, M.RES)
    for integ in M.INTEGRATORS:
        for drive in M.DRIVERS:
            cell = M.cell_id(family, sky, integ, drive)
            assert M.film_hash(M.render(mts, scene, cam, integ, drive)) == golden[cell], cell


# --- 3. selection and depth ----------------------------------------------------------------------------------------------
def _quads(S, n_quads, p):
    """black Lambertian quads facing the camera, filling its view, in front of the constant background L_BG"""
    sd = S.SceneDescription("mask quads")
    for k in range(n_quads):
        pos, tri = S._quad((-2, -2, -0.5 * k), (4, 0, 0), (0, 4, 0), (0, 0, 1))
        sd.add_mesh(pos, tri, bsdf=sd.mask(sd.lambertian(0.0), p), face_normals=True, name="quad %d" % k)
    sd.add_lum(S.abi.LUM_CONSTANT, [L_BG] * 3)
    sd.camera = dict(origin=(0.0, 0.0, 3.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=39.3)
    return sd


def _li(mts, sd, max_depth, rr_depth, ms, sf, res=32, spp=4):
    it, scene = _prep(mts, sd, res, spp, max_depth=max_depth, rr_depth=rr_depth)
    assert scene.bsdf_mask is not None
    it.set_tuning(miss_shaded=ms, sync_free=sf)
    li = it.li_samples(_all_samples(res, spp))
    assert np.isfinite(li).all() and (li[:, 3] == 1).all(), "alpha is 1 everywhere: every camera ray hits the quad"
    assert (li[:, 0] == li[:, 1]).all() and (li[:, 0] == li[:, 2]).all()
    return li[:, 0].astype(np.float64)


@pytest.mark.parametrize("ms, sf", MODES)
def test_one_quad_selection_and_depth(gpu_lib, mts, ms, sf):
    p = 0.25
    sd = _quads(mts.scenes, 1, p)
    v = _li(mts, sd, -1, 10, ms, sf)
    n = len(v)
    nz = v != 0
    ratio = v[nz] / L_BG
    print("one quad: %d of %d samples non-zero, factors %s" % (nz.sum(), n, sorted(set(ratio.tolist()))))
    assert ((ratio >= 1 - 2.0 ** -24) & (ratio <= 1 + 2.0 ** -23)).all()
    sigma = np.sqrt(n * p * (1 - p))
    assert abs(nz.sum() - n * (1 - p)) <= 5 * sigma
    assert (_li(mts, sd, 1, 10, ms, sf) == 0).all(), "maxDepth = 1: the pass-through is a bounce"
    assert np.array_equal(_li(mts, sd, 2, 10, ms, sf), v), "maxDepth = 2 is the unlimited frame"


@pytest.mark.parametrize("ms, sf", MODES)
def test_two_quads_selection_depth_and_roulette(gpu_lib, mts, ms, sf):
    p = 0.5
    sd = _quads(mts.scenes, 2, p)
    v = _li(mts, sd, -1, 10, ms, sf)
    n = len(v)
    for w, what in ((v, "unlimited depth"), (_li(mts, sd, 3, 10, ms, sf), "maxDepth = 3")):
        nz = w != 0
        share = 0.25
        sigma = np.sqrt(n * share * (1 - share))
        print("two quads, %s: %d of %d samples non-zero, factors %s" % (what, nz.sum(), n, sorted(set((w[nz] / L_BG).tolist()))))
        assert abs(nz.sum() - n * share) <= 5 * sigma, what
        assert np.isin(w[nz] / L_BG, B2).all(), what
        assert np.array_equal(w, v), what
    assert (_li(mts, sd, 2, 10, ms, sf) == 0).all(), "maxDepth = 2: the second quad is met at the depth limit"
    # rrDepth = 1: a pass-through is a transmission, exempt from Russian roulette -- no 1 / 0.9 factor, no sample consumed
    assert np.array_equal(_li(mts, sd, -1, 1, ms, sf), v)


# --- 4. scaling and opaque shadows ---------------------------------------------------------------------------------------
def _floor(S, floor_mask, plate=None):
    sd = S.SceneDescription("mask floor")
    white = sd.lambertian(1.0)
    pos, tri = S._quad((-1, 0, -1), (2, 0, 0), (0, 0, 2), (0, 1, 0))
    sd.add_mesh(pos, tri, bsdf=white if floor_mask is None else sd.mask(white, floor_mask), face_normals=True, name="floor")
    if plate is not None:
        # between the light and the floor, above the camera's view
        grey = sd.twosided(sd.lambertian(0.5))
        pos, tri = S._quad((-0.4, 2.5, -0.4), (0.8, 0, 0), (0, 0, 0.8), (0, -1, 0))
        sd.add_mesh(pos, tri, bsdf=grey if plate == "plain" else sd.mask(grey, 0.5), face_normals=True, name="plate")
    sd.point_light((0.0, 3.0, 0.0), 10.0)
    sd.camera = dict(origin=(0.0, 1.0, 1.8), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=39.3)
    return sd


def test_half_opacity_halves_every_sample_and_shadows_stay_opaque(gpu_lib, mts):
    S = mts.scenes
    ps = _all_samples(32, 4)
    plain = _prep(mts, _floor(S, None), max_depth=2)[0].li_samples(ps)
    half = _prep(mts, _floor(S, 0.5), max_depth=2)[0].li_samples(ps)
    assert (plain[:, :3] > 0).mean() > 0.3
    assert np.array_equal(bits(half[:, :3]), bits(plain[:, :3] * F(0.5))), "f and the light term scale by p = 0.5 exactly"
    assert np.array_equal(bits(half[:, 3:6]), bits(plain[:, 3:6]))
    films = {}
    for plate in ("plain", "masked"):
        it, scene = _prep(mts, _floor(S, 0.5, plate), max_depth=2)
        assert scene.bsdf_mask is not None
        assert it.render()
        films[plate] = it.film()
    assert np.array_equal(bits(films["plain"]), bits(films["masked"])), "shadow rays do not see masks: the plate occludes completely"
    it = _prep(mts, _floor(S, 0.5), max_depth=2)[0]
    assert it.render() and not np.array_equal(bits(it.film()), bits(films["plain"])), "the plate casts a shadow in this frame"


# --- 5. cutout -----------------------------------------------------------------------------------------------------------
CUT = np.float32([[1, 0, 0, 1], [0, 0, 1, 0], [1, 1, 0, 0], [0, 1, 0, 1]])          # [y][x]: 1 opaque, 0 cut out


def _cutout(S, opacity, nested=0.0):
    """a quad that fills the view exactly, uv from (0, 0) to (1, 1) across it: a texel of a 4 x 4 texture covers 8 x 8 pixels"""
    sd = S.SceneDescription("mask cutout")
    d = 3.0
    h = d * np.tan(np.radians(39.3 / 2))
    pos, tri = S._quad((-h, -h, 0), (2 * h, 0, 0), (0, 2 * h, 0), (0, 0, 1))
    uv = ((np.asarray(pos, dtype=np.float64)[:, :2] + h) / (2 * h)).astype(np.float32)
    sd.add_mesh(pos, tri, bsdf=sd.mask(sd.lambertian(nested), opacity), face_normals=True, name="cutout", texcoords=uv)
    sd.add_lum(S.abi.LUM_CONSTANT, [L_BG] * 3)
    sd.camera = dict(origin=(0.0, 0.0, d), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=39.3)
    return sd, h


@pytest.mark.parametrize("kind", ["bitmap", "checkerboard", "bitmap over a textured slot"])
def test_cutout(gpu_lib, mts, kind):
    S = mts.scenes
    if kind == "checkerboard":
        opacity = S.Checkerboard(bright=1.0, dark=0.0, uscale=2.0, vscale=2.0)       # (int) (2 uv') changes every quarter of uv
        opaque = lambda xi, yi: (xi & 1) == (yi & 1)
    else:
        opacity = S.BitmapTexture(texels=np.ascontiguousarray(np.repeat(CUT[:, :, None], 3, axis=2)), wrap="repeat")
        opaque = lambda xi, yi: CUT[yi, xi] == 1
    nested = S.GridTexture(bright=0.0, dark=0.0) if kind.endswith("slot") else 0.0
    sd, h = _cutout(S, opacity, nested)
    res, spp = 32, 4
    it, scene = _prep(mts, sd, res, spp)
    assert scene.bsdf_mask is not None and scene.bsdf_mask[0].kind == mts.abi.MASK_TEXTURE
    assert (scene.bsdf_slot_texture is not None) == kind.endswith("slot")
    ps = _all_samples(res, spp)
    li = it.li_samples(ps)
    assert np.isfinite(li).all() and (li[:, 3] == 1).all()
    # where each sample's ray meets the quad, in binary64 from the camera record of the sample
    rays = it.camera_rays(ps.astype(np.int32)).astype(np.float64)
    t = -rays[:, 2] / rays[:, 6]
    u = (rays[:, 0] + t * rays[:, 4] + h) / (2 * h) * 4
    v = (rays[:, 1] + t * rays[:, 5] + h) / (2 * h) * 4
    # a texel covers 8 pixels: at least one pixel away from its edges
    keep = (u % 1 >= 1 / 8) & (u % 1 <= 7 / 8) & (v % 1 >= 1 / 8) & (v % 1 <= 7 / 8) & (u > 0) & (u < 4) & (v > 0) & (v < 4)
    assert keep.mean() >= 0.5, "at most half of the samples are left out (%.3f kept)" % keep.mean()
    xi, yi = np.clip(np.floor(u).astype(int), 0, 3), np.clip(np.floor(v).astype(int), 0, 3)
    solid = opaque(xi, yi)
    val = li[:, 0].astype(np.float64)
    assert (li[:, 0] == li[:, 1]).all() and (li[:, 0] == li[:, 2]).all()
    print("%s: %.3f of the samples kept, %d under opaque texels, %d under cut-out texels" % (kind, keep.mean(), (keep & solid).sum(), (keep & ~solid).sum()))
    assert (keep & solid).sum() > 500 and (keep & ~solid).sum() > 500
    assert (val[keep & solid] == 0).all(), "opacity 1: the black nested BSDF, every time"
    ratio = val[keep & ~solid] / L_BG
    assert ((ratio >= 1 - 2.0 ** -24) & (ratio <= 1 + 2.0 ** -23)).all(), "opacity 0: straight through to the background"


# --- 6. one film ---------------------------------------------------------------------------------------------------------
def _mixed(mts, sky):
    """a masked bitmap quad, a masked constant sphere, mask(twosided(phong)), a coloured slot, a tangent mesh and a composite"""
    import tan_cases
    S = mts.scenes
    sd = tan_cases.mixed_scene(mts, sky=sky)
    cut = S.BitmapTexture(texels=np.ascontiguousarray(np.repeat(CUT[:, :, None], 3, axis=2)) * F(0.75), wrap="repeat", uscale=3.0, vscale=3.0)
    pos, tri = S._quad((-0.6, 0.3, 0.5), (0.5, 0, 0), (0, 0.5, 0), (0, 0, 1))
    uv = np.float32([[0, 0], [1, 0], [1, 1], [0, 1]])[:len(pos)]
    sd.add_mesh(pos, tri, bsdf=sd.mask(sd.lambertian(0.7, 0.6, 0.2), cut), face_normals=True, name="cutout", texcoords=uv)
    sd.add_sphere((0.3, 0.35, 0.55), 0.2, bsdf=sd.mask(sd.roughmetal(0.2), (0.6, 0.3, 0.9)))
    pos, tri = S._quad((0.1, 0.8, 0.4), (0.5, 0, 0), (0, 0.4, 0), (0, 0, 1))
    sd.add_mesh(pos, tri, bsdf=sd.mask(sd.twosided(sd.phong(20.0, rd=0.4, rs=0.3))), face_normals=True, name="sheet")
    g = S.vcol_grid(2).meshes[0]
    sd.add_mesh((g.positions * F(0.2) + np.float32([-0.5, 1.2, 0.3])).astype(np.float32), g.triangles, bsdf=sd.lambertian(S.VERTEX_COLORS),
                colors=g.colors, name="coloured")
    lam, ward = sd.lambertian(0.5), sd.ward(0.2, 0.2)
    sd.add_sphere((0.0, 1.4, 0.2), 0.12, bsdf=sd.composite([0.5, 0.5], [lam, ward]))
    return sd


@pytest.mark.parametrize("sky", [False, True])
def test_drivers_tile_parts_ragged_passes_group_and_direct_give_one_film(gpu_lib, mts, sky):
    sd = _mixed(mts, sky)
    scene = mts.Scene(sd)
    assert scene.bsdf_mask is not None and scene.wants_tangents and scene.bsdf_color_slots is not None
    assert sorted(scene.bsdf_mask[b].kind for b in sd.bsdf_masks) == [1, 1, 2] and 9 in {t & 0xFF for t in sd.bsdf_type}
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
        return it, it.film()
    for integ in ("path", (1, 1), (2, 3)):
        it0, base = render(integ, 0)
        assert np.isfinite(base).all() and (base[..., :3] > 0).any()
        for drive in (1, 2, 3):
            assert np.array_equal(bits(base), bits(render(integ, drive)[1])), (integ, "drive %d differs from the device-driven frame" % drive)
        total = sum(render(integ, 0, part, 2)[1] for part in range(2))
        assert np.array_equal(bits(base), bits(total)), (integ, "two tile parts do not add up to the frame")
        g = mts.DeviceGroup([0, 0], maxDepth=sd.max_depth)
        g.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=5)
        if integ != "path":
            for i in range(len(g)):
                assert mts.lib().mtsgpu_set_direct_integrator(g.member(i), *integ) == 0
        assert g.render(block_size=16, ordered_reduce=True)
        assert np.array_equal(bits(base), bits(g.film())), (integ, "the two-member group's film differs")
        g.close()
        if integ == "path":
            # the masks matter in this frame
            it0.set_uv_masked_textures()
            it0.clear_film()
            assert it0.render() and not np.array_equal(bits(it0.film()), bits(base))


# --- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_set_uv_masked_textures_refusals(gpu_lib, mts):
    S, A = mts.scenes, mts.abi
    sd = S.SceneDescription("mask refusals")
    lam, met = sd.lambertian(0.6), sd.roughmetal(0.2)
    child = sd.phong(10.0)
    comp = sd.composite([0.5, 0.5], [child, sd.ward(0.2, 0.2)])
    unused = sd.lambertian(0.3)                                                             # BSDF 5: no shape has it
    pos, tri, uv = S.tex_grid_mesh(2)
    sd.add_mesh(pos, tri, bsdf=lam, face_normals=True, name="floor", texcoords=uv)       # shape 0
    sd.add_sphere((0, 0.5, 0), 0.3, bsdf=met)                                             # shape 1
    sd.add_sphere((0.8, 0.5, 0), 0.2, bsdf=comp)                                          # shape 2
    sd.point_light((0, 3, 1), 10.0)
    sd.camera = dict(origin=(0.0, 2.0, 3.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=39.3)
    sd.max_depth = 3
    it, scene = _prep(mts, sd)
    assert scene.bsdf_mask is None
    assert it.render()
    off = it.film().copy()
    pool, has = scene.vertex_texcoords()
    check = S.Checkerboard(bright=1.0, dark=0.0, uscale=3.0, vscale=3.0)
    texs = [check.descriptor()]
    nb = len(sd.bsdf_type)
    none = (A.MASK_NONE, -1, (0, 0, 0))

    def table(**rows):
        return [rows.get("b%d" % b, none) for b in range(nb)]

    def attempt(masks, t=texs, p=pool, h=has):
        try:
            it.set_uv_masked_textures(p, h, t, None, None, None, masks)
        except mts.MtsGpuError as e:
            assert "code -1" in str(e), e
            it.clear_film(); assert it.render()
            assert np.array_equal(bits(it.film()), bits(off)), "a refused call leaves masks and textures switched off"
            return str(e)
        return ""

    C_float3 = C.c_float * 3

    def raw(**kw):
        m = A.BsdfMask(A.MASK_CONSTANT, -1, C_float3(0.5, 0.5, 0.5), 0)
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    good = table(b0=(A.MASK_TEXTURE, 0, (0, 0, 0)), b1=(A.MASK_CONSTANT, -1, (0.5, 0.5, 0.5)))
    assert attempt(good) == ""
    it.clear_film(); assert it.render()
    on = it.film().copy()
    assert not np.array_equal(bits(on), bits(off))
    assert "BSDF 1: unknown mask kind 3" in attempt(table(b1=raw(kind=3)))
    assert "BSDF 0: the reserved word of its mask is not zero" in attempt(table(b0=raw(reserved=7)))
    for bad in (np.nan, np.inf, -np.inf):
        assert "BSDF 1: the opacity of its mask is not finite" in attempt(table(b1=raw(opacity=C_float3(0.5, bad, 0.5)))), bad
    assert "BSDF 0: its mask names texture 1 of 1" in attempt(table(b0=(A.MASK_TEXTURE, 1, (0, 0, 0))))
    assert "BSDF 0: its mask names texture -1 of 1" in attempt(table(b0=(A.MASK_TEXTURE, -1, (0, 0, 0))))
    assert "BSDF 0: its mask names texture 0 of 0" in attempt(table(b0=(A.MASK_TEXTURE, 0, (0, 0, 0))), t=None)
    assert "BSDF %d: a mask around a composite is not supported" % comp in attempt(table(**{"b%d" % comp: raw()}))
    msg = attempt(table(**{"b%d" % child: raw()}))
    assert "BSDF %d: composite child 0 has a mask" % comp in msg, msg
    # the (int) cast of the mask's texture: on the shapes whose BSDF has the mask, and for a BSDF no shape uses
    huge = check.descriptor(); huge.uscale = 2.0e9
    msg = attempt(table(b0=(A.MASK_TEXTURE, 0, (0, 0, 0))), t=[huge])
    assert "shape 0: BSDF 0: the opacity of its mask: texture 0 maps a texcoord outside the range of the (int) cast" in msg, msg
    msg = attempt(table(b1=(A.MASK_TEXTURE, 0, (0, 0, 0))), t=[huge])
    assert "shape 1: BSDF 1" in msg, "the sphere too: " + msg
    assert attempt(table(**{"b%d" % unused: (A.MASK_TEXTURE, 0, (0, 0, 0))}), t=[huge]) == "", "uv = 0 is inside the range whatever the scale"
    far = check.descriptor(); far.voffset = -1.2e9
    msg = attempt(table(**{"b%d" % unused: (A.MASK_TEXTURE, 0, (0, 0, 0))}), t=[far])
    assert "BSDF %d: the opacity of its mask: texture 0 maps a texcoord outside the range" % unused in msg, msg
    assert attempt(table(b1=raw()), t=[far]) == "", "an unused texture's range is nobody's cast"
    # the checks of the older calls still hold
    assert "both be given or both be NULL" in attempt(good, h=None)
    # the older calls replace what this one set, and everything NULL switches it off
    assert attempt(good) == ""
    it.clear_film(); assert it.render()
    assert np.array_equal(bits(it.film()), bits(on))
    it.set_uv_bitmap_textures(pool, has, [check], None)
    it.clear_film(); assert it.render()
    assert np.array_equal(bits(it.film()), bits(off)), "the bitmap call knows no masks: they are gone"
    assert attempt(good) == ""
    it.set_uv_masked_textures()
    it.clear_film(); assert it.render()
    assert np.array_equal(bits(it.film()), bits(off))
    # a new upload clears the masks
    assert attempt(good) == ""
    it.preprocess(scene, mts.PerspectiveCamera.for_description(sd, 32, 32), sampler="independent", sampleCount=4, seed=5)
    it.clear_film(); assert it.render()
    assert np.array_equal(bits(it.film()), bits(off))
    fresh = mts.MIPathTracer(maxDepth=2)
    with pytest.raises(mts.MtsGpuError, match="mtsgpu_set_uv_masked_textures before mtsgpu_upload_scene"):
        fresh.set_uv_masked_textures(pool, has, texs, None, None, None, good)


def test_all_none_through_the_new_call_is_the_bitmap_call(gpu_lib, mts):
    sd = mts.scenes.cornell_bmp()
    it, scene = _prep(mts, sd)
    ps = _all_samples(32, 4)
    assert it.render()
    base_film, base_li = it.film().copy(), it.li_samples(ps)
    ub = scene.uv_bitmap_texture_args()
    none = mts.bsdf_mask_array([(0, -1, (0, 0, 0))] * len(sd.bsdf_type))
    for masks in (None, none):
        it._chk(mts.lib().mtsgpu_set_uv_masked_textures(it._ctx, *(ub + (masks,))), "set_uv_masked_textures")
        it.clear_film()
        assert it.render()
        assert (base_film[..., :3] > 0).any()
        assert np.array_equal(bits(it.film()), bits(base_film)) and np.array_equal(bits(it.li_samples(ps)), bits(base_li))
