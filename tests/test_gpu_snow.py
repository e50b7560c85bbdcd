"""The snow BRDFs `wiscombe` and `hanrahankrueger` on the device: the read-out hook against the float32 mirror of
tests/ref64_snow.py bit for bit, the refusals of mtsgpu_set_snow_bsdfs in both call orders, frames that must not change (a table
of MTSGPU_SNOW_NONE, a table set and cleared, a masked Lambertian next to a snow entry), the closed form of a planar floor under
one directional light, the same floor under a constant background with MIS against quadrature (the t-test of the test-case mode), one film across
drivers, tile parts, ragged passes, a device group and both integrators, and the twosided adapter.  The host side is tests/test_snow.py.

Closed form.  A planar floor y = 0 (two triangles, face normal (0, 1, 0) exactly, so the shading frame is made of axis vectors and
its.wi, woL are the ray's and the light's components, sign and order aside, without a rounding), one directional light, `path` with
maxDepth = 2 or `direct`: the only radiance a sample collects is the direct light at the camera hit,

    Li = ((thr * value) * (f(wi, wo) * |cos wo|)) * weight          thr = 1 and weight = 1 (a delta light: bsdfPdf = 0), both exact,

two rounded products around f.  So |Li - I f64 cos| <= I cos (bound of f64) + gamma(2) I f64 cos + 2^-149 with f64 and its
first-order bound from ref64_snow.eval64 at the sample's own camera ray (mtsgpu_camera_rays) and gamma(2) = 2 U / (1 - 2 U),
U = 2^-24.  For the scenes below that is 11.6 to 12.1 units of 2^-24 of the value for the Wiscombe floor and 8.8 to 26.3 for the
HanrahanKrueger floor (the test prints the range)."""
import ctypes as C
import json

import numpy as np
import pytest

import ref64_snow as R
import snow_cases
import test_shade_matrix as M

pytestmark = pytest.mark.gpu

F = np.float32
U24 = 2.0 ** -24


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _all_samples(res_x, res_y, spp):
    y, x, j = np.meshgrid(np.arange(res_y), np.arange(res_x), np.arange(spp), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), j.ravel()], axis=1).astype(np.uint32)


def _integrator(mts, integ, max_depth):
    return mts.MIPathTracer(maxDepth=max_depth) if integ == "path" else mts.MIDirectIntegrator(*integ)


def _prep(mts, sd, res=32, spp=4, integ="path", max_depth=2, seed=5, res_y=None):
    scene = mts.Scene(sd)
    cam = mts.PerspectiveCamera.for_description(sd, res, res if res_y is None else res_y)
    it = _integrator(mts, integ, max_depth)
    it.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=seed)
    return it, scene


@pytest.fixture(scope="module")
def device(gpu_lib, mts):
    return mts.MIPathTracer(maxDepth=2)


# --- 1. the hook against the mirror, bit for bit ------------------------------------------------------------------------
def test_hook_equals_the_mirror_bit_for_bit(device, mts):
    """every model x class x plain / twosided x f / pdf / sample, the grazing class included; the derived values are the library's"""
    n = 0
    for name, kind, raw in snow_cases.models():
        entry = mts.snow_configure(kind, raw)
        D = np.float32(list(entry.derived))
        for cls in snow_cases.CLASSES:
            ewi, ewo = snow_cases.eval_records(cls)
            swi, ss = snow_cases.sample_records(cls)
            for two in (0, R.TWOSIDED):
                tag = (name, cls, two)
                want = R.eval32(kind, D, two != 0, 0, ewi, ewo)
                got = device.bsdf_eval_snow(two, entry, 0, ewi, ewo)
                assert np.array_equal(bits(got[:, :3]), bits(want.f)), (tag, "f", np.nonzero((bits(got[:, :3]) != bits(want.f)).any(axis=1))[0][:4])
                assert not got[:, 3:].any()
                want = R.eval32(kind, D, two != 0, 1, ewi, ewo)
                got = device.bsdf_eval_snow(two, entry, 1, ewi, ewo)
                assert np.array_equal(bits(got[:, 0]), bits(want.pdf)) and not got[:, 1:].any(), (tag, "pdf")
                want = R.eval32(kind, D, two != 0, 2, swi, ss)
                got = device.bsdf_eval_snow(two, entry, 2, swi, ss)
                for what, g, w in (("wo", got[:, 0:3], want.wo), ("pdf", got[:, 3], want.pdf), ("f", got[:, 4:7], want.f)):
                    same = bits(g) == bits(w)
                    nan = np.isnan(g) & np.isnan(w)          # 0 * inf at two denormal cosines: a NaN in both, whatever its payload
                    assert (same | nan).all(), (tag, "sample", what, np.nonzero(~(same | nan))[0][:4])
                assert np.array_equal(got[:, 7].view(np.uint32), want.stype.astype(np.uint32)), (tag, "sampledType")
                n += 2 * len(ewi) + len(swi)
    print("%d records" % n)
    assert n > 4000


def test_hook_kind_none_is_the_lambertian_hook_bit_for_bit(device, mts):
    A = mts.abi
    P = np.zeros(16, dtype=np.float32); P[:3] = [0.5, 0.6, 0.4]
    entry = (A.SNOW_NONE, P[:3])
    for cls in snow_cases.CLASSES:
        ewi, ewo = snow_cases.eval_records(cls)
        swi, ss = snow_cases.sample_records(cls)
        for two in (0, A.BSDF_TWOSIDED):
            for op, wi, aux in ((0, ewi, ewo), (1, ewi, ewo), (2, swi, ss)):
                assert np.array_equal(bits(device.bsdf_eval_snow(two, entry, op, wi, aux)), bits(device.bsdf_eval(A.BSDF_LAMBERTIAN | two, P, op, wi, aux))), (cls, two, op)


def test_hook_refusals(device, mts):
    A, L = mts.abi, mts.lib()
    one = [[0, 0, 1]]
    good = mts.snow_configure(A.SNOW_WISCOMBE, R.wiscombe_raw())
    for bad_type in (5, 9, 0x200, 0x105):
        with pytest.raises(mts.MtsGpuError, match="a snow record sits on a Lambertian entry"):
            device.bsdf_eval_snow(bad_type, good, 0, one, one)
    with pytest.raises(mts.MtsGpuError, match="bad BSDF type or operation"):
        device.bsdf_eval_snow(0, good, 3, one, one)
    with pytest.raises(mts.MtsGpuError, match="unknown snow kind 3"):
        device.bsdf_eval_snow(0, (3, [0.5]), 0, one, one)
    e = A.BsdfSnow(A.SNOW_HK, 7, good.derived)
    with pytest.raises(mts.MtsGpuError, match="the reserved word of its snow record is not zero"):
        device.bsdf_eval_snow(0, e, 0, one, one)
    with pytest.raises(mts.MtsGpuError, match="derived word 4 of its snow record is not finite"):
        device.bsdf_eval_snow(0, (A.SNOW_HK, [1, 1, 1, 1, np.inf]), 0, one, one)
    q = np.zeros(6, np.float32); out = np.zeros(8, np.float32)
    assert L.mtsgpu_bsdf_eval_snow(device._ctx, 0, None, 0, 1, A.ptr(q, A.f32p), A.ptr(out, A.f32p)) == -1
    assert L.mtsgpu_bsdf_eval_snow(device._ctx, 0, C.byref(good), 0, 1, None, A.ptr(out, A.f32p)) == -1
    assert L.mtsgpu_bsdf_eval_snow(device._ctx, 0, C.byref(good), 0, (1 << 24) + 1, A.ptr(q, A.f32p), A.ptr(out, A.f32p)) == -1
    assert L.mtsgpu_bsdf_eval_snow(device._ctx, 0, C.byref(good), 0, 0, A.ptr(q, A.f32p), A.ptr(out, A.f32p)) == 0


# --- 2. the refusals of mtsgpu_set_snow_bsdfs --------------------------------------------------------------------------
def _refusal_scene(mts):
    S = mts.scenes
    sd = S.SceneDescription("snow refusals")
    lam, met = sd.lambertian(0.6), sd.roughmetal(0.2)
    child = sd.lambertian(0.4)
    comp = sd.composite([0.5, 0.5], [child, sd.ward(0.2, 0.2)])
    two = sd.twosided(sd.lambertian(0.3))
    pos, tri, uv = S.tex_grid_mesh(2)
    sd.add_mesh(pos, tri, bsdf=lam, face_normals=True, name="floor", texcoords=uv, colors=np.full((len(pos), 3), 0.5, dtype=np.float32))
    sd.add_sphere((0, 0.5, 0), 0.3, bsdf=met)
    sd.add_sphere((0.8, 0.5, 0), 0.2, bsdf=comp)
    sd.add_sphere((-0.8, 0.5, 0), 0.2, bsdf=two)
    sd.point_light((0, 3, 1), 10.0)
    sd.camera = dict(origin=(0.0, 2.0, 3.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=39.3)
    sd.max_depth = 3
    return sd, dict(lam=lam, met=met, child=child, comp=comp, two=two)


def test_set_snow_bsdfs_refusals_in_both_call_orders(gpu_lib, mts):
    S, A = mts.scenes, mts.abi
    sd, b = _refusal_scene(mts)
    it, scene = _prep(mts, sd, max_depth=3)
    assert scene.bsdf_snow is None
    nb = len(sd.bsdf_type)
    w = mts.snow_configure(A.SNOW_WISCOMBE, R.wiscombe_raw())
    hk = mts.snow_configure(A.SNOW_HK, R.hk_raw())

    def film():
        it.clear_film(); assert it.render()
        return it.film().copy()
    off = film()

    def table(**rows):
        return [rows.get(k) for k in ("b%d" % i for i in range(nb))]

    def row(name, entry):
        return {"b%d" % b[name]: entry}

    def refused(call, *words):
        with pytest.raises(mts.MtsGpuError) as e:
            call()
        assert "code -1" in str(e.value), e.value
        for word in words:
            assert word in str(e.value), (word, str(e.value))
        return str(e.value)

    def snow_refused(rows, *words):
        refused(lambda: it.set_snow_bsdfs(table(**rows)), *words)
        assert np.array_equal(bits(film()), bits(off)), "a refused call leaves the table off"

    it.set_snow_bsdfs(table(**row("lam", w), **row("two", hk)))
    on = film()
    assert not np.array_equal(bits(on), bits(off)), "the table matters in this frame"
    snow_refused(row("lam", (3, [0.5])), "BSDF %d: unknown snow kind 3" % b["lam"])
    snow_refused(row("lam", A.BsdfSnow(A.SNOW_WISCOMBE, 1, w.derived)), "BSDF %d: the reserved word of its snow record is not zero" % b["lam"])
    for bad in (np.nan, np.inf, -np.inf):
        snow_refused(row("two", (A.SNOW_HK, [0.5, 0.5, bad])), "BSDF %d: derived word 2 of its snow record is not finite" % b["two"])
    snow_refused(row("met", w), "BSDF %d: a snow record sits on a Lambertian entry" % b["met"])
    snow_refused(row("comp", w), "BSDF %d: a snow record sits on a Lambertian entry" % b["comp"])
    snow_refused(row("child", hk), "BSDF %d: composite child 0 has a snow record" % b["comp"], "as a Lambertian")
    # a coloured slot, a textured slot, a mask: refused by whichever call comes second
    pool_c, has_c = scene.vertex_colors()
    pool_uv, has_uv = scene.vertex_texcoords()
    slots = np.zeros(nb, dtype=np.uint32); slots[b["lam"]] = 1
    check = S.Checkerboard()
    slot_tex = np.full((nb, 2), -1, dtype=np.int32); slot_tex[b["lam"], 0] = 0
    none = (A.MASK_NONE, -1, (0, 0, 0))
    masks = [none] * nb; masks[b["lam"]] = (A.MASK_CONSTANT, -1, (0.5, 0.5, 0.5))
    second = [
        (lambda: it.set_vertex_colors(pool_c, has_c, slots), lambda: it.set_vertex_colors(),
         "the entry takes vertex colours", "BSDF %d: the entry takes vertex colours and has a snow record" % b["lam"]),
        (lambda: it.set_uv_textures(pool_uv, has_uv, [check], slot_tex), lambda: it.set_uv_textures(),
         "the entry has a uv texture", "BSDF %d: the entry has a uv texture and a snow record" % b["lam"]),
        (lambda: it.set_uv_masked_textures(pool_uv, has_uv, None, None, None, None, masks), lambda: it.set_uv_masked_textures(),
         "a mask around a snow BRDF is not supported", "BSDF %d: the entry has a mask and a snow record" % b["lam"]),
    ]
    for other, other_off, snow_second, other_second in second:
        it.set_snow_bsdfs(None)
        other()
        with_other = film()
        refused(lambda: it.set_snow_bsdfs(table(**row("lam", w))), "BSDF %d" % b["lam"], snow_second)
        assert np.array_equal(bits(film()), bits(with_other)), "the refused snow table is off, what the other call set stays"
        # on another entry the two live together
        it.set_snow_bsdfs(table(**row("two", hk)))
        other_off()
        it.set_snow_bsdfs(table(**row("lam", w), **row("two", hk)))
        refused(other, other_second)
        assert np.array_equal(bits(film()), bits(on)), "the refused call is off, the snow table stays"
    # ownership: NULL and a table of NONE switch it off, a new upload clears it
    it.set_snow_bsdfs(None)
    assert np.array_equal(bits(film()), bits(off))
    it.set_snow_bsdfs(table(**row("lam", w), **row("two", hk)))
    it.set_snow_bsdfs(table())
    assert np.array_equal(bits(film()), bits(off))
    it.set_snow_bsdfs(table(**row("lam", w), **row("two", hk)))
    it.preprocess(scene, mts.PerspectiveCamera.for_description(sd, 32, 32), sampler="independent", sampleCount=4, seed=5)
    assert np.array_equal(bits(film()), bits(off)), "a new upload clears the snow table"
    fresh = mts.MIPathTracer(maxDepth=2)
    with pytest.raises(mts.MtsGpuError, match="mtsgpu_set_snow_bsdfs before mtsgpu_upload_scene"):
        fresh.set_snow_bsdfs(table(**row("lam", w)))


# --- 3. frames that must not change ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family, sky", [(f, s) for f in ("plain", "tex", "tan") for s in (False, True)])
def test_a_table_of_none_and_a_cleared_table_give_the_recorded_films(gpu_lib, mts, family, sky):
    """the launch-matrix scenes with a table of MTSGPU_SNOW_NONE (even cells) or a table set on the sphere row's Lambertian and
    cleared again (odd cells): every cell's film is the one tests/golden/shade_launch_matrix.json holds"""
    A = mts.abi
    golden = json.load(open(M.GOLDEN))["films"]
    sd = M.scene_description(mts, family, sky)
    scene = mts.Scene(sd)
    assert M.family_of(scene) == family and scene.bsdf_snow is None
    cam = mts.PerspectiveCamera.for_description(sd, M.RES, M.RES)
    nb = len(sd.bsdf_type)
    # the Lambertian of the sphere row: a constant block, no slot of it coloured or textured, and a composite's child where
    # the family has one -- so the set-and-cleared table sits on the last plain Lambertian that is no child
    children = set()
    for i, t in enumerate(sd.bsdf_type):
        if t & 0xFF == 9:
            k = int(sd.bsdf_params[i][0])
            children |= {int(c) for c in sd.bsdf_params[i][1 + k:1 + 2 * k]}
    free = [i for i, t in enumerate(sd.bsdf_type) if t & ~A.BSDF_TWOSIDED == A.BSDF_LAMBERTIAN and i not in children
            and not sd.bsdf_color_slots[i] and sd.bsdf_slot_texture[i] == [-1, -1] and i not in sd.bsdf_masks]
    w = mts.snow_configure(A.SNOW_WISCOMBE, R.wiscombe_raw())
    for k, (integ, drive) in enumerate((i, d) for i in M.INTEGRATORS for d in M.DRIVERS):
        it = _integrator(mts, M.INTEGRATORS[integ], M.MAX_DEPTH)
        it.preprocess(scene, cam, sampler="independent", sampleCount=M.SPP, seed=M.SEED)
        it.set_tuning(**M.DRIVERS[drive])
        if k % 2 == 0 or not free:
            it.set_snow_bsdfs([None] * nb)
        else:
            it.set_snow_bsdfs([w if i == free[-1] else None for i in range(nb)])
            it.set_snow_bsdfs(None)
        assert it.render()
        cell = M.cell_id(family, sky, integ, drive)
        assert M.film_hash(it.film()) == golden[cell], cell


def _floor_scene(S, floor, light=(0.3, -0.8, -0.5), intensity=(2.0, 1.5, 1.0), plate=None, camera=None, extent=10.0):
    """a planar floor y = 0 of two triangles under one directional light; plate: a small horizontal quad above it"""
    sd = S.SceneDescription("snow floor")
    pos, tri = S._quad((-extent, 0, -extent), (2 * extent, 0, 0), (0, 0, 2 * extent), (0, 1, 0))
    sd.add_mesh(pos, tri, bsdf=floor(sd), face_normals=True, name="floor")
    if plate is not None:
        pos, tri = S._quad((-0.3, 0.5, -0.3), (0.6, 0, 0), (0, 0, 0.6), (0, 1, 0))
        sd.add_mesh(pos, tri, bsdf=plate(sd), face_normals=True, name="plate")
    sd.directional_light(light, intensity)
    sd.camera = camera or dict(origin=(0.0, 1.0, 1.8), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=39.3)
    return sd


FLOORS = {"wiscombe": lambda sd: sd.wiscombe(), "hk": lambda sd: sd.hanrahan_krueger(g=0.5)}


def test_a_masked_lambertian_beside_a_snow_entry_keeps_its_samples(gpu_lib, mts):
    """a masked Lambertian plate above a floor, maxDepth = 2: the BSDF is evaluated at the camera hit alone, so no path meets both
    materials, and the samples whose camera ray meets the plate are those of the same scene with a plain Lambertian floor --
    through k_shade_snw here, through k_shade_msk there"""
    S = mts.scenes
    plate = lambda sd: sd.mask(sd.lambertian(0.7, 0.5, 0.3), 0.5)
    ps = _all_samples(32, 32, 4)
    it_s, sc_s = _prep(mts, _floor_scene(S, FLOORS["wiscombe"], plate=plate))
    it_l, sc_l = _prep(mts, _floor_scene(S, lambda sd: sd.lambertian(0.5), plate=plate))
    assert sc_s.bsdf_snow is not None and sc_s.bsdf_mask is not None and sc_l.bsdf_snow is None and sc_l.bsdf_mask is not None
    a, c = it_s.li_samples(ps), it_l.li_samples(ps)
    rays = it_s.camera_rays(ps.astype(np.int32)).astype(np.float64)
    t = (0.5 - rays[:, 1]) / rays[:, 5]
    x, z = rays[:, 0] + t * rays[:, 4], rays[:, 2] + t * rays[:, 6]
    on_plate = (np.abs(x) < 0.29) & (np.abs(z) < 0.29)
    off_plate = (np.abs(x) > 0.31) | (np.abs(z) > 0.31)
    assert on_plate.sum() > 100 and off_plate.sum() > 1000
    assert np.array_equal(bits(a[on_plate]), bits(c[on_plate])), "the masked plate's samples"
    assert (a[on_plate, :3] > 0).all(), "the plate is lit: f times p at every camera hit, whichever way the sample then goes"
    lit = off_plate & (c[:, :3] > 0).all(axis=1)
    assert lit.sum() > 500 and (bits(a[lit, :3]) != bits(c[lit, :3])).any(axis=1).mean() > 0.99, "the floor is another material"


# --- 4. closed form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integ", ["path", (1, 1)])
@pytest.mark.parametrize("model", sorted(FLOORS))
def test_a_floor_under_a_directional_light_is_the_closed_form(gpu_lib, mts, model, integ):
    """The derivation is the module's docstring.  Derived tolerance, relative to the value: 11.6 to 12.1 units of 2^-24 (wiscombe)
    and 8.8 to 26.3 (hk) over the samples of these frames; measured: the worst error is 0.35 and 0.47 of it, and every sample is
    bit-equal to intensity * (mirror f * cos)."""
    S, A = mts.scenes, mts.abi
    light, I = np.float32([0.3, -0.8, -0.5]), np.float64([2.0, 1.5, 1.0])
    sd = _floor_scene(S, FLOORS[model], light=light, intensity=I)
    it, scene = _prep(mts, sd, integ=integ)
    ps = _all_samples(32, 32, 4)
    li = it.li_samples(ps)
    assert (li[:, 3] == 1).all(), "every camera ray meets the floor"
    rays = it.camera_rays(ps.astype(np.int32))
    d = rays[:, 4:7]
    # local frame of the floor: N = (0, 1, 0); the order and the signs of the two tangent components change nothing bit for bit
    wi = np.stack([-d[:, 0], -d[:, 2], -d[:, 1]], axis=1).astype(np.float32)
    ln = light / np.sqrt((light * light).sum(), dtype=np.float32)
    wo = np.broadcast_to(np.float32([-ln[0], -ln[2], -ln[1]]), wi.shape)
    kind, raw = sd.bsdf_snow[0]
    D = np.float32(list(mts.snow_configure(kind, raw).derived))
    cos = float(wo[0, 2])
    f64 = R.eval64(kind, D, False, 0, wi, wo).f
    want = I[None, :] * f64.v * cos
    gamma2 = 2 * U24 / (1 - 2 * U24)
    tol = I[None, :] * cos * f64.e + gamma2 * np.abs(want) + 2.0 ** -149
    got = li[:, :3].astype(np.float64)
    err = np.abs(got - want)
    f32 = R.eval32(kind, D, False, 0, wi, wo).f
    exact = bits(li[:, :3]) == bits(np.float32(I)[None, :] * (f32 * F(cos)))
    print("%s, %s: tolerance %.2f to %.2f units of 2^-24 of the value; worst error %.3f of the tolerance; %.4f of the values bit-equal to the mirror"
          % (model, integ, (tol / np.abs(want)).min() / U24, (tol / np.abs(want)).max() / U24, (err / tol).max(), exact.mean()))
    assert (want > 0).all() and (err <= tol).all()
    # the check can fail: the mutations lie far outside
    for mutation in ("f_one_inv_pi", "mu_swapped") if model == "wiscombe" else ("ft_same_direction", "dot_without_minus"):
        wrong = I[None, :] * R.eval32(kind, D, False, 0, wi, wo, mutation).f.astype(np.float64) * cos
        margin = np.abs(got - wrong) / tol
        print("  %s: |Li - mutated| / tolerance between %.3g and %.3g" % (mutation, margin.min(), margin.max()))
        assert np.median(margin) > 100 and (margin > 1).mean() > 0.99, mutation


MIS_L, MIS_SPP, MIS_FOV = 4.0, 4096, 2.0


def _hemisphere_integral(kind, D, cos_wi, G):
    """what one sample of `path` with maxDepth = 2 expects of a floor under a constant background of radiance 1, per channel and for
    each cos(wi): the integral over the upper hemisphere of cos(wo) (f w_lum + s w_bsdf) dwo, with f the value of f(), s the value
    sample() returns for wo (Wiscombe: pi f, its sample() carries one 1 / pi where its f() carries two; HanrahanKrueger: f) and the
    two MIS weights of path.cpp:218-222 from pdf_lum = 1 / (4 pi) (constant.cpp:89-91) and pdf_bsdf = cos(wo) / pi.  The midpoint
    rule on G x G cells of (cos(wo), phi), the restatement's binary64 values.  The BRDFs are isotropic, so wi lies in the x-z plane.
    (eval64 takes binary32 queries: the nodes move by 2^-24 of themselves, seven orders below the error bar this is compared under.)"""
    mu = (np.arange(G) + 0.5) / G
    M, PH = np.meshgrid(mu, (np.arange(G) + 0.5) / G * 2 * np.pi, indexing="ij")
    s = np.sqrt(1 - M * M)
    wo = np.stack([s * np.cos(PH), s * np.sin(PH), M], axis=-1).reshape(-1, 3)
    out = []
    for c in cos_wi:
        wi = np.broadcast_to(np.float64([np.sqrt(1 - c * c), 0.0, c]), wo.shape)
        f = R.eval64(kind, D, False, 0, wi, wo).f.v
        sv = R.eval64(kind, D, False, 2, wi, np.zeros((len(wo), 2)), wo).f.v
        pl, pb = 1 / (4 * np.pi), wo[:, 2:3] / np.pi
        wl = pl * pl / (pl * pl + pb * pb)
        out.append((wo[:, 2:3] * (f * wl + sv * (1 - wl))).sum(axis=0) * (1.0 / G) * (2 * np.pi / G))
    return np.array(out)


def _pixel_expectation(kind, D, cam, sub, G):
    """the one pixel's expected radiance: MIS_L times the hemisphere integral, averaged over sub x sub points of the footprint"""
    r2c = np.array(list(cam.raster_to_camera), dtype=np.float64).reshape(4, 4)
    c2w = np.array(list(cam.camera_to_world), dtype=np.float64).reshape(4, 4)
    u = (np.arange(sub) + 0.5) / sub
    x, y = np.meshgrid(u * cam.width, u * cam.height, indexing="ij")
    ras = np.stack([x.ravel(), y.ravel(), 0 * x.ravel(), 1 + 0 * x.ravel()], axis=1)
    pc = ras @ r2c.T
    pc = pc[:, :3] / pc[:, 3:4]
    d = pc @ c2w[:3, :3].T
    d /= np.linalg.norm(d, axis=1)[:, None]
    return MIS_L * _hemisphere_integral(kind, D, -d[:, 1], G).mean(axis=0)


@pytest.mark.parametrize("model", sorted(FLOORS))
def test_a_floor_under_a_constant_background_passes_the_t_test_against_quadrature(gpu_lib, mts, model, tmp_path):
    """pdf() and sample() inside a frame, with MIS: the floor under a constant background L, `path` with maxDepth = 2, a film of one
    pixel as the reference's test scenes have, 4096 spp.  Expected: L times what _hemisphere_integral restates -- for a BRDF whose
    sample() agrees with its f() the integral of f cos, for the Wiscombe as written 2.7 times that -- over the pixel's footprint.  Accepted by testmode.analyze: Student's t per channel on the frame's
    own per-pixel variance (set_film_statistics) at the significance of the test-case mode, 0.01.  The quadrature's own error,
    bounded by halving both grids, has to stay below a tenth of the standard error."""
    S, T = mts.scenes, mts.testmode
    sd = S.SceneDescription("snow floor under a constant background")
    pos, tri = S._quad((-50, 0, -50), (100, 0, 0), (0, 0, 100), (0, 1, 0))
    sd.add_mesh(pos, tri, bsdf=FLOORS[model](sd), face_normals=True, name="floor")
    sd.add_lum(S.abi.LUM_CONSTANT, [MIS_L] * 3)
    sd.camera = dict(origin=(0.0, 1.0, 1.8), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=MIS_FOV)
    scene = mts.Scene(sd)
    cam = mts.PerspectiveCamera.for_description(sd, 1, 1)
    it = mts.MIPathTracer(maxDepth=2)
    it.preprocess(scene, cam, sampler="independent", sampleCount=MIS_SPP, seed=11)
    it.set_film_statistics(True)
    assert it.render()
    film = it.film()
    var, n = it.film_statistics()
    assert n[0, 0] == MIS_SPP and np.isfinite(film).all()
    kind, raw = sd.bsdf_snow[0]
    D = np.float32(list(mts.snow_configure(kind, raw).derived))
    E = _pixel_expectation(kind, D, cam.c, 4, 96)
    qerr = np.abs(E - _pixel_expectation(kind, D, cam.c, 4, 48)) + np.abs(E - _pixel_expectation(kind, D, cam.c, 2, 96))
    value = film[0, 0, :3].astype(np.float64) / film[0, 0, 4]
    se = np.sqrt(var[0, 0].astype(np.float64) / MIS_SPP)
    print("%s: expected %s, rendered %s, standard error %s, quadrature error <= %s, deviation %s standard errors"
          % (model, E, value, se, qerr, np.abs(value - E) / se))
    assert (E > 0.1).all() and (se > 0).all() and (se < 0.05 * E).all() and (qerr < 0.1 * se).all()
    m, ref = str(tmp_path / "floor.m"), str(tmp_path / "floor.ref")
    T.write_mfile(m, film, (var, n), spectra=True)
    open(ref, "w").write("[%s]\n" % " ".join("%f" % e for e in E))
    res = T.analyze(m, ref, T.T_TEST, 0.01)
    assert res[0], res[1]
    # the t-test can fail: an expectation six standard errors off is rejected (the accepted value lies within 2.6 of E)
    open(ref, "w").write("[%s]\n" % " ".join("%f" % e for e in E + 6 * se))
    assert not T.analyze(m, ref, T.T_TEST, 0.01)[0]


# --- 5. one film -------------------------------------------------------------------------------------------------------
def _one_film_scene(mts, sky):
    """a snow floor (wiscombe), a twosided hanrahankrueger wall, a Lambertian wall and a masked Lambertian plate"""
    S = mts.scenes
    sd = _floor_scene(S, FLOORS["wiscombe"], plate=lambda sd: sd.mask(sd.lambertian(0.7, 0.5, 0.3), 0.5), extent=2.0)
    pos, tri = S._quad((-2, 0, -2), (4, 0, 0), (0, 2, 0), (0, 0, 1))
    sd.add_mesh(pos, tri, bsdf=sd.lambertian(0.6, 0.3, 0.3), face_normals=True, name="wall")
    pos, tri = S._quad((-2, 0, -2), (0, 0, 4), (0, 2, 0), (1, 0, 0))
    sd.add_mesh(pos, tri, bsdf=sd.twosided(sd.hanrahan_krueger(g=-0.5)), face_normals=True, name="snow wall")
    sd.add_sphere((0.6, 0.3, 0.2), 0.3, bsdf=sd.roughmetal(0.2))
    sd.point_light((0.5, 1.5, 1.0), 4.0)
    if sky:
        sd.sky(sun_direction=(0.3, 0.2, 0.8), turbidity=3.0, sky_scale=0.2)
    sd.max_depth = 5
    return sd


@pytest.mark.parametrize("sky", [False, True])
def test_drivers_tile_parts_ragged_passes_group_and_direct_give_one_film(gpu_lib, mts, sky):
    A = mts.abi
    sd = _one_film_scene(mts, sky)
    scene = mts.Scene(sd)
    assert scene.bsdf_snow is not None and scene.bsdf_mask is not None
    assert sorted(scene.bsdf_snow[i].kind for i in range(len(sd.bsdf_type))).count(0) == len(sd.bsdf_type) - 2

    def render(integ, drive, res=(32, 32), spp=4, part=0, n_parts=1):
        cam = mts.PerspectiveCamera.for_description(sd, *res)
        it = _integrator(mts, integ, sd.max_depth)
        it.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=5)
        if drive == 1: it.set_tuning(sync_free=0)
        elif drive == 2: it.set_tuning(sync_free=0); it.set_options(max_paths=spp * (res[0] * res[1] // 3 + 1))
        elif drive == 3: it.set_tuning(sync_free=1, shade_fused=0)
        if n_parts > 1:
            it.set_tiles(16, part, n_parts)
        assert it.render()
        return it, it.film()
    for integ in ("path", (1, 1), (2, 3)):
        it0, base = render(integ, 0)
        assert np.isfinite(base).all() and (base[..., :3] > 0).any()
        entries = it0.bin_entries()
        assert entries[0] > 0 and entries[2] > 0 and sum(entries[1:2] + entries[3:10]) == 0, "the snow hits land in bin 0: %s" % entries
        assert np.array_equal(bits(base), bits(render(integ, 0)[1])), (integ, "a repeat run differs")
        for drive in (1, 2, 3):
            assert np.array_equal(bits(base), bits(render(integ, drive)[1])), (integ, "drive %d differs from the device-driven frame" % drive)
        total = sum(render(integ, 0, part=part, n_parts=2)[1] for part in range(2))
        assert np.array_equal(bits(base), bits(total)), (integ, "two tile parts do not add up to the frame")
        # ragged passes: 33 x 31 x 1 = 1023 paths and 41 x 25 x 1 = 1025, one below and one above a workgroup's 1024
        for res in ((33, 31), (41, 25)):
            ragged = render(integ, 0, res, 1)[1]
            for drive in (1, 3):
                assert np.array_equal(bits(ragged), bits(render(integ, drive, res, 1)[1])), (integ, res, drive)
        g = mts.DeviceGroup([0, 0], maxDepth=sd.max_depth)
        g.preprocess(scene, mts.PerspectiveCamera.for_description(sd, 32, 32), sampler="independent", sampleCount=4, seed=5)
        if integ != "path":
            for i in range(len(g)):
                assert mts.lib().mtsgpu_set_direct_integrator(g.member(i), *integ) == 0
        assert g.render(block_size=16, ordered_reduce=True)
        assert np.array_equal(bits(base), bits(g.film())), (integ, "the two-member group's film differs")
        g.close()
        if integ == "path":
            it0.set_snow_bsdfs(None)
            it0.clear_film()
            assert it0.render() and not np.array_equal(bits(it0.film()), bits(base)), "the snow table matters in this frame"


# --- 6. twosided -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", sorted(FLOORS))
def test_a_floor_seen_from_below_is_black_plain_and_the_view_from_above_when_twosided(gpu_lib, mts, model):
    """the view from below is the view from above turned by 180 degrees about the z axis, (x, y, z) -> (-x, -y, z): camera and
    light turn, the plane y = 0 stays; every ray and the light keep their components up to two signs, exactly, and the adapter
    flips wi.z and wo.z, so the twosided floor gives the same samples bit for bit"""
    S = mts.scenes
    above = dict(origin=(0.0, 1.0, 1.8), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=39.3)
    below = dict(origin=(0.0, -1.0, 1.8), target=(0.0, 0.0, 0.0), up=(0.0, -1.0, 0.0), fov=39.3)
    light_above, light_below = (0.3, -0.8, -0.5), (-0.3, 0.8, -0.5)
    ps = _all_samples(32, 32, 4)
    two = lambda sd: sd.twosided(FLOORS[model](sd))
    top = _prep(mts, _floor_scene(S, FLOORS[model], light=light_above, camera=above))[0].li_samples(ps)
    assert (top[:, :3] > 0).all() and (top[:, 3] == 1).all()
    plain = _prep(mts, _floor_scene(S, FLOORS[model], light=light_below, camera=below))[0].li_samples(ps)
    assert (plain[:, 3] == 1).all() and not plain[:, :3].any(), "seen from the back side the material is black"
    flipped = _prep(mts, _floor_scene(S, two, light=light_below, camera=below))[0].li_samples(ps)
    assert np.array_equal(bits(flipped[:, :4]), bits(top[:, :4]))
    assert np.array_equal(bits(_prep(mts, _floor_scene(S, two, light=light_above, camera=above))[0].li_samples(ps)[:, :4]), bits(top[:, :4]))
