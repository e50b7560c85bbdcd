"""The woven-cloth BRDF `irawan` on the device: mtsgpu_bsdf_eval_cloth -- the device function the cloth kernels call -- against
the float32 mirror of tests/ref64_cloth.py bit for bit, on every weave and record of tests/cloth_cases.py, all four ops, plain and
twosided; the mirror's seven-word Random against the device's whole generator (mtsgpu_random_values); the refusals of the hook
and of mtsgpu_set_cloth_bsdfs, in both call orders with the colour, texture, mask and snow calls; the recorded films of the
launch-matrix scenes with no table and with a table of -1; a cloth whose specular part is off against the Lambertian it then
is, film for film; two yarns whose kd differ by a factor of 4 against the one-yarn scene, sample for sample, on a floor and on a
sphere; one film across host- and device-driven loops, tile parts, ragged passes, a two-member group and both integrators.

and a specular floor, sample for sample, against intensity x f x cos of the binary64 restatement at the sample's own camera
ray.

The same on the quarter-cylinder patch of tests/tan_cases.py, whose frame comes from the uploaded tangents."""
import ctypes as C
import json

import numpy as np
import pytest

import cloth_cases as CC
import tan_cases
import ref64_cloth as R
import test_shade_matrix as M

pytestmark = pytest.mark.gpu

F = np.float32
INV_PI = F(0.31830988618379067154)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _all_samples(res_x, res_y, spp):
    y, x, j = np.meshgrid(np.arange(res_y), np.arange(res_x), np.arange(spp), indexing="ij")
    return np.stack([x.ravel(), y.ravel(), j.ravel()], axis=1).astype(np.uint32)


def _integrator(mts, integ, max_depth):
    return mts.MIPathTracer(maxDepth=max_depth) if integ == "path" else mts.MIDirectIntegrator(*integ)


def _prep(mts, sd, res=32, spp=4, integ="path", max_depth=2, seed=5):
    scene = mts.Scene(sd)
    cam = mts.PerspectiveCamera.for_description(sd, res, res)
    it = _integrator(mts, integ, max_depth)
    it.preprocess(scene, cam, sampler="independent", sampleCount=spp, seed=seed)
    return it, scene


@pytest.fixture(scope="module")
def device(gpu_lib, mts):
    return mts.MIPathTracer(maxDepth=2)


@pytest.fixture(scope="module")
def weaves(mts):
    return CC.weaves(mts)


def _same(got, want):
    """bit for bit, a NaN in both whatever its payload"""
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


# --- 1. the hook against the mirror, bit for bit ------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(11))
def test_hook_equals_the_mirror_bit_for_bit(device, weaves, k):
    """one weave of cloth_cases.weaves(): random and named records x plain / twosided x f / pdf / sample / the internals.  The
    internals are compared first, so that a failure names the stage: yarn id, centre, random1, random2, intensityVariation, u, v"""
    name, W = weaves[k]
    rwi, rwo, ruv, rs = (np.concatenate(p) for p in zip(CC.random_records(100 + k), CC.outside_records(100 + k)))
    names, nwi, nwo, nuv, ns = CC.named_records(W)
    if not (W.period > 0 or W.fineness > 0):      # the highlight tests' own thresholds, bracketed to one binary32 step
        tn, twi, two_, tuv, ts = CC.threshold_records(W)
        assert len(tn) >= 60
        names, nwi, nwo, nuv, ns = names + tn, np.concatenate([nwi, twi]), np.concatenate([nwo, two_]), np.concatenate([nuv, tuv]), np.concatenate([ns, ts])
    wi, wo, uv, s = np.concatenate([rwi, nwi]), np.concatenate([rwo, nwo]), np.concatenate([ruv, nuv]), np.concatenate([rs, ns])
    index = np.nonzero(CC.usable(W, uv))[0]      # with the noise on, a negative xy is refused: its casts leave their range
    wi, wo, uv, s = wi[index], wo[index], uv[index], s[index]
    stages = ("yarn id", "centre x", "centre y", "random1", "random2", "intensityVariation", "u", "v")
    for two in (0, R.TWOSIDED):
        for op, aux in ((3, wo), (0, wo), (1, wo), (2, s)):
            want = R.eval32(W, two != 0, op, wi, aux, uv)
            got = device.bsdf_eval_cloth(two, W, op, wi, aux, uv)
            ok = _same(got, want)
            bad = np.nonzero(~ok.all(axis=1))[0]
            where = [(int(index[i]), names[index[i] - len(rwi)] if index[i] >= len(rwi) else "random", [stages[c] if op == 3 else int(c) for c in np.nonzero(~ok[i])[0]],
                      got[i].tolist(), want[i].tolist()) for i in bad[:3]]
            assert not len(bad), (name, "twosided" if two else "plain", "op %d" % op, "%d records differ" % len(bad), where)
    live = (wi[:, 2] > 0) & (wo[:, 2] > 0)
    assert live.sum() > 2000


def test_the_seven_word_generator_is_the_device_generator(device, mts):
    """the first three nextULong() of Random(seed): the mirror's seven words of the seeding recurrence -- the form the cloth's
    device function runs, compared through random1 / random2 / intensityVariation above -- against the device's whole 312-word
    generator.  Non-zero seeds: to mtsgpu_random_values a seed of 0 means a default-constructed Random"""
    rng = np.random.RandomState(3)
    seeds = [1, 2, 5489, 1 << 32, (1 << 64) - 1] + [int(x) for x in rng.randint(1, 1 << 62, size=20, dtype=np.int64)]
    want = R.random_first_three(np.array(seeds, dtype=np.uint64))
    for i, seed in enumerate(seeds):
        got = device.random_values(0, 3, seed)
        assert [int(x) for x in got] == [int(x) for x in want[:, i]], seed


def test_hook_refusals(device, mts, weaves):
    A, L = mts.abi, mts.lib()
    W = weaves[0][1]
    one, uv = [[0, 0, 1]], [[0.3, 0.3]]
    for bad_type in (5, 9, 0x200, 0x105):
        with pytest.raises(mts.MtsGpuError, match="a weave sits on a Lambertian entry"):
            device.bsdf_eval_cloth(bad_type, W, 0, one, one, uv)
    with pytest.raises(mts.MtsGpuError, match="bad BSDF type or operation"):
        device.bsdf_eval_cloth(0, W, 4, one, one, uv)
    with pytest.raises(mts.MtsGpuError, match="pattern size 3 is not tileWidth \\* tileHeight = 4"):
        device.bsdf_eval_cloth(0, mts.Weave(W.name, W.pattern[:3], W.yarns, **{n: getattr(W, n) for n in A.WEAVE_SCALARS}), 0, one, one, uv)
    with pytest.raises(mts.MtsGpuError, match="outside the range of the \\(int\\) cast"):
        device.bsdf_eval_cloth(0, W, 0, one, one, [[2.0e9, 0.3]])
    with pytest.raises(mts.MtsGpuError, match="a noise argument can leave the range of floorToInt"):
        device.bsdf_eval_cloth(0, W.replace(period=1e-6), 0, one, one, [[-0.5, 0.3]])
    with pytest.raises(mts.MtsGpuError, match="a fineness seed factor can leave the range of its cast"):
        device.bsdf_eval_cloth(0, W.replace(fineness=1.0), 0, one, one, [[-0.5, 0.3]])
    with pytest.raises(mts.MtsGpuError, match="non-finite texcoord"):
        device.bsdf_eval_cloth(0, W, 0, one, one, [[np.nan, 0.3]])
    arr, keep = mts.weave_array([W])
    q = np.zeros(8, np.float32); out = np.zeros(8, np.float32)
    assert L.mtsgpu_bsdf_eval_cloth(device._ctx, 0, None, 0, 1, A.ptr(q, A.f32p), A.ptr(out, A.f32p)) == -1
    assert L.mtsgpu_bsdf_eval_cloth(device._ctx, 0, arr, 0, 1, None, A.ptr(out, A.f32p)) == -1
    assert L.mtsgpu_bsdf_eval_cloth(device._ctx, 0, arr, 0, 0, A.ptr(q, A.f32p), A.ptr(out, A.f32p)) == 0


# --- 2. the refusals of mtsgpu_set_cloth_bsdfs -------------------------------------------------------------------------
def _refusal_scene(mts):
    S = mts.scenes
    sd = S.SceneDescription("cloth refusals")
    lam, met = sd.lambertian(0.6), sd.roughmetal(0.2)
    child = sd.lambertian(0.4)
    comp = sd.composite([0.5, 0.5], [child, sd.ward(0.2, 0.2)])
    two = sd.twosided(sd.lambertian(0.3))
    bare = sd.lambertian(0.2)
    smooth = sd.lambertian(0.25)
    pos, tri, uv = S.tex_grid_mesh(2)
    sd.add_mesh(pos, tri, bsdf=lam, face_normals=True, name="floor", texcoords=uv, colors=np.full((len(pos), 3), 0.5, dtype=np.float32))
    sd.add_sphere((0, 0.5, 0), 0.3, bsdf=met)
    sd.add_sphere((0.8, 0.5, 0), 0.2, bsdf=comp)
    sd.add_sphere((-0.8, 0.5, 0), 0.2, bsdf=two)
    pos, tri = S._quad((-3, -0.5, -3), (6, 0, 0), (0, 0, 6), (0, 1, 0))
    sd.add_mesh(pos, tri, bsdf=bare, face_normals=True, name="no texcoords")
    pos, tri = S._quad((-3, -0.7, -3), (6, 0, 0), (0, 0, 6), (0, 1, 0))
    sd.add_mesh(pos, tri, bsdf=smooth, face_normals=False, name="vertex normals, no tangents", texcoords=[(0, 0), (1, 0), (1, 1), (0, 1)])
    sd.point_light((0, 3, 1), 10.0)
    sd.camera = dict(origin=(0.0, 2.0, 3.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=39.3)
    sd.max_depth = 3
    return sd, dict(lam=lam, met=met, child=child, comp=comp, two=two, bare=bare, smooth=smooth)


def test_set_cloth_bsdfs_refusals_in_both_call_orders(gpu_lib, mts, weaves):
    S, A = mts.scenes, mts.abi
    sd, b = _refusal_scene(mts)
    it, scene = _prep(mts, sd, max_depth=3)
    assert scene.cloth is None
    nb = len(sd.bsdf_type)
    W, W2 = weaves[0][1], weaves[8][1]      # on the floor, whose texcoords reach below zero, the noise is off; on the sphere it is on
    pool_c, has_c = scene.vertex_colors()
    pool_uv, has_uv = scene.vertex_texcoords()

    def film():
        it.clear_film(); assert it.render()
        return it.film().copy()
    off = film()

    def table(**rows):
        t = np.full(nb, -1, dtype=np.int32)
        for name, k in rows.items():
            t[b[name]] = k
        return t

    def refused(call, *words):
        with pytest.raises(mts.MtsGpuError) as e:
            call()
        assert "code -1" in str(e.value), e.value
        for word in words:
            assert word in str(e.value), (word, str(e.value))

    # before the texture call: a cloth mesh has no texcoords on the device yet
    refused(lambda: it.set_cloth_bsdfs([W], table(lam=0)), "shape 0", "needs texture coordinates")
    it.set_uv_textures(pool_uv, has_uv, None, None)
    assert np.array_equal(bits(film()), bits(off)), "texcoords alone change nothing"

    def cloth_refused(ws, rows, *words):
        refused(lambda: it.set_cloth_bsdfs(ws, table(**rows)), *words)
        assert np.array_equal(bits(film()), bits(off)), "a refused call leaves the table off"

    it.set_cloth_bsdfs([W, W2], table(lam=0, two=1))
    on = film()
    assert not np.array_equal(bits(on), bits(off)), "the table matters in this frame"
    scal = lambda w: {n: getattr(w, n) for n in A.WEAVE_SCALARS}
    cloth_refused([mts.Weave("", W.pattern[:3], W.yarns, **scal(W))], dict(lam=0), "weave 0: pattern size 3 is not tileWidth * tileHeight = 4")
    cloth_refused([W.replace(tileWidth=0)], dict(lam=0), "weave 0: zero tile dimension")
    cloth_refused([mts.Weave("", [1, 2, 3, 1], W.yarns, **scal(W))], dict(lam=0), "weave 0: pattern entry 2 = 3 is outside 1..2")
    cloth_refused([mts.Weave("", [1, 0, 2, 1], W.yarns, **scal(W))], dict(lam=0), "weave 0: pattern entry 1 = 0 is outside 1..2")
    bad_yarn = mts.Yarn(type=2, umax=0.5, width=1, length=1)
    cloth_refused([mts.Weave("", W.pattern, [W.yarns[0], bad_yarn], **scal(W))], dict(lam=0), "weave 0: yarn 1: unknown type 2")
    for bad in (np.nan, np.inf):
        cloth_refused([W.replace(beta=bad)], dict(lam=0), "weave 0: beta is not finite")
    for kw in (dict(width=0.0), dict(length=-1.0), dict(umax=0.0)):
        y = mts.Yarn(**{**dict(type="warp", umax=0.5, width=1, length=1), **kw})
        cloth_refused([mts.Weave("", W.pattern, [W.yarns[0], y], **scal(W))], dict(lam=0), "weave 0: yarn 1: width, length and umax must be positive")
    cloth_refused([W.replace(warpArea=0.0)], dict(lam=0), "weave 0: warpArea and weftArea must be positive")
    cloth_refused([W.replace(period=-1.0)], dict(lam=0), "weave 0: fineness and period must not be negative")
    cloth_refused([W], dict(lam=1), "BSDF %d: weave index 1 out of range (1 weaves)" % b["lam"])
    cloth_refused([W], dict(met=0), "BSDF %d: a weave sits on a Lambertian entry" % b["met"])
    cloth_refused([W], dict(comp=0), "BSDF %d: a weave sits on a Lambertian entry" % b["comp"])
    cloth_refused([W], dict(child=0), "BSDF %d: composite child 0 has a weave" % b["comp"], "as a Lambertian")
    cloth_refused([W], dict(bare=0), "shape 4", "needs texture coordinates")
    cloth_refused([W], dict(smooth=0), "shape 5", "a mesh with vertex normals needs its tangents")
    cloth_refused([W.replace(repeatU=1e10)], dict(lam=0), "shape 0: weave 0", "outside the range of the (int) cast")
    cloth_refused([W.replace(period=1e-6)], dict(lam=0), "shape 0: weave 0", "a noise argument can leave the range of floorToInt")
    cloth_refused([W.replace(fineness=1e9)], dict(two=0), "shape 3: weave 0", "a fineness seed factor can leave the range of its cast")
    # a coloured slot, a textured slot, a mask, a snow record: refused by whichever call comes second
    slots = np.zeros(nb, dtype=np.uint32); slots[b["lam"]] = 1
    check = S.Checkerboard()
    slot_tex = np.full((nb, 2), -1, dtype=np.int32); slot_tex[b["lam"], 0] = 0
    none = (A.MASK_NONE, -1, (0, 0, 0))
    masks = [none] * nb; masks[b["lam"]] = (A.MASK_CONSTANT, -1, (0.5, 0.5, 0.5))
    snow = [None] * nb; snow[b["lam"]] = mts.snow_configure(A.SNOW_WISCOMBE, np.float32([0.874, 1.0, 0.99, 0.99, 0.99, 16.4967, 6.0957, 4.6547]))
    uv_only = lambda: it.set_uv_textures(pool_uv, has_uv, None, None)
    second = [
        (lambda: it.set_vertex_colors(pool_c, has_c, slots), lambda: it.set_vertex_colors(),
         "the entry takes vertex colours", "BSDF %d: the entry takes vertex colours and has a weave" % b["lam"]),
        (lambda: it.set_uv_textures(pool_uv, has_uv, [check], slot_tex), uv_only,
         "the entry has a uv texture", "BSDF %d: the entry has a uv texture and a weave" % b["lam"]),
        (lambda: it.set_uv_masked_textures(pool_uv, has_uv, None, None, None, None, masks), uv_only,
         "a mask around a cloth BRDF is not supported", "BSDF %d: the entry has a mask and a weave" % b["lam"]),
        (lambda: it.set_snow_bsdfs(snow), lambda: it.set_snow_bsdfs(None),
         "the entry has a snow record and a weave", "BSDF %d: the entry has a weave and a snow record" % b["lam"]),
    ]
    for other, other_off, cloth_second, other_second in second:
        it.set_cloth_bsdfs()
        other()
        with_other = film()
        refused(lambda: it.set_cloth_bsdfs([W], table(lam=0)), "BSDF %d" % b["lam"], cloth_second)
        assert np.array_equal(bits(film()), bits(with_other)), "the refused cloth table is off, what the other call set stays"
        other_off()
        it.set_cloth_bsdfs([W, W2], table(lam=0, two=1))
        refused(other, other_second)
        assert np.array_equal(bits(film()), bits(on)), "the refused call changes nothing, the cloth table stays"
    # any texture call while a table is in force: the texture call comes first
    refused(uv_only, "while a cloth table is in force")
    assert np.array_equal(bits(film()), bits(on))
    # ownership: NULL and a table of -1 switch it off, a new upload clears it
    it.set_cloth_bsdfs()
    assert np.array_equal(bits(film()), bits(off))
    it.set_cloth_bsdfs([W, W2], table(lam=0, two=1))
    it.set_cloth_bsdfs([W, W2], table())
    assert np.array_equal(bits(film()), bits(off))
    it.set_cloth_bsdfs([W, W2], table(lam=0, two=1))
    it.preprocess(scene, mts.PerspectiveCamera.for_description(sd, 32, 32), sampler="independent", sampleCount=4, seed=5)
    assert np.array_equal(bits(film()), bits(off)), "a new upload clears the cloth table"
    fresh = mts.MIPathTracer(maxDepth=2)
    with pytest.raises(mts.MtsGpuError, match="mtsgpu_set_cloth_bsdfs before mtsgpu_upload_scene"):
        fresh.set_cloth_bsdfs([W], table(lam=0))


# --- 3. frames that must not change ------------------------------------------------------------------------------------
@pytest.mark.parametrize("family, sky", [(f, s) for f in ("plain", "tex", "tan") for s in (False, True)])
def test_no_table_and_a_table_of_minus_one_give_the_recorded_films(gpu_lib, mts, family, sky, weaves):
    """the launch-matrix scenes without a cloth call (even cells) and with a table of -1 alone (odd cells): every cell's film is
    the one tests/golden/shade_launch_matrix.json holds"""
    golden = json.load(open(M.GOLDEN))["films"]
    sd = M.scene_description(mts, family, sky)
    scene = mts.Scene(sd)
    assert M.family_of(scene) == family and scene.cloth is None
    cam = mts.PerspectiveCamera.for_description(sd, M.RES, M.RES)
    nb = len(sd.bsdf_type)
    for k, (integ, drive) in enumerate((i, d) for i in M.INTEGRATORS for d in M.DRIVERS):
        it = _integrator(mts, M.INTEGRATORS[integ], M.MAX_DEPTH)
        it.preprocess(scene, cam, sampler="independent", sampleCount=M.SPP, seed=M.SEED)
        it.set_tuning(**M.DRIVERS[drive])
        if k % 2:
            it.set_cloth_bsdfs([weaves[0][1]], np.full(nb, -1, dtype=np.int32))
        assert it.render()
        cell = M.cell_id(family, sky, integ, drive)
        assert M.film_hash(it.film()) == golden[cell], cell


# --- 4. the diffuse part alone -----------------------------------------------------------------------------------------
QUAD_UV = [(0, 0), (1, 0), (1, 1), (0, 1)]


def _diffuse_weave(mts, kds, pattern=(1, 2, 2, 1), tile=(2, 2), repeat=(3.0, 2.0)):
    """ksMultiplier = 0, kdMultiplier = 1: f is the yarn's kd where both directions are above the surface"""
    yarns = [mts.Yarn(type="warp" if i % 2 == 0 else "weft", umax=0.5, width=1, length=1, centerU=0.25, centerV=0.25, kd=kd) for i, kd in enumerate(kds)]
    return mts.Weave("diffuse", pattern, yarns, tileWidth=tile[0], tileHeight=tile[1], warpArea=1, weftArea=1, hWidth=0.5, beta=1.0,
                     repeatU=repeat[0], repeatV=repeat[1], kdMultiplier=1.0, ksMultiplier=0.0)


def _box(mts, material):
    """the five faces of the Cornell box with texcoords, a block in it, an area light; material(sd, rho) makes a face's BSDF"""
    S = mts.scenes
    sd = S.SceneDescription("cloth box")
    rho = {"left": (0.63, 0.065, 0.05), "right": (0.14, 0.45, 0.091)}
    for name, p0, e1, e2, nrm in S._box_faces():
        pos, tri = S._quad(p0, e1, e2, nrm)
        sd.add_mesh(pos, tri, bsdf=material(sd, rho.get(name, (0.73, 0.73, 0.73))), face_normals=True, name=name, texcoords=QUAD_UV)
    sd.add_sphere((0.3, 0.4, 0.1), 0.4, bsdf=material(sd, (0.5, 0.6, 0.7)))
    S._add_light(sd, intensity=4.0)
    sd.max_depth = 5
    return sd


def test_a_cloth_without_its_specular_part_is_the_lambertian_film_for_film(gpu_lib, mts):
    """ksMultiplier = 0, every yarn's kd = float32(rho * INV_PI), kdMultiplier = 1: the 32 x 32, 16-spp, maxDepth-5 film of the box
    equals the film of the box of Lambertians, byte for byte -- through k_shade_clo here, through the plain kernels there"""
    def cloth(sd, rho):
        kd = [float(F(r) * INV_PI) for r in rho]
        return sd.irawan(_diffuse_weave(mts, [kd, kd]))
    films = {}
    for name, material in (("cloth", cloth), ("lambertian", lambda sd, rho: sd.lambertian(*rho))):
        sd = _box(mts, material)
        it, scene = _prep(mts, sd, res=32, spp=16, max_depth=5)
        assert (scene.cloth is not None) == (name == "cloth")
        assert it.render()
        films[name] = it.film().copy()
        entries = it.bin_entries()
        assert entries[0] > 0 and sum(entries[1:10]) == 0
    assert (films["lambertian"][..., :3] > 0).any()
    assert np.array_equal(bits(films["cloth"]), bits(films["lambertian"]))


@pytest.mark.parametrize("shape", ["floor", "sphere"])
def test_two_yarns_whose_kd_differ_by_four_give_one_or_four_times_the_one_yarn_sample(gpu_lib, mts, shape):
    """ks = 0, a directional light, the direct integrator with one luminaire sample: every radiance sample of the two-yarn scene
    is exactly 1 or 4 times the sample of the scene whose yarns share the smaller kd (a power of two scales exactly), and both
    factors occur -- the pattern lookup at its.uv is the only thing that differs"""
    S = mts.scenes

    def scene_of(kds):
        sd = S.SceneDescription("cloth kd")
        b = sd.irawan(_diffuse_weave(mts, kds, repeat=(5.0, 7.0)))
        if shape == "floor":
            pos, tri = S._quad((-2, 0, -2), (4, 0, 0), (0, 0, 4), (0, 1, 0))
            sd.add_mesh(pos, tri, bsdf=b, face_normals=True, name="floor", texcoords=QUAD_UV)
        else:
            sd.add_sphere((0, 0.5, 0), 0.5, bsdf=b)
        sd.directional_light((0.3, -0.8, -0.5), (2.0, 1.5, 1.0))
        sd.camera = dict(origin=(0.0, 1.2, 1.8), target=(0.0, 0.3, 0.0), up=(0.0, 1.0, 0.0), fov=39.3)
        return sd
    ps = _all_samples(32, 32, 4)
    k = (0.0625, 0.125, 0.03125)
    one = _prep(mts, scene_of([k, k]), integ=(1, 1))[0].li_samples(ps)
    two = _prep(mts, scene_of([k, [4 * x for x in k]]), integ=(1, 1))[0].li_samples(ps)
    lit = (one[:, :3] > 0).all(axis=1)
    assert lit.sum() > 500
    assert np.array_equal(bits(two[~lit]), bits(one[~lit]))
    same = (bits(two[lit, :3]) == bits(one[lit, :3])).all(axis=1)
    four = (bits(two[lit, :3]) == bits(one[lit, :3] * F(4))).all(axis=1)
    assert (same | four).all(), "a sample that is neither 1 nor 4 times the one-yarn sample: %s" % np.nonzero(~(same | four))[0][:4]
    assert same.mean() > 0.2 and four.mean() > 0.2, (same.mean(), four.mean())


# --- 5. one film across drivers ----------------------------------------------------------------------------------------
def _one_film_scene(mts, sky, weaves):
    """a specular cloth floor with vertex normals and tangents, a snow floor beside it, a twosided cloth wall, a Lambertian wall,
    a cloth sphere and a metal sphere"""
    S = mts.scenes
    sd = S.SceneDescription("cloth film")
    pos, tri = S._quad((-2, 0, -2), (2, 0, 0), (0, 0, 4), (0, 1, 0))
    sd.add_mesh(pos, tri, bsdf=sd.irawan(weaves[3][1], repeat_u=6.0, repeat_v=12.0), face_normals=False, name="cloth floor", texcoords=QUAD_UV)
    pos, tri = S._quad((0, 0, -2), (2, 0, 0), (0, 0, 4), (0, 1, 0))
    sd.add_mesh(pos, tri, bsdf=sd.wiscombe(), face_normals=True, name="snow floor")
    pos, tri = S._quad((-2, 0, -2), (4, 0, 0), (0, 2, 0), (0, 0, 1))
    sd.add_mesh(pos, tri, bsdf=sd.lambertian(0.6, 0.3, 0.3), face_normals=True, name="wall")
    pos, tri = S._quad((-2, 0, -2), (0, 0, 4), (0, 2, 0), (1, 0, 0))
    sd.add_mesh(pos, tri, bsdf=sd.twosided(sd.irawan(weaves[6][1], repeat_u=4.0, repeat_v=4.0)), face_normals=True, name="cloth wall", texcoords=QUAD_UV)
    sd.add_sphere((0.6, 0.3, 0.2), 0.3, bsdf=sd.roughmetal(0.2))
    sd.add_sphere((-0.7, 0.35, 0.6), 0.35, bsdf=sd.irawan(weaves[1][1], repeat_u=8.0, repeat_v=4.0))
    sd.point_light((0.5, 1.5, 1.0), 4.0)
    if sky:
        sd.sky(sun_direction=(0.3, 0.2, 0.8), turbidity=3.0, sky_scale=0.2)
    sd.camera = dict(origin=(0.0, 1.0, 1.8), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=39.3)
    sd.max_depth = 5
    return sd


@pytest.mark.parametrize("sky", [False, True])
def test_drivers_tile_parts_ragged_passes_group_and_direct_give_one_film(gpu_lib, mts, sky, weaves):
    sd = _one_film_scene(mts, sky, weaves)
    scene = mts.Scene(sd)
    assert scene.cloth is not None and scene.bsdf_snow is not None and scene.wants_tangents
    assert (scene.cloth[2] >= 0).sum() == 3

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
        assert entries[0] > 0 and entries[2] > 0 and sum(entries[1:2] + entries[3:10]) == 0, "the cloth hits land in bin 0: %s" % entries
        assert np.array_equal(bits(base), bits(render(integ, 0)[1])), (integ, "a repeat run differs")
        for drive in (1, 2, 3):
            assert np.array_equal(bits(base), bits(render(integ, drive)[1])), (integ, "drive %d differs from the device-driven frame" % drive)
        total = sum(render(integ, 0, part=part, n_parts=2)[1] for part in range(2))
        assert np.array_equal(bits(base), bits(total)), (integ, "two tile parts do not add up to the frame")
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
            it0.set_cloth_bsdfs()
            it0.clear_film()
            assert it0.render() and not np.array_equal(bits(it0.film()), bits(base)), "the cloth table matters in this frame"


# --- 6. the specular part inside a frame ---------------------------------------------------------------------------------
UV_REACH = 2e-6      # what its.uv of a hit may differ by from the binary64 uv of the same camera ray: the hit point of a 4-unit quad
                     # is good to a few 2^-24 of its extent, and the interpolation of three texcoords adds three roundings


@pytest.mark.parametrize("k", [0, 2, 5])
def test_a_specular_floor_is_intensity_times_f_times_cos_of_the_restatement(gpu_lib, mts, weaves, k):
    """a planar floor y = 0 without vertex normals under one directional light, `direct` with one luminaire sample, ks > 0, noise
    off.  Its frame is the reference's coordinateSystem((0, 1, 0)) = (s, t, n) = (+z, +x, +y) (trimesh.cpp:562-565), made of axis
    vectors, so wi and wo are components of the camera ray and of the light with no rounding, and its.uv is an affine map of the
    hit point.  Every radiance sample is held against I * f(uv, wi, wo) * cos with f from the binary64 restatement at the
    sample's own camera ray (mtsgpu_camera_rays).  Tolerance: the restatement's bound on f, plus what f moves by when uv moves by
    UV_REACH in either axis (the propagated error of uv; wi and wo carry none), times I cos, plus 6 roundings of the products
    around f.  Samples whose decisions are ambiguous, at uv or at a moved uv, are fragile: at most 1 %.  The same scene with the
    uv rotated by 90 degrees must differ: it tells warp from weft and u from v.

    The mesh with vertex normals and uploaded tangents is the next test."""
    S = mts.scenes
    name, W0 = weaves[k]
    W = W0.replace(repeatU=5.0, repeatV=7.0)
    assert W.ksMultiplier > 0 and not W.period > 0 and not W.fineness > 0
    I = np.float32([2.0, 1.5, 1.0])
    light = np.float32([-0.1, -0.8, 0.6])      # from behind the floor as the camera sees it: the half vector is near the normal

    def scene_of(rotated):
        sd = S.SceneDescription("specular cloth floor")
        pos, tri = S._quad((-2, 0, -2), (4, 0, 0), (0, 0, 4), (0, 1, 0))
        a, b = (pos[:, 0] + 2) / 4, (pos[:, 2] + 2) / 4
        uv = np.stack([b, 1 - a], axis=1) if rotated else np.stack([a, b], axis=1)
        sd.add_mesh(pos, tri, bsdf=sd.irawan(W), face_normals=True, name="floor", texcoords=uv.astype(np.float32))
        sd.directional_light(light, I)
        sd.camera = dict(origin=(0.3, 1.2, 1.8), target=(0.0, 0.0, 0.1), up=(0.0, 1.0, 0.0), fov=39.3)
        return sd
    ps = _all_samples(48, 48, 4)
    it, _ = _prep(mts, scene_of(False), res=48, integ=(1, 1))
    got = it.li_samples(ps)[:, :3].astype(np.float64)
    rays = it.camera_rays(ps.astype(np.int32)).astype(np.float64)
    o, d = rays[:, 0:3], rays[:, 4:7]
    t = -o[:, 1] / d[:, 1]
    hit = (d[:, 1] < 0) & (np.abs(o[:, 0] + t * d[:, 0]) < 1.999) & (np.abs(o[:, 2] + t * d[:, 2]) < 1.999)
    assert hit.sum() > 2000
    px, pz = o[:, 0] + t * d[:, 0], o[:, 2] + t * d[:, 2]
    uv = np.stack([(px + 2) / 4, (pz + 2) / 4], axis=1)[hit]
    wi = np.stack([-d[:, 2], -d[:, 0], -d[:, 1]], axis=1)[hit].astype(np.float32)      # (wi . s, wi . t, wi . n), s = +z, t = +x
    ld = (light / np.sqrt((light * light).sum(), dtype=np.float32)).astype(np.float32)
    wo = np.tile(np.float32([-ld[2], -ld[0], -ld[1]]), (hit.sum(), 1))
    assert np.array_equal(wi.astype(np.float64), np.stack([-d[:, 2], -d[:, 0], -d[:, 1]], axis=1)[hit]), "the ray's components are binary32 numbers"
    # the restatement takes binary32 inputs: uv rounded, and moved by the reach in either axis
    base, frag, live = R.f64(W, wi, wo, uv.astype(np.float32))
    assert live.all()
    moved = np.zeros_like(base.v)
    for du, dv in ((UV_REACH, 0), (-UV_REACH, 0), (0, UV_REACH), (0, -UV_REACH)):
        m, fr, _ = R.f64(W, wi, wo, (uv + [du, dv]).astype(np.float32))
        frag |= fr
        moved = np.maximum(moved, np.abs(m.v - base.v) + m.e)
    cos = float(wo[0, 2])
    want = I.astype(np.float64) * base.v * cos
    tol = I.astype(np.float64) * cos * (base.e + moved) + 6 * 2.0 ** -24 * np.abs(want)
    share = frag.mean()
    assert share <= 0.01, (name, "fragile share", share)
    err = np.abs(got[hit] - want)
    bad = ~frag & (err > tol).any(axis=1)
    print("%s: %d samples, %.2f %% fragile, worst error / tolerance %.3f" % (name, hit.sum(), 100 * share, (err / tol)[~frag].max()))
    assert not bad.any(), (name, int(bad.sum()), got[hit][bad][:2], want[bad][:2], tol[bad][:2], uv[bad][:2])
    diffuse = R.f64(W.replace(ksMultiplier=0.0), wi, wo, uv.astype(np.float32))[0].v
    specular = ~frag & ((base.v - diffuse) > 1e-3).any(axis=1)
    assert specular.sum() > 50, "the highlight is in the frame: %d samples" % specular.sum()
    miss = (d[:, 1] >= 0) | (np.abs(o[:, 0] + t * d[:, 0]) > 2.001) | (np.abs(o[:, 2] + t * d[:, 2]) > 2.001)
    assert not got[miss].any()
    # the uv rotated by 90 degrees is another picture
    rot = _prep(mts, scene_of(True), res=48, integ=(1, 1))[0].li_samples(ps)[:, :3]
    assert (np.abs(rot[hit] - got[hit]) > 1e-3).any(axis=1).mean() > 0.2


DIR_REACH = 4 * 2.0 ** -24     # what a component of its.wi or of the light's local direction may differ by from the binary64 dot product
                               # of the same binary32 frame and direction: three products and two sums of terms below 1, and one rounding
                               # where the test hands the restatement a binary32 number


@pytest.mark.parametrize("k", [0, 5])
def test_a_specular_cylinder_patch_with_uploaded_tangents_is_intensity_times_f_times_cos(gpu_lib, mts, weaves, k):
    """the quarter-cylinder patch of tests/tan_cases.py -- smooth normals, uv = (angle, height), so the mesh receives vertex tangents
    and k_shade_clo shades it in the frame of skdtree.h:392-399 -- under one directional light, `direct`, ks > 0.  Per sample:
    the camera ray (mtsgpu_camera_rays), its hit (mtsgpu_trace_rays: primitive and barycentrics), the device's binary32 frame at
    the hit (mtsgpu_shading_frame_eval, held to tests/ref64_tan.py by tests/test_gpu_tan.py) taken as exact, wi and wo as binary64
    projections on it, its.uv as the binary64 interpolation of the primitive's texcoords; then I * f * cos with f from the
    binary64 restatement.  Tolerance: the restatement's bound, plus what f moves by when uv moves by UV_REACH in either axis and
    a component of wi or wo by DIR_REACH (the propagated error of the three), times I cos, plus what the cosine's own reach
    adds and 6 roundings.  Fragile -- a decision ambiguous at the point or at a moved one -- at most 1 %.  The patch with its
    uv rotated by 90 degrees, whose tangents then run along the axis instead of around it, must differ"""
    S = mts.scenes
    name, W0 = weaves[k]
    W = W0.replace(repeatU=3.0, repeatV=2.0)
    assert W.ksMultiplier > 0 and not W.period > 0 and not W.fineness > 0
    I = np.float32([2.0, 1.5, 1.0])
    light = np.float32([0.2, -0.9, -0.3])
    pos, tri, nrm, tex = tan_cases.cylinder()

    def scene_of(rotated):
        sd = S.SceneDescription("specular cloth cylinder")
        uv = np.stack([tex[:, 1] + 1, 4 - tex[:, 0]], axis=1).astype(np.float32) if rotated else tex
        sd.add_mesh(pos, tri, bsdf=sd.irawan(W), face_normals=False, normals=nrm, name="patch", texcoords=uv)
        sd.directional_light(light, I)
        sd.camera = dict(origin=(0.4, 3.2, 0.6), target=(0.0, 0.8, 0.0), up=(0.0, 0.0, -1.0), fov=39.3)
        return sd
    ps = _all_samples(40, 40, 4)
    it, scene = _prep(mts, scene_of(False), res=40, integ=(1, 1))
    assert scene.wants_tangents and scene.vertex_tangents()[1][0] == 1
    got = it.li_samples(ps)[:, :3].astype(np.float64)
    rays = it.camera_rays(ps.astype(np.int32))
    hits = it.trace_rays(rays[:, :8])
    hit = hits[:, 3] != 0xFFFFFFFF
    assert hit.sum() > 2000 and not got[~hit].any()
    prim = hits[hit, 3]
    bu, bv = hits[hit, 1].view(np.float32).astype(np.float64), hits[hit, 2].view(np.float32).astype(np.float64)
    frame = it.shading_frame_eval(prim, np.stack([bu, bv, 0 * bu], axis=1)).astype(np.float64).reshape(-1, 3, 3)
    d = rays[hit, 4:7].astype(np.float64)
    ld = (light / np.sqrt((light * light).sum(), dtype=np.float32)).astype(np.float64)
    wi = -np.einsum("nij,nj->ni", frame, d)
    wo = -np.einsum("nij,j->ni", frame, ld)
    t3 = tex.astype(np.float64)[tri[prim]]
    uv = t3[:, 0] * (1 - bu - bv)[:, None] + t3[:, 1] * bu[:, None] + t3[:, 2] * bv[:, None]
    base, frag, live = R.f64(W, wi.astype(np.float32), wo.astype(np.float32), uv.astype(np.float32))
    moved = np.zeros_like(base.v)
    moves = [(np.array(m, dtype=np.float64), None, None) for m in ((UV_REACH, 0), (-UV_REACH, 0), (0, UV_REACH), (0, -UV_REACH))]
    for axis in range(3):
        for sign in (1, -1):
            e = np.zeros(3); e[axis] = sign * DIR_REACH
            moves += [(None, e, None), (None, None, e)]
    for du, dwi, dwo in moves:
        m, fr, lv = R.f64(W, (wi + (0 if dwi is None else dwi)).astype(np.float32), (wo + (0 if dwo is None else dwo)).astype(np.float32),
                          (uv + (0 if du is None else du)).astype(np.float32))
        frag |= fr | (lv != live)
        moved = np.maximum(moved, np.abs(m.v - base.v) + m.e)
    cos = np.abs(wo[:, 2:3])
    Id = I.astype(np.float64)
    want = Id * base.v * cos
    tol = Id * cos * (base.e + moved) + Id * np.abs(base.v) * DIR_REACH + 6 * 2.0 ** -24 * np.abs(want)
    lit = live & ~frag
    assert live.mean() > 0.8, "the patch faces the light and the camera"
    share = frag[live].mean()
    err = np.abs(got[hit] - want)
    print("%s: %d samples on the patch, %.2f %% fragile, worst error / tolerance %.3f" % (name, hit.sum(), 100 * share, (err[lit] / tol[lit]).max()))
    assert share <= 0.01, (name, "fragile share", share)
    bad = lit & (err > tol).any(axis=1)
    assert not bad.any(), (name, int(bad.sum()), got[hit][bad][:2], want[bad][:2], tol[bad][:2], uv[bad][:2], wi[bad][:2])
    assert not got[hit][~live & ~frag].any(), "a direction below the shading frame's surface: f is zero"
    diffuse = R.f64(W.replace(ksMultiplier=0.0), wi.astype(np.float32), wo.astype(np.float32), uv.astype(np.float32))[0].v
    specular = lit & ((base.v - diffuse) > 1e-3).any(axis=1)
    assert specular.sum() > 50, "the highlight is in the frame: %d samples" % specular.sum()
    rot = _prep(mts, scene_of(True), res=40, integ=(1, 1))[0].li_samples(ps)[:, :3]
    assert (np.abs(rot[hit] - got[hit]) > 1e-3).any(axis=1).mean() > 0.2
