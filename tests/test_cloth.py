"""The woven-cloth BRDF `irawan`, host side (no GPU): load_weave on the two weave files of tests/golden/ against hand-written
structs, and its errors; the seven-word form of Random's first three draws against a plain restatement of random.cpp; the
specifications the float32 mirror of tests/ref64_cloth.py uses in place of libm against numpy's; the Perlin noise's lattice
zeros; every mutation of the mirror reported on the shared inputs of tests/cloth_cases.py; SceneDescription.irawan(), the weave
table and the tangents a cloth mesh receives; the flattener's refusal; and the ABI: version 8, the pinned sizes, the new exports
declared, exported and documented.  The device side -- the library's own f against the mirror, the setter's refusals, the
kernels -- is tests/test_gpu_cloth.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cloth_cases as CC
import ref64_cloth as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["mtsgpu_set_cloth_bsdfs", "mtsgpu_group_set_cloth_bsdfs", "mtsgpu_flatten_tangents_flagged", "mtsgpu_bsdf_eval_cloth",
               "mtsgpu_cloth_check", "mtsgpu_devmath"]
PARAMS = dict(fineness=2.0, period=3.0, weft_ks=(0.6, 0.7, 0.8))


def _deg(x):
    return F(float(F(x)) * np.pi / 180)


def test_load_weave_reads_the_two_golden_files(mts):
    Y, W = mts.Yarn, mts.Weave
    got = mts.load_weave(CC.text("cloth_plain_2x2.weave"), PARAMS)
    want = W("plain 2x2", [1, 2, 2, 1],
             [Y("warp", 0.0, _deg(38), 0.5, 1, 1.5, 0.25, 0.25, (0.05, 0.2, 0.1), (0.9, 0.8, 0.7)),
              Y("weft", _deg(-30), _deg(24), 0.3, 1, 1.25, 0.75, 0.25, (0.2, 0.05, 0.1), (0.6, 0.7, 0.8))],
             tileWidth=2, tileHeight=2, alpha=0.01, beta=4.0, ss=0.25, hWidth=0.5, warpArea=8, weftArea=6, dWarpUmaxOverDWarp=_deg(10),
             dWarpUmaxOverDWeft=_deg(5), dWeftUmaxOverDWarp=_deg(4), dWeftUmaxOverDWeft=_deg(8), fineness=2.0, period=3.0)
    assert got == want
    assert (got.repeatU, got.repeatV, got.kdMultiplier, got.ksMultiplier) == (1, 1, 1, 1)
    assert got.yarns[0].type == mts.abi.YARN_WARP and got.yarns[1].type == mts.abi.YARN_WEFT
    assert got.yarns[1].psi == F(-30 * np.pi / 180), "degrees to radians in binary64, rounded once"
    got = mts.load_weave(CC.text("cloth_conics_3x2.weave"), dict(fineness=0, period=0))
    want = W("conics 3x2", [1, 2, 3, 3, 1, 2],
             [Y("warp", 0.0, _deg(50), 0.0, 1, 2, 0.1666667, 0.5, (0.1, 0.1, 0.3), 1.0),
              Y("weft", 0.0, _deg(45), -0.5, 1, 2, 0.5, 0.25, (0.3, 0.1, 0.1), (0.5, 0.6, 0.7)),
              Y("weft", _deg(20), _deg(45), -0.8, 1.5, 1.75, 0.8333333, 0.75, (0.1, 0.3, 0.1), (0.7, 0.6, 0.5))],
             tileWidth=3, tileHeight=2, alpha=0.02, beta=1.5, ss=0, hWidth=0.75, warpArea=5, weftArea=7, dWarpUmaxOverDWarp=_deg(6),
             dWarpUmaxOverDWeft=_deg(3), dWeftUmaxOverDWarp=_deg(2), dWeftUmaxOverDWeft=_deg(7))
    assert got == want
    # the parabola of the second yarn: rhat == 0 exactly in binary32
    y = got.yarns[1]
    assert F(1) + y.kappa * (F(1) + F(1) / R.tan32(y.umax)) == 0
    # replace() copies
    r = got.replace(repeatU=3.0, ksMultiplier=0.0)
    assert r.repeatU == 3 and r.ksMultiplier == 0 and got.repeatU == 1 and r.pattern == got.pattern and r != got


def test_load_weave_errors(mts):
    good = CC.text("cloth_plain_2x2.weave")
    with pytest.raises(ValueError, match=r"parameter \$period is not given"):
        mts.load_weave(good, dict(fineness=1.0, weft_ks=0.5))
    with pytest.raises(ValueError, match=r"parameter \$weft_ks is not given"):
        mts.load_weave(good, dict(fineness=1.0, period=1.0))
    for text, why in (("pattern { 1 }", "expected weave"), ("weave { colour = 3 }", "unknown weave parameter 'colour'"),
                      ("weave { yarn { twist = 3 } }", "unknown yarn parameter 'twist'"), ("weave { yarn { type = bias } }", "neither warp nor weft"),
                      ("weave { tileWidth = 2.5 }", "not an unsigned integer"), ("weave { pattern { 1, -2 } }", "not an unsigned integer"),
                      ("weave { alpha = x }", "expected a number"), ("weave { name = plain }", "quoted string"),
                      ("weave { yarn { kd = 0.5 } }", "a spectrum is"), ("weave { alpha = 1 ", "found the end"),
                      ("weave { alpha = 1 } weave { }", "text after the weave")):
        with pytest.raises(ValueError, match=why):
            mts.load_weave(text)
    # comments, a spectrum parameter given as a grey level, no trailing separators needed
    w = mts.load_weave('weave { /* a */ name = "n", yarn { kd = $c /* b */ } }', dict(c=0.25))
    assert w.name == "n" and list(w.yarns[0].kd) == [0.25, 0.25, 0.25] and w.tileWidth == 0


def test_the_seven_word_generator_equals_the_plain_restatement():
    rng = np.random.RandomState(11)
    seeds = [0, 1, 1 << 32, (1 << 64) - 1] + [int(a) << 32 | int(b) for a, b in rng.randint(0, 1 << 32, size=(100, 2), dtype=np.int64)]
    got = R.random_first_three(np.array(seeds, dtype=np.uint64))
    for i, seed in enumerate(seeds):
        assert [int(x) for x in got[:, i]] == R.random_plain(seed, 3), seed
    # the known answer of the generator's authors for init_genrand64(5489): its first output
    assert R.random_plain(5489, 1)[0] == 14514284786278117030
    # nextFloat lies in [0, 1) and uses the low 32 bits
    f = R.ulong_to_float(np.array([0, 0xFFFFFFFF, 0xFFFFFFFF00000000, 1 << 31], dtype=np.uint64))
    assert f[0] == 0 and f[1] == F(1) - F(2.0 ** -23) and f[2] == 0 and f[3] == 0.5


def test_the_specifications_in_place_of_libm_are_within_one_unit_of_numpy():
    x = np.float32(np.concatenate([np.linspace(-8, 8, 3201), [0.0, -0.0, 1e-5, -1e-5, 1e-10, 0.00012207031, 0.0001220704]]))
    for mine, ref in ((R.sinh32, np.sinh), (R.cosh32, np.cosh), (R.atan32, np.arctan), (R.sin32, np.sin), (R.cos32, np.cos), (R.exp32, np.exp)):
        want = ref(x.astype(np.float64))
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (np.abs(mine(x).astype(np.float64) - want) <= ulp).all(), ref.__name__
    assert R.sinh32(F(0)) == 0 and np.signbit(R.sinh32(F(-0.0))) and R.cosh32(F(0)) == 1
    pos = np.float32(np.concatenate([np.geomspace(1e-30, 1e30, 2001), [1.0, 2.0, 0.5]]))
    want = np.log(pos.astype(np.float64))
    assert (np.abs(R.log32(pos).astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    assert R.log32(F(0)) == -np.inf and np.isnan(R.log32(F(-1)))
    unit = np.float32(np.linspace(-1, 1, 2001))
    want = np.arccos(unit.astype(np.float64))
    assert (np.abs(R.acos32(unit).astype(np.float64) - want) <= np.spacing(want.astype(np.float32))).all()
    assert np.isnan(R.acos32(F(1.5))) and R.acos32(F(-1)) == F(np.pi)
    rng = np.random.RandomState(5)
    y, xx = np.float32(rng.randn(4000)), np.float32(rng.randn(4000))
    want = np.arctan2(y.astype(np.float64), xx.astype(np.float64))
    assert (np.abs(R.atan2_32(y, xx).astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    assert R.atan2_32(F(1), F(0)) == F(np.pi / 2) and R.atan2_32(F(-0.0), F(-1)) == F(-np.pi) and R.atan2_32(F(0), F(-1)) == F(np.pi)
    t = np.float32(np.linspace(-1.5, 1.5, 1001))
    want = np.tan(t.astype(np.float64))
    assert (np.abs(R.tan32(t).astype(np.float64) - want) <= np.spacing(np.abs(want).astype(np.float32))).all()
    assert R.tan32(F(np.pi / 4)) == 1, "the parabola of cloth_conics_3x2.weave rests on this"


def test_perlin_noise_vanishes_on_the_lattice_and_stays_in_range():
    k = np.float32(np.arange(-300, 300))
    assert not R.perlin32(k).any(), "gradient noise is zero at integer points"
    x = np.float32(np.linspace(-700.0, 700.0, 20001))
    v = R.perlin32(x)
    assert np.isfinite(v).all() and np.abs(v).max() <= 1 and np.abs(v).max() > 0.3
    exact = np.float32(np.arange(0, 200) * 0.25)
    assert np.array_equal(R.perlin32(exact), R.perlin32(exact + F(256.0))), "the permutation repeats every 256 cells"
    assert (R.perlin32(x, pbrt=True) != v).any(), "the PBRT gradient is another noise"


def test_every_mutation_of_the_mirror_is_reported(mts):
    """each of the twelve mutations changes f or the sample on some record of the shared inputs: the cases reach the line"""
    assert len(R.MUTATIONS) >= 10
    weaves = CC.weaves(mts)
    wi, wo, uv, s = (np.concatenate(p) for p in zip(CC.random_records(1, 1500), CC.outside_records(1, 400)))
    base = {}
    silent = set(R.MUTATIONS)
    for k, (name, W) in enumerate(weaves):
        keep = CC.usable(W, uv)
        a, b, c, d = wi[keep], wo[keep], uv[keep], s[keep]
        base = (R.eval32(W, False, 0, a, b, c), R.eval32(W, False, 2, a, d, c))
        assert np.isfinite(base[0][(a[:, 2] > 0) & (b[:, 2] > 0)]).mean() > 0.99, name
        for m in sorted(silent):
            got = (R.eval32(W, False, 0, a, b, c, m), R.eval32(W, False, 2, a, d, c, m))
            if any((~((g == w) | (np.isnan(g) & np.isnan(w)))).any() for g, w in zip(got, base)):
                silent.discard(m)
    assert not silent, "mutations no record reports: %s" % sorted(silent)


def test_the_mirror_on_hand_computed_records(mts):
    """ksMultiplier = 0: f is kd * kdMultiplier of the yarn the pattern names at its.uv, with v flipped and the tile repeated; the
    unsigned centre of a negative cell; pdf and the sampled type"""
    W = CC.weaves(mts)[4][1]          # plain 2x2, repeat (3, 2.5), diffuse only, kdMultiplier 0.75
    assert W.ksMultiplier == 0 and W.kdMultiplier == 0.75 and W.pattern == [1, 2, 2, 1]
    up = np.float32([[0, 0, 1]])
    kd = [np.float32(y.kd) * F(0.75) for y in W.yarns]
    # uv = (0.1, 0.9): xy = (0.1 * 3 * 2, 0.1 * 2.5 * 2) = (0.6, 0.5) -> cell (0, 0) -> yarn 1; uv = (0.2, 0.9): xy.x = 1.2 -> yarn 2
    for uv, yarn in (((0.1, 0.9), 0), ((0.2, 0.9), 1), ((0.2, 0.7), 0), ((0.1, 0.7), 1), ((0.1 + 1.0 / 3, 0.9), 0)):
        v, info = R.f32(W, up, up, [uv])
        assert info[0, 0] == yarn and np.array_equal(v[0], kd[yarn]), uv
    # u < 0: (int) xy.x = -2 -> modulo 0 -> yarn 1 of row 0, and the centre is ((unsigned) -2 / 2) * 2 + 0.25 * 2 = 2^32 - 2 + 0.5
    v, info = R.f32(W, up, up, [(-0.4, 0.9)])
    assert info[0, 0] == 0 and info[0, 1] == F(4294967294.0) + F(0.5)
    assert not R.f32(W, -up, up, [(0.1, 0.9)])[0].any() and not R.f32(W, up, -up, [(0.1, 0.9)])[0].any()
    out = R.eval32(W, True, 0, -up, -up, [(0.1, 0.9)])
    assert np.array_equal(out[0, :3], kd[0]), "the twosided adapter flips both"
    s = R.eval32(W, False, 2, up, [(0.25, 0.5)], [(0.1, 0.9)])
    assert s[0, 3] == s[0, 2] * R.INV_PI and s[0, 7].view(np.uint32) == 0x10 and np.array_equal(s[0, 4:7], kd[0])
    assert R.eval32(W, False, 1, up, [(0.6, 0.0, 0.8)], [(0.1, 0.9)])[0, 0] == F(0.8) * R.INV_PI


def test_scene_description_weaves_and_the_tangents_of_a_cloth_mesh(mts):
    S, A = mts.scenes, mts.abi
    weaves = CC.weaves(mts)
    sd = S.SceneDescription("cloth")
    lam = sd.lambertian(0.5)
    a = sd.irawan(weaves[0][1])
    b = sd.twosided(sd.irawan(weaves[5][1], repeat_u=4.0, ks_multiplier=0.5))
    c = sd.irawan(weaves[0][1])
    assert sd.bsdf_type == [A.BSDF_LAMBERTIAN, A.BSDF_LAMBERTIAN, A.BSDF_LAMBERTIAN | A.BSDF_TWOSIDED, A.BSDF_LAMBERTIAN]
    assert not sd.bsdf_params[a].any() and len(sd.weaves) == 2 and sd.weaves[1].repeatU == 4 and sd.weaves[1].ksMultiplier == 0.5
    assert list(sd.weave_table()) == [-1, 0, 1, 0]
    pos, tri = S._quad((-1, 0, -1), (2, 0, 0), (0, 0, 2), (0, 1, 0))
    uv = [(0, 0), (1, 0), (1, 1), (0, 1)]
    sd.add_mesh(pos, tri, bsdf=a, face_normals=False, name="smooth cloth", texcoords=uv)
    sd.add_mesh(pos + F(3), tri, bsdf=b, face_normals=True, name="flat cloth", texcoords=uv)
    sd.add_mesh(pos - F(3), tri, bsdf=lam, face_normals=False, name="lambertian", texcoords=uv)
    sd.add_sphere((0, 1, 0), 0.5, bsdf=c)
    sd.point_light((0, 3, 0), 1.0)
    scene = mts.Scene(sd)
    assert scene.cloth is not None and list(scene.cloth[2]) == [-1, 0, 1, 0] and scene.wants_tangents
    arr = scene.cloth[0]
    assert arr[0].tileWidth == 2 and arr[1].tileWidth == 3 and arr[1].n_pattern == 6 and arr[1].n_yarns == 3 and arr[1].repeatU == 4
    assert arr[1].yarns[2].kappa == F(-0.8) and [arr[0].pattern[i] for i in range(4)] == [1, 2, 2, 1]
    tan, has = scene.vertex_tangents()
    assert list(has[:4]) == [1, 0, 0, 0], "the mesh with vertex normals and a cloth BSDF receives tangents; a Lambertian's does not"
    assert mts.Scene(S.cornell_c1()).cloth is None
    # the flattener refuses a flagged mesh without texcoords like an anisotropic Ward's
    sd2 = S.SceneDescription("no uv")
    w = sd2.irawan(weaves[0][1])
    sd2.add_mesh(pos, tri, bsdf=w, face_normals=False, name="a")
    sd2.add_mesh(pos + F(3), tri, bsdf=sd2.lambertian(0.5), face_normals=False, name="b", texcoords=uv)
    sd2.point_light((0, 3, 0), 1.0)
    desc, keep = sd2.to_ctypes()
    tcs = (A.f32p * 2)()
    tcs[1] = A.ptr(sd2.meshes[1].texcoords, A.f32p)
    h = C.c_void_p()
    flags = np.uint32([1, 0])
    kp = A.KdParams()
    assert mts.lib().mtsgpu_flatten_tangents_flagged(C.byref(desc), C.byref(kp), tcs, A.ptr(flags, A.u32p), C.byref(h)) == -1
    assert "texture" in mts.lib().mtsgpu_last_error(None).decode()
    assert mts.lib().mtsgpu_flatten_tangents_flagged(C.byref(desc), C.byref(kp), tcs, None, C.byref(h)) == 0
    mts.lib().mtsgpu_flat_scene_free(h)


def test_abi_is_unchanged_and_the_exports_exist(mts):
    L, a = mts.lib(), mts.abi
    assert L.mtsgpu_abi_version() == a.ABI_VERSION == 8
    assert [L.mtsgpu_abi_sizeof(i) for i in range(6)] == [288, 172, 184, 72, 96, 48]
    assert a.BSDF_NTYPES == 10
    core = open(os.path.join(ROOT, "include", "mtsgpu.h")).read()
    header = open(os.path.join(ROOT, "include", "mtsgpu_cloth.h")).read()
    find = lambda text: set(re.findall(r"\b(mtsgpu_[a-z0-9_]+)\s*\(", text))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert find(header) - {"mtsgpu_set_snow_bsdfs"} == set(NEW_EXPORTS) == set(mts.CLOTH_EXPORTS) and not find(core) & set(NEW_EXPORTS)
    assert sorted(mts.EXPORTS) == sorted(find(core))
    for name in NEW_EXPORTS:
        assert hasattr(L, name), name
        assert name in doc, name
    assert '#include "mtsgpu.h"' in header and "mtsgpu_cloth.h" in core and "mtsgpu_cloth.h" in doc
    assert "#define MTSGPU_ABI_VERSION 8" in core
    assert C.sizeof(a.Yarn) == 56 and a.Yarn.kd.offset == 32 and a.Yarn.ks.offset == 44
    assert C.sizeof(a.Weave) == 96 and a.Weave.tileWidth.offset == 24 and a.Weave.n_pattern.offset == 72 and a.Weave.pattern.offset == 80 \
        and a.Weave.yarns.offset == 88
    assert (a.YARN_WARP, a.YARN_WEFT) == (0, 1)
    # a NULL context is refused before anything is read
    assert L.mtsgpu_set_cloth_bsdfs(None, 0, None, None) == -1 and L.mtsgpu_bsdf_eval_cloth(None, 0, None, 0, 0, None, None) == -1
    assert L.mtsgpu_group_set_cloth_bsdfs(None, 0, None, None) == -1


# --- the binary64 restatement ------------------------------------------------------------------------------------------
FRAGILE_CAP = 0.01


def _restated(W, two, op, wi, aux, uv, mutation=None):
    """(the mirror's value [n][3], the restatement E, fragile, live) of f (op 0) or of the sample's value (op 2)"""
    out = R.eval32(W, two, op, wi, aux, uv, mutation)
    got = out[:, :3] if op == 0 else out[:, 4:7]
    base = out if mutation is None else R.eval32(W, two, op, wi, aux, uv)      # the direction is the unmutated mirror's
    want, fragile, live = R.eval64(W, two, op, wi, aux, uv, wo32=base[:, :3])
    return got, want, fragile, live, None


def test_the_mirror_lies_inside_the_bound_of_the_binary64_restatement(mts):
    """every weave x the random set x f / sample x plain / twosided: at most 1 % of the live random records are fragile (the
    conic of a yarn whose rhat is a constant is taken in binary32, so the parabola yarn of cloth_conics_3x2.weave is compared like
    any other), and on every other record the mirror's error is below the restatement's bound.  Largest
    ratio found: 0.78 on these records, 0.90 on another seed of the random set (LABNOTES.md).  The named and the out-of-square records are compared where they are not fragile"""
    worst = (0.0, None)
    for k, (name, W) in enumerate(CC.weaves(mts)):
        wi, wo, uv, s = CC.random_records(200 + k)
        names, nwi, nwo, nuv, ns = CC.named_records(W)
        owi, owo, ouv, os_ = CC.outside_records(200 + k)
        if not (W.period > 0 or W.fineness > 0):
            _, twi, two_, tuv, ts = CC.threshold_records(W)
            nwi, nwo, nuv, ns = np.concatenate([nwi, twi]), np.concatenate([nwo, two_]), np.concatenate([nuv, tuv]), np.concatenate([ns, ts])
        keep = CC.usable(W, np.concatenate([nuv, ouv]))
        extra = [np.concatenate(p)[keep] for p in ((nwi, owi), (nwo, owo), (nuv, ouv), (ns, os_))]
        for two in (False, True):
            for op in (0, 2):
                got, want, fragile, live, on_rhat = _restated(W, two, op, wi, s if op == 2 else wo, uv)
                share = fragile.sum() / max(live.sum(), 1)
                assert live.sum() > 2000 and share <= FRAGILE_CAP, (name, two, op, "fragile share of the random set", share)
                r, at = R.ratio(got, want, fragile | ~live)
                assert r < 1, (name, two, op, "record %d" % at, r, got[at], want.v[at], want.e[at])
                if r > worst[0]:
                    worst = (r, (name, two, op))
                got, want, fragile, live, _ = _restated(W, two, op, extra[0], extra[3] if op == 2 else extra[1], extra[2])
                r, at = R.ratio(got, want, fragile | ~live)
                assert r < 1, (name, two, op, "named or outside record %d" % at, r)
                assert (live & ~fragile).sum() > 100, (name, "the named records that can be compared")
    print("largest error / bound: %.3f at %s" % worst)
    assert worst[0] > 0.05, "a bound nothing comes near says nothing"


def test_every_mutation_is_reported_by_the_restatement(mts):
    """each mutation of the mirror leaves the restatement's bound on some record that is not fragile"""
    silent = set(R.MUTATIONS)
    wi, wo, uv, s = (np.concatenate(p) for p in zip(CC.random_records(1, 1500), CC.outside_records(1, 400)))
    for name, W in CC.weaves(mts):
        keep = CC.usable(W, uv)
        a, b, c, d = wi[keep], wo[keep], uv[keep], s[keep]
        for m in sorted(silent):
            for op in (0, 2):
                got, want, fragile, live, _ = _restated(W, False, op, a, d if op == 2 else b, c, m)
                r, _ = R.ratio(got, want, fragile | ~live)
                if r > 1:
                    silent.discard(m)
                    break
    assert not silent, "mutations inside the bound everywhere: %s" % sorted(silent)


def test_the_mirror_uses_the_librarys_elementary_functions_bit_for_bit(mts):
    """csrc/devmath.h through the host build (mtsgpu_devmath) against the numpy restatements the mirror evaluates: sin, cos, tan,
    exp, log, atan, acos, atan2 and the two added for the cloth, sinh and cosh, with pow(x, 1.5)"""
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    rng = np.random.RandomState(9)
    x = np.float32(np.concatenate([np.linspace(-12, 12, 4801), rng.randn(2000) * 3, [0.0, -0.0, 1e-5, -1e-5, 1e-10, 0.00012207031, 0.0001220704,
                                                                                   -0.00012207031, 88.0, -100.0, 1e-30]]))
    for name, mine in (("sin", R.sin32), ("cos", R.cos32), ("tan", R.tan32), ("exp", R.exp32), ("atan", R.atan32), ("sinh", R.sinh32), ("cosh", R.cosh32)):
        got, want = mts.devmath(name, x), mine(x)
        assert ((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(), name
    pos = np.float32(np.concatenate([np.geomspace(1e-38, 1e38, 3001), [0.0, 1.0, 2.0, 0.5, -1.0, np.inf]]))
    for name, mine in (("log", R.log32), ("pow15", R.pow15_32)):
        got, want = mts.devmath(name, pos), mine(pos)
        assert ((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all(), name
    unit = np.float32(np.concatenate([np.linspace(-1, 1, 4001), [1.5, -1.5, np.nextafter(F(1), F(0)), np.nextafter(F(-1), F(0))]]))
    got, want = mts.devmath("acos", unit), R.acos32(unit)
    assert ((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))).all()
    y, xx = np.float32(rng.randn(5000)), np.float32(rng.randn(5000))
    y[:6], xx[:6] = [0, -0.0, 0, -0.0, 1, -1], [1, 1, -1, -1, 0, 0]
    assert np.array_equal(bits(mts.devmath("atan2", y, xx)), bits(R.atan2_32(y, xx)))


def test_weave_and_cast_refusals_without_a_device(mts):
    """checkWeave and the cast bound of the setter, through the context-free mtsgpu_cloth_check"""
    A = mts.abi
    W = CC.weaves(mts)[0][1]
    noisy = CC.weaves(mts)[1][1]
    scal = lambda w: {n: getattr(w, n) for n in A.WEAVE_SCALARS}
    mts.cloth_check(W); mts.cloth_check(W, (0, 1, 0, 1)); mts.cloth_check(noisy, (0, 1, 0, 1)); mts.cloth_check(W, (-3, 4, -2, 5))

    def refused(w, why, rng=None):
        with pytest.raises(mts.MtsGpuError, match=why):
            mts.cloth_check(w, rng)
    refused(mts.Weave("", W.pattern[:3], W.yarns, **scal(W)), r"pattern size 3 is not tileWidth \* tileHeight = 4")
    refused(W.replace(tileWidth=0), "zero tile dimension")
    refused(W.replace(tileHeight=0), "zero tile dimension")
    refused(W.replace(tileWidth=40000), "a tile dimension above 32768")
    refused(mts.Weave("", [1, 2, 3, 1], W.yarns, **scal(W)), r"pattern entry 2 = 3 is outside 1\.\.2")
    refused(mts.Weave("", [0, 2, 2, 1], W.yarns, **scal(W)), r"pattern entry 0 = 0 is outside 1\.\.2")
    refused(mts.Weave("", W.pattern, [], **scal(W)), "no pattern or no yarns")
    refused(mts.Weave("", W.pattern, [W.yarns[0], mts.Yarn(type=2, umax=0.5, width=1, length=1)], **scal(W)), "yarn 1: unknown type 2")
    for n in A.WEAVE_SCALARS:
        if n not in ("tileWidth", "tileHeight"):
            for bad in (np.nan, np.inf, -np.inf):
                refused(W.replace(**{n: bad}), "%s is not finite" % n)
    for field in ("psi", "umax", "kappa", "width", "length", "centerU", "centerV"):
        y = mts.Yarn(**{**dict(type="weft", umax=0.5, width=1, length=1), field: np.nan})
        refused(mts.Weave("", W.pattern, [W.yarns[0], y], **scal(W)), "yarn 1: a parameter is not finite")
    refused(mts.Weave("", W.pattern, [W.yarns[0], mts.Yarn(umax=0.5, width=1, length=1, kd=(0.1, np.inf, 0.1))], **scal(W)), "yarn 1: a parameter is not finite")
    for kw in (dict(width=0.0), dict(width=-1.0), dict(length=0.0), dict(umax=0.0), dict(umax=-0.1)):
        y = mts.Yarn(**{**dict(type="warp", umax=0.5, width=1, length=1), **kw})
        refused(mts.Weave("", W.pattern, [y, W.yarns[1]], **scal(W)), "yarn 0: width, length and umax must be positive")
    for kw in (dict(warpArea=0.0), dict(weftArea=-1.0)):
        refused(W.replace(**kw), "warpArea and weftArea must be positive")
    for kw in (dict(fineness=-1.0), dict(period=-0.5)):
        refused(W.replace(**kw), "fineness and period must not be negative")
    # the casts: (int) xy, the noise arguments, the fineness seed factors -- 2^31 - 2^16, from the extremes of the texcoords
    lim = 2147483648.0 - 65536.0
    mts.cloth_check(W, (0, lim / 2 * 0.999, 0, 1))
    refused(W, r"outside the range of the \(int\) cast", (0, lim / 2 * 1.001, 0, 1))
    refused(W, r"outside the range of the \(int\) cast", (0, 1, -lim / 2 * 1.001, 1))
    refused(W.replace(repeatU=1e10), r"outside the range of the \(int\) cast", (0, 1, 0, 1))
    refused(noisy, "a noise argument can leave the range of floorToInt", (-0.6, 1, 0, 1))      # a negative cell: the centre is 2^32
    refused(noisy, "a noise argument can leave the range of floorToInt", (0, 1, 0, 1.6))
    refused(W.replace(period=1e-9), "a noise argument can leave the range of floorToInt", (0, 1, 0, 1))
    refused(W.replace(period=1.0, repeatV=2e9), "tileHeight \\* repeatV leaves the range of the seed's cast", (0, 0.1, 1, 1))
    refused(W.replace(fineness=1e9), "a fineness seed factor can leave the range of its cast", (0, 1, 0, 1))
    refused(W.replace(fineness=1.0), "a fineness seed factor can leave the range of its cast", (-0.6, 1, 0, 1))
    mts.cloth_check(W.replace(fineness=1e9))         # without a range only the weave is checked
    assert mts.lib().mtsgpu_cloth_check(None, None) == -1


def test_the_threshold_records_sit_on_the_highlight_tests(mts):
    """cloth_cases.threshold_records: across every bracket the mirror's margin of the named test changes sign between two
    neighbouring binary32 directions, and for the conics weave every one of the five tests has a bracket across which the value
    of f changes, so `<` against `<=` there is seen by whoever is compared with the mirror.  Perlin's permutation, the one table
    the tests transcribe, is spot-checked against noise.cpp:10-13 by hand"""
    name, W = CC.weaves(mts)[5]
    names, wi, wo, uv, s = CC.threshold_records(W)
    assert len(names) == 6 * 3 * 5
    value = R.f32(W, wi, wo, uv)[0]
    margins, _ = CC._margins(W, wi, wo, uv)
    decides = {}
    for i in range(0, len(names), 6):
        test = names[i].split(" | ")[0]
        before, after = margins[test][i], margins[test][i + 3]
        assert (before < 0) != (after < 0), (names[i], before, after)      # the test holds on one side only; a margin of exactly 0 occurs
        assert np.abs(wo[i] - wo[i + 3]).max() <= 2 * np.spacing(np.abs(wo[i]).max()), (names[i], "the two ends are neighbours")
        decides[test] = decides.get(test, 0) + (not np.array_equal(value[i], value[i + 3]))
    assert set(decides) == set(CC.THRESHOLDS) and min(decides.values()) >= 1, decides
    assert list(R.PERM[:8]) == [151, 160, 137, 91, 90, 15, 131, 13] and list(R.PERM[16:21]) == [140, 36, 103, 30, 69]
    assert R.PERM[255] == 180 and sorted(R.PERM) == list(range(256)), "a permutation of 0 .. 255 that ends as noise.cpp:40 does"
