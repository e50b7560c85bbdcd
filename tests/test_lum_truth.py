"""The non-delta luminaires and the selection among a scene's luminaires against the binary64 restatement
(tests/ref64_lum.py), on the CPU: the oracle's read-out (orc_scene_lum_eval) through the check the device's read-out goes
through (tests/lum_cases.py, tests/test_gpu_lum_truth.py), the host's binary32 tables against their binary64 recomputation
for the product's flattener and the oracle's, the ambiguity cap with no evaluator in the loop, and the check's own sight."""
import numpy as np
import pytest

import closed_forms as cf
import lum_cases
import ref64_lum as R

F = np.float32
N_SCENES = 9


@pytest.fixture(scope="module")
def scenes(mts):
    s = lum_cases.scenes(mts)
    assert len(s) == N_SCENES
    return s


@pytest.fixture(scope="module")
def flat(scenes, orc):
    """the oracle's flat scenes, kept alive for the module"""
    return [orc.FlatScene(sd) for _, sd in scenes]


# --- 1. the oracle's read-out ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(N_SCENES))
def test_oracle_luminaires_against_binary64(scenes, flat, orc, k):
    name = scenes[k][0]
    failures, report = lum_cases.check_scene(lambda op, q: orc.scene_lum_eval(flat[k].scene, op, q), flat[k].arrays(), 100 + k)
    print("%s\n%s" % (name, lum_cases.format_report(report)))
    assert not failures, name + "\n" + "\n".join(failures)
    # the margin the comment in lum_cases.py records
    for cls, (v, d, _, _) in report.items():
        assert v <= lum_cases.WORST_ORACLE[0] and d <= lum_cases.WORST_ORACLE[1], (name, cls, v, d)


def test_oracle_hook_refusals(scenes, flat, orc):
    q = np.zeros((1, 16), dtype=np.float32)
    q[0, 9:12] = (0, 1, 0)
    by_name = {n: f for (n, _), f in zip(scenes, flat)}
    five = by_name["five: quad, spot, sphere, point, envmap"]
    for lum in (1, 3, 5, -1, 0.5, np.nan):          # the spot, the point light, one past the end, and no index at all
        q[0, 12] = lum
        with pytest.raises(ValueError):
            orc.scene_lum_eval(five.scene, 1, q)
    q[0, 12] = 4
    assert orc.scene_lum_eval(five.scene, 1, q)[0, 0] > 0
    with pytest.raises(ValueError):
        orc.scene_lum_eval(by_name["quad"].scene, 2, q)       # no background luminaire
    with pytest.raises(ValueError):
        orc.scene_lum_eval(five.scene, 3, q)


# --- 2. the tables that are arithmetic on the description ------------------------------------------------------------
def _check_tables(A, who):
    T = R.tables(A)
    nl = len(A["lum_type"])
    def close(got, ref, what):
        got = np.asarray(got, dtype=np.float64)
        tol = cf.K_VALUE * cf.EPS * np.broadcast_to(ref.e, got.shape) + cf.ATOL
        bad = ~(np.abs(got - ref.v) <= tol)
        assert not bad.any(), "%s %s: %s != %s (bound %s)" % (who, what, got[bad][:3], np.broadcast_to(ref.v, got.shape)[bad][:3], tol[bad][:3])
    close(A["lum_sel_cdf"], T.sel_cdf, "lum_sel_cdf")
    close(A["lum_sel_pdf"], T.sel_pdf, "lum_sel_pdf")
    close(A["lum_sel_sum"], T.sel_sum, "lum_sel_sum")
    assert A["lum_sel_cdf"][0] == 0 and A["lum_sel_cdf"][-1] == 1
    for l in range(nl):
        if A["lum_type"][l] != R.AREA:
            continue
        close(A["lum_inv_area"][l], T.inv_area[l], "lum_inv_area[%d]" % l)
        s = int(A["lum_shape"][l])
        if A["shape_type"][s] == 1:
            close(A["shape_params"][s][23], T.inv_area[l], "shape_params[%d][23]" % s)
            assert A["lum_cdf_offset"][l + 1] == A["lum_cdf_offset"][l]
        else:
            o0, o1 = int(A["lum_cdf_offset"][l]), int(A["lum_cdf_offset"][l + 1])
            assert o1 - o0 == len(T.tri_cdf[l].v)
            cdf = A["lum_tri_cdf"][o0:o1]
            close(cdf, T.tri_cdf[l], "lum_tri_cdf of luminaire %d" % l)
            assert cdf[0] == 0 and cdf[-1] == 1 and (np.diff(cdf) >= 0).all()
    if A["env_size"][2]:
        # without restating the MIP pyramid: a density, summing to 1 within binary32 summation error, and its running sum
        pdf, cdf = A["env_pdf"].astype(np.float64), A["env_cdf"].astype(np.float64)
        n = len(pdf)
        assert (pdf >= 0).all() and (pdf == 0).any(), "the bitmap's black block should leave cells of zero density"
        assert abs(pdf.sum() - 1) <= n * cf.EPS
        assert cdf[0] == 0 and cdf[-1] == 1 and len(cdf) == n + 1
        run = np.concatenate([[0.0], np.cumsum(pdf)])
        assert (np.abs(cdf - run) <= n * cf.EPS).all()
        assert (np.diff(A["env_cdf"]) >= 0).all()


@pytest.mark.parametrize("k", range(N_SCENES))
def test_host_tables_against_binary64(scenes, flat, mts, k):
    name, sd = scenes[k]
    A_orc, A_mts = flat[k].arrays(), mts.Scene(sd).arrays()
    _check_tables(A_orc, "oracle, " + name)
    _check_tables(A_mts, "flattener, " + name)
    # and the two flatteners agree on every table the luminaires read, bit for bit
    for key in ("lum_sel_cdf", "lum_sel_pdf", "lum_inv_area", "lum_tri_cdf", "lum_params", "env_pdf", "env_cdf", "env_pixels", "shape_params"):
        assert np.array_equal(np.asarray(A_orc[key]).view(np.uint32), np.asarray(A_mts[key]).view(np.uint32)), (name, key)


# --- 3. the ambiguity cap: a condition on the inputs, no evaluator in the loop ---------------------------------------
@pytest.mark.parametrize("k", range(N_SCENES))
def test_inputs_stay_under_the_ambiguity_cap(scenes, flat, k):
    name = scenes[k][0]
    A = flat[k].arrays()
    T = R.tables(A)
    rng = np.random.RandomState(100 + k)                 # the generator check_scene uses, in its order
    I = lum_cases.sample_inputs(A, rng)
    ref = R.sample_luminaire(T, *I.cols)
    thresholds = 0
    for cls, idx in I.classes.items():
        if cls.endswith(lum_cases.THRESHOLD_MARK):
            thresholds += 1
            continue
        aside = (ref.amb | ref.knot)[idx]
        assert aside.sum() <= cf.MAX_AMBIGUOUS * len(idx), (name, cls, int(aside.sum()), len(idx))
    assert thresholds >= 1
    for l, J in lum_cases.pdf_inputs(A, rng).items():
        val, cond, knot, amb = R.pdf_luminaire(T, J.cols[0], l, *J.cols[1:])
        for cls, idx in J.classes.items():
            if not cls.endswith(lum_cases.THRESHOLD_MARK):
                assert (knot | amb)[idx].sum() <= cf.MAX_AMBIGUOUS * len(idx), (name, l, cls)
        assert np.isfinite(val[~(knot | amb)]).all()
    J = lum_cases.le_inputs(A, rng)
    if J is not None:
        val, cond, amb = R.background_le(T, J.cols[0])
        assert not amb.any() and np.isfinite(val).all() and (val >= 0).all()


def test_restatement_flags_its_branches(scenes, flat):
    """what ref64_lum flags, on inputs built to sit on each threshold"""
    by_name = {n: f.arrays() for (n, _), f in zip(scenes, flat)}
    # a sample on a selection knot
    A = by_name["two: sphere and point"]; T = R.tables(A)
    r = R.sample_luminaire(T, F([[0, 4, 0]] * 2), F([[0.5, 0.3], [0.25, 0.3]]))
    assert r.knot[0] and not r.knot[1]
    lo, hi = (R.sample_luminaire(T, F([[0, 4, 0]]), F([[0.5, 0.3]]), tie=t) for t in (-1, 1))
    assert lo.lum[0] == 0 and hi.lum[0] == 1
    # the 1 - Epsilon switch, the inside of the sphere, the plane of a triangle
    A = by_name["sphere"]; T = R.tables(A)
    c, rad = A["shape_params"][1][0:3].astype(np.float64), 0.5
    p = F([c + [rad / (1 - R.EPSILON), 0, 0], c + [rad / 0.9, 0, 0], c + [0.1, 0, 0], c])
    r = R.sample_luminaire(T, p, F([[0.3, 0.6]] * 4))
    assert r.knot.tolist() == [True, False, False, False] and r.found.tolist() == [False, True, False, False]
    assert r.detail["inside"].tolist()[1:] == [0, 1, 1]
    A = by_name["quad"]; T = R.tables(A)
    r = R.sample_luminaire(T, F([[0.9, 2.0, 0.1], [0.0, 1.0, 0.0], [0.0, 3.0, 0.0]]), F([[0.3, 0.6]] * 3))
    assert r.amb.tolist() == [True, False, False] and r.found.tolist()[1:] == [True, False]
    # the boundary of the bounding sphere; a zero-density cell is never chosen
    A = by_name["envmap"]; T = R.tables(A)
    LP = A["lum_params"][0]
    on = F(LP[3:6].astype(np.float64) + np.array([0, 0, 1.0]) * float(LP[6]))
    r = R.sample_luminaire(T, np.stack([on, F(LP[3:6])]), F([[0.3, 0.6]] * 2))
    assert r.knot.tolist() == [True, False]
    rng = np.random.RandomState(3)
    r = R.sample_luminaire(T, np.tile(F(LP[3:6]), (4000, 1)), F(rng.random_sample((4000, 2))))
    assert (A["env_pdf"][r.detail["cell"]] > 0).all() and r.found.all()


# --- 4. the check sees a planted error -------------------------------------------------------------------------------
def _ulps(x, k):
    return (x.view(np.int32) + np.int32(k)).view(np.float32)


@pytest.mark.parametrize("name", ["quad", "sphere", "envmap"])
def test_the_check_sees_a_planted_error(scenes, flat, orc, name):
    """self-test: good read-outs pass; one output off by a few hundred to a few thousand ulp (see below) fails, so does n swapped
    for -n, a NaN, a wrong luminaire index and a lost sample -- each planted in ONE decidable record"""
    k = [n for n, _ in scenes].index(name)
    A = flat[k].arrays()
    T = R.tables(A)
    I = lum_cases.sample_inputs(A, np.random.RandomState(100 + k))
    q = np.zeros((I.n, 16), dtype=np.float32)
    q[:, 0:3], q[:, 3:5] = I.cols
    got = orc.scene_lum_eval(flat[k].scene, 0, q)
    assert not lum_cases.check_sample(T, I, got)[0]
    ref = R.sample_luminaire(T, *I.cols)
    plain = np.concatenate([idx for cls, idx in I.classes.items() if not cls.endswith(lum_cases.THRESHOLD_MARK)])
    ok = np.zeros(I.n, dtype=bool); ok[plain] = True
    ok &= ref.found & ~ref.amb & ~ref.knot & (got[:, 0] != 0) & np.isfinite(got).all(axis=1)
    cands = np.nonzero(ok)[0]
    assert len(cands) > 100
    # the planting runs on these records alone, as one class of their own
    keep = np.random.RandomState(4).choice(cands, 300, replace=False)
    J = lum_cases.Inputs(); J.add("planted", I.cols[0][keep], I.cols[1][keep])
    I, got, ref, cands = J, got[keep], R.sample_luminaire(T, *J.cols), np.arange(300)
    assert not lum_cases.check_sample(T, I, got)[0]
    # The reach of the check on one output is K x its derived bound: K_DIR = 64 times a bound of at least a few units for a
    # component of p, n or d, K_VALUE = 16 times the bound of the whole chain for a pdf and the value divided by it (cond 12
    # .. 30 at best: the area sum alone contributes half a unit per triangle).  The bounds are worst-case sums over every
    # rounding of the chain (the oracle's worst ratio is 1, not 16 or 64), so the reach is wider than a few hundred ulp: the
    # error is planted in the ten best-conditioned outputs of each group, at 300 ulp where that exceeds the reach and at
    # one and a half times the reach otherwise -- never more than 8000 ulp, i.e. 1e-3 of the value or of a unit vector's length (reached by lRec.d on the sphere alone,
    # whose bound carries the whole cone-and-intersection chain; the others stay below 3000).
    err = np.zeros((I.n, 16)); err[:, 2:5], err[:, 5:8], err[:, 8:11], err[:, 11], err[:, 12:15] = ref.p_err, ref.n_err, ref.d_err, ref.pdf_err, ref.value_err
    K = np.zeros(16); K[2:11], K[11:15] = cf.K_DIR, cf.K_VALUE
    rng = np.random.RandomState(9)
    with np.errstate(invalid="ignore", divide="ignore"):
        reach = K * err / np.abs(got.astype(np.float64)) * 2         # in ulp of the output: 2^-23 x bound / (|x| 2^-24)
    reach = np.where(np.isfinite(reach) & (got != 0), reach, np.inf)
    for cols, what in (((11,), "value ratio"), ((12, 13, 14), "value ratio"), ((2, 3, 4), "vector ratio"), ((5, 6, 7), "vector ratio"), ((8, 9, 10), "vector ratio")):
        pairs = sorted((reach[i, c], i, c) for c in cols for i in cands)[:10]
        for j in range(len(pairs)):
            r, i, c = pairs[j]
            ulps = max(300, int(1.5 * r) + 1)
            assert r < ulps <= 8000, (name, cols, r)
            for sign in (-1, 1):
                bad = got.copy(); bad[i, c] = _ulps(bad[i:i + 1, c], sign * ulps)[0]
                f = lum_cases.check_sample(T, I, bad)[0]
                assert any(what in x for x in f), (name, i, c, sign * ulps, got[i].tolist())
    for i in rng.choice(cands, 8, replace=False):
        bad = got.copy(); bad[i, 5:8] = -bad[i, 5:8]
        assert any("vector ratio" in x for x in lum_cases.check_sample(T, I, bad)[0]), (name, i, "n -> -n")
        bad = got.copy(); bad[i, 4] = np.nan
        assert any("non-finite" in x for x in lum_cases.check_sample(T, I, bad)[0])
        bad = got.copy(); bad[i, 0] = 0
        assert any("differ in found" in x for x in lum_cases.check_sample(T, I, bad)[0])
        bad = got.copy(); bad[i, 1] += 1
        assert any("differ in found" in x for x in lum_cases.check_sample(T, I, bad)[0])
    # and the pdf and Le checks
    for l, J in lum_cases.pdf_inputs(A, np.random.RandomState(1)).items():
        q = np.zeros((J.n, 16), dtype=np.float32)
        q[:, 0:3], q[:, 3:6], q[:, 6:9], q[:, 9:12] = J.cols
        q[:, 12] = l
        g = orc.scene_lum_eval(flat[k].scene, 1, q)[:, 0]
        assert not lum_cases.check_pdf(T, l, J, g)[0]
        val, cond, knot, amb = R.pdf_luminaire(T, J.cols[0], l, *J.cols[1:])
        first = J.classes[next(iter(J.classes))]
        sel = first[(val[first] > 0) & ~(knot | amb)[first]]
        i = int(sel[np.argmin(cond[sel])])
        for ulps in (-1, 1):
            bad = g.copy(); bad[i] = _ulps(bad[i:i + 1], ulps * max(300, int(4 * cf.K_VALUE * cond[i])))[0]
            assert any("worst ratio" in x for x in lum_cases.check_pdf(T, l, J, bad)[0])
    J = lum_cases.le_inputs(A, np.random.RandomState(2))
    if J is not None:
        q = np.zeros((J.n, 16), dtype=np.float32); q[:, 0:3] = J.cols[0]
        g = orc.scene_lum_eval(flat[k].scene, 2, q)[:, 0:3]
        assert not lum_cases.check_le(T, J, g)[0]
        val, cond, amb = R.background_le(T, J.cols[0])
        i = int(np.argmin(np.where((val > 0).all(axis=1), cond.max(axis=1), np.inf)))
        bad = g.copy(); bad[i, 1] = _ulps(bad[i:i + 1, 1], max(300, int(4 * cf.K_VALUE * cond[i, 1])))[0]
        assert any("worst ratio" in x for x in lum_cases.check_le(T, J, bad)[0])
        bad = g.copy(); bad[i, 2] = np.nan
        assert any("non-finite" in x for x in lum_cases.check_le(T, J, bad)[0])


# --- 5. ABI ----------------------------------------------------------------------------------------------------------
def test_abi_surface(mts):
    L, a = mts.lib(), mts.abi
    assert L.mtsgpu_abi_version() == a.ABI_VERSION == 8             # a new entry point, no structure changed
    assert "mtsgpu_scene_lum_eval" in mts.EXPORTS and hasattr(L, "mtsgpu_scene_lum_eval")
    root = mts.__file__.replace("mitsuba-renderer_amd/__init__.py", "")
    header = open(root + "include/mtsgpu.h").read()
    assert "int  mtsgpu_scene_lum_eval(mtsgpu_ctx *ctx, int op, uint32_t n, const float *queries, float *out);" in header
    assert "mtsgpu_scene_lum_eval" in open(root + "INTEGRATION.md").read()
