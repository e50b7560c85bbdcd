"""The sky luminaire without a GPU: mtsgpu_sky_configure against the binary64 restatement (tests/ref64_sky.py), the Python
mirror of the constructor (scenes.py), what the flattener derives and refuses, the ABI surface, and the condition that the
device comparison (tests/test_gpu_sky.py) leaves out no more than closed_forms.MAX_AMBIGUOUS of its records."""
import ctypes as C

import numpy as np
import pytest

import closed_forms as cf
import ref64_sky
import sky_cases

F = np.float32


def _sky_scene(mts, lums=None, **kw):
    sd = mts.scenes.SceneDescription("sky host")
    pos, tri = mts.scenes._quad((-4, 0, -4), (8, 0, 0), (0, 0, 8), (0, 1, 0))
    sd.add_mesh(pos, tri, bsdf=sd.lambertian(0.5), face_normals=True)
    sd.camera = dict(origin=(0.0, 30.0, 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), fov=40.0)     # far outside the scene's sphere
    l = sd.sky(**kw) if lums is None else lums(sd)
    return sd, l


# --- configure() -----------------------------------------------------------------------------------------------------
def test_host_configure_against_the_restatement(mts):
    """every derived quantity within 16 * 2^-23 * cond of the binary64 restatement (closed_forms.K_VALUE); sin / cos of thetaS
    ([21], [22]) against numpy's"""
    worst = (0.0, None)
    for name, P in sky_cases.parameter_sets(mts):
        got = mts.sky_configure(P).astype(np.float64)
        val, cond = ref64_sky.configure(P)
        assert np.isfinite(got).all(), name
        ratio = np.abs(got[:21] - val) / (cf.EPS * cond * np.abs(val))
        k = int(np.argmax(ratio))
        if ratio[k] > worst[0]:
            worst = (float(ratio[k]), "%s, entry %d: got %.9g ref %.9g cond %.3g" % (name, k, got[k], val[k], cond[k]))
        assert (ratio <= cf.K_VALUE).all(), (name, k, got[k], val[k], cond[k], ratio[k])
        th = float(P[16])
        assert abs(got[21] - np.sin(th)) <= 2 * cf.EPS and abs(got[22] - np.cos(th)) <= 2 * cf.EPS
    print("worst ratio of mtsgpu_sky_configure over the case list: %.3g of %g allowed (%s)" % (worst[0], cf.K_VALUE, worst[1]))


def test_configure_null_arguments(mts):
    out = np.zeros(mts.abi.SKY_NDERIVED, dtype=np.float32)
    assert mts.lib().mtsgpu_sky_configure(None, mts.abi.ptr(out, mts.abi.f32p)) == -1


# --- the constructor's mirror (sky.cpp:47-103) -----------------------------------------------------------------------
def test_defaults_follow_the_constructor(mts):
    sd = mts.scenes.SceneDescription("d")
    l = sd.sky()
    P = sd.lum_params[l]
    assert sd.lum_type[l] == mts.abi.LUM_SKY == 7
    assert P[0] == 1 and P[1] == 2 and P[2] == 1 and (P[18:23] == 1).all() and not P[3:7].any() and not P[23:].any()
    # rotate(x, -90 deg) * identity maps the luminaire's up (+z) to the world's +y: world->luminaire sends +y to +z
    M = P[7:16].reshape(3, 3).astype(np.float64)
    assert np.allclose(M @ [0, 1, 0], [0, 0, 1], atol=1e-7) and np.allclose(M @ [1, 0, 0], [1, 0, 0], atol=1e-7)
    assert np.allclose(M @ M.T, np.eye(3), atol=1e-6)
    # the default sun: latitude 51.050891, longitude 13.694458, meridian 0, day 200, 22:00 (:90-94)
    th, ph = ref64_sky.sun_from_location(51.050891, 13.694458, 0, 200, 22.0)
    assert abs(P[16] - th) < 1e-5 and abs(P[17] - ph) < 1e-5
    assert P[16] > np.pi / 2                        # at 22:00 the sun is below the horizon


def test_sun_placement_is_either_or(mts):
    sd = mts.scenes.SceneDescription("e")
    with pytest.raises(ValueError, match="decide for either"):
        sd.sky(sun_direction=(0, 0, 1), latitude=10.0)
    with pytest.raises(ValueError, match="At least one is missing"):
        sd.sky(latitude=10.0, longitude=20.0)
    assert not sd.lum_type


def test_julian_day_and_meridian_are_truncated(mts):
    """configureSunPosition takes them as int (sky.cpp:186-187)"""
    kw = dict(latitude=35.0, longitude=-100.0, time_of_day=10.25)
    a = mts.scenes.SceneDescription("a"); la = a.sky(julian_day=200.7, standard_meridian=-105.9, **kw)
    b = mts.scenes.SceneDescription("b"); lb = b.sky(julian_day=200, standard_meridian=-105, **kw)
    c = mts.scenes.SceneDescription("c"); lc = c.sky(julian_day=201, standard_meridian=-105, **kw)
    assert np.array_equal(a.lum_params[la].view(np.uint32), b.lum_params[lb].view(np.uint32))
    assert not np.array_equal(a.lum_params[la], c.lum_params[lc])


@pytest.mark.parametrize("kw", [
    dict(sun_direction=(0.3, 0.2, 0.8)), dict(sun_direction=(-2.0, -1.0, 0.1)), dict(sun_direction=(0.0, -1.0, -0.5)),
    dict(latitude=35.0, longitude=-100.0, standard_meridian=-105.0, julian_day=172.0, time_of_day=12.5),
    dict(latitude=-33.9, longitude=151.2, standard_meridian=150.0, julian_day=355.0, time_of_day=7.0),
    dict(latitude=48.1, longitude=11.6, standard_meridian=15.0, julian_day=20.0, time_of_day=9.75),
])
def test_sun_angles_against_the_restatement(mts, kw):
    """thetaS, phiS of the mirror (binary32 stores, sky.cpp:186-219) against binary64.  The angles come out of asin / atan2 /
    acos of quantities that carry a few roundings of binary32 inputs of order 10 (hours, degrees): allowed are 64 * 2^-23
    absolute, plus 2^-23 relative to the 2 pi added to a negative azimuth"""
    sd = mts.scenes.SceneDescription("s")
    P = sd.lum_params[sd.sky(**kw)]
    if "sun_direction" in kw:
        th, ph = ref64_sky.sun_from_direction(kw["sun_direction"])
    else:
        th, ph = ref64_sky.sun_from_location(kw["latitude"], kw["longitude"], kw["standard_meridian"], kw["julian_day"], kw["time_of_day"])
    tol = 64 * cf.EPS
    assert abs(float(P[16]) - th) <= tol and abs(float(P[17]) - ph) <= tol + cf.EPS * 2 * np.pi, (P[16], th, P[17], ph)
    assert 0 <= P[16] <= np.pi


# --- flattening ------------------------------------------------------------------------------------------------------
def test_flattener_derives_the_bounding_sphere(mts):
    """block [3..6]: the scene's bounding sphere x 1.01 with NO camera expansion (sky.cpp:221-227); a constant luminaire in the
    same scene's place grows its sphere to hold the camera (constant.cpp:49-63)"""
    sd, l = _sky_scene(mts, sun_direction=(0.2, 0.1, 0.9), turbidity=3.0)
    flat = mts.Scene(sd).arrays()
    assert flat["background_lum"] == l and int(flat["lum_type"][l]) == 7
    P = flat["lum_params"][l]
    bmin, bmax = flat["aabb_min"], flat["aabb_max"]
    centre = (bmax + bmin) * F(0.5)
    d = centre - bmax
    radius = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2], dtype=np.float32) * F(1.01)
    assert np.array_equal(P[3:6].view(np.uint32), centre.view(np.uint32)) and P[6] == radius
    assert P[6] < 10.0                                         # the camera sits 30 units away and is not inside
    keep = np.r_[0:3, 7:32]
    assert np.array_equal(P[keep].view(np.uint32), sd.lum_params[l][keep].view(np.uint32))
    sd2, l2 = _sky_scene(mts, lums=lambda sd: sd.add_lum(mts.abi.LUM_CONSTANT, [1, 1, 1]))
    assert mts.Scene(sd2).arrays()["lum_params"][l2][6] > 25.0


def _bad(sd, index, value):
    l = sd.sky(sun_direction=(0.2, 0.1, 0.9))
    sd.lum_params[l][index] = value
    return l


@pytest.mark.parametrize("lums, words", [
    (lambda sd: (sd.sky(), sd.sky()), ["more than one background luminaire"]),
    (lambda sd: (sd.sky(), sd.add_lum(1, [1, 1, 1])), ["the sky must be the background luminaire"]),
    (lambda sd: (sd.add_lum(1, [1, 1, 1]), sd.sky()), ["more than one background luminaire"]),
    (lambda sd: _bad(sd, 1, np.nan), ["non-finite sky parameter"]),
    (lambda sd: _bad(sd, 0, np.inf), ["non-finite sky parameter"]),
    (lambda sd: _bad(sd, 9, np.nan), ["non-finite sky parameter"]),
    (lambda sd: _bad(sd, 20, -np.inf), ["non-finite sky parameter"]),
    # turbidity 1e20 overflows the zenith polynomials' turbidity^2 in binary32
    (lambda sd: _bad(sd, 1, 1e20), ["non-finite"]),
    # cConst = eConst = 0 and aConst = 0 leave 1 * 1 everywhere; aConst chosen so that 1 + A exp(B) = 0 for the x coefficients
    (lambda sd: _zero_denominator(sd), ["Perez denominator of the sky is zero"]),
])
def test_flattener_rejections(mts, lums, words):
    sd, _ = _sky_scene(mts, lums=lums)
    with pytest.raises(mts.MtsGpuError) as e:
        mts.Scene(sd)
    for w in words:
        assert w in str(e.value), str(e.value)


def _zero_denominator(sd):
    """turbidity 0 makes the Perez L coefficient B = .42749 * bConst and A = -1.46303 * aConst: with bConst = 0 the first
    factor of the L denominator is 1 + A, which aConst = 1 / 1.46303 makes exactly 0 in binary32 when A rounds to -1"""
    l = sd.sky(sun_direction=(0.2, 0.1, 0.9), turbidity=0.0, b=0.0)
    a = F(1.0 / 1.46303)
    for cand in (a, np.nextafter(a, F(0)), np.nextafter(a, F(1))):
        if F(np.float64(-1.46303) * np.float64(cand)) == F(-1):
            sd.lum_params[l][18] = cand
            return l
    raise AssertionError("no binary32 aConst gives A = -1")


def test_zenith_y_of_the_cases_is_not_zero(mts):
    """the shared check refuses a zenith y of exactly 0 (Y / y, sky.cpp:484).  No binary32 pair (turbidity, thetaS) is known
    that makes the polynomial vanish exactly, so that refusal has no case of its own here; what is checked is that none of
    the case list's skies is anywhere near it"""
    for name, P in sky_cases.parameter_sets(mts):
        assert abs(mts.sky_configure(P)[1]) > 0.05, name


# --- ABI -------------------------------------------------------------------------------------------------------------
def test_abi_surface(mts):
    L, a = mts.lib(), mts.abi
    assert L.mtsgpu_abi_version() == a.ABI_VERSION == 8
    assert a.LUM_SKY == 7 and a.LUM_NPARAMS == 32 and a.SKY_NDERIVED == 24
    for name in ("mtsgpu_sky_configure", "mtsgpu_lum_eval"):
        assert name in mts.EXPORTS and hasattr(L, name)
    for which, typ in enumerate([a.Scene, a.Camera, a.Stats, a.Mesh, a.SceneDesc, a.KdParams]):
        assert L.mtsgpu_abi_sizeof(which) == C.sizeof(typ), typ.__name__
    # unchanged since the sky did not exist: sizeof(mtsgpu_scene) on LP64
    assert [L.mtsgpu_abi_sizeof(i) for i in range(6)] == [288, 172, 184, 72, 96, 48]
    header = open(mts.__file__.replace("mitsuba-renderer_amd/__init__.py", "include/mtsgpu.h")).read()
    for line in ("#define MTSGPU_ABI_VERSION 8", "MTSGPU_LUM_SKY = 7", "#define MTSGPU_LUM_NPARAMS 32", "#define MTSGPU_BSDF_NPARAMS 16",
                 "int  mtsgpu_sky_configure(const float *block, float *derived);", "int  mtsgpu_lum_eval(mtsgpu_ctx *ctx, uint32_t lum_type"):
        assert line in header, line
    doc = open(mts.__file__.replace("mitsuba-renderer_amd/__init__.py", "INTEGRATION.md")).read()
    assert "mtsgpu_sky_configure" in doc and "mtsgpu_lum_eval" in doc


# --- the inputs of the device comparison stay decidable --------------------------------------------------------------
@pytest.mark.parametrize("k", range(12))
def test_device_comparison_inputs_stay_under_the_ambiguity_cap(mts, k):
    """closed_forms.MAX_AMBIGUOUS is a condition on the inputs, decided by the restatement alone: counted here on the
    directions and samples the device test draws (same generator seeds).  No edge class is left out as a whole."""
    cases = sky_cases.parameter_sets(mts)
    assert len(cases) == 12
    name, P = cases[k]
    rng = np.random.RandomState(900 + k)
    dirs, classes = sky_cases.directions(P, rng)
    val, cond, amb = ref64_sky.le(P, dirs)
    assert amb.sum() <= cf.MAX_AMBIGUOUS * len(dirs), (name, int(amb.sum()), len(dirs))
    # Directions on the horizon of a CLIPPED sky are undecidable by nature (d.z = 0 within its rounding): the device test
    # holds them to "exactly black, or the unclipped value", so what must stay decidable for them is the unclipped sky
    P_open = P.copy(); P_open[2] = 0
    _, _, amb_open = ref64_sky.le(P_open, dirs)
    for cls, idx in classes.items():
        on_horizon = P[2] != 0 and cls in ("horizon", "horizon + 1 ulp", "horizon - 1 ulp")
        assert not (amb_open if on_horizon else amb)[idx].all(), (name, cls)
    assert np.isfinite(val).all() and (val >= 0).all()
    # the reach of the comparison: cond is a worst-case first-order bound, so 16 * 2^-23 * cond is the tolerance a record gets.
    # At cond 1e3 that is 0.2 % of the value, at 1e4 2 %: beyond that a record shows little more than the absence of NaNs.  At
    # least 95 % of the lit, decidable records must lie below the first figure and 99 % below the second.
    lit = ~amb & (val != 0).any(axis=1)
    assert (cond[lit] < 1e3).mean() >= 0.95 and (cond[lit] < 1e4).mean() >= 0.99, (name, float((cond[lit] < 1e3).mean()), float((cond[lit] < 1e4).mean()))
    s = cf.sample_inputs(rng, 4000)
    r = ref64_sky.sample(P, sky_cases.sample_points(rng, len(s)), s)
    assert r.amb.sum() <= cf.MAX_AMBIGUOUS * len(s), (name, int(r.amb.sum()))
    _, _, amb_v = ref64_sky.le(P, -r.d.astype(np.float32))
    assert amb_v.sum() <= cf.MAX_AMBIGUOUS * len(s), (name, int(amb_v.sum()))


def test_restatement_flags_its_branches(mts):
    """what ref64_sky flags: a direction on the horizon of a clipped sky, one at d.z = 0.001, the sun's own direction"""
    P = dict(sky_cases.parameter_sets(mts))["sun at zenith, turbidity 2"]
    M = P[7:16].reshape(3, 3).astype(np.float64)
    loc = np.array([[1.0, 0.0, 0.0], [1.0, 0.0, 0.001], [0.0, 0.0, 1.0], [0.6, 0.0, 0.8]])
    val, cond, amb = ref64_sky.le(P, (loc @ M).astype(np.float32))
    assert amb[0] and amb[1] and amb[2] and not amb[3]
    # below a clipped horizon the restatement is exactly black
    val, cond, amb = ref64_sky.le(P, (np.array([[0.6, 0.0, -0.8]]) @ M).astype(np.float32))
    assert (val == 0).all() and not amb.any()
