"""The snow BRDFs `wiscombe` and `hanrahankrueger`, host side (no GPU): the library's two configure calls against the float32
mirror of tests/ref64_snow.py bit for bit and inside the bound of its binary64 restatement, their refusals; the mirror's f / pdf
/ sample inside the bound on the shared inputs of tests/snow_cases.py, every mutation reported, the cap on the fragile cases;
the two specifications the mirror uses in place of libm against the oracle's; SceneDescription's two constructors and
snow_table(); and the ABI: version 8, the pinned sizes, the new exports declared, exported and documented.  The device side is
tests/test_gpu_snow.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ref64_snow as R
import snow_cases

F = np.float32
EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["mtsgpu_wiscombe_configure", "mtsgpu_hk_configure", "mtsgpu_set_snow_bsdfs", "mtsgpu_group_set_snow_bsdfs",
               "mtsgpu_bsdf_eval_snow"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _library(mts, kind, raw):
    e = mts.snow_configure(kind, raw)
    assert e.kind == kind and e.reserved == 0
    return np.float32(list(e.derived))


def test_configure_equals_the_mirror_bit_for_bit_and_lies_inside_the_bound(mts):
    for name, kind, raw in snow_cases.models():
        got = _library(mts, kind, raw)
        mirror, dec32 = R.configure32(kind, raw)
        want, dec64 = R.configure64(kind, raw)
        assert np.array_equal(_bits(got), _bits(mirror)), (name, got, mirror)
        assert dec32 == dec64, (name, "eta > 1 / eta == 1 decided differently", dec32, dec64)
        assert (np.abs(got.astype(np.float64) - want.v) <= want.e).all(), (name, got, want.v, want.e)
        rel = want.e[want.v != 0] / np.abs(want.v[want.v != 0])
        assert rel.max() < 1e-4, (name, "a derived value whose bound says nothing", rel.max())
        assert not got[12:].any()
    # hand-computed: the delta-Eddington g* of the default and HK's albedo sigmaS / (sigmaA + sigmaS)
    d = _library(mts, R.WISCOMBE, R.wiscombe_raw())
    g = F(0.874)
    assert d[3] == (F(1) - d[0] * (g / (F(1) + g))) * (F(1) / (g / (F(1) + g))), "bStar = bTmp / gStar, as compiled"
    h = _library(mts, R.HK, R.hk_raw())
    assert h[0] == F(0.7) / (F(0.0014) + F(0.7)) and h[9] == 0 and h[10] == F(1.32) / F(1) and h[11] == 1
    assert list(h[3:6]) == [1, 1, 1]
    # eta == 1: Fdr = 0, Fdt = 1, so A = 1 and the exponent is (4/3) var1 rounded once
    one = _library(mts, R.HK, R.hk_raw(eta_int=1.5, eta_ext=1.5))
    ra = (F(0.7) * F(1)) / (F(0.0014) + F(0.7) * F(1))
    v1 = -np.sqrt((F(1) - ra) * F(3))
    assert one[6] == ((ra * F(0.5)) * (F(1) + R.dexp32(v1 * F(4.0 / 3.0)))) * R.dexp32(v1)


def test_configure_refusals(mts):
    L, a = mts.lib(), mts.abi
    out = a.BsdfSnow()
    raw = R.wiscombe_raw()
    f32p = C.POINTER(C.c_float)
    assert L.mtsgpu_wiscombe_configure(None, C.byref(out)) == EINVAL
    assert L.mtsgpu_wiscombe_configure(raw.ctypes.data_as(f32p), None) == EINVAL
    assert L.mtsgpu_hk_configure(None, C.byref(out)) == EINVAL
    assert L.mtsgpu_hk_configure(R.hk_raw().ctypes.data_as(f32p), None) == EINVAL
    with pytest.raises(mts.MtsGpuError, match=r"Wiscombe: bStar\[0\] is not finite \(g = 0"):
        mts.snow_configure(a.SNOW_WISCOMBE, R.wiscombe_raw(g=0.0))
    with pytest.raises(mts.MtsGpuError, match="Wiscombe: .* is not finite"):
        mts.snow_configure(a.SNOW_WISCOMBE, R.wiscombe_raw(w0=float("nan")))
    with pytest.raises(mts.MtsGpuError, match=r"HanrahanKrueger: albedo\[0\] is not finite \(sigmaA \+ sigmaS = 0"):
        mts.snow_configure(a.SNOW_HK, R.hk_raw(sigma_a=0.0, sigma_s=0.0))
    with pytest.raises(mts.MtsGpuError, match="HanrahanKrueger: .* is not finite .* / 0"):
        mts.snow_configure(a.SNOW_HK, R.hk_raw(eta_ext=0.0))
    with pytest.raises(ValueError):
        mts.snow_configure(a.SNOW_WISCOMBE, np.zeros(16, dtype=np.float32))
    # the mirror says the same of these inputs
    assert not np.isfinite(R.configure32(R.WISCOMBE, R.wiscombe_raw(g=0.0))[0]).all()
    assert not np.isfinite(R.configure32(R.HK, R.hk_raw(sigma_a=0.0, sigma_s=0.0))[0]).all()


def _runs(mutation=None):
    """(model, class, twosided, op, got, want) over the shared inputs; the derived values are the mirror's own"""
    for name, kind, raw in snow_cases.models():
        D = R.configure32(kind, raw, mutation if mutation in R.CONFIGURE_MUTATIONS else None)[0]
        D0 = R.configure32(kind, raw)[0]
        for cls in snow_cases.CLASSES:
            ewi, ewo = snow_cases.eval_records(cls)
            swi, ss = snow_cases.sample_records(cls)
            for two in (False, True):
                for op, wi, aux in ((0, ewi, ewo), (1, ewi, ewo), (2, swi, ss)):
                    got = R.eval32(kind, D, two, op, wi, aux, mutation)
                    want = R.eval64(kind, D0, two, op, wi, aux, got.local_wo if op == 2 else None)
                    yield name, cls, two, op, got, want


def test_the_mirror_lies_inside_the_bound_and_few_cases_are_fragile():
    """A case is fragile when a discrete decision differs between the precisions or its bound exceeds 1e-3 of the value; such
    cases are not compared, and at most 5 % of any class but the grazing one may be."""
    total, left_out = {}, {}
    for name, cls, two, op, got, want in _runs():
        skip = R.fragile(got, want, op)
        bad = R.check(op, got, want, skip)
        assert len(bad) == 0, (name, cls, two, op, bad[:8])
        total[cls] = total.get(cls, 0) + len(skip); left_out[cls] = left_out.get(cls, 0) + int(skip.sum())
    for cls in snow_cases.CLASSES:
        print("%-8s %6d records, %5d fragile (%.2f %%)" % (cls, total[cls], left_out[cls], 100.0 * left_out[cls] / total[cls]))
        if cls != snow_cases.GRAZING:
            assert left_out[cls] <= 0.05 * total[cls], cls
    assert sum(total.values()) > 4000
    assert left_out[snow_cases.GRAZING] < total[snow_cases.GRAZING], "the grazing class is compared as well"


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_mutations_are_reported(mutation):
    if mutation == "sample_signed_cos":
        # behind `wi.z <= 0 -> 0` and the adapter's flip no query reaches sample() with a negative cosine, so the interface
        # cannot tell cos from |cos|: the value expression is held to the restatement without that test in front of it
        D = R.configure32(R.WISCOMBE, R.wiscombe_raw())[0]
        wi, s = snow_cases.sample_records("oblique")
        below = wi[:, 2] < 0
        wi, s = wi[below], s[below]
        up = wi * np.float32([1, 1, -1])
        reported = {}
        for m in (None, mutation):
            got = R.eval32(R.WISCOMBE, D, False, 2, wi, s, m, guard=False)
            want = R.eval64(R.WISCOMBE, D, False, 2, up, s, got.local_wo)
            reported[m] = int((np.abs(got.f.astype(np.float64) - want.f.v) > want.f.e).any(axis=1).sum())
        print("%s: %d of %d unguarded records reported (%d without the mutation)" % (mutation, reported[mutation], len(s), reported[None]))
        assert reported[None] == 0 and reported[mutation] > 0
        assert sum(len(R.check(op, g, w, R.fragile(g, w, op))) for _, _, _, op, g, w in _runs(mutation) if op == 2) == 0
        return
    if mutation in R.CONFIGURE_MUTATIONS:
        off = 0
        for name, kind, raw in snow_cases.models():
            want, _ = R.configure64(kind, raw)
            got = R.configure32(kind, raw, mutation)[0]
            off += int((np.abs(got.astype(np.float64) - want.v) > want.e).any())
        print("%s: configure of %d models reported" % (mutation, off))
        assert off > 0
    reported = sum(len(R.check(op, got, want, R.fragile(got, want, op))) for _, _, _, op, got, want in _runs(mutation))
    print("%s: %d records reported" % (mutation, reported))
    assert reported > 0


def test_the_specifications_in_place_of_libm(orc):
    """dexp and squareToHemispherePSA of the mirror are the oracle's, bit for bit; base * sqrt(base) is within 1 ulp of pow"""
    L = orc.lib()
    xs = np.float32(list(np.linspace(-20, 3, 97)) + [0.0, -0.0, -1e-8, 88.5, 90.0, -103.5, -105.0, -87.4])
    L.orc_expf.restype = C.c_float; L.orc_expf.argtypes = [C.c_float]
    want = np.float32([L.orc_expf(float(x)) for x in xs])
    assert np.array_equal(_bits(R.dexp32(xs)), _bits(want))
    s = snow_cases.sample_points()
    want = np.zeros((len(s), 3), dtype=np.float32)
    f32p = C.POINTER(C.c_float)
    for i in range(len(s)):
        L.orc_square_to_hemisphere_psa(np.ascontiguousarray(s[i]).ctypes.data_as(f32p), want[i].ctypes.data_as(f32p))
    assert np.array_equal(_bits(R.hemisphere_psa32(s)), _bits(want))
    base = np.concatenate([np.linspace(1e-6, 4.0, 4001), [(1 - 0.5) ** 2, (1 + 0.5) ** 2, 1.0, 2.25, 0.0]])
    got, ref = R.pow15_32(base), np.power(base, 1.5)
    ulp = np.spacing(ref.astype(np.float32)).astype(np.float64)
    assert (np.abs(got.astype(np.float64) - ref) <= ulp).all()
    assert R.pow15_32(np.float64([2.25]))[0] == F(3.375) and R.pow15_32(np.float64([1.0]))[0] == 1


def test_scene_description_constructors_and_snow_table(mts):
    S, A = mts.scenes, mts.abi
    sd = S.SceneDescription("snow")
    lam = sd.lambertian(0.5)
    w = sd.wiscombe()
    h = sd.twosided(sd.hanrahan_krueger(g=0.5, size_multiplier=2.0, diffuse_reflectance=False))
    assert sd.bsdf_type == [A.BSDF_LAMBERTIAN, A.BSDF_LAMBERTIAN, A.BSDF_LAMBERTIAN | A.BSDF_TWOSIDED]
    assert not sd.bsdf_params[w].any() and not sd.bsdf_params[h].any(), "the main table's block of a snow entry is zero"
    assert sd.bsdf_snow[w][0] == A.SNOW_WISCOMBE and np.array_equal(sd.bsdf_snow[w][1], R.wiscombe_raw())
    assert np.array_equal(sd.bsdf_snow[h][1], R.hk_raw(g=0.5, size_multiplier=2.0, diffuse_reflectance=False))
    sd2 = S.SceneDescription("defaults"); k = sd2.hanrahan_krueger()
    assert np.array_equal(sd2.bsdf_snow[k][1], R.hk_raw()), "the reference's defaults"
    rows = sd.snow_table()
    assert rows[lam] is None and rows[w].kind == A.SNOW_WISCOMBE and rows[h].kind == A.SNOW_HK
    assert np.array_equal(_bits(list(rows[w].derived)), _bits(R.configure32(R.WISCOMBE, R.wiscombe_raw())[0]))
    assert np.array_equal(_bits(list(rows[h].derived)), _bits(R.configure32(R.HK, sd.bsdf_snow[h][1])[0]))
    # a configure of one's own takes the library's place
    seen = []
    sd.snow_table(lambda kind, raw: seen.append(kind))
    assert seen == [A.SNOW_WISCOMBE, A.SNOW_HK]
    # the flattened scene keeps the table; a scene without a snow BRDF has none
    g = S.vcol_grid(2).meshes[0]
    for i in range(len(sd.bsdf_type)):
        sd.add_mesh(g.positions + F(i), g.triangles, bsdf=i)
    sd.point_light((0, 3, 0), 1.0)
    t = mts.Scene(sd).bsdf_snow
    assert t is not None and len(t) == 3 and [t[i].kind for i in range(3)] == [0, 1, 2] and t[0].reserved == 0
    assert not any(t[0].derived)
    assert mts.Scene(S.cornell_c1()).bsdf_snow is None
    arr = mts.bsdf_snow_array([None, (A.SNOW_HK, [1, 2, 3]), rows[w]])
    assert [arr[i].kind for i in range(3)] == [0, 2, 1] and list(arr[1].derived)[:4] == [1, 2, 3, 0]


def test_abi_is_unchanged_and_the_exports_exist(mts):
    L, a = mts.lib(), mts.abi
    assert L.mtsgpu_abi_version() == a.ABI_VERSION == 8
    assert [L.mtsgpu_abi_sizeof(i) for i in range(6)] == [288, 172, 184, 72, 96, 48]
    assert a.BSDF_NTYPES == 10
    core = open(os.path.join(ROOT, "include", "mtsgpu.h")).read()
    header = open(os.path.join(ROOT, "include", "mtsgpu_snow.h")).read()
    find = lambda text: set(re.findall(r"\b(mtsgpu_[a-z0-9_]+)\s*\(", text))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the extension header declares exactly the new entry points; the list of mtsgpu.h, which ABI version 8 fixes, stays what it was
    assert find(header) == set(NEW_EXPORTS) == set(mts.SNOW_EXPORTS) and not find(core) & set(NEW_EXPORTS)
    assert sorted(mts.EXPORTS) == sorted(find(core)) and not (set(mts.EXPORTS) | set(mts.MASK_EXPORTS)) & set(NEW_EXPORTS)
    for name in NEW_EXPORTS:
        assert hasattr(L, name), name
        assert name in doc, name
    assert '#include "mtsgpu.h"' in header and "mtsgpu_snow.h" in core and "mtsgpu_snow.h" in doc
    assert "#define MTSGPU_ABI_VERSION 8" in core and "MTSGPU_BSDF_NTYPES = 10," in core
    assert "enum { MTSGPU_SNOW_NONE = 0, MTSGPU_SNOW_WISCOMBE = 1, MTSGPU_SNOW_HK = 2 };" in header
    assert "typedef struct mtsgpu_bsdf_snow {" in header and "} mtsgpu_bsdf_snow;" in header
    assert (a.SNOW_NONE, a.SNOW_WISCOMBE, a.SNOW_HK) == (0, 1, 2)
    assert C.sizeof(a.BsdfSnow) == 64 and a.BsdfSnow.kind.offset == 0 and a.BsdfSnow.reserved.offset == 4 and a.BsdfSnow.derived.offset == 8
    assert a.SNOW_NDERIVED == 14 and C.sizeof(a.BsdfMask) == 24
