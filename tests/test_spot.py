"""Projection textures of the spot luminaire, host side (no GPU): the float32 mirror of tests/ref64_spot.py inside the binary64
restatement's bound on every case of tests/spot_cases.py, the fragile share, every mutation reported, hand-computed records,
mtsgpu_spot_textures_check walked through every refusal and the acceptances next to them, uvFactor of the layout against the mirror
bit for bit, the ABI (mtsgpu.h's exports unchanged, the new header's present, the struct sizes), and what
SceneDescription.spot_light(texture=...) hands to the library.  The device side is tests/test_gpu_spot.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ref64_bmp as B
import ref64_spot as R
import ref64_tex as T
import spot_cases as SC

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def evaluated(mts):
    """every case once: (name, spot, texture, points, mirror, restatement)"""
    out = []
    for i, (name, spot, st) in enumerate(SC.cases(mts)):
        p = SC.points(spot, st, seed=i)
        out.append((name, spot, st, p, R.mirror(spot, st, p), R.restate(spot, st, p)))
    return out


# --- 1. the mirror against the restatement -----------------------------------------------------------------------------------------
def test_mirror_inside_the_bound_and_fragile_share(evaluated):
    """the mirror's value and uv lie inside the restatement's first-order bound on every record that is not fragile; at most 1 % of
    the records are fragile -- the case counts are chosen so that the restatement alone stays within that"""
    n = frag = 0
    worst = 0.0
    for name, spot, st, p, m, r in evaluated:
        ok = ~r.fragile
        n += len(p); frag += int(r.fragile.sum())
        err = np.abs(m.value.astype(np.float64) - r.value64)[ok]
        bound = r.bound[ok] + 1e-45
        assert (err <= bound).all(), (name, float((err / bound).max()))
        worst = max(worst, float((err / bound).max()) if err.size else 0.0)
        uerr = np.abs(m.uv.astype(np.float64) - r.uv64)[ok].max(axis=1) if ok.any() else np.zeros(0)
        assert (uerr <= r.uv_bound[ok] + 1e-45).all(), name
        # the cases reach what they are there for: lit and dark records, both sides of the beam
        assert r.inside.any() and (~r.inside).any(), name
    print("records %d, fragile %d (%.3f %%), largest error over bound %.3f" % (n, frag, 100.0 * frag / n, worst))
    assert frag <= 0.01 * n, (frag, n)
    assert 0.0 < worst <= 1.0


def test_every_mutation_is_reported(evaluated):
    """each mutation of ref64_spot.MUTATIONS changes the mirror bit for bit on some record, and -- unless it changes roundings only
    -- puts the mutated restatement outside the bound of the mirror on a record that is not fragile"""
    seen32 = {m: False for m in R.MUTATIONS}
    seen64 = {m: False for m in R.MUTATIONS}
    for name, spot, st, p, m, r in evaluated[::3]:
        ok = ~r.fragile
        for mut in R.MUTATIONS:
            mm = R.mirror(spot, st, p, mut)
            if not np.array_equal(bits(mm.value), bits(m.value)):
                seen32[mut] = True
            if mut in R.ROUNDING_MUTATIONS or seen64[mut]:
                continue
            v = R.sample(spot, st, p, np.float64, mut).value
            if (np.abs(m.value.astype(np.float64) - v)[ok] > r.bound[ok] + 1e-45).any():
                seen64[mut] = True
    assert all(seen32.values()), [k for k, v in seen32.items() if not v]
    missing = [k for k, v in seen64.items() if not v and k not in R.ROUNDING_MUTATIONS]
    assert not missing, missing
    assert len(R.MUTATIONS) >= 10


# --- 2. hand-computed records ----------------------------------------------------------------------------------------------------
def _point_for_uv(spot, u, v, dist=2.0):
    return SC._from_uv(spot, np.array([u]), np.array([v]), np.array([dist]))


def test_hand_computed_records(mts):
    """cutoff = beam = 45 degrees: uvFactor = 1 and no ramp.  The axis point maps to uv = (0.5, 0.5); one point per checker colour;
    a bilinear lookup at a texel centre returns the texel, and at the corner of four texels their mean"""
    spot = SC.down_spot(mts)
    I = spot.intensity.astype(np.float64)
    checker = R.SpotTex(T.Tex(T.CHECKERBOARD, bright=1.0, dark=0.25))
    # the axis: d = (0, -1, 0), localDir = (0, 0, 1), uv = (0.5, 0.5): 2 uv = (1, 1), both odd: cx * cy = 1: bright
    m = R.mirror(spot, checker, np.float32([[0.0, 0.0, 0.0]]))
    assert np.array_equal(m.uv, np.float32([[0.5, 0.5]])) and np.array_equal(m.d, np.float32([[0.0, -1.0, 0.0]]))
    assert np.array_equal(m.value[0], (spot.intensity * F(1.0)) * F(0.25))         # 1 / dist^2 = 1 / 4
    # uv = (0.25, 0.75): (int)(0.5) = 0 even -> -1, (int)(1.5) = 1 odd -> +1: dark
    p = _point_for_uv(spot, 0.25, 0.75)
    m, r = R.mirror(spot, checker, p), R.restate(spot, checker, p)
    assert not r.fragile[0] and abs(r.uv64[0, 0] - 0.25) < 1e-6 and abs(r.uv64[0, 1] - 0.75) < 1e-6
    d2 = ((p[0].astype(np.float64) - spot.position) ** 2).sum()
    assert np.allclose(r.value64[0], I * 0.25 / d2, rtol=1e-6) and np.allclose(m.value[0], I * 0.25 / d2, rtol=1e-5)
    # uv = (0.75, 0.75): both odd: bright
    p = _point_for_uv(spot, 0.75, 0.75)
    r = R.restate(spot, checker, p)
    d2 = ((p[0].astype(np.float64) - spot.position) ** 2).sum()
    assert np.allclose(r.value64[0], I * 1.0 / d2, rtol=1e-6)
    # a 4 x 4 bitmap, bilinear: the centre of texel (x = 2, y = 1) is uv = (2.5 / 4, 1.5 / 4)
    tx = np.random.RandomState(5).uniform(0.1, 1.0, (4, 4, 3)).astype(np.float32)
    bil = R.SpotTex(B.Bmp(tx, B.CLAMP), True)
    p = _point_for_uv(spot, 2.5 / 4, 1.5 / 4)
    r = R.restate(spot, bil, p)
    d2 = ((p[0].astype(np.float64) - spot.position) ** 2).sum()
    assert np.allclose(r.value64[0], I * tx[1, 2] / d2, rtol=1e-5)
    # the corner shared by texels (1, 1), (2, 1), (1, 2), (2, 2) is uv = (0.5, 0.5): dx = dy = 0.5, the mean of the four
    r = R.restate(spot, bil, np.float32([[0.0, 0.0, 0.0]]))
    mean = tx[1:3, 1:3].astype(np.float64).reshape(4, 3).mean(axis=0)
    assert np.allclose(r.value64[0], I * mean / 4.0, rtol=1e-12)
    m = R.mirror(spot, bil, np.float32([[0.0, 0.0, 0.0]]))
    assert np.allclose(m.value[0], I * mean / 4.0, rtol=1e-6)
    # the column quirk: under `black` a tap in column 0 is the constant.  uv = (0.5 / 4, 2.5 / 4): xPos = 0, dx = 0: T00 alone, black
    blk = R.SpotTex(B.Bmp(tx, B.BLACK_MODE), True)
    r = R.restate(spot, blk, _point_for_uv(spot, 0.5 / 4 + 1e-4, 2.5 / 4))
    assert r.value64[0].max() < 1e-3 * I.max()


# --- 3. the check ----------------------------------------------------------------------------------------------------------------
def _refused(mts, match, *a, **k):
    with pytest.raises(mts.MtsGpuError, match=match):
        mts.spot_textures_check(*a, **k)


def test_check_walks_every_refusal_and_the_acceptances_next_to_them(mts):
    S, A = mts.scenes, mts.abi
    sp = SC.spots(mts)
    deg = F(np.pi) / F(180.0)

    def block(cutoff_deg, beam_deg=10.0):
        P = sp[0].block.copy()
        P[8] = F(cutoff_deg) * deg; P[19] = F(beam_deg) * deg
        P[7] = F(np.cos(np.float64(P[8]))); P[6] = F(np.cos(np.float64(P[19]))); P[9] = F(1) / (P[8] - P[19])
        return P
    lt = [A.LUM_POINT, A.LUM_SPOT]
    lp = np.stack([np.zeros(A.LUM_NPARAMS, np.float32), block(60.0)])
    chk = S.Checkerboard(bright=1.0, dark=0.25)
    grid = S.GridTexture(uscale=4.0, vscale=4.0, uoffset=0.25)
    tx16 = SC.bilinear_texels("16x16")
    bmp = S.BitmapTexture(texels=tx16, wrap="clamp")
    one = S.BitmapTexture(texels=np.full((1, 1, 3), 0.5, np.float32))
    odd = S.BitmapTexture(texels=np.full((3, 5, 3), 0.5, np.float32))
    # acceptances: every kind, both filter flags, a 1 x 1 bilinear bitmap, an odd size with the nearest lookup, cutoff 89.9
    f = mts.spot_textures_check(lt, lp, [chk, grid, bmp, one, odd], [0, 0, 1, 1, 0], [-1, 2])
    assert f[0] == 0.0 and bits(f[1]) == bits(R.uv_factor(R.Spot(lp[1]), np.float32, fn=dict(tan=lambda a: mts.devmath("tan", [a])[0])))
    for k in range(5):
        mts.spot_textures_check(lt, lp, [chk, grid, bmp, one, odd], [0, 0, 1, 1, 0], [-1, k])
    lp89 = np.stack([lp[0], block(89.9)])
    assert mts.spot_textures_check(lt, lp89, [chk], [0], [-1, 0])[1] > 500.0
    # switched off: all -1, or nothing at all
    assert not mts.spot_textures_check(lt, lp, [chk], [0], [-1, -1]).any()
    assert not mts.spot_textures_check(lt, lp, None, None, None).any()
    # ... even beside a mask, a snow table or a cloth table
    assert not mts.spot_textures_check(lt, lp, [chk], [0], [-1, -1], in_force=7).any()
    # refusals
    _refused(mts, "power of two", lt, lp, [odd], [1], [-1, 0])
    _refused(mts, "cutoffAngle < 90", lt, np.stack([lp[0], block(90.0)]), [chk], [0], [-1, 0])
    _refused(mts, "cutoffAngle < 90", lt, np.stack([lp[0], block(120.0)]), [chk], [0], [-1, 0])
    _refused(mts, "not a spot", lt, lp, [chk], [0], [0, -1])
    _refused(mts, "texture index 1 out of range", lt, lp, [chk], [0], [-1, 1])
    _refused(mts, "texture index -2 out of range", lt, lp, [chk], [0], [-1, -2])
    _refused(mts, "unknown filter flag 2", lt, lp, [bmp], [2], [-1, 0])
    bad = chk.descriptor(); bad.kind = 7
    _refused(mts, "unknown kind 7", lt, lp, [bad], [0], [-1, 0], bitmaps=[], texture_bitmap=None)
    nan = S.Checkerboard(uscale=float("nan"))
    _refused(mts, "non-finite parameter", lt, lp, [nan], [0], [-1, 0])
    lpn = lp.copy(); lpn[1, 4] = np.inf
    _refused(mts, "non-finite spot parameter", lt, lpn, [chk], [0], [-1, 0])
    bw = bmp.bitmap(); bw.wrap_mode = 9
    _refused(mts, "unknown wrap mode 9", lt, lp, [bmp.descriptor()], [0], [-1, 0], bitmaps=[bw], texture_bitmap=[0])
    _refused(mts, "bitmap index 3 out of range", lt, lp, [bmp.descriptor()], [0], [-1, 0], bitmaps=[bmp.bitmap()], texture_bitmap=[3])
    # the casts: (|scale| + |offset| + 1) * max(2, w, h) against 2^31 - 2^16
    lim = 2147483648.0 - 65536.0
    mts.spot_textures_check(lt, lp, [S.Checkerboard(uscale=lim / 2 - 2.0e3)], [0], [-1, 0])
    _refused(mts, r"\(int\) cast", lt, lp, [S.Checkerboard(uscale=lim / 2)], [0], [-1, 0])
    _refused(mts, r"\(int\) cast", lt, lp, [S.Checkerboard(voffset=-lim / 2)], [0], [-1, 0])
    mts.spot_textures_check(lt, lp, [S.BitmapTexture(texels=tx16, uscale=lim / 16 - 2.0e3)], [1], [-1, 0])
    _refused(mts, r"\(int\) cast", lt, lp, [S.BitmapTexture(texels=tx16, vscale=-lim / 16)], [1], [-1, 0])
    # a mask, a snow table or a cloth table in force
    for bit, word in ((1, "mask"), (2, "snow"), (4, "cloth")):
        _refused(mts, word + ".*textured spot", lt, lp, [chk], [0], [-1, 0], in_force=bit)
    _refused(mts, "textures without lum_texture", lt, lp, [chk], [0], None)


def test_uv_factor_of_the_layout_is_the_mirrors(mts):
    """tan(cutoffAngle) of every case's spot, bit for bit: the layout's, the mirror's with the library's tangent, and the mirror's
    own (the correctly rounded binary64 tangent)"""
    sp = SC.spots(mts)
    lt = [mts.abi.LUM_SPOT] * len(sp)
    lp = np.stack([s.block for s in sp])
    f = mts.spot_textures_check(lt, lp, [mts.scenes.Checkerboard()], [0], [0] * len(sp))
    fn = dict(tan=lambda a: mts.devmath("tan", [a])[0])
    for k, s in enumerate(sp):
        assert bits(f[k]) == bits(R.uv_factor(s, np.float32, fn)) == bits(R.uv_factor(s, np.float32)), k
        assert abs(float(f[k]) - R.uv_factor(s, np.float64)) <= 2.0 ** -23 * float(f[k])


# --- 4. the ABI and the mirror of the description ----------------------------------------------------------------------------------
def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mtsgpu_[a-z0-9_]+)\s*\(", src)))


def test_abi_is_version_8_and_the_header_declares_the_exports(mts):
    L = mts.lib()
    assert L.mtsgpu_abi_version() == 8
    L.mtsgpu_abi_sizeof.restype = C.c_size_t
    assert [L.mtsgpu_abi_sizeof(i) for i in range(6)] == [288, 172, 184, 72, 96, 48]
    assert sorted(mts.EXPORTS) == _declared("mtsgpu.h")
    assert sorted(mts.SPOT_EXPORTS) == _declared("mtsgpu_spot.h")
    assert C.sizeof(mts.abi.UvTexture) == 48 and C.sizeof(mts.abi.Bitmap) == 24
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in mts.SPOT_EXPORTS + ["mtsgpu_spot.h"]:
        assert name in doc, name
    for name in mts.SPOT_EXPORTS:
        assert hasattr(L, name)


def test_spot_light_with_a_texture_and_its_argument_arrays(mts):
    S = mts.scenes
    tx = SC.bilinear_texels("2x2")
    sd = SC.e2e_description(mts, extra_light=True)
    assert mts.Scene(sd).spot_texture_args() is None and not getattr(sd, "spot_textures", None)
    sd = S.SceneDescription("three")
    b = sd.lambertian(0.5)
    sd.add_mesh(np.float32([[-1, 0, -1], [1, 0, -1], [0, 0, 1]]), np.uint32([[0, 1, 2]]), bsdf=b, face_normals=True, name="floor")
    sd.point_light((0, 1, 0), 1.0)
    l1 = sd.spot_light((0, 2, 0), (0, 0, 0), 1.0, texture=S.BitmapTexture(texels=tx, wrap="white"), bilinear=True)
    l2 = sd.spot_light((0, 2, 1), (0, 0, 0), 1.0)
    l3 = sd.spot_light((1, 2, 0), (0, 0, 0), 1.0, texture=S.Checkerboard(), bilinear=True)
    l4 = sd.spot_light((1, 2, 1), (0, 0, 0), 1.0, texture=S.BitmapTexture(texels=tx, wrap="white"))
    textures, flags, lum = sd.spot_texture_table()
    assert [l1, l2, l3, l4] == [1, 2, 3, 4] and lum.tolist() == [-1, 0, -1, 1, 2] and flags.tolist() == [1, 1, 0]
    assert [t.kind for t in textures] == [mts.abi.TEX_BITMAP, mts.abi.TEX_CHECKERBOARD, mts.abi.TEX_BITMAP]
    sc = mts.Scene(sd)
    n_tex, tarr, n_bmp, barr, tb, fl, lx = sc.spot_texture_args()
    assert n_tex == 3 and n_bmp == 1 and tarr[1].kind == mts.abi.TEX_CHECKERBOARD and barr[0].width == 2 and barr[0].wrap_mode == mts.abi.WRAP_WHITE
    assert [tb[i] for i in range(3)] == [0, -1, 0] and [fl[i] for i in range(3)] == [1, 1, 0] and [lx[i] for i in range(5)] == [-1, 0, -1, 1, 2]
    # the library accepts exactly these arrays for this scene's luminaires
    A = sc.arrays()
    f = mts.spot_textures_check(A["lum_type"], A["lum_params"], textures, flags, lum)
    assert (f > 0).tolist() == [False, True, False, True, True]
    with pytest.raises(TypeError):
        sd.spot_light((0, 2, 0), (0, 0, 0), 1.0, texture=0.5)
