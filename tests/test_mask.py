"""The mask BSDF, host side (no GPU): the float32 mirror of tests/ref64_mask.py against its binary64 restatement on the shared
inputs of tests/mask_cases.py, every mutation reported by the module's own check, the luminance, SceneDescription.mask (table,
averages, refusals), the argument builders of the two older texture calls unchanged, and the ABI: version 8, the pinned sizes,
the new exports declared, exported and documented.  The device side is tests/test_gpu_mask.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mask_cases
import ref64_mask as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["mtsgpu_set_uv_masked_textures", "mtsgpu_group_set_uv_masked_textures", "mtsgpu_bsdf_eval_masked"]


def _runs(mts, mutation=None):
    """(op, got, want, skip) of every model x opacity x op on the shared inputs"""
    ewi, ewo = mask_cases.eval_records()
    for name, btype, P in mask_cases.models(mts):
        for p in mask_cases.P_VALUES:
            swi, ss = mask_cases.sample_records(p)
            for op, wi, aux in ((0, ewi, ewo), (1, ewi, ewo), (2, swi, ss)):
                got = R.mask32(btype, P, F(p), op, wi, aux, mutation)
                want = R.mask64(btype, P, F(p), op, wi, aux)
                yield name, p, op, got, want, (R.undefined(F(p), aux) if op == 2 else None)


def test_the_mirror_agrees_with_binary64(mts):
    n = taken = through = 0
    for name, p, op, got, want, skip in _runs(mts):
        bad = R.check(op, got, want, skip)
        assert len(bad) == 0, (name, p, op, bad[:8])
        if op == 2:
            n += len(want.took_nested); taken += int(want.took_nested.sum()); through += int((~want.took_nested).sum())
    print("%d sample records: %d nested, %d pass-through" % (n, taken, through))
    assert taken > n // 4 and through > n // 4


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_mutations_are_reported(mts, mutation):
    if mutation == "channel_mean":
        rgb = np.float32(mask_cases.COLOURS)
        off = np.abs(R.luminance32(rgb, mutation).astype(np.float64) - R.luminance64(rgb)) > R.luminance_bound(rgb)
        print("channel_mean: %d of %d colours reported" % (off.sum(), len(rgb)))
        assert off.all()
        return
    reported = sum(len(R.check(op, got, want, skip)) for _, _, op, got, want, skip in _runs(mts, mutation))
    print("%s: %d records reported" % (mutation, reported))
    assert reported > 0


def test_luminance():
    rgb = np.float32(mask_cases.COLOURS + [(p, p, p) for p in mask_cases.P_VALUES])
    l32, l64 = R.luminance32(rgb), R.luminance64(rgb)
    assert (np.abs(l32.astype(np.float64) - l64) <= R.luminance_bound(rgb)).all()
    # hand-computed: the three weights, and a grey level is its own luminance in binary32 for the shared opacities
    assert l32[1] == F(0.212671) and l32[2] == F(0.072169) and l32[4] == F(0.715160)
    assert l32[0] == (F(0.2) * F(0.212671) + F(0.7) * F(0.715160)) + F(0.1) * F(0.072169)
    assert np.array_equal(l32[len(mask_cases.COLOURS):], np.float32(mask_cases.P_VALUES))


def test_the_planted_undefined_records():
    for p in mask_cases.P_VALUES:
        wi, s = mask_cases.sample_records(p)
        planted = mask_cases.planted_undefined(p, s)
        assert np.array_equal(planted, R.undefined(F(p), s))
        assert planted.sum() == (2 * len(mask_cases.directions()) if p == 0 else 0)
        xs = mask_cases.sample_x(p)
        assert all(0 <= x < 1 for x in xs)
        if 0 < p < 1:
            assert float(F(p)) in xs and float(np.nextafter(F(p), F(0))) in xs and float(np.nextafter(F(p), F(2))) in xs


def test_scene_description_mask_table_averages_and_refusals(mts):
    S, A = mts.scenes, mts.abi
    sd = S.SceneDescription("m")
    check = S.Checkerboard()
    tx = np.float32([[[0.2, 0.5, 0.1], [0.9, 0.3, 0.4]], [[0.6, 0.7, 1.5], [0.05, 0.8, 0.25]]])
    bmp = S.BitmapTexture(texels=tx, wrap="repeat")
    lam, ph, mir, dt = sd.lambertian(check), sd.twosided(sd.phong(9.0)), sd.mirror(0.5), sd.difftrans(0.4)
    comp = sd.composite([0.5, 0.5], [lam, dt])
    assert sd.mask(ph) == ph and sd.mask(mir, (0.1, 0.2, 0.3)) == mir
    free = sd.lambertian(0.3)
    assert sd.mask(free, bmp) == free
    assert sd.textures == [check, bmp], "a mask's texture joins the scene's list"
    rows = sd.mask_table()
    assert [r[0] for r in rows] == [A.MASK_NONE, A.MASK_CONSTANT, A.MASK_CONSTANT, A.MASK_NONE, A.MASK_NONE, A.MASK_TEXTURE]
    assert [r[1] for r in rows] == [-1, -1, -1, -1, -1, 1]
    assert rows[ph][2] == [F(0.5)] * 3, "the default opacity is the constant 0.5"
    assert rows[mir][2] == [F(0.1), F(0.2), F(0.3)]
    assert np.array_equal(np.float32(rows[free][2]), bmp.average()) and np.array_equal(bmp.average(), tx[0, 0])
    assert sd.bsdf_type[ph] & A.BSDF_TWOSIDED, "mask(twosided(x)): the type keeps the adapter bit, the mask is a side table"
    assert sd.bsdf_slot_texture[free] == [-1, -1] and sd.bsdf_slot_texture[lam] == [0, -1]
    other = S.GridTexture()
    sd.mask(sd.lambertian(0.1), other)
    assert sd.textures == [check, bmp, other] and sd.mask_table()[-1][:2] == (A.MASK_TEXTURE, 2)
    with pytest.raises(ValueError, match="vertex colours"):
        sd.mask(sd.lambertian(0.2), S.VERTEX_COLORS)
    with pytest.raises(ValueError, match="around a composite"):
        sd.mask(comp)
    with pytest.raises(ValueError, match="inside a composite"):
        sd.mask(lam)
    with pytest.raises(ValueError, match="nested masks"):
        sd.mask(ph, 0.25)
    with pytest.raises(ValueError, match="not finite"):
        sd.mask(sd.lambertian(0.2), float("nan"))
    # the flattened scene keeps the table, and asks for the new call only because a BSDF is masked
    g = S.vcol_grid(2).meshes[0]
    for i in range(len(sd.bsdf_type)):
        sd.add_mesh(g.positions + F(i), g.triangles, bsdf=i)
    sd.point_light((0, 3, 0), 1.0)
    scene = mts.Scene(sd)
    m = scene.bsdf_mask
    assert m is not None and len(m) == len(sd.bsdf_type)
    assert [m[i].kind for i in range(6)] == [0, 1, 1, 0, 0, 2] and m[free].texture == 1 and m[mir].reserved == 0
    assert list(m[mir].opacity) == [F(0.1), F(0.2), F(0.3)] and list(m[free].opacity) == list(tx[0, 0])
    args = scene.uv_masked_texture_args()
    assert args is not None and len(args) == 9 and args[2] == 3 and args[5] == 1 and args[8] is m


def test_the_older_texture_calls_take_what_they_took(mts):
    S = mts.scenes
    plain = mts.Scene(S.cornell_tex())
    assert plain.bsdf_mask is None and plain.uv_masked_texture_args() is None
    assert plain.uv_bitmap_texture_args() is None and plain.uv_texture_args() is not None and len(plain.uv_texture_args()) == 5
    bmp = mts.Scene(S.cornell_bmp())
    assert bmp.bsdf_mask is None and bmp.uv_masked_texture_args() is None and len(bmp.uv_bitmap_texture_args()) == 8
    c1 = mts.Scene(S.cornell_c1())
    assert c1.bsdf_mask is None and c1.uv_masked_texture_args() is None and c1.uv_texture_args() is None
    # a mask alone: no slot table, no bitmaps, and the two older builders still say "nothing"
    sd = S.cornell_c1()
    sd.mask(0, 1.0)
    masked = mts.Scene(sd)
    assert masked.uv_texture_args() is None and masked.uv_bitmap_texture_args() is None
    args = masked.uv_masked_texture_args()
    assert args[2] == 0 and args[3] is None and not args[4] and args[5] == 0 and args[6] is None and args[8] is masked.bsdf_mask


def test_abi_is_unchanged_and_the_exports_exist(mts):
    L, a = mts.lib(), mts.abi
    assert L.mtsgpu_abi_version() == a.ABI_VERSION == 8
    assert [L.mtsgpu_abi_sizeof(i) for i in range(6)] == [288, 172, 184, 72, 96, 48]
    assert a.BSDF_NTYPES == 10
    core = open(os.path.join(ROOT, "include", "mtsgpu.h")).read()
    header = open(os.path.join(ROOT, "include", "mtsgpu_mask.h")).read()
    find = lambda text: set(re.findall(r"\b(mtsgpu_[a-z0-9_]+)\s*\(", text))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    # the extension header declares exactly the new entry points; the list of mtsgpu.h, which ABI version 8 fixes, stays what it was
    assert find(header) == set(NEW_EXPORTS) == set(mts.MASK_EXPORTS) and not find(core) & set(NEW_EXPORTS)
    assert sorted(mts.EXPORTS) == sorted(find(core)) and not set(mts.EXPORTS) & set(NEW_EXPORTS)
    for name in NEW_EXPORTS:
        assert hasattr(L, name), name
        assert name in doc, name
    assert '#include "mtsgpu.h"' in header and "mtsgpu_mask.h" in core and "mtsgpu_mask.h" in doc
    assert "#define MTSGPU_ABI_VERSION 8" in core and "MTSGPU_BSDF_NTYPES = 10," in core
    assert "enum { MTSGPU_MASK_NONE = 0, MTSGPU_MASK_CONSTANT = 1, MTSGPU_MASK_TEXTURE = 2 };" in header
    assert "typedef struct mtsgpu_bsdf_mask {" in header and "} mtsgpu_bsdf_mask;" in header
    assert (a.MASK_NONE, a.MASK_CONSTANT, a.MASK_TEXTURE) == (0, 1, 2)
    assert C.sizeof(a.BsdfMask) == 24 and a.BsdfMask.texture.offset == 4 and a.BsdfMask.opacity.offset == 8 and a.BsdfMask.reserved.offset == 20
    assert C.sizeof(a.UvTexture) == 48 and C.sizeof(a.Bitmap) == 24
