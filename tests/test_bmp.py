"""Unfiltered bitmap textures, host side (no GPU): mtsgpu_ldr_texels against the binary64 gamma table of tests/ref64_bmp.py
inside its derived bound with the texel order exact, what it refuses, BitmapTexture's average and maximum per wrap mode at
hand-computed values, the slot table, block and bitmap list of a scene description, the restatement against its mirror and
hand-computed points, every mutation reported, the fragile share of the end-to-end inputs, and the ABI: version 8, the pinned
sizes, the header strings, the new exports declared, exported and documented.  The device side is tests/test_gpu_bmp.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bmp_cases
import ref64_bmp as R
import tex_cases

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["mtsgpu_set_uv_bitmap_textures", "mtsgpu_group_set_uv_bitmap_textures", "mtsgpu_bitmap_texture_eval", "mtsgpu_ldr_texels"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# --- mtsgpu_ldr_texels -------------------------------------------------------------------------------------------------
def _pixels(rng, bpp, w, h):
    """every byte value occurs among the first 256 table bytes"""
    n = {1: (w * h + 7) // 8, 8: w * h, 16: 2 * w * h, 24: 3 * w * h, 32: 4 * w * h}[bpp]
    d = rng.randint(0, 256, n).astype(np.uint8)
    step = max(bpp // 8, 1)
    k = min(256, n // step)
    d[:k * step:step] = np.arange(k, dtype=np.uint8)
    return d


@pytest.mark.parametrize("gamma", [-1.0, 2.2, 1.0, 0.45])
@pytest.mark.parametrize("bpp", [1, 8, 16, 24, 32])
def test_ldr_texels_are_the_binary64_table_inside_the_bound(mts, bpp, gamma):
    """each texel channel is the table entry of ITS byte (the order is exact: a bound-sized window around another entry's value
    does not contain it, checked below), and differs from the binary64 entry by no more than the derived bound"""
    w, h = 23, 13                      # 299 pixels: not a multiple of 8, more than 256
    data = _pixels(np.random.RandomState(bpp), bpp, w, h)
    got = mts.ldr_texels(data, gamma, bpp=bpp, width=w, height=h)
    assert got.shape == (h, w, 3) and got.dtype == np.float32
    table, bound = R.gamma_table(gamma)
    idx = R.ldr_indices(bpp, w, h, data)
    err = np.abs(got.astype(np.float64) - table[idx])
    ratio = (err[bound[idx] > 0] / bound[idx][bound[idx] > 0]).max()
    print("bpp %d, gamma %g: largest error / bound = %.3f over %d entries in use" % (bpp, gamma, ratio, len(np.unique(idx))))
    assert (err <= bound[idx]).all()
    assert (got[idx == 0] == 0).all() and np.isfinite(got).all() and (got >= 0).all()
    # the entries are further apart than their bounds, so the check above pins the entry, not only the value
    assert (np.diff(table) > bound[1:] + bound[:-1]).all()
    if bpp in (8, 24, 32):
        assert len(np.unique(idx)) == 256
    if bpp == 1:
        assert set(np.unique(idx)) == {0, 255}
    # one table for all channels and depths: equal bytes give equal bits
    flat, fi = bits(got).reshape(-1), idx.reshape(-1)
    first = {}
    for b, i in zip(flat.tolist(), fi.tolist()):
        assert first.setdefault(i, b) == b


def test_ldr_texels_layouts(mts):
    """the array forms of the Python mirror are the flat call, alpha is dropped, grey is replicated, and bit pos % 8 of byte pos / 8
    is pixel pos of a 1 bpp image"""
    rng = np.random.RandomState(3)
    rgba = rng.randint(0, 256, (4, 5, 4)).astype(np.uint8)
    t32 = mts.ldr_texels(rgba)
    assert np.array_equal(bits(t32), bits(mts.ldr_texels(rgba[..., :3].copy())))
    other = rgba.copy(); other[..., 3] = 255 - other[..., 3]
    assert np.array_equal(bits(t32), bits(mts.ldr_texels(other))), "alpha is dropped"
    grey = rgba[..., 0].copy()
    t8 = mts.ldr_texels(grey)
    assert np.array_equal(bits(t8), bits(t32[..., :1].repeat(3, axis=2)))
    assert np.array_equal(bits(mts.ldr_texels(rgba[..., [0, 3]].copy())), bits(t8)), "16 bpp: luminance, alpha"
    one = mts.ldr_texels(np.uint8([0b00000101, 0b00000010]), bpp=1, width=5, height=2)
    assert one[..., 0].tolist() == [[1, 0, 1, 0, 0], [0, 0, 0, 0, 1]]
    # sRGB at hand-computed entries: the linear segment, and the two ends
    t = mts.ldr_texels(np.uint8([[0, 10, 255]]))[0, :, 0]
    assert t[0] == 0 and t[1] == F(F(10) / F(255)) / F(12.92) and abs(float(t[2]) - 1.0) <= 10 * R.U24
    assert mts.ldr_texels(np.uint8([[51]]), gamma=1.0)[0, 0, 0] == F(51) / F(255)


def test_ldr_texels_refusals(mts):
    L, a = mts.lib(), mts.abi
    d = np.zeros(64, np.uint8); out = np.zeros(64 * 3, np.float32)
    dp, op = d.ctypes.data_as(C.POINTER(C.c_uint8)), a.ptr(out, a.f32p)
    for bpp in (0, 2, 4, 12, 48, 64, 128, -8):
        assert L.mtsgpu_ldr_texels(bpp, 2, 2, dp, C.c_float(-1), op) == -1
        assert L.mtsgpu_last_error(None).decode() == "%i bpp images are currently not supported!" % bpp
        with pytest.raises(mts.MtsGpuError, match="bpp images are currently not supported"):
            mts.ldr_texels(d, bpp=bpp, width=2, height=2)
    assert L.mtsgpu_ldr_texels(8, 0, 2, dp, C.c_float(-1), op) == -1 and "zero dimension (0 x 2)" in L.mtsgpu_last_error(None).decode()
    assert L.mtsgpu_ldr_texels(8, 2, 0, dp, C.c_float(-1), op) == -1 and "zero dimension" in L.mtsgpu_last_error(None).decode()
    assert L.mtsgpu_ldr_texels(8, 2, 2, None, C.c_float(-1), op) == -1 and "null argument" in L.mtsgpu_last_error(None).decode()
    assert L.mtsgpu_ldr_texels(8, 2, 2, dp, C.c_float(-1), None) == -1
    with pytest.raises(ValueError, match="bytes for"):
        mts.ldr_texels(d[:3], bpp=8, width=2, height=2)
    assert not out.any()


# --- the Python mirror -------------------------------------------------------------------------------------------------
def test_average_and_maximum_per_wrap_mode(mts):
    """average = triangle(0, 0, 0) = getTexel(0, 0, 0), where column 0 counts as out of range: texel (0, 0) under repeat and
    clamp, 0 under black, 1 under white; maximum per channel over the texels, at least 1 under white"""
    S = mts.scenes
    tx = np.float32([[[0.2, 0.5, 0.1], [0.9, 0.3, 0.4]], [[0.6, 0.7, 1.5], [0.05, 0.8, 0.25]]])
    want = {"repeat": ([0.2, 0.5, 0.1], [0.9, 0.8, 1.5]), "clamp": ([0.2, 0.5, 0.1], [0.9, 0.8, 1.5]),
            "black": ([0, 0, 0], [0.9, 0.8, 1.5]), "white": ([1, 1, 1], [1.0, 1.0, 1.5])}
    for wrap, (avg, mx) in want.items():
        t = S.BitmapTexture(texels=tx, wrap=wrap, uscale=3.0, voffset=0.5)      # getAverage() ignores the transform
        assert np.array_equal(t.average(), np.float32(avg)) and np.array_equal(t.maximum(), np.float32(mx)), wrap
        r = R.Bmp(tx, S.WRAP_MODES[wrap])
        assert np.array_equal(R.average(r), t.average()) and np.array_equal(R.maximum(r), t.maximum())
        d, b = t.descriptor(), t.bitmap()
        assert (d.kind, d.uscale, d.voffset, d.line_width, list(d.bright)) == (2, 3.0, 0.5, 0.0, [0, 0, 0])
        assert (b.width, b.height, b.wrap_mode, b.reserved) == (2, 2, S.WRAP_MODES[wrap], 0)
    assert [S.WRAP_MODES[k] for k in ("repeat", "clamp", "black", "white")] == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="texels or pixels"):
        S.BitmapTexture()
    with pytest.raises(ValueError, match=r"\[height\]\[width\]\[3\]"):
        S.BitmapTexture(texels=np.zeros((2, 2)))
    with pytest.raises(KeyError):
        S.BitmapTexture(texels=tx, wrap="mirror")
    px = np.random.RandomState(1).randint(0, 256, (3, 4, 3)).astype(np.uint8)
    t = S.BitmapTexture(pixels=px, gamma=2.2, wrap="clamp")
    assert (t.width, t.height) == (4, 3) and np.array_equal(bits(t.texels), bits(mts.ldr_texels(px, 2.2)))


def test_scene_description_slot_table_block_and_bitmap_list(mts):
    S = mts.scenes
    tx = bmp_cases.texels("5x3")
    a = S.BitmapTexture(texels=tx, wrap="repeat", uscale=2.0)
    b = S.BitmapTexture(texels=tx, wrap="repeat", vscale=-1.0)          # the same bitmap under another transform
    c = S.BitmapTexture(texels=tx, wrap="white")                          # another wrap mode: another bitmap
    check = S.Checkerboard()
    sd = S.SceneDescription("m")
    ids = [sd.lambertian(a), sd.phong(9.0, rd=check, rs=b, kd=0.3, ks=0.2), sd.microfacet(0.2, 0.4, 0.3, rd=c, rs=S.VERTEX_COLORS), sd.mirror(0.5)]
    assert sd.textures == [a, check, b, c] and sd.bsdf_slot_texture == [[0, -1], [1, 2], [3, -1], [-1, -1]] and sd.bsdf_color_slots == [0, 0, 2, 0]
    assert np.array_equal(sd.bsdf_params[ids[0]][:3], tx[0, 0]) and np.array_equal(sd.bsdf_params[ids[1]][8:11], tx[0, 0])
    assert np.array_equal(sd.bsdf_params[ids[2]][5:8], np.ones(3, np.float32)), "white: getAverage() is the column-0 constant"
    # verifyEnergyConservation reads getMaximum(): under white it is at least 1
    p = sd.bsdf_params[sd.phong(9.0, rd=c, rs=0.5, kd=1.0, ks=1.0)]
    assert p[1] == F(1) * (F(1) / (F(1) * F(1) + F(1) * F(0.5)))
    p = sd.bsdf_params[sd.phong(9.0, rd=a, rs=0.0, kd=1.0, ks=0.0)]
    assert p[1] == F(1), "the maximum %g of the texels is below 1: nothing is scaled" % tx.max()
    g = S.vcol_grid(2).meshes[0]
    for i in ids:
        sd.add_mesh(g.positions + F(i), g.triangles, bsdf=i, colors=g.colors)
    sd.point_light((0, 3, 0), 1.0)
    scene = mts.Scene(sd)
    assert scene.texture_bitmap.tolist() == [0, -1, 0, 1] and len(scene._bitmap_objects) == 2
    assert [scene.bitmaps[i].wrap_mode for i in range(2)] == [0, 3] and scene.bitmaps[0].width == 5 and scene.bitmaps[1].height == 3
    args = scene.uv_bitmap_texture_args()
    assert args is not None and len(args) == 8 and args[:5][2] == 4 and args[5] == 2
    assert [t.kind for t in scene.textures] == [2, 0, 2, 2]
    # a scene without a bitmap takes the old call with the old arguments
    plain = mts.Scene(S.cornell_tex())
    assert plain.uv_bitmap_texture_args() is None and plain.uv_texture_args() is not None and len(plain.uv_texture_args()) == 5
    assert mts.Scene(S.cornell_c1()).uv_bitmap_texture_args() is None
    mixed = mts.Scene(S.cornell_bmp())
    kinds = sorted(t.kind for t in mixed.textures)
    assert kinds == [0, 1, 2] and mixed.bsdf_color_slots is not None and mixed.uv_bitmap_texture_args() is not None


# --- the restatement ---------------------------------------------------------------------------------------------------
def test_hand_computed_points():
    tx = np.arange(5 * 3 * 3, dtype=np.float32).reshape(3, 5, 3)          # texel (x, y) holds 3 * (5 y + x) + channel
    pts = [  # uv, the cell under repeat, clamp, black (white alike)
        ((0.5, 0.5), 7, 7, 7), ((0.1, 0.5), 5, 5, R.BLACK), ((0.0, 0.0), 0, 0, R.BLACK), ((0.25, 0.0), 1, 1, 1),
        ((1.0, 0.5), 5, 9, R.BLACK), ((-0.1, 0.5), 9, 5, R.BLACK), ((0.5, -0.1), 12, 2, R.BLACK), ((0.5, 1.0), 2, 12, R.BLACK),
        ((-1.1, -0.4), 9, 0, R.BLACK), ((2.3, 1.4), 6, 14, R.BLACK), ((0.2, 0.34), 6, 6, 6), ((0.199, 0.33), 0, 0, R.BLACK)]
    for dtype in (np.float32, np.float64):
        for (x, y), rep, cl, bl in pts:
            ux, uy = np.float32([x]), np.float32([y])
            got = [int(R.lookup(R.Bmp(tx, w), ux, uy, dtype)[0]) for w in range(4)]
            assert got == [rep, cl, bl, R.WHITE if bl == R.BLACK else bl], ((x, y), got)
    assert np.array_equal(R.value(R.Bmp(tx), [7, R.BLACK, R.WHITE]), np.float32([[21, 22, 23], [0, 0, 0], [1, 1, 1]]))
    # the transform: the product is rounded before the sum
    t = R.Bmp(tx, 0, 0.3, -0.3, 3.7, -3.7)
    x, y = R.transform(t, np.float32([0.7]), np.float32([0.2]), np.float32)
    assert x[0] == F(F(0.7) * F(3.7)) + F(0.3) and y[0] == F(F(0.2) * F(-3.7)) + F(-0.3)
    # a 1 x 1 bitmap is its texel under repeat and clamp and the constant under black and white: every lookup is in column 0
    one = np.float32([[[0.25, 0.5, 0.75]]])
    uv = np.random.RandomState(2).uniform(-3, 3, (2, 100)).astype(np.float32)
    assert [np.unique(R.lookup(R.Bmp(one, w), uv[0], uv[1], np.float64)).tolist() for w in range(4)] == [[0], [0], [R.BLACK], [R.WHITE]]


def _shared_decisions(mts, name, mutation=None):
    """the decisions of texture `name` on the shared inputs: random records on the floor, the boundary strip, and for the
    identity transform the huge strip"""
    S = mts.scenes
    t = bmp_cases.textures()[name]
    rng = np.random.RandomState(31)
    pos, tri, uv = S.tex_grid_mesh(tex_cases.CELLS)
    prim, u, v = tex_cases.triangle_records(rng, 0, len(tri), 4096)
    out = [R.decide_triangles(t, uv, tri, prim, u, v, mutation)]
    strips = [bmp_cases.boundary_strip()] + ([bmp_cases.huge_strip()] if name.endswith("/id") else [])
    for pos, tri, uv in strips:
        z = np.zeros(len(tri), dtype=np.float32)
        out.append(R.decide_triangles(t, uv, tri, np.arange(len(tri)), z, z, mutation))
    return out


@pytest.mark.parametrize("name", sorted(bmp_cases.textures()))
def test_restatement_agrees_with_its_mirror(mts, name):
    t = bmp_cases.textures()[name]
    ds = _shared_decisions(mts, name)
    floor = ds[0]
    assert floor.uv32.min() < -0.5 and floor.uv32.max() > 0.5, "the texcoords reach below zero"
    for d in ds:
        keep = ~d.fragile
        assert np.array_equal(d.cell32[keep], d.cell64[keep]) and np.array_equal(bits(d.value32[keep]), bits(d.value64[keep]))
    assert floor.fragile.mean() <= tex_cases.MAX_FRAGILE
    if t.wrap == R.REPEAT and not name.endswith("/id"):
        assert len(np.unique(floor.cell32)) == t.width * t.height, "every texel is drawn"
    elif t.wrap in (R.REPEAT, R.CLAMP) and t.width * t.height > 1:
        assert len(np.unique(floor.cell32)) > 1
    elif t.width > 1:
        assert (floor.cell32 < 0).any() and (floor.cell32 >= 0).any(), "the constant and texels both occur"
    if name.endswith("/id"):
        # nothing is rounded before the product with the size, and on the huge strip that product is exact too
        huge = ds[2]
        assert np.abs(huge.uv32).max() == bmp_cases.HUGE and np.abs(huge.uv32).max() * 16.0 < bmp_cases.CAST_LIMIT
        if (t.width, t.height) == (16, 16):
            assert not huge.fragile.any() and not ds[1].fragile.any()
    sp = tex_cases.sphere_points(np.random.RandomState(5), 4096)
    d = R.decide_sphere(t, tex_cases.SPHERE_CENTER, tex_cases.SPHERE_RADIUS, np.eye(3), sp)
    # (the first twelve points are the poles, the seam and the equator: texel edges by construction)
    assert np.array_equal(d.cell32[~d.fragile], d.cell64[~d.fragile]) and d.fragile[12:].mean() <= tex_cases.MAX_FRAGILE


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_mutations_are_reported(mts, mutation):
    """each mutated restatement disagrees with the mirror on records that are not fragile, for at least one shared texture of
    the wrap modes it touches"""
    # (clamp hides truncation: floor and the cast differ below zero only, and everything there clamps to 0)
    wraps = {"col0_inside": ("black", "white"), "clamp_w": ("clamp",), "c_remainder": ("repeat",),
             "trunc": ("repeat", "black", "white")}.get(mutation, R.WRAP_NAMES)
    reported = {}
    for name in sorted(bmp_cases.textures()):
        size, wrap, tr = name.split("/")
        if wrap not in wraps or size == "1x1":
            continue
        n = 0
        for d in _shared_decisions(mts, name, mutation):
            keep = ~d.fragile
            n += int((bits(d.value32[keep]) != bits(d.value64[keep])).any(axis=1).sum())
        reported[name] = n
    print("%s: %d records reported; textures that report none: %s" % (mutation, sum(reported.values()), [k for k, v in reported.items() if not v]))
    for wrap in wraps:
        assert any(v > 0 for k, v in reported.items() if k.split("/")[1] == wrap), wrap


# --- the inputs of the device's end-to-end comparison ------------------------------------------------------------------
@pytest.mark.parametrize("shape, wrap, transform", bmp_cases.E2E)
def test_end_to_end_inputs_stay_under_the_cap(mts, shape, wrap, transform):
    """uniformly drawn raster positions on the 16 x 16 palette bitmap: the fragile share stays under tex_cases.MAX_FRAGILE, many
    palette entries are met, and under black and white the column-0 constant is"""
    t, entry = bmp_cases.palette_bitmap(wrap, transform)
    pal = bmp_cases.palette()
    assert len({tuple(p) for p in pal.T.reshape(3, -1).tolist()}) == 3 and all(len(set(pal[:, c].tolist())) == len(pal) for c in range(3))
    assert (np.log2(pal) == np.round(np.log2(pal))).all() and not (pal == 1).any()
    geo = (bmp_cases.FloorGeometry if shape == "grid" else bmp_cases.SphereGeometry)(mts, t)
    assert geo.sd.max_depth < geo.sd.rr_depth
    raster = np.random.RandomState(8).uniform(0, tex_cases.E2E_RES, (40000, 2)).astype(np.float32)
    hit = geo.locate(raster)
    cells = hit.cell[hit.hit & ~hit.fragile]
    print("%s / %s: fragile %.3g, hit %.3g, %d distinct cells, constant %.3g" % (shape, R.WRAP_NAMES[wrap], hit.fragile.mean(), hit.hit.mean(),
                                                                             len(np.unique(cells)), (cells < 0).mean()))
    assert hit.fragile.mean() <= tex_cases.MAX_FRAGILE
    assert hit.hit.mean() > 0.4 and len(np.unique(entry.reshape(-1)[cells[cells >= 0]])) >= 8
    if wrap in (R.BLACK_MODE, R.WHITE_MODE):
        assert (cells < 0).mean() > 0.02, "the column-0 constant is seen"


# --- ABI ---------------------------------------------------------------------------------------------------------------
def test_abi_is_unchanged_and_the_exports_exist(mts):
    L, a = mts.lib(), mts.abi
    assert L.mtsgpu_abi_version() == a.ABI_VERSION == 8
    assert [L.mtsgpu_abi_sizeof(i) for i in range(6)] == [288, 172, 184, 72, 96, 48]
    header = open(os.path.join(ROOT, "include", "mtsgpu.h")).read()
    declared = set(re.findall(r"\b(mtsgpu_[a-z0-9_]+)\s*\(", header))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_EXPORTS:
        assert name in declared and name in mts.EXPORTS and hasattr(L, name), name
        assert name in doc, name
    assert C.sizeof(a.UvTexture) == 48 and a.UvTexture.line_width.offset == 44 and a.UvTexture.bright.offset == 20
    assert C.sizeof(a.Bitmap) == 24 and a.Bitmap.texels.offset == 16
    assert "#define MTSGPU_ABI_VERSION 8" in header and "MTSGPU_TEX_CHECKERBOARD = 0, MTSGPU_TEX_GRID = 1" in header
    assert "MTSGPU_TEX_BITMAP = 2" in header and "MTSGPU_TEX_NKINDS = 2" in header
    assert "MTSGPU_WRAP_REPEAT = 0, MTSGPU_WRAP_CLAMP = 1, MTSGPU_WRAP_BLACK = 2, MTSGPU_WRAP_WHITE = 3" in header
    assert "#define MTSGPU_BITMAP_MAX_TEXELS %du" % a.BITMAP_MAX_TEXELS in header
    assert (a.TEX_BITMAP, a.WRAP_REPEAT, a.WRAP_CLAMP, a.WRAP_BLACK, a.WRAP_WHITE) == (2, 0, 1, 2, 3)
