"""The camera on the CPU: the product's mtsgpu_make_camera / _crop / _ortho against form A of tests/ref64_camera.py, form A
against form B, and the oracle's camera_generate_ray (orc_camera_rays) pushed through the check the device rows go through
in tests/test_gpu_camera_truth.py.  The quantity asserted is worst |error| / bound <= 1 against the binary64 restatement,
the bound being the first-order one the restatement derives per value; the figures are printed and kept in LABNOTES.md
(oracle: configure <= 0.40, rays 0.18 perspective, 0.76 orthographic, 0.75 thin lens; properties <= 0.76).  No sample is
excluded: where binary32 takes another branch of the concentric map than binary64 (8 of the 105 lens samples) the bound
covers both."""
import os

import numpy as np
import pytest

import camera_cases as cc
import ref64_camera as rc

_TRUTH = {}


def _truth(c):
    if c["name"] not in _TRUTH:
        _TRUTH[c["name"]] = cc.truth(c)
    return _TRUTH[c["name"]]


def _oracle_rows(orc, mts, c, mutate=None):
    """the oracle's rows for the case's direct samples, the mirror's rows and branches, and the samples the (possibly
    altered) restatement expects"""
    pix, draws = cc.direct_requests(c)
    raster, lens = cc.samples_of(c, pix, draws)
    rows = orc.camera_rays(cc.oracle_camera(orc, c), np.concatenate([raster, lens], axis=1))
    mrows, branches = rc.mirror(cc.product_camera(mts, c).c, raster, lens, cc.sincos_of(orc))
    return rows, mrows, branches, cc.samples_of(c, pix, draws, mutate)


# --- 1. configure ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", cc.FAMILIES)
def test_make_camera_inside_form_a(mts, orc, family):
    """every entry of rasterToCamera and cameraToWorld inside its bound, entries that are zero by construction equal, the
    scalar fields equal; the product (mtsgpu_make_camera, _crop, _ortho) and the oracle alike"""
    worst = 0.0
    for c in cc.cases(family):
        T = _truth(c)
        pc = cc.product_camera(mts, c).c
        w = rc.check_configure(T, pc)
        assert w <= 1.0, (c["name"], w)
        assert rc.check_configure(T, cc.oracle_camera(orc, c)) <= 1.0, c["name"]
        assert (pc.width, pc.height) == cc.size(c) and (pc.crop_offset_x, pc.crop_offset_y) == cc.offset(c)
        assert (pc.film_width, pc.film_height) == (c["film"] if c["crop"] else (0, 0))
        worst = max(worst, w)
    print("configure, %s: worst error / bound %.3f over %d cameras" % (family, worst, len(cc.cases(family))))


def test_forms_a_and_b_agree():
    """the matrices of the reference and the camera's geometry give the same ray through every raster point: the film's
    corners, its centre, the corners of the crop window and of the border, arbitrary points"""
    worst = 0.0
    for c in cc.cases():
        (W, H), (w, h), (ox, oy), b = c["film"], cc.size(c), cc.offset(c), c["border"]
        pts = [(0, 0), (W, 0), (0, H), (W, H), (W / 2.0, H / 2.0), (ox - b, oy - b), (ox + w + b, oy + h + b), (3.25, 17.5), (W - 0.125, 0.0625)]
        d = rc.forms_disagreement(_truth(c), np.array(pts, dtype=np.float64))
        assert d <= rc.AGREE, (c["name"], d)
        worst = max(worst, d)
    print("forms A and B: worst disagreement %.2e" % worst)


# --- 2. the oracle's rays ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", cc.FAMILIES)
def test_oracle_rays(mts, orc, family):
    worst, worst_prop, differ, total = 0.0, 0.0, 0, 0
    for c in cc.cases(family):
        T = _truth(c)
        rows, mrows, branches, (raster, lens) = _oracle_rows(orc, mts, c)
        assert cc.same_bits(rows[:, :8], mrows), c["name"]                  # the float32 mirror, bit for bit
        w, k = rc.check(T, rows, branches, raster, lens)
        val, bnd, _ = rc.generate(T, branches, raster, lens)
        assert rc.ratio(rows, val, bnd).shape == (len(raster), 8)           # every value of every sample takes part
        p = rc.properties(T, rows, bnd, raster, lens)
        assert w <= 1.0 and p <= 1.0, (c["name"], w, p)
        worst, worst_prop, differ, total = max(worst, w), max(worst_prop, p), differ + k, total + len(raster)
    print("oracle rays, %s: worst error / bound %.3f, properties %.3f, %d of %d samples with a differing branch, 0 excluded"
          % (family, worst, worst_prop, differ, total))
    if family == "thinlens":
        assert differ > 0                    # the lens samples do reach a border of the concentric map


def test_lens_samples_reach_every_branch():
    L = cc.lens_samples()
    r1, r2 = np.float32(2) * L[:, 0] - np.float32(1), np.float32(2) * L[:, 1] - np.float32(1)
    reg = rc._disk_region(r1, r2)
    assert sorted(set(reg.tolist())) == [0, 1, 2, 3, 4]
    assert (r1 == r2).any() and (r1 == -r2).any()
    assert ((L == 0) | (L == 1)).any(axis=1).sum() >= 8


# --- 3. mutations ------------------------------------------------------------------------------------------------------------------
_WHERE = {"fov_larger_side": ("perspective", "ortho"), "aspect_branch_swapped": ("perspective", "ortho"),
          "y_not_flipped": ("perspective", "ortho"), "x_mirrored": ("perspective", "ortho"), "full_angle": ("perspective",),
          "crop_aspect": ("crop",), "crop_offset_dropped": ("crop",), "border_offset_dropped": ("border",),
          "near_far_exchanged": ("perspective",), "invz_omitted": ("perspective",), "focal_along_ray": ("thinlens",),
          "lens_raster_exchanged": ("thinlens",), "disk_regions_exchanged": ("thinlens",), "aperture_not_scaled": ("thinlens",),
          "ortho_maxt_far": ("ortho",), "ortho_origin_no_scale": ("ortho",)}


def test_every_mutation_is_listed():
    assert sorted(_WHERE) == sorted(rc.MUTATIONS) and len(rc.MUTATIONS) == 16


@pytest.mark.parametrize("mutation", rc.MUTATIONS)
def test_mutation_is_reported(mts, orc, mutation):
    """the restatement altered in one place disagrees with the oracle's rows beyond the unchanged bound"""
    ratios = {}
    for family in _WHERE[mutation]:
        for c in cc.cases(family)[::2 if family in ("perspective", "ortho") else 1]:
            rows, _, branches, (raster, lens) = _oracle_rows(orc, mts, c, mutation)
            ratios[c["name"]] = rc.check(cc.truth(c, mutation), rows, branches, raster, lens, mutation)[0]
    caught = [n for n, r in ratios.items() if r > 1.0]
    print("%s: reported on %d of %d cases, smallest ratio where reported %.3g"
          % (mutation, len(caught), len(ratios), min([ratios[n] for n in caught], default=0.0)))
    assert caught, ratios


# --- 4. the properties discriminate ---------------------------------------------------------------------------------------------
def test_properties_report_a_wrong_ray(mts, orc):
    c = cc.cases("thinlens")[0]
    T = _truth(c)
    rows, _, branches, (raster, lens) = _oracle_rows(orc, mts, c)
    _, bnd, _ = rc.generate(T, branches, raster, lens)
    assert rc.properties(T, rows, bnd, raster, lens) <= 1.0
    # a direction too long, mint and maxt off their planes, an origin outside the lens plane: each a thousand times the
    # largest bound of its column
    for cols, axis in (((4, 5, 6), None), ((3,), None), ((7,), None), ((0, 1, 2), 2)):
        bad = rows.copy()
        if axis is None:
            bad[:, cols] *= np.float32(1 + 1e3 * (bnd[:, cols] / np.abs(rows[:, cols]).max()).max())
        else:
            bad[:, axis] += np.float32(1e3 * bnd[:, cols].max())             # along z: the view direction of this pose
        assert rc.properties(T, bad, bnd, raster, lens) > 1.0, cols
    c = cc.cases("perspective")[1]
    T = _truth(c)
    rows, _, branches, (raster, lens) = _oracle_rows(orc, mts, c)
    _, bnd, _ = rc.generate(T, branches, raster, lens)
    bad = rows.copy(); bad[:, 1] += np.float32(1e3 * max(bnd[:, 1].max(), 1e-7))      # a pinhole origin off the camera position
    assert rc.properties(T, rows, bnd, raster, lens) <= 1.0 < rc.properties(T, bad, bnd, raster, lens)


# --- 5. ABI --------------------------------------------------------------------------------------------------------------------------
def test_abi_surface(mts):
    L, a = mts.lib(), mts.abi
    assert L.mtsgpu_abi_version() == a.ABI_VERSION == 8             # a new entry point, no structure changed
    for which, typ in enumerate([a.Scene, a.Camera, a.Stats, a.Mesh, a.SceneDesc, a.KdParams]):
        assert L.mtsgpu_abi_sizeof(which) == __import__("ctypes").sizeof(typ)
    assert mts.EXPORTS[-1] == "mtsgpu_camera_rays" and len(mts.EXPORTS) == len(set(mts.EXPORTS)) == 94
    assert hasattr(L, "mtsgpu_camera_rays") and a.CAMERA_RAY_FLOATS == 14
    root = os.path.dirname(os.path.dirname(os.path.abspath(mts.__file__)))
    header = open(os.path.join(root, "include", "mtsgpu.h")).read()
    assert "int  mtsgpu_camera_rays(mtsgpu_ctx *ctx, const int32_t *pix_samples, uint32_t first, uint32_t n, float *out);" in header
    assert "int  mtsgpu_pass_samples(mtsgpu_ctx *ctx, uint32_t first, uint32_t n, float *out);" in header
    assert "mtsgpu_camera_rays" in open(os.path.join(root, "INTEGRATION.md")).read()
