"""The film stage against a binary64 truth that does not go through the oracle (tests/ref64_film.py): the five filter tables
of mtsgpu_tabulate_filter within the restatement's per-entry bound, and the oracle's films (orc.render, orc.render_tiles)
within B = gamma_(n+6) * S of ImageBlock::putSample restated over the oracle's own Li samples.  The same comparison with the
restatement altered in one place at a time must fail: that is what shows the bound discriminates.  CPU only.

Worst observed error / B (information; the bound does not follow from these) are printed by every test and kept in
LABNOTES.md."""
import ctypes as C

import numpy as np
import pytest

import film_cases as fc
import ref64_film as rf

_cache = {}


def _oracle(mts, orc, name):
    """(case, table, scene, camera, params, pixels [n][2], records [n][8]) -- the oracle's Li for every pixel of the crop
    window and every sample; computed once per case"""
    if name in _cache:
        return _cache[name]
    c = fc.case(name)
    sd = fc.scene_of(mts, c)
    fs = orc.FlatScene(sd)
    cam = orc.make_camera(sd, *(fc.FILM if c["crop"] else (c["W"], c["H"])))
    kind = {"independent": mts.abi.SAMPLER_INDEPENDENT_KEYED, "halton": mts.abi.SAMPLER_HALTON}[c["sampler"]]
    kw = dict(integrator="direct", luminaire_samples=2, bsdf_samples=2) if c["integrator"] == "direct" else {}
    prm = orc.render_params(fc.MAX_DEPTH, sampler=kind, spp=c["spp"], seed=fc.SEED, **kw)
    x0, y0 = fc.CROP[:2] if c["crop"] else (0, 0)
    ys, xs, js = np.meshgrid(np.arange(y0, y0 + c["H"]), np.arange(x0, x0 + c["W"]), np.arange(c["spp"]), indexing="ij")
    ps = np.stack([xs.ravel(), ys.ravel(), js.ravel()], axis=1).astype(np.uint32)
    rec = orc.li_samples(fs.scene, cam, prm, ps)
    _cache[name] = (c, fc.filter_table(mts, c), fs, cam, prm, ps[:, :2].astype(np.int64), rec)
    return _cache[name]


def _tabfilter(orc, table):
    f = orc.TabFilter()
    f.size_x, f.size_y = float(table[0]), float(table[1])
    for y in range(16):
        for x in range(16):
            f.values[y][x] = float(table[2][y, x])
    return f


def _oracle_film(orc, name, c, table, fs, cam, prm, part=0, n_parts=1):
    if c["filter"][0] == "box" and n_parts == 1:
        if c["crop"]:
            x0, y0 = fc.CROP[:2]
            return orc.render(fs.scene, cam, prm, rect=(x0, y0, x0 + c["W"], y0 + c["H"]))[0][y0:y0 + c["H"], x0:x0 + c["W"]]
        return orc.render(fs.scene, cam, prm)[0]
    return orc.render_tiles(fs.scene, cam, prm, _tabfilter(orc, table), block_size=c["bs"], part=part, n_parts=n_parts)[0]


# --- 1. tables -------------------------------------------------------------------------------------------------------------
TABLES = [("box", None, None, None), ("gaussian", None, None, None), ("gaussian", 2.5, 0.7, None), ("mitchell", None, None, None),
          ("mitchell", 1.75, 0.2, 0.6), ("catmullrom", None, None, None), ("catmullrom", 2.5, None, None),
          ("wsinc", None, None, None), ("wsinc", 2.5, 2.0, None)]


def _table_ratio(mts, kind, hs, p0, p1, mutate=None):
    c = dict(filter=(kind, hs, p0, p1))
    sx, sy, got = fc.filter_table(mts, c)
    rx, ry, val, bound = rf.tabulate(kind, hs, p0, p1, mutate=mutate)
    assert (float(sx), float(sy)) == (rx, ry)
    assert (got[15, :] == 0).all() and (got[:, 15] == 0).all()
    err = np.abs(got.astype(np.float64) - val)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0, 0.0, err / bound)


@pytest.mark.parametrize("kind,hs,p0,p1", TABLES)
def test_filter_table_within_the_restatements_bound(mts, kind, hs, p0, p1):
    """mtsgpu_tabulate_filter, defaults and one non-default parameter set per plugin; the oracle's tables are asserted
    bit-equal to these elsewhere.  Worst error / bound observed: box 0, gaussian 0.09, mitchell 0.07, catmullrom 0.04,
    wsinc 0.27"""
    r = _table_ratio(mts, kind, hs, p0, p1)
    print("table %s %s: worst error / bound %.3f" % (kind, (hs, p0, p1), r.max()))
    assert (r <= 1.0).all(), (kind, np.unravel_index(r.argmax(), r.shape), r.max())


@pytest.mark.parametrize("kind", rf.KINDS)
def test_a_smooth_factor_on_the_filter_function_is_reported(mts, kind):
    """the function times 1 + 0.05 r before normalisation survives "integrates to one"; not the per-entry bound"""
    r = _table_ratio(mts, kind, None, None, None, mutate="radial")
    print("table %s with the function times 1 + 0.05 r: worst error / bound %.0f" % (kind, r.max()))
    assert r.max() > 1.0


# --- 2. the oracle's film ----------------------------------------------------------------------------------------------------
ORACLE_FILMS = ["box_independent", "box_halton", "box_wave", "box_crop", "gaussian_bs8", "mitchell_bs8", "catmullrom_bs8", "wsinc_bs8",
                "gaussian_bs16", "asymmetric"]


@pytest.mark.parametrize("name", ORACLE_FILMS)
def test_oracle_film_within_the_bound(mts, orc, name):
    c, table, fs, cam, prm, pix, rec = _oracle(mts, orc, name)
    geom = fc.geometry(rf, c, table[0], table[1])
    res = fc.restate(rf, geom, table, rec, pix)
    film = _oracle_film(orc, name, c, table, fs, cam, prm)
    w = fc.worst(res, film)
    print("oracle film %s: worst error / B %.3f, fragile taps %d of %d" % (name, w, res.fragile, res.taps))
    assert w <= 1.0
    assert (rec[:, 3] == 0).any() and (rec[:, 3] == 1).any() and np.nanmax(rec[:, :3]) > 5 * np.nanmedian(rec[:, :3][rec[:, :3] > 0])
    if name == "box_halton":
        assert np.array_equal(film[..., 4], np.full((c["H"], c["W"]), c["spp"] - 1, dtype=np.float32))     # sample 0 sits on the corner


def test_oracle_tile_parts_summed(mts, orc):
    """two parts: each part's film against the restatement of that part's samples, and their binary32 sum against the whole"""
    c, table, fs, cam, prm, pix, rec = _oracle(mts, orc, "gaussian_bs8")
    geom = fc.geometry(rf, c, table[0], table[1])
    t = geom.tile_of(pix)
    part = rf.morton(t[:, 0], t[:, 1]) % 2
    acc = np.zeros((c["H"], c["W"], 5), dtype=np.float32)
    for k in range(2):
        film = _oracle_film(orc, "gaussian_bs8", c, table, fs, cam, prm, part=k, n_parts=2)
        w = fc.worst(fc.restate(rf, geom, table, rec[part == k], pix[part == k]), film)
        print("oracle part %d of 2: worst error / B %.3f" % (k, w))
        assert w <= 1.0
        acc += film
    w = fc.worst(fc.restate(rf, geom, table, rec, pix), acc, extra=1)
    print("oracle parts summed: worst error / B %.3f" % w)
    assert w <= 1.0


# --- 3. mutations --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutate,name", [("no_half", "gaussian_bs8"), ("factor16", "gaussian_bs8"), ("round_index", "gaussian_bs8"),
                                         ("foreign_samples", "gaussian_bs8"), ("weight_needs_alpha", "gaussian_bs8"),
                                         ("transposed", "asymmetric"),
                                         ("no_half", "box_independent"), ("factor16", "box_independent"), ("round_index", "box_independent"),
                                         ("weight_needs_alpha", "box_independent")])
def test_an_altered_restatement_is_reported(mts, orc, mutate, name):
    c, table, fs, cam, prm, pix, rec = _oracle(mts, orc, name)
    geom = fc.geometry(rf, c, table[0], table[1])
    film = _oracle_film(orc, name, c, table, fs, cam, prm)
    r = fc.restate(rf, geom, table, rec, pix, mutate=mutate).ratio(film)
    print("%s on %s: %d of %d values outside the bound, worst error / B %.3g" % (mutate, name, (r > 1).sum(), r.size, r.max()))
    assert (r > 1.0).any()


def test_a_larger_border_is_reported_by_the_rendered_rectangle(mts, orc):
    """border = ceil(size) instead of ceil(size - 0.5) cannot change a film value (ref64_film's docstring): it changes the
    rectangle highQualityEdges renders.  The asymmetric filter (2.5: border 2, not 3) on a 20 x 12 film"""
    sd = mts.scenes.envlit()
    fs = orc.FlatScene(sd); cam = orc.make_camera(sd, 20, 12)
    prm = orc.render_params(1, spp=1, seed=fc.SEED)
    table = fc.asymmetric_table()
    _, st = orc.render_tiles(fs.scene, cam, prm, _tabfilter(orc, table), block_size=8, hq_edges=True)
    c = dict(fc.case("asymmetric"), W=20, H=12, hq=True)
    good = fc.geometry(rf, c, table[0], table[1]); bad = fc.geometry(rf, c, table[0], table[1], mutate="border_ceil")
    assert good.border == 2 and bad.border == 3
    assert st.camera_samples == good.size[0] * good.size[1] == 24 * 16
    assert st.camera_samples != bad.size[0] * bad.size[1]


# --- 4. the cap on fragile taps ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(fc.CASES))
def test_fragile_taps_are_rare(mts, orc, name):
    """at most 1 in 1000 taps may be decided differently by binary32 and binary64, for every configuration of this file and
    of test_gpu_film_truth.py, on the oracle's samples (with highQualityEdges: those of the film's own pixels, which is all
    the oracle hands out)"""
    c, table, fs, cam, prm, pix, rec = _oracle(mts, orc, name)
    res = fc.restate(rf, fc.geometry(rf, c, table[0], table[1]), table, rec, pix)
    print("%s: %d fragile of %d taps" % (name, res.fragile, res.taps))
    assert res.taps > 0 and res.fragile <= fc.MAX_FRAGILE * res.taps


# --- 5. the restatement itself -------------------------------------------------------------------------------------------------
def _synthetic(geom, spp, seed):
    rng = np.random.RandomState(seed)
    pix = np.repeat(geom.rendered_pixels(), spp, axis=0)
    xy = (pix + rng.rand(len(pix), 2)).astype(np.float32)
    xy = np.minimum(xy, np.nextafter((pix + 1).astype(np.float32), np.float32(-np.inf)))      # stays inside its pixel
    rec = np.zeros((len(pix), 8), dtype=np.float32)
    rec[:, :4] = 1.0; rec[:, 4:6] = xy
    return pix, rec


@pytest.mark.parametrize("kind", ["gaussian", "mitchell", "wsinc", "table"])
def test_constant_radiance_with_high_quality_edges_develops_to_one(mts, kind):
    """Li = 1, alpha = 1 over the grown rectangle: rgb / weight and alpha / weight are 1 in every film pixel, to B, and every
    pixel of the film -- its edge included -- has the weight of an interior pixel's full filter support to within the noise
    of 16 jittered samples"""
    c = dict(fc.case("gaussian_hq"), filter=(kind,), W=21, H=13)
    table = fc.filter_table(mts, c)
    geom = fc.geometry(rf, c, table[0], table[1])
    pix, rec = _synthetic(geom, 16, 4)
    res = fc.restate(rf, geom, table, rec, pix)
    B = res.bound()
    for ch in range(4):
        assert (np.abs(res.T[..., ch] - res.T[..., 4]) <= B[..., ch]).all()
    assert (res.T[..., 4] > 0).all()
    assert abs(res.T[0, :, 4].mean() / res.T[6, :, 4].mean() - 1) < 0.1 and abs(res.T[:, 0, 4].mean() / res.T[:, 10, 4].mean() - 1) < 0.1


def test_invalid_samples_are_dropped_whole(mts):
    """Spectrum::isValid (imageblock.h:85-88): a NaN or negative channel drops the sample -- radiance, alpha and weight -- and
    the input flag alone decides; a synthetic list, since no legal scene yields such a sample"""
    c = dict(fc.case("gaussian_bs8"), W=21, H=13)
    table = fc.filter_table(mts, c)
    geom = fc.geometry(rf, c, table[0], table[1])
    pix, rec = _synthetic(geom, 4, 5)
    clean = fc.restate(rf, geom, table, rec, pix)
    bad = rec.copy()
    bad[3::7, 0] = np.nan; bad[5::11, 2] = -1.0
    ok = rf.is_valid(bad[:, :3])
    assert 0 < (~ok).sum() < len(ok) / 3 and not ok[3] and not ok[5] and ok[0]
    dropped = fc.restate(rf, geom, table, bad, pix)
    kept = fc.restate(rf, geom, table, rec[ok], pix[ok])
    for a in ("T", "S", "lo", "hi"):
        assert np.array_equal(getattr(dropped, a), getattr(kept, a))
    assert np.array_equal(dropped.n, kept.n) and (dropped.T[..., 4] < clean.T[..., 4]).any() and np.isfinite(dropped.T).all()
    # the rule, not the values, decides: flagged valid, the same records poison the sums
    assert not np.isfinite(fc.restate(rf, geom, table, bad, pix, valid=np.ones(len(bad), dtype=bool)).T).all()
