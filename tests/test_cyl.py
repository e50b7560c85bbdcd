"""The cylinder shape on the CPU: the constructors, getAABB / getClippedAABB of the kd-tree builder, the flattener, the
refusals and the ABI, against the binary32 mirror and the binary64 truth of tests/ref64_cyl.py.  The device side is
tests/test_gpu_cyl.py.

Bounds, from the number format and the operation counts, not from what the code returns:
  * t of a ray: K_GEOM first-order bounds, the figure every other shape is held to (tests/geom_cases.py).
  * a clipped box: a coordinate is the end of a chain of at most 64 binary32 operations on values no larger than the scene's
    largest coordinate S, through one quadratic whose roots the cells below keep away from tangency (amplification <= 4):
    256 x 2^-23 x S.  The sampled surface adds half the diagonal of a grid cell.
What the sampled truth of a clipped box is: Cylinder::getClippedAABB cuts the INFINITE cylinder with the faces of
(getAABB() clipped to the cell) (cylinder.cpp:340-341), so the box must CONTAIN every point of the finite surface inside the
cell (what the tree needs) and must not EXCEED the extent of the infinite surface inside (getAABB() clipped to the cell)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cyl_cases as CC
import ref64_cyl as R
from geom_cases import K_GEOM
from ref64 import EPS32

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _blocks(mts):
    out = {name: mts.cylinder_configure(mts.scenes.CylinderDesc(p1, p2, r)) for name, p1, p2, r in CC.POSES}
    out["sheared"] = mts.cylinder_configure(mts.scenes.CylinderDesc(to_world=CC.SHEARED))
    return out


# --- 1. the constructors ---------------------------------------------------------------------------------------------
def test_configure_equals_the_mirror_and_binary64(mts):
    for name, p1, p2, r in CC.POSES:
        got = mts.cylinder_configure(mts.scenes.CylinderDesc(p1, p2, r))
        assert np.array_equal(bits(got), bits(R.configure_points32(p1, p2, r))), name
        # binary64: an orthonormal frame whose third column is the axis, p1 the origin, the inverse the inverse
        o2w, w2o = got[0:12].astype(np.float64).reshape(3, 4), got[12:24].astype(np.float64).reshape(3, 4)
        p1d, p2d = np.float32(p1).astype(np.float64), np.float32(p2).astype(np.float64)
        length = np.linalg.norm(p2d - p1d)
        S = max(1.0, np.abs(p1d).max(), np.abs(p2d).max())
        tol = 16 * EPS32 * S                                 # sqrt, reciprocal, three products and two sums per entry, doubled
        assert abs(got[25] - length) <= tol and got[24] == F(r)
        assert np.abs(o2w[:, 2] - (p2d - p1d) / length).max() <= tol and np.abs(o2w[:, 3] - p1d).max() == 0
        assert np.abs(o2w[:, :3].T @ o2w[:, :3] - np.eye(3)).max() <= tol
        full = lambda m: np.vstack([m, [0, 0, 0, 1]])
        assert np.abs(full(w2o) @ full(o2w) - np.eye(4)).max() <= 4 * tol
        assert abs(got[26] * (2 * np.pi * got[24] * got[25]) - 1) <= 8 * EPS32
    got = mts.cylinder_configure(mts.scenes.CylinderDesc(to_world=CC.SHEARED))
    assert np.array_equal(bits(got), bits(R.configure_toworld32(CC.SHEARED)))
    assert not np.array_equal(bits(got), bits(R.configure_toworld32(CC.SHEARED, keep_scale=True)))       # mutation: the scale not removed
    m = CC.SHEARED.astype(np.float64)
    o2w, w2o = got[0:12].astype(np.float64).reshape(3, 4), got[12:24].astype(np.float64).reshape(3, 4)
    tol = 64 * EPS32                                         # Gauss-Jordan on a 4 x 4 with entries <= 2, condition number < 8
    assert abs(got[24] - np.linalg.norm(m[:3, 0])) <= 4 * EPS32 and abs(got[25] - np.linalg.norm(m[:3, 2])) <= 8 * EPS32
    want = m[:3] @ np.diag([1 / np.linalg.norm(m[:3, 0]), 1 / np.linalg.norm(m[:3, 0]), 1 / np.linalg.norm(m[:3, 2]), 1])
    assert np.abs(o2w - want).max() <= tol
    assert np.abs(np.vstack([w2o, [0, 0, 0, 1]]) @ np.vstack([o2w, [0, 0, 0, 1]]) - np.eye(4)).max() <= tol
    assert abs(np.linalg.norm(o2w[:, 0]) - 1) <= tol and abs(np.linalg.norm(o2w[:, 2]) - 1) <= tol      # the scale is gone


def test_configure_refusals(mts):
    cd = mts.scenes.CylinderDesc
    bad = [(cd((0, 0, 0), (0, 0, 1), 0.0), "radius > 0"), (cd((0, 0, 0), (0, 0, 1), -1.0), "radius > 0"),
           (cd((1, 2, 3), (1, 2, 3), 0.5), "length > 0"), (cd((0, 0, np.nan), (0, 0, 1), 0.5), "non-finite"),
           (cd((0, 0, 0), (0, 0, 1), np.inf), "non-finite"), (cd(to_world=np.zeros((4, 4))), "0 0 0 1"),
           (cd(to_world=np.diag([1.0, 1.0, 0.0, 1.0])), "singular"), (cd(to_world=np.diag([np.nan, 1, 1, 1])), "non-finite")]
    persp = np.eye(4); persp[3, 2] = 0.1
    bad.append((cd(to_world=persp), "0 0 0 1"))
    for c, why in bad:
        with pytest.raises(mts.MtsGpuError, match=why):
            mts.cylinder_configure(c)
    s = mts.scenes.CylinderDesc((0, 0, 0), (0, 0, 1), 0.5).to_struct(); s.form = 7
    with pytest.raises(mts.MtsGpuError, match="unknown cylinder form"):
        mts.cylinder_configure(s)


# --- 2. rays: the mirror against binary64 (the device is held to the mirror bit for bit in the GPU suite) -----------------
@pytest.fixture(scope="module")
def ray_set(mts):
    block = mts.cylinder_configure(mts.scenes.CylinderDesc((0, 0, -1), (0, 0, 1), 0.5))
    rays = CC.random_rays(block, 200000, seed=3, mint=1e-4)
    named = CC.named_rays(block)
    return block, np.concatenate([rays, np.stack([r for r, _ in named.values()])]), named


@pytest.mark.parametrize("shadow", [False, True])
def test_ray_mirror_against_binary64(ray_set, shadow):
    block, rays, named = ray_set
    mint, maxt = rays[:, 3].copy(), rays[:, 7].copy()
    hit, t = R.intersect32(block, rays, mint, maxt, shadow=shadow)
    tr = R.intersect64(block, rays, mint, maxt, shadow=shadow)
    share = tr["fragile"][:200000].mean()
    print("fragile share %.4f %%, hits %.1f %%" % (100 * share, 100 * hit.mean()))
    assert share <= R.FRAGILE_CAP
    dec = ~tr["fragile"]
    assert np.array_equal(hit[dec], tr["hit"][dec]), np.nonzero(dec & (hit != tr["hit"]))[0][:5]
    assert 0.2 < hit[:200000].mean() < 0.9
    if not shadow:
        sel = dec & hit
        ratio = np.abs(t[sel].astype(np.float64) - tr["t"].v[sel]) / (EPS32 * tr["t"].e[sel])
        rel = np.abs(t[sel].astype(np.float64) - tr["t"].v[sel]) / np.abs(tr["t"].v[sel])
        print("t: worst %.3f bounds, worst relative error %.3g, 99.9th percentile %.3g" % (ratio.max(), rel.max(), np.percentile(rel, 99.9)))
        assert ratio.max() <= K_GEOM
        # the second form: the point lies on the tube.  Its own tolerance: the bound of t along the ray plus the rounding of t
        dist, z = R.second_form(block, rays[sel], tr["t"].v[sel])
        assert dist.max() <= 1e-12 and z.min() >= -1e-12 and z.max() <= float(block[25]) + 1e-12
        dist32, _ = R.second_form(block, rays[sel], t[sel])
        assert (dist32 <= (K_GEOM * EPS32 * tr["t"].e[sel] + EPS32 * np.abs(t[sel])) * np.linalg.norm(rays[sel, 4:7], axis=1) + 1e-12).all()
        # the first root of an outside ray, the far root of an inside one
        first = tr["first"][sel]
        assert first.any() and (~first).any()
    for k, (name, (ray, want)) in enumerate(named.items()):
        i = 200000 + k
        if want is not None and not tr["fragile"][i]:
            assert bool(hit[i]) == want and bool(tr["hit"][i]) == want, name
    i = 200000 + list(named).index("inside_looking_out")
    assert hit[i] and not tr["first"][i]


def test_ray_mutations_are_reported(ray_set):
    block, rays, _ = ray_set
    rng = np.random.RandomState(5)
    rays = rays[:50000].copy()
    mint = rays[:, 3].copy()
    # intervals that end near the cylinder: maxt between, before and behind the roots
    maxt = (rng.rand(len(rays)) * 6).astype(np.float32)
    for shadow, mutation in ((True, "anyhit_far_accepted"), (False, "far_before_near"), (False, "near_mint_dropped")):
        r = rays
        if mutation == "near_mint_dropped":          # origins on the surface: the near root is 0 < mint
            h, t = R.intersect32(block, rays, mint, np.full(len(rays), np.inf, dtype=np.float32))
            sel = h
            o = rays[sel, 0:3] + t[sel, None] * rays[sel, 4:7]
            r = rays[sel].copy(); r[:, 0:3] = o
        mn, mx = r[:, 3].copy(), (maxt[:len(r)] if mutation != "near_mint_dropped" else np.full(len(r), np.inf, dtype=np.float32))
        tr = R.intersect64(block, r, mn, mx, shadow=shadow)
        good, tg = R.intersect32(block, r, mn, mx, shadow=shadow)
        bad, tb = R.intersect32(block, r, mn, mx, shadow=shadow, mutation=mutation)
        dec = ~tr["fragile"]
        print(mutation, "fragile share %.4f %%" % (100 * tr["fragile"].mean()))
        assert tr["fragile"].mean() <= R.FRAGILE_CAP, mutation
        assert np.array_equal(good[dec], tr["hit"][dec]), mutation
        differs = dec & ((bad != tr["hit"]) | (False if shadow else (tr["hit"] & bad & (np.abs(tb - tr["t"].v) > K_GEOM * EPS32 * tr["t"].e))))
        assert differs.any(), "the mutation %s goes unreported" % mutation


# --- 3. getAABB and getClippedAABB ------------------------------------------------------------------------------------
def test_aabb_and_clip_hook_equal_the_mirror(mts):
    for name, block in _blocks(mts).items():
        own = mts.cylinder_aabb(block)
        assert np.array_equal(bits(own), bits(R.aabb32(block))), name
        cells = CC.cells(block, own)
        out, valid = mts.cylinder_clip(block, np.stack(list(cells.values())))
        for (cell_name, cell), o, v in zip(cells.items(), out, valid):
            want, wv = R.clipped32(block, cell)
            assert wv == bool(v), (name, cell_name)
            assert np.array_equal(bits(o), bits(want)), (name, cell_name, o, want)


def _extent(points, lo, hi):
    inside = ((points >= lo) & (points <= hi)).all(axis=1)
    p = points[inside]
    return (p.min(axis=0), p.max(axis=0)) if len(p) else None


def _clip_judgement(block, cell, box, valid, finite, infinite, spacing):
    """-> list of complaints about one clipped box against the sampled truth"""
    S = max(np.abs(finite).max(), 1.0)
    tol = 256 * EPS32 * S + spacing
    cell = cell.astype(np.float64); box = box.astype(np.float64)
    out = []
    ext = _extent(finite, cell[:3] + tol, cell[3:] - tol)          # points that are inside whatever binary32 makes of the faces
    if ext is not None:
        if not valid:
            return ["an invalid box although the surface enters the cell"]
        if (ext[0] < box[:3] - tol).any() or (ext[1] > box[3:] + tol).any():
            out.append("the box does not contain the surface inside the cell: %s %s vs %s" % (ext[0], ext[1], box))
    if valid:
        own = R.aabb32(block).astype(np.float64)
        lo, hi = np.maximum(own[:3], cell[:3]), np.minimum(own[3:], cell[3:])
        ext = _extent(infinite, lo - tol, hi + tol)
        if ext is None:
            out.append("a valid box although the surface misses the cell")
        elif (box[:3] < np.maximum(ext[0], lo) - tol).any() or (box[3:] > np.minimum(ext[1], hi) + tol).any():
            out.append("the box exceeds the surface's extent: %s vs %s %s" % (box, ext[0], ext[1]))
    return out


def _infinite_points(block, own):
    """the grid of R.surface_points on the tube extended over the whole of getAABB()"""
    D = np.asarray(block, dtype=np.float64).copy()
    diag = np.linalg.norm(own[3:].astype(np.float64) - own[:3].astype(np.float64))
    ext = D.copy(); ext[25] = D[25] + 2 * diag
    M = D[0:12].reshape(3, 4)
    ext[[3, 7, 11]] = M[:, 3] - diag * M[:, 2]
    return R.surface_points(ext, 512, 1024)


def test_clip_against_the_sampled_surface_and_mutations(mts):
    caught = {"base_clip": 0, "face_pair_missing": 0, "maxima_missing": 0, "if0": 0}
    cases = fragile = 0
    for name, block in _blocks(mts).items():
        if name in CC.AXIS_PARALLEL:
            # every cell is a threshold case (cyl_cases.AXIS_PARALLEL): fragile by construction, held to the mirror alone
            continue
        if name == "sheared":
            # the clip models a circular tube of m_radius around objectToWorld(0, 0, 1): the surface only under a rigid objectToWorld.
            # What remains of a sheared toWorld after the scale is removed is not rigid; that pose is held to the mirror alone
            continue
        own = mts.cylinder_aabb(block)
        finite, spacing = R.surface_points(block, 512, 512)
        infinite, spacing_inf = _infinite_points(block, own)
        spacing = max(spacing, spacing_inf)
        # getAABB: contains the surface, and is tight (the #if 0 variant is not)
        S = max(np.abs(finite).max(), 1.0)
        for variant in (None, "if0"):
            b = R.aabb32(block, variant).astype(np.float64)
            tight = (np.abs(b[:3] - finite.min(axis=0)) <= 64 * EPS32 * S + spacing).all() and (np.abs(b[3:] - finite.max(axis=0)) <= 64 * EPS32 * S + spacing).all()
            if variant is None:
                assert tight, name
            else:
                caught["if0"] += not tight
        cells = CC.cells(block, own)
        out, valid = mts.cylinder_clip(block, np.stack(list(cells.values())))
        for (cell_name, cell), o, v in zip(cells.items(), out, valid):
            R.clipped32(block, cell)
            cases += 1
            if R.CLIP_NOTES["fragile"]:
                fragile += 1
                continue
            assert not _clip_judgement(block, cell, o, bool(v), finite, infinite, spacing), (name, cell_name, _clip_judgement(block, cell, o, bool(v), finite, infinite, spacing))
            for mutation in ("base_clip", "face_pair_missing", "maxima_missing"):
                mo, mv = R.clipped32(block, cell, mutation)
                caught[mutation] += bool(_clip_judgement(block, cell, mo, mv, finite, infinite, spacing))
        assert not valid[list(cells).index("outside")] and not valid[list(cells).index("inside_tube")], name
    print(caught, "cells", cases, "fragile", fragile)
    assert fragile <= R.FRAGILE_CAP * cases
    assert all(caught.values()), caught


# --- 4. the host builder and the flattener ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def flat(mts):
    out = {}
    for name in CC.SCENES:
        sd = CC.scene_description(mts, name)
        out[name] = (sd, mts.Scene(sd, kd_params=CC.kd_params(mts, name, 1)), mts.Scene(sd, kd_params=CC.kd_params(mts, name, 16)))
    return out


def test_host_builder_threads_and_cylinder_coverage(mts, flat):
    """two views of one question, which leaves list a cylinder.  The truth that knows no clip: a leaf the sampled surface enters lists
    it, a leaf farther from the surface than the bound does not.  And, for every pair including those in between (the SAH cuts where
    the clipped boxes end, so a tube touching a cell from outside is the rule), the replay of the builder's classification with the
    mirror's clip (cyl_cases.leaf_membership), which leaves undecided only a box lying IN a split plane: the 1 % cap is on those"""
    total = undecided = 0
    for name, (sd, one, many) in flat.items():
        a, b = CC.tree_words(one), CC.tree_words(many)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), name
        blocks = one.cylinder_blocks()
        prim = 0
        S = max(np.abs(np.array(list(one.sc.aabb_min) + list(one.sc.aabb_max))).max(), 1.0)
        for s, m in enumerate(sd.meshes):
            if m.shape_type != mts.abi.SHAPE_CYLINDER:
                prim += 1 if m.sphere is not None else len(m.triangles)
                continue
            finite, spacing = R.surface_points(blocks[s], 256, 512)
            infinite, sp2 = _infinite_points(blocks[s], mts.cylinder_aabb(blocks[s]))
            tol = 256 * EPS32 * S + max(spacing, sp2)
            for lo, hi, ids, member in CC.leaf_membership(one, blocks[s]):
                total += 1
                if member is None:
                    undecided += 1
                else:
                    assert (prim in ids) == member, (name, s, lo, hi, ids, "the replay of the classification with the mirror's clip")
                enters = ((finite >= lo + tol) & (finite <= hi - tol)).all(axis=1).any()
                d = np.maximum(np.maximum(lo - infinite, infinite - hi), 0.0)
                near = (np.linalg.norm(d, axis=1) <= tol).any()
                if enters or not near:
                    assert (prim in ids) == bool(enters), (name, s, lo, hi, ids)
            prim += 1
    print("leaves x cylinders", total, "undecided", undecided)
    assert total >= 40 and undecided <= R.FRAGILE_CAP * total
    # the thin cylinder: the clip keeps it out of most of the leaves its box touches
    sd, one, _ = flat["thin"]
    listed = sum(64 in ids for _, _, ids in CC.leaves(one))
    own = mts.cylinder_aabb(one.cylinder_blocks()[1]).astype(np.float64)
    touched = sum(bool(((lo <= own[3:]) & (hi >= own[:3])).all()) for lo, hi, _ in CC.leaves(one))
    print("thin: listed in", listed, "of", touched, "leaves its box touches")
    assert listed < 0.6 * touched


@pytest.mark.parametrize("n_threads", [1, 16])
@pytest.mark.parametrize("name", CC.SCENES)
def test_host_trees_hold_the_properties_of_ref64_kd(mts, name, n_threads):
    """coverage, tightness, greedy SAH optimality, termination, the statistics and the enlarged box (tests/ref64_kd.py, imported) on the
    cylinder scenes, with the checker's clip taught Cylinder::getClippedAABB (cyl_cases.kd_clip), under its own caps on fragile cases"""
    import kd_cases as KC
    import ref64_kd as K
    sd, kp = CC.scene_description(mts, name), CC.kd_params(mts, name, n_threads)
    rep, prims = CC.kd_report(K, mts, sd, mts.Scene(sd, kd_params=kp), kp)
    print(name, rep.left_out, rep.share)
    f = KC.failures(rep, "host x %d / %s" % (n_threads, name))
    assert not f, "\n".join(f)
    if name == "thin":
        assert rep.left_out["sah"][1] >= 30 and rep.left_out["tightness"][1] >= 100      # the exact sweep was held on that many nodes
        # the mutation "the clip replaced by the base-class clip": the checker without the cylinder's clip reports this tree
        arrays = {k: mts.Scene(sd, kd_params=kp).arrays()[k] for k in ("kd_nodes", "kd_indices", "aabb_min", "aabb_max")}
        plain = K.check(prims, arrays, K.Params(kp, prims.n))
        assert "sah" in plain.names() or "termination" in plain.names(), plain.names()


def test_flattener(mts, flat):
    A = mts.abi
    sd, sc, _ = flat["mixed"]
    s = sc.sc
    assert s.n_tris == 14 and s.n_shapes == 3 and s.n_verts == 36
    tri = np.ctypeslib.as_array(s.tri_idx, shape=(3 * s.n_tris,)).reshape(-1, 3)
    assert (tri[0] == 0xFFFFFFFF).all() and (tri[1] == 0xFFFFFFFF).all() and (tri[2:] != 0xFFFFFFFF).all()
    ta = np.ctypeslib.as_array(s.triaccel, shape=(12 * s.n_tris,)).reshape(-1, 12)
    assert ta[0, 0] == 0xFFFFFFFF and ta[0, 10] == 0 and ta[1, 10] == 1
    assert list(np.ctypeslib.as_array(s.shape_type, shape=(3,))) == [A.SHAPE_CYLINDER, A.SHAPE_SPHERE, A.SHAPE_TRIMESH]
    blocks = sc.cylinder_blocks()
    assert blocks.shape == (3, A.CYLINDER_NDERIVED) and not blocks[1:].any()
    assert np.array_equal(bits(blocks[0]), bits(mts.cylinder_configure(sd.meshes[0])))
    # the enlarged box of the tree holds the cylinder's own box (skdtree.cpp:62-101, gkdtree.h:1046-1052)
    own = mts.cylinder_aabb(blocks[0])
    assert (np.array(list(s.aabb_min)) < own[:3]).all() and (np.array(list(s.aabb_max)) > own[3:]).all()
    sd1, sc1, _ = flat["one"]
    own = mts.cylinder_aabb(sc1.cylinder_blocks()[0]).astype(np.float32)
    eps = F(1e-4)
    lo = own[:3] - ((own[3:] - own[:3]) * eps + eps)
    assert np.array_equal(bits(np.array(list(sc1.sc.aabb_min), dtype=np.float32)), bits(lo))
    # a scene without a cylinder has no pool
    plain = mts.Scene(mts.scenes.cornell_c1())
    assert plain.cylinder_blocks() is None and not plain.has_cylinders


def test_refusals_at_flatten(mts):
    L, A = mts.lib(), mts.abi
    sd = CC.scene_description(mts, "one")
    desc, keep = sd.to_ctypes()
    h = C.c_void_p()
    kp = A.KdParams()
    # the old calls refuse the type and name the new one
    assert L.mtsgpu_flatten(C.byref(desc), C.byref(kp), C.byref(h)) != 0
    assert b"mtsgpu_flatten_cylinders" in L.mtsgpu_last_error(None)
    tcs = (A.f32p * 1)()
    assert L.mtsgpu_flatten_tangents(C.byref(desc), C.byref(kp), tcs, C.byref(h)) != 0
    assert L.mtsgpu_flatten_tangents_flagged(C.byref(desc), C.byref(kp), tcs, None, C.byref(h)) != 0
    assert L.mtsgpu_flatten_cylinders(C.byref(desc), C.byref(kp), None, None, None, C.byref(h)) != 0
    assert b"mtsgpu_flatten_cylinders" in L.mtsgpu_last_error(None)
    # a cylinder with an area luminaire: the reference cannot render it either
    sd = mts.scenes.SceneDescription("lit")
    lum = sd.add_lum(A.LUM_AREA, [1, 1, 1])
    sd.add_cylinder((0, 0, 0), (0, 0, 1), 0.5, bsdf=sd.lambertian(0.5), lum=lum)
    with pytest.raises(mts.MtsGpuError, match="pdfArea"):
        mts.Scene(sd)
    sd = mts.scenes.SceneDescription("bad")
    sd.add_lum(A.LUM_POINT, [1, 1, 1])
    sd.add_cylinder((0, 0, 0), (0, 0, 1), -0.5, bsdf=sd.lambertian(0.5))
    with pytest.raises(mts.MtsGpuError, match="radius > 0"):
        mts.Scene(sd)


# --- 5. the ABI -------------------------------------------------------------------------------------------------------
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
    assert sorted(mts.CYLINDER_EXPORTS) == _declared("mtsgpu_cylinder.h")
    assert C.sizeof(mts.abi.Cylinder) == 4 + 12 + 12 + 4 + 64
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in mts.CYLINDER_EXPORTS + ["mtsgpu_cylinder.h", "MTSGPU_SHAPE_CYLINDER"]:
        assert name in doc, name
    for name in mts.CYLINDER_EXPORTS:
        assert hasattr(L, name)
