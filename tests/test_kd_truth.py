"""The kd-tree builders held to tests/ref64_kd.py, a binary64 truth that is not a builder: the oracle's builder
(oracle/orc_kdtree.c, until now pinned by nothing) and the host builder (csrc/kdbuild.cpp, one thread and sixteen) over every
scene x parameter set of tests/kd_cases.py, through all six properties; the planted errors, each of which the checker must
name; hand-built trees whose optimum is known by inspection; and the checker's clip against the oracle's, bit for bit.
The device phases go through the same check in test_gpu_kd_truth.py.

Derived bounds (ref64_kd's docstring has the operation counts): eps(P) = 51 x 2^-53 x M x perimeter / area for the coverage of
a triangle, at most 5.4e-6 over these scenes (the slivers); TAU = 2 gamma_17 = 2.03e-6 for a cost ratio of the exact sweep,
2 gamma_(17 + minMaxBins) for the min-max phase; gamma_(n + 6) for a statistic summed over n nodes.

Measured over the oracle's and the host's trees (the same trees word for word, test_host.py) as shares of those bounds:
coverage deficit / eps 0.0067; cost ratio of the exact sweep / TAU 0.024 (fuzz_0, empty_space_bonus 0.5); of the min-max
phase 1.3e-9; statistics 0.26 (spheres, max_depth 3).  Fragile shares against the 1 % cap: coverage 0, tightness 0, sah 0,
termination 1 case of 1181 (0.08 %: twins, exact_prim_threshold 4), minmax 0, stats 0 -- every scene met its caps as named."""
import ctypes as C

import numpy as np
import pytest

import kd_cases as KC
import ref64_kd as K

CASES = [(s, p) for s in KC.SCENES for p in KC.PARAMS]
WORST = {}
# the measured shares of the docstring above; the test holds the trees to four times each, so the figures bind and go stale
# loudly (the derived bound itself is a share of 1).  The min-max excess is binary64 noise about a zero: held below 1e-6.
RECORDED = {"coverage_deficit_over_eps": 0.0067, "sah_excess_over_tau": 0.024, "minmax_excess_over_tau": 2.5e-7,
            "stats_error_over_bound": 0.26}


def _note(rep):
    for k, v in rep.share.items():
        WORST[k] = max(WORST.get(k, 0.0), float(v))


@pytest.mark.parametrize("sname,pname", CASES)
def test_oracle_trees_hold_every_property(mts, orc, sname, pname):
    sd, _ = KC.scene(mts, sname)
    rep = KC.report(mts, sname, pname, orc.FlatScene(sd, kd_params=KC.kd_params(mts, pname)))
    _note(rep)
    f = KC.failures(rep, "oracle / %s / %s" % (sname, pname))
    assert not f, "\n".join(f)


@pytest.mark.parametrize("n_threads", [1, 16])
@pytest.mark.parametrize("sname,pname", CASES)
def test_host_trees_hold_every_property(mts, sname, pname, n_threads):
    sd, _ = KC.scene(mts, sname)
    rep = KC.report(mts, sname, pname, mts.Scene(sd, kd_params=KC.kd_params(mts, pname, n_threads=n_threads)))
    _note(rep)
    f = KC.failures(rep, "host x %d / %s / %s" % (n_threads, sname, pname))
    assert not f, "\n".join(f)


def test_measured_shares_of_the_derived_bounds(mts, orc):
    """every measured maximum stays below its derived bound (a share of 1), and the phases were exercised: the figures
    of this module's docstring"""
    for sname, pname in CASES:                              # shared with the tests above when they ran first
        sd, _ = KC.scene(mts, sname)
        _note(KC.report(mts, sname, pname, orc.FlatScene(sd, kd_params=KC.kd_params(mts, pname))))
    print("worst shares", WORST)
    for k in ("coverage_deficit_over_eps", "sah_excess_over_tau", "minmax_excess_over_tau", "stats_error_over_bound"):
        assert WORST[k] <= 1.0, (k, WORST[k])
        assert WORST[k] <= 4 * RECORDED[k], (k, WORST[k], RECORDED[k])
    assert WORST["coverage_eps_max"] < 1e-5
    assert WORST["bad_refines_max"] == 3                   # some path uses every bad refine the default allows
    n_minmax = sum(KC.report(mts, s, "small_exact", orc.FlatScene(KC.scene(mts, s)[0], kd_params=KC.kd_params(mts, "small_exact")))
                   .left_out["minmax"][1] for s in KC.SCENES)
    assert n_minmax > 1000                                  # the min-max phase was held to its property on that many nodes


# ---------------------------------------------------------------------------------------------------------------------
# planted errors
# ---------------------------------------------------------------------------------------------------------------------
def _built(mts, orc, sname, pname):
    sd, prims = KC.scene(mts, sname)
    flat = orc.FlatScene(sd, kd_params=KC.kd_params(mts, pname))
    return prims, KC.tree_arrays(flat), K.Params(KC.kd_params(mts, pname), prims.n), K.stats_dict(flat.kdstats())


def _with_lists(arrays, edit):
    """a copy of the tree with its leaf lists edited: edit(lists), lists = {leaf node: [indices]}"""
    nodes = arrays["kd_nodes"].copy()
    leaf = (nodes[:, 0] & 0x80000000) != 0
    lists = {int(i): arrays["kd_indices"][int(nodes[i, 0] & 0x7FFFFFFF):int(nodes[i, 1])].tolist() for i in np.nonzero(leaf)[0]}
    edit(lists)
    out = []
    for i in sorted(lists):
        nodes[i] = [0x80000000 | len(out), len(out) + len(lists[i])]
        out += lists[i]
    return dict(arrays, kd_nodes=nodes, kd_indices=np.array(out if out else [0], dtype=np.uint32)[:max(len(out), 1)])


def _with_plane(arrays, node, axis=None, split=None):
    nodes = arrays["kd_nodes"].copy()
    if axis is not None:
        nodes[node, 0] = (nodes[node, 0] & ~np.uint32(3)) | np.uint32(axis)
    if split is not None:
        nodes[node, 1] = np.array([split], dtype=np.float32).view(np.uint32)[0]
    return dict(arrays, kd_nodes=nodes)


def _swapped(arrays, node):
    """the two children of an inner node exchanged (offsets are relative to a node's own place)"""
    nodes = arrays["kd_nodes"].copy()
    l = node + int(nodes[node, 0] >> 2)
    a, b = nodes[l].copy(), nodes[l + 1].copy()
    if not a[0] & 0x80000000:
        a[0] = (a[0] & 3) | (((a[0] >> 2) - 1) << 2)
    if not b[0] & 0x80000000:
        b[0] = (b[0] & 3) | (((b[0] >> 2) + 1) << 2)
    nodes[l], nodes[l + 1] = b, a
    return dict(arrays, kd_nodes=nodes)


def _candidates(prims, tree, params, node):
    boxes = K._NodeBoxes(prims, tree, params, [node])
    _, blo, bhi, kept = boxes.at[node]
    return K._sweep(params, tree.lo[node], tree.hi[node], blo[kept], bhi[kept])[2]


def _mutations(mts, orc):
    """name -> (property that must report it, prims, arrays, params, stats)"""
    out = {}
    prims, arrays, params, stats = _built(mts, orc, "twins", "defaults")
    tree = K.Tree(prims, arrays["kd_nodes"], arrays["kd_indices"], params)
    assert not K.check(prims, arrays, params, stats).names()

    # an index removed from a leaf that the triangle crosses with the largest area
    leaf3 = next(i for i in tree.leaves if len(tree.sets[i]) >= 2)
    held = tree.sets[leaf3]
    V, cnt = K.clip_polygons(prims.tri[prims.tri_of[held]], np.tile(tree.lo[leaf3], (len(held), 1)), np.tile(tree.hi[leaf3], (len(held), 1)))
    victim = int(held[np.argmax(K.polygon_area(V, cnt))])
    out["index_removed"] = ("coverage", prims, _with_lists(arrays, lambda L: L[leaf3].remove(victim)), params, None)

    # a triangle added to a leaf its box misses
    far = next(int(p) for p in range(prims.n) if ((prims.lo[p] > tree.hi[leaf3]) | (prims.hi[p] < tree.lo[leaf3])).any())
    out["triangle_added"] = ("tightness", prims, _with_lists(arrays, lambda L: L[leaf3].append(far)), params, None)

    # the root's plane: moved to the neighbouring candidate, off every candidate, onto another axis; its children swapped
    a, s = int(tree.axis[0]), float(tree.split[0])
    cands = _candidates(prims, tree, params, 0)
    k = int(np.nonzero(cands[a] == s)[0][0])
    neighbour = float(cands[a][k + 1] if k + 1 < len(cands[a]) else cands[a][k - 1])
    out["plane_to_neighbour"] = ("sah", prims, _with_plane(arrays, 0, split=neighbour), params, None)
    between = float(np.float32(0.5 * (s + neighbour)))
    assert not (cands[a] == between).any()
    out["plane_off_candidates"] = ("sah", prims, _with_plane(arrays, 0, split=between), params, None)
    out["axis_changed"] = ("sah", prims, _with_plane(arrays, 0, axis=(a + 1) % 3), params, None)
    out["children_swapped"] = ("coverage", prims, _swapped(arrays, 0), params, None)

    # misreadings of the cost, planted in the checker's parameters: a correct tree must then be reported
    out["bonus_always"] = ("sah", prims, arrays, K.Params(None, prims.n, bonus_always=True), None)
    out["costs_exchanged"] = ("sah", prims, arrays, K.Params(None, prims.n, traversal_cost=20.0, query_cost=15.0), None)
    # a triangle that lies in the plane, listed on the side that is the more likely to be visited
    _, fp, fpar, _, _, dear = _four_trees(mts, False)
    out["planar_to_the_dearer_side"] = ("sah", fp, dear, fpar, None)

    # one bad refine more than allowed, one level more than allowed
    tp, ta, tpar, _ = _built(mts, orc, "twins", "noretract")
    rep = K.check(tp, ta, tpar)
    assert rep.share["bad_refines_max"] == 3 and not rep.names()
    out["fourth_bad_refine"] = ("termination", tp, ta, K.Params(KC.kd_params(mts, "noretract"), tp.n, max_bad_refines=2), None)
    deepest = int(tree.depth.max())
    out["leaf_too_deep"] = ("termination", prims, arrays, K.Params(None, prims.n, max_depth=deepest - 1), None)

    # a sphere removed from a leaf its surface crosses
    sp, sa, spar, _ = _built(mts, orc, "spheres", "defaults")
    st = K.Tree(sp, sa["kd_nodes"], sa["kd_indices"], spar)
    ball = int(sp.sph_prim[1])                               # radius 1 at (0, 0.5, 0)
    holder = next(i for i in st.leaves if ball in st.sets[i] and len(st.sets[i]) > 1 and
                  np.linalg.norm(np.maximum(np.maximum(st.lo[i] - sp.sph[1, :3], sp.sph[1, :3] - st.hi[i]), 0)) < 0.9 and
                  np.linalg.norm(np.maximum(np.abs(st.lo[i] - sp.sph[1, :3]), np.abs(st.hi[i] - sp.sph[1, :3]))) > 1.1)
    out["sphere_removed"] = ("coverage", sp, _with_lists(sa, lambda L: L[holder].remove(ball)), spar, None)

    # statistics: one figure divided by the root's area twice; the enlarged maximum from the unmoved minimum
    e = prims.box_hi - prims.box_lo
    area = 2 * (e[0] * e[1] + e[0] * e[2] + e[1] * e[2])
    assert abs(area - 1) > 0.1
    out["statistic_scaled_twice"] = ("stats", prims, arrays, params, dict(stats, exp_leaves=stats["exp_leaves"] / area))
    mp, ma, mpar, mstats = _built(mts, orc, "soup_small", "defaults")
    lo, hi = mp.box_lo.astype(np.float32), mp.box_hi.astype(np.float32)
    wrong = hi + ((hi - lo) * K.EPSILON + K.EPSILON)
    assert not np.array_equal(wrong, ma["aabb_max"])
    out["enlarged_maximum_from_the_unmoved_minimum"] = ("stats", mp, dict(ma, aabb_max=wrong), mpar, mstats)

    # the min-max phase: the root's plane moved to nine tenths of its tight box
    bp, ba, bpar, _ = _built(mts, orc, "twins", "bins4")
    bt = K.Tree(bp, ba["kd_nodes"], ba["kd_indices"], bpar)
    assert bt.minmax[0]
    x = int(bt.axis[0])
    out["binned_plane_moved"] = ("minmax", bp, _with_plane(ba, 0, split=float(bp.box_lo[x] + 0.9 * (bp.box_hi[x] - bp.box_lo[x]))), bpar, None)

    # two errors that one property alone can see.  A tree binned into 128 bins read as one binned into 4: its planes lie on
    # no boundary of four bins, and nothing else in the tree is wrong.  And a triangle added to a leaf that the min-max phase
    # made outright: the nodes above it take their primitives from the geometry, not from the lists below.
    mp, ma, mpar, _ = _built(mts, orc, "twins", "small_exact")
    out["bin_count_misread"] = ("minmax", mp, ma, K.Params(KC.kd_params(mts, "small_exact"), mp.n, min_max_bins=4), None)
    mt = K.Tree(mp, ma["kd_nodes"], ma["kd_indices"], mpar)
    outright = next(i for i in mt.leaves if not mt.exact[i] and len(mt.sets[i]))
    away = next(int(p) for p in range(mp.n) if ((mp.lo[p] > mt.hi[outright]) | (mp.hi[p] < mt.lo[outright])).any())
    out["triangle_added_above_the_sweep"] = ("tightness", mp, _with_lists(ma, lambda L: L[outright].append(away)), mpar, None)
    return out


_MUT = {}
MUTATIONS = ("index_removed", "sphere_removed", "triangle_added", "plane_to_neighbour", "plane_off_candidates", "axis_changed",
             "children_swapped", "planar_to_the_dearer_side", "bonus_always", "costs_exchanged", "fourth_bad_refine",
             "leaf_too_deep", "statistic_scaled_twice", "enlarged_maximum_from_the_unmoved_minimum", "binned_plane_moved",
             "bin_count_misread", "triangle_added_above_the_sweep")


def _mutation(mts, orc, name):
    if not _MUT:
        _MUT.update(_mutations(mts, orc))
        assert sorted(_MUT) == sorted(MUTATIONS)
    return _MUT[name]


@pytest.mark.parametrize("name", MUTATIONS)
def test_planted_error_is_reported_by_name(mts, orc, name):
    prop, prims, arrays, params, stats = _mutation(mts, orc, name)
    rep = K.check(prims, arrays, params, stats)
    assert prop in rep.names(), (name, rep.names())
    print(name, "->", rep.names(), rep.violations[prop][0])


@pytest.mark.parametrize("prop", K.PROPERTIES)
def test_a_property_turned_off_lets_a_planted_error_through(mts, orc, prop, monkeypatch):
    """each of the six properties is the only one to see at least one of the planted errors: with that property a no-op, the
    checker as a whole reports nothing on that tree"""
    mine = [name for name in MUTATIONS if _mutation(mts, orc, name)[0] == prop]
    monkeypatch.setattr(K, "check_" + prop, lambda *a, **k: None)
    unseen = [name for name in mine if K.check(*_mutation(mts, orc, name)[1:]).names() == []]
    print(prop, "alone sees", unseen, "of", mine)
    assert unseen, (prop, mine)


# ---------------------------------------------------------------------------------------------------------------------
# hand-built trees: the optimum is known by inspection
# ---------------------------------------------------------------------------------------------------------------------
def _four_triangles(mts, mirrored):
    """a box 4 x 1 x 1: triangle 0 lies in the plane x = 1, triangle 1 fills the slab to its left, 2 and 3 the wide slab to its
    right (mirrored: x -> 4 - x).  Every other box face lies on the cell's bounds, so x = 1 is the only candidate; the narrow
    side is the less likely to be visited, so the triangle in the plane belongs to it."""
    tris = np.array([[[1, 0, 0], [1, 1, 0], [1, 0, 1]], [[0, 0, 0], [1, 1, 0], [0.5, 0, 1]],
                     [[1, 0, 0], [4, 1, 0], [2, 0, 1]], [[1, 1, 1], [4, 0, 1], [3, 1, 0]]], dtype=np.float64)
    if mirrored:
        tris[:, :, 0] = 4 - tris[:, :, 0]
    sd = mts.scenes.SceneDescription("four")
    KC.add_triangles(sd, tris, sd.lambertian(0.5))
    sd.point_light((0.0, 5.0, 0.0), 1.0)
    return sd


def _four_trees(mts, mirrored):
    """-> description, primitives, parameters, KdParams, the tree with the triangle in the plane on the narrow side, and the
    tree with it on the wide side"""
    sd = _four_triangles(mts, mirrored)
    prims = K.Prims(sd)
    kp = mts.abi.KdParams(); kp.stop_prims = 2; kp.retract = -1
    narrow, wide = [1, 0], [2, 3]
    split = np.array([3.0 if mirrored else 1.0], dtype=np.float32).view(np.uint32)[0]

    def tree(left, right):
        nodes = np.array([[0 | (1 << 2), split], [0x80000000 | 0, len(left)], [0x80000000 | len(left), 4]], dtype=np.uint32)
        return dict(kd_nodes=nodes, kd_indices=np.array(left + right, dtype=np.uint32))
    good = tree(wide, narrow) if mirrored else tree(narrow, wide)
    dear = tree(wide + [0], [1]) if mirrored else tree([1], [0] + wide)
    return sd, prims, K.Params(kp, prims.n), kp, good, dear


@pytest.mark.parametrize("mirrored", [False, True])
def test_hand_built_trees_over_four_triangles(mts, orc, mirrored):
    sd, prims, params, kp, good, dear = _four_trees(mts, mirrored)
    plane = 3.0 if mirrored else 1.0
    assert K.check(prims, good, params).names() == []
    rep = K.check(prims, dear, params)
    assert "sah" in rep.names() and "costs" in rep.violations["sah"][0], rep.violations
    assert not rep.violations["coverage"] and not rep.violations["tightness"]
    # the cost by hand: area fractions 3/9 and 7/9 of the 4 x 1 x 1 box (surface 18: a 1 x 1 x 1 part has 6, a 3 x 1 x 1 part 14)
    t = K.Tree(prims, good["kd_nodes"], good["kd_indices"], params)
    cl, cr = (float(c[0]) for c in K.plane_costs(params, t.lo[0], t.hi[0], 0, np.array([plane]), 2 if mirrored else 1, 1 if mirrored else 2, 1))
    near, far = 15 + 20 * (6 / 18 * 2 + 14 / 18 * 2), 15 + 20 * (6 / 18 * 1 + 14 / 18 * 3)
    assert np.allclose([cl, cr], [far, near] if mirrored else [near, far], rtol=1e-14)
    # and the oracle's builder makes the good tree
    oa = orc.FlatScene(sd, kd_params=kp).arrays()
    assert np.array_equal(oa["kd_nodes"][0], good["kd_nodes"][0])
    ot = K.Tree(prims, oa["kd_nodes"], oa["kd_indices"], params)
    assert 0 in ot.sets[ot.left[0] + (1 if mirrored else 0)] and 0 not in ot.sets[ot.left[0] + (0 if mirrored else 1)]


# ---------------------------------------------------------------------------------------------------------------------
# the clip restatement
# ---------------------------------------------------------------------------------------------------------------------
def test_clip_restatement_against_the_oracles_clipped_box(mts, orc):
    """ref64_kd.clipped_boxes against orc_clipped_aabb, bit for bit, over cells that cut, graze and miss random triangles and
    cells collapsed to a plane.  (The product's clippedTriangleBox has no export; it is held through the trees it builds.)"""
    rng = np.random.RandomState(5)
    n = 2000
    tri = (rng.rand(n, 3, 3) * 2 - 1).astype(np.float32)
    c = rng.rand(n, 3) * 2 - 1
    h = rng.rand(n, 3) * np.where(rng.rand(n, 1) < 0.3, 0.05, 1.0)
    lo, hi = (c - h).astype(np.float32), (c + h).astype(np.float32)
    flat = rng.rand(n) < 0.2
    hi[flat, 0] = lo[flat, 0] = tri[flat, 0, 0]              # a cell collapsed onto a vertex's plane
    sd = mts.scenes.SceneDescription("clip")
    KC.add_triangles(sd, tri.astype(np.float64), sd.lambertian(0.5))
    prims = K.Prims(sd)
    blo, bhi, kept = K.clipped_boxes(prims, np.arange(n), lo.astype(np.float64), hi.astype(np.float64))
    valid = (bhi >= blo).all(axis=1)
    f32p = C.POINTER(C.c_float)
    p = lambda a: np.ascontiguousarray(a, dtype=np.float32).ctypes.data_as(f32p)
    omin, omax = np.zeros(3, dtype=np.float32), np.zeros(3, dtype=np.float32)
    seen = {True: 0, False: 0}
    for i in range(n):
        ok = bool(orc.lib().orc_clipped_aabb(p(tri[i, 0]), p(tri[i, 1]), p(tri[i, 2]), p(lo[i]), p(hi[i]), omin.ctypes.data_as(f32p), omax.ctypes.data_as(f32p)))
        assert ok == bool(valid[i]), i
        seen[ok] += 1
        if ok:
            assert np.array_equal(omin, blo[i].astype(np.float32)) and np.array_equal(omax, bhi[i].astype(np.float32)), i
    assert seen[True] > 400 and seen[False] > 400, seen          # the mix of this test's own cases
