"""The oracle's traversal (closest hit and any hit) held against the binary64 restatement of tests/ref64_geom.py, which
knows no kd-tree: every scene x ray class of tests/geom_cases.py under the SAH tree and under the hand-built trees (the
oracle takes a substituted tree through a copy of its scene struct, like the device).  Also: the two binary64 forms of the
triangle hit against each other, the ambiguity caps, the measured ratio behind geom_cases.K_GEOM, and mutations of the
oracle's read-out that the comparison must report."""
import ctypes as C

import numpy as np
import pytest

import geom_cases as GC

_WORST = {}


def _trace(orc, mts, c, tree, shadow):
    fs = c.__dict__.setdefault("oracle_scene", orc.FlatScene(c.sd))
    if tree == "sah":
        return orc.trace_rays(fs.scene, c.rays, shadow=shadow)
    sc = GC.with_tree(mts, fs.sc, c.trees[tree])
    return orc.trace_rays(C.pointer(sc), c.rays, shadow=shadow)


@pytest.mark.parametrize("scene", GC.SCENES)
def test_oracle_agrees_with_the_truth_under_every_tree(mts, orc, scene):
    c = GC.case(mts, scene)
    fs = c.__dict__.setdefault("oracle_scene", orc.FlatScene(c.sd))
    assert list(fs.sc.aabb_min) == list(c.scene.sc.aabb_min) and list(fs.sc.aabb_max) == list(c.scene.sc.aabb_max)
    failures = []
    for tree in GC.TREES:
        what = "%s / %s" % (scene, tree)
        f, worst = GC.check_closest(c.closest, _trace(orc, mts, c, tree, False), what)
        failures += f + GC.check_shadow(c.shadow, _trace(orc, mts, c, tree, True), what)
        for k, (ratio, ray) in worst.items():
            if ratio > _WORST.get(scene, (0.0,))[0]:
                cls = [n for n in c.names if c.slices[n].start <= ray < c.slices[n].stop][0]
                _WORST[scene] = (ratio, k, cls, tree)
    print("worst |oracle - truth| / bound:", _WORST.get(scene))
    assert not failures, "\n".join(failures)
    # a decided miss of a ray aimed at the middle of a primitive is a bug, whoever shares it
    s = c.slices["interior"]
    assert (c.closest.hit[s] | c.closest.ambiguous[s]).all()


def test_the_measured_ratio_behind_K(mts, orc):
    """K_GEOM = 5 x the worst |oracle - truth| / bound over all CPU cases; the constant next to it must be that figure"""
    for scene in GC.SCENES:
        if scene not in _WORST:
            test_oracle_agrees_with_the_truth_under_every_tree(mts, orc, scene)
    worst = max(_WORST.values())
    print("worst ratio %.3f (%s of class %s, tree %s)" % worst, {k: round(v[0], 3) for k, v in _WORST.items()})
    assert worst[0] <= GC.WORST_MEASURED, worst
    assert worst[0] >= 0.8 * GC.WORST_MEASURED, "WORST_MEASURED is stale: measured %r" % (worst,)
    assert GC.WORST_MEASURED <= GC.K_VALUE / 5, "the bounds of ref64_geom are too optimistic"
    assert GC.K_GEOM == 5 * GC.WORST_MEASURED
    assert GC.EXCEPTIONS == []


@pytest.mark.parametrize("scene", GC.SCENES)
def test_the_two_binary64_forms_agree(mts, scene):
    """TriAccel restated (projection, precomputed record) against Moeller-Trumbore from the three vertices, on every
    decided record: a misreading inside the restatement shows here, on the CPU"""
    c = GC.case(mts, scene)
    assert c.forms["records"] > 10000
    for k in "tuv":
        assert c.forms[k] <= 1.0, (scene, k, c.forms)


@pytest.mark.parametrize("scene", GC.SCENES)
def test_case_lists_stay_under_the_ambiguity_cap(mts, scene):
    c = GC.case(mts, scene)
    for truth, mode in ((c.closest, "closest"), (c.shadow, "shadow")):
        for cls in c.names:
            amb = truth.ambiguous[c.slices[cls]]
            assert len(amb) >= 100, (scene, cls)
            if cls in GC.AMBIGUOUS_BY_DESIGN:
                assert amb.mean() <= 0.75, (scene, cls, mode, amb.mean())
                assert amb.mean() > 0.05 or mode == "shadow", (scene, cls, mode, "the class no longer probes the undecidable")
            else:
                assert amb.mean() <= GC.MAX_AMBIGUOUS, (scene, cls, mode, amb.mean())


def test_scenes_hold_what_they_are_there_for(mts):
    g = GC.case(mts, "axes").geom
    assert set(g.k.tolist()) == {0, 1, 2}
    T = g.tri
    N = np.abs(np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]))
    N.sort(axis=1)
    near_tie = (N[:, 2] - N[:, 1]) / N[:, 2] < 2e-3
    assert near_tie.sum() >= 30 and set(g.k[near_tie].tolist()) == {0, 1, 2}
    assert ((N[:, 1] == 0) & (N[:, 0] == 0)).sum() >= 20            # normals along the axes
    assert GC.case(mts, "degenerate").geom.degenerate.sum() == 20
    s = GC.case(mts, "spheres").geom
    assert sorted(s.sph[:, 3].tolist())[:1] == [float(np.float32(0.01))] and 100.0 in s.sph[:, 3] and 1.0 in s.sph[:, 3]
    assert (~s.occluder).sum() == 3
    far, near, small = (GC.case(mts, n) for n in ("soup_far", "soup", "soup_small"))
    # the binary32 bound scales with the scene: a thousand times smaller in the scaled soup, far larger in the translated one
    b = [np.nanmedian(c.closest.te[c.slices["interior"], 0] * c.closest.t[c.slices["interior"], 0] ** 0) for c in (far, near, small)]
    assert b[0] > 20 * b[1] and 500 * b[2] < b[1] < 2000 * b[2], b
    for n in GC.SCENES:
        c = GC.case(mts, n)
        for k, t in c.trees.items():
            assert set(t.indices[:t.n_indices].tolist()) == set(range(c.geom.n_prims)), (n, k)
    k = GC.kernel_constants()
    assert len(c.trees["median_small"].nodes) < k["lds_nodes"] and len(c.trees["median_large"].nodes) > 2 * k["top_nodes"]
    assert len(c.trees["chain"].nodes) == 2 * GC.chain_levels() + 1 and len(c.trees["one_leaf"].nodes) == 1


def test_oracle_counters_prove_the_tree_shapes(mts, orc):
    c = GC.case(mts, "twins")
    fs = orc.FlatScene(c.sd)
    rays = c.classes["interior"]
    _, tc = orc.trace_rays(C.pointer(GC.with_tree(mts, fs.sc, c.trees["one_leaf"])), rays, counts=True)
    assert tc.n_inner == 0 and tc.n_idx == len(rays) * c.geom.n_prims
    diag = c.classes["chords"][:2]
    _, up = orc.trace_rays(C.pointer(GC.with_tree(mts, fs.sc, c.trees["chain"])), diag[:1], counts=True)
    assert up.n_inner == GC.chain_levels() and up.n_leaf == GC.chain_levels() + 1      # one push per level, every leaf visited


def _mutations(c, hits, shadow_hits):
    """(name, closest read-out, shadow read-out) with one defect each"""
    t = hits[:, 0].copy().view(np.float32)
    hit = hits[:, 3] != GC.MISS
    m = hits.copy(); m[:, 1], m[:, 2] = hits[:, 2], hits[:, 1]
    yield "u and v swapped", m, shadow_hits
    m = hits.copy(); m[:, 0] = (t * np.float32(1 + 2.0 ** -18)).view(np.uint32)
    yield "t scaled by 1 + 2^-18", m, shadow_hits
    m = hits.copy()
    some = np.nonzero(hit)[0][::100]
    m[some, 3] = (m[some, 3] + 1) % c.geom.n_prims
    yield "the primitive of 1 % of the hits replaced by its neighbour", m, shadow_hits
    s = shadow_hits.copy(); s[:, 3] = hit
    yield "the occluder bit ignored", hits, s
    m = hits.copy()
    col = np.argmax(c.closest.prim == np.where(hit, hits[:, 3].astype(np.int64), -2)[:, None], axis=1)
    far = c.closest.far[np.arange(len(hits)), col]
    swap = hit & np.isfinite(far) & (np.abs(far - t) > 1e-3 * np.abs(far))
    m[swap, 0] = far[swap].astype(np.float32).view(np.uint32)
    yield "the sphere's far root where the near one is valid", m, shadow_hits
    m = hits.copy(); m[np.nonzero(hit & ~c.closest.ambiguous)[0][:1], 0] = np.float32(np.nan).view(np.uint32)
    yield "a NaN t", m, shadow_hits


def test_mutated_read_outs_fail_the_checks(mts, orc):
    c = GC.case(mts, "spheres")
    hits, sh = _trace(orc, mts, c, "sah", False), _trace(orc, mts, c, "sah", True)
    assert not GC.check_closest(c.closest, hits)[0] and not GC.check_shadow(c.shadow, sh)
    seen = []
    for name, m, s in _mutations(c, hits, sh):
        failures = GC.check_closest(c.closest, m)[0] + GC.check_shadow(c.shadow, s)
        assert failures, "not reported: " + name
        seen.append(name)
    assert len(seen) == 6
    # a tree-independent answer: the triangle scenes report the first three too
    c = GC.case(mts, "twins")
    hits, sh = _trace(orc, mts, c, "sah", False), _trace(orc, mts, c, "sah", True)
    for name, m, s in list(_mutations(c, hits, sh))[:3]:
        assert GC.check_closest(c.closest, m)[0], "not reported: " + name
