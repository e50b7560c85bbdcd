"""A binary64 truth for the kd-tree builders that is not a builder: order-free properties that every correct SAH kd-tree of the
reference's kind satisfies, checked from the scene's vertices and radii and the flat tree alone.  It knows nothing of events,
histograms, jobs or sort order; the oracle's, the host's and the device phases' trees all go through check().  One thing it
reads from the tree under test where geometry cannot say: on which side of a min-max node lies a primitive that is flat in
that node's plane when no other box is cut by it (Tree.__init__); property 5 then holds the partition with that primitive
placed as the tree placed it, and coverage and tightness hold the placement itself.  Written from
    GenericKDTree::buildInternal, buildTree       include/mitsuba/render/gkdtree.h:711-724, :913-1214, :1898-2345
    SurfaceAreaHeuristic                          include/mitsuba/render/sahkdtree3.h:35-79
    Triangle::getClippedAABB, sutherlandHodgman   src/libcore/triangle.cpp:58-158;  Shape::getClippedAABB src/librender/shape.cpp:59-63
    Sphere::getAABB                               src/shapes/sphere.cpp:80-86
not from csrc/ or oracle/.  Test infrastructure.

A node's cell is found by descending from the un-enlarged scene box; its primitive set is the union of the lists of the
leaves below it.  A node is in the min-max phase (gkdtree.h:1735-1867) when the primitives that reach it through the planes
above it, by their unclipped boxes (Tree.__init__ says how a box with a face in a plane is placed), number more than
exactPrimThreshold and it is not a leaf that phase makes outright (:1741-1744: at most stopPrims primitives, or maxDepth
reached; such a leaf is not clipped); every other node belongs to the exact sweep (:1898-2345).

The properties (Report.violations[name], Report.left_out[name] = (fragile cases, cases the property applies to)):

coverage     For every triangle P the areas of the polygons P n cell, summed over the leaves that list P, reach
             area(P n scene box) x (1 - eps).  The clip is Sutherland-Hodgman in binary64 against the six planes.  eps is the
             checker's own rounding: an intersection point costs 6 operations per plane (two differences, a quotient, a
             difference, a product, a sum), 36 in a chain through six planes, the fan area 15 more (differences, products,
             the sum over at most seven fan triangles, the norm): K_CLIP = 51 operations of 2^-53 each, on coordinates of
             magnitude M.  A point off by K_CLIP x 2^-53 x M moves the area by at most the perimeter times that, so
             eps(P) = K_CLIP x 2^-53 x M x perimeter(P) / area(P).  (A zero-area triangle can never be hit, triaccel.h:80-83,
             and asks nothing.)  A sphere must be listed by every leaf whose cell its surface crosses: the nearest point of
             the cell lies nearer the centre than |r| - m and the farthest farther than |r| + m, m = 2 x 2^-24 x (max|c| + |r|),
             twice the one binary32 rounding of a face of Sphere::getAABB.  A cell that does not overlap the sphere's float32
             box in volume is not crossed -- an exact comparison of binary32 values, and the reference's own measure of where
             the shape is; the SAH likes to cut along those very faces.  A cell inside the box and inside the margin that does
             not list the sphere is fragile.
tightness    Every primitive a leaf lists has a box that meets the closed cell; with clip on, below the exact sweep, a listed
             triangle's polygon in the cell grown by one binary32 step is not empty (the reference rounds its clipped boxes
             outward, triangle.cpp:126-150).
sah          Every inner node of the exact sweep splits at a candidate -- a face, strictly inside the cell, of the clipped box
             (clip off: the box) of one of its primitives -- and the cost of its plane (gkdtree.h:1974-2014: traversalCost +
             queryCost x (pL nL + pR nR), times emptySpaceBonus when a side is empty, planar primitives on the side the tree
             put them) is at most (1 + TAU) x the minimum over all candidates with planar primitives on the cheaper side.
             No tie order is restated.  TAU = 2 x gamma(K_COST): the binary32 cost of kdbuild.h's SAH and planeCost is
             17 roundings from the box: extents 1, the three products 3, their sum 5, the reciprocal 6; t0 = (e e) temp 10,
             t1 = (e + e) temp 9; a width 1, t1 x width 11, + t0 12; x count 13, the sum 14, x queryCost 15, + traversalCost
             16, x bonus 17; all terms are positive, so gamma_17 bounds each cost and 2 gamma_17 their ratio.  The clip here
             is the reference's own arithmetic (binary64, then outward to binary32), so the boxes are the builders' except
             where a builder keeps the box a primitive had in the parent's cell: that one may differ by a step.  A node that
             fails and has two distinct faces (or a face and a cell bound) one binary32 step apart is therefore left out as
             fragile -- a count could change there -- and not reported; a node that passes is never left out.
termination  No leaf deeper than maxDepth (root = 1); on no root-to-leaf path more than maxBadRefines inner nodes whose minimum
             cost is at least queryCost x n x (1 + TAU) (:2049-2060); retract off: a leaf above maxDepth with more than
             stopPrims primitives has a minimum cost of at least the leaf cost; retract on: the bottom-up cost
             (:2321-2341, no bonus) of a surviving inner node of the exact sweep is below queryCost x n.  A subtree of
             height h compounds 15 roundings a level: its tolerance is 2 x gamma(15 h + 2).  Fragile: within the tolerance;
             and, as in sah, a leaf that fails the retract-off rule beside two faces one binary32 step apart.  Bad refines
             are counted whatever the faces.
stats        kdstats(): inner, leaf and index counts recounted; expTraversalSteps, expLeavesVisited, expPrimitivesIntersected
             (:1178-1213) in binary64 within gamma(n + K_AREA) x the value, n the number of float32 accumulations and K_AREA = 6
             the roundings of one AABB::getSurfaceArea plus the final quotient: every term is positive.  The enlarged box
             (:1170-1176, the maximum from the already-moved minimum) in a float32 mirror, bit for bit.

minmax       Every inner node of the min-max phase (:1735-1867, :2405-2596): the primitives that reach it are parted by its plane
             exactly as by some inner bin boundary of its tight box (left only when the box ends below the boundary, right only
             when it begins at or above it: what `max <= pos`, `min > pos` say at the largest binary32 value below the
             boundary, :2517-2545), and the binned cost at that boundary -- binary64, from geometric counts, no histogram -- is
             within 2 x gamma(K_COST + minMaxBins) of the minimum over the minMaxBins - 1 boundaries of the three axes (the
             left width is a running float32 sum of up to minMaxBins bin sizes).  The plane lies strictly inside the tight box.
             The move of the plane onto the nearer child bound (:2575-2590) changes no partition and is not restated.  The
             tight box of a child is its primitives' boxes within the parent's tight box, cut at the plane.  A node that fails
             and has a face within two binary32 steps of a boundary is left out as fragile."""
import numpy as np

F = np.float32
U32 = 2.0 ** -24
U64 = 2.0 ** -53
K_CLIP = 51
K_COST = 17
K_AREA = 6
EPSILON = F(1e-4)                                  # constants.h:31
MAX_DEPTH = 48                                     # MTS_KD_MAXDEPTH
PROPERTIES = ("coverage", "tightness", "sah", "termination", "minmax", "stats")
M = 10                                             # vertices of a clipped triangle: 3 + one per plane, and one to spare


def gamma(k, u=U32):
    return k * u / (1 - k * u)


TAU = 2 * gamma(K_COST)


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
class Params:
    """the effective parameters: the caller's, the reference's defaults where it gave none (gkdtree.h:711-724, :945-947).
    bonus_always: a deliberately wrong reading, for the mutation tests"""

    def __init__(self, kp, n_prims, **override):
        g = (lambda k: getattr(kp, k)) if kp is not None else (lambda k: 0)
        self.traversal_cost = float(F(g("traversal_cost"))) if g("traversal_cost") > 0 else 15.0
        self.query_cost = float(F(g("query_cost"))) if g("query_cost") > 0 else 20.0
        self.empty_space_bonus = float(F(g("empty_space_bonus"))) if g("empty_space_bonus") > 0 else float(F(0.9))
        self.stop_prims = g("stop_prims") if g("stop_prims") > 0 else 6
        self.max_bad_refines = g("max_bad_refines") if g("max_bad_refines") > 0 else 3
        self.exact_prim_threshold = g("exact_prim_threshold") if g("exact_prim_threshold") > 0 else 65536
        self.min_max_bins = g("min_max_bins") if g("min_max_bins") > 1 else 128
        self.clip = not g("clip") < 0
        self.retract = not g("retract") < 0
        self.max_depth = g("max_depth") if g("max_depth") > 0 else 0
        if self.max_depth == 0 and n_prims > 0:
            self.max_depth = int(F(8) + F(1.3) * F(int(n_prims).bit_length() - 1))
        self.max_depth = min(self.max_depth, MAX_DEPTH)
        self.bonus_always = False
        for k, v in override.items():
            assert hasattr(self, k), k
            setattr(self, k, v)


class Prims:
    """the primitives of a scene description in the index space of ShapeKDTree (skdtree.cpp:43-65): triangle corners as
    float32 values taken to binary64, sphere centres and radii, and the float32 box of each (Triangle::getAABB, Sphere::getAABB)"""

    def __init__(self, sd):
        tris, tprim, sph, sprim = [], [], [], []
        p = 0
        for m in sd.meshes:
            if m.sphere is not None:
                sph.append(list(m.sphere[0]) + [m.sphere[1]]); sprim.append(p); p += 1
            else:
                v = np.asarray(m.positions, dtype=np.float32).astype(np.float64)[np.asarray(m.triangles).astype(np.int64)]
                tris.append(v); tprim += range(p, p + len(v)); p += len(v)
        self.n = p
        self.tri = np.concatenate(tris) if tris else np.zeros((0, 3, 3))
        self.tri_prim = np.array(tprim, dtype=np.int64)
        self.sph = np.array(sph, dtype=np.float64).reshape(-1, 4)
        self.sph_prim = np.array(sprim, dtype=np.int64)
        self.tri_of = np.full(p, -1, dtype=np.int64); self.tri_of[self.tri_prim] = np.arange(len(self.tri_prim))
        self.lo = np.zeros((p, 3)); self.hi = np.zeros((p, 3))
        if len(self.tri):
            self.lo[self.tri_prim] = self.tri.min(axis=1); self.hi[self.tri_prim] = self.tri.max(axis=1)
        if len(self.sph):
            c, r = self.sph[:, 0:3].astype(F), np.abs(self.sph[:, 3:4]).astype(F)
            self.lo[self.sph_prim] = (c - r).astype(np.float64); self.hi[self.sph_prim] = (c + r).astype(np.float64)
        self.box_lo = self.lo.min(axis=0) if p else np.zeros(3)
        self.box_hi = self.hi.max(axis=0) if p else np.zeros(3)


# ---------------------------------------------------------------------------------------------------------------------
# the clip: Sutherland-Hodgman in binary64 (triangle.cpp:58-104), many (triangle, cell) pairs at once
# ---------------------------------------------------------------------------------------------------------------------
def _clip_plane(V, cnt, axis, pos, is_min):
    n = len(V)
    idx = np.arange(M)[None, :]
    valid = (idx < cnt[:, None]) & (cnt[:, None] >= 3)                                       # :61-62
    nxt_i = np.where(idx + 1 < cnt[:, None], idx + 1, 0)
    nxt = np.take_along_axis(V, nxt_i[:, :, None], axis=1)
    sign = 1.0 if is_min else -1.0
    cin = sign * (V[:, :, axis] - pos[:, None]) >= 0                                          # :66-67
    nin = sign * (nxt[:, :, axis] - pos[:, None]) >= 0                                        # :75-76
    t = (pos[:, None] - V[:, :, axis]) / (nxt[:, :, axis] - V[:, :, axis])                    # :84 / :91
    p = V + (nxt - V) * t[:, :, None]                                                         # :86 / :93
    p[:, :, axis] = pos[:, None]                                                              # :87 / :94
    out = np.stack([p, nxt], axis=2).reshape(n, 2 * M, 3)
    keep = np.stack([(cin != nin) & valid, nin & valid], axis=2).reshape(n, 2 * M)
    order = np.argsort(~keep, axis=1, kind="stable")[:, :M]
    cnt2 = keep.sum(axis=1)
    assert (cnt2 <= M).all()
    return np.take_along_axis(out, order[:, :, None], axis=1), cnt2


def clip_polygons(tri, lo, hi):
    """tri [n][3][3], lo / hi [n][3] -> vertices [n][M][3], counts [n] of the polygons tri n [lo, hi]"""
    n = len(tri)
    V = np.zeros((n, M, 3)); V[:, :3] = tri
    cnt = np.full(n, 3, dtype=np.int64)
    with np.errstate(all="ignore"):
        for axis in range(3):                                                                 # triangle.cpp:119-122
            V, cnt = _clip_plane(V, cnt, axis, lo[:, axis], True)
            V, cnt = _clip_plane(V, cnt, axis, hi[:, axis], False)
    return V, cnt


def polygon_area(V, cnt):
    valid = np.arange(M)[None, :] < cnt[:, None]
    with np.errstate(all="ignore"):
        W = np.where(valid[:, :, None], np.where(valid[:, :, None], V, 0.0) - np.where(valid[:, 0:1, None], V[:, 0:1], 0.0), 0.0)
        c = np.cross(W[:, 1:-1], W[:, 2:]).sum(axis=1)
    return np.where(cnt >= 3, 0.5 * np.linalg.norm(c, axis=1), 0.0)


def clipped_boxes(prims, ids, lo, hi):
    """Triangle::getClippedAABB (triangle.cpp:106-158) / Shape::getClippedAABB (shape.cpp:59-63) of primitives ids [n] in cells
    lo / hi [n][3] -> box_lo, box_hi [n][3] (float32 values), kept [n]: valid and of non-zero surface area (gkdtree.h:1513,
    :2190-2200)"""
    n = len(ids)
    blo = np.full((n, 3), np.inf); bhi = np.full((n, 3), -np.inf)
    t = prims.tri_of[ids]
    it = np.nonzero(t >= 0)[0]
    if len(it):
        V, cnt = clip_polygons(prims.tri[t[it]], lo[it], hi[it])
        valid = (np.arange(M)[None, :] < cnt[:, None])[:, :, None]
        f = V.astype(F)
        with np.errstate(all="ignore"):
            down = np.where(f > V, np.nextafter(f, F(-np.inf)), f).astype(np.float64)         # :133-146
            up = np.where(f < V, np.nextafter(f, F(np.inf)), f).astype(np.float64)
        blo[it] = np.where(valid, down, np.inf).min(axis=1)
        bhi[it] = np.where(valid, up, -np.inf).max(axis=1)
    isph = np.nonzero(t < 0)[0]
    blo[isph] = prims.lo[ids[isph]]; bhi[isph] = prims.hi[ids[isph]]
    blo = np.maximum(blo, lo); bhi = np.minimum(bhi, hi)                                       # result.clip(aabb), :155
    ok = (bhi >= blo).all(axis=1)
    with np.errstate(all="ignore"):
        d = np.where(ok[:, None], bhi - blo, 0.0).astype(F)
        area = F(2.0) * (d[:, 0] * d[:, 1] + d[:, 0] * d[:, 2] + d[:, 1] * d[:, 2])            # aabb.h:326-329, in float32
    return blo, bhi, ok & (area > 0)


# ---------------------------------------------------------------------------------------------------------------------
# the tree
# ---------------------------------------------------------------------------------------------------------------------
class Tree:
    def __init__(self, prims, kd_nodes, kd_indices, params):
        nodes = np.ascontiguousarray(kd_nodes, dtype=np.uint32).reshape(-1, 2)
        self.indices = np.ascontiguousarray(kd_indices, dtype=np.uint32).astype(np.int64)
        n = len(nodes)
        self.n = n
        self.leaf = (nodes[:, 0] & 0x80000000) != 0
        self.axis = (nodes[:, 0] & 3).astype(np.int64)
        self.left = np.arange(n) + (nodes[:, 0] >> 2).astype(np.int64)
        self.split = nodes[:, 1].copy().view(np.float32).astype(np.float64)
        self.start = (nodes[:, 0] & 0x7FFFFFFF).astype(np.int64)
        self.end = nodes[:, 1].astype(np.int64)
        self.lo = np.zeros((n, 3)); self.hi = np.zeros((n, 3))
        self.depth = np.zeros(n, dtype=np.int64)
        self.parent = np.full(n, -1, dtype=np.int64)
        self.errors = []
        self.order = []                                     # parents before children
        seen = np.zeros(n, dtype=bool)
        self.lo[0], self.hi[0], self.depth[0] = prims.box_lo, prims.box_hi, 1
        todo = [0]
        while todo:
            i = todo.pop()
            if seen[i]:
                self.errors.append("node %d is reached twice" % i); continue
            seen[i] = True
            self.order.append(i)
            if self.leaf[i]:
                if not (0 <= self.start[i] <= self.end[i] <= len(self.indices)):
                    self.errors.append("leaf %d lists [%d, %d) of %d indices" % (i, self.start[i], self.end[i], len(self.indices)))
                    self.end[i] = self.start[i] = 0
                continue
            l = self.left[i]
            if self.axis[i] > 2 or not (i < l and l + 1 < n):
                self.errors.append("inner node %d: axis %d, children %d" % (i, self.axis[i], l))
                self.leaf[i] = True; self.start[i] = self.end[i] = 0
                continue
            for c in (l, l + 1):
                self.lo[c], self.hi[c], self.depth[c], self.parent[c] = self.lo[i], self.hi[i], self.depth[i] + 1, i
            self.hi[l, self.axis[i]] = self.split[i]
            self.lo[l + 1, self.axis[i]] = self.split[i]
            todo += [l + 1, l]
        if not seen.all():
            self.errors.append("%d nodes are not reachable" % (~seen).sum())
        if (self.indices >= prims.n).any():
            self.errors.append("an index past the last primitive")
            self.indices = np.minimum(self.indices, prims.n - 1)
        # primitive sets (union of the leaves below) and heights, children before parents
        self.sets = [None] * n
        self.height = np.zeros(n, dtype=np.int64)
        for i in reversed(self.order):
            if self.leaf[i]:
                self.sets[i] = np.unique(self.indices[self.start[i]:self.end[i]])
            else:
                l = self.left[i]
                self.sets[i] = np.union1d(self.sets[l], self.sets[l + 1])
                self.height[i] = 1 + max(self.height[l], self.height[l + 1])
        # the phase of every node: how many primitives reach it through the planes above, by their unclipped boxes
        self.minmax = np.zeros(n, dtype=bool)
        direct = np.zeros(n, dtype=bool)                    # a leaf the min-max phase made itself (gkdtree.h:1741-1744): unclipped
        reach = {0: np.arange(prims.n)}
        tight = {0: (prims.box_lo.copy(), prims.box_hi.copy())}
        self.reach, self.tight, self.reach_all = {}, {}, {}  # of the nodes of the min-max phase; reach_all: and of their children
        for i in self.order:
            r = reach.pop(i, None)
            if r is None:
                continue
            tlo, thi = tight.pop(i)
            self.reach_all[i] = r
            direct[i] = self.leaf[i] and (len(r) <= params.stop_prims or self.depth[i] >= params.max_depth)
            self.minmax[i] = len(r) > params.exact_prim_threshold and not direct[i]
            if not self.minmax[i]:
                continue
            self.reach[i], self.tight[i] = r, (tlo, thi)
            if self.leaf[i]:
                continue
            a, s, l = self.axis[i], self.split[i], self.left[i]
            mn, mx = prims.lo[r, a], prims.hi[r, a]
            # a box that ends in the plane is left only and one cut by it goes both ways, wherever the plane came to rest.
            # One that begins in the plane: while another box is cut, the plane is still the boundary's (the largest
            # binary32 value below it) and `min > pos` fails: both ways; otherwise the plane has moved onto the right
            # child's bound, which this box set: right only.  One that lies in the plane: left (`max <= pos`) while a box
            # is cut, else on the side whose bound the plane moved to, which only the lists below tell.
            cut = bool(((mn < s) & (mx > s)).any())
            flat = (mn == s) & (mx == s)
            flat_right = flat & (not cut) & np.isin(r, self.sets[l + 1]) & ~np.isin(r, self.sets[l])
            go_l = (mn < s) | (flat & ~flat_right) | ((mn == s) & cut)
            go_r = (mx > s) | flat_right
            reach[l], reach[l + 1] = r[go_l], r[go_r]
            # the children's tight boxes: their primitives' boxes within the parent's, cut at the plane (gkdtree.h:2560-2590)
            for c, rc in ((l, reach[l]), (l + 1, reach[l + 1])):
                if len(rc):
                    clo, chi = np.maximum(prims.lo[rc].min(axis=0), tlo), np.minimum(prims.hi[rc].max(axis=0), thi)
                else:
                    clo, chi = tlo.copy(), thi.copy()
                if c == l:
                    chi[a] = min(chi[a], s)
                else:
                    clo[a] = max(clo[a], s)
                tight[c] = (clo, chi)
        # exact[i]: the node was built by the exact sweep (itself or an ancestor is the transition node)
        self.exact = np.zeros(n, dtype=bool)
        for i in self.order:
            self.exact[i] = (self.parent[i] >= 0 and self.exact[self.parent[i]]) or not (self.minmax[i] or direct[i])
        self.leaves = [i for i in self.order if self.leaf[i]]
        self.count = np.array([len(self.reach[i]) if i in self.reach else len(self.sets[i]) for i in range(n)])   # the builder's n
        self.inner = [i for i in self.order if not self.leaf[i]]


class Report:
    def __init__(self):
        self.violations = {k: [] for k in PROPERTIES}
        self.violations["structure"] = []
        self.left_out = {k: (0, 0) for k in PROPERTIES}
        self.share = {}                                     # measured maxima as shares of their bounds

    def names(self):
        return sorted(k for k, v in self.violations.items() if v)


# ---------------------------------------------------------------------------------------------------------------------
# 1. coverage
# ---------------------------------------------------------------------------------------------------------------------
def check_coverage(prims, tree, params, rep):
    bad = rep.violations["coverage"]
    pl, pp = [], []                                          # (leaf, triangle primitive) pairs
    for i in tree.leaves:
        s = tree.sets[i]
        s = s[prims.tri_of[s] >= 0]
        pl += [i] * len(s); pp += s.tolist()
    pl, pp = np.array(pl, dtype=np.int64), np.array(pp, dtype=np.int64)
    got = np.zeros(prims.n)
    if len(pp):
        V, cnt = clip_polygons(prims.tri[prims.tri_of[pp]], tree.lo[pl], tree.hi[pl])
        np.add.at(got, pp, polygon_area(V, cnt))
    T = prims.tri
    if len(T):
        nt = len(T)
        V, cnt = clip_polygons(T, np.tile(prims.box_lo, (nt, 1)), np.tile(prims.box_hi, (nt, 1)))
        want = polygon_area(V, cnt)
        perim = sum(np.linalg.norm(T[:, (j + 1) % 3] - T[:, j], axis=1) for j in range(3))
        mag = max(np.abs(prims.box_lo).max(), np.abs(prims.box_hi).max())
        with np.errstate(all="ignore"):
            eps = np.where(want > 0, K_CLIP * U64 * mag * perim / want, 0.0)
        rep.share["coverage_eps_max"] = float(eps.max())
        g = got[prims.tri_prim]
        short = g < want * (1 - eps)
        for k in np.nonzero(short)[0][:8]:
            bad.append("triangle %d: its leaves hold area %.17g of %.17g (eps %.3g)" % (prims.tri_prim[k], g[k], want[k], eps[k]))
        with np.errstate(all="ignore"):
            rep.share["coverage_deficit_over_eps"] = float(np.nan_to_num(np.where(eps > 0, (1 - g / want) / eps, 0.0)).max())
    applies = len(T)
    fragile = 0
    for k, (cx, cy, cz, r) in enumerate(prims.sph):
        c, r, p = np.array([cx, cy, cz]), abs(r), prims.sph_prim[k]
        lo, hi = tree.lo[tree.leaves], tree.hi[tree.leaves]
        near = np.linalg.norm(np.maximum(np.maximum(lo - c, c - hi), 0.0), axis=1)
        far = np.linalg.norm(np.maximum(np.abs(lo - c), np.abs(hi - c)), axis=1)
        m = 2 * U32 * (np.abs(c).max() + r)
        inside_box = ((lo < prims.hi[p]) & (hi > prims.lo[p])).all(axis=1)     # exact: cells and box faces are float32 values
        crosses = (near < r - m) & (far > r + m) & inside_box
        maybe = (near < r + m) & (far > r - m) & ~crosses & inside_box
        listed = np.array([p in tree.sets[i] for i in tree.leaves])
        applies += int((crosses | maybe).sum()); fragile += int((maybe & ~listed).sum())
        for j in np.nonzero(crosses & ~listed)[0][:8]:
            bad.append("sphere %d crosses the cell of leaf %d, which does not list it" % (p, tree.leaves[j]))
    rep.left_out["coverage"] = (fragile, applies)


# ---------------------------------------------------------------------------------------------------------------------
# 2. tightness
# ---------------------------------------------------------------------------------------------------------------------
def check_tightness(prims, tree, params, rep):
    bad = rep.violations["tightness"]
    pl, pp = [], []
    for i in tree.leaves:
        pl += [i] * len(tree.sets[i]); pp += tree.sets[i].tolist()
    pl, pp = np.array(pl, dtype=np.int64), np.array(pp, dtype=np.int64)
    if not len(pp):
        return
    apart = ((prims.lo[pp] > tree.hi[pl]) | (prims.hi[pp] < tree.lo[pl])).any(axis=1)
    for k in np.nonzero(apart)[0][:8]:
        bad.append("leaf %d lists primitive %d, whose box misses its cell" % (pl[k], pp[k]))
    n_cases = len(pp)
    if params.clip:
        sel = np.nonzero(tree.exact[pl] & (prims.tri_of[pp] >= 0))[0]
        if len(sel):
            lo = np.nextafter(tree.lo[pl[sel]].astype(F), F(-np.inf)).astype(np.float64)
            hi = np.nextafter(tree.hi[pl[sel]].astype(F), F(np.inf)).astype(np.float64)
            _, cnt = clip_polygons(prims.tri[prims.tri_of[pp[sel]]], lo, hi)
            for k in np.nonzero(cnt == 0)[0][:8]:
                bad.append("leaf %d lists triangle %d, which does not enter its cell" % (pl[sel[k]], pp[sel[k]]))
            n_cases += len(sel)
    rep.left_out["tightness"] = (0, n_cases)


# ---------------------------------------------------------------------------------------------------------------------
# 3. greedy SAH optimality of the exact sweep; the minimum costs also serve property 4
# ---------------------------------------------------------------------------------------------------------------------
def _probabilities(lo, hi, axis, pos):
    """SurfaceAreaHeuristic (sahkdtree3.h:37-58) in binary64: the areas of the two parts over the area of the cell"""
    e = hi - lo
    temp = 1.0 / (e[0] * e[1] + e[1] * e[2] + e[0] * e[2])
    o = [(1, 2), (0, 2), (0, 1)][axis]
    t0, t1 = e[o[0]] * e[o[1]] * temp, (e[o[0]] + e[o[1]]) * temp
    return t0 + t1 * (pos - lo[axis]), t0 + t1 * (hi[axis] - pos)


def plane_costs(params, lo, hi, axis, pos, nl, nr, npl):
    """gkdtree.h:1983-2004 in binary64 -> the cost with the planar primitives on the left, and on the right"""
    pl, pr = _probabilities(lo, hi, axis, pos)
    T, Q, B = params.traversal_cost, params.query_cost, params.empty_space_bonus
    cl = T + Q * (pl * (nl + npl) + pr * nr)
    cr = T + Q * (pl * nl + pr * (nr + npl))
    el = (nl + npl == 0) | (nr == 0) | params.bonus_always
    er = (nl == 0) | (nr + npl == 0) | params.bonus_always
    return np.where(el, cl * B, cl), np.where(er, cr * B, cr)


def _one_step_apart(values):
    v = np.unique(np.asarray(values, dtype=F))
    return bool(len(v) > 1 and (np.nextafter(v[:-1], F(np.inf)) == v[1:]).any())


class _NodeBoxes:
    """the boxes the sweep sees in every node of the exact phase: clipped to the cell, or the plain boxes with clip off"""

    def __init__(self, prims, tree, params, nodes):
        pn, pp = [], []
        for i in nodes:
            pn += [i] * len(tree.sets[i]); pp += tree.sets[i].tolist()
        pn, pp = np.array(pn, dtype=np.int64), np.array(pp, dtype=np.int64)
        if params.clip and len(pp):
            blo, bhi, kept = clipped_boxes(prims, pp, tree.lo[pn], tree.hi[pn])
        else:
            blo, bhi, kept = prims.lo[pp], prims.hi[pp], np.ones(len(pp), dtype=bool)
        self.at = {}
        ends = np.cumsum([len(tree.sets[i]) for i in nodes])
        for i, e in zip(nodes, ends):
            s = slice(e - len(tree.sets[i]), e)
            self.at[i] = (pp[s], blo[s], bhi[s], kept[s])


def _sweep(params, lo, hi, blo, bhi):
    """-> (minimum cost with planar primitives on the cheaper side, fragile, candidates: the positions per axis)"""
    best, fragile, cands = np.inf, False, []
    for a in range(3):
        mn, mx = blo[:, a], bhi[:, a]
        faces = np.unique(np.concatenate([mn, mx]))
        fragile |= _one_step_apart(np.concatenate([faces, [lo[a], hi[a]]]))
        pos = faces[(faces > lo[a]) & (faces < hi[a])]                                        # gkdtree.h:1975
        cands.append(pos)
        if not len(pos):
            continue
        nl = (mn[None, :] < pos[:, None]).sum(axis=1)
        nr = (mx[None, :] > pos[:, None]).sum(axis=1)
        npl = ((mn[None, :] == pos[:, None]) & (mx[None, :] == pos[:, None])).sum(axis=1)
        cl, cr = plane_costs(params, lo, hi, a, pos, nl, nr, npl)
        c = np.where(npl > 0, np.minimum(cl, cr), cl)
        best = min(best, float(c.min()))
    return best, fragile, cands


def _judge_plane(params, tree, i, ids, blo, bhi, cands, best):
    """the plane of inner node i against the candidates -> its excess cost as a share of TAU, or the violation as text"""
    lo, hi = tree.lo[i], tree.hi[i]
    a, s, l = tree.axis[i], tree.split[i], tree.left[i]
    if not (cands[a] == s).any():
        return "node %d: its plane %d @ %.9g is no candidate" % (i, a, s)
    mn, mx = blo[:, a], bhi[:, a]
    planar = (mn == s) & (mx == s)
    nl, nr, npl = int((mn < s).sum()), int((mx > s).sum()), int(planar.sum())
    cl, cr = (float(x[0]) for x in plane_costs(params, lo, hi, a, np.array([s]), nl, nr, npl))
    cost = cl
    if npl:
        in_l, in_r = np.isin(ids[planar], tree.sets[l]), np.isin(ids[planar], tree.sets[l + 1])
        if in_r.all() and not in_l.any():
            cost = cr
        elif not (in_l.all() and not in_r.any()):
            return "node %d: the primitives in its plane are not all on one side" % i
    if cost > best * (1 + TAU):
        return ("node %d: plane %d @ %.9g costs %.17g, the best candidate %.17g (ratio - 1 = %.3g, tau %.3g)"
                % (i, a, s, cost, best, cost / best - 1, TAU))
    return (cost / best - 1) / TAU


def check_sah(prims, tree, params, rep):
    bad = rep.violations["sah"]
    nodes = [i for i in tree.order if tree.exact[i] and (not tree.leaf[i] or len(tree.sets[i]) > params.stop_prims)]
    boxes = _NodeBoxes(prims, tree, params, nodes)
    tree.min_cost, tree.cost_fragile = {}, {}
    applies = fragile = 0
    worst = 0.0
    for i in nodes:
        ids, blo, bhi, kept = boxes.at[i]
        if not kept.all() and not tree.leaf[i]:
            bad.append("node %d holds primitives %s, whose clipped boxes are empty or flat" % (i, ids[~kept][:4].tolist()))
        ids, blo, bhi = ids[kept], blo[kept], bhi[kept]
        lo, hi = tree.lo[i], tree.hi[i]
        with np.errstate(all="ignore"):
            best, frag, cands = _sweep(params, lo, hi, blo, bhi)
        tree.min_cost[i], tree.cost_fragile[i] = best, frag
        if tree.leaf[i]:
            continue
        applies += 1
        found = _judge_plane(params, tree, i, ids, blo, bhi, cands, best)
        if isinstance(found, str):
            if frag:                                         # a face one step from another: the count there is not the checker's to call
                fragile += 1
            else:
                bad.append(found)
        else:
            worst = max(worst, found)
    rep.left_out["sah"] = (fragile, applies)
    rep.share["sah_excess_over_tau"] = worst


# ---------------------------------------------------------------------------------------------------------------------
# 4. termination and bad refines
# ---------------------------------------------------------------------------------------------------------------------
def check_termination(prims, tree, params, rep):
    bad = rep.violations["termination"]
    costs, cost_fragile = getattr(tree, "min_cost", {}), getattr(tree, "cost_fragile", {})    # what properties 3 and 5 found
    Q = params.query_cost
    tau_of = lambda i: 2 * gamma(K_COST + params.min_max_bins) if tree.minmax[i] else TAU
    applies = fragile = 0
    for i in tree.leaves:
        applies += 1
        if tree.depth[i] > params.max_depth:
            bad.append("leaf %d lies at depth %d, maxDepth is %d" % (i, tree.depth[i], params.max_depth))
    # bad refines on every root-to-leaf path
    refines = np.zeros(tree.n, dtype=np.int64)
    for i in tree.order:
        up = refines[tree.parent[i]] if tree.parent[i] >= 0 else 0
        mine = 0
        if not tree.leaf[i] and i in costs:
            applies += 1
            leaf_cost, c = Q * tree.count[i], costs[i]
            if abs(c - leaf_cost) <= tau_of(i) * leaf_cost:
                fragile += 1
            elif c >= leaf_cost:
                mine = 1
        refines[i] = up + mine
        if tree.leaf[i] and refines[i] > params.max_bad_refines:
            bad.append("the path to leaf %d holds %d bad refines, maxBadRefines is %d" % (i, refines[i], params.max_bad_refines))
    rep.share["bad_refines_max"] = int(refines.max()) if tree.n else 0
    if not params.retract:
        for i in tree.leaves:
            n = tree.count[i]
            if i in costs and tree.depth[i] < params.max_depth and n > params.stop_prims:
                applies += 1
                c = costs[i]
                if np.isfinite(c) and abs(c - Q * n) <= tau_of(i) * Q * n:
                    fragile += 1
                elif c < Q * n and cost_fragile[i]:
                    fragile += 1
                elif c < Q * n:
                    bad.append("leaf %d holds %d primitives and a plane of cost %.17g < %.17g was there to split it" % (i, n, c, Q * n))
    else:
        whole = prims.n <= params.exact_prim_threshold
        sub = np.zeros(tree.n)
        for i in reversed(tree.order):
            n = len(tree.sets[i])
            if tree.leaf[i]:
                sub[i] = Q * n; continue
            l = tree.left[i]
            with np.errstate(all="ignore"):
                pl, pr = _probabilities(tree.lo[i], tree.hi[i], tree.axis[i], tree.split[i])
            sub[i] = params.traversal_cost + pl * sub[l] + pr * sub[l + 1]                   # gkdtree.h:2321-2324
            if whole or (tree.exact[i] and not tree.minmax[i]):
                applies += 1
                tol = 2 * gamma(15 * int(tree.height[i]) + 2)
                if abs(sub[i] - Q * n) <= tol * Q * n:
                    fragile += 1
                elif sub[i] >= Q * n:
                    bad.append("inner node %d survives with a subtree cost of %.17g >= %.17g, the cost of a leaf" % (i, sub[i], Q * n))
    rep.left_out["termination"] = (fragile, applies)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the min-max phase above the threshold
# ---------------------------------------------------------------------------------------------------------------------
def _binned(params, tlo, thi, mn, mx):
    """the binned costs of gkdtree.h:2405-2470 in binary64 from geometric counts: over the minMaxBins - 1 inner boundaries of
    every axis of the tight box, a primitive counts left when its box begins below the boundary and right when it ends at or
    above it -> per axis (boundaries, costs, left [b][n], right [b][n]), and whether a face lies within two binary32 steps of
    a boundary"""
    nb = params.min_max_bins
    out, near = [], False
    for a in range(3):
        x = tlo[a] + (np.arange(1, nb) / nb) * (thi[a] - tlo[a])
        x = x[(x > tlo[a]) & (x < thi[a])]
        left, right = mn[None, :, a] < x[:, None], mx[None, :, a] >= x[:, None]
        pl, pr = _probabilities(tlo, thi, a, x)
        cost = params.traversal_cost + params.query_cost * (pl * left.sum(axis=1) + pr * right.sum(axis=1))
        out.append((x, cost, left, right))
        if len(x):
            faces = np.concatenate([mn[:, a], mx[:, a]])
            step = 2 * np.spacing(np.abs(faces).astype(F)).astype(np.float64)
            near |= bool((np.abs(faces[None, :] - x[:, None]) <= step[None, :]).any())
    return out, near


def check_minmax(prims, tree, params, rep):
    bad = rep.violations["minmax"]
    tau = 2 * gamma(K_COST + params.min_max_bins)
    applies = fragile = 0
    worst = 0.0
    if not hasattr(tree, "min_cost"):
        tree.min_cost, tree.cost_fragile = {}, {}
    for i, r in tree.reach.items():
        tlo, thi = tree.tight[i]
        with np.errstate(all="ignore"):
            axes, near = _binned(params, tlo, thi, prims.lo[r], prims.hi[r])
        best = min([float(c.min()) for _, c, _, _ in axes if len(c)] + [np.inf])
        tree.min_cost[i], tree.cost_fragile[i] = best, near
        if tree.leaf[i]:
            continue
        applies += 1
        a, s, l = tree.axis[i], tree.split[i], tree.left[i]
        found = None
        if not (tlo[a] < s < thi[a]):
            found = "node %d: its plane %d @ %.9g is not strictly inside its tight box %.9g .. %.9g" % (i, a, s, tlo[a], thi[a])
        else:
            x, cost, left, right = axes[a]
            in_l, in_r = np.isin(r, tree.reach_all[l]), np.isin(r, tree.reach_all[l + 1])
            same = (left == in_l[None, :]).all(axis=1) & (right == in_r[None, :]).all(axis=1)
            if not same.any():
                found = "node %d: no bin boundary of axis %d parts its primitives as its plane @ %.9g does" % (i, a, s)
            else:
                c = float(cost[same].min())
                if c > best * (1 + tau):
                    found = ("node %d: the boundary behind plane %d @ %.9g costs %.17g, the best boundary %.17g (ratio - 1 = %.3g, tau %.3g)"
                             % (i, a, s, c, best, c / best - 1, tau))
                else:
                    worst = max(worst, (c / best - 1) / tau)
        if found and near:
            fragile += 1
        elif found:
            bad.append(found)
    rep.left_out["minmax"] = (fragile, applies)
    rep.share["minmax_excess_over_tau"] = worst


# ---------------------------------------------------------------------------------------------------------------------
# 6. statistics and the enlarged box
# ---------------------------------------------------------------------------------------------------------------------
def enlarged_box(prims):
    """gkdtree.h:1170-1176 in float32: the maximum moves by the extent measured from the already-moved minimum"""
    lo, hi = prims.box_lo.astype(F), prims.box_hi.astype(F)
    lo2 = lo - ((hi - lo) * EPSILON + EPSILON)
    hi2 = hi + ((hi - lo2) * EPSILON + EPSILON)
    return lo2, hi2


def expected_stats(tree):
    """gkdtree.h:1100-1125, :1178-1181 in binary64 -> dict of the six figures and the number of terms of the three sums"""
    e = tree.hi - tree.lo
    area = 2.0 * (e[:, 0] * e[:, 1] + e[:, 0] * e[:, 2] + e[:, 1] * e[:, 2])
    count = (tree.end - tree.start).astype(np.float64)
    inner, leaves = np.array(tree.inner, dtype=np.int64), np.array(tree.leaves, dtype=np.int64)
    root = area[0]
    with np.errstate(all="ignore"):
        out = dict(inner=float(len(inner)), leaf=float(len(leaves)), indices=float(count[leaves].sum()),
                   exp_traversals=float(area[inner].sum() / root), exp_leaves=float(area[leaves].sum() / root),
                   exp_prims=float((area[leaves] * count[leaves]).sum() / root))
    return out, dict(exp_traversals=len(inner), exp_leaves=len(leaves), exp_prims=len(leaves) + 1)


def check_stats(prims, tree, params, rep, stats=None, aabb_min=None, aabb_max=None):
    bad = rep.violations["stats"]
    if stats is not None:
        want, terms = expected_stats(tree)
        for k in ("inner", "leaf", "indices"):
            if stats[k] != want[k]:
                bad.append("%s: %r, the tree holds %r" % (k, stats[k], want[k]))
        worst = 0.0
        for k, n in terms.items():
            bound = gamma(n + K_AREA) * want[k]
            err = abs(stats[k] - want[k])
            if not np.isfinite(want[k]):                     # a flat scene box has no area to divide by
                continue
            if err > bound:
                bad.append("%s: %.9g, recomputed %.17g, off by %.3g > %.3g" % (k, stats[k], want[k], err, bound))
            if bound > 0:
                worst = max(worst, err / bound)
        rep.share["stats_error_over_bound"] = worst
    if aabb_min is not None:
        lo, hi = enlarged_box(prims)
        if not (np.array_equal(lo.view(np.uint32), np.asarray(aabb_min, dtype=F).view(np.uint32))
                and np.array_equal(hi.view(np.uint32), np.asarray(aabb_max, dtype=F).view(np.uint32))):
            bad.append("the enlarged box is %s .. %s, the mirror gives %s .. %s" % (list(aabb_min), list(aabb_max), lo.tolist(), hi.tolist()))
    rep.left_out["stats"] = (0, 8)


# ---------------------------------------------------------------------------------------------------------------------
def check(prims, arrays, params, stats=None):
    """arrays: kd_nodes, kd_indices, aabb_min, aabb_max as arrays() gives them; stats: kdstats() as a dict -> Report"""
    rep = Report()
    if prims.n == 0:
        return rep
    tree = Tree(prims, arrays["kd_nodes"], arrays["kd_indices"], params)
    rep.tree = tree
    rep.violations["structure"] = tree.errors
    check_coverage(prims, tree, params, rep)
    check_tightness(prims, tree, params, rep)
    check_sah(prims, tree, params, rep)
    check_minmax(prims, tree, params, rep)
    check_termination(prims, tree, params, rep)
    check_stats(prims, tree, params, rep, stats, arrays.get("aabb_min"), arrays.get("aabb_max"))
    return rep


STAT_KEYS = ("inner", "leaf", "indices", "exp_traversals", "exp_leaves", "exp_prims")


def stats_dict(s):
    """kdstats() of the product (a dict) or of the oracle (a list)"""
    return dict(s) if isinstance(s, dict) else dict(zip(STAT_KEYS, s))
