"""Scenes, rays and hand-built kd-trees that hold a float32 traversal (the oracle's in the CPU suite, the device's in
the GPU suite) against tests/ref64_geom.py, and the comparison itself.  Test infrastructure.

The geometric answer does not depend on the tree, so the same primitives are put under trees shaped to force the rare
paths of k_trace: the root as a leaf, a chain as deep as mtsgpu_upload_scene accepts (stack spills), a median tree that
fits the LDS copy of the top of the tree and one that reaches past the breadth-first prefix into the treelets.  A leaf
lists every primitive whose bounding box, padded by PAD of the scene's extent, overlaps its cell: a conservative list
is a valid tree, and the padding keeps a hit whose float32 entry / exit points fall on the other side of a split plane
inside the list of the leaf the traversal visits."""
import os
import re

import numpy as np

import ref64_geom as G
from closed_forms import K_VALUE, MAX_AMBIGUOUS          # noqa: F401  (re-exported for the tests)
from conftest import chord_rays
from ref64 import EPS32

F = np.float32
INF = np.inf
EPS = G.EPSILON
NR = 500                      # rays per class and scene
PAD = 1e-4
MISS = 0xFFFFFFFF

# |got - truth| <= K_GEOM x 2^-23 x bound for t, u and v of every compared ray.  Measured over every scene x ray class x
# tree of the CPU suite (the oracle against the truth, tests/test_geom_truth.py, which fails when this figure goes stale):
# the worst ratio is 0.495, t of a ray of class "edges" in scene "spheres" (the same under every tree); the worst per
# scene lies between 0.23 and 0.50.  K_GEOM leaves the factor of five closed_forms.K_VALUE documents.  0.495 is below
# K_VALUE / 5 = 3.2: the first-order bounds of ref64_geom are not optimistic.  The device is held to the same K_GEOM.
WORST_MEASURED = 0.495
K_GEOM = 5 * WORST_MEASURED

# Ray classes that exist to be ambiguous: only "at least a quarter is still compared" is asked of them
AMBIGUOUS_BY_DESIGN = ("edges", "tangent")
# Named, counted classes of decided rays on which the reference's own algorithm departs from the tree-free truth:
# (name, cause in one sentence, selector).  None was found.
EXCEPTIONS = []

SCENES = ("axes", "slivers", "soup", "soup_far", "soup_small", "fan", "twins", "degenerate", "spheres")
TREES = ("sah", "one_leaf", "chain", "median_small", "median_large")


# ---------------------------------------------------------------------------------------------------------------------
# what kernels.h fixes: the depth of the traversal stack and the size of the top of the tree (not reachable from Python)
# ---------------------------------------------------------------------------------------------------------------------
def kernel_constants():
    """kStackLDS + kSpillLevels (trace_stack_levels), 2 * kTopPairs (the LDS copy) and kTopNodes (trace_top_nodes) as
    mitsuba-renderer_amd/csrc/kernels.h defines them for the product build"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mitsuba-renderer_amd", "csrc", "kernels.h")
    src = open(path).read()
    lds = int(re.search(r"#define MG_STACK_LDS (\d+)", src).group(1))
    total = int(re.search(r"kSpillLevels = (\d+) - kStackLDS", src).group(1))
    block = int(re.search(r"#define MG_TRACE_BLOCK (\d+)", src).group(1))
    big, small = re.search(r"#define MG_TOP_PAIRS \(MG_TRACE_BLOCK >= 512 \? (\d+) : (\d+)\)", src).groups()
    pairs = int(big) if block >= 512 else int(small)
    mult = int(re.search(r"kTopNodes = (\d+) \* kTopPairs", src).group(1))
    return dict(stack_levels=total, stack_lds=lds, lds_nodes=2 * pairs, top_nodes=mult * pairs, block=block)


def chain_levels():
    """inner nodes of the deepest chain mtsgpu_upload_scene accepts: it refuses an inner node at depth
    trace_stack_levels() - 2 (root = depth 1)"""
    return kernel_constants()["stack_levels"] - 3


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def _frame(n):
    n = n / np.linalg.norm(n)
    a = np.array([1.0, 0, 0]) if abs(n[0]) < 0.6 else np.array([0, 1.0, 0])
    s = np.cross(n, a); s /= np.linalg.norm(s)
    return s, np.cross(n, s)


def _planar_triangle(rng, normal, centre, size):
    s, t = _frame(np.asarray(normal, dtype=np.float64))
    ang = rng.rand() * 2 * np.pi + np.array([0.0, 2.1, 4.2]) + rng.rand(3) * 0.8
    rad = size * (0.5 + 0.5 * rng.rand(3))
    return centre + (np.cos(ang) * rad)[:, None] * s + (np.sin(ang) * rad)[:, None] * t


def _soup(rng, count, size=0.5):
    c = rng.rand(count, 1, 3) * 2 - 1
    return c + size * (rng.rand(count, 3, 3) * 2 - 1)


def _mesh(sd, tris, bsdf):
    tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    sd.add_mesh(tris.reshape(-1, 3), np.arange(3 * len(tris)).reshape(-1, 3), bsdf=bsdf, face_normals=True)


def scene_description(mts, name):
    rng = np.random.RandomState(SCENES.index(name) + 100)
    sd = mts.scenes.SceneDescription("geom_" + name)
    grey = sd.lambertian(0.5)
    if name == "axes":
        # normals along each axis (both directions) and within 1e-3 of a tie between two dominant axes: every ordered
        # pair (a dominant, b second) gives all three projection cases k and both sides of every choice
        tris = []
        for a in range(3):
            for sign in (1.0, -1.0):
                for _ in range(4):
                    c = rng.rand(3) * 2 - 1
                    c[a] = float(F(c[a]))
                    tri = _planar_triangle(rng, np.eye(3)[a] * sign, c, 0.5)
                    tri[:, a] = c[a]                      # exactly in the plane: the other two components of N are exact zeros
                    tris.append(tri)
        for a in range(3):
            for b in range(3):
                if a != b:
                    n = np.full(3, 0.3); n[a] = 1.0; n[b] = 1.0 - 1e-3
                    for sign in (1.0, -1.0):
                        for _ in range(3):
                            tris.append(_planar_triangle(rng, n * sign, rng.rand(3) * 2 - 1, 0.5))
        _mesh(sd, tris, grey)
    elif name == "slivers":
        # aspect ratio 1e4: 0.25 long, 2.5e-5 high, in a plane normal to a coordinate axis with the long edge along another.
        # (In general position the normal N and the denominator of TriAccel::load are differences of nearly equal
        # products: binary32 knows such a sliver's plane to about 1e-3 rad and its b_nu .. c_nv to about 1e-3 of values
        # that cancel to four digits in u and v, so no ray at it is decidable and ref64_geom says so.)
        tris = list(_soup(rng, 40))
        for i in range(18):
            a = i % 3
            c = np.float32(rng.rand(3) * 2 - 1).astype(np.float64)
            s, t = _frame(np.eye(3)[a])
            if i % 2:
                s, t = t, s
            tri = np.stack([c, c + 0.25 * s, c + 0.125 * s + 2.5e-5 * t])
            tri[:, a] = c[a]
            tris.append(tri)
        _mesh(sd, tris, grey)
    elif name.startswith("soup"):
        tris = _soup(np.random.RandomState(7), 10, size=0.3) * 6.0       # the same soup three times
        if name == "soup_far":
            tris = tris + np.array([1000.0, -800.0, 600.0])
        if name == "soup_small":
            tris = tris * 1e-3
        _mesh(sd, tris, grey)
    elif name == "fan":
        # a closed double fan: 16 triangles around an apex, 16 around the centre of the base, every edge shared
        off = np.array([0.3, -0.2, 0.1])
        ang = 0.1 + np.arange(16) * np.pi / 8
        ring = np.stack([np.cos(ang), np.sin(ang), np.zeros(16)], axis=1) + off
        pos = np.concatenate([ring, [off + [0, 0, 1.0]], [off]])
        rot = np.array([[1, 0, 0], [0, np.cos(0.3), -np.sin(0.3)], [0, np.sin(0.3), np.cos(0.3)]])
        roty = np.array([[np.cos(0.2), 0, np.sin(0.2)], [0, 1, 0], [-np.sin(0.2), 0, np.cos(0.2)]])
        pos = pos @ rot.T @ roty.T                        # no face contains a coordinate direction
        idx = [[i, (i + 1) % 16, 16] for i in range(16)] + [[(i + 1) % 16, i, 17] for i in range(16)]
        sd.add_mesh(pos, np.array(idx), bsdf=grey, face_normals=True)
    elif name == "twins":
        base = _soup(rng, 40)
        _mesh(sd, np.concatenate([base, base, base[:, [0, 2, 1], :]]), grey)     # coplanar duplicates, reversed winding
    elif name == "degenerate":
        base = _soup(rng, 100)
        pos = base.reshape(-1, 3)
        idx = np.arange(300).reshape(-1, 3).tolist()
        idx += [[3 * i, 3 * i, 3 * i + 1 + (i & 1)] for i in range(0, 100, 5)]   # zero area: the first vertex repeated
        order = rng.permutation(len(idx))
        sd.add_mesh(pos, np.array(idx)[order], bsdf=grey, face_normals=True)
    elif name == "spheres":
        sd.add_sphere((0.0, -100.6, 0.0), 100.0, bsdf=grey)
        sd.add_sphere((0.0, 0.5, 0.0), 1.0, bsdf=grey)
        sd.add_sphere((1.6, 0.2, 0.3), 0.01, bsdf=grey)
        _mesh(sd, _soup(rng, 40) * 2, grey)
        quad = lambda h, z: [[[-h, -h + 2, z], [h, -h + 2, z], [h, h + 2, z]], [[-h, -h + 2, z], [h, h + 2, z], [-h, h + 2, z]]]
        _mesh(sd, quad(1.5, 3.5), -1)                     # no BSDF: no occluder (Shape::isOccluder) ...
        _mesh(sd, quad(0.5, 3.0), grey)                   # ... in front of a smaller occluder
        sd.add_sphere((-2.0, 2.0, 3.0), 0.3, bsdf=-1)
    else:
        raise KeyError(name)
    sd.point_light((0.0, 5.0, 0.0), 1.0)                  # a scene needs a luminaire (scene.cpp:310-318)
    return sd


# ---------------------------------------------------------------------------------------------------------------------
# trees
# ---------------------------------------------------------------------------------------------------------------------
class Tree:
    def __init__(self, nodes, indices, splits):
        self.nodes = np.array(nodes, dtype=np.uint32).reshape(-1, 2)
        self.indices = np.array(indices if len(indices) else [0], dtype=np.uint32)
        self.n_indices = len(indices)
        self.splits = splits                              # (axis, value) of the inner nodes, root first


def _bits(x):
    return int(np.array([x], dtype=np.float32).view(np.uint32)[0])


def _boxes(geom):
    lo = np.zeros((geom.n_prims, 3)); hi = np.zeros((geom.n_prims, 3))
    lo[geom.tri_prim] = geom.tri.min(axis=1); hi[geom.tri_prim] = geom.tri.max(axis=1)
    lo[geom.sph_prim] = geom.sph[:, 0:3] - np.abs(geom.sph[:, 3:4]); hi[geom.sph_prim] = geom.sph[:, 0:3] + np.abs(geom.sph[:, 3:4])
    pad = PAD * (geom.aabb_max - geom.aabb_min).max()
    return lo - pad, hi + pad


def _grow(geom, rule):
    """rule(level, on_chain, lo, hi, cand) -> (axis, split, left_on_chain, right_on_chain) or None for a leaf"""
    blo, bhi = _boxes(geom)
    nodes, indices, splits = [[0, 0]], [], []
    todo = [(0, geom.aabb_min.copy(), geom.aabb_max.copy(), np.arange(geom.n_prims), 0, True)]
    while todo:
        i, lo, hi, cand, level, on = todo.pop(0)
        r = rule(level, on, lo, hi, cand)
        if r is None:
            nodes[i] = [0x80000000 | len(indices), len(indices) + len(cand)]
            indices += cand.tolist()
            continue
        axis, s, on_l, on_r = r
        s = float(F(s))
        left = len(nodes)
        nodes += [[0, 0], [0, 0]]
        nodes[i] = [axis | ((left - i) << 2), _bits(s)]
        splits.append((axis, s))
        hl, lr = hi.copy(), lo.copy()
        hl[axis] = s; lr[axis] = s
        todo.append((left, lo, hl, cand[blo[cand, axis] <= s], level + 1, on_l))
        todo.append((left + 1, lr, hi, cand[bhi[cand, axis] >= s], level + 1, on_r))
    return Tree(nodes, indices, splits)


def one_leaf(geom):
    return _grow(geom, lambda *a: None)


def chain(geom, levels):
    """a left-deep chain of `levels` inner nodes: level j splits axis j % 3 at 1 - (j + 1) / (levels + 1) of the box, the
    upper part is a leaf, the lower part goes on.  A ray up the diagonal of the box finds its exit point above every
    split and pushes at every level; the same ray reversed pops at every level."""
    lo0, hi0 = geom.aabb_min, geom.aabb_max

    def rule(level, on, lo, hi, cand):
        if not on or level >= levels:
            return None
        a = level % 3
        return a, lo0[a] + (1 - (level + 1) / (levels + 1)) * (hi0[a] - lo0[a]), True, False
    return _grow(geom, rule)


def median(geom, depth):
    """balanced median splits cycling the axes, `depth` levels of inner nodes everywhere (2^(depth+1) - 1 nodes): the
    median of the candidates' box centres, or the middle of a cell that holds none"""
    blo, bhi = _boxes(geom)

    def rule(level, on, lo, hi, cand):
        if level >= depth:
            return None
        a = level % 3
        s = np.median(0.5 * (blo[cand, a] + bhi[cand, a])) if len(cand) else 0.5 * (lo[a] + hi[a])
        s = float(F(s))
        if not (lo[a] < s < hi[a]):
            s = 0.5 * (lo[a] + hi[a])
        return a, s, True, True
    return _grow(geom, rule)


def tree_depths():
    """depths of the two median trees: the small one lies wholly inside the LDS copy (fewer than 2 * kTopPairs nodes),
    the large one has more than 2 * trace_top_nodes() nodes (LDS copy, breadth-first prefix and treelets)"""
    k = kernel_constants()
    small = int(np.floor(np.log2(k["lds_nodes"]))) - 1
    large = int(np.floor(np.log2(2 * k["top_nodes"])))
    assert 2 ** (small + 1) - 1 < k["lds_nodes"] and 2 ** (large + 1) - 1 > 2 * k["top_nodes"]
    return small, large


def build_tree(geom, kind):
    if kind == "one_leaf":
        return one_leaf(geom)
    if kind == "chain":
        return chain(geom, chain_levels())
    small, large = tree_depths()
    return median(geom, small if kind == "median_small" else large)


def with_tree(mts, scene_struct, tree):
    """a copy of a mtsgpu_scene with the tree substituted (as test_malformed_trees_are_refused hands trees in)"""
    cp = mts.abi.Scene.from_buffer_copy(scene_struct)
    cp.kd_nodes = mts.abi.ptr(tree.nodes, mts.abi.u32p); cp.n_nodes = len(tree.nodes)
    cp.kd_indices = mts.abi.ptr(tree.indices, mts.abi.u32p); cp.n_indices = tree.n_indices
    cp.keep = tree
    return cp


# ---------------------------------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------------------------------
def _rays(o, d, mint=EPS, maxt=INF):
    r = np.zeros((len(o), 8), dtype=np.float32)
    r[:, 0:3] = o; r[:, 3] = mint; r[:, 4:7] = d; r[:, 7] = maxt
    return r


def _aim(o, target, mint=EPS, maxt=INF):
    """float32 origins, unit float32 directions towards the targets (components that are exactly 0 stay 0)"""
    o = np.asarray(o, dtype=np.float32)
    d = np.asarray(target, dtype=np.float32).astype(np.float64) - o.astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return _rays(o, d, mint, maxt)


def _unit(rng, n):
    v = rng.randn(n, 3)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


class _Targets:
    """random points of random primitives.  A sliver's TriAccel plane is known to binary32 only to about 1e-3 rad (its
    normal is the difference of nearly equal products), which moves an oblique ray's hit point by many sliver widths: slivers
    are aimed at along their normal and near their middle, and the classes that fix the ray's direction by other means
    (`oblique`) aim at the well-shaped triangles only."""

    def __init__(self, geom, rng):
        self.g, self.rng = geom, rng
        ok = ~geom.degenerate
        self.tris = geom.tri[ok]
        T = self.tris
        edge = np.stack([np.linalg.norm(T[:, (i + 1) % 3] - T[:, i], axis=1) for i in range(3)]).max(axis=0)
        area2 = np.linalg.norm(np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0]), axis=1)
        self.thin = area2 / edge ** 2 < 1e-2 if len(T) else np.zeros(0, dtype=bool)
        self.size = float(np.linalg.norm(geom.aabb_max - geom.aabb_min))

    def interior(self, n, spheres=True, oblique=False):
        """-> points, outward directions (a side from which the point is visible)"""
        rng, g = self.rng, self.g
        ns = (n // 4 if len(self.tris) else n) if (spheres and len(g.sph)) else 0
        pool = np.nonzero(~self.thin)[0] if oblique else np.arange(len(self.tris))
        pick = pool[rng.randint(len(pool), size=n - ns)]
        T, thin = self.tris[pick], self.thin[pick][:, None]
        w = np.where(thin, 0.25 + 0.25 * rng.dirichlet([1, 1, 1], size=n - ns),
                     0.1 + 0.7 * rng.dirichlet([1, 1, 1], size=n - ns))           # every weight >= 0.1 (slivers: >= 0.25)
        p = (w[:, :, None] * T).sum(axis=1)
        nrm = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        side = nrm * np.where(rng.rand(n - ns, 1) < 0.5, 1.0, -1.0) + np.where(thin, 0.01, 0.7) * _unit(rng, n - ns)
        if ns:
            S = g.sph[rng.randint(len(g.sph), size=ns)]
            dirs = _unit(rng, ns)
            p = np.concatenate([p, S[:, 0:3] + S[:, 3:4] * dirs])
            side = np.concatenate([side, dirs + 0.5 * _unit(rng, ns)])
        return p, side / np.linalg.norm(side, axis=1, keepdims=True)

    def edges(self, n):
        """points within 1e-6 (relative to the triangle) of edges and vertices, either side; two in five within 1e-2"""
        rng = self.rng
        T = self.tris[rng.randint(len(self.tris), size=n)]
        w = rng.dirichlet([1, 1, 1], size=n)
        w[:, 0] = 0; w /= w.sum(axis=1, keepdims=True)                  # on the edge B-C
        vert = rng.rand(n) < 0.3
        w[vert] = [0, 0, 1.0]
        w += (rng.rand(n, 3) * 2 - 1) * np.where(np.arange(n) % 5 < 2, 1e-2, 1e-6)[:, None]      # two in five stay decidable
        roll = rng.randint(3, size=n)
        w = np.stack([np.roll(w[i], roll[i]) for i in range(n)])
        p = (w[:, :, None] * T).sum(axis=1)
        nrm = np.cross(T[:, 1] - T[:, 0], T[:, 2] - T[:, 0])
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        side = nrm * np.where(rng.rand(n, 1) < 0.5, 1.0, -1.0) + 0.7 * _unit(rng, n)
        return p, side / np.linalg.norm(side, axis=1, keepdims=True)


def ray_classes(geom, splits, seed):
    """dict class -> rays [n][8]; `splits` = (axis, value) of inner nodes of a supplied tree"""
    rng = np.random.RandomState(seed)
    tg = _Targets(geom, rng)
    lo, hi = geom.aabb_min, geom.aabb_max
    centre, radius = 0.5 * (lo + hi), 0.5 * float(np.linalg.norm(hi - lo))
    inside = lambda n: lo + (hi - lo) * (0.02 + 0.96 * rng.rand(n, 3))
    # how far from its target a ray starts: the scene's radius, or a few primitive sizes where one huge primitive sets the
    # radius (a sphere seen from a hundred radii away is a badly conditioned quadratic in any precision)
    blo, bhi = _boxes(geom)
    dist = min(radius, 6.0 * float(np.median((bhi - blo).max(axis=1))))
    out = {}
    out["chords"] = chord_rays(NR, centre, radius, seed)
    p, side = tg.interior(NR)
    out["interior"] = _aim(p + side * dist * (0.3 + rng.rand(NR, 1)), p)
    if len(tg.tris):
        p, side = tg.edges(NR)
        out["edges"] = _aim(p + side * dist * (0.3 + rng.rand(NR, 1)), p)
    # one or two direction components exactly 0: origin and target share those coordinates
    p, _ = tg.interior(NR, oblique=True)
    p = p.astype(np.float32).astype(np.float64)
    keep = rng.rand(NR, 3) < 0.5
    keep[keep.all(axis=1)] = [True, False, True]
    keep[~keep.any(axis=1)] = [False, True, False]
    o = np.where(keep, p, p + np.where(rng.rand(NR, 3) < 0.5, 1.0, -1.0) * dist * (0.2 + rng.rand(NR, 3)))
    out["axis"] = _aim(o, p)
    # origins exactly on a split plane of the supplied tree and on the faces of the scene's box
    p, _ = tg.interior(NR, oblique=True)
    o = inside(NR)
    for i in range(NR):
        if i % 2 and splits:
            a, s = splits[rng.randint(min(len(splits), 64))]
            o[i, a] = s
        else:
            a = rng.randint(3)
            o[i, a] = (lo, hi)[rng.randint(2)][a]
            if i % 4 == 0:
                p[i, a] = o[i, a]                          # along the face
    out["planes"] = _aim(o, p)
    # origins inside the box, aimed at primitives; origins outside, pointing away
    p, _ = tg.interior(NR, oblique=True)
    r_in = _aim(inside(NR // 2), p[:NR // 2])
    o = centre + _unit(rng, NR - NR // 2) * radius * 1.5
    out["inout"] = np.concatenate([r_in, _aim(o, o + (o - centre))])
    # maxt short of and beyond the hit, mint beyond the hit: 12 bounds away (decided), a few one bound away (ambiguous)
    p, side = tg.interior(NR)
    base = _aim(p + side * dist * (0.3 + rng.rand(NR, 1)), p)
    tr = G.trace(geom, base)
    t, bound = tr.t[:, 0], EPS32 * tr.te[:, 0]
    ok = tr.hit & ~tr.ambiguous & np.isfinite(bound)
    step = np.where(np.arange(NR) % 64 == 0, 1.0, 3.0 * G.REACH) * bound
    kind = np.arange(NR) % 3
    lim = base[ok].copy()
    lim[:, 7] = np.where(kind == 0, t - step, np.where(kind == 1, t + step, INF))[ok]
    lim[:, 3] = np.where(kind == 2, t + step, EPS)[ok]
    out["limits"] = lim
    # shadow segments as Scene::isOccluded forms them: d = p2 - p1, mint = 1e-3, maxt = 1 - 1e-3
    p, side = tg.interior(NR, oblique=True)
    off = max(1e-3 * dist, 2e-5 * float(np.abs(np.concatenate([lo, hi])).max()))     # well clear of the surface in binary32
    p1 = (p + side * off).astype(np.float32)
    p2 = np.where(rng.rand(NR, 1) < 0.5, inside(NR), p + side * dist * rng.rand(NR, 1)).astype(np.float32)
    out["shadow"] = _rays(p1, p2.astype(np.float64) - p1.astype(np.float64), 1e-3, 1 - 1e-3)
    if len(geom.sph):
        S = geom.sph[rng.randint(len(geom.sph), size=NR)]
        c, rad = S[:, 0:3], S[:, 3:4]
        dirs = _unit(rng, NR)
        o_in = c + dirs * rad * 0.9 * rng.rand(NR, 1)
        o_in[::3] = c[::3]                                  # at the centre
        r1 = _aim(o_in, o_in + _unit(rng, NR))
        r1[1::4, 7] = (0.05 * rad[1::4, 0]).astype(np.float32)     # inside, maxt short of the far root: no hit
        o_out = c + dirs * (rad * 3 + 0.5)
        r2 = _aim(o_out, c)
        r2[:, 7] = np.linalg.norm(o_out - c, axis=1)        # maxt between the two roots
        out["sphere"] = np.concatenate([r1[:NR // 2], r2[:NR // 2]])
        # tangent rays: most pass 1e-3 of the radius inside or outside, a quarter 1e-7 (undecidable)
        perp = np.cross(dirs, _unit(rng, NR)); perp /= np.linalg.norm(perp, axis=1, keepdims=True)
        delta = np.where(np.arange(NR) % 4 == 0, 1e-7, 1e-3) * np.where(rng.rand(NR) < 0.5, 1.0, -1.0)
        out["tangent"] = _aim(o_out, c + perp * rad * (1 + delta[:, None]))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# a case: scene, geometry, trees, rays and the truth, built once and shared
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    pass


_CASES = {}


def case(mts, name):
    if name in _CASES:
        return _CASES[name]
    c = Case()
    c.name = name
    c.sd = scene_description(mts, name)
    c.scene = mts.Scene(c.sd)                                # the product's flattener: TriAccel records and the SAH tree
    c.geom = G.Geometry(c.sd, list(c.scene.sc.aabb_min), list(c.scene.sc.aabb_max))
    assert c.geom.n_prims == c.scene.sc.n_tris
    c.trees = {k: build_tree(c.geom, k) for k in TREES if k != "sah"}
    c.classes = ray_classes(c.geom, c.trees["median_small"].splits, seed=SCENES.index(name) + 1)
    # the diagonal of the box, both ways: pushes at every level of the chain, pops at every level
    lo, hi = c.geom.aabb_min, c.geom.aabb_max
    diag = _aim(np.stack([lo + 1e-3 * (hi - lo), hi - 1e-3 * (hi - lo)]), np.stack([hi, lo]))
    c.classes["chords"] = np.concatenate([diag, c.classes["chords"]])
    c.names = list(c.classes)
    c.rays = np.concatenate([c.classes[k] for k in c.names])
    ends = np.cumsum([len(c.classes[k]) for k in c.names])
    c.slices = {k: slice(e - len(c.classes[k]), e) for k, e in zip(c.names, ends)}
    c.forms = {}
    c.closest = G.trace(c.geom, c.rays, shadow=False, check_forms=c.forms)
    c.shadow = G.trace(c.geom, c.rays, shadow=True)
    _CASES[name] = c
    return c


# ---------------------------------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------------------------------
def check_closest(truth, hits, what="", K=None):
    """hits [n][4] u32 as mtsgpu_trace_rays returns them.  -> (failures, worst): worst[x] = (ratio |got - truth| / bound,
    ray) over the compared rays, x in t, u, v"""
    K = K_GEOM if K is None else K
    hits = np.ascontiguousarray(hits, dtype=np.uint32)
    t, u, v = (hits[:, i].copy().view(np.float32).astype(np.float64) for i in range(3))
    prim = hits[:, 3].astype(np.int64)
    miss = hits[:, 3] == MISS
    dec = ~truth.ambiguous
    failures, worst = [], {}

    def report(bad, text):
        if bad.any():
            i = int(np.nonzero(bad)[0][0])
            failures.append("%s: %s on %d rays, e.g. ray %d: got t %.9g u %.9g v %.9g prim %d, truth hit %s prims %s t %s"
                            % (what, text, bad.sum(), i, t[i], u[i], v[i], prim[i], truth.hit[i], truth.prim[i].tolist(), truth.t[i].tolist()))
    report(dec & (miss == truth.hit), "hit / miss differs from the truth")
    match = truth.prim == np.where(miss, -2, prim)[:, None]
    named = match.any(axis=1)
    report(dec & truth.hit & ~miss & ~named, "the primitive is not one of the truth's tied set")
    sel = dec & truth.hit & ~miss & named
    col = np.argmax(match, axis=1)
    rows = np.arange(len(t))
    for name, got in (("t", t), ("u", u), ("v", v)):
        ref, bound = getattr(truth, name)[rows, col], getattr(truth, name + "e")[rows, col]
        with np.errstate(all="ignore"):
            diff = np.abs(got - ref)
            ratio = np.where(diff == 0, 0.0, diff / (EPS32 * bound))
        ratio = np.where(np.isfinite(got), ratio, np.inf)
        ratio = np.where(sel & ~np.isinf(bound), np.nan_to_num(ratio, nan=np.inf), 0.0)
        i = int(np.argmax(ratio)) if len(ratio) else 0
        worst[name] = (float(ratio[i]) if len(ratio) else 0.0, i)
        if len(ratio) and ratio[i] > K:
            failures.append("%s: %s off by %.3g bounds > K = %.3g at ray %d: got %.9g truth %.9g bound %.3g x 2^-23 (prim %d)"
                            % (what, name, ratio[i], K, i, got[i], ref[i], bound[i], prim[i]))
    # ambiguous rays came back, finite or a miss, naming a primitive they pass within reach of
    for i in np.nonzero(truth.ambiguous)[0]:
        if not miss[i] and not (np.isfinite(t[i]) and int(prim[i]) in truth.possible[i]):
            failures.append("%s: ambiguous ray %d returned t %.9g prim %d, within reach are %s"
                            % (what, i, t[i], prim[i], sorted(truth.possible[i])[:8]))
            break
    return failures, worst


def check_shadow(truth, hits, what=""):
    flag = np.ascontiguousarray(hits, dtype=np.uint32)[:, 3]
    failures = []
    if (flag > 1).any():
        failures.append("%s: any-hit flags other than 0 / 1" % what)
    bad = ~truth.ambiguous & ((flag != 0) != truth.hit)
    if bad.any():
        i = int(np.nonzero(bad)[0][0])
        failures.append("%s: the any-hit flag differs from the truth on %d rays, e.g. ray %d: got %d, truth %s"
                        % (what, bad.sum(), i, flag[i], truth.hit[i]))
    return failures
