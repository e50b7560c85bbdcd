"""Scenes, rays and cells that hold the cylinder shape (include/mtsgpu_cylinder.h) against tests/ref64_cyl.py, and the glue
that puts cylinders into the tree-free brute force of tests/ref64_geom.py (imported, not copied: its triangle and sphere
records, its clip against the scene's box and its tie logic run as they are; the cylinders join the spheres' columns).
Test infrastructure."""
import contextlib

import numpy as np

import ref64_cyl as R
import ref64_geom as G
from ref64_sky import E

F = np.float32
INF = np.inf
EPS = G.EPSILON
MISS = 0xFFFFFFFF
SCENES = ("one", "mixed", "thin", "cross")
# poses of the constructor tests: (name, p1, p2, radius)
POSES = (("axis_aligned", (0.0, 0.0, 0.0), (0.0, 0.0, 2.0), 0.5), ("diagonal", (-0.4, 0.3, 0.1), (0.9, 1.2, -0.7), 0.25),
         ("minus_z", (0.2, -0.1, 1.0), (0.2, -0.1, -1.5), 0.75), ("along_x", (1.0, 2.0, 3.0), (4.0, 2.0, 3.0), 0.1),
         ("tilted", (0.5, -1.0, 0.25), (0.8, 1.1, 0.6), 0.4))
# the poses whose axis is parallel to a coordinate axis: every face of (getAABB() clipped to a cell) that is a face of getAABB()
# is tangent to the tube, so the edge roots of Cylinder::intersectCylFace sit on the sign of a discriminant that is zero
AXIS_PARALLEL = ("axis_aligned", "minus_z", "along_x")
# a toWorld with unequal scales and a shear
SHEARED = np.array([[0.6, 0.2, 0.1, 0.3], [0.0, 0.5, 0.4, -0.2], [0.1, 0.0, 1.7, 0.5], [0, 0, 0, 1]], dtype=np.float32)


def scene_description(mts, name):
    sd = mts.scenes.SceneDescription("cyl_" + name)
    grey = sd.lambertian(0.5)
    rng = np.random.RandomState(7 + SCENES.index(name))
    if name == "one":
        sd.add_cylinder((-0.4, 0.3, 0.1), (0.9, 1.2, -0.7), 0.25, bsdf=grey)
    elif name == "mixed":
        sd.add_cylinder((0.0, 0.0, -1.0), (0.0, 0.0, 1.0), 0.5, bsdf=grey)
        sd.add_sphere((1.2, 0.1, 0.2), 0.4, bsdf=grey)
        c = rng.rand(12, 1, 3) * 3 - 1.5
        tris = c + 0.6 * (rng.rand(12, 3, 3) * 2 - 1)
        sd.add_mesh(tris.reshape(-1, 3), np.arange(36).reshape(-1, 3), bsdf=grey, face_normals=True)
    elif name == "thin":
        # a grid of 64 triangles in the plane y = 0 and a thin cylinder through it on a diagonal
        g = np.linspace(-1, 1, 9)
        tris = []
        for i in range(8):
            for j in range(4):
                x0, x1, z0, z1 = g[i], g[i + 1], g[2 * j], g[2 * j + 2]
                tris += [[(x0, 0, z0), (x1, 0, z0), (x1, 0, z1)], [(x0, 0, z0), (x1, 0, z1), (x0, 0, z1)]]
        tris = np.array(tris, dtype=np.float64)
        sd.add_mesh(tris.reshape(-1, 3), np.arange(3 * len(tris)).reshape(-1, 3), bsdf=grey, face_normals=True)
        sd.add_cylinder((-1.1, -0.9, -1.0), (1.0, 0.8, 1.1), 0.03, bsdf=grey)
    elif name == "cross":
        sd.add_cylinder((-1.0, 0.0, 0.0), (1.0, 0.1, 0.0), 0.2, bsdf=grey)
        sd.add_cylinder((0.0, -1.0, 0.05), (0.1, 1.0, 0.0), 0.25, bsdf=grey)
        sd.add_cylinder((0.05, 0.0, -1.0), (0.0, 0.1, 1.0), 0.3, bsdf=grey)
    sd.add_lum(mts.abi.LUM_POINT, [1, 1, 1])
    return sd


def kd_params(mts, name, n_threads=1):
    kp = mts.abi.KdParams()
    kp.n_threads = n_threads
    if name == "thin":
        kp.stop_prims = 1           # clipping decides the leaf lists
    return kp


# ---------------------------------------------------------------------------------------------------------------------
# the brute force with cylinders
# ---------------------------------------------------------------------------------------------------------------------
class Geometry(G.Geometry):
    """G.Geometry with the cylinders of the description: they join the spheres' primitive list behind the spheres"""

    def __init__(self, sd, aabb_min, aabb_max, blocks):
        tris, tprim, sph, sprim, cyl, cprim, occ = [], [], [], [], [], [], []
        p = 0
        for s, m in enumerate(sd.meshes):
            if getattr(m, "cylinder", None) is not None:
                cyl.append(np.asarray(blocks[s], dtype=np.float32)); cprim.append(p); occ.append(m.bsdf >= 0); p += 1
            elif m.sphere is not None:
                sph.append(list(m.sphere[0]) + [m.sphere[1]]); sprim.append(p); occ.append(m.bsdf >= 0); p += 1
            else:
                v = m.positions.astype(np.float64)[m.triangles.astype(np.int64)]
                tris.append(v); tprim += range(p, p + len(v)); occ += [m.bsdf >= 0] * len(v); p += len(v)
        self.n_prims = p
        self.tri = np.concatenate(tris) if tris else np.zeros((0, 3, 3))
        self.tri_prim = np.array(tprim, dtype=np.int64)
        self.sph = np.array(sph, dtype=np.float64).reshape(-1, 4)
        self.cyl = cyl
        self.cyl_prim = np.array(cprim, dtype=np.int64)
        self.sph_prim = np.concatenate([np.array(sprim, dtype=np.int64), self.cyl_prim])
        self.occluder = np.array(occ, dtype=bool)
        self.is_sphere = np.zeros(p, dtype=bool); self.is_sphere[self.sph_prim] = True
        self.aabb_min = np.asarray(aabb_min, dtype=np.float32).astype(np.float64)
        self.aabb_max = np.asarray(aabb_max, dtype=np.float32).astype(np.float64)
        with np.errstate(all="ignore"):
            self._load()


@contextlib.contextmanager
def _cylinders_in_the_brute_force():
    original = G._spheres

    def both(geom, O, D, mint, maxt, closest):
        out = original(geom, O, D, mint, maxt, closest)
        if not getattr(geom, "cyl", None):
            return out
        rays = np.zeros((len(O), 8), dtype=np.float32); rays[:, 0:3] = O; rays[:, 4:7] = D
        cols = {k: [] for k in ("accepted", "undecided", "tv", "te", "far")}
        for block in geom.cyl:
            # the interval keeps its own bound: a threshold against mint or maxt is judged with both
            r = R.intersect64(block, rays, mint.v, maxt.v, shadow=not closest)
            und = r["fragile"] | R._close(r["t"], mint) & r["hit"] | R._close(r["t"], maxt) & r["hit"]
            cols["accepted"].append(r["hit"] & ~und); cols["undecided"].append(und)
            cols["tv"].append(r["t"].v); cols["te"].append(r["t"].e); cols["far"].append(np.full(len(O), np.nan))
        st = lambda k: np.stack(cols[k], axis=1)
        cat = lambda a, b: np.concatenate([a, b], axis=1)
        t = E(cat(out["t"].v, st("tv")), cat(out["t"].e, st("te")))
        near = E(cat(out["near"].v, st("tv")), cat(out["near"].e, st("te")))
        far = E(cat(out["far"].v, st("far")), cat(out["far"].e, st("far")))
        return dict(accepted=cat(out["accepted"], st("accepted")), undecided=cat(out["undecided"], st("undecided")), t=t, far=far, near=near)
    G._spheres = both
    try:
        yield
    finally:
        G._spheres = original


def trace(geom, rays, shadow=False):
    with _cylinders_in_the_brute_force():
        return G.trace(geom, rays, shadow=shadow)


# ---------------------------------------------------------------------------------------------------------------------
# the binary32 mirror of the prologue of ShapeKDTree::rayIntersect (skdtree.cpp:108-124 / :180-194) and the brute force over
# cylinders alone
# ---------------------------------------------------------------------------------------------------------------------
def clip32(aabb_min, aabb_max, rays, closest):
    """AABB::rayIntersect (aabb.h:349-382), the adaptive epsilon and the interval test -> mint, maxt, enters (binary32)"""
    R8 = np.asarray(rays, dtype=np.float32).reshape(-1, 8)
    lo, hi = np.asarray(aabb_min, dtype=np.float32), np.asarray(aabb_max, dtype=np.float32)
    n = len(R8)
    with np.errstate(all="ignore"):
        mint = np.full(n, -INF, dtype=np.float32); maxt = np.full(n, INF, dtype=np.float32)
        go = np.ones(n, dtype=bool)
        for i in range(3):
            d, o = R8[:, 4 + i], R8[:, i]
            rc = F(1) / d
            zero = d == 0
            go &= ~(zero & ((o < lo[i]) | (o > hi[i])))
            t1 = (lo[i] - o) * rc; t2 = (hi[i] - o) * rc
            sw = t1 > t2
            t1, t2 = np.where(sw, t2, t1), np.where(sw, t1, t2)
            mint = np.where(zero, mint, np.where(mint < t1, t1, mint)).astype(np.float32)      # std::max(mint, t1)
            maxt = np.where(zero, maxt, np.where(t2 < maxt, t2, maxt)).astype(np.float32)      # std::min(maxt, t2)
            go &= zero | ~(mint > maxt)
        ray_min = R8[:, 3].copy()
        m = np.maximum(np.maximum(np.abs(R8[:, 0]), np.abs(R8[:, 1])), np.abs(R8[:, 2]))
        if closest:
            m = np.maximum(m, F(EPS))
        ray_min = np.where(ray_min == F(EPS), ray_min * m, ray_min).astype(np.float32)
        mint = np.where(ray_min > mint, ray_min, mint).astype(np.float32)
        maxt = np.where(R8[:, 7] < maxt, R8[:, 7], maxt).astype(np.float32)
        go &= maxt > mint
    return mint, maxt, go


def brute32(blocks, prims, aabb_min, aabb_max, rays, shadow=False):
    """the binary32 answer of a scene of cylinders alone -> (hit, t, prim, tied): every cylinder is tested with the interval
    the smaller hits have left, which gives the smallest accepted t (see the module text of ref64_cyl.py); tied = two
    cylinders offer that t, where the leaf order decides"""
    mint, maxt, go = clip32(aabb_min, aabb_max, rays, not shadow)
    n = len(mint)
    best = np.full(n, INF, dtype=np.float32); prim = np.full(n, -1, dtype=np.int64)
    tied = np.zeros(n, dtype=bool); any_hit = np.zeros(n, dtype=bool)
    for block, p in zip(blocks, prims):
        hit, t = R.intersect32(block, rays, mint, maxt, shadow=shadow)
        hit &= go
        if shadow:
            any_hit |= hit
            continue
        tied |= hit & (t == best)
        better = hit & (t < best)
        tied &= ~better
        best = np.where(better, t, best).astype(np.float32); prim = np.where(better, p, prim)
    if shadow:
        return any_hit, None, None, tied
    return prim >= 0, best, prim, tied


# ---------------------------------------------------------------------------------------------------------------------
# rays
# ---------------------------------------------------------------------------------------------------------------------
def _rays(o, d, mint=EPS, maxt=INF):
    o = np.asarray(o, dtype=np.float64).reshape(-1, 3); d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    r = np.zeros((len(o), 8), dtype=np.float32)
    r[:, 0:3] = o; r[:, 3] = mint; r[:, 4:7] = d; r[:, 7] = maxt
    return r


def random_rays(block, n, seed, mint=EPS):
    """from a sphere of radius 3 about the cylinder's middle towards uniform points of a box 0.2 to 0.3 larger than it"""
    rng = np.random.RandomState(seed)
    D = np.asarray(block, dtype=np.float64)
    M = D[0:12].reshape(3, 4)
    r, l = D[24], D[25]
    mid = M[:, :3] @ np.array([0, 0, l / 2]) + M[:, 3]
    o = rng.normal(size=(n, 3)); o = mid + 3.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    pad = 0.2 + 0.1 * rng.rand(n, 1)
    loc = (rng.rand(n, 3) * 2 - 1) * (np.array([r, r, l / 2]) + pad) + np.array([0, 0, l / 2])
    tgt = loc @ M[:, :3].T + M[:, 3]
    d = tgt - o; d /= np.linalg.norm(d, axis=1, keepdims=True)
    return _rays(o, d, mint)


def named_rays(block):
    """-> dict name: (ray [8], what the closest-hit form must say: True / False / None = a threshold case left to the mirror)"""
    D = np.asarray(block, dtype=np.float64)
    M = D[0:12].reshape(3, 4)
    r, l = D[24], D[25]
    P = lambda x, y, z: M[:, :3] @ np.array([x, y, z]) + M[:, 3]
    V = lambda x, y, z: M[:, :3] @ np.array([x, y, z])
    out = {}
    out["along_axis_inside"] = (_rays(P(0.1 * r, 0, 0.1 * l), V(0, 0, 1))[0], False)          # A == 0: the linear case returns false
    out["inside_looking_out"] = (_rays(P(0.2 * r, 0.1 * r, 0.5 * l), V(1, 0.3, 0.1))[0], True)      # the far root
    out["on_surface_mint_below"] = (_rays(P(r, 0, 0.5 * l), V(-1, 0.2, 0), mint=1e-6)[0], None)
    out["on_surface_mint_above"] = (_rays(P(r, 0, 0.5 * l), V(-1, 0.2, 0), mint=1e-2)[0], True)
    out["through_both_ends"] = (_rays(P(0.1 * r, 0, -1.0), V(0.02 * r, 0, 1.0) / (l + 2))[0], False)
    far = _rays(P(3 * r, 0, 0.5 * l), V(-1, 0, 0), maxt=3 * r)                                         # maxt between the roots
    out["maxt_between_roots"] = (far[0], True)
    out["tangent"] = (_rays(P(r, -3, 0.5 * l), V(0, 1, 0))[0], None)
    out["parallel_outside"] = (_rays(P(2 * r, 0, -1), V(0, 0, 1))[0], False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cells of the clip tests, and the walk over a flattened tree
# ---------------------------------------------------------------------------------------------------------------------
def cells(block, own):
    """own = getAABB [6] -> dict name: cell [6]"""
    own = np.asarray(own, dtype=np.float64).copy()
    lo, hi = own[:3], own[3:]
    mid = 0.5 * (lo + hi)
    D = np.asarray(block, dtype=np.float64)
    M = D[0:12].reshape(3, 4)
    r, l = D[24], D[25]
    out = {"own": own.copy()}
    for a in range(3):
        c = own.copy(); c[3 + a] = mid[a]; out["lower_half_%d" % a] = c
        c = own.copy(); c[a] = mid[a]; out["upper_half_%d" % a] = c
        c = own.copy(); c[a] = mid[a] - 0.2 * r; c[3 + a] = mid[a] + 0.2 * r; out["slab_%d" % a] = c      # thinner than the radius
    for k in range(8):
        c = own.copy()
        for a in range(3):
            if (k >> a) & 1: c[a] = mid[a]
            else: c[3 + a] = mid[a]
        out["eighth_%d" % k] = c
    centre = M[:, :3] @ np.array([0, 0, l / 2]) + M[:, 3]
    h = 0.3 * r / np.sqrt(3)
    out["inside_tube"] = np.concatenate([centre - h, centre + h])                # wholly inside: the surface misses it
    out["outside"] = np.concatenate([hi + 0.5, hi + 1.0])                        # misses the cylinder's own box
    corner = np.concatenate([lo, lo + 0.02 * (hi - lo)])                         # a corner of the box the surface may miss
    out["corner"] = corner
    return {k: v.astype(np.float32) for k, v in out.items()}


def leaves(scene):
    """the leaves of a flattened scene's tree -> list of (lo [3], hi [3], primitive ids) with binary64 cell bounds"""
    sc = scene.sc
    nodes = np.ctypeslib.as_array(sc.kd_nodes, shape=(2 * sc.n_nodes,)).reshape(-1, 2).copy()
    idx = np.ctypeslib.as_array(sc.kd_indices, shape=(max(sc.n_indices, 1),)).copy()
    out = []
    stack = [(0, np.array(list(sc.aabb_min), dtype=np.float64), np.array(list(sc.aabb_max), dtype=np.float64))]
    while stack:
        i, lo, hi = stack.pop()
        a, b = int(nodes[i, 0]), int(nodes[i, 1])
        if a & 0x80000000:
            out.append((lo, hi, idx[(a & 0x7FFFFFFF):b].tolist()))
            continue
        axis, left = a & 3, i + ((a & 0x3FFFFFFC) >> 2)
        split = float(np.array([b], dtype=np.uint32).view(np.float32)[0])
        lhi = hi.copy(); lhi[axis] = split
        rlo = lo.copy(); rlo[axis] = split
        stack.append((left, lo, lhi)); stack.append((left + 1, rlo, hi))
    return out


def tree_words(scene):
    sc = scene.sc
    return (np.ctypeslib.as_array(sc.kd_nodes, shape=(2 * sc.n_nodes,)).copy(), np.ctypeslib.as_array(sc.kd_indices, shape=(max(sc.n_indices, 1),))[:sc.n_indices].copy())


# ---------------------------------------------------------------------------------------------------------------------
# the properties of tests/ref64_kd.py on trees with cylinders
# ---------------------------------------------------------------------------------------------------------------------
def kd_prims(K, sd, blocks):
    """ref64_kd.Prims of a description with cylinders: a cylinder is a primitive that is neither a triangle nor a sphere, with the
    float32 box of Cylinder::getAABB (the mirror's); its clipped boxes come from kd_clip below"""
    class _Rest:
        pass
    plain = _Rest(); plain.meshes = [m for m in sd.meshes if getattr(m, "cylinder", None) is None]
    base = K.Prims(plain)                                    # the triangles and spheres, numbered without the cylinders
    first, p, q = [], 0, 0
    shift = np.zeros(base.n, dtype=np.int64)
    cyl_prim, cyl_block = [], []
    for s, m in enumerate(sd.meshes):
        if getattr(m, "cylinder", None) is not None:
            cyl_prim.append(p); cyl_block.append(np.asarray(blocks[s], dtype=np.float32)); p += 1
        else:
            n = 1 if m.sphere is not None else len(m.triangles)
            shift[q:q + n] = p - q; q += n; p += n
    prims = base
    old = np.arange(base.n) + shift                          # old number -> number in the scene with cylinders
    prims.n = p
    prims.tri_prim = old[base.tri_prim] if len(base.tri_prim) else base.tri_prim
    prims.sph_prim = old[base.sph_prim] if len(base.sph_prim) else base.sph_prim
    lo, hi = np.zeros((p, 3)), np.zeros((p, 3))
    lo[old] = base.lo; hi[old] = base.hi
    for k, b in zip(cyl_prim, cyl_block):
        own = R.aabb32(b).astype(np.float64)
        lo[k], hi[k] = own[:3], own[3:]
    prims.lo, prims.hi = lo, hi
    prims.tri_of = np.full(p, -1, dtype=np.int64); prims.tri_of[prims.tri_prim] = np.arange(len(prims.tri_prim))
    prims.box_lo, prims.box_hi = lo.min(axis=0), hi.max(axis=0)
    prims.cyl = dict(zip(cyl_prim, cyl_block))
    return prims


@contextlib.contextmanager
def kd_clip(K, prims):
    """ref64_kd.clipped_boxes with Cylinder::getClippedAABB for the cylinders: the binary32 mirror (the builders' boxes are binary32
    values, and the checker's own triangle clip rounds to them as well), kept = valid and of non-zero area"""
    original = K.clipped_boxes

    def with_cylinders(p, ids, lo, hi):
        blo, bhi, kept = original(p, ids, lo, hi)
        for j in np.nonzero(np.isin(ids, list(getattr(p, "cyl", {}))))[0]:
            box, valid = R.clipped32(p.cyl[int(ids[j])], np.concatenate([lo[j], hi[j]]).astype(np.float32))
            d = (box[3:] - box[:3]).astype(np.float32) if valid else np.zeros(3, dtype=np.float32)
            area = F(2.0) * (d[0] * d[1] + d[0] * d[2] + d[1] * d[2])
            blo[j], bhi[j], kept[j] = box[:3], box[3:], bool(valid and area > 0)
        return blo, bhi, kept
    K.clipped_boxes = with_cylinders
    try:
        yield
    finally:
        K.clipped_boxes = original


def kd_report(K, mts, sd, scene, kp):
    prims = kd_prims(K, sd, scene.cylinder_blocks())
    arrays = {k: scene.arrays()[k] for k in ("kd_nodes", "kd_indices", "aabb_min", "aabb_max")}
    with kd_clip(K, prims):
        return K.check(prims, arrays, K.Params(kp, prims.n), K.stats_dict(scene.kdstats())), prims


def leaf_membership(scene, block):
    """which leaves a cylinder belongs to, replayed from the root with the mirror's clip as the builder's exact phase classifies a
    primitive (gkdtree.h:2053-2103, :2140-2219): its current box against the plane -- ends at or before it: left only; begins at or
    behind it: right only; lies in it: either side (the cheaper one, not decided here); straddles it: clipped anew to each child's
    cell, dropped where that box is invalid or has no area.  -> list of (lo, hi, ids, member) per leaf, member True / False / None"""
    sc = scene.sc
    nodes = np.ctypeslib.as_array(sc.kd_nodes, shape=(2 * sc.n_nodes,)).reshape(-1, 2).copy()
    idx = np.ctypeslib.as_array(sc.kd_indices, shape=(max(sc.n_indices, 1),)).copy()

    def clipped(lo, hi):
        box, valid = R.clipped32(block, np.concatenate([lo, hi]).astype(np.float32))
        d = (box[3:] - box[:3]).astype(np.float32) if valid else np.zeros(3, dtype=np.float32)
        ok = bool(valid and F(2.0) * (d[0] * d[1] + d[0] * d[2] + d[1] * d[2]) > 0)
        return (box.astype(np.float64) if ok else None)
    out = []
    lo0 = np.array(list(sc.aabb_min), dtype=np.float64); hi0 = np.array(list(sc.aabb_max), dtype=np.float64)
    stack = [(0, lo0, hi0, clipped(lo0, hi0), False)]          # node, cell, the cylinder's box in it (None: not here), undecided
    while stack:
        i, lo, hi, box, maybe = stack.pop()
        a, b = int(nodes[i, 0]), int(nodes[i, 1])
        if a & 0x80000000:
            out.append((lo, hi, idx[(a & 0x7FFFFFFF):b].tolist(), None if (maybe and box is not None) else box is not None))
            continue
        axis, left = a & 3, i + ((a & 0x3FFFFFFC) >> 2)
        split = float(np.array([b], dtype=np.uint32).view(np.float32)[0])
        lhi = hi.copy(); lhi[axis] = split
        rlo = lo.copy(); rlo[axis] = split
        if box is None:
            bl = br = None; ml = mr = maybe
        else:
            mn, mx = box[axis], box[3 + axis]
            if mn == mx == split: bl = br = box; ml = mr = True
            elif mx <= split: bl, br = box, None; ml = mr = maybe
            elif mn >= split: bl, br = None, box; ml = mr = maybe
            else: bl, br = clipped(lo, lhi), clipped(rlo, hi); ml = mr = maybe
        stack.append((left, lo, lhi, bl, ml)); stack.append((left + 1, rlo, hi, br, mr))
    return out
