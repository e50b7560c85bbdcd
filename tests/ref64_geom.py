"""A binary64 restatement of the geometry queries: where a ray hits a set of triangles and spheres, with no kd-tree.
Written from the reference's sources, not from csrc/ or oracle/:
    TriAccel::load, TriAccel::rayIntersect      include/mitsuba/render/triaccel.h:63-96, :98-159
    Sphere::rayIntersect, both overloads        src/shapes/sphere.cpp:92-113, :115-131; solveQuadratic src/libcore/util.cpp:450-488
    ShapeKDTree::rayIntersect, both overloads   src/librender/skdtree.cpp:108-132, :180-199; AABB::rayIntersect
                                                include/mitsuba/core/aabb.h:349-382; Ray::dRcp include/mitsuba/core/ray.h:63-74
    ShapeKDTree::intersect (occluders)          include/mitsuba/render/skdtree.h:243-336
Conventions of tests/ref64_sky.py: float32 inputs promoted exactly, every quantity a pair (value, first-order bound of the
error of a binary32 evaluation in the reference's operation order, in units of 2^-23) -- the class E of that module.  The
bound of a triangle hit therefore covers the rounding of the precomputed TriAccel record as well as of the intersection.
Test infrastructure.

The geometric answer does not depend on the tree: rayIntersectHavran (sahkdtree3.h:170-300) hands every primitive of every
leaf it visits to intersect() with the ray's whole clipped interval [mint, maxt] (:272-283), lowers maxt to each accepted
t, and leaves when the exit distance of a leaf lies beyond maxt (:290).  Over a valid tree the result is the accepted
primitive of smallest t, or for a shadow ray whether any occluder is accepted.

What a sphere hit stores as (u, v): nothing.  ShapeKDTree::intersect leaves cache->u / cache->v untouched for a
non-triangle shape (skdtree.h:287-296) and Sphere::fillIntersectionRecord derives its uv from the hit point
(sphere.cpp:133-145).  They are not geometric: for spheres only t and the primitive are compared.

A record (ray, primitive) is ACCEPTED when all its acceptance tests hold by more than REACH bounds, REJECTED when one of
them fails by more than REACH bounds, UNDECIDED otherwise.  A ray is ambiguous when an undecided record could change its
answer or when the clip against the scene's box is within REACH bounds of deciding the other way.

Degenerate triangles: load() sets k = 3 and returns when denom == 0 (triaccel.h:80-83); rayIntersect's switch then takes
`default: return false` (:134-135): a zero-area triangle never hits.  Here a triangle is degenerate when denom is exactly
zero with an exactly zero bound (a repeated first vertex: b or c is the zero vector and every product is exact); a
triangle whose denom or whose choice of k lies within reach of its bound is refused (Geometry raises), because a first-
order bound cannot say what binary32 makes of it."""
import numpy as np

from ref64 import EPS32
from ref64_sky import E, _sqrt, _where, REACH

EPSILON = float(np.float32(1e-4))          # constants.h:31
WALD = np.array([1, 2, 0, 1])              # waldModulo, triaccel.h:64
CHUNK = 512                                # rays per block of the rays x primitives arrays
AGREE = 2.0 ** -38                         # the two binary64 forms agree to AGREE x (bound + |value|), the bound in units of 1
                                           # instead of 2^-23: 2^15 below what binary32 is granted
_TINY = 1e-300


def _pick(three, idx):
    return E(np.choose(idx, [x.v for x in three]), np.choose(idx, [x.e for x in three]))


def _scale(a, s):
    """multiplication by a power of two: exact"""
    return E(a.v * s, a.e * abs(s))


def _close(a, b):
    """a and b within REACH of their bounds of each other"""
    with np.errstate(invalid="ignore"):
        return np.isfinite(a.v) & np.isfinite(b.v) & (np.abs(a.v - b.v) <= REACH * EPS32 * (a.e + b.e))


class Geometry:
    """the primitives of a scene description in the index space of ShapeKDTree (skdtree.cpp:43-65: the shapes' triangles
    in order, every other shape one primitive) and the TriAccel record of every triangle"""

    def __init__(self, sd, aabb_min, aabb_max):
        tris, tprim, sph, sprim, occ = [], [], [], [], []
        p = 0
        for m in sd.meshes:
            if m.sphere is not None:
                sph.append(list(m.sphere[0]) + [m.sphere[1]]); sprim.append(p); occ.append(m.bsdf >= 0); p += 1
            else:
                v = m.positions.astype(np.float64)[m.triangles.astype(np.int64)]
                tris.append(v); tprim += range(p, p + len(v)); occ += [m.bsdf >= 0] * len(v); p += len(v)
        self.n_prims = p
        self.tri = np.concatenate(tris) if tris else np.zeros((0, 3, 3))
        self.tri_prim = np.array(tprim, dtype=np.int64)
        self.sph = np.array(sph, dtype=np.float64).reshape(-1, 4)
        self.sph_prim = np.array(sprim, dtype=np.int64)
        self.occluder = np.array(occ, dtype=bool)            # Shape::isOccluder: has a BSDF (skdtree.h:329-333)
        self.is_sphere = np.zeros(p, dtype=bool); self.is_sphere[self.sph_prim] = True
        self.aabb_min = np.asarray(aabb_min, dtype=np.float32).astype(np.float64)
        self.aabb_max = np.asarray(aabb_max, dtype=np.float32).astype(np.float64)
        with np.errstate(all="ignore"):
            self._load()

    def _load(self):
        """TriAccel::load (triaccel.h:63-96) for every triangle"""
        T = self.tri
        A, B, C = ([E(T[:, j, i]) for i in range(3)] for j in range(3))
        b = [C[i] - A[i] for i in range(3)]; c = [B[i] - A[i] for i in range(3)]                     # :66
        N = [c[1] * b[2] - c[2] * b[1], c[2] * b[0] - c[0] * b[2], c[0] * b[1] - c[1] * b[0]]        # cross(c, b)
        absN = np.stack([np.abs(x.v) for x in N])
        k = np.argmax(absN, axis=0)                                                                  # :68-73, first maximum wins
        ku, kv = WALD[k], WALD[k + 1]                                                                # :75-76
        n_k = _pick(N, k)
        denom = _pick(b, ku) * _pick(c, kv) - _pick(b, kv) * _pick(c, ku)                            # :78
        self.degenerate = (denom.v == 0) & (denom.e == 0)                                            # :80-83
        undecided = ~self.degenerate & (np.abs(denom.v) <= REACH * EPS32 * denom.e)
        for j in range(3):
            other = (k != j) & ~self.degenerate
            undecided |= other & (np.abs(absN[j] - np.abs(n_k.v)) <= REACH * EPS32 * (N[j].e + n_k.e))
        if undecided.any():
            raise ValueError("triangles %s: binary32 cannot decide their projection axis or whether they are degenerate"
                             % np.nonzero(undecided)[0][:8].tolist())
        self.k, self.ku, self.kv = k, ku, kv
        self.n_u = _pick(N, ku) / n_k; self.n_v = _pick(N, kv) / n_k                                 # :86-87
        self.n_d = (A[0] * N[0] + A[1] * N[1] + A[2] * N[2]) / n_k                                   # :88
        self.b_nu = _pick(b, ku) / denom; self.b_nv = -_pick(b, kv) / denom                          # :89-90
        self.a_u = _pick(A, ku); self.a_v = _pick(A, kv)                                             # :91-92
        self.c_nu = _pick(c, kv) / denom; self.c_nv = -_pick(c, ku) / denom                          # :93-94


def _row(x):
    return E(x.v[None, :], x.e[None, :])


def _col(x):
    return E(x.v[:, None], x.e[:, None])


def _margin(num, bound):
    return num / (EPS32 * bound + _TINY)


def clip(geom, rays, closest):
    """the common prologue of ShapeKDTree::rayIntersect (skdtree.cpp:108-124 / :180-194): AABB::rayIntersect
    (aabb.h:349-382), the adaptive epsilon, the interval test.  -> mint, maxt (E [n]), enters [n], ambiguous [n]"""
    R = np.asarray(rays, dtype=np.float32).astype(np.float64)
    O, D = R[:, 0:3], R[:, 4:7]
    n = len(R)
    near, far = E(np.full(n, -np.inf)), E(np.full(n, np.inf))
    miss = np.zeros(n, dtype=bool)
    for i in range(3):
        par = D[:, i] == 0                                                                           # :359-362
        miss |= par & ((O[:, i] < geom.aabb_min[i]) | (O[:, i] > geom.aabb_max[i]))
        rc = 1.0 / E(np.where(par, 1.0, D[:, i]))                                                    # ray.h:68-70
        t1 = (geom.aabb_min[i] - E(O[:, i])) * rc; t2 = (geom.aabb_max[i] - E(O[:, i])) * rc         # :365-366
        swap = t1.v > t2.v
        t1, t2 = _where(swap, t2, t1), _where(swap, t1, t2)
        near = _where(~par & (t1.v > near.v), t1, near); far = _where(~par & (t2.v < far.v), t2, far)  # :374-375
    amb_box = _close(near, far) & ~miss                   # a miss by a parallel slab is an exact comparison
    miss |= near.v > far.v                                                                           # :377-378
    eps_ray = R[:, 3] == EPSILON                                                                     # skdtree.cpp:116-119 / :187-189
    m = np.abs(O).max(axis=1)
    if closest:
        m = np.maximum(m, EPSILON)                        # only the (ray, its) overload has the inner max
    ray_min = _where(eps_ray, E(np.full(n, EPSILON)) * E(m), E(R[:, 3]))
    mint = _where(ray_min.v > near.v, ray_min, near)                                                 # :121
    maxt = _where(R[:, 7] < far.v, E(R[:, 7]), far)                                                  # :122
    enters = ~miss & (maxt.v > mint.v)                                                               # :124
    return mint, maxt, enters, amb_box | (_close(mint, maxt) & ~miss)


def _triangles(geom, O, D, mint, maxt):
    """TriAccel::rayIntersect (triaccel.h:98-159) for rays [r] x triangles [t] -> dict of [r][t] arrays"""
    g = geom
    o_u, o_v, o_k = O[:, g.ku], O[:, g.kv], O[:, g.k]                                                # :108-133
    d_u, d_v, d_k = D[:, g.ku], D[:, g.kv], D[:, g.k]
    n_u, n_v, n_d = _row(g.n_u), _row(g.n_v), _row(g.n_d)
    den = E(d_u) * n_u + E(d_v) * n_v + E(d_k)                                                       # :141
    parallel = (den.v == 0) & (den.e == 0)
    recip = 1.0 / den
    t = (n_d - E(o_u) * n_u - E(o_v) * n_v - E(o_k)) * recip                                         # :142
    hu = E(o_u) + t * E(d_u) - _row(g.a_u)                                                           # :152-153
    hv = E(o_v) + t * E(d_v) - _row(g.a_v)
    u = hv * _row(g.b_nu) + hu * _row(g.b_nv)                                                        # :156-157
    v = hu * _row(g.c_nu) + hv * _row(g.c_nv)
    uv = u + v
    mn, mx = _col(mint), _col(maxt)
    margins = np.stack([_margin(t.v - mn.v, t.e + mn.e),                                             # t >= mint   (:148)
                        _margin(mx.v - t.v, t.e + np.where(np.isfinite(mx.v), mx.e, 0.0)),           # t <= maxt
                        _margin(u.v, u.e), _margin(v.v, v.e),                                        # u >= 0, v >= 0 (:158)
                        _margin(1.0 - uv.v, uv.e)])                                                  # u + v <= 1
    never = parallel | g.degenerate[None, :]                                                         # :134-135
    rej = (margins < -REACH).any(axis=0) | never
    acc = (margins > REACH).all(axis=0) & ~never
    return dict(t=t, u=u, v=v, margins=margins, accepted=acc, undecided=~(acc | rej), never=never)


def moller_trumbore(geom, O, D):
    """the second, independent binary64 form: Moeller-Trumbore straight from the three vertices (u weighs B, v weighs C,
    as TriAccel's do: triaccel.h:89-94 with b = C - A, c = B - A) -> t, u, v [r][t]"""
    A = geom.tri[None, :, 0, :]; e1 = geom.tri[None, :, 1, :] - A; e2 = geom.tri[None, :, 2, :] - A
    d = D[:, None, :]
    p = np.cross(d, e2)
    det = (e1 * p).sum(axis=-1)
    tv = O[:, None, :] - A
    q = np.cross(tv, e1)
    return (e2 * q).sum(axis=-1) / det, (tv * p).sum(axis=-1) / det, (d * q).sum(axis=-1) / det


def _spheres(geom, O, D, mint, maxt, closest):
    """Sphere::rayIntersect (sphere.cpp:92-113 closest, :115-131 any hit) over solveQuadratic (util.cpp:450-488) for rays
    [r] x spheres [s] -> accepted, undecided, t (the reported root) and the far root, [r][s]"""
    ctr, rad = geom.sph[:, 0:3], geom.sph[:, 3]
    o = [E(O[:, i, None]) - E(ctr[None, :, i]) for i in range(3)]                                    # :93
    d = [E(D[:, i, None]) for i in range(3)]
    A = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]                                                      # :94
    B = _scale(d[0] * o[0] + d[1] * o[1] + d[2] * o[2], 2.0)                                         # :95
    Cq = o[0] * o[0] + o[1] * o[1] + o[2] * o[2] - E(rad[None, :]) * E(rad[None, :])                 # :96
    disc = B * B - _scale(A, 4.0) * Cq                                                               # util.cpp:460
    none = disc.v < 0                                                                                # :463-464
    und = np.abs(disc.v) <= REACH * EPS32 * disc.e
    sq = _sqrt(_where(none, 1.0, disc))
    temp = _scale(_where(B.v < 0, B - sq, B + sq), -0.5)                                             # :475-478
    x0, x1 = temp / A, Cq / temp                                                                     # :480-481
    swap = x0.v > x1.v                                                                               # :484-485
    near, far = _where(swap, x1, x0), _where(swap, x0, x1)
    mn, mx = _col(mint), _col(maxt)
    outside = (near.v > mx.v) | (far.v < mn.v)                                                       # sphere.cpp:102 / :125
    und |= _close(near, mx) | _close(far, mn)
    inside = near.v < mn.v                                                                           # :104 / :127
    und |= _close(near, mn) & ~outside if closest else _close(near, mn) & (far.v > mx.v) & ~outside
    both = inside & (far.v > mx.v)                                                                   # :105 / :127
    und |= inside & _close(far, mx) & ~outside
    hit = ~none & ~outside & ~both
    und |= ~(np.isfinite(near.v) & np.isfinite(far.v)) & ~none
    t = _where(inside, far, near)                                                                    # :107-109
    return dict(accepted=hit & ~und, undecided=und, t=t, far=far, near=near)


class Truth:
    """the per-ray answer.  closest: hit, ambiguous, enters, and the tied set -- the accepted primitives whose t lies within
    reach of the smallest accepted t (one normally; several for coplanar duplicates and shared edges) -- as padded
    arrays [n][m]: prim (-1 = unused), t, u, v and their bounds te, ue, ve (units of 2^-23), far (the sphere's other root).
    possible[i] = every primitive ray i passes within reach of (accepted or undecided records).  shadow: occluded."""


def trace(geom, rays, shadow=False, check_forms=None):
    """brute force over rays [n][8] (o, mint, d, maxt: the layout of mtsgpu_trace_rays) x all primitives.  check_forms: a
    dict that receives the worst disagreement of the two binary64 triangle forms, in units of AGREE x (bound + |value|)"""
    with np.errstate(all="ignore"):
        return _trace(geom, rays, shadow, check_forms)


def _trace(geom, rays, shadow, check_forms):
    R = np.asarray(rays, dtype=np.float32).astype(np.float64).reshape(-1, 8)
    n = len(R)
    mint, maxt, enters, camb = clip(geom, R, not shadow)
    out = Truth()
    out.n, out.enters, out.clip_ambiguous = n, enters, camb
    out.ambiguous = camb.copy()
    out.hit = np.zeros(n, dtype=bool)
    out.possible = [()] * n
    prim_ids = np.concatenate([geom.tri_prim, geom.sph_prim])
    occ = geom.occluder[prim_ids]
    tied = []
    for s in range(0, n, CHUNK):
        e = min(n, s + CHUNK)
        O, D = R[s:e, 0:3], R[s:e, 4:7]
        mn, mx = E(mint.v[s:e], mint.e[s:e]), E(maxt.v[s:e], maxt.e[s:e])
        tr = _triangles(geom, O, D, mn, mx)
        sp = _spheres(geom, O, D, mn, mx, not shadow)
        if check_forms is not None and len(geom.tri):
            t2, u2, v2 = moller_trumbore(geom, O, D)
            dec = ~tr["undecided"] & ~tr["never"] & enters[s:e, None]
            for name, a, b in (("t", tr["t"], t2), ("u", tr["u"], u2), ("v", tr["v"], v2)):
                ratio = np.abs(a.v - b) / (AGREE * (a.e + np.abs(a.v)) + _TINY)
                ratio = np.where(dec & np.isfinite(a.v) & np.isfinite(a.e), ratio, 0.0)
                check_forms[name] = max(check_forms.get(name, 0.0), float(np.nan_to_num(ratio, nan=np.inf).max()))
            check_forms["records"] = check_forms.get("records", 0) + int(dec.sum())
        cat = lambda a, b: np.concatenate([a, b], axis=1)
        acc = cat(tr["accepted"], sp["accepted"]) & enters[s:e, None]
        und = cat(tr["undecided"], sp["undecided"]) & enters[s:e, None]
        if shadow:
            acc &= occ[None, :]; und &= occ[None, :]                                                 # skdtree.h:329-333
        t = cat(tr["t"].v, sp["t"].v); te = cat(tr["t"].e, sp["t"].e)
        if shadow:
            hit = acc.any(axis=1)
            out.hit[s:e] = hit
            out.ambiguous[s:e] |= ~hit & und.any(axis=1)
            continue
        reach = REACH * EPS32 * te
        t_hi = np.where(acc, t + reach, np.inf).min(axis=1)
        t_lo = np.where(np.isfinite(t) & np.isfinite(te), t - reach, -np.inf)
        within = (acc | und) & (t_lo <= t_hi[:, None])
        out.ambiguous[s:e] |= (und & within).any(axis=1)
        tie = acc & within
        out.hit[s:e] = tie.any(axis=1)
        u = cat(tr["u"].v, np.zeros_like(sp["t"].v)); ue = cat(tr["u"].e, np.full_like(sp["t"].v, np.inf))
        v = cat(tr["v"].v, np.zeros_like(sp["t"].v)); ve = cat(tr["v"].e, np.full_like(sp["t"].v, np.inf))
        far = cat(np.full_like(tr["t"].v, np.nan), sp["far"].v)
        for r, c in zip(*np.nonzero(tie)):
            tied.append((s + r, prim_ids[c], t[r, c], te[r, c], u[r, c], ue[r, c], v[r, c], ve[r, c], far[r, c]))
        poss = acc | und
        for r in np.nonzero(out.ambiguous[s:e])[0]:
            out.possible[s + r] = frozenset(prim_ids[poss[r]].tolist())
    if shadow:
        return out
    # the tied sets as padded arrays
    count = np.zeros(n, dtype=np.int64)
    for row in tied:
        count[row[0]] += 1
    m = max(1, int(count.max()) if n else 1)
    out.prim = np.full((n, m), -1, dtype=np.int64)
    names = ("t", "te", "u", "ue", "v", "ve", "far")
    for k in names:
        setattr(out, k, np.full((n, m), np.nan))
    fill = np.zeros(n, dtype=np.int64)
    for row in tied:
        i, j = row[0], fill[row[0]]
        out.prim[i, j] = row[1]
        for k, val in zip(names, row[2:]):
            getattr(out, k)[i, j] = val
        fill[i] += 1
    return out
