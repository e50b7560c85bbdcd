"""A binary64 restatement of the non-delta luminaires and of the selection among a scene's luminaires, written from the
reference's sources, not from csrc/ or oracle/:

  Scene::sampleLuminaire / pdfLuminaire       src/librender/scene.cpp:381-415
  DiscretePDF::build / sample / sampleReuse   include/mitsuba/core/pdf.h:82-133
  AreaLuminaire::sample / pdf                 src/luminaires/area.cpp:68-83
  Shape::sampleSolidAngle / pdfSolidAngle     src/librender/shape.cpp:65-83
  TriMesh::configure / sampleArea             src/librender/trimesh.cpp:266-302
  Triangle::sample / surfaceArea              src/libcore/triangle.cpp:23-55
  Sphere::sampleSolidAngle / pdfSolidAngle    src/shapes/sphere.cpp:191-246 (rayIntersect :92-113, area :59)
  ConstantLuminaire::sample / pdf / Le        src/luminaires/constant.cpp:70-92
  EnvMapLuminaire                             src/luminaires/envmap.cpp:134-199
  MIPMap::triangle / getTexel                 src/librender/mipmap.cpp:203-243
  BSphere::contains / rayIntersect            include/mitsuba/core/bsphere.h:67-118
  squareToSphere / Triangle / Cone, coordinateSystem, solveQuadratic      src/libcore/util.cpp:450-488, :552-558, :602-662

Conventions of tests/ref64.py and tests/ref64_sky.py: binary32 inputs promoted to binary64, every quantity carried as an
E(value, err) pair (ref64_sky.E), err a first-order bound in units of 2^-23 on the absolute error of a binary32 evaluation
in the reference's operation order.  cond = err / |value|, so the conditioning factors are derived, not chosen: the
1 / (1 - cosThetaMax) of the cone pdf of a distant sphere comes out of the subtraction, the 1 / sinTheta of the envmap
density out of the division, the tangent factor of a grazing cone ray out of the discriminant b^2 - 4ac of the ray-sphere
root, the 1 / (cdf[i+1] - cdf[i]) of a reused sample out of DiscretePDF::sampleReuse.

What goes in.  A scene is a dict of the arrays of a flattened mtsgpu_scene (abi.scene_arrays).  Taken as data: vertex
positions and normals, triangle indices, sphere centres and radii, the luminaire blocks (intensities, the envmap's two
rotations, the bounding sphere), and the three envmap tables env_pixels, env_pdf, env_cdf (binary32 data like a parameter
block).  Recomputed here in binary64 from vertices and radii: the selection pdf / cdf / sum, the per-emitter triangle
cdf, the inverse areas of meshes and spheres (Tables); tests/test_lum_truth.py holds the host's binary32 tables to them.

Branches.  A comparison whose operand lies within REACH of its own error of the threshold is undecidable in binary32.
Those of the kind a case class is built to sit on -- a sample on a CDF knot, the 1 - Epsilon switch of the sphere, the
boundary of the bounding sphere, a direction on a cell border of the envmap density -- set `knot`; with tie = -1 / +1 the
restatement takes the lower / upper branch at every such comparison, so a check can demand one of the two (tie = 2: the
upper branch, and on the bounding sphere's boundary the third outcome described in _bsphere).  All others
(dp > 0 in the plane of a triangle, a tangent cone ray that misses by roundoff, a pole) set `amb`.  Test infrastructure."""
import numpy as np

from ref64 import EPS32, _f64
from ref64_sky import E, _E, _sin, _cos, _atan2, _where, PI32, REACH

EPSILON = float(np.float32(1e-4))           # constants.h:31
AREA, CONSTANT, POINT, DIRECTIONAL, SPOT, ENVMAP, COLLIMATED, SKY = range(8)
NON_DELTA = (AREA, CONSTANT, ENVMAP, SKY)


def _sqrt(a):
    """sqrt with the first-order bound err / (2 sqrt(v)), capped by what holds at any v >= 0: sqrt(v + d) - sqrt(v) <= sqrt(d).
    The cap keeps the bound finite where the argument is exactly 0 (the cone axis, the poles of squareToSphere, a reused
    sample of exactly 1)"""
    v = np.sqrt(a.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.fmin(a.e / (2 * v), np.sqrt(a.e * EPS32) / EPS32)
    return E(v, e)._r()


def _acos(a):
    """acos of a clamped argument; first-order bound err / sqrt(1 - c^2), capped by acos(c - d) - acos(c) <= 2 sqrt(d)"""
    c = np.clip(a.v, -1.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.fmin(a.e / np.sqrt(1 - c * c), 2 * np.sqrt(a.e * EPS32) / EPS32)
    return E(np.arccos(c), e)._r()


# ---------------------------------------------------------------------------------------------------------------------
# vectors of E
# ---------------------------------------------------------------------------------------------------------------------
def _V(a):
    a = _f64(a).reshape(-1, 3)
    return [E(a[:, 0]), E(a[:, 1]), E(a[:, 2])]


def _C(a):
    """a constant vector (three binary32 scalars)"""
    return [E(float(np.float32(x))) for x in a]


def _sub(a, b): return [x - y for x, y in zip(a, b)]
def _add(a, b): return [x + y for x, y in zip(a, b)]
def _scale(a, s): return [x * s for x in a]
def _neg(a): return [-x for x in a]
def _dot(a, b): return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
def _len(a): return _sqrt(_dot(a, a))


def _normalize(a):
    l = _len(a)                                 # vector.h:403-405: v / v.length()
    return [x / l for x in a]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _mat3(M, v):
    """a 3x3 rotation block applied to a vector (Transform::operator()(Vector), transform.h)"""
    return [E(M[3 * i]) * v[0] + E(M[3 * i + 1]) * v[1] + E(M[3 * i + 2]) * v[2] for i in range(3)]


def _vals(a, n):
    return np.stack([np.broadcast_to(x.v, (n,)) for x in a], axis=1)


def _errs(a, n):
    return np.stack([np.broadcast_to(x.e, (n,)) for x in a], axis=1)


def _near(q, thr=0.0):
    with np.errstate(invalid="ignore"):
        return np.abs(q.v - thr) <= REACH * EPS32 * q.e + 1e-300


def _decide(cond, near, tie, upper):
    """the outcome of a comparison: `cond` where binary64 decides it; within reach and with tie != 0 the branch the tie
    names (`upper` = the outcome that counts as the upper branch)"""
    if tie == 0:
        return cond
    return np.where(near, upper if tie > 0 else (not upper), cond)


# ---------------------------------------------------------------------------------------------------------------------
# the tables that are arithmetic on the description
# ---------------------------------------------------------------------------------------------------------------------
def _build_cdf(w):
    """DiscretePDF::build (pdf.h:82-95) on weights E: running sum, then every entry divided by the sum; the last knot is set
    to 1.  -> (cdf E [n + 1], pdf E [n], sum E)"""
    w = _E(w)
    n = len(w.v)
    run = np.concatenate([[0.0], np.cumsum(w.v)])
    # knot k has seen k additions of half a unit of the partial sum each, on top of the weights' own errors
    err = np.concatenate([[0.0], np.cumsum(w.e)]) + 0.5 * np.arange(n + 1) * run
    total = E(run[-1], err[-1])
    cdf = E(run, err) / total
    cdf.v[-1], cdf.e[-1] = 1.0, 0.0
    cdf.e[0] = 0.0
    return cdf, w / total, total


class Tables:
    """selection and area tables of a scene, recomputed in binary64"""

    def __init__(self, A):
        self.A = A
        nl = len(A["lum_type"])
        self.n_lums = nl
        self.sel_cdf, self.sel_pdf, self.sel_sum = _build_cdf(E(np.ones(nl)))      # scene.cpp:320-330, weight 1
        self.tri_cdf, self.inv_area, self.tris = {}, {}, {}
        pos = A["vtx_pos"].astype(np.float64)
        for l in range(nl):
            if A["lum_type"][l] != AREA:
                continue
            s = int(A["lum_shape"][l])
            if A["shape_type"][s] == 1:
                r = E(float(A["shape_params"][s][3]))
                self.inv_area[l] = 1 / (4 * PI32 * r * r)                            # sphere.cpp:59
                continue
            t0, t1 = int(A["shape_tri_offset"][s]), int(A["shape_tri_offset"][s + 1])
            idx = A["tri_idx"][t0:t1].astype(np.int64)
            p0, p1, p2 = pos[idx[:, 0]], pos[idx[:, 1]], pos[idx[:, 2]]
            a, b = _sub(_V(p1), _V(p0)), _sub(_V(p2), _V(p0))
            area = 0.5 * _len(_cross(a, b))                                          # triangle.cpp:49-55
            cdf, _, total = _build_cdf(area)                                         # trimesh.cpp:279-283
            self.tri_cdf[l], self.inv_area[l], self.tris[l] = cdf, 1.0 / total, idx


def tables(A):
    return Tables(A)


# ---------------------------------------------------------------------------------------------------------------------
# DiscretePDF::sampleReuse (pdf.h:102-133)
# ---------------------------------------------------------------------------------------------------------------------
def _sample_reuse(cdf, s, tie):
    """-> (index, reused sample E, knot): std::lower_bound over the n + 1 knots, index = max(0, pos - 1), capped at n - 1;
    the sample becomes (s - cdf[i]) / (cdf[i + 1] - cdf[i])"""
    n = len(cdf.v) - 1
    pos = np.searchsorted(cdf.v, s.v, side="left")                  # first knot >= s
    index = np.clip(pos - 1, 0, n - 1)
    # the nearest knot decides whether binary32 could have gone the other way
    k = np.clip(np.where(np.abs(cdf.v[np.clip(pos, 0, n)] - s.v) <= np.abs(s.v - cdf.v[np.clip(pos - 1, 0, n)]), pos, pos - 1), 0, n)
    near = np.abs(s.v - cdf.v[k]) <= REACH * EPS32 * (s.e + cdf.e[k]) + 1e-300
    near &= (k > 0) & (k < n)                                        # at the two ends both outcomes are clamped to the same cell
    if tie != 0:
        index = np.where(near, np.clip(k - 1 if tie < 0 else k, 0, n - 1), index)
    lo, hi = E(cdf.v[index], cdf.e[index]), E(cdf.v[index + 1], cdf.e[index + 1])
    r = (s - lo) / (hi - lo)
    if tie != 0:
        r = E(np.where(near, np.clip(r.v, 0.0, 1.0), r.v), r.e)
    return index, r, near


# ---------------------------------------------------------------------------------------------------------------------
# util.cpp
# ---------------------------------------------------------------------------------------------------------------------
def _square_to_sphere(sx, sy):
    z = 1.0 - 2.0 * sy                                               # util.cpp:552-558
    r = 1.0 - z * z
    r = _sqrt(E(np.maximum(r.v, 0.0), r.e))
    phi = 2.0 * PI32 * sx
    return [r * _cos(phi), r * _sin(phi), z]


def _coordinate_system(a):
    """util.cpp:602-611 -> (b, c, undecidable |a.x| > |a.y|).  Either branch yields an orthonormal frame, but not the same one."""
    first = np.abs(a[0].v) > np.abs(a[1].v)
    near = np.abs(np.abs(a[0].v) - np.abs(a[1].v)) < REACH * EPS32 * (a[0].e + a[1].e)
    zero = E(np.zeros_like(a[0].v))
    il1 = 1.0 / _sqrt(a[0] * a[0] + a[2] * a[2])
    il2 = 1.0 / _sqrt(a[1] * a[1] + a[2] * a[2])
    b1 = [-a[2] * il1, zero, a[0] * il1]
    b2 = [zero, -a[2] * il2, a[1] * il2]
    b = [_where(first, u, v) for u, v in zip(b1, b2)]
    return b, _cross(a, b), near


class Rec:
    """what a luminaire's sample() leaves: E triples p, n, d, value; E pdf; alive; knot / amb flags"""


def _zero3(n):
    return [E(np.zeros(n)) for _ in range(3)]


def _sel3(m, a, b):
    return [_where(m, x, y) for x, y in zip(a, b)]


# ---------------------------------------------------------------------------------------------------------------------
# the luminaires' sample(p, lRec, sample)
# ---------------------------------------------------------------------------------------------------------------------
def _finish_area(r, p, pdf, P, N, LP, amb):
    """AreaLuminaire::sample (area.cpp:68-79) after Shape::sampleSolidAngle returned pdf"""
    d = _sub(p, P)
    dn = _dot(d, N)
    with np.errstate(invalid="ignore"):
        ok = (pdf.v > 0) & (dn.v > 0)
    r.amb = amb | (_near(dn) & (pdf.v > 0))
    r.p, r.n, r.d = P, N, _sel3(ok, _normalize(d), d)
    r.pdf = _where(ok, pdf, 0.0)
    r.value = _C(LP[0:3])
    r.alive = ok
    return r


def _solid_angle_from_area(p, P, N, pdf_area):
    """shape.cpp:65-75 / sphere.cpp:202-208"""
    l2p = _sub(p, P)
    d2 = _dot(l2p, l2p)
    dp = _dot(l2p, N)
    with np.errstate(invalid="ignore", divide="ignore"):
        pdf = _where(dp.v > 0, pdf_area * d2 * _sqrt(d2) / dp, 0.0)
    return pdf, _near(dp)


def _sample_mesh(T, l, p, sx, sy, tie):
    A = T.A
    r = Rec()
    index, sy, r.knot = _sample_reuse(T.tri_cdf[l], sy, tie)          # trimesh.cpp:297-302: newSeed.y is reused
    tri = T.tris[l][index]
    pos = A["vtx_pos"].astype(np.float64)
    p0, p1, p2 = _V(pos[tri[:, 0]]), _V(pos[tri[:, 1]]), _V(pos[tri[:, 2]])
    a = _sqrt(1.0 - sx)                                               # squareToTriangle (util.cpp:613-616)
    bx, by = 1 - a, a * sy
    sideA, sideB = _sub(p1, p0), _sub(p2, p0)
    P = _add(_add(p0, _scale(sideA, bx)), _scale(sideB, by))          # triangle.cpp:29-31
    s = int(A["lum_shape"][l])
    if A["shape_flags"][s] & 1:
        nrm = A["vtx_nrm"].astype(np.float64)
        n0, n1, n2 = _V(nrm[tri[:, 0]]), _V(nrm[tri[:, 1]]), _V(nrm[tri[:, 2]])
        b0 = 1.0 - bx - by
        N = _normalize(_add(_add(_scale(n0, b0), _scale(n1, bx)), _scale(n2, by)))       # triangle.cpp:33-41
    else:
        N = _normalize(_cross(sideA, sideB))                          # :43
    pdf, amb = _solid_angle_from_area(p, P, N, T.inv_area[l])
    r.tri = index
    return _finish_area(r, p, pdf, P, N, A["lum_params"][l], amb)


def _sphere_switch(T, l, p_minus_c_or_c_minus_p, tie):
    """squareTerm >= 1 - Epsilon (sphere.cpp:192-195 / :231-234) -> (inside, knot, squareTerm)"""
    A = T.A
    SP = A["shape_params"][int(A["lum_shape"][l])]
    radius = E(float(SP[3]))
    w = p_minus_c_or_c_minus_p
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1 / _len(w)
        sq = radius * inv
    sq = E(np.abs(sq.v), sq.e)
    thr = 1 - EPSILON                                                 # a binary32 constant expression
    thr = float(np.float32(thr))
    with np.errstate(invalid="ignore"):
        knot = _near(sq, thr) & np.isfinite(sq.v)
        inside = _decide(~(sq.v < thr), knot, tie, True)             # p at the centre: 1 / 0 = inf >= threshold
    return inside, knot, sq, inv, radius


def _sample_sphere(T, l, p, sx, sy, tie):
    A = T.A
    SP = A["shape_params"][int(A["lum_shape"][l])]
    center = _C(SP[0:3])
    r = Rec()
    w = _sub(center, p)
    inside, r.knot, sq, inv, radius = _sphere_switch(T, l, w, tie)
    # --- uniform sampling (sphere.cpp:195-209) ---
    d_u = _square_to_sphere(sx, sy)
    P_u = _add(center, _scale(d_u, radius))
    pdf_u, amb_u = _solid_angle_from_area(p, P_u, d_u, T.inv_area[l])
    # --- cone sampling (:211-227) ---
    with np.errstate(invalid="ignore", divide="ignore"):
        t = 1 - sq * sq
        cmax = _sqrt(E(np.maximum(t.v, 0.0), t.e))
        cos_t = (1 - sx) + sx * cmax                                  # squareToCone (util.cpp:656-662)
        u = 1 - cos_t * cos_t
        sin_t = _sqrt(E(np.maximum(u.v, 0.0), u.e))
        phi = sy * (2 * PI32)
        cone = [_cos(phi) * sin_t, _sin(phi) * sin_t, cos_t]
        fn = _scale(w, inv)
        fs, ft, amb_frame = _coordinate_system(fn)
        d = [fs[i] * cone[0] + ft[i] * cone[1] + fn[i] * cone[2] for i in range(3)]      # Frame::toWorld (frame.h)
        # Sphere::rayIntersect (sphere.cpp:92-113) with solveQuadratic (util.cpp:450-488), mint 0, maxt inf
        o = _neg(w)
        Aq = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        Bq = 2 * (d[0] * o[0] + d[1] * o[1] + d[2] * o[2])
        # The componentwise bounds cannot see two orthogonalities, and without them every narrow cone would look tangent.
        # d = fs x + ft y + fn cosTheta with o = -|w| fn: the error of x and y (that of sinTheta, large where cosTheta is
        # close to 1) reaches d.o only through fs.fn and ft.fn, rounding residues of coordinateSystem (<= 2 units each).  So
        # d.o = -|w| (cosTheta + residues * sinTheta), plus the roundings of the three products and two sums of the dot
        # product itself.  Likewise d.d = cosTheta^2 + sinTheta^2 (+ residues), and sinTheta was taken from the rounded
        # cosTheta, so A is 1 to within the roundings of squares, sums and the square root.
        dist = _len(w)
        Bq = E(Bq.v, 2 * (dist.v * (cos_t.e + 4 * sin_t.v) + dist.e * np.abs(cos_t.v)) + 3 * np.abs(Bq.v))
        Aq = E(Aq.v, 2 * np.abs(cos_t.v) * cos_t.e + 2 * sin_t.v * np.minimum(sin_t.e, u.e / np.maximum(2 * sin_t.v, 1e-300)) + 4.0)
        Cq = o[0] * o[0] + o[1] * o[1] + o[2] * o[2] - radius * radius
        disc = Bq * Bq - 4.0 * Aq * Cq
        hit = disc.v >= 0
        sd = _sqrt(E(np.maximum(disc.v, 0.0), disc.e))
        temp = _where(Bq.v < 0, -0.5 * (Bq - sd), -0.5 * (Bq + sd))
        x0, x1 = temp / Aq, Cq / temp
        near_t, far_t = _where(x0.v > x1.v, x1, x0), _where(x0.v > x1.v, x0, x1)
        hit &= ~(far_t.v < 0)
        tt = _where(near_t.v < 0, far_t, near_t)
        P_c = [p[i] + tt * d[i] for i in range(3)]                    # ray(t)
        N_c = _normalize(_sub(P_c, center))
        om = 1 - cmax
        pdf_cone = 1 / ((2 * PI32) * om)
        pdf_c = _where(hit, pdf_cone, 0.0)
        # 1 - cosThetaMax within binary32 reach of 0 (radius / distance below about 1e-3): the reference's own arithmetic may
        # then divide by an exact 0, and does below 2.4e-4: pdf = inf, value = 0
        r.ovf = _near(om) & ~inside
        r.pdf_if_found = _where(inside, np.nan, pdf_cone)
        # a tangent ray that misses by roundoff, a root whose sign is in doubt, a frame that could be the other one
        amb_c = _near(disc) | (_near(near_t) & hit) | amb_frame
    P, N = _sel3(inside, P_u, P_c), _sel3(inside, d_u, N_c)
    pdf = _where(inside, pdf_u, pdf_c)
    amb = np.where(inside, amb_u, amb_c)
    r.inside = inside
    r = _finish_area(r, p, pdf, P, N, A["lum_params"][l], amb)
    # lRec.d = normalize(p - (p + t d)): the error of t moves the point along the ray and leaves the direction alone, which
    # the componentwise bound cannot see.  What reaches d is the cone direction's own error, the roundings of the sum and
    # the difference (half a unit of |p + t d| and of the difference each, seen from the distance t) and the normalisation
    with np.errstate(invalid="ignore", divide="ignore"):
        own = [d[i].e + (np.abs(P_c[i].v) + np.abs(tt.v * d[i].v)) / np.abs(tt.v) + 1.0 for i in range(3)]
        length = sum(np.abs(d[j].v) * own[j] for j in range(3))      # the length's error, which the division spreads over all three
        for i in range(3):
            e = own[i] + np.abs(d[i].v) * (length + 2.5)
            r.d[i] = E(r.d[i].v, np.where(inside | ~r.alive, r.d[i].e, np.minimum(r.d[i].e, e)))
    return r


def _bsphere(LP, p, dray, tie):
    """m_bsphere.contains(p) && m_bsphere.rayIntersect(Ray(p, dray), nearHit, farHit) (bsphere.h:67-118) ->
    (ok, nearHit E, knot, amb).  A point the first test admits and the second one puts outside is within reach of the
    boundary by construction."""
    center, radius = _C(LP[3:6]), E(float(LP[6]))
    oc = _sub(center, p)
    dist = _len(_sub(p, center))
    tmp1 = _dot(oc, oc) - radius * radius
    knot = _near(dist - radius) | _near(tmp1)
    inside = _decide((dist.v <= radius.v) & (tmp1.v <= 0), knot, tie, False)
    dtc = _dot(oc, dray)
    with np.errstate(invalid="ignore"):
        near = _sqrt(dtc * dtc - tmp1) + dtc                          # :90-96
    if tie == 2:
        # the third outcome on the boundary: contains() admits p (length <= radius) while lengthSquared - radius^2 > 0 sends
        # rayIntersect down its outside branch (:98-117), whose near root is p itself to within the rounding of
        # distToRayClosest - sqrt(radius^2 - |oc|^2 + distToRayClosest^2), for a ray that points inwards (a near root of
        # exactly 0 is replaced by the far one, :114-115, which is the inside branch's answer)
        inside = np.where(knot, dtc.v >= 0, inside)
        with np.errstate(invalid="ignore"):
            half = radius * radius - _dot(oc, oc) + dtc * dtc         # :102-104
            near3 = dtc - _sqrt(E(np.maximum(half.v, 0.0), half.e))  # :110-111
        near = _where(knot, near3, near)
    return inside, near, knot


def _sample_constant(T, l, p, sx, sy, tie):
    LP = T.A["lum_params"][l]
    n = len(sx.v)
    r = Rec()
    d = _square_to_sphere(sx, sy)                                     # constant.cpp:76
    ok, near, r.knot = _bsphere(LP, p, d, tie)
    center = _C(LP[3:6])
    with np.errstate(invalid="ignore", divide="ignore"):
        P = [p[i] + d[i] * near for i in range(3)]
        N = _normalize(_sub(center, P))
    r.p, r.n, r.d = P, N, _neg(d)
    r.pdf = _where(ok, E(1.0) / (4 * PI32), 0.0)
    r.value = _C(LP[0:3])
    r.alive, r.amb = ok, np.zeros(n, dtype=bool)
    return r


def _texel(A, tx, ty):
    """MIPMap::getTexel, ERepeat (mipmap.cpp:203-225); modulo (util.cpp:424-427)"""
    H, W = A["env_pixels"].shape[:2]
    out = (tx <= 0) | (ty < 0) | (tx >= W) | (ty >= H)
    tx = np.where(out, np.mod(tx, W), tx)
    ty = np.where(out, np.mod(ty, H), ty)
    return A["env_pixels"].astype(np.float64)[ty, tx]


def _triangle(A, x, y):
    """MIPMap::triangle(0, x, y) (mipmap.cpp:233-241) -> E triple.  The lookup is continuous across texel borders, wrap-around
    included, so the floor needs no flag: either cell gives the value, to within the error carried."""
    H, W = A["env_pixels"].shape[:2]
    x = x * float(W) - 0.5
    y = y * float(H) - 0.5
    with np.errstate(invalid="ignore"):
        xp = np.floor(np.where(np.isfinite(x.v), x.v, 0.0)).astype(np.int64)
        yp = np.floor(np.where(np.isfinite(y.v), y.v, 0.0)).astype(np.int64)
    dx, dy = x - E(xp.astype(np.float64)), y - E(yp.astype(np.float64))
    t00, t01, t10, t11 = _texel(A, xp, yp), _texel(A, xp, yp + 1), _texel(A, xp + 1, yp), _texel(A, xp + 1, yp + 1)
    out = []
    for c in range(3):
        out.append(E(t00[:, c]) * (1.0 - dx) * (1.0 - dy) + E(t01[:, c]) * (1.0 - dx) * dy
                   + E(t10[:, c]) * dx * (1.0 - dy) + E(t11[:, c]) * dx * dy)
    return out


def _sample_envmap(T, l, p, sx, sy, tie):
    A = T.A
    LP = A["lum_params"][l]
    n = len(sx.v)
    r = Rec()
    _, _, rx, ry = A["env_size"]
    cdf = E(A["env_cdf"].astype(np.float64))                           # data: exact
    idx, sx, r.knot = _sample_reuse(cdf, sx, tie)                      # envmap.cpp:141
    pdf = E(A["env_pdf"].astype(np.float64)[idx])
    row = idx // rx
    col = idx - rx * row
    with np.errstate(invalid="ignore", divide="ignore"):
        x, y = E(col.astype(np.float64)) + sx, E(row.astype(np.float64)) + sy           # :144
        inv_rx, inv_ry = float(np.float32(1.0) / np.float32(rx)), float(np.float32(1.0) / np.float32(ry))
        value = [v * float(LP[0]) for v in _triangle(A, x * inv_rx, y * inv_ry)]        # :145-146
        psx, psy = float(np.float32(2 * np.float32(PI32)) / np.float32(rx)), float(np.float32(PI32) / np.float32(ry))
        theta, phi = psy * y, psx * x - PI32                            # :147
        st, ct, sp, cp = _sin(theta), _cos(theta), _sin(phi), _cos(phi)
        pdf = pdf / (E(psx) * psy * st)                                 # :150
        d = _mat3(_f64(LP[16:25]), [-st * sp, -ct, st * cp])            # :152-153
        ok, near, knot2 = _bsphere(LP, p, _neg(d), tie)                 # :173-180
        r.knot = r.knot | knot2
        P = [p[i] - d[i] * near for i in range(3)]
        N = _normalize(_sub(_C(LP[3:6]), P))
    r.p, r.n, r.d = P, N, d
    r.pdf = _where(ok, pdf, 0.0)
    r.value = value
    with np.errstate(invalid="ignore"):
        r.alive = ok & (r.pdf.v != 0)
    # sinTheta = 0 (y = 0 exactly) gives pdf = inf by the reference's own arithmetic: no ambiguity, the check expects inf
    r.amb = np.zeros(n, dtype=bool)
    r.cell = idx
    return r


def _sample_delta(T, l, p, n):
    """the delta luminaires are held to ref64.py elsewhere; here they only have to be recognisable in a selection"""
    r = Rec()
    r.p = r.n = r.d = r.value = _zero3(n)
    r.pdf = E(np.ones(n))
    r.alive, r.amb, r.knot = np.ones(n, dtype=bool), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    r.delta = True
    return r


class Sample:
    """sample_luminaire()'s result: found, lum, p / n / d / value [n][3] and pdf [n] with their error bounds *_err (units of
    2^-23, absolute), delta (the selected luminaire is a delta one: only found and lum are stated), knot, amb; ovf and
    pdf_if_found for a cone-sampled sphere: where pdf = inf, value = 0 is the reference's own answer, and the pdf a found
    sample has whether or not the restatement can decide that the cone ray hits"""


def sample_luminaire(T, p, s, tie=0):
    """Scene::sampleLuminaire(p, lRec, s, testVisibility = false) (scene.cpp:396-415)"""
    A = T.A
    p32, s32 = _f64(p).reshape(-1, 3), _f64(s).reshape(-1, 2)
    n = len(p32)
    pe = _V(p32)
    sx, sy = E(s32[:, 0]), E(s32[:, 1])
    index, sx, knot = _sample_reuse(T.sel_cdf, sx, tie)               # :401: sample.x is reused
    out = Sample()
    out.lum = index.copy()
    out.p, out.n, out.d, out.value = (np.zeros((n, 3)) for _ in range(4))
    out.p_err, out.n_err, out.d_err, out.value_err = (np.zeros((n, 3)) for _ in range(4))
    out.pdf, out.pdf_err = np.zeros(n), np.zeros(n)
    out.found = np.zeros(n, dtype=bool)
    out.delta = np.zeros(n, dtype=bool)
    out.amb = np.zeros(n, dtype=bool)
    out.knot = knot.copy()
    out.ovf = np.zeros(n, dtype=bool)
    out.pdf_if_found, out.pdf_if_found_err = np.full(n, np.nan), np.full(n, np.nan)
    out.detail = {}
    for l in np.unique(index):
        m = index == l
        t = int(A["lum_type"][l])
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if t == AREA and A["shape_type"][int(A["lum_shape"][l])] == 1:
                r = _sample_sphere(T, l, pe, sx, sy, tie)
            elif t == AREA:
                # the reuse of the triangle cdf only makes sense for the records that selected this luminaire; for the others
                # sx is some other cell's sample, which is still a number in [0, 1]
                r = _sample_mesh(T, l, pe, E(np.clip(sx.v, 0, 1), sx.e), sy, tie)
            elif t == CONSTANT:
                r = _sample_constant(T, l, pe, sx, sy, tie)
            elif t == ENVMAP:
                r = _sample_envmap(T, l, pe, E(np.clip(sx.v, 0, 1), sx.e), sy, tie)
            elif t == SKY:
                raise ValueError("the sky has its own restatement (ref64_sky)")
            else:
                r = _sample_delta(T, l, pe, n)
            # :405-411
            pdf = r.pdf * E(T.sel_pdf.v[l], T.sel_pdf.e[l])
            recip = 1.0 / pdf
            value = [v * recip for v in r.value]
        out.found[m] = (r.alive & (r.pdf.v != 0))[m]
        out.delta[m] = getattr(r, "delta", False)
        for name, vec in (("p", r.p), ("n", r.n), ("d", r.d), ("value", value)):
            getattr(out, name)[m] = _vals(vec, n)[m]
            getattr(out, name + "_err")[m] = _errs(vec, n)[m]
        out.pdf[m], out.pdf_err[m] = np.broadcast_to(pdf.v, (n,))[m], np.broadcast_to(pdf.e, (n,))[m]
        out.amb[m] = r.amb[m]
        if hasattr(r, "ovf"):
            out.ovf[m] = r.ovf[m]
            pif = r.pdf_if_found * E(T.sel_pdf.v[l], T.sel_pdf.e[l])
            out.pdf_if_found[m], out.pdf_if_found_err[m] = pif.v[m], pif.e[m]
        out.knot[m] |= r.knot[m]
        for k in ("inside", "tri", "cell"):
            if hasattr(r, k):
                out.detail.setdefault(k, np.full(n, -1, dtype=np.int64))[m] = np.asarray(getattr(r, k))[m]
    out.pdf = np.where(out.found, out.pdf, 0.0)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# Scene::pdfLuminaire (scene.cpp:381-394)
# ---------------------------------------------------------------------------------------------------------------------
def _env_pdf(T, l, ld, tie):
    """EnvMapLuminaire::pdf (envmap.cpp:187-197) -> (pdf E, knot, amb)"""
    A = T.A
    LP = A["lum_params"][l]
    _, _, rx, ry = A["env_size"]
    d = _mat3(_f64(LP[7:16]), _neg(ld))
    x = .5 * (1 + _atan2(d[0], -d[2]) / PI32) * float(rx)
    dy = E(np.clip(d[1].v, -1.0, 1.0), d[1].e)
    y = _acos(dy) / PI32 * float(ry)
    def cell(q, hi):
        f = np.floor(q.v)
        k = np.round(q.v)                                              # the nearest border
        near = (np.abs(q.v - k) <= REACH * EPS32 * q.e) & (k > 0) & (k < hi)       # beyond the ends the clamp absorbs it
        if tie != 0:
            f = np.where(near, k - 1 if tie < 0 else k, f)
        return np.clip(f, 0, hi - 1).astype(np.int64), near
    xp, kx = cell(x, rx)
    yp, ky = cell(y, ry)
    # the seam: atan2(d.x, -d.z) = +-pi by the sign of a d.x within reach of 0, the first column or the last
    seam = _near(d[0]) & (d[2].v > 0)
    if tie != 0:
        xp = np.where(seam, 0 if tie < 0 else rx - 1, xp)
    kx = kx | seam
    pdf = E(A["env_pdf"].astype(np.float64)[xp + yp * rx])
    t = 1 - d[1] * d[1]
    # atan2(0, 0) at the poles is a number (0), x then falls into one definite column: no flag.  The clamp max(Epsilon, .):
    clamp = ~(t.v > EPSILON)
    amb = _near(t, EPSILON)
    st = _sqrt(E(np.where(clamp, EPSILON, t.v), np.where(clamp, 0.0, t.e)))
    psx, psy = float(np.float32(2 * np.float32(PI32)) / np.float32(rx)), float(np.float32(PI32) / np.float32(ry))
    _env_pdf.clamp = clamp
    return pdf / (E(psx) * psy * st), kx | ky, amb


def pdf_luminaire(T, p, lum, lp, ln, ld, tie=0):
    """-> (pdf, cond, knot, amb) for one luminaire index `lum` (an int: the hook's records of one call may mix them, the
    case lists do not).  pdf_luminaire.ovf holds, for the last call, where the cone pdf of a distant sphere divides by a
    1 - cosThetaMax within binary32 reach of 0 (see _sample_sphere): inf is then the reference's own answer."""
    A = T.A
    p, lp, ln, ld = _V(p), _V(lp), _V(ln), _V(ld)
    n = len(p[0].v)
    l = int(lum)
    t = int(A["lum_type"][l])
    knot, amb, ovf = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    fraction = 1.0 / T.sel_sum                                        # scene.cpp:392, weight 1
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if t == AREA and A["shape_type"][int(A["lum_shape"][l])] == 1:
            center = _C(A["shape_params"][int(A["lum_shape"][l])][0:3])
            inside, knot, sq, inv, radius = _sphere_switch(T, l, _sub(p, center), tie)
            pdf_u, amb_u = _solid_angle_from_area(p, lp, ln, T.inv_area[l])            # sphere.cpp:236-241
            tt = 1 - sq * sq
            cmax = _sqrt(E(np.maximum(tt.v, 0.0), tt.e))
            om = 1 - cmax
            pdf_c = 1 / (2 * PI32 * om)                                # squareToConePdf (util.cpp:652-654)
            ovf = _near(om) & ~inside
            pdf = _where(inside, pdf_u, pdf_c)
            amb = np.where(inside, amb_u, False)
        elif t == AREA:
            l2p = _sub(p, lp)                                          # shape.cpp:77-83
            d2 = _dot(l2p, l2p)
            dp = _dot(l2p, ln)
            inv_dp = _sqrt(d2) / dp
            amb = _near(dp)
            inv_dp = _where(inv_dp.v > 0, inv_dp, 0.0)
            pdf = T.inv_area[l] * d2 * inv_dp
        elif t == ENVMAP:
            pdf, knot, amb = _env_pdf(T, l, ld, tie)
        elif t in (CONSTANT, SKY):
            pdf = E(np.ones(n)) / (4 * PI32)                           # constant.cpp:90-92
        else:
            raise ValueError("Scene::pdfLuminaire is not asked for a delta luminaire")
        pdf = pdf * fraction
        cond = np.where(pdf.v != 0, pdf.e / np.abs(pdf.v), 1.0)
    pdf_luminaire.ovf = ovf
    pdf_luminaire.clamp = _env_pdf.clamp if t == ENVMAP else np.zeros(n, dtype=bool)      # max(Epsilon, .) took Epsilon (envmap.cpp:195)
    return np.broadcast_to(pdf.v, (n,)).copy(), np.broadcast_to(cond, (n,)).copy(), knot, amb


# ---------------------------------------------------------------------------------------------------------------------
# Scene::LeBackground: ConstantLuminaire::Le (constant.cpp:70-72), EnvMapLuminaire::Le(ray) (envmap.cpp:157-167)
# ---------------------------------------------------------------------------------------------------------------------
def background_le(T, direction):
    """-> (Le [n][3], cond [n][3], amb)"""
    A = T.A
    l = int(A["background_lum"])
    if l < 0:
        raise ValueError("no background luminaire")
    LP = A["lum_params"][l]
    d = _V(direction)
    n = len(d[0].v)
    if int(A["lum_type"][l]) == CONSTANT:
        v = np.tile(_f64(LP[0:3]), (n, 1))
        return v, np.ones((n, 3)), np.zeros(n, dtype=bool)
    if int(A["lum_type"][l]) != ENVMAP:
        raise ValueError("the sky has its own restatement (ref64_sky)")
    with np.errstate(invalid="ignore", divide="ignore"):
        d = _mat3(_f64(LP[7:16]), _normalize(d))
        u = .5 * (1 + _atan2(d[0], -d[2]) / PI32)
        dy = E(np.clip(d[1].v, -1.0, 1.0), d[1].e)
        v = _acos(dy) / PI32
        val = [c * float(LP[0]) for c in _triangle(A, u, v)]
    vals, errs = _vals(val, n), _errs(val, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        cond = np.where(vals != 0, errs / np.abs(vals), 1.0)
    return vals, cond, np.zeros(n, dtype=bool)
