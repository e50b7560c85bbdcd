"""The cylinder shape restated twice from the reference's sources (src/shapes/cylinder.cpp), not from csrc/:

  * a binary32 MIRROR in numpy, operation for operation: the constructors (:34-64), both rayIntersect forms (:82-152), the
    intersection record (:154-176), getAABB (:187-208) and getClippedAABB (:216-375).  numpy's float32 operations are the
    IEEE ones, one rounding each, nothing fused.  std::atan2 is the library's own (mts.devmath("atan2")), handed in by the
    caller, because the product defines it.
  * a binary64 TRUTH with a first-order bound of the error of the binary32 evaluation per value (class E of ref64_sky.py,
    units of 2^-23).  The bound of t carries the 1 / sqrt(discriminant) factor through _sqrt: a near-tangent ray is granted
    what binary32 loses there.  A second binary64 form knows no quadratic: the hit point's distance from the axis is the
    radius and its axial coordinate lies in [0, length].

Every discrete decision of the ray tests is taken in both precisions; a ray on which they differ, or whose decision lies
within REACH bounds of its threshold, is FRAGILE and left out of a comparison (the tests cap their share at 1 %).  The
thresholds: the discriminant's sign, nearT > maxt, farT < mint, z against 0 and length, nearT >= mint, farT <= maxt.
Test infrastructure."""
import numpy as np

from ref64 import EPS32
from ref64_sky import E, _sqrt, _where, REACH

F = np.float32
EPSILON = F(1e-4)
PI32 = F(3.14159265358979323846)
FRAGILE_CAP = 0.01


def _f(x):
    return np.asarray(x, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# binary32 mirror: constructors
# ---------------------------------------------------------------------------------------------------------------------
def _mul4(a, b):
    """Matrix4x4 operator* (matrix.h): sum += a[i][k] * b[k][j] from 0"""
    r = np.zeros((4, 4), dtype=np.float32)
    for i in range(4):
        for j in range(4):
            s = F(0)
            for k in range(4):
                s = F(s + F(a[i, k] * b[k, j]))
            r[i, j] = s
    return r


def _invert4(src):
    """Gauss-Jordan Matrix::invert (matrix.inl:140-190); None when singular"""
    t = np.array(src, dtype=np.float32)
    indxc, indxr, ipiv = [0] * 4, [0] * 4, [0] * 4
    for i in range(4):
        irow = icol = -1
        big = F(0)
        for j in range(4):
            if ipiv[j] == 1:
                continue
            for k in range(4):
                if ipiv[k] == 0:
                    if abs(t[j, k]) >= big:
                        big = abs(t[j, k]); irow, icol = j, k
                elif ipiv[k] > 1:
                    return None
        ipiv[icol] += 1
        if irow != icol:
            t[[irow, icol]] = t[[icol, irow]]
        indxr[i], indxc[i] = irow, icol
        if t[icol, icol] == 0:
            return None
        pivinv = F(1) / t[icol, icol]
        t[icol, icol] = F(1)
        for j in range(4):
            t[icol, j] = F(t[icol, j] * pivinv)
        for j in range(4):
            if j == icol:
                continue
            save = t[j, icol]
            t[j, icol] = F(0)
            for k in range(4):
                t[j, k] = F(t[j, k] - F(t[icol, k] * save))
    for j in range(3, -1, -1):
        if indxr[j] != indxc[j]:
            t[:, [indxr[j], indxc[j]]] = t[:, [indxc[j], indxr[j]]]
    return t


def coordinate_system32(a):
    """coordinateSystem (util.cpp:602-611) -> b, c"""
    a = _f(a)
    if abs(a[0]) > abs(a[1]):
        inv = F(1) / np.sqrt(F(F(a[0] * a[0]) + F(a[2] * a[2])))
        b = _f([F(-a[2]) * inv, F(0), a[0] * inv])
    else:
        inv = F(1) / np.sqrt(F(F(a[1] * a[1]) + F(a[2] * a[2])))
        b = _f([F(0), F(-a[2]) * inv, a[1] * inv])
    return b, _cross32(a, b)


def _cross32(a, b):
    return _f([F(F(a[1] * b[2]) - F(a[2] * b[1])), F(F(a[2] * b[0]) - F(a[0] * b[2])), F(F(a[0] * b[1]) - F(a[1] * b[0]))])


def _len32(v):
    return np.sqrt(F(F(F(v[0] * v[0]) + F(v[1] * v[1])) + F(v[2] * v[2])))


def _block(o2w, w2o, radius, length):
    D = np.zeros(28, dtype=np.float32)
    D[0:12] = o2w[:3].ravel(); D[12:24] = w2o[:3].ravel()
    D[24], D[25] = radius, length
    D[26] = F(1) / F(F(F(F(2) * PI32) * radius) * length)                      # m_invSurfaceArea (:62)
    return D


def configure_points32(p1, p2, radius, keep_scale=False):
    """Cylinder(p1, p2, radius) (:41-52, :61-62) -> the derived block [28] of include/mtsgpu_cylinder.h"""
    p1, p2, radius = _f(p1), _f(p2), F(radius)
    rel = _f(p2 - p1)
    length = _len32(rel)
    n = _f(rel * (F(1) / length))                                              # Vector / Float multiplies by the reciprocal
    s, t = coordinate_system32(n)
    fwd = np.eye(4, dtype=np.float32); fwd[:3, 0], fwd[:3, 1], fwd[:3, 2] = s, t, n        # Transform::fromFrame
    inv = fwd.T.copy()
    tr = np.eye(4, dtype=np.float32); tr[:3, 3] = p1
    tri = np.eye(4, dtype=np.float32); tri[:3, 3] = -p1
    return _block(_mul4(tr, fwd), _mul4(inv, tri), radius, length)             # Transform::operator* (transform.cpp:28-31)


def configure_toworld32(m, keep_scale=False):
    """Cylinder(toWorld) (:54-62).  keep_scale: the mutation that leaves the scale in objectToWorld"""
    m = _f(m).reshape(4, 4)
    inv = _invert4(m)
    if inv is None:
        raise ValueError("singular")
    radius = _len32(_f([F(F(F(m[i, 0] * F(1)) + F(m[i, 1] * F(0))) + F(m[i, 2] * F(0))) for i in range(3)]))
    length = _len32(_f([F(F(F(m[i, 0] * F(0)) + F(m[i, 1] * F(0))) + F(m[i, 2] * F(1))) for i in range(3)]))
    if keep_scale:
        return _block(m, inv, radius, length)
    sx, sz = F(1) / radius, F(1) / length
    S = np.diag(_f([sx, sx, sz, 1])); Si = np.diag(_f([F(1) / sx, F(1) / sx, F(1) / sz, 1]))
    return _block(_mul4(m, S), _mul4(Si, inv), radius, length)


# ---------------------------------------------------------------------------------------------------------------------
# binary32 mirror: ray tests (vectorised over rays)
# ---------------------------------------------------------------------------------------------------------------------
def _xf(M, p, point):
    """Transform::operator()(Point / Vector) with w == 1 (transform.h:102-119, :152-160): M [12], p [n][3] -> three [n]"""
    out = []
    for i in range(3):
        r = M[4 * i] * p[:, 0] + M[4 * i + 1] * p[:, 1] + M[4 * i + 2] * p[:, 2]
        out.append(r + M[4 * i + 3] if point else r)
    return out


def solve_quadratic32(a, b, c):
    """solveQuadratic (util.cpp:450-488), arrays -> ok, x0, x1"""
    with np.errstate(all="ignore"):
        lin = a == 0
        disc = b * b - F(4) * a * c
        ok = np.where(lin, b != 0, ~(disc < 0))
        sq = np.sqrt(np.where(disc < 0, F(0), disc))
        temp = np.where(b < 0, F(-0.5) * (b - sq), F(-0.5) * (b + sq))
        x0 = np.where(lin, -c / b, temp / a); x1 = np.where(lin, -c / b, c / temp)
        swap = x0 > x1
        return ok, np.where(swap, x1, x0).astype(np.float32), np.where(swap, x0, x1).astype(np.float32)


def intersect32(D, rays, mint, maxt, shadow=False, mutation=None):
    """Cylinder::rayIntersect on rays [n][8] (o, -, d, -) with the intervals mint, maxt [n]: the closest-hit form (:82-118)
    -> (hit, t), or with shadow the any-hit form (:120-152) -> (hit, None).  mutation: one of the named wrong versions"""
    D = _f(D); R = _f(rays).reshape(-1, 8)
    mint, maxt = _f(mint), _f(maxt)
    with np.errstate(all="ignore"):
        ox, oy, oz = _xf(D[12:24], R[:, 0:3], True)
        dx, dy, dz = _xf(D[12:24], R[:, 4:7], False)
        A = dx * dx + dy * dy
        B = F(2) * (dx * ox + dy * oy)
        Cq = ox * ox + oy * oy - D[24] * D[24]
        ok, near, far = solve_quadratic32(A, B, Cq)
        ok = ok & ~((near > maxt) | (far < mint))
        zn = oz + dz * near; zf = oz + dz * far
        first = (zn >= 0) & (zn <= D[25]) & (near >= mint)
        second = (zf >= 0) & (zf <= D[25])
        if mutation == "near_mint_dropped":
            first = (zn >= 0) & (zn <= D[25])
        if mutation == "far_before_near":
            hit = ok & ((second & ~(far > maxt)) | (~second & first))
            return hit, np.where(second, far, near).astype(np.float32)
        if shadow:
            if mutation == "anyhit_far_accepted":
                return ok & (first | second), None
            return ok & (first | (second & (far <= maxt))), None
        hit = ok & (first | (second & ~(far > maxt)))
        return hit, np.where(first, near, far).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# binary32 mirror: the intersection record
# ---------------------------------------------------------------------------------------------------------------------
def _normalize32(x, y, z):
    inv = F(1) / np.sqrt(x * x + y * y + z * z)
    return np.stack([x * inv, y * inv, z * inv], axis=1).astype(np.float32)


def record32(D, p, atan2, mutation=None):
    """Cylinder::fillIntersectionRecord (:154-176) at the world points p [n][3] -> dict uv [n][2], dpdu, dpdv, n, s, t [n][3].
    atan2(y, x): the library's binary32 arctangent"""
    D = _f(D); p = _f(p).reshape(-1, 3)
    with np.errstate(all="ignore"):
        lx, ly, lz = _xf(D[12:24], p, True)
        phi = _f(atan2(ly, lx))
        if mutation != "phi_no_wrap":
            phi = np.where(phi < 0, phi + F(2) * PI32, phi).astype(np.float32)
        uv = np.stack([lz / D[25], phi / (F(2) * PI32)], axis=1).astype(np.float32)
        if mutation == "uv_swapped":
            uv = uv[:, ::-1].copy()
        two_pi = F(2) * PI32
        zero = np.zeros_like(lx)
        du = np.stack([-ly * two_pi, lx * two_pi, zero * two_pi], axis=1).astype(np.float32)
        dv = np.stack([zero, zero, zero + D[25]], axis=1).astype(np.float32)
        O = np.zeros(12, dtype=np.float32); O[:] = D[0:12]
        dpdu = np.stack(_xf(O, du, False), axis=1).astype(np.float32)
        dpdv = np.stack(_xf(O, dv, False), axis=1).astype(np.float32)
        cr = np.stack([du[:, 1] * dv[:, 2] - du[:, 2] * dv[:, 1], du[:, 2] * dv[:, 0] - du[:, 0] * dv[:, 2],
                       du[:, 0] * dv[:, 1] - du[:, 1] * dv[:, 0]], axis=1).astype(np.float32)
        if mutation == "normal_as_normal":       # Transform::operator()(Normal): the transposed inverse (transform.h:173-181)
            W = D[12:24]
            nx = [W[0 + i] * cr[:, 0] + W[4 + i] * cr[:, 1] + W[8 + i] * cr[:, 2] for i in range(3)]
        else:
            nx = _xf(O, cr, False)
        n = _normalize32(*nx)
        s = _normalize32(dpdu[:, 0], dpdu[:, 1], dpdu[:, 2])
        t = _normalize32(dpdv[:, 0], dpdv[:, 1], dpdv[:, 2])
        if mutation == "frame_orthogonalised":
            d = (n * s).sum(axis=1, keepdims=True).astype(np.float32)
            s = _normalize32(*(s - n * d).T)
            t = np.cross(n, s).astype(np.float32)
    return dict(uv=uv, dpdu=dpdu, dpdv=dpdv, n=n, s=s, t=t)


# ---------------------------------------------------------------------------------------------------------------------
# binary32 mirror: getAABB, getClippedAABB (scalar code, as written)
# ---------------------------------------------------------------------------------------------------------------------
def _pt(D, p):
    return _f([F(F(F(F(D[4 * i] * p[0]) + F(D[4 * i + 1] * p[1])) + F(D[4 * i + 2] * p[2])) + D[4 * i + 3]) for i in range(3)])


def _vec(D, v):
    return _f([F(F(F(D[4 * i] * v[0]) + F(D[4 * i + 1] * v[1])) + F(D[4 * i + 2] * v[2])) for i in range(3)])


def aabb32(D, variant=None):
    """Cylinder::getAABB (:187-208) -> [6]; variant "if0": the disabled one of :417-430"""
    D = _f(D); r, l = D[24], D[25]
    p0, p1 = _pt(D, _f([0, 0, 0])), _pt(D, _f([0, 0, l]))
    if variant == "if0":
        lo = np.minimum(p0 - r, p1 - r); hi = np.maximum(p0 + r, p1 + r)
        return np.concatenate([lo, hi]).astype(np.float32)
    x1, x2 = _vec(D, _f([r, 0, 0])), _vec(D, _f([0, r, 0]))
    out = np.zeros(6, dtype=np.float32)
    for i in range(3):
        rng = np.sqrt(F(F(x1[i] * x1[i]) + F(x2[i] * x2[i])))
        out[i] = min(min(F(np.inf), F(p0[i] - rng)), F(p1[i] - rng))
        out[3 + i] = max(max(F(-np.inf), F(p0[i] + rng)), F(p1[i] + rng))
    return out


def _dot32(a, b):
    return F(F(F(a[0] * b[0]) + F(a[1] * b[1])) + F(a[2] * b[2]))


# what the last clipped32 met on its way: a decision within reach of its threshold makes the box FRAGILE -- an edge root's
# discriminant near zero (the ellipse touches an edge of the face: a cell face tangent to the tube, as every face of the own box
# of an axis-parallel cylinder is), an edge root near 0 or 1, |dot(n, d)| near Epsilon.  (alpha == 0 in the componentwise maxima is no threshold: its NaN
# points change nothing in either precision.)
CLIP_NOTES = {"fragile": False}
_NEAR = 64 * float(EPS32)


def _note(cond):
    if cond:
        CLIP_NOTES["fragile"] = True


class _Box:
    def __init__(self):
        self.mn = _f([np.inf] * 3); self.mx = _f([-np.inf] * 3)

    def expand(self, p):
        for i in range(3):
            if p[i] < self.mn[i]: self.mn[i] = p[i]          # std::min(min, p): p when p < min
            if self.mx[i] < p[i]: self.mx[i] = p[i]          # std::max(max, p): p when max < p


def _expand_box(a, b):
    for i in range(3):
        if b.mn[i] < a.mn[i]: a.mn[i] = b.mn[i]
        if a.mx[i] < b.mx[i]: a.mx[i] = b.mx[i]


def _cyl_plane32(plane_pt, nrm, cyl_pt, cyl_d, radius):
    """intersectCylPlane (:216-255) -> None or (center, axes, lengths)"""
    with np.errstate(all="ignore"):
        _note(abs(float(abs(_dot32(nrm, cyl_d))) - float(EPSILON)) <= _NEAR)
        if abs(_dot32(nrm, cyl_d)) < EPSILON:
            return None
        A = _f(cyl_d - _f(nrm * _dot32(cyl_d, nrm)))
        length = _len32(A)
        if length != 0:
            A = _f(A * (F(1) / length))
            B = _cross32(nrm, A)
        else:
            A, B = coordinate_system32(nrm)
        delta = _f(plane_pt - cyl_pt)
        dproj = _f(delta - _f(cyl_d * _dot32(delta, cyl_d)))
        ad, bd = _dot32(A, cyl_d), _dot32(B, cyl_d)
        c0 = F(F(1) - F(ad * ad)); c1 = F(F(1) - F(bd * bd))
        c2 = F(F(2) * _dot32(A, dproj)); c3 = F(F(2) * _dot32(B, dproj))
        c4 = F(_dot32(delta, dproj) - F(radius * radius))
        lam = F(F(F(F(F(c2 * c2) / F(F(4) * c0)) + F(F(c3 * c3) / F(F(4) * c1))) - c4) / F(c0 * c1))
        alpha0 = F(F(-c2) / F(F(2) * c0)); beta0 = F(F(-c3) / F(F(2) * c1))
        lengths = (np.sqrt(F(c1 * lam)), np.sqrt(F(c0 * lam)))
        center = _f(_f(plane_pt + _f(A * alpha0)) + _f(B * beta0))
        return center, [A, B], lengths


def _cyl_face32(axis, mn, mx, cyl_pt, cyl_d, radius, skip_maxima=False):
    """intersectCylFace (:257-330)"""
    a1, a2 = (axis + 1) % 3, (axis + 2) % 3
    nrm = _f([0, 0, 0]); nrm[axis] = 1
    box = _Box()
    got = _cyl_plane32(mn, nrm, cyl_pt, cyl_d, radius)
    if got is None:
        return box
    center, axes, lengths = got
    with np.errstate(all="ignore"):
        for i in range(4):
            p1, p2 = _f([0, 0, 0]), _f([0, 0, 0])
            p1[axis] = p2[axis] = mn[axis]
            p1[a1] = mn[a1] if ((i + 1) & 2) else mx[a1]
            p1[a2] = mn[a2] if ((i + 0) & 2) else mx[a2]
            p2[a1] = mn[a1] if ((i + 2) & 2) else mx[a1]
            p2[a2] = mn[a2] if ((i + 1) & 2) else mx[a2]
            p1l = [F(_dot32(_f(p1 - center), axes[k]) / lengths[k]) for k in range(2)]
            p2l = [F(_dot32(_f(p2 - center), axes[k]) / lengths[k]) for k in range(2)]
            rel = [F(p2l[0] - p1l[0]), F(p2l[1] - p1l[1])]
            A = F(F(rel[0] * rel[0]) + F(rel[1] * rel[1]))
            B = F(F(2) * F(F(p1l[0] * rel[0]) + F(p1l[1] * rel[1])))
            Cq = F(F(F(p1l[0] * p1l[0]) + F(p1l[1] * p1l[1])) - F(1))
            ok, x0, x1 = solve_quadratic32(_f([A]), _f([B]), _f([Cq]))
            _note(abs(float(B) * float(B) - 4.0 * float(A) * float(Cq)) <= _NEAR * (float(B) * float(B) + abs(4.0 * float(A) * float(Cq))))
            if ok[0]:
                for x in (x0[0], x1[0]):
                    _note(abs(float(x)) <= _NEAR or abs(float(x) - 1.0) <= _NEAR)
                    if x >= 0 and x <= 1:
                        box.expand(_f(p1 + _f(_f(p2 - p1) * x)))
        ax = [_f(axes[0] * lengths[0]), _f(axes[1] * lengths[1])]
        if not skip_maxima:
            for i in range(2):
                j = a1 if i == 0 else a2
                alpha, beta = ax[0][j], ax[1][j]
                ratio = F(beta / alpha); tmp = np.sqrt(F(F(1) + F(ratio * ratio)))
                ct, st = F(F(1) / tmp), F(ratio / tmp)
                q1 = _f(_f(center + _f(ax[0] * ct)) + _f(ax[1] * st))
                q2 = _f(_f(center - _f(ax[0] * ct)) - _f(ax[1] * st))
                for q in (q1, q2):
                    # AABB::contains (aabb.h:133-138); a NaN coordinate fails neither comparison and changes nothing in expandBy
                    if not any(q[c] < mn[c] or q[c] > mx[c] for c in range(3)):
                        box.expand(q)
    return box


def clipped32(D, cell, mutation=None):
    """Cylinder::getClippedAABB (:332-375) of the cell [6] -> ([6], valid).  mutation: "base_clip" (Shape::getClippedAABB),
    "face_pair_missing" (the two z faces left out), "maxima_missing" """
    D = _f(D); cell = _f(cell)
    CLIP_NOTES["fragile"] = False
    own = aabb32(D)
    lo = np.maximum(own[:3], cell[:3]).astype(np.float32); hi = np.minimum(own[3:], cell[3:]).astype(np.float32)
    # std::max(a, b) = b when a < b: equal for non-NaN input
    if mutation == "base_clip":
        out = np.concatenate([lo, hi]); return out, bool((hi >= lo).all())
    cyl_pt, cyl_d = _pt(D, _f([0, 0, 0])), _vec(D, _f([0, 0, 1]))
    r = D[24]
    faces = [(0, [lo[0], lo[1], lo[2]], [lo[0], hi[1], hi[2]]), (0, [hi[0], lo[1], lo[2]], [hi[0], hi[1], hi[2]]),
             (1, [lo[0], lo[1], lo[2]], [hi[0], lo[1], hi[2]]), (1, [lo[0], hi[1], lo[2]], [hi[0], hi[1], hi[2]]),
             (2, [lo[0], lo[1], lo[2]], [hi[0], hi[1], lo[2]]), (2, [lo[0], lo[1], hi[2]], [hi[0], hi[1], hi[2]])]
    if mutation == "face_pair_missing":
        faces = faces[:4]
    box = _Box()
    for axis, a, b in faces:
        _expand_box(box, _cyl_face32(axis, _f(a), _f(b), cyl_pt, cyl_d, r, skip_maxima=(mutation == "maxima_missing")))
    mn = np.maximum(box.mn, cell[:3]).astype(np.float32); mx = np.minimum(box.mx, cell[3:]).astype(np.float32)
    return np.concatenate([mn, mx]), bool(not (mx < mn).any())


# ---------------------------------------------------------------------------------------------------------------------
# binary64 truth
# ---------------------------------------------------------------------------------------------------------------------
def _xfE(M, p, point):
    M = np.asarray(M, dtype=np.float64)
    out = []
    for i in range(3):
        r = E(M[4 * i]) * E(p[:, 0]) + E(M[4 * i + 1]) * E(p[:, 1]) + E(M[4 * i + 2]) * E(p[:, 2])
        out.append(r + E(M[4 * i + 3]) if point else r)
    return out


def _close(a, b):
    with np.errstate(invalid="ignore"):
        both = np.isfinite(a.v) & np.isfinite(b.v)          # an infinite end of the interval is close to nothing; a NaN to everything
        return np.isnan(a.v) | np.isnan(b.v) | (both & (np.abs(a.v - b.v) <= REACH * EPS32 * (a.e + b.e) + 1e-300))


def intersect64(D, rays, mint, maxt, shadow=False):
    """the ray tests in binary64 on the binary32 block and rays -> dict hit, t (E), fragile.  The block is taken as given:
    its own rounding belongs to the constructor's bound, not to the ray's."""
    D = _f(D).astype(np.float64); R = _f(rays).astype(np.float64).reshape(-1, 8)
    mn, mx = E(_f(mint).astype(np.float64)), E(_f(maxt).astype(np.float64))
    with np.errstate(all="ignore"):
        ox, oy, oz = _xfE(D[12:24], R[:, 0:3], True)
        dx, dy, dz = _xfE(D[12:24], R[:, 4:7], False)
        A = dx * dx + dy * dy
        B = E(2.0) * (dx * ox + dy * oy)
        Cq = ox * ox + oy * oy - E(D[24]) * E(D[24])
        lin = A.v == 0
        disc = B * B - E(4.0) * A * Cq
        none = np.where(lin, B.v == 0, disc.v < 0)
        fragile = ~lin & (np.abs(disc.v) <= REACH * EPS32 * disc.e)
        sq = _sqrt(_where(disc.v < 0, 1.0, disc))
        temp = E(-0.5) * _where(B.v < 0, B - sq, B + sq)
        x0 = _where(lin, -Cq / B, temp / A); x1 = _where(lin, -Cq / B, Cq / temp)
        swap = x0.v > x1.v
        near, far = _where(swap, x1, x0), _where(swap, x0, x1)
        out = (near.v > mx.v) | (far.v < mn.v)
        fragile |= ~none & (_close(near, mx) | _close(far, mn))
        zn = oz + dz * near; zf = oz + dz * far
        L = E(D[25]); Z = E(0.0)
        first = (zn.v >= 0) & (zn.v <= L.v) & (near.v >= mn.v)
        second = (zf.v >= 0) & (zf.v <= L.v)
        live = ~none & ~out
        fragile |= live & (_close(zn, Z) | _close(zn, L) | _close(near, mn))
        fragile |= live & ~first & (_close(zf, Z) | _close(zf, L) | _close(far, mx))
        if shadow:
            hit = live & (first | (second & (far.v <= mx.v)))
        else:
            hit = live & (first | (second & ~(far.v > mx.v)))
        t = _where(first, near, far)
    return dict(hit=hit, t=t, fragile=fragile, first=first)


def second_form(D, rays, t):
    """what a reported hit must satisfy without any quadratic: -> (|distance from the axis - radius|, axial coordinate) of
    ray(t) in object space, binary64"""
    D = _f(D).astype(np.float64); R = _f(rays).astype(np.float64).reshape(-1, 8)
    p = R[:, 0:3] + np.asarray(t, dtype=np.float64)[:, None] * R[:, 4:7]
    W = D[12:24].reshape(3, 4)
    loc = p @ W[:, :3].T + W[:, 3]
    return np.abs(np.hypot(loc[:, 0], loc[:, 1]) - D[24]), loc[:, 2]


def record64(D, p):
    """the intersection record in binary64 with bounds -> dict of lists of E (uv: 2, the vectors: 3 each)"""
    D = _f(D).astype(np.float64); p = _f(p).astype(np.float64).reshape(-1, 3)
    from ref64_sky import _atan2
    with np.errstate(all="ignore"):
        lx, ly, lz = _xfE(D[12:24], p, True)
        phi = _atan2(ly, lx)
        two_pi = E(float(F(2) * PI32))
        phi = _where(phi.v < 0, phi + two_pi, phi)
        uv = [lz / E(D[25]), phi / two_pi]
        du = [-ly * two_pi, lx * two_pi, E(np.zeros(len(p)))]
        dv = [E(np.zeros(len(p))), E(np.zeros(len(p))), E(np.full(len(p), D[25]))]

        def xv(v):
            return [E(D[4 * i]) * v[0] + E(D[4 * i + 1]) * v[1] + E(D[4 * i + 2]) * v[2] for i in range(3)]

        def norm(v):
            inv = E(1.0) / _sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            return [c * inv for c in v]
        dpdu, dpdv = xv(du), xv(dv)
        cr = [du[1] * dv[2] - du[2] * dv[1], du[2] * dv[0] - du[0] * dv[2], du[0] * dv[1] - du[1] * dv[0]]
        return dict(uv=uv, dpdu=dpdu, dpdv=dpdv, n=norm(xv(cr)), s=norm(dpdu), t=norm(dpdv), phi=phi)


def surface_points(D, n_angle=512, n_height=512):
    """the surface on an (angle, height) grid in binary64, world space -> [n_angle * n_height][3], and the grid spacing's
    bound: no surface point is farther from a sample than half the diagonal of a grid cell"""
    D = _f(D).astype(np.float64)
    r, l = D[24], D[25]
    a = (np.arange(n_angle) + 0.5) * (2 * np.pi / n_angle)
    h = np.linspace(0.0, l, n_height)
    aa, hh = np.meshgrid(a, h, indexing="ij")
    loc = np.stack([r * np.cos(aa), r * np.sin(aa), hh], axis=-1).reshape(-1, 3)
    M = D[0:12].reshape(3, 4)
    scale = np.linalg.norm(M[:, :3], ord=2)
    spacing = 0.5 * np.hypot(r * 2 * np.pi / n_angle, l / (n_height - 1)) * scale
    return loc @ M[:, :3].T + M[:, 3], spacing
