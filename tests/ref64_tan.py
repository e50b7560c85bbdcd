"""Vertex tangents from texture coordinates and the shading frame built on them, restated from the reference's lines (not from
flatten.cpp or shade.hip):

    TriMesh::computeTangentSpaceBasis   trimesh.cpp:547-669
        a zero vertex normal becomes (1, 0, 0); per triangle, in triangle order:
            dP1 = v1 - v0, dP2 = v2 - v0, dUV1 = uv1 - uv0, dUV2 = uv2 - uv0
            determinant = dUV1.x * dUV2.y - dUV1.y * dUV2.x;  invDet = 1 / determinant, or 1 when it is zero
            dpdu = ( dUV2.y * dP1 - dUV1.y * dP2) * invDet;   dpdv = (-dUV2.x * dP1 + dUV1.x * dP2) * invDet
            dpdu.length() == 0:  n = cross(dP1, dP2); if its length is not 0: n /= length, dpdu = cross(n, dpdv), and
                                 coordinateSystem(n, dpdu, dpdv) if that is zero again
            dpdv.length() == 0:  likewise with dpdv = cross(dpdu, n)
            both are added to the triangle's three vertices, whose `sharers` count goes up by one
        per vertex: coordinateSystem(normal, dpdu, dpdv) when either squared length is 0, else both divided by sharers
    fillIntersectionRecord              skdtree.h:364,388-401
        b = ((1 - u) - v, u, v);  dpdu = (t0.dpdu * b.x + t1.dpdu * b.y) + t2.dpdu * b.z
        n = normalize((n0 * b.x + n1 * b.y) + n2 * b.z);  s = normalize(dpdu - n * dot(n, dpdu));  t = cross(n, s)
    which meshes                        trimesh.cpp:288-290, ward.cpp:84-85
        those whose BSDF is anisotropic (a Ward with alphaU != alphaV, alone, in a composite or a twosided), that have
        texcoords and vertex normals

Vector / scalar is one reciprocal and three products, normalize(v) = v / v.length(), dot and cross as vector.h:386-401 write them.

Every function takes `dtype`.  numpy.float32 gives the MIRROR: the reference's Float expressions, one rounding per operation,
no contraction, accumulation in triangle order, every `== 0` decided in binary32.  numpy.float64 gives the RESTATEMENT from
the same binary32 inputs, together with a first-order bound, in units of 2^-23, on the absolute error the binary32 evaluation
makes (the convention of tests/ref64_vcol.py: every rounded operation adds half a unit of its result; a sum adds its operands'
bounds; a product a * b adds |a| e(b) + |b| e(a); 1 / a adds e(a) / a^2; sqrt(a) adds e(a) / (2 sqrt(a)); the inputs carry
none).  The restatement takes its `== 0` branches as the mirror took them (`decisions`), so both follow one path.

`mutation` swaps one line for a plausible mistake (MUTATIONS); tests/test_tan.py shows that each one is reported.  Test
infrastructure, not product code."""
import numpy as np

from ref64 import EPS32

F = np.float32
MUTATIONS = ("s_not_orthogonalised", "t_is_s_cross_n", "dpdu_dpdv_exchanged", "no_division_by_sharers", "no_inv_det",
             "normalised_per_vertex", "tangents_on_isotropic_mesh")
# |binary32 - binary64| <= bound * TOL32 + DENORM: the first-order bound, a margin for its second-order remainder (the chains
# here are a few dozen roundings deep) and one denormal step for results that underflow
TOL32 = EPS32 * (1.0 + 2.0 ** -10)
DENORM = 2.0 ** -149
WARD, COMPOSITE = 8, 9


class N:
    """a number (array) of the mirror (e is None) or of the restatement (e = its bound in units of 2^-23)"""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v, self.e = v, e

    @staticmethod
    def _rounded(v, e):
        return N(v, None if e is None else e + 0.5 * np.abs(v))

    def __add__(self, o):
        return N._rounded(self.v + o.v, None if self.e is None else self.e + o.e)

    def __sub__(self, o):
        return N._rounded(self.v - o.v, None if self.e is None else self.e + o.e)

    def __mul__(self, o):
        return N._rounded(self.v * o.v, None if self.e is None else np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    def __neg__(self):
        return N(-self.v, self.e)

    def recip(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.asarray(self.v).dtype.type(1) / self.v
            return N._rounded(v, None if self.e is None else self.e * v * v)

    def sqrt(self):
        with np.errstate(divide="ignore", invalid="ignore"):
            v = np.sqrt(self.v)
            return N._rounded(v, None if self.e is None else np.where(v > 0, self.e / (2 * np.where(v > 0, v, 1)), self.e * np.inf))


def num(a, dtype):
    """binary32 inputs as numbers of `dtype`: exact, so their bound is zero"""
    v = np.asarray(a, dtype=np.float32).astype(dtype)
    return N(v, None if dtype == np.float32 else np.zeros(v.shape))


def vec(a, dtype):
    a = np.asarray(a, dtype=np.float32)
    return tuple(num(a[..., k], dtype) for k in range(3))


def vadd(a, b): return tuple(x + y for x, y in zip(a, b))
def vsub(a, b): return tuple(x - y for x, y in zip(a, b))
def vscale(a, s): return tuple(x * s for x in a)
def vneg(a): return tuple(-x for x in a)
def dot(a, b): return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
def length(a): return dot(a, a).sqrt()
def vdiv(a, s): return vscale(a, s.recip())
def normalize(a): return vdiv(a, length(a))


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def coordinate_system(a, dtype):
    """util.cpp:602-611 for one vector (0-d numbers); the comparison is between inputs of the mirror's own values"""
    zero = num(0.0, dtype)
    if abs(float(a[0].v)) > abs(float(a[1].v)):
        inv = (a[0] * a[0] + a[2] * a[2]).sqrt().recip()
        b = (-a[2] * inv, zero, a[0] * inv)
    else:
        inv = (a[1] * a[1] + a[2] * a[2]).sqrt().recip()
        b = (zero, -a[2] * inv, a[1] * inv)
    return b, cross(a, b)


def _is_zero(x, decisions, replay):
    """`x == 0` of a 0-d number: decided by the mirror, replayed by the restatement"""
    if replay is not None:
        return replay.pop(0)
    d = bool(x.v == 0)
    decisions.append(d)
    return d


def tangent_space(positions, normals, texcoords, triangles, dtype, mutation=None, decisions=None):
    """computeTangentSpaceBasis past its early returns -> (dpdu [n][3], dpdv [n][3], bound_u, bound_v, normals, decisions).
    normals: the vertex normals with the zero ones replaced (binary32).  dtype float32: the mirror, bounds None, `decisions`
    the list of its `== 0` outcomes; float64: pass that list in as `decisions`"""
    pos, uv = np.asarray(positions, dtype=np.float32), np.asarray(texcoords, dtype=np.float32)
    nrm = np.array(normals, dtype=np.float32)
    nrm[(nrm == 0).all(axis=1)] = (1.0, 0.0, 0.0)
    tri = np.asarray(triangles, dtype=np.int64)
    nv = len(pos)
    replay = None if dtype == np.float32 else list(decisions)
    made = []
    zero = num(0.0, dtype)
    acc_u = [(zero, zero, zero)] * nv
    acc_v = [(zero, zero, zero)] * nv
    sharers = [0] * nv
    for i0, i1, i2 in tri:
        v0, v1, v2 = vec(pos[i0], dtype), vec(pos[i1], dtype), vec(pos[i2], dtype)
        dP1, dP2 = vsub(v1, v0), vsub(v2, v0)
        dU1 = (num(uv[i1, 0], dtype) - num(uv[i0, 0], dtype), num(uv[i1, 1], dtype) - num(uv[i0, 1], dtype))
        dU2 = (num(uv[i2, 0], dtype) - num(uv[i0, 0], dtype), num(uv[i2, 1], dtype) - num(uv[i0, 1], dtype))
        det = dU1[0] * dU2[1] - dU1[1] * dU2[0]
        inv_det = num(1.0, dtype)
        if not _is_zero(det, made, replay) and mutation != "no_inv_det":
            inv_det = det.recip()
        dpdu = vscale(vsub(vscale(dP1, dU2[1]), vscale(dP2, dU1[1])), inv_det)
        dpdv = vscale(vadd(vscale(dP1, -dU2[0]), vscale(dP2, dU1[0])), inv_det)
        if _is_zero(length(dpdu), made, replay):
            n = cross(dP1, dP2)
            ln = length(n)
            if not _is_zero(ln, made, replay):
                n = vdiv(n, ln)
                dpdu = cross(n, dpdv)
                if _is_zero(length(dpdu), made, replay):
                    dpdu, dpdv = coordinate_system(n, dtype)
        if _is_zero(length(dpdv), made, replay):
            n = cross(dP1, dP2)
            ln = length(n)
            if not _is_zero(ln, made, replay):
                n = vdiv(n, ln)
                dpdv = cross(dpdu, n)
                if _is_zero(length(dpdv), made, replay):
                    dpdu, dpdv = coordinate_system(n, dtype)
        if mutation == "dpdu_dpdv_exchanged":
            dpdu, dpdv = dpdv, dpdu
        for i in (i0, i1, i2):
            acc_u[i] = vadd(acc_u[i], dpdu)
            acc_v[i] = vadd(acc_v[i], dpdv)
            sharers[i] += 1
    for i in range(nv):
        if _is_zero(dot(acc_u[i], acc_u[i]), made, replay) | _is_zero(dot(acc_v[i], acc_v[i]), made, replay):
            acc_u[i], acc_v[i] = coordinate_system(vec(nrm[i], dtype), dtype)
        elif sharers[i] > 0 and mutation != "no_division_by_sharers":
            s = num(float(sharers[i]), dtype)
            acc_u[i], acc_v[i] = vdiv(acc_u[i], s), vdiv(acc_v[i], s)
        if mutation == "normalised_per_vertex":
            acc_u[i], acc_v[i] = normalize(acc_u[i]), normalize(acc_v[i])
    def gather(acc, field):
        return np.array([[float(getattr(c, field)) if getattr(c, field) is not None else 0.0 for c in a] for a in acc])
    du, dv = gather(acc_u, "v").astype(dtype), gather(acc_v, "v").astype(dtype)
    if dtype == np.float32:
        return du, dv, None, None, nrm, made
    return du, dv, gather(acc_u, "e"), gather(acc_v, "e"), nrm, made


def tangents32(positions, normals, texcoords, triangles, mutation=None):
    """the mirror -> (tan [n_verts][6] float32 = dpdu, dpdv; normals; decisions)"""
    du, dv, _, _, nrm, made = tangent_space(positions, normals, texcoords, triangles, np.float32, mutation)
    return np.concatenate([du, dv], axis=1).astype(np.float32), nrm, made


def tangents64(positions, normals, texcoords, triangles, decisions, mutation=None):
    """the restatement on the mirror's path -> (tan [n_verts][6] float64, bound [n_verts][6] in units of 2^-23)"""
    du, dv, eu, ev, _, _ = tangent_space(positions, normals, texcoords, triangles, np.float64, mutation, decisions)
    return np.concatenate([du, dv], axis=1), np.concatenate([eu, ev], axis=1)


def within_bound(got32, value, bound):
    return np.abs(np.asarray(got32, dtype=np.float64) - value) <= bound * TOL32 + DENORM


def frame(dpdu, normals, triangles, prim, u, v, dtype, mutation=None, dpdu_bound=None):
    """the shading frame of records (prim, u, v) on a mesh with vertex tangents: dpdu [n_verts][3] (binary32 for the mirror;
    for the restatement the binary64 tangents with their bound) and the mesh's vertex normals (binary32) ->
    (frames [n][3][3] rows s, t, n; bounds [n][3][3] or None)"""
    idx = np.asarray(triangles, dtype=np.int64)[np.asarray(prim, dtype=np.int64)]
    u_, v_ = num(u, dtype), num(v, dtype)
    bx, by, bz = (num(np.ones(len(idx)), dtype) - u_) - v_, u_, v_
    def corner(a, k, bound=None):
        a = np.asarray(a)
        if dtype == np.float32:
            return vec(a[idx[:, k]], dtype)
        e = np.zeros((len(idx), 3)) if bound is None else np.asarray(bound)[idx[:, k]]
        return tuple(N(a[idx[:, k], c].astype(np.float64), e[:, c]) for c in range(3))
    d0, d1, d2 = (corner(dpdu, k, dpdu_bound) for k in range(3))
    n0, n1, n2 = (corner(np.asarray(normals, dtype=np.float32), k) for k in range(3))
    d = vadd(vadd(vscale(d0, bx), vscale(d1, by)), vscale(d2, bz))
    n = normalize(vadd(vadd(vscale(n0, bx), vscale(n1, by)), vscale(n2, bz)))
    s = normalize(d) if mutation == "s_not_orthogonalised" else normalize(vsub(d, vscale(n, dot(n, d))))
    t = cross(s, n) if mutation == "t_is_s_cross_n" else cross(n, s)
    rows = np.stack([np.stack([c.v for c in r], axis=1) for r in (s, t, n)], axis=1)
    if dtype == np.float32:
        return rows.astype(np.float32), None
    return rows, np.stack([np.stack([c.e for c in r], axis=1) for r in (s, t, n)], axis=1)


def plain_frame(n, dtype=np.float64):
    """Frame(n) (frame.h, coordinateSystem) for unit normals [k][3] -> [k][3][3] rows s, t, n: what a mesh without tangents gets"""
    n = np.asarray(n, dtype=dtype)
    first = np.abs(n[:, 0]) > np.abs(n[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        ia = 1 / np.sqrt(n[:, 0] * n[:, 0] + n[:, 2] * n[:, 2]); ib = 1 / np.sqrt(n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
    zero = np.zeros(len(n), dtype=dtype)
    with np.errstate(invalid="ignore"):       # the branch not taken may be 0 * inf
        s = np.where(first[:, None], np.stack([-n[:, 2] * ia, zero, n[:, 0] * ia], axis=1), np.stack([zero, -n[:, 2] * ib, n[:, 1] * ib], axis=1))
    t = np.stack([n[:, 1] * s[:, 2] - n[:, 2] * s[:, 1], n[:, 2] * s[:, 0] - n[:, 0] * s[:, 2], n[:, 0] * s[:, 1] - n[:, 1] * s[:, 0]], axis=1)
    return np.stack([s, t, n], axis=1).astype(dtype)


# --- which meshes -----------------------------------------------------------------------------------------------------------
def bsdf_is_anisotropic(types, params, b):
    t, P = int(types[b]) & 0xFF, params[b]
    if t == WARD:
        return bool(np.float32(P[1]) != np.float32(P[2]))
    if t == COMPOSITE:
        n = int(P[0])
        return any(bsdf_is_anisotropic(types, params, int(P[1 + n + i])) for i in range(n))
    return False


def shape_flags(sd, mutation=None):
    """one flag per shape of a scene description: 1 = the reference computes tangents for it"""
    out = []
    for m in sd.meshes:
        mesh = m.sphere is None and m.texcoords is not None and not m.face_normals and m.bsdf >= 0
        out.append(int(mesh and (mutation == "tangents_on_isotropic_mesh" or bsdf_is_anisotropic(sd.bsdf_type, sd.bsdf_params, m.bsdf))))
    return out
