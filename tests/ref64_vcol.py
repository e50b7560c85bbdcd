"""A binary64 restatement of the per-vertex colour interpolation of fillIntersectionRecord, written from
include/mitsuba/render/skdtree.h:364,417-421 of the reference, not from csrc/:

    const Vector b(1 - cache->u - cache->v, cache->u, cache->v);
    its.color = c0 * b.x + c1 * b.y + c2 * b.z;

with c0, c1, c2 the colours of the triangle's three vertices.  C++ evaluates both lines left to right: b.x = (1 - u) - v and,
per channel, color = (c0 * b.x + c1 * b.y) + c2 * b.z.  Test infrastructure.

Two functions:

  color64   the value in binary64 from the float32 inputs, with a first-order bound, in units of 2^-23, on the absolute error
            a binary32 evaluation in that operation order makes (the convention of tests/ref64_sky.py: every rounded
            operation adds half a unit of its result, a sum adds its operands' bounds, a product a * b adds |a| err(b) +
            |b| err(a); the inputs u, v and the colours are binary32 numbers and carry no error).  Spelled out:
                e(bx) = (|1 - u| + |bx|) / 2
                e(t0) = |c0| e(bx) + |c0 bx| / 2          t0 = c0 * bx
                e(t1) = |c1 u| / 2                        t1 = c1 * u
                e(s)  = e(t0) + e(t1) + |s| / 2           s  = t0 + t1
                e(t2) = |c2 v| / 2                        t2 = c2 * v
                e(r)  = e(s) + e(t2) + |r| / 2            r  = s + t2
            The binary64 evaluation itself is off by at most 2^-29 of that bound and is ignored.
  color32   the same operations in numpy float32, one rounding each and no contraction: what a binary32 implementation in
            the reference's order returns bit for bit.

  gradient_bound   how far the colour can move when (u, v) move by (du, dv): |c1 - c0| du + |c2 - c0| dv per channel, the
            exact derivative of the linear interpolant; used where the barycentrics themselves are only known to a bound."""
import numpy as np

from ref64 import EPS32, _f64

F = np.float32
# |binary32 - binary64| <= bound * TOL32: the first-order bound, its second-order remainder (6 roundings deep) and one
# denormal step for results that underflow
TOL32 = EPS32 * (1.0 + 8 * 2.0 ** -24)
DENORM = 2.0 ** -149


def _corners(colors, tri_idx, prim):
    """colours [n_verts][3], triangles [n_tris][3], prim [n] -> c0, c1, c2 each [n][3] (dtype of `colors`)"""
    t = np.asarray(tri_idx, dtype=np.int64)[np.asarray(prim, dtype=np.int64)]
    return colors[t[:, 0]], colors[t[:, 1]], colors[t[:, 2]]


def color64(colors, tri_idx, prim, u, v):
    """-> (value [n][3] float64, bound [n][3] in units of 2^-23)"""
    c0, c1, c2 = _corners(_f64(colors), tri_idx, prim)
    u, v = _f64(u)[:, None], _f64(v)[:, None]
    omu = 1.0 - u
    bx = omu - v
    e_bx = 0.5 * (np.abs(omu) + np.abs(bx))
    t0, t1, t2 = c0 * bx, c1 * u, c2 * v
    e_t0 = np.abs(c0) * e_bx + 0.5 * np.abs(t0)
    s = t0 + t1
    e_s = e_t0 + 0.5 * np.abs(t1) + 0.5 * np.abs(s)
    r = s + t2
    e_r = e_s + 0.5 * np.abs(t2) + 0.5 * np.abs(r)
    return r, e_r


def color32(colors, tri_idx, prim, u, v):
    """the float32 mirror of the exact operation order -> [n][3] float32"""
    c0, c1, c2 = _corners(np.asarray(colors, dtype=np.float32), tri_idx, prim)
    u, v = np.asarray(u, dtype=np.float32)[:, None], np.asarray(v, dtype=np.float32)[:, None]
    bx = (F(1) - u) - v
    return ((c0 * bx + c1 * u) + c2 * v).astype(np.float32)


def gradient_bound(colors, tri_idx, prim, du, dv):
    """|d colour| <= |c1 - c0| du + |c2 - c0| dv, per channel (binary64) -> [n][3]"""
    c0, c1, c2 = _corners(_f64(colors), tri_idx, prim)
    du, dv = np.asarray(du, dtype=np.float64).reshape(-1, 1), np.asarray(dv, dtype=np.float64).reshape(-1, 1)
    return np.abs(c1 - c0) * du + np.abs(c2 - c0) * dv


def within_bound(got32, value, bound):
    """got32 [n][3] float32 against color64's (value, bound) -> boolean [n][3]"""
    return np.abs(np.asarray(got32, dtype=np.float64) - value) <= bound * TOL32 + DENORM
