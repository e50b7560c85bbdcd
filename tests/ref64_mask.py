"""A binary64 restatement of the Mask BSDF (src/bsdfs/mask.cpp:73-161, typeMask = EAll, component = -1) over the nested models
of tests/ref64.py and tests/ref64_ward.py, a float32 mirror of the mask's own operations in the reference's order, the luminance
of an RGB spectrum (spectrum.h:387-389), and the check that holds the mirror to the restatement.  Written from the reference
sources, not from csrc/.  Test infrastructure.

What the mask adds to its nested BSDF is a handful of operations, and the check looks at exactly those:
  p       = (r * 0.212671f + g * 0.715160f) + b * 0.072169f       the binary32 value lies within three roundings of the sum
  f, pdf  = nested * p                                              one rounding each
  sample  : s.x <= p compares two binary32 values, so both precisions decide alike; the nested sample is drawn at s.x / p,
            which the reference forms in binary32: one correctly rounded division, the same value as the binary64 quotient
            rounded once (53 >= 2 * 24 + 2), so the nested models of both readings get the same query;
            otherwise wo = -wi, sampledType = EDeltaTransmission, pdf = (1 - p) |cosTheta(wo)|, value 1 - p.
Both readings take p as a binary32 value (the restatement promoted), as ref64 takes every query.  The records with p == 0 and
s.x == 0 divide 0 by 0 in the reference; `undefined` names them and nothing compares them."""
import numpy as np

import ref64
import ref64_ward

F = np.float32
U24 = 2.0 ** -24
LUM_WEIGHTS = (F(0.212671), F(0.715160), F(0.072169))
DELTA_TRANS, GLOSSY_REFL = ref64.DELTA_TRANS, ref64.GLOSSY_REFL
MUTATIONS = ("lt_for_le", "sx_not_rescaled", "pdf_without_cos", "value_one", "only_z_negated", "channel_mean", "glossy_type",
             "f_not_scaled")
_TABLE = ref64_ward.Table()


def luminance64(rgb):
    """getLuminance of binary32 channels with the binary32 weights, summed exactly enough"""
    c = np.asarray(rgb, dtype=np.float32).astype(np.float64).reshape(-1, 3)
    w = [float(x) for x in LUM_WEIGHTS]
    return (c[:, 0] * w[0] + c[:, 1] * w[1]) + c[:, 2] * w[2]


def luminance32(rgb, mutation=None):
    """the same in binary32, every operation rounded, in the reference's order"""
    c = np.asarray(rgb, dtype=np.float32).reshape(-1, 3)
    if mutation == "channel_mean":
        return ((c[:, 0] + c[:, 1]) + c[:, 2]) * F(1.0 / 3.0)
    return (c[:, 0] * LUM_WEIGHTS[0] + c[:, 1] * LUM_WEIGHTS[1]) + c[:, 2] * LUM_WEIGHTS[2]


def luminance_bound(rgb):
    """|binary32 - binary64| of the luminance: two products and two sums, each rounded once, on terms of one sign or another"""
    c = np.abs(np.asarray(rgb, dtype=np.float32).astype(np.float64).reshape(-1, 3))
    w = [float(x) for x in LUM_WEIGHTS]
    return 3 * U24 * (c[:, 0] * w[0] + c[:, 1] * w[1] + c[:, 2] * w[2]) + 2.0 ** -149


def nested(btype, P, op, wi, aux):
    """the nested BSDF as a batch evaluator with the layout of mtsgpu_bsdf_eval, in binary64: op 0 -> f [n][0:3], op 1 -> pdf
    [n][0], op 2 -> wo, pdf, f, sampledType of sample(bRec, pdf, s); zero where the sample fails"""
    aux = np.atleast_2d(np.asarray(aux, dtype=np.float32))
    out = np.zeros((len(aux), 8), dtype=np.float64)
    with np.errstate(all="ignore"):
        if op == 0:
            out[:, 0:3] = _TABLE.f(btype, P, wi, aux)[0]
        elif op == 1:
            out[:, 0] = _TABLE.pdf(btype, P, wi, aux)[0]
        else:
            r = _TABLE.sample(btype, P, wi, aux)
            if r.delta:
                fv, pv = r.f, r.pdf
            else:
                fv, pv = _TABLE.f(btype, P, wi, r.wo)[0], _TABLE.pdf(btype, P, wi, r.wo)[0]
            ok = r.alive
            out[:, 0:3] = np.where(ok[:, None], r.wo, 0.0)
            out[:, 3] = np.where(ok, pv, 0.0)
            out[:, 4:7] = np.where(ok[:, None], fv, 0.0)
            out[:, 7] = np.where(ok, r.stype, 0)
    return np.nan_to_num(out, nan=0.0, posinf=0.0, neginf=0.0)


class Result:
    """op 0: f; op 1: pdf; op 2: took_nested, sx (the nested query's x), wo, pdf, f, stype"""


def undefined(p, s):
    p = np.asarray(p, dtype=np.float32); s = np.asarray(s, dtype=np.float32).reshape(-1, 2)
    return (p == 0) & (s[:, 0] == 0)


def _prep(p, wi, aux):
    aux = np.atleast_2d(np.asarray(aux, dtype=np.float32))
    n = len(aux)
    wi = np.broadcast_to(np.asarray(wi, dtype=np.float32).reshape(-1, 3), (n, 3))
    p = np.broadcast_to(np.asarray(p, dtype=np.float32).reshape(-1), (n,))
    return p, wi, aux, n


def mask64(btype, P, p, op, wi, aux):
    """Mask::f (:73-75), pdf (:81-83), sample(bRec, pdf, s) (:127-161) in binary64"""
    p, wi, aux, n = _prep(p, wi, aux)
    p64, wi64 = p.astype(np.float64), wi.astype(np.float64)
    r = Result()
    if op == 0:
        r.f = nested(btype, P, 0, wi, aux)[:, 0:3] * p64[:, None]
    elif op == 1:
        r.pdf = nested(btype, P, 1, wi, aux)[:, 0] * p64
    else:
        sx = aux[:, 0].astype(np.float64)
        r.took_nested = sx <= p64
        with np.errstate(all="ignore"):
            r.sx = np.where(r.took_nested, sx / p64, sx)
        q = aux.copy(); q[:, 0] = r.sx.astype(np.float32)          # the nested models take binary32 queries
        nv = nested(btype, P, 2, wi, np.nan_to_num(q))
        t = r.took_nested
        r.wo = np.where(t[:, None], nv[:, 0:3], -wi64)
        r.pdf = np.where(t, nv[:, 3] * p64, (1 - p64) * np.abs(wi64[:, 2]))
        r.f = np.where(t[:, None], nv[:, 4:7] * p64[:, None], (1 - p64)[:, None] * np.ones(3))
        r.stype = np.where(t, nv[:, 7], DELTA_TRANS).astype(np.int64)
    return r


def mask32(btype, P, p, op, wi, aux, mutation=None):
    """the mask's own operations in binary32, each rounded once, around the binary64 nested models rounded to binary32"""
    p, wi, aux, n = _prep(p, wi, aux)
    r = Result()
    if op == 0:
        nf = nested(btype, P, 0, wi, aux)[:, 0:3].astype(np.float32)
        r.f = nf if mutation == "f_not_scaled" else nf * p[:, None]
    elif op == 1:
        r.pdf = nested(btype, P, 1, wi, aux)[:, 0].astype(np.float32) * p
    else:
        sx = aux[:, 0]
        r.took_nested = (sx < p) if mutation == "lt_for_le" else (sx <= p)
        with np.errstate(all="ignore"):
            r.sx = np.where(r.took_nested & (mutation != "sx_not_rescaled"), sx / p, sx).astype(np.float32)
        q = aux.copy(); q[:, 0] = r.sx
        nv = nested(btype, P, 2, wi, np.nan_to_num(q))
        t = r.took_nested
        one = F(1)
        through = wi * np.float32([1, 1, -1]) if mutation == "only_z_negated" else -wi
        tpdf = (one - p) if mutation == "pdf_without_cos" else (one - p) * np.abs(through[:, 2])
        tval = np.ones(n, dtype=np.float32) if mutation == "value_one" else (one - p)
        r.wo = np.where(t[:, None], nv[:, 0:3].astype(np.float32), through)
        r.pdf = np.where(t, nv[:, 3].astype(np.float32) * p, tpdf)
        r.f = np.where(t[:, None], nv[:, 4:7].astype(np.float32) * p[:, None], tval[:, None] * np.ones(3, dtype=np.float32))
        r.stype = np.where(t, nv[:, 7], GLOSSY_REFL if mutation == "glossy_type" else DELTA_TRANS).astype(np.int64)
    return r


def _close(a32, a64, roundings):
    """binary32 values within `roundings` roundings of the binary64 ones (relative; the smallest denormal absolute)"""
    a64 = np.asarray(a64, dtype=np.float64)
    return np.abs(np.asarray(a32, dtype=np.float64) - a64) <= roundings * U24 * np.abs(a64) + 2.0 ** -149


def check(op, got, want, skip=None):
    """the indices of the records on which the mirror `got` (mask32) departs from the restatement `want` (mask64); skip: a mask
    of records that are not compared (undefined())"""
    if op == 0:
        bad = ~_close(got.f, want.f, 2).all(axis=1)            # the nested value rounded, the product rounded
    elif op == 1:
        bad = ~_close(got.pdf, want.pdf, 2)
    else:
        bad = got.took_nested != want.took_nested
        with np.errstate(invalid="ignore"):
            bad |= got.sx.astype(np.float64) != want.sx.astype(np.float32).astype(np.float64)   # the one correctly rounded quotient
        t = want.took_nested
        # nested: the nested models saw the same query, so wo and the type agree exactly; pass-through: -wi is exact
        bad |= (got.wo.astype(np.float64) != np.where(t[:, None], want.wo.astype(np.float32).astype(np.float64), want.wo)).any(axis=1)
        bad |= got.stype != want.stype
        bad |= ~_close(got.pdf, want.pdf, 2)                   # nested: value, product; pass-through: 1 - p, product
        bad |= ~_close(got.f, want.f, 2).all(axis=1)
    if skip is not None:
        bad &= ~skip
    return np.nonzero(bad)[0]
