"""The snow BRDFs of the reference, Wiscombe (src/bsdfs/wiscombe.cpp) and HanrahanKrueger (src/bsdfs/hanrahan-krueger.cpp):
a binary64 restatement of both configure()s and of f / pdf / sample(bRec, pdf, s) that carries a first-order bound on what a
binary32 evaluation may differ by, and a float32 mirror in the reference's operation order.  Written from the reference sources,
not from csrc/.  Test infrastructure.

The restatement (configure64, eval64) computes with `E`, a binary64 value next to a bound on |binary32 evaluation - value|:
every binary32 operation of the formula adds one rounding -- half a unit in the last place of the largest value the result
can take, 2^(floor(log2(|result| + bound)) - 24), and 2^-150 in the denormals -- to the bound its operands propagate to first
order (the second-order term of a product is kept as well); a product with an exact power of two adds none, and a result
that can exceed the largest binary32 number has no bound (1 / (|cos wi| + |cos wo|) of two denormal cosines overflows).  Sub-expressions the reference forms in
binary64 because of a double literal (1.07 * mu0 - 0.84; 1.0 - gSq; the base of the phase function; (4.0 / 3.0) * A) propagate
their operands' bounds and add one rounding where the result is stored in a Float.  Queries are binary32 values promoted, so
they carry no bound.  A sampled direction is compared on its own (ref64.square_to_hemisphere_psa and its DIR_REACH); the value
of a sample is then restated at the mirror's binary32 direction, as tests/ref64_mask.py restates a nested sample.

Every discrete decision -- wi.z <= 0, wo.z <= 0, cosThetaI < 0, sinThetaT > 1 in fresnel (util.cpp:704-727), eta > 1 and
eta == 1 in HanrahanKrueger::configure -- is recorded by both readings (`dec`), so that a record on which they part can be named.

The mirror (configure32, eval32) is binary32 numpy in the operation order of the sources with the operators as compiled
(spectrum.h: Float * Spectrum and Float / Spectrum are friends that return spd * f and spd / f; Spectrum / Float multiplies by
1.0f / f), with two specifications in place of libm:
  std::exp(x)         dexp: the binary64 polynomial below, rounded once
  std::pow(base, 1.5) base * sqrt(base) in binary64 with the correctly rounded sqrt, rounded once (within 1 ulp of binary32 of pow:
                      the binary64 product is within 2 ulp of binary64 of base^1.5)
and the polynomial sine / cosine of squareToHemispherePSA."""
import numpy as np

import ref64

F = np.float32
U24 = 2.0 ** -24
TINY = 2.0 ** -149
INV_PI = F(0.31830988618379067154)
PI32 = F(3.14159265358979323846)
EPSILON = F(1e-4)
NONE, WISCOMBE, HK = 0, 1, 2
TWOSIDED = 0x100
DIFFUSE_REFL = ref64.DIFFUSE_REFL
FRAGILE_RELATIVE = 1e-3
MUTATIONS = ("bstar_inverted", "mu_swapped", "f_one_inv_pi", "sample_two_inv_pi", "sample_signed_cos", "ft_same_direction",
             "dot_without_minus", "exponent_one", "diffuse_without_F", "eta_inverted", "fdr_fits_swapped")
CONFIGURE_MUTATIONS = ("bstar_inverted", "eta_inverted", "fdr_fits_swapped")


# ---------------------------------------------------------------------------------------------------------------------
# binary64 values with a bound on the binary32 evaluation
# ---------------------------------------------------------------------------------------------------------------------
class E:
    """v: the binary64 value; e: a bound on |the binary32 evaluation of the same expression - v|"""

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.broadcast_to(np.asarray(e, dtype=np.float64), self.v.shape)

    @staticmethod
    def lift(x):
        return x if isinstance(x, E) else E(x)

    def rounded(self):
        """one rounding to binary32: half an ulp of the binade the binary32 result can lie in"""
        with np.errstate(all="ignore"):
            top = np.nan_to_num(np.abs(self.v) + self.e, nan=np.inf, posinf=np.inf)
            half = np.where(np.isfinite(top) & (top > 0), np.ldexp(1.0, np.floor(np.log2(np.where(top > 0, top, 1.0))).astype(np.int64).clip(-126, 1023) - 24), 0.0)
            half = np.where(np.isfinite(top) & (top < 3.4028235677973366e38), half, np.inf)        # binary32 may overflow: no bound
        return E(self.v, self.e + half)

    def _pow2(self):
        """exactly a power of two, known exactly: scaling by it is exact (above the denormals)"""
        with np.errstate(all="ignore"):
            m, _ = np.frexp(self.v)
        return (np.abs(m) == 0.5) & (self.e == 0)

    def __neg__(self):
        return E(-self.v, self.e)

    def __abs__(self):
        return E(np.abs(self.v), self.e)

    def add64(self, o):
        o = E.lift(o)
        return E(self.v + o.v, self.e + o.e)

    def mul64(self, o):
        o = E.lift(o)
        with np.errstate(invalid="ignore", over="ignore"):
            return E(self.v * o.v, np.nan_to_num(np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e, nan=np.inf))

    def div64(self, o):
        o = E.lift(o)
        with np.errstate(all="ignore"):
            q = self.v / o.v
            den = np.abs(o.v) - o.e
            e = np.where(den > 0, (self.e + np.abs(q) * o.e) / np.where(den > 0, den, 1.0), np.inf)
            e = np.where((self.e == 0) & (o.e == 0), 0.0, e)
        return E(q, np.nan_to_num(e, nan=np.inf))

    def sqrt64(self):
        with np.errstate(all="ignore"):
            r = np.sqrt(np.maximum(self.v, 0.0))
            lo = np.sqrt(np.maximum(self.v - self.e, 0.0))
            e = np.where(self.e == 0, 0.0, self.e / np.where(r + lo > 0, r + lo, TINY))
        return E(np.sqrt(self.v), e)

    def __add__(self, o):
        return self.add64(o).rounded()

    __radd__ = __add__

    def __sub__(self, o):
        return self.add64(-E.lift(o)).rounded()

    def __rsub__(self, o):
        return E.lift(o).add64(-self).rounded()

    def __mul__(self, o):
        o = E.lift(o)
        p = self.mul64(o)
        r = p.rounded()
        exact = (self._pow2() | o._pow2()) & (np.abs(p.v) >= 2.0 ** -126)
        return E(p.v, np.where(exact, p.e, r.e))

    __rmul__ = __mul__

    def __truediv__(self, o):
        return self.div64(o).rounded()

    def __rtruediv__(self, o):
        return E.lift(o).div64(self).rounded()

    def sqrt(self):
        return self.sqrt64().rounded()

    def exp(self):
        """dexp: the polynomial is within 2^-45 of exp, relative"""
        with np.errstate(over="ignore"):
            v = np.exp(self.v)
            return E(v, v * (np.expm1(self.e) + 2.0 ** -45)).rounded()


def where(c, a, b):
    a, b = E.lift(a), E.lift(b)
    return E(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


def stack(items):
    return E(np.stack([i.v for i in items], axis=-1), np.stack([np.broadcast_to(i.e, i.v.shape) for i in items], axis=-1))


# ---------------------------------------------------------------------------------------------------------------------
# the specifications in place of libm, in binary64 numpy (the operations of csrc/devmath.h are plain IEEE binary64)
# ---------------------------------------------------------------------------------------------------------------------
def dexp32(x):
    """std::exp of a binary32 argument: reduction by ln 2 in two parts, a degree-13 Taylor polynomial, one rounding"""
    x = np.asarray(x, dtype=np.float32)
    xd = x.astype(np.float64)
    with np.errstate(all="ignore"):
        kd = xd * 1.44269504088896338700e+00
        k = np.trunc(np.nan_to_num(kd + np.where(kd >= 0, 0.5, -0.5)))
        r = (xd - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10
        p = np.full_like(r, 1.0 / 6227020800.0)
        for c in (479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0):
            p = p * r + 1.0 / c
        p = p * r + 0.5
        p = p * r + 1.0
        p = p * r + 1.0
        out = (p * np.ldexp(1.0, np.clip(k, -1022, 1023).astype(np.int64))).astype(np.float32)
    out = np.where(xd > 89.0, F(np.inf), np.where(xd < -104.0, F(0), out))
    return np.where(np.isnan(x), x, out).astype(np.float32)


def sincos32(x):
    """(sin, cos) of a binary32 argument: reduction by pi / 2 in two parts, Taylor polynomials of degree 15 / 14, one rounding"""
    xd = np.asarray(x, dtype=np.float32).astype(np.float64)
    kd = xd * 0.63661977236758134308
    k = np.trunc(kd + np.where(kd >= 0, 0.5, -0.5))
    r = (xd - k * 1.57079632679489655800e+00) - k * 6.12323399573676603587e-17
    r2 = r * r
    ps = np.full_like(r, -1.0 / 1307674368000.0)
    for c, sgn in ((6227020800.0, 1), (39916800.0, -1), (362880.0, 1), (5040.0, -1), (120.0, 1), (6.0, -1)):
        ps = ps * r2 + sgn * (1.0 / c)
    sr = r + r * (r2 * ps)
    pc = np.full_like(r, -1.0 / 87178291200.0)
    for c, sgn in ((479001600.0, 1), (3628800.0, -1), (40320.0, 1), (720.0, -1), (24.0, 1)):
        pc = pc * r2 + sgn * (1.0 / c)
    pc = pc * r2 - 0.5
    cr = 1.0 + r2 * pc
    q = k.astype(np.int64) & 3
    s = np.where(q == 0, sr, np.where(q == 1, cr, np.where(q == 2, -sr, -cr)))
    c = np.where(q == 0, cr, np.where(q == 1, -sr, np.where(q == 2, -cr, sr)))
    return s.astype(np.float32), c.astype(np.float32)


def pow15_32(base):
    """std::pow(base, 1.5) of a binary64 base, as specified above"""
    base = np.asarray(base, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (base * np.sqrt(base)).astype(np.float32)


def hemisphere_psa32(s):
    """squareToHemispherePSA (util.cpp:572-588) in binary32"""
    s = np.asarray(s, dtype=np.float32).reshape(-1, 2)
    r = np.sqrt(s[:, 0])
    phi = (F(2.0) * PI32) * s[:, 1]
    sn, cs = sincos32(phi)
    x, y = r * cs, r * sn
    q = x * x + y * y
    z = np.sqrt(F(1) - np.where(q < F(1), q, F(1)))
    rim = z == 0
    with np.errstate(all="ignore"):
        inv = F(1) / np.sqrt((x * x + y * y) + EPSILON * EPSILON)
    return np.stack([np.where(rim, x * inv, x), np.where(rim, y * inv, y), np.where(rim, EPSILON * inv, z)], axis=1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# configure()
# ---------------------------------------------------------------------------------------------------------------------
def wiscombe_raw(g=0.874, depth=1.0, w0=0.99, sigma_t=(16.4967, 6.0957, 4.6547)):
    """what Wiscombe::serialize writes (wiscombe.cpp:172-179), the defaults of its constructor (:44-55)"""
    return np.float32([g, depth] + list(np.broadcast_to(np.float32(w0), (3,))) + list(np.broadcast_to(np.float32(sigma_t), (3,))))


def hk_raw(sigma_a=(0.0014, 0.0025, 0.0142), sigma_s=(0.7, 1.22, 1.9), size_multiplier=1.0, g=0.0, eta_int=1.32, eta_ext=1.0,
           ss_factor=1.0, dr_factor=1.0, diffuse_reflectance=True):
    """the members HanrahanKrueger::configure reads, the defaults of its constructor (hanrahan-krueger.cpp:46-74)"""
    m = F(size_multiplier)
    b = lambda v: list(np.broadcast_to(np.float32(v), (3,)))
    return np.float32([x * m for x in b(sigma_a)] + [x * m for x in b(sigma_s)] + [g, eta_int, eta_ext] + b(ss_factor) + b(dr_factor)
                      + [1.0 if diffuse_reflectance else 0.0])


def configure32(kind, raw, mutation=None):
    """-> (derived [14] float32, dec): the mirror of Wiscombe::configure (:70-101) / HanrahanKrueger::configure (:89-132)"""
    raw = np.asarray(raw, dtype=np.float32)
    D = np.zeros(14, dtype=np.float32)
    one = F(1)
    with np.errstate(all="ignore"):
        if kind == WISCOMBE:
            g, w0 = raw[0], raw[2:5]
            gSq = g * g
            wStar = (w0 * (one - gSq)) / (one - w0 * gSq)
            gStar = g / (one + g)
            bTmp = one - wStar * gStar
            bStar = gStar / bTmp if mutation == "bstar_inverted" else bTmp * (one / gStar)
            xiSq = ((one - wStar * gStar) * (one - wStar)) * F(3)
            xi = np.sqrt(xiSq)
            P = (xi * F(2)) / ((one - wStar * gStar) * F(3))
            D[0:3], D[3:6], D[6:9], D[9:12] = wStar, bStar, xi, P
            return D, ()
        sigmaA, sigmaS, g = raw[0:3], raw[3:6], raw[6]
        eta = raw[8] / raw[7] if mutation == "eta_inverted" else raw[7] / raw[8]
        sigmaT = sigmaA + sigmaS
        albedo = sigmaS / sigmaT
        sigmaSPrime = sigmaS * (one - g)
        sigmaTPrime = sigmaA + sigmaSPrime
        reducedAlbedo = sigmaSPrime / sigmaTPrime
        groenhuis = ((F(-1.440) / (eta * eta) + F(0.710) / eta) + F(0.668)) + F(0.0636) * eta
        egan = ((F(-0.4399) + F(0.7099) / eta) - F(0.3319) / (eta * eta)) + F(0.0636) / ((eta * eta) * eta)
        big = bool(eta > 1)
        Fdr = (egan if big else groenhuis) if mutation == "fdr_fits_swapped" else (groenhuis if big else egan)
        Fdt = one - Fdr
        if eta == one:
            Fdr, Fdt = F(0), F(1)
        A = (one + Fdr) / Fdt
        var1 = -np.sqrt((one - reducedAlbedo) * F(3))
        fourThirdsA = F((4.0 / 3.0) * float(A))
        dr = ((reducedAlbedo * (one / F(2))) * (one + dexp32(var1 * fourThirdsA))) * dexp32(var1)
        D[0:3], D[3:6], D[6:9] = albedo, raw[9:12], dr * raw[12:15]
        D[9], D[10], D[11] = g, eta, F(1.0 if raw[15] != 0 else 0.0)
        return D, (big, bool(eta == one))


def configure64(kind, raw):
    """-> (derived E [14], dec): the restatement with its bounds"""
    raw = np.asarray(raw, dtype=np.float32).astype(np.float64)
    lit = lambda x: E(float(F(x)))                                 # a float literal of the source
    with np.errstate(all="ignore"):
        if kind == WISCOMBE:
            g, w0 = E(raw[0]), E(raw[2:5])
            gSq = g * g
            wStar = ((1 - gSq) * w0) / (1 - gSq * w0)
            gStar = g / (1 + g)
            bTmp = 1 - wStar * gStar
            bStar = bTmp * (1 / gStar)
            xi = ((1 - wStar * gStar) * (1 - wStar) * 3).sqrt()
            P = (2 * xi) / ((1 - wStar * gStar) * 3)
            parts, dec = [wStar, bStar, xi, P], ()
            tail = [E(0.0), E(0.0)]
        else:
            sigmaA, sigmaS, g = E(raw[0:3]), E(raw[3:6]), E(raw[6])
            eta = E(raw[7]) / E(raw[8])
            albedo = sigmaS / (sigmaA + sigmaS)
            sigmaSPrime = sigmaS * (1 - g)
            reducedAlbedo = sigmaSPrime / (sigmaA + sigmaSPrime)
            big, unit = bool(eta.v > 1), bool(eta.v == 1)
            if big:
                Fdr = lit(-1.440) / (eta * eta) + lit(0.710) / eta + lit(0.668) + lit(0.0636) * eta
            else:
                Fdr = lit(-0.4399) + lit(0.7099) / eta - lit(0.3319) / (eta * eta) + lit(0.0636) / (eta * eta * eta)
            Fdt = 1 - Fdr
            if unit:
                Fdr, Fdt = E(0.0), E(1.0)
            A = (1 + Fdr) / Fdt
            var1 = -((1 - reducedAlbedo) * 3).sqrt()
            fourThirdsA = E(4.0 / 3.0).mul64(A).rounded()
            dr = (reducedAlbedo * 0.5) * (1 + (var1 * fourThirdsA).exp()) * var1.exp()
            parts, dec = [albedo, E(raw[9:12]), dr * E(raw[12:15])], (big, unit)
            tail = [g, eta, E(1.0 if raw[15] != 0 else 0.0), E(0.0), E(0.0)]
        v = np.concatenate([p.v for p in parts] + [np.atleast_1d(t.v) for t in tail])
        e = np.concatenate([np.broadcast_to(p.e, (3,)) for p in parts] + [np.atleast_1d(t.e) for t in tail])
    return E(v, e), dec


# ---------------------------------------------------------------------------------------------------------------------
# f / pdf / sample(bRec, pdf, s): the float32 mirror
# ---------------------------------------------------------------------------------------------------------------------
def _fresnel32(c, ext, inte):
    """util.cpp:704-727 -> (F, (cosThetaI < 0, sinThetaT > 1))"""
    inside = c < 0
    etaI, etaT = np.where(inside, inte, ext).astype(np.float32), np.where(inside, ext, inte).astype(np.float32)
    t = F(1) - c * c
    sinT = etaI / etaT * np.sqrt(np.where(F(0) < t, t, F(0)))
    tir = sinT > F(1)
    with np.errstate(all="ignore"):
        cosT = np.sqrt(F(1) - sinT * sinT)
        c1 = np.abs(c)
        Rs = (etaI * c1 - etaT * cosT) / (etaI * c1 + etaT * cosT)
        Rp = (etaT * c1 - etaI * cosT) / (etaT * c1 + etaI * cosT)
        Fr = (Rs * Rs + Rp * Rp) / F(2)
    return np.where(tir, F(1), Fr).astype(np.float32), (inside, tir)


def _wiscombe_reflectance32(D, mu0, muPrime):
    """Wiscombe::reflectance (:122-127) with albedo (:133-135) -> [n][3]"""
    wStar, bStar, xi, P = D[None, 0:3], D[None, 3:6], D[None, 6:9], D[None, 9:12]
    b = (1.07 * mu0.astype(np.float64) - 0.84).astype(np.float32)
    fBar = (F(3) / (F(3) - b)) * (F(1) + b * (muPrime - F(1)))
    m = mu0[:, None]
    albedo = (wStar / (F(1) + P)) * ((F(1) - xi * m * bStar) / (F(1) + xi * m))
    return albedo * fBar[:, None] * INV_PI


def _hk_radiance32(D, wi, wo, mutation=None):
    """HanrahanKrueger::radiance (:171-193) with hgPhaseFunction (:140-147) -> ([n][3], dec)"""
    g, eta = D[9], D[10]
    cwi, cwo = wi[:, 2], wo[:, 2]
    R1, d1 = _fresnel32(cwo, F(1), eta)
    R2, d2 = _fresnel32(cwo if mutation == "ft_same_direction" else cwi, F(1), eta)
    Fq = (F(1) - R1) * (F(1) - R2)
    a = wi if mutation == "dot_without_minus" else -wi
    costheta = (a[:, 0] * wo[:, 0] + a[:, 1] * wo[:, 1]) + a[:, 2] * wo[:, 2]
    gSq = g * g
    num = F(1.0 - float(gSq))
    base = 1.0 + float(gSq) - 2.0 * float(g) * costheta.astype(np.float64)
    den = base.astype(np.float32) if mutation == "exponent_one" else pow15_32(base)
    with np.errstate(all="ignore"):
        p = (0.5 * (num / den).astype(np.float64)).astype(np.float32)
        recip = F(1) / (np.abs(cwi) + np.abs(cwo))
        f1 = D[None, 0:3] * Fq[:, None] * p[:, None] * recip[:, None]
        Lo = D[None, 3:6] * f1
        if D[11] != 0:
            Lo = Lo + (D[None, 6:9] * (F(1) if mutation == "diffuse_without_F" else Fq[:, None])) * INV_PI
    return Lo.astype(np.float32), d1 + d2


class Result:
    """op 0: f; op 1: pdf; op 2: wo, pdf, f, stype.  dec: the decisions taken, a tuple of boolean arrays"""


def _prep(wi, aux):
    aux = np.atleast_2d(np.asarray(aux, dtype=np.float32))
    wi = np.array(np.broadcast_to(np.asarray(wi, dtype=np.float32).reshape(-1, 3), (len(aux), 3)))
    return wi, aux.copy()


def eval32(kind, D, twosided, op, wi, aux, mutation=None, guard=True):
    """the mirror behind the TwoSidedBRDF adapter (twosided.cpp:80-130), layout of mtsgpu_bsdf_eval.  kind NONE: the
    Lambertian whose reflectance is D[0:3] (lambertian.cpp:95-126).  guard=False: the value expressions without the side
    tests in front of them (what a mutation behind a test that hides it would compute)"""
    D = np.asarray(D, dtype=np.float32)
    wi, aux = _prep(wi, aux)
    n = len(aux)
    r = Result()
    flip = (wi[:, 2] < 0) & bool(twosided)
    wi[flip, 2] *= F(-1)
    dec = ()
    with np.errstate(all="ignore"):
        if op in (0, 1):
            wo = aux[:, 0:3].copy()
            wo[flip, 2] *= F(-1)
            dead = ((wi[:, 2] <= 0) | (wo[:, 2] <= 0)) & guard
            if op == 1:
                r.pdf = np.where(dead, F(0), wo[:, 2] * INV_PI).astype(np.float32)
            elif kind == NONE:
                r.f = np.where(dead[:, None], F(0), np.broadcast_to(D[None, 0:3] * INV_PI, (n, 3))).astype(np.float32)
            elif kind == WISCOMBE:
                mu0, muPrime = (wi[:, 2], wo[:, 2]) if mutation == "mu_swapped" else (wo[:, 2], wi[:, 2])
                v = _wiscombe_reflectance32(D, mu0, muPrime)
                r.f = np.where(dead[:, None], F(0), v if mutation == "f_one_inv_pi" else v * INV_PI).astype(np.float32)
            else:
                v, dec = _hk_radiance32(D, wi, wo, mutation)
                r.f = np.where(dead[:, None], F(0), v * INV_PI).astype(np.float32)
            r.dec = (wi[:, 2] <= 0, wo[:, 2] <= 0) + tuple(d & ~dead for d in dec)      # (fresnel's only where its value is used)
            return r
        dead = (wi[:, 2] <= 0) & guard
        wo = hemisphere_psa32(aux[:, 0:2])
        pdf = wo[:, 2] * INV_PI
        if kind == NONE:
            v = np.broadcast_to(D[None, 0:3] * INV_PI, (n, 3))
        elif kind == WISCOMBE:
            cwi = wi[:, 2] if mutation == "sample_signed_cos" else np.abs(wi[:, 2])
            mu0, muPrime = (cwi, wo[:, 2]) if mutation == "mu_swapped" else (wo[:, 2], cwi)
            v = _wiscombe_reflectance32(D, mu0, muPrime)
            if mutation == "sample_two_inv_pi":
                v = v * INV_PI
        else:
            v, dec = _hk_radiance32(D, wi, wo, mutation)
            v = v * INV_PI
        v = np.where(dead[:, None], F(0), v).astype(np.float32)
        pdf = np.where(dead, F(0), pdf).astype(np.float32)
        wo = np.where(dead[:, None], F(0), wo).astype(np.float32)
        r.local_wo = wo.copy()                                     # what the nested sample() left, before the adapter's flip
        back = flip & ~dead & ~(v == 0).all(axis=1) & (pdf != 0)
        wo[back, 2] *= F(-1)
        r.wo, r.pdf, r.f, r.stype = wo, pdf, v, np.where(dead, 0, DIFFUSE_REFL).astype(np.int64)
        r.dec = (wi[:, 2] <= 0,) + tuple(d & ~dead for d in dec)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# f / pdf / sample(bRec, pdf, s): the binary64 restatement with its bounds
# ---------------------------------------------------------------------------------------------------------------------
def _fresnel64(c, ext, inte):
    """util.cpp:704-727 on a binary32 cosine promoted -> (E, (cosThetaI < 0, sinThetaT > 1))"""
    inside = c.v < 0
    etaI, etaT = where(inside, inte, ext), where(inside, ext, inte)
    t = 1 - c * c
    t = where(t.v > 0, t, E(0.0, 0.0))
    sinT = etaI / etaT * t.sqrt()
    tir = sinT.v > 1
    cosT = (1 - sinT * sinT).sqrt()
    c1 = abs(c)
    Rs = (etaI * c1 - etaT * cosT) / (etaI * c1 + etaT * cosT)
    Rp = (etaT * c1 - etaI * cosT) / (etaT * c1 + etaI * cosT)
    Fr = (Rs * Rs + Rp * Rp) / 2
    return where(tir, E(1.0), Fr), (inside, tir)


def _wiscombe_reflectance64(D, mu0, muPrime):
    wStar, bStar, xi, P = (E(D[3 * k:3 * k + 3][None, :].astype(np.float64)) for k in range(4))
    b = E(1.07).mul64(mu0).add64(-0.84).rounded()
    fBar = (3 / (3 - b)) * (1 + b * (muPrime - 1))
    m = E(mu0.v[:, None], mu0.e[:, None])
    albedo = (wStar / (1 + P)) * ((1 - xi * m * bStar) / (1 + xi * m))
    return albedo * E(fBar.v[:, None], fBar.e[:, None]) * float(INV_PI)


def _hk_radiance64(D, wi, wo):
    D = D.astype(np.float64)
    g, eta = D[9], D[10]
    cwi, cwo = E(wi[:, 2]), E(wo[:, 2])
    R1, d1 = _fresnel64(cwo, E(1.0), E(eta))
    R2, d2 = _fresnel64(cwi, E(1.0), E(eta))
    Fq = (1 - R1) * (1 - R2)
    costheta = (E(-wi[:, 0]) * E(wo[:, 0]) + E(-wi[:, 1]) * E(wo[:, 1])) + E(-wi[:, 2]) * E(wo[:, 2])
    gSq = E(g) * E(g)
    num = E(1.0).add64(-gSq).rounded()
    base = E(1.0).add64(gSq).add64(-(E(2.0 * g).mul64(costheta)))
    den = base.mul64(base.sqrt64()).rounded()
    p = (num / den).mul64(0.5)
    recip = 1 / (abs(cwi) + abs(cwo))
    col = lambda x: E(x.v[:, None], x.e[:, None])
    f1 = E(D[None, 0:3]) * col(Fq) * col(p) * col(recip)
    Lo = E(D[None, 3:6]) * f1
    if D[11] != 0:
        Lo = Lo + (E(D[None, 6:9]) * col(Fq)) * float(INV_PI)
    return Lo, d1 + d2


def eval64(kind, D, twosided, op, wi, aux, wo32=None):
    """the restatement, same layout; values are E.  op 2 takes the mirror's local (unflipped) binary32 direction wo32 as the
    query of the value and returns the binary64 direction of the sample next to it (wo, wo_cond)"""
    D = np.asarray(D, dtype=np.float32)
    wi, aux = _prep(wi, aux)
    wi = wi.astype(np.float64); aux = aux.astype(np.float64)
    n = len(aux)
    r = Result()
    flip = (wi[:, 2] < 0) & bool(twosided)
    wi[flip, 2] *= -1
    dec = ()
    inv_pi = float(INV_PI)
    with np.errstate(all="ignore"):
        if op in (0, 1):
            wo = aux[:, 0:3].copy()
            wo[flip, 2] *= -1
            dead = (wi[:, 2] <= 0) | (wo[:, 2] <= 0)
            if op == 1:
                r.pdf = where(dead, 0.0, E(wo[:, 2]) * inv_pi)
            elif kind == NONE:
                r.f = where(dead[:, None], 0.0, E(np.broadcast_to(D[None, 0:3].astype(np.float64), (n, 3))) * inv_pi)
            elif kind == WISCOMBE:
                r.f = where(dead[:, None], 0.0, _wiscombe_reflectance64(D, E(wo[:, 2]), E(wi[:, 2])) * inv_pi)
            else:
                v, dec = _hk_radiance64(D, wi, wo)
                r.f = where(dead[:, None], 0.0, v * inv_pi)
            r.dec = (wi[:, 2] <= 0, wo[:, 2] <= 0) + tuple(d & ~dead for d in dec)
            return r
        dead = wi[:, 2] <= 0
        d64, dcond = ref64.square_to_hemisphere_psa(aux[:, 0:2])
        wo = np.asarray(wo32, dtype=np.float32).astype(np.float64)
        pdf = E(wo[:, 2]) * inv_pi
        if kind == NONE:
            v = E(np.broadcast_to(D[None, 0:3].astype(np.float64), (n, 3))) * inv_pi
        elif kind == WISCOMBE:
            v = _wiscombe_reflectance64(D, E(wo[:, 2]), E(np.abs(wi[:, 2])))
        else:
            v, dec = _hk_radiance64(D, wi, wo)
            v = v * inv_pi
        r.f, r.pdf = where(dead[:, None], 0.0, v), where(dead, 0.0, pdf)
        back = flip & ~dead & ~(r.f.v == 0).all(axis=1) & (r.pdf.v != 0)
        d64 = np.where(dead[:, None], 0.0, d64)
        d64[back, 2] *= -1
        r.wo = d64
        r.wo_cond = dcond
        r.stype = np.where(dead, 0, DIFFUSE_REFL).astype(np.int64)
        r.dec = (wi[:, 2] <= 0,) + tuple(d & ~dead for d in dec)
    return r


# ---------------------------------------------------------------------------------------------------------------------
# holding the mirror to the restatement
# ---------------------------------------------------------------------------------------------------------------------
def _inside(got, want):
    """binary32 values inside the bound of the binary64 ones"""
    with np.errstate(invalid="ignore"):
        return np.abs(np.asarray(got, dtype=np.float64) - want.v) <= want.e


def fragile(got, want, op):
    """the records that are left out of the comparison: a discrete decision differs between the readings, or the bound of a
    value exceeds FRAGILE_RELATIVE of it.  Relative to max(|value|, 2^-126): below the smallest normal number binary32 has no
    relative precision to lose (one rounding there is up to the value itself), so such a value is held to its absolute bound"""
    out = np.zeros(len(got.dec[0]), dtype=bool)
    for a, b in zip(got.dec, want.dec):
        out |= np.asarray(a) != np.asarray(b)
    val = want.pdf if op == 1 else want.f
    with np.errstate(all="ignore"):
        rel = val.e / np.maximum(np.abs(val.v), 2.0 ** -126)
    rel = np.nan_to_num(rel, nan=np.inf)
    out |= (rel > FRAGILE_RELATIVE) if rel.ndim == 1 else (rel > FRAGILE_RELATIVE).any(axis=1)
    if op == 2:
        out |= want.pdf.e / np.maximum(np.abs(want.pdf.v), 2.0 ** -126) > FRAGILE_RELATIVE
    return out


def check(op, got, want, skip=None):
    """the indices of the records on which the mirror `got` (eval32) departs from the restatement `want` (eval64)"""
    if op == 0:
        bad = ~_inside(got.f, want.f).all(axis=1)
    elif op == 1:
        bad = ~_inside(got.pdf, want.pdf)
    else:
        reach = ref64.DIR_REACH * ref64.EPS32 * want.wo_cond
        bad = (np.abs(got.wo.astype(np.float64) - want.wo) > reach[:, None]).any(axis=1)
        bad |= got.stype != want.stype
        bad |= ~_inside(got.pdf, want.pdf)
        bad |= ~_inside(got.f, want.f).all(axis=1)
    if skip is not None:
        bad &= ~skip
    return np.nonzero(bad)[0]
