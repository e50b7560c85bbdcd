"""A binary64 restatement of the shading formulas on the path: the BSDF plugins (f, pdf, sample(bRec, pdf, s)), the
Fresnel terms of src/libcore/util.cpp and the radiance that a delta luminaire delivers to a point.  Written from the
reference sources, not from oracle/ or csrc/: a second, independent reading that the device and the oracle are both
held against (tests/test_closed_forms.py, tests/test_gpu_closed_forms.py).  Test infrastructure.

Every function takes the float32 query values promoted to float64, so what is left between a float32 evaluator and this
module is the evaluator's own rounding.  Each value comes with
  cond  a conditioning factor: the relative error that rounding every float32 operation of the formula once can cause,
        in units of 2^-23 (1 for a well-conditioned product, large where a cancellation or a steep function amplifies);
  amb   True where a branch of the formula is decided by a computed quantity that lies within float32 reach of its
        threshold (a side check, a TIR test, a lobe choice) or where float32 would under- or overflow: the two readings
        may then legitimately take different branches, and such records are not compared."""
import numpy as np

EPS32 = 2.0 ** -23
MARGIN = 1e-5                 # |quantity| below this (quantities of order 1): a float32 evaluator may decide either way
DIR_REACH = 64               # a sampled direction is trusted to DIR_REACH * 2^-23 * dir_cond per component

DIFFUSE_REFL, DIFFUSE_TRANS, DELTA_REFL, DELTA_TRANS, GLOSSY_REFL, GLOSSY_TRANS = 1, 2, 4, 8, 0x10, 0x20  # bsdf.h:157-167
LAMBERTIAN, DIELECTRIC, ROUGHMETAL, MICROFACET, MIRROR, PHONG, ROUGHGLASS, DIFFTRANS = range(8)
TWOSIDED = 0x100


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _normalize(v):
    # vector.h:403-405: v / v.length(), so a zero vector gives NaN
    with np.errstate(invalid="ignore", divide="ignore"):
        return v / np.sqrt(_dot(v, v))[:, None]


def _tan_theta(v):
    # include/mitsuba/core/frame.h:102-108
    t = 1.0 - v[:, 2] ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(t <= 0, 0.0, np.sqrt(np.maximum(t, 0)) / v[:, 2])


def _mix_cond(terms):
    """conditioning of a sum of (value, cond) terms: sum |v_i| cond_i / |sum v_i|, 1 where the sum is zero"""
    num = sum(np.abs(v) * c for v, c in terms)
    den = np.abs(sum(v for v, _ in terms))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1) + 1, 1.0)


def _relevant(amb, term, rest):
    """an under- or overflow flag of one term of a sum only matters where that term is not negligible next to the rest
    (float32 loses a term below 2^-24 of the sum anyway)"""
    with np.errstate(invalid="ignore"):
        return amb & ~(np.abs(term) < 1e-8 * np.abs(rest))


# ---------------------------------------------------------------------------------------------------------------------
# src/libcore/util.cpp
# ---------------------------------------------------------------------------------------------------------------------
def fresnel_dielectric(cos1, cos2, eta_i, eta_t):
    """util.cpp:680-688: the unpolarised mean of the two amplitude ratios squared"""
    with np.errstate(invalid="ignore", divide="ignore"):
        rs = (eta_i * cos1 - eta_t * cos2) / (eta_i * cos1 + eta_t * cos2)
        rp = (eta_t * cos1 - eta_i * cos2) / (eta_t * cos1 + eta_i * cos2)
    return 0.5 * (rs * rs + rp * rp)


def fresnel_conductor(cos, eta, k):
    """util.cpp:690-702; cos [n], eta / k [3] -> [n][3]"""
    c = np.asarray(cos, dtype=np.float64)[:, None]
    eta, k = np.asarray(eta, dtype=np.float64)[None, :], np.asarray(k, dtype=np.float64)[None, :]
    ek = eta * eta + k * k
    par = (ek * c * c - 2 * eta * c + 1) / (ek * c * c + 2 * eta * c + 1)
    perp = (ek - 2 * eta * c + c * c) / (ek + 2 * eta * c + c * c)
    return 0.5 * (par + perp)


def fresnel(cos_i, ext, inte):
    """util.cpp:704-725 -> (F, cond, amb).  Near the critical angle cos(theta_t) = sqrt(1 - sin^2) is steep: a float32
    error of eps in sin^2 moves cos(theta_t) by eps / cos^2(theta_t), relative."""
    c = np.asarray(cos_i, dtype=np.float64)
    inside = c < 0
    eta_i = np.where(inside, inte, ext); eta_t = np.where(inside, ext, inte)
    sin_t = eta_i / eta_t * np.sqrt(np.maximum(0.0, 1.0 - c * c))
    tir = sin_t > 1.0
    cos_t = np.sqrt(np.maximum(0.0, 1.0 - sin_t * sin_t))
    F = np.where(tir, 1.0, fresnel_dielectric(np.abs(c), cos_t, eta_i, eta_t))
    with np.errstate(divide="ignore"):
        cond = 4 + np.where(tir, 0.0, np.minimum(1.0 / np.maximum(cos_t * cos_t, 1e-300), 1e30))
    amb = np.abs(sin_t - 1.0) < MARGIN
    return F, cond, amb


# ---------------------------------------------------------------------------------------------------------------------
# Beckmann microfacets (roughmetal.cpp:79-117, microfacet.cpp:93-129; the same code in both plugins)
# ---------------------------------------------------------------------------------------------------------------------
def beckmann_d(m, alpha, hs=1.0):
    """roughmetal.cpp:79-84 -> (D, cond, amb).  hs bounds the float32 error of m itself (2 / |wi + wo| for a half-vector):
    exp(-x) with x = tan^2/alpha^2 = (1 - z^2) / (z^2 alpha^2) moves by |dx/dz| = 2 / (z^3 alpha^2) per unit of z."""
    z = m[:, 2]
    ex = _tan_theta(m) / alpha
    x = ex * ex
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        D = np.exp(-x) / (np.pi * alpha * alpha * z ** 4)
        cond = 2 + x + hs * (2.0 / (np.abs(z) ** 3 * alpha * alpha) + 4.0 / np.abs(z))
    amb = x > 86.0                           # float32 exp() underflows into the denormals beyond 87.3
    return D, cond, amb


def smith_beckmann_g1(v, m, alpha):
    """roughmetal.cpp:99-113 -> (G1, cond, amb); the rational fit above a = 1.6 is replaced by 1"""
    side = _dot(v, m) * v[:, 2]
    t = _tan_theta(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        a = 1.0 / (alpha * t)
        g = np.where(t == 0, 1.0, np.where(a >= 1.6, 1.0, (3.535 * a + 2.181 * a * a) / (1 + 2.276 * a + 2.577 * a * a)))
        cond = 2 + np.where((t == 0) | (a >= 1.6), 0.0, 4.0 / np.maximum(1 - v[:, 2] ** 2, 1e-300))
    g = np.where(side <= 0, 0.0, g)
    amb = (np.abs(_dot(v, m)) < MARGIN) | (np.abs(a - 1.6) < 1.6 * MARGIN)
    return g, cond, amb


def sample_beckmann(s, alpha):
    """roughmetal.cpp:89-94 with util.cpp:543-550 (sphericalDirection) -> (m, direction cond)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        th = np.arctan(np.sqrt(-alpha * alpha * np.log(1.0 - s[:, 0])))
        # log(1 - x) in float32 loses x's low bits when x is small (relative error eps / x in theta^2), and 1 - x itself
        # when x is close to 1 (relative error eps / (1 - x))
        dcond = 4 + alpha / np.sqrt(np.maximum(s[:, 0], 1e-300)) + alpha / np.maximum(1.0 - s[:, 0], 1e-300)
    ph = 2 * np.pi * s[:, 1]
    return np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1), dcond


def square_to_hemisphere_psa(s):
    """util.cpp:572-588 -> (direction, direction cond): z = sqrt(1 - r^2) is steep at the rim"""
    r = np.sqrt(s[:, 0]); ph = 2 * np.pi * s[:, 1]
    x, y = r * np.cos(ph), r * np.sin(ph)
    z = np.sqrt(1 - np.minimum(1.0, x * x + y * y))
    rim = z == 0
    d = np.stack([x, y, np.where(rim, 1e-4, z)], axis=1)           # Epsilon (constants.h:31) guard, normalised
    d[rim] /= np.linalg.norm(d[rim], axis=1)[:, None]
    with np.errstate(divide="ignore"):
        dcond = 4 + 1.0 / np.maximum(z * z, 1e-300)
    return d, dcond


def coordinate_system(a):
    """util.cpp:602-611: (b, c) completing a to an orthonormal frame"""
    ax = np.abs(a[:, 0]) > np.abs(a[:, 1])
    inv_xz = 1 / np.sqrt(a[:, 0] ** 2 + a[:, 2] ** 2); inv_yz = 1 / np.sqrt(a[:, 1] ** 2 + a[:, 2] ** 2)
    b = np.where(ax[:, None], np.stack([-a[:, 2] * inv_xz, 0 * a[:, 0], a[:, 0] * inv_xz], axis=1),
                 np.stack([0 * a[:, 0], -a[:, 2] * inv_yz, a[:, 1] * inv_yz], axis=1))
    return b, np.cross(a, b)


# ---------------------------------------------------------------------------------------------------------------------
# f / pdf of every plugin.  P = the parameter block of include/mtsgpu.h as float64; wi, wo [n][3] float64.
# Returned: (value, cond, amb); value is [n][3] for f and [n] for pdf.
# ---------------------------------------------------------------------------------------------------------------------
def _rgb(P, i):
    return np.asarray(P[i:i + 3], dtype=np.float64)[None, :]


def _both_up(wi, wo):
    return (wi[:, 2] > 0) & (wo[:, 2] > 0)


def _phong_lobe(P, wi, wo):
    """phong.cpp:114-131, :133-141: alpha = <R, wo> with R the mirror direction of wi; pow(alpha, n) amplifies
    alpha's rounding (3 eps absolute) n / alpha times and its own log n |ln alpha| times"""
    n = P[0]
    R = np.stack([-wi[:, 0], -wi[:, 1], wi[:, 2]], axis=1)
    al = _dot(R, wo)
    with np.errstate(divide="ignore", invalid="ignore"):
        p = np.where(al > 0, np.power(np.maximum(al, 0), n), 0.0)
        cond = 4 + np.where(al > 0, n * (3.0 / al + np.abs(np.log(np.maximum(al, 1e-300)))), 0.0)
    amb = (np.abs(al) < MARGIN) | ((al > 0) & (p > 0) & (p < 1e-30))
    return al, p, cond, amb


def _microfacet_parts(P, wi, wo, alpha):
    H = _normalize(wi + wo)
    with np.errstate(divide="ignore"):
        hs = 2.0 / np.sqrt(_dot(wi + wo, wi + wo))
    D, cD, aD = beckmann_d(H, alpha, hs)
    g1i, ci, ai = smith_beckmann_g1(wi, H, alpha)
    g1o, co, ao = smith_beckmann_g1(wo, H, alpha)
    return H, D, g1i * g1o, cD + ci + co, aD | ai | ao


def f(btype, P, wi, wo):
    """BSDF::f(bRec) with bRec.typeMask = EAll, component = -1, quantity = ERadiance"""
    P = _f64(P); wi = _f64(wi).reshape(-1, 3); wo = _f64(wo).reshape(-1, 3)
    n = len(wo); wi = np.broadcast_to(wi, (n, 3)).copy()
    if btype & TWOSIDED:
        # twosided.cpp:80-88: both directions mirrored through the surface when wi is below it
        flip = wi[:, 2] < 0
        wi[flip, 2] *= -1; wo = wo.copy(); wo[flip, 2] *= -1
        return f(btype & 0xFF, P, wi, wo)
    zero3, one, no = np.zeros((n, 3)), np.ones(n), np.zeros(n, dtype=bool)
    up = _both_up(wi, wo)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if btype == LAMBERTIAN:                                                         # lambertian.cpp:95-101
            return np.where(up[:, None], _rgb(P, 0) / np.pi, 0.0), one * 2, no
        if btype in (DIELECTRIC, MIRROR):                                               # dielectric.cpp:101-103, mirror.cpp:61-63
            return zero3, one, no
        if btype == DIFFTRANS:                                                          # difftrans.cpp:92-98
            return np.where((wi[:, 2] * wo[:, 2] < 0)[:, None], _rgb(P, 0) / np.pi, 0.0), one * 2, no
        if btype == ROUGHMETAL:                                                         # roughmetal.cpp:120-139
            alpha = P[0]
            H, D, G, c, amb = _microfacet_parts(P, wi, wo, alpha)
            F = fresnel_conductor(_dot(wi, H), P[1:4], P[4:7])
            v = _rgb(P, 7) * F * (D * G / (4 * wi[:, 2] * wo[:, 2]))[:, None]
            cond = c + 6 + 8 * hs_cos(wi, wo)
            return np.where(up[:, None], v, 0.0), np.where(up, cond, 1), up & amb
        if btype == MICROFACET:                                                         # microfacet.cpp:151-173
            alpha, kd, ks, inte, ext = P[0:5]
            H, D, G, c, amb = _microfacet_parts(P, wi, wo, alpha)
            F, cF, aF = fresnel(_dot(wi, H), ext, inte)
            spec = (D * G / (4 * wi[:, 2] * wo[:, 2]) * F * ks)[:, None] * _rgb(P, 8)
            diff = _rgb(P, 5) * ((1 - F) * kd / np.pi)[:, None]
            cs = c + cF + 6 + 8 * hs_cos(wi, wo)
            cd = 4 + cF * F / np.where(1 - F > 0, 1 - F, 1)
            cond = _mix_cond([(spec[:, 0], cs), (diff[:, 0], cd)])
            amb = _relevant(amb, spec[:, 0], diff[:, 0])
            return np.where(up[:, None], spec + diff, 0.0), np.where(up, cond, 1), up & (amb | aF)
        if btype == PHONG:                                                              # phong.cpp:104-131
            ne, kd, ks = P[0:3]
            al, p, cp, amb = _phong_lobe(P, wi, wo)
            spec = ((ne + 2) / (2 * np.pi) * p * ks)[:, None] * _rgb(P, 8)
            diff = np.broadcast_to(_rgb(P, 5) * (kd / np.pi), (n, 3))
            cond = _mix_cond([(spec[:, 0], cp), (diff[:, 0], 4 * one)])
            return np.where(up[:, None], spec + diff, 0.0), np.where(up, cond, 1), up & _relevant(amb, spec[:, 0], diff[:, 0])
        if btype == ROUGHGLASS:
            return _roughglass_f(P, wi, wo)
    raise ValueError(btype)


def hs_cos(wi, wo):
    """2 / |wi + wo|: how much the float32 rounding of wi + wo (eps per component) is amplified, relative, in the
    half-vector normalize(wi + wo)"""
    with np.errstate(divide="ignore"):
        return 2.0 / np.sqrt(_dot(wi + wo, wi + wo))


def pdf(btype, P, wi, wo):
    """BSDF::pdf(bRec), typeMask = EAll, component = -1, no sampler in the record (path.cpp:106,133 build it from the
    intersection alone)"""
    P = _f64(P); wi = _f64(wi).reshape(-1, 3); wo = _f64(wo).reshape(-1, 3)
    n = len(wo); wi = np.broadcast_to(wi, (n, 3)).copy()
    if btype & TWOSIDED:
        flip = wi[:, 2] < 0                                                             # twosided.cpp:90-98
        wi[flip, 2] *= -1; wo = wo.copy(); wo[flip, 2] *= -1
        return pdf(btype & 0xFF, P, wi, wo)
    zero, one, no = np.zeros(n), np.ones(n), np.zeros(n, dtype=bool)
    up = _both_up(wi, wo)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if btype == LAMBERTIAN:                                                         # lambertian.cpp:103-107
            return np.where(up, wo[:, 2] / np.pi, 0.0), one * 2, no
        if btype in (DIELECTRIC, MIRROR):
            return zero, one, no
        if btype == DIFFTRANS:                                                          # difftrans.cpp:100-104
            return np.where(wi[:, 2] * wo[:, 2] < 0, np.abs(wo[:, 2]) / np.pi, 0.0), one * 2, no
        if btype == ROUGHMETAL:                                                         # roughmetal.cpp:141-149
            alpha = P[0]
            H = _normalize(wi + wo)
            D, cD, aD = beckmann_d(H, alpha, hs_cos(wi, wo))
            v = D * H[:, 2] / (4 * np.abs(_dot(wo, H)))
            return np.where(up, v, 0.0), np.where(up, cD + 6 + 4 * hs_cos(wi, wo), 1), up & aD
        if btype == MICROFACET:                                                         # microfacet.cpp:175-205
            alpha, kd, ks, inte, ext = P[0:5]
            fr, cF, aF = fresnel(wi[:, 2], ext, inte)
            fr = np.clip(fr, 0.05, 0.95)
            dsw, ssw = (1 - fr) * kd, fr * ks
            norm = 1 / (dsw + ssw)
            H = _normalize(wi + wo)
            D, cD, aD = beckmann_d(H, alpha, hs_cos(wi, wo))
            ps = D * H[:, 2] / (4 * np.abs(_dot(wo, H)))
            pd = wo[:, 2] / np.pi
            cond = _mix_cond([(ssw * ps * norm, cD + 6 + 4 * hs_cos(wi, wo) + cF), (dsw * pd * norm, 4 + cF)])
            aD = _relevant(aD, ssw * ps, dsw * pd)
            return np.where(up, (ssw * ps + dsw * pd) * norm, 0.0), np.where(up, cond, 1), up & (aD | aF)
        if btype == PHONG:                                                              # phong.cpp:133-160
            ne, ssw, dsw = P[0], P[3], P[4]
            al, p, cp, amb = _phong_lobe(P, wi, wo)
            ps = p * (ne + 1) / (2 * np.pi)
            pd = wo[:, 2] / np.pi
            cond = _mix_cond([(ssw * ps, cp), (dsw * pd, 4 * one)])
            return np.where(up, ssw * ps + dsw * pd, 0.0), np.where(up, cond, 1), up & _relevant(amb, ssw * ps, dsw * pd)
        if btype == ROUGHGLASS:
            return _roughglass_pdf(P, wi, wo)
    raise ValueError(btype)


# ---------------------------------------------------------------------------------------------------------------------
# roughglass (src/bsdfs/roughglass.cpp)
# ---------------------------------------------------------------------------------------------------------------------
def _signum(x):
    return np.where(x < 0, -1.0, 1.0)                                                  # roughglass.cpp:197-199


def rg_eval_d(distr, m, alpha, hs=1.0):
    """roughglass.cpp:209-250 -> (D, cond, amb); D below 1e-40 is set to 0"""
    z = m[:, 2]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        t = _tan_theta(m)
        if distr == 0:
            D, c, amb = beckmann_d(m, alpha, hs)
        elif distr == 1:
            D = (alpha + 2) / (2 * np.pi) * np.power(np.maximum(z, 0), alpha)
            c = 4 + alpha * (hs / np.maximum(z, 1e-300) + np.abs(np.log(np.maximum(z, 1e-300))))
            amb = (D > 0) & (D < 1e-30)
        else:
            root = alpha / (z * z * (alpha * alpha + t * t))
            D = root * root / np.pi
            # (z^2 alpha^2 + 1 - z^2): the float32 rounding of z moves it by 2 z (1 - alpha^2) eps
            c = 6 + 4 * hs * (1 + np.abs(1 - alpha * alpha) * z * z / (z * z * alpha * alpha + t * t * z * z)) / np.maximum(z, 1e-300)
            amb = np.zeros(len(z), dtype=bool)
    below = ~(z > 0)                                 # cosTheta(m) <= 0 -> 0; a NaN normal passes on (below is False)
    below = np.where(np.isnan(z), False, below)
    D = np.where(below, 0.0, D)
    amb = amb | (np.abs(z) < MARGIN) | ((D > 0) & (np.abs(np.log(np.maximum(D, 1e-300)) - np.log(1e-40)) < 1.0))
    D = np.where(D < 1e-40, 0.0, D)
    return D, c, amb


def rg_smith_g1(distr, v, m, alpha):
    """roughglass.cpp:298-343 -> (G1, cond, amb): no shadowing at normal incidence, then the side check"""
    t = np.abs(_tan_theta(v))
    side = _dot(v, m) * v[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        if distr == 2:
            r = alpha * t
            g = 2.0 / (1.0 + np.sqrt(1.0 + r * r))
            a = np.full(len(t), np.inf)
        else:
            al = np.sqrt(0.5 * alpha + 1) / t if distr == 1 else alpha   # Walter's Beckmann stand-in for Phong
            a = 1.0 / (al * t)
            g = np.where(a >= 1.6, 1.0, (3.535 * a + 2.181 * a * a) / (1 + 2.276 * a + 2.577 * a * a))
        cond = 2 + np.where(t == 0, 0.0, 4.0 / np.maximum(1 - v[:, 2] ** 2, 1e-300))
    g = np.where(side <= 0, 0.0, g)
    g = np.where(t == 0, 1.0, g)
    amb = (t != 0) & ((np.abs(_dot(v, m)) < MARGIN) | (np.abs(a - 1.6) < 1.6 * MARGIN))
    return g, cond, amb


def _rg_half(P, wi, wo):
    distr, alpha, inte, ext = int(P[0]), P[1], P[2], P[3]
    refl = wi[:, 2] * wo[:, 2] > 0
    swap = wi[:, 2] < 0
    eta_i = np.where(swap, inte, ext); eta_t = np.where(swap, ext, inte)
    Hr = _normalize(wo + wi) * _signum(wo[:, 2])[:, None]
    ht = wi * eta_i[:, None] + wo * eta_t[:, None]
    Ht = (1.0 if ext > inte else -1.0) * _normalize(ht)
    H = np.where(refl[:, None], Hr, Ht)
    with np.errstate(divide="ignore", invalid="ignore"):
        hs = np.where(refl, 2.0 / np.sqrt(_dot(wi + wo, wi + wo)), 2.0 * (eta_i + eta_t) / np.sqrt(_dot(ht, ht)))
    return distr, alpha, inte, ext, refl, eta_i, eta_t, H, hs


def _roughglass_f(P, wi, wo):
    """roughglass.cpp:345-413"""
    distr, alpha, inte, ext, refl, eta_i, eta_t, H, hs = _rg_half(P, wi, wo)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        D, cD, aD = rg_eval_d(distr, H, alpha, hs)
        F, cF, aF = fresnel(_dot(wi, H), ext, inte)
        g1i, ci, ai = rg_smith_g1(distr, wi, H, alpha)
        g1o, co, ao = rg_smith_g1(distr, wo, H, alpha)
        G = g1i * g1o
        vr = F * D * G / (4 * wi[:, 2] * wo[:, 2])
        sd = eta_i * _dot(wi, H) + eta_t * _dot(wo, H)
        vt = ((1 - F) * D * G * eta_t * eta_t * _dot(wi, H) * _dot(wo, H)) / (wi[:, 2] * wo[:, 2] * sd * sd)
        vt = np.abs(vt * (eta_i * eta_i) / (eta_t * eta_t))
        # the transmitted value subtracts in sd = etaI <wi,H> + etaT <wo,H>: relative error of sd ~ hs (eta_i + eta_t) / |sd|
        ct = (cD + ci + co + cF * F / np.where(1 - F > 0, 1 - F, 1) + 10 + 4 * (eta_i + eta_t) * hs / np.abs(sd) + hs
              + 2 * hs / np.abs(_dot(wi, H)) + 2 * hs / np.abs(_dot(wo, H)))
        cr = cD + ci + co + cF + 8 + hs
    v = np.where(refl, vr, vt)
    v = np.where(D == 0, 0.0, v)                      # D == 0 -> f = 0 before anything else is looked at
    val = np.where(refl[:, None], _rgb(P, 4), _rgb(P, 7)) * v[:, None]
    amb = (aD | aF | ai | ao | (np.abs(H[:, 2]) < MARGIN)) & ~(D == 0) | aD
    return val, np.where(refl, cr, ct), amb


def _roughglass_pdf(P, wi, wo):
    """roughglass.cpp:415-485, clamped macro-surface Fresnel for the lobe choice (bRec.sampler is NULL)"""
    distr, alpha, inte, ext, refl, eta_i, eta_t, H, hs = _rg_half(P, wi, wo)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        dr = 1.0 / (4.0 * _dot(wo, H))
        sd = eta_i * _dot(wi, H) + eta_t * _dot(wo, H)
        dt = (eta_t * eta_t * _dot(wo, H)) / (sd * sd)
        dwh = np.where(refl, dr, dt)
        sa = alpha * (1.2 - 0.2 * np.sqrt(np.abs(wi[:, 2])))
        D, cD, aD = rg_eval_d(distr, H, sa, hs)
        F, cF, aF = fresnel(wi[:, 2], ext, inte)
        F = np.clip(F, 0.1, 0.9)
        prob = D * np.where(refl, F, 1 - F)
        v = np.abs(prob * H[:, 2] * dwh)
        cond = cD + cF + 8 + hs + np.where(refl, hs / np.abs(4 * _dot(wo, H)),
                                           4 * (eta_i + eta_t) * hs / np.abs(sd) + 2 * hs / np.abs(_dot(wo, H)))
        # the sampling alpha depends on sqrt|cos theta_i|: exponents / tan^2 / alpha^2 carry its rounding
        cond = cond + np.where(distr == 1, sa * 2, 2 + 2 * _tan_theta(H) ** 2 / sa ** 2)
    amb = aD | aF | (np.abs(H[:, 2]) < MARGIN)
    return v, cond, amb


# ---------------------------------------------------------------------------------------------------------------------
# sample(bRec, pdf, s): (wo, pdf, f, sampledType, alive, dir_cond, amb)
#   alive     False where the reference returns a zero spectrum (the evaluator then reports f = 0 and pdf = 0)
#   dir_cond  conditioning of the sampled direction (float32 error of each component, in units of eps); inf = only
#             the weight at the evaluator's own direction is comparable
# For the plugins without an override of sample(bRec, pdf, s) the weight is re-evaluated at the sampled direction
# (src/librender/bsdf.cpp:37-48): its f and pdf are those of f() / pdf() above at the evaluator's own wo.
# ---------------------------------------------------------------------------------------------------------------------
class Sample:
    def __init__(self, n):
        self.wo = np.zeros((n, 3)); self.pdf = np.zeros(n); self.f = np.zeros((n, 3))
        self.stype = np.zeros(n, dtype=np.int64); self.alive = np.zeros(n, dtype=bool)
        self.dir_cond = np.full(n, np.inf); self.amb = np.zeros(n, dtype=bool)
        self.delta = False           # True: f and pdf are the sample's own (no f()/pdf() to re-evaluate them with)
        self.cond = np.ones(n)


def sample(btype, P, wi, s):
    P = _f64(P); wi = _f64(wi).reshape(-1, 3); s = _f64(s).reshape(-1, 2)
    n = len(s); wi = np.broadcast_to(wi, (n, 3)).copy()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if btype & TWOSIDED:                                                            # twosided.cpp:115-127
            flip = wi[:, 2] < 0
            wi[flip, 2] *= -1
            r = sample(btype & 0xFF, P, wi, s)
            fl = flip & r.alive
            r.wo[fl, 2] *= -1
            return r
        r = _SAMPLERS[btype](P, wi, s)
    # a side test on a sampled direction is undecidable where the direction's own float32 error reaches it
    if btype & 0xFF in (ROUGHMETAL, MICROFACET, PHONG):
        reach = MARGIN + DIR_REACH * EPS32 * np.where(np.isfinite(r.dir_cond), r.dir_cond, 0)
        r.amb = r.amb | (np.abs(r.wo[:, 2]) < reach)
    return r


def _s_lambertian(P, wi, s):                                                            # lambertian.cpp:118-126
    r = Sample(len(s))
    r.alive = wi[:, 2] > 0
    r.wo, r.dir_cond = square_to_hemisphere_psa(s)
    r.pdf = r.wo[:, 2] / np.pi; r.f[:] = _rgb(P, 0) / np.pi; r.stype[:] = DIFFUSE_REFL
    return r


def _s_difftrans(P, wi, s):                                                             # difftrans.cpp:119-131
    r = Sample(len(s))
    r.wo, r.dir_cond = square_to_hemisphere_psa(s)
    r.wo[wi[:, 2] > 0, 2] *= -1
    r.pdf = np.abs(r.wo[:, 2]) / np.pi; r.f[:] = _rgb(P, 0) / np.pi; r.stype[:] = DIFFUSE_TRANS
    r.alive = r.wo[:, 2] != 0
    return r


def _s_mirror(P, wi, s):                                                                # mirror.cpp:78-86
    r = Sample(len(s))
    r.wo = np.stack([-wi[:, 0], -wi[:, 1], wi[:, 2]], axis=1); r.dir_cond[:] = 0
    r.pdf = np.abs(wi[:, 2]); r.f[:] = _rgb(P, 0); r.stype[:] = DELTA_REFL; r.alive[:] = True
    r.delta = True
    return r


def _s_dielectric(P, wi, s):                                                            # dielectric.cpp:205-261
    r = Sample(len(s))
    inte, ext = P[0], P[1]
    c = wi[:, 2]
    entering = c > 0
    eta_i = np.where(entering, ext, inte); eta_t = np.where(entering, inte, ext)
    eta = eta_i / eta_t
    st2 = eta * eta * (1 - c * c)
    tir = st2 >= 1
    ct = np.sqrt(np.maximum(0.0, 1 - st2))
    Fr = np.where(tir, 1.0, fresnel_dielectric(np.abs(c), ct, eta_i, eta_t))
    ct = np.where(entering, -ct, ct)
    refl = s[:, 0] <= Fr
    r.wo = np.where(refl[:, None], np.stack([-wi[:, 0], -wi[:, 1], wi[:, 2]], axis=1),
                    np.stack([-eta * wi[:, 0], -eta * wi[:, 1], ct], axis=1))
    r.pdf = np.where(refl, Fr, 1 - Fr) * np.abs(r.wo[:, 2])
    r.f = np.where(refl[:, None], _rgb(P, 2) * Fr[:, None], _rgb(P, 5) * ((1 - Fr) * eta * eta)[:, None])
    r.stype = np.where(refl, DELTA_REFL, DELTA_TRANS)
    r.alive[:] = True
    cF = 4 + np.where(tir, 0.0, 1.0 / np.maximum(ct * ct, 1e-300))
    r.cond = cF * (1 + np.where(refl, 1.0, Fr / np.where(1 - Fr > 0, 1 - Fr, 1)))
    r.dir_cond = np.where(refl, 0.0, cF)
    r.amb = (np.abs(st2 - 1) < MARGIN) | (~tir & (np.abs(s[:, 0] - Fr) < MARGIN * (1 + cF)))
    r.delta = True
    return r


def _s_phong(P, wi, s):                                                                 # phong.cpp:164-230
    r = Sample(len(s))
    ne, ssw, dsw = P[0], P[3], P[4]
    u = s.copy()
    spec = u[:, 0] <= ssw
    u[:, 0] = np.where(spec, u[:, 0] / ssw, (u[:, 0] - ssw) / dsw)
    R = np.stack([-wi[:, 0], -wi[:, 1], wi[:, 2]], axis=1)
    sin_a = np.sqrt(1 - np.power(u[:, 1], 2 / (ne + 1)))
    cos_a = np.power(u[:, 1], 1 / (ne + 1))
    ph = 2 * np.pi * u[:, 0]
    b, c = coordinate_system(R)
    ws = b * (sin_a * np.cos(ph))[:, None] + c * (sin_a * np.sin(ph))[:, None] + R * cos_a[:, None]
    wd, cd = square_to_hemisphere_psa(u)
    r.wo = np.where(spec[:, None], ws, wd)
    r.stype = np.where(spec, GLOSSY_REFL, DIFFUSE_REFL)
    cs = 8 + 4 / np.maximum(sin_a * sin_a, 1e-300) + 2 * np.abs(np.log(np.maximum(u[:, 1], 1e-300)))
    r.dir_cond = np.where(spec, cs / ssw, cd / dsw)
    fv, _, fa = f(PHONG, P, wi, r.wo)
    pv, _, pa = pdf(PHONG, P, wi, r.wo)
    r.alive = (wi[:, 2] > 0) & (r.wo[:, 2] > 0) & (pv != 0) & fv.any(axis=1)
    r.amb = (np.abs(s[:, 0] - ssw) < MARGIN) | fa | pa
    return r


def _s_beckmann_lobe(alpha, wi, u):
    m, dc = sample_beckmann(u, alpha)
    wo = 2 * _dot(wi, m)[:, None] * m - wi
    return wo, dc


def _s_roughmetal(P, wi, s):                                                            # roughmetal.cpp:151-164
    r = Sample(len(s))
    r.wo, r.dir_cond = _s_beckmann_lobe(P[0], wi, s)
    r.stype[:] = GLOSSY_REFL
    fv, _, fa = f(ROUGHMETAL, P, wi, r.wo)
    pv, _, pa = pdf(ROUGHMETAL, P, wi, r.wo)
    r.alive = (wi[:, 2] > 0) & (r.wo[:, 2] > 0) & fv.any(axis=1) & (pv != 0)
    r.amb = fa | pa
    return r


def _s_microfacet(P, wi, s):                                                            # microfacet.cpp:207-266
    r = Sample(len(s))
    alpha, kd, ks, inte, ext = P[0:5]
    fr, _, aF = fresnel(wi[:, 2], ext, inte)
    fr = np.clip(fr, 0.05, 0.95)
    dsw, ssw = (1 - fr) * kd, fr * ks
    norm = 1 / (dsw + ssw); dsw, ssw = dsw * norm, ssw * norm
    u = s.copy()
    spec = u[:, 0] < ssw
    u[:, 0] = np.where(spec, u[:, 0] / ssw, (u[:, 0] - ssw) / dsw)
    ws, dcs = _s_beckmann_lobe(alpha, wi, u)
    wd, dcd = square_to_hemisphere_psa(u)
    r.wo = np.where(spec[:, None], ws, wd)
    r.stype = np.where(spec, GLOSSY_REFL, DIFFUSE_REFL)
    r.dir_cond = np.where(spec, dcs / ssw, dcd / dsw)
    fv, _, fa = f(MICROFACET, P, wi, r.wo)
    pv, _, pa = pdf(MICROFACET, P, wi, r.wo)
    r.alive = (wi[:, 2] > 0) & (r.wo[:, 2] > 0) & (pv != 0) & fv.any(axis=1)
    r.amb = (np.abs(s[:, 0] - ssw) < MARGIN) | aF | fa | pa
    return r


def _s_roughglass(P, wi, s):                                                            # roughglass.cpp:496-617
    r = Sample(len(s))
    distr, alpha, inte, ext = int(P[0]), P[1], P[2], P[3]
    sF, _, aF = fresnel(wi[:, 2], ext, inte)
    sF = np.clip(sF, 0.1, 0.9)
    u = s.copy()
    refl = u[:, 0] < sF
    u[:, 0] = np.where(refl, u[:, 0] / sF, (u[:, 0] - sF) / (1 - sF))
    sa = alpha * (1.2 - 0.2 * np.sqrt(np.abs(wi[:, 2])))
    ph = 2 * np.pi * u[:, 1]
    if distr == 0:
        th = np.arctan(np.sqrt(-sa * sa * np.log(1 - u[:, 0])))
        dc = 4 + sa / np.sqrt(np.maximum(u[:, 0], 1e-300)) + sa / np.maximum(1 - u[:, 0], 1e-300)
    elif distr == 1:
        th = np.arccos(np.power(u[:, 0], 1 / (sa + 2)))
        c = np.power(u[:, 0], 1 / (sa + 2))
        dc = 4 + 1 / np.maximum(1 - c * c, 1e-300)
    else:
        th = np.arctan(sa * np.sqrt(u[:, 0]) / np.sqrt(1 - u[:, 0]))
        dc = 4 + 1 / np.maximum(1 - u[:, 0], 1e-300)
    m = np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)], axis=1)
    c = _dot(wi, m)
    wr = 2 * c[:, None] * m - wi
    swap = wi[:, 2] < 0
    eta = np.where(swap, inte, ext) / np.where(swap, ext, inte)
    k = 1 + eta * eta * (c * c - 1)
    wt = m * (eta * c - _signum(wi[:, 2]) * np.sqrt(np.maximum(k, 0)))[:, None] - wi * eta[:, None]
    r.wo = np.where(refl[:, None], wr, wt)
    r.stype = np.where(refl, GLOSSY_REFL, GLOSSY_TRANS)
    side = wi[:, 2] * r.wo[:, 2]
    ok = np.where(refl, side > 0, (k >= 0) & (side < 0))
    # the weight of sample(bRec, s): zero iff its numerator D G1 G1 <wi,m> F is (the denominator never is, here)
    g1i, _, ai = rg_smith_g1(distr, wi, m, alpha)
    g1o, _, ao = rg_smith_g1(distr, r.wo, m, alpha)
    D, _, aD = rg_eval_d(distr, m, alpha)
    Fm, _, aFm = fresnel(c, ext, inte)
    num = D * g1i * g1o * c * np.where(refl, Fm, 1 - Fm)
    r.alive = ok & (num != 0)
    r.dir_cond = (dc + np.where(refl, 0.0, 4 / np.maximum(np.abs(k), 1e-300))) / np.where(refl, sF, 1 - sF)
    reach = MARGIN + DIR_REACH * EPS32 * r.dir_cond
    r.amb = ((np.abs(s[:, 0] - sF) < MARGIN) | (np.abs(side) < reach) | (np.abs(k) < MARGIN) | aF | ai | ao | aD | aFm
             | (np.abs(_dot(r.wo, m)) < reach) | (1 - u[:, 0] < MARGIN))
    return r


_SAMPLERS = {LAMBERTIAN: _s_lambertian, DIELECTRIC: _s_dielectric, ROUGHMETAL: _s_roughmetal, MICROFACET: _s_microfacet,
             MIRROR: _s_mirror, PHONG: _s_phong, ROUGHGLASS: _s_roughglass, DIFFTRANS: _s_difftrans}


# ---------------------------------------------------------------------------------------------------------------------
# Delta luminaires: LuminaireSamplingRecord (lRec.d = direction of propagation, lRec.value) at a point p [n][3],
# src/luminaires/{point,spot,directional,collimated}.cpp.  One luminaire in the scene: lRec.pdf = 1 and the value is
# not rescaled (scene.cpp:396-415).  Returned (d [n][3], value [n][3]).
# ---------------------------------------------------------------------------------------------------------------------
def point_light(I, pos, p):
    """point.cpp:55-63: I / |p - pos|^2, d = (p - pos) / |p - pos|"""
    v = p - np.asarray(pos, dtype=np.float64)
    d2 = _dot(v, v)
    return v / np.sqrt(d2)[:, None], np.asarray(I, dtype=np.float64)[None, :] / d2[:, None]


def spot_falloff(I, w2l, cutoff, beam, d):
    """spot.cpp:87-108 (constant texture): zero at or beyond the cutoff cone, I inside the beam, and in between a ramp
    that is linear in the ANGLE, (cutoff - acos(cos theta)) / (cutoff - beam)"""
    cos = (np.asarray(w2l, dtype=np.float64).reshape(3, 3) @ d.T).T[:, 2]
    ramp = (cutoff - np.arccos(np.clip(cos, -1, 1))) / (cutoff - beam)
    k = np.where(cos <= np.cos(cutoff), 0.0, np.where(cos >= np.cos(beam), 1.0, ramp))
    return np.asarray(I, dtype=np.float64)[None, :] * k[:, None]


def spot_light(I, pos, w2l, cutoff, beam, p):
    """spot.cpp:115-124: falloffCurve(d) / |p - pos|^2"""
    v = p - np.asarray(pos, dtype=np.float64)
    d2 = _dot(v, v)
    d = v / np.sqrt(d2)[:, None]
    return d, spot_falloff(I, w2l, cutoff, beam, d) / d2[:, None]


def directional_light(I, direction, p):
    """directional.cpp:81-89: d = the light's direction, value = I, wherever p is"""
    d = np.broadcast_to(np.asarray(direction, dtype=np.float64), p.shape)
    return d, np.broadcast_to(np.asarray(I, dtype=np.float64)[None, :], p.shape)


def collimated_light(I, radius, w2l, l2w, p):
    """collimated.cpp:63-76: I along the beam axis where p lies in the half-space in front of the emitting disk and
    within `radius` of the axis, nothing elsewhere"""
    W = np.asarray(w2l, dtype=np.float64).reshape(3, 4)
    L = np.asarray(l2w, dtype=np.float64).reshape(3, 4)
    loc = p @ W[:, :3].T + W[:, 3]
    inside = (np.hypot(loc[:, 0], loc[:, 1]) <= radius) & (loc[:, 2] >= 0)
    d = np.broadcast_to(L[:, 2] / np.linalg.norm(L[:, 2]), p.shape)
    return d, np.where(inside[:, None], np.asarray(I, dtype=np.float64)[None, :], 0.0)


def direct_radiance(btype, P, frame, wi_world, d, value):
    """what path.cpp:100-125 adds at the first hit for a delta luminaire (miWeight(1, 0) = 1): value * f(wi, -d) |cos|,
    with wi / wo taken into the shading frame (s, t, n) [3][3] rows"""
    F = np.asarray(frame, dtype=np.float64)
    wi = wi_world @ F.T
    wo = (-d) @ F.T
    fv, _, _ = f(btype, P, wi, wo)
    return value * fv * np.abs(wo[:, 2])[:, None]
