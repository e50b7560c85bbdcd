"""A binary64 restatement of the sky luminaire (the Preetham / Perez daylight model): configure(), both ways to place the
sun, Le(direction), sample(p, s) and pdf, written from src/luminaires/sky.cpp, src/libcore/util.cpp:618-626
(toSphericalCoordinates) and src/libcore/spectrum.cpp:94-98 (fromXYZ, RGB) of the reference, not from csrc/.  Conventions of
tests/ref64.py: float32 inputs promoted to float64, every value with a conditioning factor `cond` and a flag `amb` where
binary32 may legitimately take the other branch.  Test infrastructure.

Parameter block (include/mtsgpu.h): [0] skyScale [1] turbidity [2] clipBelowHorizon [3..5] bsphere centre [6] radius
[7..15] world->luminaire 3x3 [16] thetaS [17] phiS [18..22] aConst..eConst.

How `cond` is obtained.  Every quantity is carried as a pair (value, err): err bounds, to first order and in units of
2^-23, the absolute error a binary32 evaluation in the reference's operation order makes.  The rules are the derivatives:
a rounded operation adds half a unit of its result; a sum adds its operands' errors; a product a * b adds |a| err(b) +
|b| err(a); exp multiplies the argument's error by the result; acos divides it by sqrt(1 - a^2); and so on.  cond = err /
|value| of the final value, so the chromaticity path's 1 - x - y and Y / y and the Perez term's exp(B / cos theta) near the
horizon raise it exactly where binary32 loses digits.  A branch is `amb` where its operand lies within REACH of its own
err of the threshold."""
import numpy as np

from ref64 import EPS32, _f64

REACH = 4.0                   # a comparison is undecidable within REACH x the operand's first-order error bound
PI32 = float(np.float32(np.pi))          # M_PI of the single-precision build (constants.h:45-46)
INV_4PI = 1.0 / (4.0 * PI32)

# SkyLuminaire::configure (sky.cpp:146-178): [A..E][constant term, turbidity term] of Y (L), x, y
_PEREZ_L = [(-1.46303, 0.17872), (0.42749, -0.35540), (5.32505, -0.02266), (-2.57705, 0.12064), (0.37027, -0.06696)]
_PEREZ_X = [(-0.25922, -0.01925), (0.00081, -0.06651), (0.21247, -0.00041), (-0.89887, -0.06409), (0.04517, -0.00325)]
_PEREZ_Y = [(-0.26078, -0.01669), (0.00921, -0.09495), (0.21023, -0.00792), (-1.65369, -0.04405), (0.05291, -0.01092)]


class E:
    """value with a first-order absolute error bound in units of 2^-23"""
    __array_ufunc__ = None                          # numpy scalars on the left defer to the reflected operators

    def __init__(self, v, e=None):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.zeros_like(self.v) if e is None else np.asarray(e, dtype=np.float64) + np.zeros_like(self.v)

    def _r(self, force=False):                      # one rounding to binary32 (none inside a binary64 expression, see _double)
        if force or not _EXACT[0]:
            self.e = self.e + 0.5 * np.abs(self.v)
        return self

    def store(self):
        """the store of a binary64 expression into a Float: its one rounding"""
        return E(self.v, self.e)._r(force=True)

    def __add__(self, o):
        o = _E(o); return E(self.v + o.v, self.e + o.e)._r()

    __radd__ = __add__

    def __sub__(self, o):
        o = _E(o); return E(self.v - o.v, self.e + o.e)._r()

    def __rsub__(self, o):
        return _E(o) - self

    def __neg__(self):
        return E(-self.v, self.e)

    def __mul__(self, o):
        o = _E(o); return E(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)._r()

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = _E(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            return E(self.v / o.v, self.e / np.abs(o.v) + np.abs(self.v) * o.e / (o.v * o.v))._r()

    def __rtruediv__(self, o):
        return _E(o) / self


_EXACT = [False]


class _double:
    """inside this block the operations are the reference's binary64 ones (a double literal promotes the expression): they
    carry their operands' errors on but add no binary32 rounding of their own; E.store() rounds once at the end"""

    def __enter__(self):
        self.was, _EXACT[0] = _EXACT[0], True

    def __exit__(self, *a):
        _EXACT[0] = self.was


def _E(x):
    return x if isinstance(x, E) else E(x)


def _exp(a):
    v = np.exp(a.v); return E(v, v * a.e)._r()


def _cos(a):
    return E(np.cos(a.v), np.abs(np.sin(a.v)) * a.e)._r()


def _sin(a):
    return E(np.sin(a.v), np.abs(np.cos(a.v)) * a.e)._r()


def _sqrt(a):
    v = np.sqrt(a.v)
    with np.errstate(divide="ignore", invalid="ignore"):
        return E(v, a.e / (2 * v))._r()


def _acos(a):
    c = np.clip(a.v, -1.0, 1.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return E(np.arccos(c), a.e / np.sqrt(1 - c * c))._r()


def _atan2(y, x):
    with np.errstate(divide="ignore", invalid="ignore"):
        return E(np.arctan2(y.v, x.v), (np.abs(x.v) * y.e + np.abs(y.v) * x.e) / (x.v * x.v + y.v * y.v))._r()


def _where(c, a, b):
    a, b = _E(a), _E(b)
    return E(np.where(c, a.v, b.v), np.where(c, a.e, b.e))


def _near(q, thr):
    """q is within reach of its own binary32 error of the threshold"""
    return np.abs(q.v - thr) <= REACH * EPS32 * q.e + 1e-300


# ---------------------------------------------------------------------------------------------------------------------
# the sun (sky.cpp:186-219)
# ---------------------------------------------------------------------------------------------------------------------
def sun_from_direction(sun_dir):
    """configureSunPosition(const Vector &) (sky.cpp:214-219) -> (thetaS, phiS): toSphericalCoordinates(normalize(sunDir))"""
    v = _f64(sun_dir)
    v = v / np.sqrt((v * v).sum())
    theta, phi = np.arccos(v[2]), np.arctan2(v[1], v[0])
    if phi < 0:
        phi += 2 * PI32                            # util.cpp:623-624
    return float(theta), float(phi)


def sun_from_location(lat, lon, std_mrd, jul_day, time_of_day):
    """configureSunPosition(lat, lon, int stdMrd, int julDay, timeOfDay) (sky.cpp:186-208): the two `int` parameters
    truncate what the constructor read as Floats (:92-93)"""
    lat, lon, time_of_day = (float(np.float32(x)) for x in (lat, lon, time_of_day))
    std_mrd, jul_day = int(np.float32(std_mrd)), int(np.float32(jul_day))
    solar_time = (time_of_day + (0.170 * np.sin(4.0 * PI32 * (jul_day - 80.0) / 373.0) - 0.129 * np.sin(2.0 * PI32 * (jul_day - 8.0) / 355.0))
                  + (std_mrd - lon) / 15.0)                                                           # :188-191
    decl = 0.4093 * np.sin(2 * PI32 * (jul_day - 81) / 368)                                           # :193
    rlat = lat * (PI32 / 180.0)
    hour = PI32 * solar_time / 12.0
    altitude = np.arcsin(np.sin(rlat) * np.sin(decl) - np.cos(rlat) * np.cos(decl) * np.cos(hour))    # :195-197
    opp = -np.cos(decl) * np.sin(hour)                                                                # :199
    adj = -(np.cos(rlat) * np.sin(decl) + np.sin(rlat) * np.cos(decl) * np.cos(hour))                 # :200-202
    return float(PI32 / 2.0 - altitude), float(-np.arctan2(opp, adj))                                 # :204-207


# ---------------------------------------------------------------------------------------------------------------------
# configure (sky.cpp:139-179) and the parameter-only part of getDistribution (:458-461)
# ---------------------------------------------------------------------------------------------------------------------
def _configure_E(P):
    """-> dict of E: zx, zy, zL, perez[3] (x, y, L: lists of five), den[3]; binary32 inputs are exact"""
    T, th = E(float(P[1])), E(float(P[16]))
    k = [E(float(P[18 + i])) for i in range(5)]
    th2 = th * th; th3 = th2 * th; T2 = T * T

    def poly(c3, c2, c1, c0):
        return c3 * th3 + c2 * th2 + c1 * th + c0

    # theta2, theta3 and turb2 are Floats (binary32 products, :140-143); the polynomials, chi's first factor, zenithL and the
    # Perez coefficients are binary64 expressions rounded once, at the store into the Float member (:146-178)
    with _double():
        zx = (poly(0.00165, -0.00374, 0.00208, 0.0) * T2 + poly(-0.02902, 0.06377, -0.03202, 0.00394) * T
              + poly(0.11693, -0.21196, 0.06052, 0.25885)).store()
        zy = (poly(0.00275, -0.00610, 0.00316, 0.0) * T2 + poly(-0.04214, 0.08970, -0.04153, 0.00515) * T
              + poly(0.15346, -0.26756, 0.06669, 0.26688)).store()
    span = PI32 - 2 * th                                                      # binary32: M_PI is a float literal
    with _double():
        chi = ((4.0 / 9.0 - T / 120.0) * span).store()
        tan_chi = E(np.tan(chi.v), chi.e / np.cos(chi.v) ** 2)._r(force=True)
        zL = ((4.0453 * T - 4.9710) * tan_chi - 0.2155 * T + 2.4192).store()
        perez = [[((c1 * T + c0) * k[i]).store() for i, (c0, c1) in enumerate(tab)] for tab in (_PEREZ_X, _PEREZ_Y, _PEREZ_L)]
    cos_s = _cos(th)
    den = [(1 + lam[0] * _exp(lam[1])) * (1 + lam[2] * _exp(lam[3] * th) + lam[4] * cos_s * cos_s) for lam in perez]
    return dict(zx=zx, zy=zy, zL=zL, perez=perez, den=den, th=th, phi=E(float(P[17])))


def configure(block):
    """SkyLuminaire::configure() -> (values [21], cond [21]) in the order of mtsgpu_sky_configure: zenith x, y, Y, the
    Perez coefficients of x, y, Y, their three denominators"""
    c = _configure_E(_f64(block))
    q = [c["zx"], c["zy"], c["zL"]] + c["perez"][0] + c["perez"][1] + c["perez"][2] + c["den"]
    val = np.array([float(x.v) for x in q])
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.array([float(x.e) / abs(float(x.v)) if x.v != 0 else np.inf for x in q])
    return val, np.maximum(cond, 1.0)


# ---------------------------------------------------------------------------------------------------------------------
# Le (sky.cpp:235-267, getSkySpectralRadiance :469-495, getAngleBetween :429-439, getDistribution :451-464)
# ---------------------------------------------------------------------------------------------------------------------
_XYZ2RGB = [(3.240479, -1.537150, -0.498535), (-0.969256, 1.875991, 0.041556), (0.055648, -0.204043, 1.057311)]


def le(block, dirs):
    """Le(direction) for world directions [n][3] (float32, any length) -> (value [n][3], cond [n], amb [n])"""
    with np.errstate(all="ignore"):              # an unbounded err (acos at +-1) times a zero derivative is a NaN the flags absorb
        return _le(block, dirs)


def _le(block, dirs):
    P = _f64(block)
    D = _f64(dirs).reshape(-1, 3)
    n = len(D)
    cfg = _configure_E(P)
    M = P[7:16].reshape(3, 3)
    # m_worldToLuminaire(direction), normalize (sky.cpp:237)
    v = [M[r, 0] * E(D[:, 0]) + M[r, 1] * E(D[:, 1]) + M[r, 2] * E(D[:, 2]) for r in range(3)]
    inv = 1.0 / _sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    d = [v[i] * inv for i in range(3)]
    clip = bool(P[2] != 0)
    amb = np.zeros(n, dtype=bool)
    below = d[2].v < 0.0
    if clip:                                                                                          # :239-243
        amb |= _near(d[2], 0.0)
    low = d[2].v < 0.001                                                                              # :246-247
    amb |= _near(d[2], 0.001)
    inv2 = 1.0 / _sqrt(d[0] * d[0] + d[1] * d[1] + E(np.float64(np.float32(0.001))) * E(np.float64(np.float32(0.001))))
    d = [_where(low, d[0] * inv2, d[0]), _where(low, d[1] * inv2, d[1]), _where(low, np.float64(np.float32(0.001)) * inv2, d[2])]
    theta = _acos(d[2])                                                                               # util.cpp:618-626
    phi = _atan2(d[1], d[0])
    phi = _where(phi.v < 0, phi + 2 * PI32, phi)
    half = PI32 * 0.5 - float(np.float32(0.001))
    # :471.  A direction clamped to d.z = 0.001 has theta = acos(0.001), within rounding of the threshold by construction: min()
    # is continuous there and theta's own err covers either reading, so only unclamped directions are flagged
    amb |= _near(theta, half) & ~low
    theta_fin = _where(theta.v < half, theta, E(half))
    # getAngleBetween(theta, phi, thetaS, phiS) (:429-439)
    th_s, ph_s = cfg["th"], cfg["phi"]
    cospsi = _sin(theta) * _sin(th_s) * _cos(ph_s - phi) + _cos(theta) * _cos(th_s)
    amb |= _near(cospsi, 1.0) | _near(cospsi, -1.0)
    gamma = _where(cospsi.v > 1.0, 0.0, _where(cospsi.v < -1.0, PI32, _acos(cospsi)))
    cos_gamma, cos_fin = _cos(gamma), _cos(theta_fin)

    def dist(lam, den):                                                                               # :451-464
        num = (1 + lam[0] * _exp(lam[1] / cos_fin)) * (1 + lam[2] * _exp(lam[3] * gamma) + lam[4] * cos_gamma * cos_gamma)
        return num / den

    x = cfg["zx"] * dist(cfg["perez"][0], cfg["den"][0])                                               # :477-479
    y = cfg["zy"] * dist(cfg["perez"][1], cfg["den"][1])
    Y = cfg["zL"] * dist(cfg["perez"][2], cfg["den"][2])
    y_frac = Y / y                                                                                    # :484-488
    X = y_frac * x
    zz = 1.0 - x - y
    amb |= _near(zz, 0.0)
    z = _where(zz.v > 0, zz, 0.0)
    Z = y_frac * z
    val = np.zeros((n, 3)); err = np.zeros((n, 3))
    for c, (a, b, g) in enumerate(_XYZ2RGB):                                                          # spectrum.cpp:94-98
        ch = float(np.float32(a)) * X + float(np.float32(b)) * Y + float(np.float32(g)) * Z
        amb |= _near(ch, 0.0) & (ch.v != 0)                                                           # clampNegative (:494)
        ch = _where(ch.v > 0, ch, 0.0) * float(P[0])                                                  # :264
        val[:, c], err[:, c] = ch.v, ch.e
    with np.errstate(divide="ignore", invalid="ignore"):
        cond = np.where(val != 0, err / np.abs(val), 0.0).max(axis=1)
    if clip:
        val = np.where(below[:, None], 0.0, val)
        cond = np.where(below, 1.0, cond)
    cond = np.where(np.isfinite(cond), np.maximum(cond, 1.0), np.inf)
    amb |= ~np.isfinite(cond)
    return val, cond, amb


# ---------------------------------------------------------------------------------------------------------------------
# sample and pdf (sky.cpp:277-292, :415-421)
# ---------------------------------------------------------------------------------------------------------------------
class SkySample:
    pass


def sample(block, p, s):
    """SkyLuminaire::sample(p, lRec, sample): d = squareToSphere(sample) (util.cpp:553-559), pdf = 1 / (4 pi), value =
    Le(-d), sRec.p = p - d * (2 radius).  -> d [n][3], dir_cond [n] (per component, absolute, in units of 2^-23), pdf, end
    point [n][3] with end_err [n][3].  The value is a function of the evaluator's own d and is checked through le()."""
    with np.errstate(all="ignore"):
        return _sample(block, p, s)


def _sample(block, p, s):
    P = _f64(block)
    p, s = _f64(p).reshape(-1, 3), _f64(s).reshape(-1, 2)
    z = 1.0 - 2.0 * E(s[:, 1])
    r2 = 1.0 - z * z
    r = _sqrt(_where(r2.v > 0, r2, 0.0))
    phi = (2.0 * PI32) * E(s[:, 0])
    d = [r * _cos(phi), r * _sin(phi), z]
    out = SkySample()
    out.d = np.stack([c.v for c in d], axis=1)
    derr = np.stack([c.e for c in d], axis=1).max(axis=1)
    # sample.y = 0: z = 1 - 0 = 1, r = sqrt(max(0, 1 - 1)) = 0 and d = (0, 0, 1) are exact in binary32 as well (the rules
    # above charge a rounding to every operation and cannot see that); any other z = +-1 has no first-order bound
    exact = s[:, 1] == 0
    derr = np.where(exact, 1.0, derr)
    out.dir_cond = np.where(np.isfinite(derr), np.maximum(derr, 1.0), np.inf)
    out.amb = ~np.isfinite(derr)
    out.pdf = INV_4PI
    k = 2.0 * float(P[6])
    end = [E(p[:, i]) - d[i] * k for i in range(3)]
    out.end = np.stack([c.v for c in end], axis=1)
    out.end_err = np.stack([c.e for c in end], axis=1)
    return out


def pdf():
    """SkyLuminaire::pdf (sky.cpp:288-292): 1.0f / (4 * M_PI) in binary32"""
    return np.float32(1.0) / (np.float32(4) * np.float32(np.pi))
