"""The woven-cloth BRDF of the reference, IrawanClothBRDF (src/bsdfs/irawan.cpp, irawan.h): a float32 mirror of f / pdf /
sample(bRec, pdf, s) in the reference's operation order and as compiled, with the `Random` (src/libcore/random.cpp) and the
Perlin noise (src/librender/noise.cpp) it draws from.  Written from the reference sources, not from csrc/.  Test infrastructure.

The second half of the file is a binary64 restatement of f with a first-order bound per value (f64, eval64), written from
the source in real-number form on numpy's own libm, which the mirror is held to.

The mirror is binary32 numpy.  Where the source mixes a Float with the double M_PI the sub-expression is binary64 and is rounded
where it is stored in a Float (v = xy.x * M_PI / w; fs * M_PI * l; 2 * M_PI * I0; al / (4.0f * M_PI) * c1 * c2 / (c1 + c2);
v_of_u * w / M_PI, which inside the staple's window test is never stored and stays binary64; M_PI / 2.0f).  The elementary
functions are the library's specifications, restated here in binary64 numpy: the operations of
csrc/devmath.h are plain IEEE binary64, evaluated in a fixed order and rounded once.
  std::sin, cos, tan      reduction by pi / 2 in two parts, Taylor polynomials; tan = sine / cosine of one reduction
  std::exp, log           reduction by ln 2 / by the exponent, polynomials
  std::atan, atan2, acos  argument reduction at tan(pi / 8) and 1, a degree-35 polynomial; acos = 2 atan(sqrt((1 - x) / (1 + x)))
  std::sinh, cosh         (exp(x) -+ exp(-x)) / 2, sinh's series below 2^-13
  std::pow(x, 2.0f)       x * x;   std::pow(x, 1.5f): x * sqrt(x) in binary64 with the correctly rounded sqrt

As compiled: tileWidth and tileHeight are uint32_t, so ((int) xy.x / tileWidth) * tileWidth is unsigned arithmetic; modulo is
the (int, int) overload; tileHeight * repeatV is a float product; (uint64_t) of a negative float is what the x86-64 build
computes, (uint64_t)(int64_t) x, and the seed arithmetic wraps modulo 2^64."""
import numpy as np

F = np.float32
U64 = np.uint64
PI64 = 3.14159265358979323846
INV_PI = F(0.31830988618379067154)
PI32 = F(3.14159265358979323846)
EPSILON = F(1e-4)
TWOSIDED = 0x100
GLOSSY_REFL = 0x10
MUTATIONS = ("rotation_sign", "center_v_plain", "signed_division", "next_float_count", "pbrt_grad", "length_for_width_in_gu",
             "no_area_factor", "circle_near_one", "weft_derivatives_swapped", "sample_divides_by_cos", "variation_clamp_one",
             "seed_without_center_y")

# Ken Perlin's reference permutation (noise.cpp:9-41 lists it twice)
PERM = np.array([
    151, 160, 137, 91, 90, 15, 131, 13, 201, 95, 96, 53, 194, 233, 7, 225, 140, 36, 103, 30, 69, 142, 8, 99, 37, 240, 21, 10, 23,
    190, 6, 148, 247, 120, 234, 75, 0, 26, 197, 62, 94, 252, 219, 203, 117, 35, 11, 32, 57, 177, 33, 88, 237, 149, 56, 87, 174,
    20, 125, 136, 171, 168, 68, 175, 74, 165, 71, 134, 139, 48, 27, 166, 77, 146, 158, 231, 83, 111, 229, 122, 60, 211, 133, 230,
    220, 105, 92, 41, 55, 46, 245, 40, 244, 102, 143, 54, 65, 25, 63, 161, 1, 216, 80, 73, 209, 76, 132, 187, 208, 89, 18, 169,
    200, 196, 135, 130, 116, 188, 159, 86, 164, 100, 109, 198, 173, 186, 3, 64, 52, 217, 226, 250, 124, 123, 5, 202, 38, 147, 118,
    126, 255, 82, 85, 212, 207, 206, 59, 227, 47, 16, 58, 17, 182, 189, 28, 42, 223, 183, 170, 213, 119, 248, 152, 2, 44, 154,
    163, 70, 221, 153, 101, 155, 167, 43, 172, 9, 129, 22, 39, 253, 19, 98, 108, 110, 79, 113, 224, 232, 178, 185, 112, 104, 218,
    246, 97, 228, 251, 34, 242, 193, 238, 210, 144, 12, 191, 179, 162, 241, 81, 51, 145, 235, 249, 14, 239, 107, 49, 192, 214, 31,
    181, 199, 106, 157, 184, 84, 204, 176, 115, 121, 50, 45, 127, 4, 150, 254, 138, 236, 205, 93, 222, 114, 67, 29, 24, 72, 243,
    141, 128, 195, 78, 66, 215, 61, 156, 180], dtype=np.int64)
PERM2 = np.concatenate([PERM, PERM])


def _f32(x):
    return np.asarray(x, dtype=np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the elementary functions, as specified
# ---------------------------------------------------------------------------------------------------------------------
def sincos_d(x):
    xd = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        kd = xd * 0.63661977236758134308
        k = np.trunc(np.nan_to_num(kd + np.where(kd >= 0, 0.5, -0.5)))
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
    return s, c


def sincos32(x):
    s, c = sincos_d(_f32(x))
    return s.astype(np.float32), c.astype(np.float32)


def sin32(x):
    return sincos32(x)[0]


def cos32(x):
    return sincos32(x)[1]


def tan32(x):
    s, c = sincos_d(_f32(x))
    with np.errstate(all="ignore"):
        return (s / c).astype(np.float32)


def exp_d(xd):
    xd = np.asarray(xd, dtype=np.float64)
    with np.errstate(all="ignore"):
        kd = xd * 1.44269504088896338700e+00
        k = np.trunc(np.nan_to_num(kd + np.where(kd >= 0, 0.5, -0.5)))
        k = np.clip(k, -1100, 1100)
        r = (xd - k * 6.93147180369123816490e-01) - k * 1.90821492927058770002e-10
        p = np.full_like(r, 1.0 / 6227020800.0)
        for c in (479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0):
            p = p * r + 1.0 / c
        p = p * r + 0.5
        p = p * r + 1.0
        p = p * r + 1.0
        out = p * np.ldexp(1.0, np.clip(k, -1022, 1023).astype(np.int64))
    out = np.where(xd > 700.0, np.inf, np.where(xd < -700.0, 0.0, out))
    return np.where(np.isnan(xd), xd, out)


def exp32(x):
    x = _f32(x)
    xd = x.astype(np.float64)
    with np.errstate(all="ignore"):
        out = exp_d(xd).astype(np.float32)
    out = np.where(xd > 89.0, F(np.inf), np.where(xd < -104.0, F(0), out))
    return np.where(np.isnan(x), x, out).astype(np.float32)


def log32(x):
    x = _f32(x)
    xd = x.astype(np.float64)
    with np.errstate(all="ignore"):
        safe = np.where((xd > 0) & np.isfinite(xd), xd, 1.0)
        m, e = np.frexp(safe)
        m, e = m * 2.0, e.astype(np.float64) - 1.0
        big = m > 1.41421356237309514547e+00
        m, e = np.where(big, m * 0.5, m), np.where(big, e + 1.0, e)
        s = (m - 1.0) / (m + 1.0)
        s2 = s * s
        p = np.full_like(s, 1.0 / 19.0)
        for c in (17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
            p = p * s2 + 1.0 / c
        p = p * s2 + 1.0
        out = (e * 6.93147180559945286227e-01 + 2.0 * s * p).astype(np.float32)
    out = np.where(x == 0, F(-np.inf), np.where(x == F(np.inf), F(np.inf), out))
    return np.where(np.isnan(x) | (x < 0), F(np.nan), out).astype(np.float32)


def atan_d(xin):
    xd = np.asarray(xin, dtype=np.float64)
    with np.errstate(all="ignore"):
        neg = xd < 0.0
        xd = np.where(neg, -xd, xd)
        inv = xd > 1.0
        xd = np.where(inv, 1.0 / xd, xd)
        red = xd > 0.41421356237309503
        y = np.where(red, (xd - 1.0) / (xd + 1.0), xd)
        base = np.where(red, 7.85398163397448278999e-01, 0.0)
        y2 = y * y
        p = np.full_like(y, 1.0 / 35.0)
        for c in range(33, 1, -2):
            p = -p * y2 + 1.0 / c
        p = -p * y2 + 1.0
        a = base + y * p
        a = np.where(inv, 1.57079632679489655800e+00 - a, a)
        a = np.where(neg, -a, a)
    return a


def atan32(x):
    x = _f32(x)
    return np.where(np.isnan(x), x, atan_d(x.astype(np.float64)).astype(np.float32)).astype(np.float32)


def acos32(x):
    x = _f32(x)
    xd = x.astype(np.float64)
    with np.errstate(all="ignore"):
        out = (2.0 * atan_d(np.sqrt((1.0 - xd) / (1.0 + xd)))).astype(np.float32)
    out = np.where(x == F(-1), F(3.14159265358979311600e+00), out)
    return np.where(np.isnan(x) | (x > 1) | (x < -1), F(np.nan), out).astype(np.float32)


def atan2_32(y, x):
    y, x = _f32(y), _f32(x)
    PI, PIO2 = 3.14159265358979311600e+00, 1.57079632679489655800e+00
    yd, xd = y.astype(np.float64), x.astype(np.float64)
    ysign, xsign = np.signbit(y), np.signbit(x)
    with np.errstate(all="ignore"):
        r = atan_d(yd / np.where(xd == 0, 1.0, xd))
        r = np.where(xd < 0, r + np.where(ysign, -PI, PI), r)
        zero = np.where(xsign, PI, 0.0)
        zero = np.where(ysign, -zero, zero)
        atx0 = np.where(yd == 0, zero, np.where(yd > 0, PIO2, -PIO2))
        r = np.where(xd == 0, atx0, r)
    return np.where(np.isnan(x) | np.isnan(y), F(np.nan), r.astype(np.float32)).astype(np.float32)


def sinh32(x):
    x = _f32(x)
    xd = x.astype(np.float64)
    with np.errstate(all="ignore"):
        small = (xd < 0.0001220703125) & (xd > -0.0001220703125)
        out = np.where(small, xd + ((xd * xd) * xd) * (1.0 / 6.0), (exp_d(xd) - exp_d(-xd)) * 0.5).astype(np.float32)
    return np.where(np.isnan(x), x, out).astype(np.float32)


def cosh32(x):
    x = _f32(x)
    xd = x.astype(np.float64)
    with np.errstate(all="ignore"):
        out = ((exp_d(xd) + exp_d(-xd)) * 0.5).astype(np.float32)
    return np.where(np.isnan(x), x, out).astype(np.float32)


def pow15_32(x):
    b = _f32(x).astype(np.float64)
    with np.errstate(all="ignore"):
        return (b * np.sqrt(b)).astype(np.float32)


def hemisphere_psa32(s):
    """squareToHemispherePSA (util.cpp:572-588) in binary32"""
    s = _f32(s).reshape(-1, 2)
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
# Random (random.cpp:99-103, 141-174, 218-227)
# ---------------------------------------------------------------------------------------------------------------------
def random_plain(seed, count):
    """`count` nextULong() of Random(seed): the whole 312-word generator, plainly, in Python integers"""
    M = (1 << 64) - 1
    mt = [seed & M]
    for i in range(1, 312):
        mt.append((6364136223846793005 * (mt[i - 1] ^ (mt[i - 1] >> 62)) + i) & M)
    UM, LM, A = 0xFFFFFFFF80000000, 0x7FFFFFFF, 0xB5026F5AA96619E9
    for i in range(312):
        x = (mt[i] & UM) | (mt[(i + 1) % 312] & LM)
        mt[i] = mt[(i + 156) % 312] ^ (x >> 1) ^ (A if x & 1 else 0)
    out = []
    for i in range(count):
        x = mt[i]
        x ^= (x >> 29) & 0x5555555555555555
        x ^= (x << 17) & 0x71D67FFFEDA60000 & M
        x ^= (x << 37) & 0xFFF7EEE000000000 & M
        x ^= x >> 43
        out.append(x)
    return out


def ulong_to_float(v):
    """Random::nextFloat of one nextULong(), single precision branch"""
    u = ((np.asarray(v, dtype=np.uint64) & U64(0xFFFFFFFF)) >> U64(9)).astype(np.uint32) | np.uint32(0x3f800000)
    return u.view(np.float32) - F(1)


def random_first_three(seed):
    """the first three nextULong() of Random(seed) for an array of seeds, from seven words of the seeding recurrence -> [3][n]"""
    seed = np.asarray(seed, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = seed.copy()
        keep = {0: x.copy()}
        for i in range(1, 159):
            x = U64(6364136223846793005) * (x ^ (x >> U64(62))) + U64(i)
            if i in (1, 2, 3, 156, 157, 158):
                keep[i] = x.copy()
    out = []
    for k in range(3):
        a, b, m = keep[k], keep[k + 1], keep[156 + k]
        y = (a & U64(0xFFFFFFFF80000000)) | (b & U64(0x7FFFFFFF))
        y = m ^ (y >> U64(1)) ^ np.where((y & U64(1)) != 0, U64(0xB5026F5AA96619E9), U64(0))
        y = y ^ ((y >> U64(29)) & U64(0x5555555555555555))
        y = y ^ ((y << U64(17)) & U64(0x71D67FFFEDA60000))
        y = y ^ ((y << U64(37)) & U64(0xFFF7EEE000000000))
        y = y ^ (y >> U64(43))
        out.append(y)
    return np.stack(out)


# ---------------------------------------------------------------------------------------------------------------------
# Noise::perlinNoise (noise.cpp:43-101), the full three-dimensional form
# ---------------------------------------------------------------------------------------------------------------------
def _grad(x, y, z, dx, dy, dz, pbrt=False):
    h = PERM2[PERM2[PERM2[x] + y] + z] & 15
    if pbrt:
        u = np.where((h < 8) | (h == 12) | (h == 13), dx, dy)
        v = np.where((h < 4) | (h == 12) | (h == 13), dy, dz)
    else:
        u = np.where(h < 8, dx, dy)
        v = np.where(h < 4, dy, np.where((h == 12) | (h == 14), dx, dz))
    return (np.where((h & 1) != 0, -u, u) + np.where((h & 2) != 0, -v, v)).astype(np.float32)


def _noise_weight(t):
    t3 = t * t * t
    t4 = t3 * t
    t5 = t4 * t
    return F(6) * t5 - F(15) * t4 + F(10) * t3


def _lerp(t, v1, v2):
    return (F(1) - t) * v1 + t * v2


def perlin32(px, py=None, pz=None, pbrt=False):
    px = _f32(px)
    py = np.zeros_like(px) if py is None else _f32(py)
    pz = np.zeros_like(px) if pz is None else _f32(pz)
    with np.errstate(all="ignore"):
        fx, fy, fz = np.floor(px), np.floor(py), np.floor(pz)
        ix, iy, iz = (np.nan_to_num(f).astype(np.int64) for f in (fx, fy, fz))
        dx, dy, dz = px - ix.astype(np.float32), py - iy.astype(np.float32), pz - iz.astype(np.float32)
        ix, iy, iz = ix & 255, iy & 255, iz & 255
        one = F(1)
        g = lambda a, b, c, x, y, z: _grad(a, b, c, x, y, z, pbrt)
        w000 = g(ix, iy, iz, dx, dy, dz)
        w100 = g(ix + 1, iy, iz, dx - one, dy, dz)
        w010 = g(ix, iy + 1, iz, dx, dy - one, dz)
        w110 = g(ix + 1, iy + 1, iz, dx - one, dy - one, dz)
        w001 = g(ix, iy, iz + 1, dx, dy, dz - one)
        w101 = g(ix + 1, iy, iz + 1, dx - one, dy, dz - one)
        w011 = g(ix, iy + 1, iz + 1, dx, dy - one, dz - one)
        w111 = g(ix + 1, iy + 1, iz + 1, dx - one, dy - one, dz - one)
        wx, wy, wz = _noise_weight(dx), _noise_weight(dy), _noise_weight(dz)
        x00, x10, x01, x11 = _lerp(wx, w000, w100), _lerp(wx, w010, w110), _lerp(wx, w001, w101), _lerp(wx, w011, w111)
        y0, y1 = _lerp(wy, x00, x10), _lerp(wy, x01, x11)
        return _lerp(wz, y0, y1).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# the BRDF
# ---------------------------------------------------------------------------------------------------------------------
def _smax(a, b):
    return np.where(a < b, b, a)


def _smin(a, b):
    return np.where(b < a, b, a)


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _length(a):
    return np.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def _normalize(a):
    r = F(1) / _length(a)
    return (a[0] * r, a[1] * r, a[2] * r)


def _to_u64(x):
    """(uint64_t) of a Float as the x86-64 build computes it"""
    with np.errstate(all="ignore"):
        return np.nan_to_num(_f32(x)).astype(np.int64).view(np.uint64)


def _atanh(arg):
    return log32((F(1) + arg) / (F(1) - arg)) / F(2)


def _radius_of_curvature(u, umax, kappa, w, l, mutation):
    rhat = F(1) + kappa * (F(1) + F(1) / tan32(umax))
    a = F(0.5) * w
    su = sin32(umax)
    circle = (F(0.5) * l - a * su) / su
    # ellipse
    tmax = atan32(rhat * tan32(umax))
    bhat = (F(0.5) * l - a * su) / sin32(tmax)
    ahat = bhat / rhat
    t = atan32(rhat * tan32(u))
    st, ct = sincos32(t)
    ellipse = pow15_32(bhat * bhat * ct * ct + ahat * ahat * st * st) / (ahat * bhat)
    # hyperbola
    tmax = -_atanh(rhat * tan32(umax))
    bhat = (F(0.5) * l - a * su) / sinh32(tmax)
    ahat = bhat / rhat
    t = -_atanh(rhat * tan32(u))
    ch, sh = cosh32(t), sinh32(t)
    hyperbola = -pow15_32(bhat * bhat * ch * ch + ahat * ahat * sh * sh) / (ahat * bhat)
    # parabola
    tmax = tan32(umax)
    ahat = (F(0.5) * l - a * su) / (F(2) * tmax)
    t = tan32(u)
    parabola = F(2) * ahat * pow15_32(F(1) + t * t)
    is_circle = rhat == F(1)
    if mutation == "circle_near_one":
        is_circle = np.abs(rhat - F(1)) < F(1e-2)
    R = np.where(is_circle, circle, np.where(rhat > 0, ellipse, np.where(rhat < 0, hyperbola, parabola)))
    return R.astype(np.float32), rhat


def _von_mises(cos_x, b):
    absB = np.abs(b)
    t = absB / F(3.75)
    t = t * t
    small = F(1) + t * (F(3.5156229) + t * (F(3.0899424) + t * (F(1.2067492) + t * (F(0.2659732) + t * (F(0.0360768) + t * F(0.0045813))))))
    t = F(3.75) / absB
    large = exp32(absB) / np.sqrt(absB) * (F(0.39894228) + t * (F(0.01328592) + t * (F(0.00225319) + t * (F(-0.00157565) + t * (F(0.00916281)
            + t * (F(-0.02057706) + t * (F(0.02635537) + t * (F(-0.01647633) + t * F(0.00392377)))))))))
    I0 = np.where(absB <= F(3.75), small, large).astype(np.float32)
    return (exp32(b * cos_x).astype(np.float64) / (2 * PI64 * I0.astype(np.float64))).astype(np.float32)


def _seeliger(cos1, cos2):
    al = F(1) / (F(0) + F(1))
    c1, c2 = _smax(F(0), cos1), _smax(F(0), cos2)
    val = (np.float64(al) / (4.0 * PI64) * c1.astype(np.float64) * c2.astype(np.float64) / (c1 + c2).astype(np.float64)).astype(np.float32)
    return np.where((c1 == 0) | (c2 == 0), F(0), val).astype(np.float32)


def _smooth_step01(value):
    v = (value - F(0)) / (F(1) - F(0))
    v = np.where(v < 0, F(0), np.where(v > 1, F(1), v))
    return v * v * (F(-2) * v + F(3))


# set to a dict, the two integrands leave the margins of their threshold tests in it (negative = the test holds): what
# tests/cloth_cases.threshold_records bisects on
PROBE = None


def _filament(W, u, v, om_i, om_r, umax, kappa, w, l, mutation):
    alpha, beta, ss = F(W.alpha), F(W.beta), F(W.ss)
    if ss < 0 or ss >= 1:
        return np.zeros_like(u)
    dead = (w * sin32(umax) >= l) | (kappa < F(-1))
    h = _normalize((om_r[0] + om_i[0], om_r[1] + om_i[1], om_r[2] + om_i[2]))
    u_of_v = atan32(h[1] / h[2])
    inside = np.abs(u_of_v) < umax
    sv, cv = sincos32(v)
    su, cu = sincos32(u_of_v)
    n = _normalize((sv, su * cv, cu * cv))
    t = _normalize((np.zeros_like(cu), cu, -su))
    lim = (F(1) - ss) * umax
    R, _ = _radius_of_curvature(_smin(np.abs(u_of_v), lim), lim, kappa, w, l, mutation)
    a = F(0.5) * (l if mutation == "length_for_width_in_gu" else w)
    s = (om_i[0] + om_r[0], om_i[1] + om_r[1], om_i[2] + om_r[2])
    tch_x = (t[1] * h[2]) - (t[2] * h[1])
    Gu = a * (R + a * cv) / (_length(s) * np.abs(tch_x))
    fc = alpha + _von_mises(-_dot(om_i, om_r), beta)
    A = _seeliger(_dot(n, om_i), _dot(n, om_r))
    if ss == 0:
        As = A
    else:
        As = A * (F(1) - _smooth_step01((np.abs(u_of_v) - (F(1) - ss) * umax) / (ss * umax)))
    fs = Gu * fc * As
    fs = (fs.astype(np.float64) * PI64 * l.astype(np.float64)).astype(np.float32)
    delta_y = l * F(W.hWidth)
    y_of_v = u_of_v * F(0.5) * l / umax
    hi, lo = F(0.5) * (l - delta_y), F(0.5) * (delta_y - l)
    y_of_v = np.where(y_of_v > hi, hi, np.where(y_of_v < lo, lo, y_of_v))
    window = np.abs(y_of_v - u * F(0.5) * l / umax) < F(0.5) * delta_y
    if PROBE is not None:
        PROBE["u_of_v = umax"] = np.abs(u_of_v).astype(np.float64) - umax
        PROBE["y window"] = np.abs(y_of_v - u * F(0.5) * l / umax).astype(np.float64) - F(0.5) * delta_y
    return np.where(~dead & inside & window, fs / delta_y, F(0)).astype(np.float32)


def _staple(W, u, v, om_i, om_r, psi, umax, kappa, w, l, mutation):
    alpha, beta = F(W.alpha), F(W.beta)
    dead = (w * sin32(umax) >= l) | (kappa < F(-1))
    h = _normalize((om_i[0] + om_r[0], om_i[1] + om_r[1], om_i[2] + om_r[2]))
    su, cu = sincos32(u)
    q = h[1] * su + h[2] * cu
    D = (h[1] * cu - h[2] * su) / (np.sqrt(h[0] * h[0] + q * q) * tan32(psi))
    v_of_u = atan2_32(-h[1] * su - h[2] * cu, h[0]) + acos32(D)
    inside = (np.abs(D) < F(1)) & (np.abs(v_of_u).astype(np.float64) < PI64 / 2.0)
    sv, cv = sincos32(v_of_u)
    n = _normalize((sv, su * cv, cu * cv))
    R, _ = _radius_of_curvature(np.abs(u), umax, kappa, w, l, mutation)
    a = F(0.5) * w
    s = (om_i[0] + om_r[0], om_i[1] + om_r[1], om_i[2] + om_r[2])
    Gv = a * (R + a * cv) / (_length(s) * _dot(n, h) * np.abs(sin32(psi)))
    fc = alpha + _von_mises(-_dot(om_i, om_r), beta)
    A = _seeliger(_dot(n, om_i), _dot(n, om_r))
    fs = Gv * fc * A
    fs = fs * F(2) * w * umax
    delta_x = w * F(W.hWidth)
    x_of_u = ((v_of_u * w).astype(np.float64) / PI64).astype(np.float32)
    hi, lo = F(0.5) * (w - delta_x), F(0.5) * (delta_x - w)
    x_of_u = np.where(x_of_u > hi, hi, np.where(x_of_u < lo, lo, x_of_u))
    window = np.abs(x_of_u.astype(np.float64) - (v * w).astype(np.float64) / PI64) < (F(0.5) * delta_x).astype(np.float64)
    if PROBE is not None:
        PROBE["D = 1"] = np.abs(D).astype(np.float64) - 1.0
        PROBE["v_of_u = pi / 2"] = np.abs(v_of_u).astype(np.float64) - PI64 / 2.0
        PROBE["x window"] = np.abs(x_of_u.astype(np.float64) - (v * w).astype(np.float64) / PI64) - (F(0.5) * delta_x).astype(np.float64)
    return np.where(~dead & inside & window, fs / delta_x, F(0)).astype(np.float32)


def f32(W, wi, wo, uv, mutation=None):
    """IrawanClothBRDF::f (irawan.cpp:105-223) for n records -> (value [n][3], info [n][8]); info: yarn id, centre x, y, random1,
    random2, intensityVariation, u, v -- zeros where f returns at once"""
    wi, wo, uv = _f32(wi).reshape(-1, 3), _f32(wo).reshape(-1, 3), _f32(uv).reshape(-1, 2)
    n = wi.shape[0]
    with np.errstate(all="ignore"):
        live = ~((wi[:, 2] <= 0) | (wo[:, 2] <= 0))
        tw, th = int(W.tileWidth), int(W.tileHeight)
        twf, thf = F(tw), F(th)
        rU, rV = F(W.repeatU), F(W.repeatV)
        uvx, uvy = uv[:, 0] * rU, (F(1) - uv[:, 1]) * rV
        xyx, xyy = uvx * twf, uvy * thf
        ix, iy = np.trunc(np.nan_to_num(xyx)).astype(np.int64), np.trunc(np.nan_to_num(xyy)).astype(np.int64)

        def modulo(a, b):
            q = (np.abs(a) // b) * np.sign(a)
            r = a - q * b
            return np.where(r < 0, r + b, r)

        lx, ly = modulo(ix, tw), modulo(iy, th)
        pattern = np.asarray(W.pattern, dtype=np.int64)
        yid = pattern[lx + ly * tw] - 1
        Y = W.yarns
        col = lambda name: np.float32([getattr(y, name) for y in Y])[yid]
        ytype = np.asarray([int(y.type) for y in Y])[yid]
        kd = np.float32([y.kd for y in Y])[yid]
        ks = np.float32([y.ks for y in Y])[yid]
        centerU, centerV = col("centerU"), col("centerV")
        if mutation == "signed_division":
            qx, qy = (np.abs(ix) // tw) * np.sign(ix) * tw, (np.abs(iy) // th) * np.sign(iy) * th
        else:
            qx = (((ix & 0xFFFFFFFF) // tw) * tw) & 0xFFFFFFFF
            qy = (((iy & 0xFFFFFFFF) // th) * th) & 0xFFFFFFFF
        cx = qx.astype(np.float32) + centerU * twf
        cy = qy.astype(np.float32) + ((centerV if mutation == "center_v_plain" else (F(1) - centerV)) * thf)
        xyx = xyx - cx
        xyy = -(xyy - cy)
        w, l, psi, kappa, umax = col("width"), col("length"), col("psi"), col("kappa"), col("umax")
        warp = ytype == 0
        dWarp = np.where(warp, F(W.dWarpUmaxOverDWarp), F(W.dWeftUmaxOverDWarp)).astype(np.float32)
        dWeft = np.where(warp, F(W.dWarpUmaxOverDWeft), F(W.dWeftUmaxOverDWeft)).astype(np.float32)
        if mutation == "weft_derivatives_swapped":
            dWarp, dWeft = dWeft, dWarp
        sgn = F(-1) if mutation == "rotation_sign" else F(1)
        # the weft's rotation by pi / 2 about z
        rx, ry = np.where(warp, xyx, sgn * -xyy), np.where(warp, xyy, sgn * xyx)
        xyx, xyy = rx, ry
        om_i = (np.where(warp, wi[:, 0], sgn * -wi[:, 1]), np.where(warp, wi[:, 1], sgn * wi[:, 0]), wi[:, 2])
        om_r = (np.where(warp, wo[:, 0], sgn * -wo[:, 1]), np.where(warp, wo[:, 1], sgn * wo[:, 0]), wo[:, 2])
        random1, random2 = np.ones(n, dtype=np.float32), np.ones(n, dtype=np.float32)
        if W.period > 0:
            with np.errstate(over="ignore"):
                seed = _to_u64(cx) * _to_u64(thf * rV)
                if mutation != "seed_without_center_y":
                    seed = seed + _to_u64(cy)
            draws = random_first_three(seed)
            first = 0 if mutation == "next_float_count" else 1
            n1, n2 = ulong_to_float(draws[first]), ulong_to_float(draws[first + 1])
            pbrt = mutation == "pbrt_grad"
            random1 = perlin32((cx * (thf * rV + n1) + cy) / F(W.period), pbrt=pbrt)
            random2 = perlin32((cy * (twf * rU + n2) + cx) / F(W.period), pbrt=pbrt)
            umax = umax + random1 * dWarp + random2 * dWeft
        u = xyy / (l / F(2)) * umax
        v = (xyx.astype(np.float64) * PI64 / w.astype(np.float64)).astype(np.float32)
        variation = np.ones(n, dtype=np.float32)
        result = np.zeros((n, 3), dtype=np.float32)
        if W.ksMultiplier > 0:
            integrand = np.where(psi != 0, _staple(W, u, v, om_i, om_r, psi, umax, kappa, w, l, mutation),
                                 _filament(W, u, v, om_i, om_r, umax, kappa, w, l, mutation)).astype(np.float32)
            if W.fineness > 0:
                fin = F(W.fineness)
                with np.errstate(over="ignore"):
                    seed = _to_u64((cx + xyx) * fin) * _to_u64(thf * rV * fin) + _to_u64((cy + xyy) * fin)
                xi = ulong_to_float(random_first_three(seed)[0])
                variation = _smin(-log32(xi), F(1.0 if mutation == "variation_clamp_one" else 10.0)).astype(np.float32)
            s = variation * F(W.ksMultiplier) * integrand
            result = ks * s[:, None]
            wa, fa = F(W.warpArea), F(W.weftArea)
            area = np.where(warp, (wa + fa) / wa, (wa + fa) / fa).astype(np.float32)
            if mutation != "no_area_factor":
                result = result * area[:, None]
        value = (result + kd * F(W.kdMultiplier)).astype(np.float32)
        info = np.stack([yid.astype(np.float32), cx, cy, random1, random2, variation, u, v], axis=1).astype(np.float32)
    value = np.where(live[:, None], value, F(0)).astype(np.float32)
    info = np.where(live[:, None], info, F(0)).astype(np.float32)
    return value, info


def eval32(W, twosided, op, wi, aux, uv, mutation=None):
    """the hook's [n][8] for ops 0 (f), 1 (pdf), 2 (sample(bRec, pdf, s)), 3 (the internals), behind the twosided adapter or not"""
    wi, aux, uv = _f32(wi).reshape(-1, 3).copy(), _f32(aux).reshape(len(np.atleast_2d(aux)), -1), _f32(uv).reshape(-1, 2)
    n = wi.shape[0]
    out = np.zeros((n, 8), dtype=np.float32)
    flip = (wi[:, 2] < 0) if twosided else np.zeros(n, dtype=bool)
    wi[:, 2] = np.where(flip, wi[:, 2] * F(-1), wi[:, 2])
    if op in (0, 1, 3):
        wo = aux[:, :3].copy()
        wo[:, 2] = np.where(flip, wo[:, 2] * F(-1), wo[:, 2])
        if op == 1:
            dead = (wi[:, 2] <= 0) | (wo[:, 2] <= 0)
            out[:, 0] = np.where(dead, F(0), wo[:, 2] * INV_PI)
            return out
        value, info = f32(W, wi, wo, uv, mutation)
        if op == 0:
            out[:, :3] = value
        else:
            out[:] = info
        return out
    wo = hemisphere_psa32(aux[:, :2])
    value, _ = f32(W, wi, wo, uv, mutation)
    if mutation == "sample_divides_by_cos":
        with np.errstate(all="ignore"):
            value = value / wo[:, 2:3]
    dead = wi[:, 2] <= 0
    pdf = wo[:, 2] * INV_PI
    nonzero = value.any(axis=1) & (pdf != 0)
    wo[:, 2] = np.where(flip & nonzero, wo[:, 2] * F(-1), wo[:, 2])
    out[:, 0:3], out[:, 3], out[:, 4:7] = wo, pdf, value
    out[:, 7] = np.uint32(GLOSSY_REFL).view(np.float32)
    out[dead] = 0
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the binary64 restatement with a first-order bound per value
# ---------------------------------------------------------------------------------------------------------------------
# Restated from irawan.cpp in real-number form with numpy's libm (not the library's polynomials), on `E` of tests/ref64_snow.py: a
# binary64 value next to a bound on |the binary32 evaluation of the same expression - value|.  Every binary32 operation of the
# source adds one rounding to what its operands propagate; the sub-expressions the double M_PI makes binary64 propagate only
# and round where they are stored in a Float; an elementary function propagates its argument's bound through its derivative
# (taken at the end of the interval where it is largest) and adds 2^-45 relative for the library's polynomial and one rounding.
# The Perlin noise is restated in the one-dimensional form it has at (x, 0, 0): (1 - w(dx)) c(ix) dx + w(dx) c(ix + 1) (dx - 1)
# with c the gradient's coefficient of dx, which the three-dimensional form of the mirror must reduce to.
#
# Discrete decisions are taken on the binary64 values.  A decision is *ambiguous* when the quantity lies within its bound of the
# threshold, so that a binary32 evaluation may decide the other way: the two (int) casts (hence the yarn id and the centre),
# |u_of_v| < umax, |D| < 1, |v_of_u| < pi / 2, the two highlight windows and their clamps, c1 == 0 || c2 == 0, the branch of rhat
# and the early returns, min(-log xi, 10), the side of atan2's cut in the staple's v_of_u, floorToInt of the noise arguments and the integer parts of the seed factors (where one
# differs the draw is another number altogether).  A record with an ambiguous decision, or whose bound is not finite or exceeds
# FRAGILE_RELATIVE of max(|value|, kd), is *fragile*: it is left out of the binary64 comparison, never out of the mirror's
# comparison with the device, and the tests cap its share.
from ref64_snow import E, where as _where      # noqa: E402

FRAGILE_RELATIVE = 1e-2
LIB = 2.0 ** -45


class _Ctx:
    """collects the ambiguity of a record's decisions"""

    def __init__(self, n):
        self.amb = np.zeros(n, dtype=bool)
        self.rhat = np.zeros(n, dtype=bool)      # ambiguous in the branch of rhat alone (kept apart: see f64)

    def lt(self, a, b, active=None):
        """a < b on the values; ambiguous where |a - b| <= the bounds"""
        a, b = E.lift(a), E.lift(b)
        with np.errstate(all="ignore"):
            near = ~(np.abs(a.v - b.v) > a.e + b.e) & ~((a.e + b.e == 0) & np.isfinite(a.v - b.v))      # exact operands decide alike
        self.amb |= near if active is None else (near & active)
        return a.v < b.v

    def integer(self, a, active=None, floor=False):
        """(int) a or floorToInt(a); ambiguous where an integer lies within the bound"""
        with np.errstate(all="ignore"):
            v = np.nan_to_num(a.v)
            near = ~(np.abs(v - np.round(v)) > a.e) & ~((a.e == 0) & np.isfinite(a.v))
        self.amb |= near if active is None else (near & active)
        return (np.floor(v) if floor else np.trunc(v)).astype(np.int64)


def _exact(r, *ins):
    """an operation whose operands are exact and whose result is a binary32 number adds no rounding"""
    ok = np.ones(r.v.shape, dtype=bool)
    for i in ins:
        ok = ok & (np.broadcast_to(E.lift(i).e, r.v.shape) == 0)
    with np.errstate(all="ignore"):
        ok = ok & (r.v.astype(np.float32).astype(np.float64) == r.v)
    return E(r.v, np.where(ok, 0.0, r.e))


def _add(a, b): return _exact(E.lift(a) + b, a, b)
def _sub(a, b): return _exact(E.lift(a) - b, a, b)
def _mul(a, b): return _exact(E.lift(a) * b, a, b)


def _fn(v, e):
    with np.errstate(all="ignore"):
        return E(v, np.nan_to_num(e + np.abs(v) * LIB, nan=np.inf)).rounded()


def _sin(a): return _fn(np.sin(a.v), a.e)
def _cos(a): return _fn(np.cos(a.v), a.e)


def _tan(a):
    with np.errstate(all="ignore"):
        t = np.tan(a.v)
        hi = np.maximum(np.abs(np.tan(a.v - a.e)), np.abs(np.tan(a.v + a.e)))
        return _fn(t, a.e * (1 + hi * hi))


def _atan(a): return _fn(np.arctan(a.v), a.e)


def _atan2(y, x):
    with np.errstate(all="ignore"):
        den = np.maximum(np.abs(x.v) - x.e, 0) ** 2 + np.maximum(np.abs(y.v) - y.e, 0) ** 2
        e = np.where(den > 0, (np.abs(x.v) * y.e + np.abs(y.v) * x.e) / np.where(den > 0, den, 1.0), np.inf)
        e = np.where((x.e == 0) & (y.e == 0), 0.0, e)
        return _fn(np.arctan2(y.v, x.v), e)


def _acos(a):
    with np.errstate(all="ignore"):
        s = 1.0 - (np.abs(a.v) + a.e) ** 2
        e = np.where(s > 0, a.e / np.sqrt(np.where(s > 0, s, 1.0)), np.inf)
        e = np.where(a.e == 0, 0.0, e)
        return _fn(np.arccos(a.v), e)


def _log(a):
    with np.errstate(all="ignore"):
        lo = a.v - a.e
        e = np.where(lo > 0, a.e / np.where(lo > 0, lo, 1.0), np.inf)
        e = np.where(a.e == 0, 0.0, e)
        return _fn(np.log(a.v), e)


def _exp(a):
    with np.errstate(all="ignore"):
        v = np.exp(a.v)
        return _fn(v, v * np.expm1(a.e))


def _sinh(a):
    with np.errstate(all="ignore"):
        return _fn(np.sinh(a.v), a.e * np.cosh(np.abs(a.v) + a.e))


def _cosh(a):
    with np.errstate(all="ignore"):
        return _fn(np.cosh(a.v), a.e * np.sinh(np.abs(a.v) + a.e))


def _pow15(a):
    with np.errstate(all="ignore"):
        return _fn(np.power(a.v, 1.5), 1.5 * np.sqrt(np.maximum(a.v, 0) + a.e) * a.e)


def _dot64(a, b): return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
def _len64(a): return (a[0] * a[0] + a[1] * a[1] + a[2] * a[2]).sqrt()


def _norm64(a):
    r = 1 / _len64(a)
    return (a[0] * r, a[1] * r, a[2] * r)


def _perlin64(cx, p, active):
    ix = cx.integer(p, active, floor=True)
    dx = p - E(ix.astype(np.float64))

    def coeff(i):
        h = PERM[PERM[PERM[i & 255]]] & 15           # y = z = 0: NoisePerm[NoisePerm[NoisePerm[x] + 0] + 0]
        u = np.where(h < 8, np.where((h & 1) != 0, -1.0, 1.0), 0.0)
        v = np.where((h == 12) | (h == 14), np.where((h & 2) != 0, -1.0, 1.0), 0.0)
        return u + v                                   # -2 .. 2: an exact factor of dx up to one rounding of the sum
    t3 = dx * dx * dx
    t4 = t3 * dx
    t5 = t4 * dx
    w = 6 * t5 - 15 * t4 + 10 * t3
    c0, c1 = coeff(ix), coeff(ix + 1)
    g0 = E(c0 * dx.v, np.abs(c0) * dx.e).rounded()
    d1 = dx - 1
    g1 = E(c1 * d1.v, np.abs(c1) * d1.e).rounded()
    return (1 - w) * g0 + w * g1


def _roc64(cx, u, umax, kappa, w, l, active):
    """radiusOfCurvature (irawan.cpp:453-483) -> R; the branch of rhat is a decision"""
    one = E(1.0)
    rhat = 1 + kappa * (1 + 1 / _tan(umax))
    a = 0.5 * w
    num = 0.5 * l - a * _sin(umax)
    with np.errstate(all="ignore"):
        # Where umax and kappa are exact -- constants of the yarn, the noise off -- rhat is a constant too, and the branch is
        # taken in binary32 as the source takes it: the restatement then evaluates the conic binary32 chose, with its bound
        # (cloth_conics_3x2.weave's parabola yarn has rhat == 0 in binary32 and a few 2^-25 in binary64).  Elsewhere the branch
        # is the binary64 one, ambiguous where rhat lies within its bound of 0 or 1.
        known = (np.broadcast_to(umax.e, rhat.v.shape) == 0) & (np.broadcast_to(kappa.e, rhat.v.shape) == 0)
        k32, u32 = kappa.v.astype(np.float32), umax.v.astype(np.float32)
        rhat32 = (F(1) + k32 * (F(1) + F(1) / tan32(u32))).astype(np.float64)
        sel = np.where(known, rhat32, rhat.v)
        is_circle = sel == 1.0
        cx.rhat |= active & ~known & ((~is_circle & ~(np.abs(rhat.v - 1.0) > rhat.e)) | ~(np.abs(rhat.v) > rhat.e))
    pos = sel > 0
    neg = sel < 0
    with np.errstate(all="ignore"):
        circle = num / _sin(umax)
        tmax = _atan(rhat * _tan(umax))
        bhat = num / _sin(tmax)
        ahat = bhat / rhat
        t = _atan(rhat * _tan(u))
        ct, st = _cos(t), _sin(t)
        ellipse = _pow15(bhat * bhat * ct * ct + ahat * ahat * st * st) / (ahat * bhat)
        ath = lambda x: _log((1 + x) / (1 - x)) / 2
        tmax = -ath(rhat * _tan(umax))
        bhat = num / _sinh(tmax)
        ahat = bhat / rhat
        t = -ath(rhat * _tan(u))
        ch, sh = _cosh(t), _sinh(t)
        hyper = -_pow15(bhat * bhat * ch * ch + ahat * ahat * sh * sh) / (ahat * bhat)
        tm = _tan(umax)
        ah = num / (2 * tm)
        tt = _tan(u)
        parab = 2 * ah * _pow15(1 + tt * tt)
    return _where(is_circle, circle, _where(pos, ellipse, _where(neg, hyper, parab)))


def _von_mises64(cos_x, b):
    absB = float(abs(F(b)))
    bE = E(float(F(b)))
    if absB <= 3.75:
        t = E(absB) / E(float(F(3.75)))
        t = t * t
        c = [float(F(x)) for x in (3.5156229, 3.0899424, 1.2067492, 0.2659732, 0.0360768, 0.0045813)]
        I0 = 1 + t * (c[0] + t * (c[1] + t * (c[2] + t * (c[3] + t * (c[4] + t * c[5])))))
    else:
        t = E(float(F(3.75))) / E(absB)
        c = [float(F(x)) for x in (0.39894228, 0.01328592, 0.00225319, -0.00157565, 0.00916281, -0.02057706, 0.02635537, -0.01647633, 0.00392377)]
        poly = c[8]
        for k in range(7, -1, -1):
            poly = c[k] + t * poly
        I0 = _exp(E(absB)) / E(absB).sqrt() * poly
    return _exp(bE * cos_x).div64(E(2 * PI64).mul64(I0)).rounded()


def _seeliger64(cx, c1, c2, active):
    p1, p2 = cx.lt(E(0.0), c1, active), cx.lt(E(0.0), c2, active)
    s = c1 + c2
    val = E(1.0 / (4.0 * PI64)).mul64(c1).mul64(c2).div64(s).rounded()
    return _where(p1 & p2, val, E(0.0)), p1 & p2


def f64(W, wi, wo, uv):
    """IrawanClothBRDF::f restated -> (value E [n][3], fragile [n] bool, live [n] bool)."""
    wi, wo, uv = (np.asarray(a, dtype=np.float32).astype(np.float64) for a in (wi, wo, uv))
    wi, wo, uv = wi.reshape(-1, 3), wo.reshape(-1, 3), uv.reshape(-1, 2)
    n = wi.shape[0]
    cx_ = _Ctx(n)
    lit = lambda x: E(float(F(x)))
    with np.errstate(all="ignore"):
        live = (wi[:, 2] > 0) & (wo[:, 2] > 0)
        tw, th = int(W.tileWidth), int(W.tileHeight)
        rU, rV = lit(W.repeatU), lit(W.repeatV)
        xyx = _mul(_mul(E(uv[:, 0]), rU), float(tw))
        xyy = _mul(_mul(_sub(1.0, E(uv[:, 1])), rV), float(th))
        ix, iy = cx_.integer(xyx, live), cx_.integer(xyy, live)
        lx, ly = np.mod(ix, tw), np.mod(iy, th)                                   # friendly modulo: always positive
        yid = np.asarray(W.pattern, dtype=np.int64)[lx + ly * tw] - 1
        Y = W.yarns
        col = lambda name: E(np.float64([float(F(getattr(y, name))) for y in Y])[yid])
        warp = np.asarray([int(y.type) for y in Y])[yid] == 0
        kd = np.float64([[float(F(c)) for c in y.kd] for y in Y])[yid]
        ks = np.float64([[float(F(c)) for c in y.ks] for y in Y])[yid]
        # the centre: unsigned division of the (int) cast, converted to Float
        qx = (((ix & 0xFFFFFFFF) // tw) * tw) & 0xFFFFFFFF
        qy = (((iy & 0xFFFFFFFF) // th) * th) & 0xFFFFFFFF
        cxx = _add(_exact(E(qx.astype(np.float64)).rounded()), _mul(col("centerU"), float(tw)))
        cyy = _add(_exact(E(qy.astype(np.float64)).rounded()), _mul(_sub(1.0, col("centerV")), float(th)))
        lx_ = xyx - cxx
        ly_ = -(xyy - cyy)
        w, l, psi, kappa, umax = col("width"), col("length"), col("psi"), col("kappa"), col("umax")
        # weft: rotate xy and both directions by pi / 2 about z
        px, py = _where(warp, lx_, -ly_), _where(warp, ly_, lx_)
        rot = lambda d: (E(np.where(warp, d[:, 0], -d[:, 1])), E(np.where(warp, d[:, 1], d[:, 0])), E(d[:, 2]))
        om_i, om_r = rot(wi), rot(wo)
        if W.period > 0:
            thrv = _mul(float(th), rV)
            twru = _mul(float(tw), rU)
            a, b, c = cx_.integer(cxx, live), cx_.integer(thrv, live), cx_.integer(cyy, live)
            with np.errstate(over="ignore"):
                seed = a.view(np.uint64) * b.view(np.uint64) + c.view(np.uint64)
            draws = random_first_three(seed)
            n1, n2 = E(ulong_to_float(draws[1]).astype(np.float64)), E(ulong_to_float(draws[2]).astype(np.float64))
            per = lit(W.period)
            r1 = _perlin64(cx_, (cxx * (thrv + n1) + cyy) / per, live)
            r2 = _perlin64(cx_, (cyy * (twru + n2) + cxx) / per, live)
            dWarp = E(np.where(warp, float(F(W.dWarpUmaxOverDWarp)), float(F(W.dWeftUmaxOverDWarp))))
            dWeft = E(np.where(warp, float(F(W.dWarpUmaxOverDWeft)), float(F(W.dWeftUmaxOverDWeft))))
            umax = umax + r1 * dWarp + r2 * dWeft
        u = py / (l * 0.5) * umax
        v = px.mul64(PI64).div64(w).rounded()
        result = E(np.zeros((n, 3)))
        if W.ksMultiplier > 0:
            alpha, hW = lit(W.alpha), lit(W.hWidth)
            staple = np.float64([float(F(y.psi)) for y in Y])[yid] != 0
            sum_ = (om_i[0] + om_r[0], om_i[1] + om_r[1], om_i[2] + om_r[2])
            h = _norm64(sum_)
            slen = _len64(sum_)
            fc = alpha + _von_mises64(-_dot64(om_i, om_r), W.beta)
            alive = live & ~cx_.lt(l, w * _sin(umax), live) & ~(kappa.v < -1) & ~((w * _sin(umax)).v == l.v)
            a_ = 0.5 * w
            # --- filament (irawan.cpp:292-366) ---
            fa = alive & ~staple
            ss = lit(W.ss)
            u_of_v = _atan(h[1] / h[2])
            inside = cx_.lt(abs(u_of_v), umax, fa)
            su, cu, sv, cv = _sin(u_of_v), _cos(u_of_v), _sin(v), _cos(v)
            nrm = _norm64((sv, su * cv, cu * cv))
            tl = (cu * cu + su * su).sqrt()
            t = (cu / tl, -su / tl)                                               # (0, t.y, t.z)
            lim = _mul(_sub(1.0, ss), umax)
            small = cx_.lt(abs(u_of_v), lim, fa & inside)
            R = _roc64(cx_, _where(small, abs(u_of_v), lim), lim, kappa, w, l, fa & inside)
            tch_x = t[0] * h[2] - t[1] * h[1]
            Gu = a_ * (R + a_ * cv) / (slen * abs(tch_x))
            A, lit_ = _seeliger64(cx_, _dot64(nrm, om_i), _dot64(nrm, om_r), fa & inside)
            if float(ss.v) == 0:
                As = A
            else:
                x = (abs(u_of_v) - (1 - ss) * umax) / (ss * umax)
                lo, hi = cx_.lt(x, E(0.0), fa & inside & lit_), cx_.lt(E(1.0), x, fa & inside & lit_)
                sv_ = _where(lo, E(0.0), _where(hi, E(1.0), x))
                As = A * (1 - sv_ * sv_ * (-2 * sv_ + 3))
            fs = (Gu * fc * As).mul64(PI64).mul64(l).rounded()
            dy = l * hW
            y_of_v = u_of_v * 0.5 * l / umax
            hi_, lo_ = 0.5 * (l - dy), 0.5 * (dy - l)
            act = fa & inside & lit_
            above, below = cx_.lt(hi_, y_of_v, act), cx_.lt(y_of_v, lo_, act)
            y_of_v = _where(above, hi_, _where(below, lo_, y_of_v))
            win = cx_.lt(abs(y_of_v - u * 0.5 * l / umax), 0.5 * dy, act)
            filament = _where(fa & inside & win, fs / dy, E(0.0))
            # --- staple (irawan.cpp:384-451) ---
            sa = alive & staple
            psiS = _where(staple, psi, E(1.0))                                    # keep the filament records finite
            su, cu = _sin(u), _cos(u)
            q = h[1] * su + h[2] * cu
            D = (h[1] * cu - h[2] * su) / ((h[0] * h[0] + q * q).sqrt() * _tan(psiS))
            inD = cx_.lt(abs(D), E(1.0), sa)
            Dc = _where(inD, D, E(0.0))
            ya = -h[1] * su - h[2] * cu
            # atan2's cut: with h.x < 0 the sign of its first argument moves v_of_u by 2 pi -- one more decision of the source
            cx_.amb |= sa & inD & ~(h[0].v - h[0].e > 0) & ~(np.abs(ya.v) > ya.e)
            v_of_u = _atan2(ya, h[0]) + _acos(Dc)
            inV = cx_.lt(abs(v_of_u), E(PI64 / 2.0), sa & inD)
            act = sa & inD & inV
            sv, cv = _sin(v_of_u), _cos(v_of_u)
            nrm = _norm64((sv, su * cv, cu * cv))
            R = _roc64(cx_, abs(u), umax, kappa, w, l, act)
            Gv = a_ * (R + a_ * cv) / (slen * _dot64(nrm, h) * abs(_sin(psiS)))
            A, lit_ = _seeliger64(cx_, _dot64(nrm, om_i), _dot64(nrm, om_r), act)
            fs = Gv * fc * A
            fs = fs * 2 * w * umax
            dx = w * hW
            x_of_u = (v_of_u * w).div64(PI64).rounded()
            hi_, lo_ = 0.5 * (w - dx), 0.5 * (dx - w)
            sel = act                                                             # the source returns fs / delta_x whatever A is: 0 * NaN stays a NaN
            act = act & lit_
            above, below = cx_.lt(hi_, x_of_u, act), cx_.lt(x_of_u, lo_, act)
            x_of_u = _where(above, hi_, _where(below, lo_, x_of_u))
            win = cx_.lt(abs(x_of_u.add64(-((v * w).div64(PI64)))), 0.5 * dx, act)
            stap = _where(sel & win, fs / dx, E(0.0))
            integrand = _where(staple, stap, filament)
            integrand = _where(alive, integrand, E(0.0))
            variation = E(np.ones(n))
            if W.fineness > 0:
                fin = lit(W.fineness)
                a, b, c = cx_.integer((cxx + px) * fin, live), cx_.integer(_mul(_mul(float(th), rV), fin), live), cx_.integer((cyy + py) * fin, live)
                with np.errstate(over="ignore"):
                    seed = a.view(np.uint64) * b.view(np.uint64) + c.view(np.uint64)
                xi = E(ulong_to_float(random_first_three(seed)[0]).astype(np.float64))
                ml = -_log(_where(xi.v > 0, xi, E(1.0)))
                ml = _where(xi.v > 0, ml, E(np.inf))
                capped = cx_.lt(E(10.0), ml, live & (xi.v > 0)) | ~(xi.v > 0)
                variation = _where(capped, E(10.0), ml)
            s = variation * lit(W.ksMultiplier) * integrand
            wa, fa_ = lit(W.warpArea), lit(W.weftArea)
            area = _where(warp, (wa + fa_) / wa, (wa + fa_) / fa_)
            result = E(ks * s.v[:, None], np.abs(ks) * s.e[:, None]).rounded() * E(area.v[:, None], area.e[:, None])
        kdm = E(kd) * lit(W.kdMultiplier)
        value = result + kdm if W.ksMultiplier > 0 else kdm
        value = E(np.where(live[:, None], value.v, 0.0), np.where(live[:, None], value.e, 0.0))
        scale = np.maximum(np.abs(value.v), np.abs(kdm.v).max(axis=1, keepdims=True))
        loose = ~(value.e <= FRAGILE_RELATIVE * np.maximum(scale, 2.0 ** -126))
        fragile = live & (cx_.amb | cx_.rhat | loose.any(axis=1) | ~np.isfinite(value.v).all(axis=1))
    return value, fragile, live


def eval64(W, twosided, op, wi, aux, uv, wo32=None):
    """ops 0 (f) and 2 (the value of sample(bRec, pdf, s) at the mirror's binary32 direction wo32) behind the twosided adapter or
    not -> (value E [n][3], fragile, live).  pdf is cos / pi, one product, and is compared where it is used"""
    wi = np.asarray(wi, dtype=np.float32).reshape(-1, 3).copy()
    flip = (wi[:, 2] < 0) if twosided else np.zeros(len(wi), dtype=bool)
    wi[flip, 2] *= -1
    wo = np.asarray(aux if op == 0 else wo32, dtype=np.float32).reshape(-1, 3).copy()
    if op == 0:
        wo[flip, 2] *= -1
    return f64(W, wi, wo, uv)


def ratio(got32, want, skip):
    """the largest |binary32 value - restatement| / bound over the records that are not skipped, and the worst record"""
    with np.errstate(all="ignore"):
        d = np.abs(np.asarray(got32, dtype=np.float64) - want.v)
        r = np.where(d == 0, 0.0, d / np.where(want.e > 0, want.e, np.where(d == 0, 1.0, 0.0)))
        r = np.where(np.isnan(r), np.inf, r)
    r = np.where(np.asarray(skip)[:, None], 0.0, r)
    k = int(np.argmax(r.max(axis=1)))
    return float(r.max()), k
