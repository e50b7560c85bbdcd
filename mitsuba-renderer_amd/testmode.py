"""Test-case mode (`mitsuba -t`): the .m file MFilm::develop writes and the per-pixel test TestSupervisor::analyze runs on it.

    write_mfile   <- MFilm::develop                (src/films/mfilm.cpp:173-221), byte for byte
    analyze       <- TestSupervisor::analyze       (src/librender/testcase.cpp:111-259)
    student_t_two_sided                            the p-value boost::math::students_t gives there

The film and its statistics come from MIPathTracer.film() / .film_statistics() (mtsgpu_read_film_statistics).  Host-side
file handling only: no device work, and nothing beyond numpy."""
import math
from collections import namedtuple

import numpy as np

F = np.float32
EPSILON = F(1e-4)                      # Epsilon of a single-precision build (include/mitsuba/core/constants.h)
T_TEST, RELERR = "t-test", "relerr"   # Scene::ETTest, Scene::ERelativeError (scene.h:55-59)

AnalyzeResult = namedtuple("AnalyzeResult", "ok message rejects")


class TestModeError(ValueError):
    """what the reference stops on with SAssert / Log(EError): a file analyze() cannot take apart"""
    __test__ = False


def luminance(spec):
    """Spectrum::getLuminance of an RGB build (spectrum.h:387-389): binary32, left to right"""
    s = np.asarray(spec, dtype=F)
    return (s[..., 0] * F(0.212671) + s[..., 1] * F(0.715160)) + s[..., 2] * F(0.072169)


def _f(v):
    """printf("%f") of a Float: glibc writes a NaN with its sign, Python's % operator drops it"""
    v = float(v)
    if v != v:
        return "-nan" if math.copysign(1.0, v) < 0 else "nan"
    return "%f" % v


def write_mfile(path, film, stats=None, spectra=False):
    """MFilm::develop (mfilm.cpp:173-221).  film: [H][W][5] f32 sums (spectrum rgb, alpha, weight); stats: None or the pair
    (variance [H][W][3] f32, nSamples [H][W] u32) -- with it every value becomes the triple `value variance nSamples`
    (m_hasVariances); spectra: the film's exportSpectra property, one entry per channel instead of the luminance."""
    film = np.asarray(film, dtype=F)
    H, W = film.shape[:2]
    w = film[..., 4]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(w > 0, F(1) / w, F(1)).astype(F)             # Float invWeight = pixel.weight > 0 ? 1/pixel.weight : 1
    var = ns = None
    if stats is not None:
        var = np.asarray(stats[0], dtype=F).reshape(H, W, 3)
        ns = np.asarray(stats[1]).reshape(H, W)
    if spectra:
        val = (inv[..., None] * film[..., :3]).astype(F)            # Spectrum spec = invWeight * pixel.spec
        vv = var
    else:
        val = (inv * luminance(film[..., :3])).astype(F)[..., None]  # invWeight * pixel.spec.getLuminance()
        vv = luminance(var)[..., None] if var is not None else None
    rows = []
    for y in range(H):
        cells = []
        for x in range(W):
            if vv is None:
                cells.append(" ".join(_f(v) for v in val[y, x]))
            else:
                cells.append(" ".join("%s %s %i" % (_f(v), _f(q), int(ns[y, x])) for v, q in zip(val[y, x], vv[y, x])))
        rows.append(", ".join(cells))
    with open(path, "w") as f:
        f.write("[" + ";\n ".join(rows) + "]\n")


def _tokens(line):
    """tokenize(line, " \\t;,[]") (src/libcore/util.cpp): split at any of the delimiters, no empty tokens"""
    for d in "\t;,[]\r":
        line = line.replace(d, " ")
    return [t for t in line.split(" ") if t]


def _number(tok, integer=False):
    try:
        return int(tok, 10) if integer else F(float(tok))
    except ValueError:
        raise TestModeError("Error while parsing a testcase output file")


def parse_ref_file(path):
    """parseRefFile (testcase.cpp:117-133): every number of the file"""
    out = []
    with open(path) as f:
        for line in f.read().split("\n"):
            out += [_number(t) for t in _tokens(line)]
    return out


def parse_mfile(path, test_type):
    """parseMFile (testcase.cpp:135-161): (value, variance, nSamples) per entry for the t-test, the value alone otherwise"""
    out = []
    with open(path) as f:
        for line in f.read().split("\n"):
            tok = _tokens(line)
            if test_type != RELERR and len(tok) % 3 != 0:
                raise TestModeError("Assertion 'testType == Scene::ERelativeError || (tokens.size() % 3) == 0' failed: "
                                    "the output file holds no (value, variance, nSamples) triples")
            i = 0
            while i < len(tok):
                value = _number(tok[i]); i += 1
                variance, n = F(0), 0
                if test_type == T_TEST:
                    if i + 1 >= len(tok):
                        raise TestModeError("Error while parsing a testcase output file")
                    variance = _number(tok[i]); n = _number(tok[i + 1], integer=True); i += 2
                out.append((value, variance, n))
    return out


# --- Student's t ---------------------------------------------------------------------------------------------------------
def _betacf(a, b, x):
    """continued fraction of the incomplete beta function (modified Lentz), arrays; converges fast for x < (a+1)/(a+b+2)"""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = np.ones_like(x)
    d = 1.0 - qab * x / qap
    d = np.where(np.abs(d) < tiny, tiny, d)
    d = 1.0 / d
    h = d.copy()
    for m in range(1, 100000):
        m2 = 2.0 * m
        aa = m * (b - m) * x / ((qam + m2) * (a + m2))
        d = 1.0 + aa * d; d = np.where(np.abs(d) < tiny, tiny, d)
        c = 1.0 + aa / c; c = np.where(np.abs(c) < tiny, tiny, c)
        d = 1.0 / d
        h = h * d * c
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))
        d = 1.0 + aa * d; d = np.where(np.abs(d) < tiny, tiny, d)
        c = 1.0 + aa / c; c = np.where(np.abs(c) < tiny, tiny, c)
        d = 1.0 / d
        delta = d * c
        h = h * delta
        if np.all(np.abs(delta - 1.0) < 3e-16):
            return h
    raise ArithmeticError("incomplete beta: continued fraction did not converge")


def betainc(a, b, x):
    """regularised incomplete beta function I_x(a, b) in binary64 (arrays broadcast)"""
    a, b, x = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(x, dtype=np.float64))
    out = np.zeros(x.shape, dtype=np.float64)
    out[x >= 1.0] = 1.0
    inside = (x > 0.0) & (x < 1.0)
    if inside.any():
        ai, bi, xi = a[inside], b[inside], x[inside]
        lg = np.vectorize(math.lgamma, otypes=[np.float64])
        front = np.exp(lg(ai + bi) - lg(ai) - lg(bi) + ai * np.log(xi) + bi * np.log1p(-xi))
        swap = xi >= (ai + 1.0) / (ai + bi + 2.0)                    # I_x(a, b) = 1 - I_(1-x)(b, a)
        res = np.empty_like(xi)
        if (~swap).any():
            res[~swap] = front[~swap] * _betacf(ai[~swap], bi[~swap], xi[~swap]) / ai[~swap]
        if swap.any():
            res[swap] = 1.0 - front[swap] * _betacf(bi[swap], ai[swap], 1.0 - xi[swap]) / bi[swap]
        out[inside] = res
    return out


def student_t_two_sided(T, df):
    """2 * (1 - cdf_t(|T|, df)) = I_x(df / 2, 1 / 2) with x = df / (df + T^2): the two-sided tail of Student's t distribution
    (what 2 * cdf(complement(students_t(df), |T|)) gives in testcase.cpp:219-220).  NaN statistics give NaN."""
    T = np.asarray(T, dtype=np.float64); df = np.asarray(df, dtype=np.float64)
    if np.any(df <= 0):
        raise TestModeError("Student's t needs at least one degree of freedom (nSamples >= 2)")
    T, df = np.broadcast_arrays(T, df)
    t2 = T * T
    ok = np.isfinite(t2)
    p = np.full(T.shape, np.nan)
    p[np.isinf(t2)] = 0.0
    if ok.any():
        t2o, dfo = t2[ok], df[ok]
        # the tail through whichever argument is the small one: x for large |T|, 1 - x = T^2 / (df + T^2) for small
        x = dfo / (dfo + t2o)
        small = t2o < dfo
        res = np.empty_like(x)
        if (~small).any():
            res[~small] = betainc(dfo[~small] / 2.0, 0.5, x[~small])
        if small.any():
            res[small] = 1.0 - betainc(0.5, dfo[small] / 2.0, t2o[small] / (dfo[small] + t2o[small]))
        p[ok] = res
    return p if p.shape else float(p)


def analyze(m_path, ref_path, test_type=T_TEST, thresh=0.01):
    """TestSupervisor::analyze (testcase.cpp:168-259) on a written .m file and its .ref: returns (ok, message, rejects).
    message is the reference's for the FIRST failing pixel (where it stops), "" on success; rejects counts all failing
    pixels.  Arithmetic in binary32 as a single-precision build does it; the p-value in binary64, then rounded."""
    if test_type not in (T_TEST, RELERR):
        raise TestModeError("Unknown test type!")
    actual = parse_mfile(m_path, test_type)
    ref = parse_ref_file(ref_path)
    if len(actual) != len(ref):
        return AnalyzeResult(False, "Output format does not match the reference (%i vs %i pixels)!" % (len(actual), len(ref)), 0)
    if not actual:
        return AnalyzeResult(True, "", 0)
    thresh = F(thresh)
    value = np.array([a[0] for a in actual], dtype=F); r = np.array(ref, dtype=F)
    diff = (value - r).astype(F)
    with np.errstate(all="ignore"):
        if test_type == T_TEST:
            variance = np.array([a[1] for a in actual], dtype=F); n = np.array([a[2] for a in actual], dtype=np.int64)
            var = np.where(variance < EPSILON, EPSILON, variance).astype(F)        # std::max(variance, Epsilon): a NaN stays
            T = (diff * np.sqrt((n.astype(F) / var).astype(F))).astype(F)
            df = n - 1
            p = np.asarray(student_t_two_sided(np.abs(T), df)).astype(F)
            bad = p <= thresh
            if bad.any():
                i = int(np.argmax(bad))
                msg = "t-test REJECTS: result=%f (ref=%f), diff=%e, var=%f T-stat=%f, df=%i, p-value=%f" % (
                    float(value[i]), float(r[i]), float(diff[i]), float(var[i]), float(T[i]), int(df[i]), float(p[i]))
                return AnalyzeResult(False, msg, int(bad.sum()))
        else:
            relerr = np.abs((diff / np.where(EPSILON < r, r, EPSILON)).astype(F))     # std::max(Epsilon, ref)
            bad = relerr > thresh
            if bad.any():
                i = int(np.argmax(bad))
                msg = "Relative error threshold EXCEEDED: result=%f (ref=%f), diff=%e, relerr=%f" % (
                    float(value[i]), float(r[i]), float(diff[i]), float(relerr[i]))
                return AnalyzeResult(False, msg, int(bad.sum()))
    return AnalyzeResult(True, "", 0)
