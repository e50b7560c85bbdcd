"""The inputs that tests/test_cloth.py (CPU) and tests/test_gpu_cloth.py (device) share for the woven-cloth BRDF: the two weave files
of tests/golden/ in four variants each, random records, and named records on and beside the thresholds of f.

Weaves.  cloth_plain_2x2.weave: one warp filament yarn (psi = 0) and one weft staple yarn (psi = -30 degrees) on a 2 x 2 tile,
both ellipses (rhat > 1).  cloth_conics_3x2.weave: three yarns on a 3 x 2 tile whose kappa reaches the circle (rhat == 1), the
parabola (rhat == 0 exactly while the noise is off), ellipses and hyperbolas next to it once the noise moves umax, and the
hyperbola.  Variants: period and fineness off / on, repeat 1 / (3, 2.5), one with ksMultiplier = 0, and one whose weft spine is nearly a
circle (kappa = 1e-3).

Records.  Random: uv in the unit square, wi and wo uniform on the upper hemisphere, every tenth record with one direction
below.  Outside: uv in [-0.5, 1.5]^2 outside the unit square, where the unsigned arithmetic of the yarn centre shows.  Thresholds: records whose wo is bisected along a great arc until the
mirror's margin of a highlight test changes sign between two neighbouring binary32 directions -- |u_of_v| = umax and the y window of
the filament, |D| = 1, |v_of_u| = pi / 2 and the x window of the staple -- with the direction on either side and one binary32 step
beyond each.  Named: uv on the borders
of the yarn cells and one binary32 step to either side; uv < 0 and uv.y > 1; a record whose center.x + xy.x is negative for the
weft yarn (the undefined cast); grazing directions (cosines of 1e-4 and one step above zero), the horizon (+0, -0) and back-side
directions; wi == wo (the half vector along both); the mirror direction of wi.  Test infrastructure."""
import os

import numpy as np

import ref64_cloth as R

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = ("cloth_plain_2x2.weave", "cloth_conics_3x2.weave")


def text(name):
    with open(os.path.join(GOLDEN, name)) as fh:
        return fh.read()


def weaves(mts):
    """[(name, Weave)]"""
    out = []
    for fname in FILES:
        for tag, fin, per, rep, ks in (("plain", 0.0, 0.0, (1.0, 1.0), 1.0), ("noise", 2.0, 3.0, (1.0, 1.0), 1.0),
                                       ("repeat", 0.0, 0.0, (3.0, 2.5), 2.0), ("noise repeat", 3.5, 1.75, (3.0, 2.5), 0.5),
                                       ("diffuse only", 2.0, 3.0, (3.0, 2.5), 0.0)):
            w = mts.load_weave(text(fname), dict(fineness=fin, period=per, weft_ks=(0.6, 0.7, 0.8)))
            out.append(("%s, %s" % (fname, tag), w.replace(repeatU=rep[0], repeatV=rep[1], ksMultiplier=ks, kdMultiplier=0.75)))
    # the weft yarn of the first file with a spine that is nearly, not exactly, a circle (rhat = 1 + 3e-3)
    w = mts.load_weave(text(FILES[0]), dict(fineness=0.0, period=0.0, weft_ks=(0.6, 0.7, 0.8)))
    w.yarns[1].kappa = F(1e-3)
    out.append(("%s, near circle" % FILES[0], w))
    return out


def usable(W, uv):
    """the records a weave takes: with period or fineness on, a negative xy (u repeatU < 0 or (1 - v) repeatV < 0) makes the yarn
    centre 2^32 and more, and the noise arguments and seed factors leave the range the library holds them to"""
    uv = np.asarray(uv, dtype=np.float32)
    if not (W.period > 0 or W.fineness > 0):
        return np.ones(len(uv), dtype=bool)
    return (uv[:, 0] * F(W.repeatU) >= 0) & ((F(1) - uv[:, 1]) * F(W.repeatV) >= 0)


def _hemisphere(rng, n):
    z = rng.rand(n)
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = 2 * np.pi * rng.rand(n)
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32)


def random_records(seed, n=3000):
    """(wi, wo, uv, sample) float32"""
    rng = np.random.RandomState(seed)
    wi, wo = _hemisphere(rng, n), _hemisphere(rng, n)
    wi[::10, 2] *= -1
    wo[5::10, 2] *= -1
    uv = rng.rand(n, 2).astype(np.float32)
    return wi, wo, uv, rng.rand(n, 2).astype(np.float32)


def outside_records(seed, n=750):
    """(wi, wo, uv, sample) with uv in [-0.5, 1.5]^2 outside the unit square: the unsigned arithmetic of the yarn centre.  Named
    inputs, counted apart from the random set: where (int) xy is negative the centre is 2^32 and xy - centre cancels, so the
    binary64 restatement has no useful bound there, and only the mirror and the device are compared"""
    rng = np.random.RandomState(seed + 1000)
    wi, wo = _hemisphere(rng, n), _hemisphere(rng, n)
    uv = (rng.rand(4 * n, 2) * 2 - 0.5).astype(np.float32)
    uv = uv[((uv < 0) | (uv > 1)).any(axis=1)][:n]
    return wi[:len(uv)], wo[:len(uv)], uv, rng.rand(len(uv), 2).astype(np.float32)


def _at(cos, phi):
    s = np.sqrt(max(0.0, 1.0 - cos * cos))
    return np.float32([s * np.cos(phi), s * np.sin(phi), cos])


def named_records(W):
    """(names, wi, wo, uv, sample): every named uv with every named pair of directions"""
    step = float(np.nextafter(F(0), F(1)))
    up = _at(0.8, 0.4)
    pairs = [("oblique", _at(0.6, 0.3), _at(0.7, 2.9)), ("same", up, up), ("mirror", up, np.float32([-up[0], -up[1], up[2]])),
             ("normal", np.float32([0, 0, 1]), np.float32([0, 0, 1])), ("grazing 1e-4", _at(1e-4, 1.0), _at(0.5, 4.0)),
             ("grazing step", _at(step, 2.0), _at(step, 5.0)), ("horizon +0", _at(0.0, 0.3), up), ("horizon -0", up, np.float32([0.6, 0.8, -0.0])),
             ("wi below", np.float32([0.3, 0.4, -0.8660254]), up), ("wo below", up, np.float32([0.3, 0.4, -0.8660254])),
             ("both below", -up, -_at(0.6, 1.0))]
    tw, th, ru, rv = float(W.tileWidth), float(W.tileHeight), float(W.repeatU), float(W.repeatV)
    uvs = []

    def beside(name, u, v):
        u, v = F(u), F(v)
        for du in (-1, 0, 1):
            for dv in (-1, 0, 1):
                uu = u if du == 0 else np.nextafter(u, F(du * np.inf))
                vv = v if dv == 0 else np.nextafter(v, F(dv * np.inf))
                uvs.append(("%s %+d %+d" % (name, du, dv), uu, vv))

    # the borders of the yarn cells: xy.x = k, xy.y = k
    for k in range(0, int(tw) + 1):
        beside("cell border x=%d" % k, k / (ru * tw), 0.3)
    for k in range(0, int(th) + 1):
        beside("cell border y=%d" % k, 0.6, 1.0 - k / (rv * th))
    beside("corner", 1.0 / (ru * tw), 1.0 - 1.0 / (rv * th))
    for name, u, v in (("centre of a cell", 0.5 / (ru * tw), 1.0 - 0.5 / (rv * th)), ("u < 0", -0.3, 0.4), ("u < -1 tile", -1.7, 0.4),
                       ("v > 1", 0.4, 1.3), ("v > 2", 0.4, 2.6), ("both outside", -0.9, 1.9), ("v < 0", 0.2, -0.7),
                       # the weft cell at the top left of either pattern: xy.y small, its centre's y large -> center.x + xy.x < 0
                       ("negative seed factor", 1.2 / (ru * tw), 1.0 - 0.05 / (rv * th)), ("negative seed factor 2", 1.9 / (ru * tw), 1.0 - 0.01 / (rv * th))):
        uvs.append((name, F(u), F(v)))
    names, wi, wo, uv = [], [], [], []
    for un, u, v in uvs:
        for pn, a, b in pairs:
            names.append(un + " | " + pn); wi.append(a); wo.append(b); uv.append((u, v))
    n = len(names)
    rng = np.random.RandomState(7)
    sample = rng.rand(n, 2).astype(np.float32)
    sample[::7] = (0.0, 0.0)
    sample[3::7] = (1.0, 0.25)      # the rim of squareToHemispherePSA
    return names, np.float32(wi), np.float32(wo), np.float32(uv), sample


THRESHOLDS = {"u_of_v = umax": False, "y window": False, "D = 1": True, "v_of_u = pi / 2": True, "x window": True}      # name: on a staple yarn


def _margins(W, wi, wo, uv):
    R.PROBE = {}
    try:
        _, info = R.f32(W, wi, wo, uv)
        return {k: np.array(v, dtype=np.float64) for k, v in R.PROBE.items()}, info[:, 0].astype(np.int64)
    finally:
        R.PROBE = None


def threshold_records(W, seed=3, per_test=3, candidates=1500):
    """(names, wi, wo, uv, sample): for every highlight test of the weave's integrands, up to per_test brackets.  A bracket: uv and wi
    fixed, wo moved along the arc from a direction where the mirror's margin of the test is negative to one where it is
    positive, bisected in binary64 until the two ends round to neighbouring binary32 directions; its four records are the end on
    either side and one more binary32 step of wo.x beyond each.  The weave's noise is off (the margins are the mirror's own)"""
    rng = np.random.RandomState(seed)
    wi, a, b = _hemisphere(rng, candidates), _hemisphere(rng, candidates).astype(np.float64), _hemisphere(rng, candidates).astype(np.float64)
    uv = rng.rand(candidates, 2).astype(np.float32)
    staple = np.array([float(y.psi) != 0 for y in W.yarns])

    def at(t):
        d = (1 - t)[:, None] * a + t[:, None] * b
        return (d / np.sqrt((d * d).sum(axis=1, keepdims=True))).astype(np.float32)
    zero, one = np.zeros(candidates), np.ones(candidates)
    m0, yid = _margins(W, wi, at(zero), uv)
    m1, _ = _margins(W, wi, at(one), uv)
    names, rec = [], []
    with np.errstate(all="ignore"):
        for test, on_staple in THRESHOLDS.items():
            if test not in m0:
                continue
            ok = np.isfinite(m0[test]) & np.isfinite(m1[test]) & (np.sign(m0[test]) * np.sign(m1[test]) < 0) & (staple[yid] == on_staple)
            if not ok.any():
                continue
            lo, hi = zero.copy(), one.copy()
            neg_at_lo = m0[test] < 0
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                mm = _margins(W, wi, at(mid), uv)[0][test]
                same = (mm < 0) == neg_at_lo
                lo, hi = np.where(same, mid, lo), np.where(same, hi, mid)
            # brackets across which the value of f changes -- the test is the one that decides there -- come first
            live = (R.f32(W, wi, at(lo), uv)[0] != R.f32(W, wi, at(hi), uv)[0]).any(axis=1)
            order = np.nonzero(ok)[0]
            pick = np.concatenate([order[live[order]], order[~live[order]]])[:per_test]
            for i in pick:
                for side, t in (("before", lo), ("after", hi)):
                    w0 = at(t)[i]
                    for step in (0, -1, 1):
                        w = w0.copy()
                        if step:
                            w[0] = np.nextafter(w[0], F(step * np.inf))
                        names.append("%s | bracket %d %s %+d" % (test, i, side, step)); rec.append((wi[i], w, uv[i]))
    n = len(names)
    return names, np.float32([r[0] for r in rec]).reshape(n, 3), np.float32([r[1] for r in rec]).reshape(n, 3), \
        np.float32([r[2] for r in rec]).reshape(n, 2), rng.rand(n, 2).astype(np.float32)
