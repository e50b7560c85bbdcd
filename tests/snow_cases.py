"""The inputs that tests/test_snow.py (CPU) and tests/test_gpu_snow.py (device) share for the snow BRDFs: the parameter sets of
both models and the direction classes -- normal incidence, the oblique class (cosines of 0.5 and 1e-3), the grazing class
(cosines of 1e-4 and of one binary32 step above zero, 2^-149, and their twins one step below), the horizon class (wi.z and wo.z
at +0 and -0) -- with samples on the borders of the unit square that squareToHemispherePSA maps.  Every case runs plain and
under the twosided adapter, and every direction comes with its twin below the surface (z negated), which the adapter flips.

A record is classed by the conditioning of its directions, which is what the classes are for.  The grazing class holds every
direction whose cosine lies in (0, 1e-4]: there fresnel's 1 - R cancels, at one step above zero completely (R rounds to 1, and
1 / (|cos wi| + |cos wo|) of two such cosines overflows binary32).  So of "zero and one step either side" the two steps are
grazing directions -- the step below is the twin of the step above -- and the horizon class keeps the two zeros, where only the
side tests decide.

The parameter sets vary one parameter at a time from the reference's defaults: the value of either model is a product of factors
that each depend on one parameter (HanrahanKrueger: albedo, the Fresnel product of eta, the phase function of g, the two
factors; Wiscombe: albedo(mu0) of the derived spectra, fBar of the cosines alone), so a cross product adds records, not paths
through the code.  A class's records pair its directions with each other and with two well-conditioned ones (normal incidence and
a cosine of 0.5), so what a class shows of conditioning is owed to its own directions.  Test infrastructure."""
import numpy as np

import ref64_snow as R

F = np.float32
CLASSES = ("normal", "oblique", "grazing", "horizon")
GRAZING = "grazing"
_AZIMUTHS = (0.3, 1.9, 3.7, 5.2)
_STEP = float(np.nextafter(F(0), F(1)))


def wiscombe_params():
    """[(name, raw)]: the defaults; g in {0.5, 0.874}; depth in {0.1, 1}; a coloured w0"""
    return [("defaults", R.wiscombe_raw()), ("g 0.5", R.wiscombe_raw(g=0.5)), ("depth 0.1", R.wiscombe_raw(depth=0.1)),
            ("g 0.5 depth 0.1", R.wiscombe_raw(g=0.5, depth=0.1)), ("coloured w0", R.wiscombe_raw(w0=(0.99, 0.95, 0.9)))]


def hk_params():
    """[(name, raw)]: the defaults (g 0, eta 1.32); g in {0.5, -0.5}; eta in {1, 1 / 1.32}; ssFactor 0; the flag off"""
    return [("defaults", R.hk_raw()), ("g 0.5", R.hk_raw(g=0.5)), ("g -0.5", R.hk_raw(g=-0.5)),
            ("eta 1", R.hk_raw(eta_int=1.0, eta_ext=1.0)), ("eta 1/1.32", R.hk_raw(eta_int=1.0, eta_ext=1.32)),
            ("ssFactor 0", R.hk_raw(g=0.5, ss_factor=0.0)), ("flag off", R.hk_raw(g=-0.5, diffuse_reflectance=False))]


def models():
    """[(name, kind, raw)] of both lists"""
    return [("wiscombe " + n, R.WISCOMBE, r) for n, r in wiscombe_params()] + [("hk " + n, R.HK, r) for n, r in hk_params()]


def _at(cos, phi):
    s = np.sqrt(max(0.0, 1.0 - cos * cos))
    return np.float32([s * np.cos(phi), s * np.sin(phi), cos])


def class_directions(name):
    """the upper-side directions of a class, binary32"""
    if name == "normal":
        return np.float32([[0, 0, 1]])
    if name == "horizon":
        return np.stack([_at(z, phi) for z, phi in ((0.0, 0.3), (-0.0, 5.2))])
    cosines = {"oblique": (0.5, 1e-3), "grazing": (1e-4, _STEP)}[name]
    return np.stack([_at(cos, phi) for cos in cosines for phi in _AZIMUTHS])


def _mix():
    """normal incidence, a cosine of 0.5, and one direction below the surface"""
    return np.stack([_at(1.0, 0.0), _at(0.5, 4.4), _at(-0.6, 1.1)])


def eval_records(name):
    """(wi [n][3], wo [n][3]) of a class: its directions as wi against the mix and as wo against the mix, and its directions
    against themselves; then the same with wi below the surface (z negated), which the twosided adapter flips"""
    own, mix = class_directions(name), _mix()
    rec = [(w, o) for w in own for o in mix] + [(w, o) for w in mix for o in own] + [(w, o) for w in own for o in own]
    wi, wo = np.float32([r[0] for r in rec]), np.float32([r[1] for r in rec])
    below = wi * np.float32([1, 1, -1])
    return np.concatenate([wi, below]), np.concatenate([wo, wo * np.float32([1, 1, -1])])


def sample_points():
    """s on the borders of the unit square and of the quadrants of phi = 2 pi s.y, one step inside them, and inside"""
    top = float(F(1) - F(2.0 ** -24))
    xs = [0.0, _STEP, 2.0 ** -24, 0.3, 0.81, top]
    ys = [0.0, _STEP, 0.25, 0.5, float(np.nextafter(F(0.5), F(0))), 0.75, 0.37, top]
    return np.float32([(x, y) for x in xs for y in ys])


def sample_records(name):
    """(wi [n][3], s [n][2]) of a class: each of its directions, above and below the surface, with every sample point"""
    own = class_directions(name)
    wi = np.concatenate([own, own * np.float32([1, 1, -1])])
    s = sample_points()
    return np.repeat(wi, len(s), axis=0), np.tile(s, (len(wi), 1))
