"""The inputs that tests/test_mask.py (CPU) and tests/test_gpu_mask.py (device) share for the Mask adapter: the opacities, the
samples on, just below and just above them, grazing and back-side directions, and every nested type 0..8 with and without the
twosided adapter.  Test infrastructure."""
import numpy as np

F = np.float32
P_VALUES = [0.0, 0.25, 0.5, 1.0, 1.5]
# spectra whose luminance is not their mean (for the luminance itself), next to the grey levels above
COLOURS = [(0.2, 0.7, 0.1), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.9, 0.1, 0.5), (0.0, 1.0, 0.0)]


def models(mts):
    """[(name, bsdf_type, params)]: one block per nested type 0..8, plain and twosided"""
    S, A = mts.scenes, mts.abi
    sd = S.SceneDescription("mask cases")
    ids = [("lambertian", sd.lambertian(0.5, 0.6, 0.4)), ("dielectric", sd.dielectric()), ("roughmetal", sd.roughmetal(0.3)),
           ("microfacet", sd.microfacet(0.2)), ("mirror", sd.mirror(0.7)), ("phong", sd.phong(15.0, 0.4, 0.3)),
           ("roughglass", sd.roughglass(0.2)), ("difftrans", sd.difftrans(0.6)), ("ward", sd.ward(0.15, 0.3))]
    out = []
    for name, i in ids:
        assert sd.bsdf_type[i] == len(out) // 2
        out.append((name, sd.bsdf_type[i], sd.bsdf_params[i].copy()))
        out.append(("twosided " + name, sd.bsdf_type[i] | A.BSDF_TWOSIDED, sd.bsdf_params[i].copy()))
    return out


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return (v / np.sqrt((v * v).sum())).astype(np.float32)


def directions():
    """wi: steep, oblique, grazing on either side, and the back side"""
    return np.stack([_unit((0.3, 0.2, 0.9)), _unit((-0.6, 0.5, 0.4)), _unit((0.7, -0.7, 1e-3)), _unit((0.5, 0.8, -1e-3)),
                     _unit((0.2, -0.3, -0.8)), _unit((-0.4, -0.1, -0.5))])


def outgoing():
    """wo of the f and pdf queries: both sides, one near the mirror direction of the first wi"""
    return np.stack([_unit((-0.3, -0.2, 0.9)), _unit((0.1, 0.6, 0.5)), _unit((0.4, 0.1, -0.7)), _unit((-0.7, 0.7, 2e-3))])


def sample_x(p):
    """s.x on p, one binary32 step below and above it, and away from it -- what a sampler can return: [0, 1)"""
    p = F(p)
    xs = [p, np.nextafter(p, F(-np.inf)), np.nextafter(p, F(np.inf)), F(0.0), F(0.1), F(0.6), F(1.0) - F(2.0 ** -24)]
    return sorted({float(x) for x in xs if 0 <= x < 1})


def sample_records(p):
    """(wi [n][3], s [n][2]) for opacity p: every direction with every s.x of sample_x(p), s.y from two values"""
    wi, xs, ys = directions(), sample_x(p), [F(0.15), F(0.7)]
    rec = [(w, (x, y)) for w in wi for x in xs for y in ys]
    return np.float32([r[0] for r in rec]), np.float32([r[1] for r in rec])


def eval_records():
    """(wi [n][3], wo [n][3]): every direction with every outgoing direction"""
    rec = [(w, o) for w in directions() for o in outgoing()]
    return np.float32([r[0] for r in rec]), np.float32([r[1] for r in rec])


def planted_undefined(p, s):
    """the records whose inputs are p == 0 and s.x == 0: the reference divides 0 by 0 there"""
    return (F(p) == 0) & (np.asarray(s, dtype=np.float32).reshape(-1, 2)[:, 0] == 0)
