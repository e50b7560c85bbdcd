"""The shared inputs of tests/test_camera_truth.py (oracle, CPU) and tests/test_gpu_camera_truth.py (device): cameras, raster
and lens samples, and the glue between a case and the product's / the oracle's camera structure.  Small on purpose."""
import numpy as np

import ref64_camera as rc

F = np.float32
FILMS = ((40, 28), (28, 40), (32, 32))                       # both aspect branches and the tie
FOVS = (1.0, 45.0, 170.0)
POSES = {
    "axis": dict(origin=(0.0, 1.0, 3.4), target=(0.0, 1.0, 0.0), up=(0.0, 1.0, 0.0)),
    # the origin near 1e3: target - origin cancels three digits, and the translation column dwarfs the rotation
    "oblique": dict(origin=(1000.3, 997.1, -1003.7), target=(998.9, 996.2, -1001.1), up=(0.1, 1.0, 0.2)),
    # straight down, `up` perpendicular to the view
    "down": dict(origin=(0.3, 5.0, -0.2), target=(0.3, 0.0, -0.2), up=(0.0, 0.0, 1.0)),
}
ORTHO_SCALES = ((1.1, 1.1), (0.3, 2.0))
THIN_LENSES = (dict(aperture=0.04, focus=3.3), dict(aperture=0.5))      # the second: focusDepth = farClip by default
CROP_FILM, CROP = (64, 48), (5, 3, 42, 28)
BORDER = 2                                                   # the gaussian filter's (ceil(2 - 0.5), renderproc.cpp:143-144)
SAMPLERS = ("independent", "ldsampler", "halton", "hammersley", "stratified")
RECORD_COUNTS = (1, 63, 64, 65, 255, 257, 1000)              # a lone lane, a ragged wave, a ragged block of k_generate
SEED = 0x5EED


def _case(family, name, desc, film, crop=None, border=0):
    return dict(family=family, name=name, desc=desc, film=film, crop=crop, border=border)


def cases(family=None):
    out = []
    for pn, pose in POSES.items():
        for film in FILMS:
            for fov in FOVS:
                out.append(_case("perspective", "%s %dx%d fov %g" % (pn, film[0], film[1], fov), dict(pose, fov=fov), film))
            for s in ORTHO_SCALES:
                out.append(_case("ortho", "%s %dx%d scale %g,%g" % (pn, film[0], film[1], s[0], s[1]), dict(pose, ortho_scale=s), film))
    for k, lens in enumerate(THIN_LENSES):
        for pn, film, fov in (("axis", (40, 28), 45.0), ("oblique", (28, 40), 45.0), ("down", (32, 32), 170.0), ("axis", (28, 40), 1.0)):
            out.append(_case("thinlens", "lens %d %s %dx%d fov %g" % (k, pn, film[0], film[1], fov), dict(POSES[pn], fov=fov, **lens), film))
    for pn, fov, lens in (("axis", 45.0, {}), ("oblique", 170.0, {}), ("down", 45.0, THIN_LENSES[0])):
        out.append(_case("crop", "crop %s fov %g%s" % (pn, fov, " lens" if lens else ""), dict(POSES[pn], fov=fov, **lens), CROP_FILM, crop=CROP))
    out.append(_case("border", "border axis 40x28", dict(POSES["axis"], fov=45.0), (40, 28), border=BORDER))
    out.append(_case("border", "border ortho 28x40", dict(POSES["down"], ortho_scale=ORTHO_SCALES[1]), (28, 40), border=BORDER))
    out.append(_case("border", "border crop lens", dict(POSES["oblique"], fov=45.0, **THIN_LENSES[0]), CROP_FILM, crop=CROP, border=BORDER))
    return [c for c in out if family is None or c["family"] == family]


FAMILIES = ("perspective", "ortho", "thinlens", "crop", "border")


class _Desc:
    def __init__(self, camera):
        self.camera = camera


def size(c):
    """the rendered window without its border"""
    return (c["crop"][2], c["crop"][3]) if c["crop"] else c["film"]


def offset(c):
    return (c["crop"][0], c["crop"][1]) if c["crop"] else (0, 0)


def key_of(c, pix):
    """the library's pixel key of pixels [n][2] of the crop window (include/mtsgpu.h, mtsgpu_pass_samples): the index of the
    raster pixel in the full film grown by the border"""
    p = np.asarray(pix, dtype=np.int64) + np.array(offset(c)) + c["border"]
    return (p[:, 1] * (c["film"][0] + 2 * c["border"]) + p[:, 0]).astype(np.uint32)


def product_camera(mts, c):
    """the product's camera object for the case (mtsgpu_make_camera, _crop or _ortho)"""
    d = _Desc(c["desc"])
    if not c["crop"]:
        return mts.PerspectiveCamera.for_description(d, c["film"][0], c["film"][1])
    cam = mts.PerspectiveCamera.cropped(d, c["film"][0], c["film"][1], c["crop"])
    if c["desc"].get("aperture", 0.0) > 0:
        cam.c.aperture_radius = c["desc"]["aperture"]
        cam.c.focus_depth = c["desc"].get("focus", cam.c.far_clip)
    return cam


def oracle_camera(orc, c):
    """the oracle's camera: raster space of the full film; camera_generate_ray reads nothing of the crop window"""
    return orc.make_camera(_Desc(c["desc"]), c["film"][0], c["film"][1])


def truth(c, mutate=None):
    return rc.configure(c["desc"], c["film"], c["crop"], mutate)


def thin(c):
    return c["desc"].get("aperture", 0.0) > 0 and "ortho_scale" not in c["desc"]


def ulp_neighbours(points):
    """every point, and the points one ulp either side of it in x and in y, inside [0, 1]"""
    p = np.asarray(points, dtype=F)
    out = [p]
    for axis in (0, 1):
        for to in (F(-1.0), F(2.0)):
            q = p.copy(); q[:, axis] = np.nextafter(q[:, axis], to)
            out.append(q)
    q = np.concatenate(out)
    return q[((q >= 0) & (q <= 1)).all(axis=1)]


def lens_samples():
    """the centre, the four edges and corners of the square, both diagonals of the concentric map (r1 = +-r2; below 0.25 the
    binary32 2 s - 1 rounds), one ulp either side of each, and a few arbitrary points"""
    base = [(0.5, 0.5), (0.0, 0.3), (1.0, 0.7), (0.3, 0.0), (0.6, 1.0), (0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0),
            (0.2, 0.2), (0.8, 0.8), (0.1, 0.1), (0.2, 0.8), (0.8, 0.2), (0.1, 0.9), (0.9, 0.1), (0.5, 0.25), (0.25, 0.5),
            (0.0625, 0.0625), (0.21, 0.21), (0.21, 0.79)]
    rnd = np.random.RandomState(7).rand(12, 2)
    return np.concatenate([ulp_neighbours(base), rnd.astype(F)])


def pixels_of(c, count, seed=1):
    """pixels [n][2] of the rendered window, border included: its corners, then arbitrary ones"""
    (w, h), b = size(c), c["border"]
    corners = [(-b, -b), (w + b - 1, -b), (-b, h + b - 1), (w + b - 1, h + b - 1), (0, 0), (w // 2, h // 2)]
    rng = np.random.RandomState(seed)
    rest = np.stack([rng.randint(-b, w + b, count), rng.randint(-b, h + b, count)], axis=1)
    return np.concatenate([np.array(corners), rest])[:max(count, 1)]


def direct_requests(c):
    """(pixels [n][2], draws [n][2][2]) for the direct checks: pixels of pixels_of with sub-pixel positions 0, 1 and arbitrary
    ones; with a thin lens, every lens sample of lens_samples() as the first draw, at several raster positions"""
    pix = pixels_of(c, 40)
    rng = np.random.RandomState(3)
    u = rng.rand(len(pix), 2).astype(F)
    u[:6] = [(0, 0), (1, 0), (0, 1), (1, 1), (0.5, 0.5), (0, 0)]
    draws = np.zeros((len(pix), 2, 2), dtype=F)
    if not thin(c):
        draws[:, 0] = u
        return pix, draws
    L = lens_samples()
    k = np.arange(len(L)) % len(pix)
    draws = np.zeros((len(L), 2, 2), dtype=F); draws[:, 0] = L; draws[:, 1] = u[k]
    return pix[k], draws


def samples_of(c, pix, draws, mutate=None):
    """(raster [n][2], lens [n][2]) float32 of the requests, by the restatement of integrator.cpp:151-164"""
    return rc.camera_samples(pix, offset(c), c["border"], draws, thin(c), mutate)


def direct_samples(c, mutate=None):
    return samples_of(c, *direct_requests(c), mutate=mutate)


def sincos_of(orc):
    """the project's sincos: the oracle's orc_sinf / orc_cosf"""
    L = orc.lib()

    def sincos(a):
        a = np.asarray(a, dtype=F)
        with np.errstate(all="ignore"):
            s = np.array([L.orc_sinf(float(x)) if np.isfinite(x) else np.nan for x in a], dtype=F)
            c = np.array([L.orc_cosf(float(x)) if np.isfinite(x) else np.nan for x in a], dtype=F)
        return s, c
    return sincos


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=F).view(np.uint32), np.ascontiguousarray(b, dtype=F).view(np.uint32))
