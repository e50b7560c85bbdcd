"""A binary64 restatement of the stage that starts every path: the configuration of the perspective and the orthographic
camera and their generateRay.  Written from the reference's sources, not from csrc/ or oracle/:
    Transform::operator*, translate, scale           src/libcore/transform.cpp:28-63
    Transform::perspective, orthographic, lookAt     src/libcore/transform.cpp:100-124, :155-158, :174-190
    Matrix::invert (Gauss-Jordan, full pivoting)     include/mitsuba/core/matrix.inl:140-195
    degToRad                                         include/mitsuba/core/util.h:302
    ProjectiveCamera / PerspectiveCamera defaults    src/librender/camera.cpp:119-124, :142, :155-167
    PerspectiveCameraImpl::configure, generateRay    src/cameras/perspective.cpp:43-71, :77-112
    OrthographicCamera::configure, generateRay       src/cameras/orthographic.cpp:55-86, :104-119
    Transform::operator()(Point), (Vector), (Ray)    include/mitsuba/core/transform.h:133-149, :163-170, :219-235
    squareToDiskConcentric                           src/libcore/util.cpp:628-650
    the camera sample of SampleIntegrator::renderBlock   src/librender/integrator.cpp:151-164
Conventions of tests/ref64_sky.py: float32 inputs promoted exactly, every quantity a pair (value, err) of its class E -- the
value in binary64, err a first-order bound, in units of 2^-23, of the absolute error of a binary32 evaluation in the
reference's operation order.  A rounded operation adds half a unit of its result; sums, products and quotients carry their
operands' errors on by the derivatives; a libm call (tan, sin, cos) is granted one ulp and adds a whole unit, as in
tests/ref64_film.py.  Operations that binary32 performs exactly whatever the other operand -- times 0, times +-1, plus 0,
1 / +-1, which is most of what a product of scales and translations consists of -- add nothing; operations that merely happen
to be exact (times 2, times 0.5) are charged like any other.  There is no factor on top of the bound.  Test infrastructure.

Form A (configure): the matrices as the reference builds them.  screenToRaster is a product of two scales and a translation
whose inverses are written down, not computed (transform.cpp:33-63), Transform(trafo) of the perspective matrix inverts it
with Matrix::invert, and rasterToCamera = cameraToScreen^-1 * screenToRaster^-1 is two chains of 4 x 4 products; every one of
these operations is restated on E, so each of the 32 entries of rasterToCamera and cameraToWorld carries the bound of its own
chain (an entry that is zero by construction has bound 0 and must be equal).  m_aspect and both getSize() are the FULL film's
(camera.cpp:142, film.cpp:33-41): a crop window only moves the rectangle that is rendered.  The orthographic camera's
cameraToWorld is lookAt * scale(sx, sy, 1), the transform its plugin is given.

Form B (no matrices): the same camera from its geometry.  right = normalize(dir x up), newUp = right x dir; the film's
smaller side spans tan(fov / 2) either way of the axis, pixels are square, raster y grows downwards:
    x_s = (sx - W/2) * 2 / min(W, H),   y_s = -(sy - H/2) * 2 / min(W, H),
    perspective   d = normalize(dir + tan(fov/2) * (x_s right + y_s newUp)),   o = p
    orthographic  o = p + scaleX x_s right + scaleY y_s newUp + near dir,      d = dir.
Forms A and B must agree to AGREE = 1e-12 (relative to |d| = 1 and to max(1, |o|)); B is what catches a misreading of the
matrix code that A would copy.

generateRay: restated on E from form A's matrices WITH their bounds, so the bound of a ray value covers the binary32
configuration as well as the binary32 ray, and the truth does not pass through the product's or the oracle's matrices.
Branches -- w != 1 of the two point transforms, the four regions and the centre of the concentric map -- are taken in
binary64 here and in binary32 by `mirror`.  Where the two differ the value is still the binary64 branch's, and the bound
becomes the larger of the two branches' bounds plus the distance between the two branches' values: the concentric map is
continuous across its region borders, so that distance is of the order of the rounding that flipped the branch.  Nothing is
excluded; `differ` merely counts.

mirror: generateRay in numpy float32, one operation and one rounding per step in the reference's order, the sine and cosine
supplied by the caller (the project's sincos is the oracle's orc_sinf / orc_cosf).  The oracle's and the device's rows must
equal it bit for bit.

Mutations: `mutate` alters the restatement in one place (MUTATIONS); the tests show that each altered restatement disagrees
with the rows beyond the unchanged bound on at least one case, which is what shows that the bound discriminates.

Properties: `properties` states what a camera ray must satisfy whatever the formulas -- unit direction, end points on the
near and far planes of the lookAt frame, a pinhole origin at the camera position, a thin lens whose rays meet in one point
of the focal plane and leave the lens plane inside the aperture.  Each residual is compared with the first-order image of
the values' bounds (the larger one-sided difference of the residual over each value's bound, summed), plus PROP_SLACK of the
residual's scale for the binary64 evaluation itself."""
import numpy as np

from ref64 import EPS32
from ref64_sky import E, _sqrt, PI32

F = np.float32
NEAR, FAR = float(F(1e-2)), float(F(1e4))                   # camera.cpp:121-123
AGREE = 1e-12
PROP_SLACK = 1e-12
MUTATIONS = ("fov_larger_side", "aspect_branch_swapped", "y_not_flipped", "x_mirrored", "full_angle", "crop_aspect",
             "crop_offset_dropped", "border_offset_dropped", "near_far_exchanged", "invz_omitted", "focal_along_ray",
             "lens_raster_exchanged", "disk_regions_exchanged", "aperture_not_scaled", "ortho_maxt_far", "ortho_origin_no_scale")


def _f64(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def _lib(v, e):
    return E(v, e + np.abs(v))                               # a libm result: within one ulp


def _sin(a):
    return _lib(np.sin(a.v), np.abs(np.cos(a.v)) * a.e)


def _cos(a):
    return _lib(np.cos(a.v), np.abs(np.sin(a.v)) * a.e)


def _tan(a):
    t = np.tan(a.v)
    return _lib(t, (1 + t * t) * a.e)


# --- vectors and matrices of E ---------------------------------------------------------------------------------------------
def _is(x, value):
    """x is exactly `value` everywhere, with no error of its own"""
    return bool(np.all(x.e == 0) and np.all(x.v == value))


def _m(a, b):
    """a * b; times 0 and times +-1 are exact in binary32 whatever the other operand and add nothing"""
    for x, y in ((a, b), (b, a)):
        if _is(x, 0.0):
            return E(np.zeros(np.broadcast(a.v, b.v).shape))
        if _is(x, 1.0):
            return E(y.v + np.zeros_like(x.v), y.e + np.zeros_like(x.v))
        if _is(x, -1.0):
            return E(-y.v + np.zeros_like(x.v), y.e + np.zeros_like(x.v))
    return a * b


def _a(a, b):
    """a + b; plus 0 is exact"""
    for x, y in ((a, b), (b, a)):
        if _is(x, 0.0):
            return E(y.v + np.zeros_like(x.v), y.e + np.zeros_like(x.v))
    return a + b


def _s(a, b):
    return _a(a, -b)


def _inv(a):
    """1 / a; 1 / +-1 is exact"""
    return a if _is(a, 1.0) or _is(a, -1.0) else 1.0 / a


def _cross(a, b):                                            # vector.h cross
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _length(v):
    return _sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _normalize(v):                                           # v / length == v * (1 / length) (vector.h)
    recip = 1.0 / _length(v)
    return [x * recip for x in v]


def _mat(rows):
    return [[x if isinstance(x, E) else E(float(x)) for x in r] for r in rows]


def _mul(a, b):                                              # Matrix * Matrix: sum = 0; sum += a[i][k] * b[k][j]
    out = []
    for i in range(4):
        row = []
        for j in range(4):
            s = E(0.0)
            for k in range(4):
                s = _a(s, _m(a[i][k], b[k][j]))
            row.append(s)
        out.append(row)
    return out


def _invert(src):
    """Matrix::invert (matrix.inl:140-195) on E; the pivots are chosen on the binary64 values"""
    t = [list(r) for r in src]
    ipiv, indxr, indxc = [0] * 4, [], []
    for _ in range(4):
        big, irow, icol = 0.0, -1, -1
        for j in range(4):
            if ipiv[j] == 1:
                continue
            for k in range(4):
                if ipiv[k] == 0 and abs(float(t[j][k].v)) >= big:
                    big, irow, icol = abs(float(t[j][k].v)), j, k
        ipiv[icol] += 1
        if irow != icol:
            t[irow], t[icol] = t[icol], t[irow]
        indxr.append(irow); indxc.append(icol)
        if float(t[icol][icol].v) == 0:
            raise ValueError("singular matrix")
        pivinv = _inv(t[icol][icol])
        t[icol][icol] = E(1.0)
        t[icol] = [_m(x, pivinv) for x in t[icol]]
        for j in range(4):
            if j == icol:
                continue
            save = t[j][icol]
            t[j][icol] = E(0.0)
            t[j] = [_s(t[j][k], _m(t[icol][k], save)) for k in range(4)]
    for j in (3, 2, 1, 0):
        if indxr[j] != indxc[j]:
            for k in range(4):
                t[k][indxr[j]], t[k][indxc[j]] = t[k][indxc[j]], t[k][indxr[j]]
    return t


def _scale_inv(x, y, z):                                     # transform.cpp:56-61
    return _mat([[_inv(x), 0, 0, 0], [0, _inv(y), 0, 0], [0, 0, _inv(z), 0], [0, 0, 0, 1]])


def _translate_inv(x, y, z):                                 # transform.cpp:40-45
    return _mat([[1, 0, 0, -x], [0, 1, 0, -y], [0, 0, 1, -z], [0, 0, 0, 1]])


def _point(M, x, y, z):                                      # transform.h:133-141, the four sums
    return [_a(_a(_a(_m(M[i][0], x), _m(M[i][1], y)), _m(M[i][2], z)), M[i][3]) for i in range(4)]


def _vector(M, x, y, z):                                     # transform.h:163-170
    return [_a(_a(_m(M[i][0], x), _m(M[i][1], y)), _m(M[i][2], z)) for i in range(3)]


# --- configure, form A -------------------------------------------------------------------------------------------------------
class Camera:
    """kind 0 perspective, 1 orthographic; r2c, c2w: 4 x 4 of E; frame = (p, right, newUp, dir) in binary64"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def values(self, which):
        return np.array([[float(x.v) for x in r] for r in getattr(self, which)])

    def bounds(self, which):
        return np.array([[float(x.e) for x in r] for r in getattr(self, which)]) * EPS32


def _look_at(origin, target, up):                            # transform.cpp:174-190
    p = [E(x) for x in _f64(origin)]; t = [E(x) for x in _f64(target)]; u = [E(x) for x in _f64(up)]
    dirct = _normalize([t[i] - p[i] for i in range(3)])
    right = _normalize(_cross(dirct, u))
    new_up = _cross(right, dirct)
    M = _mat([[right[0], new_up[0], dirct[0], p[0]], [right[1], new_up[1], dirct[1], p[1]],
              [right[2], new_up[2], dirct[2], p[2]], [0, 0, 0, 1]])
    return M


def _raster_to_screen(width, height, mutate):
    """screenToRaster.inverse() of perspective.cpp:52-63 / orthographic.cpp:59-78, mapSmallerSide = true"""
    aspect = E(float(width)) / E(float(height))              # camera.cpp:142
    if mutate == "aspect_branch_swapped":
        aspect = E(float(height)) / E(float(width))
    first = bool(F(aspect.v) >= F(1.0))
    if mutate == "fov_larger_side":
        first = not first
    if first:
        s2, tr = [1.0 / (2.0 * aspect), E(-0.5), E(1.0)], [aspect, E(-1.0), E(0.0)]
    else:
        s2, tr = [E(0.5), -0.5 * aspect, E(1.0)], [E(1.0), -(1.0 / aspect), E(0.0)]
    if mutate == "y_not_flipped":
        s2[1], tr[1] = -s2[1], -tr[1]
    if mutate == "x_mirrored":
        s2[0], tr[0] = -s2[0], -tr[0]
    # (scale(size) * scale(s2)) * translate(tr): the inverses multiply the other way round (transform.cpp:28-31)
    inv = _mul(_scale_inv(*s2), _scale_inv(E(float(width)), E(float(height)), E(1.0)))
    return _mul(_translate_inv(*tr), inv)


def _frame(desc):
    p, t, u = _f64(desc["origin"]), _f64(desc["target"]), _f64(desc["up"])
    d = (t - p) / np.linalg.norm(t - p)
    r = np.cross(d, u); r /= np.linalg.norm(r)
    return p, r, np.cross(r, d), d


def configure(desc, film, crop=None, mutate=None):
    """desc: origin, target, up and fov (degrees) or ortho_scale (sx, sy); optional aperture, focus.  film = (W, H) of the
    full film, crop = (x, y, w, h) or None"""
    W, H = film
    if mutate == "crop_aspect" and crop is not None:
        W, H = crop[2], crop[3]
    near, far = E(NEAR), E(FAR)
    r2s = _raster_to_screen(W, H, mutate)
    look = _look_at(desc["origin"], desc["target"], desc["up"])
    if "ortho_scale" in desc:
        sx, sy = (float(F(v)) for v in desc["ortho_scale"])
        scale = _mat([[sx, 0, 0, 0], [0, sy, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        c2w = look if mutate == "ortho_origin_no_scale" else _mul(look, scale)
        # Transform::orthographic = scale(1, 1, 1 / (far - near)) * translate(0, 0, -near)
        c2s_inv = _mul(_translate_inv(E(0.0), E(0.0), -near), _scale_inv(E(1.0), E(1.0), 1.0 / (far - near)))
        return Camera(kind=1, r2c=_mul(c2s_inv, r2s), c2w=c2w, near=near, far=far, aperture=0.0, focus=FAR, frame=_frame(desc),
                      desc=desc, film=film)
    fov = E(float(F(desc["fov"])))
    recip = 1.0 / (far - near)                               # transform.cpp:110-117
    trafo = _mat([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, far * recip, (-near) * far * recip], [0, 0, 1, 0]])
    half = fov if mutate == "full_angle" else fov / 2.0
    cot = 1.0 / _tan(half * (E(PI32) / 180.0))               # degToRad (util.h:302)
    c2s_inv = _mul(_invert(trafo), _scale_inv(cot, cot, E(1.0)))
    aperture = float(F(desc.get("aperture", 0.0)))
    focus = float(F(desc["focus"])) if desc.get("focus") is not None else FAR     # camera.cpp:164
    return Camera(kind=0, r2c=_mul(c2s_inv, r2s), c2w=look, near=near, far=far, aperture=aperture, focus=focus,
                  frame=_frame(desc), desc=desc, film=film)


def check_configure(cam, c32):
    """the product's mtsgpu_camera against form A: worst |error| / bound over the 32 matrix entries (inf for an entry that
    must be exact and is not, or for a wrong scalar field)"""
    worst = 0.0
    for which, got in (("r2c", c32.raster_to_camera), ("c2w", c32.camera_to_world)):
        g = np.array(list(got), dtype=np.float64).reshape(4, 4)
        err, b = np.abs(g - cam.values(which)), cam.bounds(which)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf))
        worst = max(worst, float(r.max()))
    ok = (c32.near_clip == F(NEAR) and c32.far_clip == F(FAR) and c32.kind == cam.kind
          and F(c32.aperture_radius) == F(cam.aperture) and F(c32.focus_depth) == F(cam.focus))
    return worst if ok else np.inf


# --- configure, form B -------------------------------------------------------------------------------------------------------
def form_b(desc, film, raster):
    """(origin [n][3], direction [n][3]) of the ray through raster positions [n][2], from the geometry alone"""
    p, right, new_up, d = _frame(desc)
    W, H = film
    r = np.asarray(raster, dtype=np.float64)
    xs = (r[:, 0] - W / 2.0) * 2.0 / min(W, H)
    ys = -(r[:, 1] - H / 2.0) * 2.0 / min(W, H)
    if "ortho_scale" in desc:
        sx, sy = (float(F(v)) for v in desc["ortho_scale"])
        o = p + np.outer(sx * xs, right) + np.outer(sy * ys, new_up) + NEAR * d
        return o, np.tile(d, (len(r), 1))
    t = np.tan(float(F(desc["fov"])) / 2.0 * (PI32 / 180.0))
    v = d + np.outer(t * xs, right) + np.outer(t * ys, new_up)
    return np.tile(p, (len(r), 1)), v / np.linalg.norm(v, axis=1, keepdims=True)


def form_a(cam, raster):
    """the same from form A's matrices, in binary64 throughout"""
    m, w = cam.values("r2c"), cam.values("c2w")
    r = np.asarray(raster, dtype=np.float64)
    h = np.concatenate([r, np.zeros((len(r), 1)), np.ones((len(r), 1))], axis=1) @ m.T
    ic = h[:, :3] / h[:, 3:4]
    if cam.kind == 1:
        o = ic @ w[:3, :3].T + w[:3, 3]
        return o, np.tile(w[:3, 2], (len(r), 1))
    d = ic / np.linalg.norm(ic, axis=1, keepdims=True)
    return np.tile(w[:3, 3], (len(r), 1)), d @ w[:3, :3].T


def forms_disagreement(cam, raster):
    oa, da = form_a(cam, raster)
    ob, db = form_b(cam.desc, cam.film, raster)
    return max(float(np.abs(da - db).max()), float((np.abs(oa - ob).max(axis=1) / np.maximum(1.0, np.abs(ob).max(axis=1))).max()))


# --- the camera sample (integrator.cpp:151-164) ---------------------------------------------------------------------------------
def camera_samples(pixels, crop_xy, border, draws, thin_lens, mutate=None):
    """pixels [n][2]: pixel of the crop window, from -border with highQualityEdges; draws [n][2][2] float32: the sampler's first
    and second next2D().  Returns (raster [n][2], lens [n][2]) in float32: the lens sample is drawn first, and the raster
    position is the second draw plus the pixel's coordinates in the full film"""
    px = np.asarray(pixels, dtype=np.int64).copy()
    if mutate != "crop_offset_dropped":
        px += np.asarray(crop_xy, dtype=np.int64)
    if mutate == "border_offset_dropped":
        px += border
    d = np.asarray(draws, dtype=F)
    first, second = d[:, 0], d[:, 1]
    if thin_lens and mutate == "lens_raster_exchanged":
        first, second = second, first
    lens, u = (first, second) if thin_lens else (np.zeros_like(first), first)
    return (u + px.astype(F)).astype(F), lens.astype(F)


# --- generateRay ----------------------------------------------------------------------------------------------------------------
def _disk_region(r1, r2):
    """0 the centre, 1..4 the regions of util.cpp:633-645"""
    with np.errstate(invalid="ignore"):
        return np.where((r1 == 0) & (r2 == 0), 0, np.where(r1 > -r2, np.where(r1 > r2, 1, 2), np.where(r1 < r2, 3, 4)))


def _choose(idx, items):
    return E(np.choose(idx, [x.v for x in items]), np.choose(idx, [x.e for x in items]))


def _either(idx64, idx32, items):
    """items[idx64], its bound widened where binary32 took items[idx32] (see the module's text)"""
    a, b = _choose(idx64, items), _choose(idx32, items)
    differ = idx64 != idx32
    with np.errstate(invalid="ignore"):
        return E(a.v, np.where(differ, np.maximum(a.e, b.e) + np.abs(a.v - b.v) / EPS32, a.e)), int(differ.sum())


def _disk(lens, region32, mutate):
    """squareToDiskConcentric (util.cpp:628-650)"""
    sx, sy = E(_f64(lens[:, 0])), E(_f64(lens[:, 1]))
    r1, r2 = 2.0 * sx - 1.0, 2.0 * sy - 1.0
    q = E(PI32) / 4.0

    def polar(r, phi):
        return [r * _cos(phi), r * _sin(phi)]

    zero = E(np.zeros_like(r1.v))
    with np.errstate(all="ignore"):
        regions = [[zero, zero], polar(r1, q * r2 / r1), polar(r2, q * (2.0 - r1 / r2)),
                   polar(-r1, q * (4.0 + r2 / r1)), polar(-r2, q * (6.0 - r1 / r2))]
    if mutate == "disk_regions_exchanged":
        regions[1], regions[2] = regions[2], regions[1]
    region64 = _disk_region(r1.v, r2.v)
    x, nx = _either(region64, region32, [r[0] for r in regions])
    y, _ = _either(region64, region32, [r[1] for r in regions])
    return [x, y], nx


def generate(cam, branches32, raster, lens, mutate=None):
    """rows o.xyz, mint, d.xyz, maxt for float32 raster positions and lens samples [n][2]: (values [n][8], bounds [n][8] as
    absolute errors, differ = how many branches binary32 (branches32, from mirror) took the other way)"""
    raster = np.asarray(raster, dtype=F); lens = np.asarray(lens, dtype=F)
    n = len(raster)
    zero, one = E(np.zeros(n)), E(np.ones(n))
    differ = 0
    with np.errstate(all="ignore"):
        h = _point(cam.r2c, E(_f64(raster[:, 0])), E(_f64(raster[:, 1])), zero)
        recip = 1.0 / h[3]
        w64 = (h[3].v != 1.0).astype(int)
        ic = []
        for i in range(3):
            v, k = _either(w64, branches32["w"].astype(int), [h[i], h[i] * recip]); ic.append(v); differ += k if i == 0 else 0
        if cam.kind == 1:
            lo, ld = ic, [zero, zero, one]
            mint, maxt = zero, _a(cam.far if mutate == "ortho_maxt_far" else cam.far - cam.near, zero)
        else:
            lo = [zero, zero, zero]
            if cam.aperture > 0:
                lp, k = _disk(lens, branches32["disk"], mutate); differ += k
                if mutate != "aperture_not_scaled":
                    lp = [x * cam.aperture for x in lp]
                tf = cam.focus / (_length(ic) if mutate == "focal_along_ray" else ic[2])
                focal = [_a(zero, tf * x) for x in ic]       # localRay(t) = o + t * d with o = 0
                lo = [_a(zero, lp[0]), _a(zero, lp[1]), zero]
                ic = [_s(focal[i], lo[i]) for i in range(3)]
            ld = _normalize(ic)
            inv_z = 1.0 / ld[2]
            if mutate == "invz_omitted":
                inv_z = one
            mint, maxt = cam.near * inv_z, cam.far * inv_z
            if mutate == "near_far_exchanged":
                mint, maxt = maxt, mint
        g = _point(cam.c2w, lo[0], lo[1], lo[2])
        recip = 1.0 / g[3]
        ow64 = (g[3].v != 1.0).astype(int)
        o = []
        for i in range(3):
            v, k = _either(ow64, branches32["ow"].astype(int), [g[i], g[i] * recip]); o.append(v); differ += k if i == 0 else 0
        d = _vector(cam.c2w, ld[0], ld[1], ld[2])
    cols = o + [mint] + d + [maxt]
    val = np.stack([c.v + np.zeros(n) for c in cols], axis=1)
    bnd = np.stack([c.e + np.zeros(n) for c in cols], axis=1) * EPS32
    return val, bnd, differ


def ratio(rows, val, bnd):
    """|rows - val| / bnd per value; inf for a non-finite value or an error where the bound is 0"""
    g = np.asarray(rows, dtype=np.float64)[:, :8]
    err = np.abs(g - val)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(bnd > 0, err / bnd, np.where(err == 0, 0.0, np.inf))
    return np.where(np.isfinite(g) & np.isfinite(val), r, np.inf)


def check(cam, rows, branches32, raster, lens, mutate=None):
    """the shared check of a set of rows (layout of mtsgpu_camera_rays) whose samples should be (raster, lens): worst
    |error| / bound (inf where a row's raster position is not the expected one, bit for bit) and the branch count"""
    rows = np.asarray(rows, dtype=F)
    val, bnd, differ = generate(cam, branches32, raster, lens, mutate)
    r = ratio(rows, val, bnd)
    same = (np.ascontiguousarray(rows[:, 8:10]).view(np.uint32) == np.ascontiguousarray(raster, dtype=F).view(np.uint32)).all(axis=1)
    worst = float(r.max()) if same.all() else np.inf
    return worst, differ


# --- the binary32 mirror -----------------------------------------------------------------------------------------------------------
def mirror(c32, raster, lens, sincos):
    """generateRay in float32 for an mtsgpu_camera structure; sincos(a float32 array) -> (sin, cos) float32 arrays.  Returns
    (rows [n][8] float32, the branches taken)"""
    m = np.array(list(c32.raster_to_camera), dtype=F).reshape(4, 4)
    w = np.array(list(c32.camera_to_world), dtype=F).reshape(4, 4)
    raster = np.asarray(raster, dtype=F); lens = np.asarray(lens, dtype=F)
    n = len(raster)
    sx, sy, z0 = raster[:, 0], raster[:, 1], np.zeros(n, dtype=F)
    near, far = F(c32.near_clip), F(c32.far_clip)
    one = F(1.0)
    with np.errstate(all="ignore"):
        h = [((m[i, 0] * sx + m[i, 1] * sy) + m[i, 2] * z0) + m[i, 3] for i in range(4)]
        bw = h[3] != one
        recip = one / h[3]
        ic = [np.where(bw, h[i] * recip, h[i]) for i in range(3)]
        region = np.zeros(n, dtype=int)
        if c32.kind == 1:
            lo, ld = ic, [z0, z0, np.ones(n, dtype=F)]
            mint, maxt = z0, np.full(n, far - near, dtype=F)
        else:
            lo = [z0, z0, z0]
            if c32.aperture_radius > 0:
                r1, r2 = F(2.0) * lens[:, 0] - one, F(2.0) * lens[:, 1] - one
                region = _disk_region(r1, r2)
                q = F(PI32) / F(4.0)
                cx = np.choose(region, [z0, r1, r2, -r1, -r2])
                cy = np.choose(region, [z0, q * r2 / r1, q * (F(2.0) - r1 / r2), q * (F(4.0) + r2 / r1), q * (F(6.0) - r1 / r2)])
                s, c = sincos(cy.astype(F))
                ap = F(c32.aperture_radius)
                lpx, lpy = (cx * c) * ap, (cx * s) * ap
                tf = F(c32.focus_depth) / ic[2]
                focal = [F(0.0) + tf * x for x in ic]
                lo = [F(0.0) + lpx, F(0.0) + lpy, z0]
                ic = [focal[i] - lo[i] for i in range(3)]
            length = np.sqrt((ic[0] * ic[0] + ic[1] * ic[1]) + ic[2] * ic[2])
            rl = one / length
            ld = [x * rl for x in ic]
            inv_z = one / ld[2]
            mint, maxt = near * inv_z, far * inv_z
        g = [((w[i, 0] * lo[0] + w[i, 1] * lo[1]) + w[i, 2] * lo[2]) + w[i, 3] for i in range(4)]
        bo = g[3] != one
        recip = one / g[3]
        o = [np.where(bo, g[i] * recip, g[i]) for i in range(3)]
        d = [(w[i, 0] * ld[0] + w[i, 1] * ld[1]) + w[i, 2] * ld[2] for i in range(3)]
    rows = np.stack([np.broadcast_to(c, (n,)).astype(F) for c in o + [mint] + d + [maxt]], axis=1)
    return rows, dict(w=np.broadcast_to(bw, (n,)), ow=np.broadcast_to(bo, (n,)), disk=region)


# --- geometric properties ------------------------------------------------------------------------------------------------------
def _residuals(cam, x, lens):
    """residuals [n][k] of rows x [n][8] (binary64), each 0 for a perfect ray, and their scales [n][k]"""
    p, right, new_up, dirv = cam.frame
    o, mint, d, maxt = x[:, 0:3], x[:, 3], x[:, 4:7], x[:, 7]
    near_end, far_end = o + mint[:, None] * d, o + maxt[:, None] * d
    depth = lambda q: (q - p) @ dirv
    res = [np.linalg.norm(d, axis=1) - 1.0, depth(near_end) - NEAR, depth(far_end) - FAR]
    scale = [np.ones(len(x)), np.maximum(1.0, np.abs(near_end).max(axis=1)), np.maximum(FAR, np.abs(far_end).max(axis=1))]
    if cam.kind == 0:
        off = o - p
        ox, oy = off @ right, off @ new_up
        s = np.maximum(1.0, np.abs(o).max(axis=1))
        res.append(depth(o)); scale.append(s)                 # pinhole: o == p; thin lens: o in the lens plane
        if cam.aperture == 0:
            res += [ox, oy]; scale += [s, s]
        else:
            l = np.asarray(lens, dtype=np.float64)
            edge = (np.minimum(l[:, 0], l[:, 1]) == 0.0) | (np.maximum(l[:, 0], l[:, 1]) == 1.0)
            centre = (l[:, 0] == 0.5) & (l[:, 1] == 0.5)
            radius = np.sqrt(ox ** 2 + oy ** 2)
            # inside the aperture; exactly on its rim for a lens sample on the square's edge, on the axis for its centre
            res += [np.where(edge, radius - cam.aperture, np.where(centre, 0.0, np.maximum(radius - cam.aperture, 0.0))),
                    np.where(centre, ox, 0.0), np.where(centre, oy, 0.0)]
            scale += [s, s, s]
    return np.stack(res, axis=1), np.stack(scale, axis=1)


def _focal_points(cam, x):
    """where each ray crosses the plane at camera depth focusDepth"""
    p, _, _, dirv = cam.frame
    o, d = x[:, 0:3], x[:, 4:7]
    t = (cam.focus - (o - p) @ dirv) / (d @ dirv)
    return o + t[:, None] * d


def properties(cam, rows, bnd, raster, lens):
    """worst residual / allowance over the properties of the module's text.  rows [n][8]; bnd their bounds (generate); for a
    thin lens the rays of one raster position must meet the pinhole ray of form B in the focal plane"""
    x = np.asarray(rows, dtype=np.float64)[:, :8]

    def allowance(fn, base):
        a = np.zeros_like(base)
        for k in range(8):
            dx = np.zeros_like(x); dx[:, k] = bnd[:, k]
            a += np.maximum(np.abs(fn(x + dx) - base), np.abs(fn(x - dx) - base))
        return a

    res, scale = _residuals(cam, x, lens)
    allow = allowance(lambda y: _residuals(cam, y, lens)[0], res) + PROP_SLACK * scale
    worst = float((np.abs(res) / allow).max())
    if cam.kind == 0 and cam.aperture > 0:
        _, db = form_b(cam.desc, cam.film, raster)
        p, _, _, dirv = cam.frame
        target = p + (cam.focus / (db @ dirv))[:, None] * db
        f = _focal_points(cam, x)
        allow = allowance(lambda y: _focal_points(cam, y), f) + PROP_SLACK * np.maximum(1.0, np.abs(target))
        # the raster position is a float32 given exactly, so form B's target carries no bound of its own
        worst = max(worst, float((np.abs(f - target) / allow).max()))
    return worst
