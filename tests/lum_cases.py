"""Small scenes, named input classes and the shared check that holds a luminaire read-out laid out like
mtsgpu_scene_lum_eval (the CPU suite hands in the oracle's, the GPU suite the device's) against tests/ref64_lum.py.
Test infrastructure.

Tolerances are the project's own (closed_forms.py): values and pdfs |got - ref| <= K_VALUE * 2^-23 * cond * |ref| + ATOL,
where cond * |ref| is the error bound ref64_lum derives; p, n, d componentwise K_DIR * 2^-23 * (their derived bound), which
for a position carries the magnitude of the operands it is summed from.  Ratios below are in units of 2^-23 x bound, so a
value passes up to K_VALUE = 16 and a vector up to K_DIR = 64.

Worst ratios of the ORACLE on the CPU, per class (tests/test_lum_truth.py prints them with -s), when this list was written:
see WORST_ORACLE at the end of this file."""
import numpy as np

import closed_forms as cf
import ref64_lum as R

F = np.float32
TOP = F(1 - 2.0 ** -24)
EPS = cf.EPS
# classes built to sit on a threshold: exempt from the ambiguity cap; every decidable-but-for-the-threshold record must
# match the restatement with the threshold taken one way or the other (ref64_lum's tie = -1 / +1)
THRESHOLD_MARK = " [threshold]"


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def _sphere_dirs(rng, n):
    v = rng.standard_normal((n, 3))
    return _unit(v)


def _steps(x):
    """x and the binary32 neighbours either side"""
    x = _f32(x)
    return np.nextafter(x, F(-np.inf)), x, np.nextafter(x, F(np.inf))


# ---------------------------------------------------------------------------------------------------------------------
# scenes
# ---------------------------------------------------------------------------------------------------------------------
def _strip_mesh():
    """20 triangles in the tilted plane y = 2 + 0.1 x, normal towards -y: ten squares of side 10^(-k/3), k = 9..0, side by
    side along x: areas span 1e6 : 1.  The smallest come first: their cells of the triangle cdf are a few binary32 steps wide,
    and s1 = 0 still lands in one exactly (a reused sample of 0 / width = 0), while s1 = 1 - 2^-24 lands in the largest."""
    pos, tri = [], []
    x = -1.0
    for k in range(9, -1, -1):
        w = 10.0 ** (-k / 3.0)
        b = len(pos)
        for (dx, dz) in ((0, 0), (w, 0), (w, w), (0, w)):
            pos.append((x + dx, 2.0 + 0.1 * (x + dx), dz))
        tri += [(b, b + 1, b + 2), (b, b + 2, b + 3)]            # cross(p1 - p0, p2 - p0) points to -y
        x += w
    return np.asarray(pos, dtype=np.float32), np.asarray(tri, dtype=np.uint32)


def _floor(sd, bsdf):
    pos = np.float32([[-3, 0, -3], [-3, 0, 3], [3, 0, 3], [3, 0, -3]])
    sd.add_mesh(pos, np.uint32([[0, 1, 2], [0, 2, 3]]), bsdf=bsdf, face_normals=True, name="floor")


def env_bitmap():
    """64 x 32 lat-long image: smooth positive gradients and one block of black texels, large enough (16 x 16, aligned) to
    leave cells of zero density on the level the sampling density is taken from"""
    y, x = np.mgrid[0:32, 0:64].astype(np.float64)
    img = np.stack([0.6 + 0.4 * np.sin(x / 64 * 2 * np.pi + 0.3) * np.cos(y / 32 * np.pi),
                    0.5 + 0.3 * np.cos(x / 64 * 4 * np.pi) + 0.01 * y,
                    0.2 + 0.02 * y + 0.1 * np.sin(x / 5.0) ** 2], axis=-1)
    img[8:24, 16:32] = 0.0
    img[4:6, 40:43] *= 30.0                                          # a bright patch
    return img.astype(np.float32)


def _rot(ax, ang):
    ax = _unit(ax)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return (np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K).astype(np.float32)


def scenes(mts):
    """[(name, SceneDescription)]: a handful of primitives each"""
    abi = mts.abi
    out = []

    def new(name):
        sd = mts.scenes.SceneDescription("lum " + name)
        sd.camera = dict(origin=(0.0, 1.0, 4.0), target=(0.0, 1.0, 0.0), up=(0.0, 1.0, 0.0), fov=40.0)
        out.append((name, sd))
        return sd, sd.lambertian(0.5), sd.lambertian(0.0)

    sd, grey, black = new("quad")
    _floor(sd, grey)
    pos, tri = mts.scenes._quad((-0.4, 2.0, -0.3), (0.8, 0, 0), (0, 0, 0.6), (0, -1, 0))
    sd.add_mesh(pos, tri, bsdf=black, lum=sd.add_lum(abi.LUM_AREA, [5.0, 4.0, 3.0]), face_normals=True, name="emitter")

    sd, grey, black = new("strip mesh")
    _floor(sd, grey)
    pos, tri = _strip_mesh()
    sd.add_mesh(pos, tri, bsdf=black, lum=sd.add_lum(abi.LUM_AREA, [2.0, 3.0, 4.0]), face_normals=True, name="emitter")

    sd, grey, black = new("strip mesh, vertex normals")
    _floor(sd, grey)
    pos, tri = _strip_mesh()
    rng = np.random.RandomState(5)
    nrm = _unit(np.array([0.1, -1.0, 0.0]) + 0.35 * rng.uniform(-1, 1, (len(pos), 3))).astype(np.float32)
    sd.add_mesh(pos, tri, bsdf=black, lum=sd.add_lum(abi.LUM_AREA, [2.0, 3.0, 4.0]), face_normals=False, normals=nrm, name="emitter")

    sd, grey, black = new("sliver")
    _floor(sd, grey)
    pos = np.float32([[-1.0, 2.0, 0.0], [1.0, 2.0, 1e-4], [1.0, 2.0, 0.0]])
    sd.add_mesh(pos, np.uint32([[0, 1, 2]]), bsdf=black, lum=sd.add_lum(abi.LUM_AREA, [9.0, 9.0, 9.0]), face_normals=True, name="emitter")

    sd, grey, black = new("sphere")
    _floor(sd, grey)
    sd.add_sphere((0.3, 1.5, -0.2), 0.5, bsdf=black, lum=sd.add_lum(abi.LUM_AREA, [7.0, 6.0, 5.0]))

    sd, grey, black = new("constant")
    _floor(sd, grey)
    sd.add_lum(abi.LUM_CONSTANT, [0.7, 0.8, 0.9])

    sd, grey, black = new("envmap")
    _floor(sd, grey)
    sd.envmap(env_bitmap(), 0.5, to_world=_rot([0.3, 1.0, 0.2], 0.8))

    sd, grey, black = new("two: sphere and point")
    _floor(sd, grey)
    sd.add_sphere((0.3, 1.5, -0.2), 0.5, bsdf=black, lum=sd.add_lum(abi.LUM_AREA, [7.0, 6.0, 5.0]))
    sd.point_light((-1.0, 2.0, 0.5), 3.0)

    sd, grey, black = new("five: quad, spot, sphere, point, envmap")
    _floor(sd, grey)
    pos, tri = mts.scenes._quad((-0.4, 2.0, -0.3), (0.8, 0, 0), (0, 0, 0.6), (0, -1, 0))
    sd.add_mesh(pos, tri, bsdf=black, lum=sd.add_lum(abi.LUM_AREA, [5.0, 4.0, 3.0]), face_normals=True, name="emitter")
    sd.spot_light((1.0, 2.5, 1.0), (0.0, 0.0, 0.0), 4.0, cutoff_deg=30.0)
    sd.add_sphere((-1.2, 1.0, -0.6), 0.3, bsdf=black, lum=sd.add_lum(abi.LUM_AREA, [7.0, 6.0, 5.0]))
    sd.point_light((-1.0, 2.0, 0.5), 3.0)
    sd.envmap(env_bitmap(), 0.5, to_world=_rot([0.3, 1.0, 0.2], 0.8))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
class Inputs:
    """records of one operation: arrays of equal length and classes {name: indices}"""

    def __init__(self):
        self.cols, self.classes, self.n = None, {}, 0

    def add(self, name, *cols):
        cols = [np.atleast_2d(_f32(c)) for c in cols]
        m = max(len(c) for c in cols)
        if min(len(c) for c in cols) == 0:
            return
        cols = [np.broadcast_to(c, (m, c.shape[1])).copy() for c in cols]
        if self.cols is None:
            self.cols = cols
        else:
            self.cols = [np.concatenate([a, b]) for a, b in zip(self.cols, cols)]
        self.classes[name] = np.arange(self.n, self.n + m)
        self.n += m


def _rand_s(rng, n):
    return _f32(rng.random_sample((n, 2)))


def _emitter_points(A, l, rng, n):
    """points on the mesh emitter of luminaire l with the face normals there, binary64"""
    s = int(A["lum_shape"][l])
    t0, t1 = int(A["shape_tri_offset"][s]), int(A["shape_tri_offset"][s + 1])
    tri = A["tri_idx"][t0:t1][rng.randint(0, t1 - t0, n)].astype(np.int64)
    pos = A["vtx_pos"].astype(np.float64)
    p0, p1, p2 = pos[tri[:, 0]], pos[tri[:, 1]], pos[tri[:, 2]]
    u = rng.random_sample((n, 2)); u = np.where(u.sum(axis=1, keepdims=True) > 1, 1 - u, u)
    pts = p0 + (p1 - p0) * u[:, :1] + (p2 - p0) * u[:, 1:]
    return pts, _unit(np.cross(p1 - p0, p2 - p0))


def _sel_samples(A, l, rng, n):
    """s0 values that select luminaire l, well inside its cell of the selection cdf"""
    c = A["lum_sel_cdf"].astype(np.float64)
    return _f32(c[l] + (c[l + 1] - c[l]) * (0.02 + 0.96 * rng.random_sample(n)))


def sample_inputs(A, rng, n=1500):
    """op 0: (p, s) records by class"""
    I = Inputs()
    nl = len(A["lum_type"])
    lo, hi = A["aabb_min"].astype(np.float64), A["aabb_max"].astype(np.float64)
    box = lambda m: lo + (hi - lo) * rng.random_sample((m, 3))                      # noqa: E731
    # --- selection ---
    I.add("selection: random", box(n), _rand_s(rng, n))
    I.add("selection: s0 = 0", box(200), np.stack([np.zeros(200), rng.random_sample(200)], axis=1))
    I.add("selection: s0 = 1 - 2^-24" + THRESHOLD_MARK, box(200), np.stack([np.full(200, TOP), rng.random_sample(200)], axis=1))
    knots = A["lum_sel_cdf"][1:-1]
    if len(knots):
        for nm, kv in zip(("one step below", "on", "one step above"), _steps(knots)):
            m = 60 * len(kv)
            I.add("selection: s0 %s a knot%s" % (nm, THRESHOLD_MARK), box(m), np.stack([np.tile(kv, 60), rng.random_sample(m)], axis=1))
    for l in range(nl):
        t = int(A["lum_type"][l])
        tag = "lum %d " % l
        s0 = lambda m, l=l: _sel_samples(A, l, rng, m)                              # noqa: E731
        S = lambda m, l=l: np.stack([s0(m), _f32(rng.random_sample(m))], axis=1)     # noqa: E731
        if t == R.AREA and A["shape_type"][int(A["lum_shape"][l])] == 0:
            pts, nrm = _emitter_points(A, l, rng, n)
            lat = 0.6 * rng.standard_normal((n, 3))
            I.add(tag + "mesh: p in front", pts + nrm * rng.uniform(0.3, 2.5, (n, 1)) + lat * 0.5, S(n))
            I.add(tag + "mesh: p behind", pts[:300] - nrm[:300] * rng.uniform(0.3, 2.5, (300, 1)), S(300))
            I.add(tag + "mesh: p in the plane of the emitter" + THRESHOLD_MARK, pts[:300] + np.cross(nrm[:300], lat[:300]), S(300))
            I.add(tag + "mesh: p at distance 1e-3", pts[:400] + nrm[:400] * 1e-3, S(400))
            I.add(tag + "mesh: p at distance 1e4", pts[:400] + nrm[:400] * 1e4 + lat[:400] * 1e3, S(400))
            if nl == 1:                      # with one luminaire the reused sample is s0 itself: the corners of squareToTriangle
                c = np.array([[0, 0], [0, TOP], [TOP, 0], [TOP, TOP]], dtype=np.float32)
                I.add(tag + "mesh: s0, s1 at 0 and 1 - 2^-24", (pts + nrm * 1.5)[:200], np.repeat(c, 50, axis=0))
            tc = A["lum_tri_cdf"][int(A["lum_cdf_offset"][l]):int(A["lum_cdf_offset"][l + 1])][1:-1]
            for nm, kv in zip(("one step below", "on", "one step above"), _steps(tc)):
                m = 20 * len(kv)
                I.add(tag + "mesh: s1 %s a triangle-cdf knot%s" % (nm, THRESHOLD_MARK), (pts + nrm * 1.5)[:1] + 0.3 * rng.standard_normal((m, 3)),
                      np.stack([s0(m), np.tile(kv, 20)], axis=1))
        elif t == R.AREA:
            SP = A["shape_params"][int(A["lum_shape"][l])]
            c, rad = SP[0:3].astype(np.float64), float(SP[3])
            d = _sphere_dirs(rng, n)
            ratio = 10 ** rng.uniform(np.log10(3e-2), np.log10(0.5), (n, 1))
            far = 10 ** rng.uniform(-4, np.log10(3e-2), (n, 1))
            I.add(tag + "sphere: radius / distance from 0.5 down to 3e-2", c + d * rad / ratio, S(n))
            # further out the discriminant of the ray-sphere root, 4 (r^2 - |w|^2 sin^2), cancels against b^2 = 4 |w|^2 cos^2 to
            # within binary32 reach: the restatement cannot say which cone rays hit.  What it can say is held: pdf if found
            I.add(tag + "sphere: radius / distance from 3e-2 down to 1e-4, the discriminant cancels" + THRESHOLD_MARK, c + d * rad / far, S(n))
            thr = 1 - R.EPSILON
            for dl in (1e-3, 1e-4, 1e-5):
                I.add(tag + "sphere: radius / distance below 1 - Epsilon by %g" % dl, c + d[:200] * rad / (thr * (1 - dl)), S(200))
                I.add(tag + "sphere: radius / distance above 1 - Epsilon by %g" % dl, c + d[:200] * rad / (thr * (1 + dl)), S(200))
            on = []
            for a in range(3):               # along each axis, at the binary32 distance nearest the switch and two steps either side
                base = _f32(c + np.eye(3)[a] * (rad / thr))
                for k in range(-2, 3):
                    q = base.copy()
                    for _ in range(abs(k)):
                        q[a] = np.nextafter(q[a], F(np.inf if k > 0 else -np.inf))
                    on.append(q)
            on = np.asarray(on, dtype=np.float32)
            I.add(tag + "sphere: radius / distance at 1 - Epsilon" + THRESHOLD_MARK, np.repeat(on, 15, axis=0), S(15 * len(on)))
            I.add(tag + "sphere: p inside", c + d[:400] * rad * rng.uniform(0.01, 0.95, (400, 1)), S(400))
            I.add(tag + "sphere: p at the centre", c[None, :], S(50))
            if l == 0:                       # s0 = 0 stays 0 through the selection's reuse
                I.add(tag + "sphere: s0 = 0, the cone axis", c + d[:300] * rad / ratio[:300], np.stack([np.zeros(300), rng.random_sample(300)], axis=1))
            k = rng.randint(4, 10 if nl == 1 else 7, 400)           # a sample reused from a cell of width 1 / n_lums has lost log2(n_lums) bits
            ratio = 10 ** rng.uniform(-1, np.log10(0.5), (n, 1))
            cell = A["lum_sel_cdf"][l:l + 2].astype(np.float64)
            I.add(tag + "sphere: s0 approaching 1, towards the tangent", c + d[:400] * rad / ratio[:400],
                  np.stack([cell[0] + (cell[1] - cell[0]) * (1 - 2.0 ** -k), rng.random_sample(400)], axis=1))
            if l == nl - 1:
                I.add(tag + "sphere: s0 = 1 - 2^-24, the tangent rays" + THRESHOLD_MARK, c + d[:200] * rad / ratio[:200],
                      np.stack([np.full(200, TOP), rng.random_sample(200)], axis=1))
        elif t in (R.CONSTANT, R.ENVMAP):
            LP = A["lum_params"][l]
            c, rad = LP[3:6].astype(np.float64), float(LP[6])
            d = _sphere_dirs(rng, n)
            I.add(tag + "background: p inside the bounding sphere", c + d * rad * rng.uniform(0, 0.98, (n, 1)), S(n))
            I.add(tag + "background: p outside the bounding sphere", c + d[:300] * rad * rng.uniform(1.02, 3, (300, 1)), S(300))
            on = _f32(c + d[:100] * rad)
            I.add(tag + "background: p on the bounding sphere" + THRESHOLD_MARK, on, S(100))
            if t == R.ENVMAP:
                _, _, rx, ry = A["env_size"]
                cdf = A["env_cdf"].astype(np.float64)
                cell = A["lum_sel_cdf"][l:l + 2].astype(np.float64)
                to_s0 = lambda v: _f32(cell[0] + (cell[1] - cell[0]) * np.asarray(v, dtype=np.float64))   # noqa: E731
                inside = c + d * rad * 0.5
                # knots of the envmap cdf, the black block's repeated knots among them
                kn = A["env_cdf"][1:-1]
                for nm, kv in zip(("one step below", "on", "one step above"), _steps(kn)):
                    if nl > 1:
                        kv = to_s0(kv)
                    I.add(tag + "envmap: s0 %s an envmap-cdf knot%s" % (nm, THRESHOLD_MARK), inside[:len(kv)], np.stack([kv, rng.random_sample(len(kv))], axis=1))
                w = cdf[1:] - cdf[:-1]
                mid = lambda rows: np.concatenate([cdf[i] + w[i] * rng.uniform(0.1, 0.9, 40) for i in range(rx * ry) if i // rx in rows and w[i] > 0])  # noqa: E731
                m0, m1 = to_s0(mid((0,))), to_s0(mid((ry - 1,)))
                I.add(tag + "envmap: first row", inside[:len(m0)], np.stack([m0, rng.random_sample(len(m0))], axis=1))
                I.add(tag + "envmap: first row, s1 = 0: y = 0, sinTheta = 0", inside[:len(m0)], np.stack([m0, np.zeros(len(m0))], axis=1))
                I.add(tag + "envmap: last row", inside[:len(m1)], np.stack([m1, rng.random_sample(len(m1))], axis=1))
                I.add(tag + "envmap: last row, s1 = 1 - 2^-24", inside[:len(m1)], np.stack([m1, np.full(len(m1), TOP)], axis=1))
    return I


def _env_dirs(A, l, rng):
    """world directions by class for the envmap's Le and pdf: (name, dirs, the class sits on a threshold of the density's
    lookup; None: a class for Le alone)"""
    LP = A["lum_params"][l]
    L2W = LP[16:25].reshape(3, 3).astype(np.float64)
    _, _, rx, ry = A["env_size"]
    H, W = A["env_pixels"].shape[:2]
    out = []
    def world(theta, phi):
        # envmap.cpp:152-153: the direction towards which (theta, phi) of the map lies, seen from the luminaire
        st, ct, sp, cp = np.sin(theta), np.cos(theta), np.sin(phi), np.cos(phi)
        return -(np.stack([-st * sp, -ct, st * cp], axis=-1) @ L2W.T)
    n = 1500
    out.append(("random", _sphere_dirs(rng, n), False))
    # Le only: at the poles themselves, and closer to them than 3e-5 rad, binary32 cannot tell the column (atan2 of two rounding
    # residues); Le's bound carries that, the density's cell does not
    out.append(("the poles", np.concatenate([world(np.array([0.0, np.pi]), np.zeros(2)),
                                             world(np.concatenate([10.0 ** -rng.uniform(4.5, 7, 100), np.pi - 10.0 ** -rng.uniform(4.5, 7, 100)]),
                                                   rng.uniform(-np.pi, np.pi, 200))]), None))
    out.append(("near the poles", world(np.concatenate([10.0 ** -rng.uniform(1.5, 4.5, 150), np.pi - 10.0 ** -rng.uniform(1.5, 4.5, 150)]),
                                        rng.uniform(-np.pi, np.pi, 300)), False))
    th = rng.uniform(0.05, np.pi - 0.05, 400)
    side = np.where(rng.random_sample(400) < 0.5, -1, 1)
    out.append(("either side of atan2 = +-pi", world(th, side * (np.pi - 10.0 ** -rng.uniform(1, 5, 400))), False))
    out.append(("on atan2 = +-pi", world(th, side * (np.pi - 10.0 ** -rng.uniform(6.5, 9, 400))), True))
    # borders of the density's cells and of the bitmap's texels (and texel centres, where the bilinear floor changes)
    for nm, nx, ny, thr in (("density cell borders", rx, ry, True), ("texel borders", W, H, None), ("texel centres", 2 * W, 2 * H, None)):
        kx, ky = rng.randint(0, nx + 1, 300), rng.randint(1, ny, 300)            # ky = 0 and ny are the poles
        a = world(np.pi * rng.uniform(0.05, 0.95, 300), -np.pi + 2 * np.pi * kx / nx)
        b = world(np.pi * ky / ny, rng.uniform(-np.pi, np.pi, 300))
        out.append((nm, np.concatenate([a, b]), thr))
    return out


def pdf_inputs(A, rng):
    """op 1: {lum: Inputs of (p, lp, ln, ld)} for the non-delta luminaires, beyond the round trip of the op 0 records"""
    out = {}
    n = 600
    for l in range(len(A["lum_type"])):
        t = int(A["lum_type"][l])
        I = Inputs()
        if t == R.AREA and A["shape_type"][int(A["lum_shape"][l])] == 0:
            pts, nrm = _emitter_points(A, l, rng, n)
            p = pts + nrm * rng.uniform(0.2, 3, (n, 1)) + 0.5 * rng.standard_normal((n, 3))
            I.add("mesh pdf: p in front", p, pts, nrm, _unit(p - pts))
            p = pts - nrm * rng.uniform(0.2, 3, (n, 1))
            I.add("mesh pdf: p behind", p[:200], pts[:200], nrm[:200], _unit(p - pts)[:200])
        elif t == R.AREA:
            SP = A["shape_params"][int(A["lum_shape"][l])]
            c, rad = SP[0:3].astype(np.float64), float(SP[3])
            d = _sphere_dirs(rng, n)
            ratio = 10 ** rng.uniform(np.log10(2e-3), np.log10(0.5), (n, 1))
            far = 10 ** rng.uniform(-4, np.log10(2e-3), (n, 1))
            lp = c + _sphere_dirs(rng, n) * rad
            nn = _unit(lp - c)
            I.add("sphere pdf: radius / distance from 0.5 down to 2e-3", c + d * rad / ratio, lp, nn, d)
            I.add("sphere pdf: radius / distance from 2e-3 down to 1e-4, 1 - cosThetaMax cancels", c + d * rad / far, lp, nn, d)
            thr = 1 - R.EPSILON
            for dl in (1e-3, 1e-5):
                I.add("sphere pdf: radius / distance below 1 - Epsilon by %g" % dl, c + d[:200] * rad / (thr * (1 - dl)), lp[:200], nn[:200], d[:200])
                I.add("sphere pdf: radius / distance above 1 - Epsilon by %g" % dl, c + d[:200] * rad / (thr * (1 + dl)), lp[:200], nn[:200], d[:200])
            I.add("sphere pdf: p inside", c + d[:200] * rad * rng.uniform(0.01, 0.95, (200, 1)), lp[:200], nn[:200], d[:200])
        elif t == R.ENVMAP:
            for nm, dirs, thr in _env_dirs(A, l, rng):
                if thr is None:              # a class for Le alone
                    continue
                z = np.zeros_like(dirs)
                I.add("envmap pdf: " + nm + (THRESHOLD_MARK if thr else ""), z, z, z, -dirs)      # pdf() looks up -lRec.d
        elif t == R.CONSTANT:
            z = np.zeros((50, 3))
            I.add("constant pdf", z, z, z, _sphere_dirs(rng, 50))
        else:
            continue
        out[l] = I
    return out


def le_inputs(A, rng):
    """op 2: directions by class, or None without a background"""
    l = int(A["background_lum"])
    if l < 0:
        return None
    I = Inputs()
    if int(A["lum_type"][l]) == R.ENVMAP:
        for nm, dirs, thr in _env_dirs(A, l, rng):
            I.add("Le: " + nm, dirs)
        d = _sphere_dirs(rng, 300)
        for k in (1e-3, 7.0, 1e3):
            I.add("Le: direction of length %g" % k, d * k)
    else:
        d = _sphere_dirs(rng, 100)
        I.add("Le: random", d)
        I.add("Le: direction of length 1e3", d * 1e3)
    return I


# ---------------------------------------------------------------------------------------------------------------------
# the check
# ---------------------------------------------------------------------------------------------------------------------
def _ratio(got, ref, err):
    """|got - ref| in units of 2^-23 x err (ATOL taken off first); inf for a non-finite got where ref is finite"""
    got, ref, err = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64), np.asarray(err, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = np.abs(got - ref) - cf.ATOL
        r = np.where(d > 0, d / np.where(err > 0, EPS * err, 1e-300), 0.0)
        r = np.where(np.isfinite(ref) & ~np.isfinite(got), np.inf, r)
        r = np.where(np.isfinite(ref), r, 0.0)
        r = np.where(np.isnan(r), np.inf, r)
    return r


def sample_ratios(ref, got):
    """per record: (value-kind ratio, vector-kind ratio, mismatch) of an op 0 read-out against one Sample of ref64_lum"""
    gfound = got[:, 0] != 0
    glum = got[:, 1].astype(np.int64)
    mismatch = gfound != ref.found
    both = gfound & ref.found
    mismatch |= both & (glum != ref.lum)
    cmp_ = both & ~ref.delta
    inf_pdf = cmp_ & ~np.isfinite(ref.pdf)                        # y = 0 of the envmap: pdf = inf and value = 0 by the reference's own arithmetic
    mismatch |= inf_pdf & ~((got[:, 11] == ref.pdf) & (got[:, 12:15] == 0).all(axis=1))
    # a distant sphere whose 1 - cosThetaMax binary32 may round to 0: pdf = inf, value = 0 is the reference's own answer
    ovf_inf = cmp_ & ref.ovf & (got[:, 11] == np.inf) & (got[:, 12:15] == 0).all(axis=1)
    fin = cmp_ & ~inf_pdf & ~ovf_inf
    rv = np.maximum(_ratio(got[:, 11], ref.pdf, ref.pdf_err), _ratio(got[:, 12:15], ref.value, ref.value_err).max(axis=1))
    rd = np.maximum.reduce([_ratio(got[:, 2:5], ref.p, ref.p_err).max(axis=1), _ratio(got[:, 5:8], ref.n, ref.n_err).max(axis=1),
                            _ratio(got[:, 8:11], ref.d, ref.d_err).max(axis=1)])
    rd_geo = np.where(inf_pdf | ovf_inf, rd, 0.0)
    return np.where(fin, rv, 0.0), np.where(fin, rd, rd_geo), mismatch


def check_sample(T, I, got):
    """op 0 read-outs `got` [n][16] of the records I against the restatement -> (failures, report {class: (worst value
    ratio, worst vector ratio, set aside, n)})"""
    p, s = I.cols
    failures, report = [], {}
    ref = R.sample_luminaire(T, p, s)
    rv, rd, mm = sample_ratios(ref, got)
    lo = None
    # non-finite output where the truth is finite fails on every record, ambiguous or not
    gfound = got[:, 0] != 0
    glum = got[:, 1].astype(np.int64)
    with np.errstate(invalid="ignore"):
        ref_fin = np.isfinite(ref.pdf) | ~ref.found
    ovf_inf = ref.ovf & (got[:, 11] == np.inf) & np.isfinite(np.delete(got[:, 2:15], 9, axis=1)).all(axis=1)
    bad = gfound & ~np.isfinite(got[:, 2:15]).all(axis=1) & ref_fin & ~ovf_inf
    bad |= ~np.isfinite(got[:, 0:2]).all(axis=1)
    if bad.any():
        i = int(np.argmax(bad))
        failures.append("%d records with non-finite output where the reference is finite, e.g. p %s s %s -> %s" % (bad.sum(), p[i].tolist(), s[i].tolist(), got[i].tolist()))
    for name, idx in I.classes.items():
        aside = (ref.amb | ref.knot)[idx]
        v, d, m = rv[idx], rd[idx], mm[idx]
        if name.endswith(THRESHOLD_MARK):
            if lo is None:
                alts = [R.sample_luminaire(T, p, s, tie=t) for t in (-1, 1, 2)]
                lo = [sample_ratios(a, got) for a in alts]
                alt_amb = alts[0].amb | alts[1].amb | alts[2].amb
            # either neighbouring branch; a record one of whose branches the restatement cannot decide for another reason is
            # set aside
            cand = [(v, d, m)] + [tuple(a[idx] for a in c) for c in lo]
            score = [np.where(c[2], np.inf, np.maximum(c[0] / cf.K_VALUE, c[1] / cf.K_DIR)) for c in cand]
            best = np.argmin(np.stack(score), axis=0)
            v = np.choose(best, [c[0] for c in cand]); d = np.choose(best, [c[1] for c in cand]); m = np.choose(best, [c[2] for c in cand])
            aside = (ref.amb | alt_amb)[idx]
        else:
            if aside.sum() > cf.MAX_AMBIGUOUS * len(idx):
                failures.append("%s: %d of %d records undecidable in binary32 -- the class tests too little" % (name, aside.sum(), len(idx)))
        v, d, m = np.where(aside, 0.0, v), np.where(aside, 0.0, d), m & ~aside
        # a record set aside because the restatement cannot decide whether a cone ray hits the sphere still has a pdf if found
        known = aside & gfound[idx] & np.isfinite(ref.pdf_if_found[idx]) & (glum[idx] == ref.lum[idx]) & ~(ref.ovf[idx] & (got[idx, 11] == np.inf))
        v = np.where(known, _ratio(got[idx, 11], ref.pdf_if_found[idx], ref.pdf_if_found_err[idx]), v)
        report[name] = (float(v.max()), float(d.max()), int(aside.sum()), len(idx))
        if m.any():
            i = int(idx[np.argmax(m)])
            failures.append("%s: %d records differ in found / luminaire index (or the pole's pdf = inf, value = 0), e.g. p %s s %s: got found %g lum %g pdf %g, ref found %s lum %d pdf %g"
                            % (name, m.sum(), p[i].tolist(), s[i].tolist(), got[i, 0], got[i, 1], got[i, 11], ref.found[i], ref.lum[i], ref.pdf[i]))
        if (v > cf.K_VALUE).any():
            i = int(idx[np.argmax(v)])
            failures.append("%s: worst value ratio %.3g > %g at p %s s %s: got pdf %.9g value %s, ref pdf %.9g (bound %.3g) value %s"
                            % (name, v.max(), cf.K_VALUE, p[i].tolist(), s[i].tolist(), got[i, 11], got[i, 12:15].tolist(), ref.pdf[i], ref.pdf_err[i], ref.value[i].tolist()))
        if (d > cf.K_DIR).any():
            i = int(idx[np.argmax(d)])
            failures.append("%s: worst vector ratio %.3g > %g at p %s s %s: got p %s n %s d %s, ref p %s n %s d %s"
                            % (name, d.max(), cf.K_DIR, p[i].tolist(), s[i].tolist(), got[i, 2:5].tolist(), got[i, 5:8].tolist(), got[i, 8:11].tolist(),
                               ref.p[i].tolist(), ref.n[i].tolist(), ref.d[i].tolist()))
    return failures, report


def check_pdf(T, l, I, got, label=""):
    """op 1 read-outs `got` [n] of luminaire l -> (failures, report)"""
    p, lp, ln, ld = I.cols
    failures, report = [], {}
    val, cond, knot, amb = R.pdf_luminaire(T, p, l, lp, ln, ld)
    ovf_inf = R.pdf_luminaire.ovf & (got == np.inf)
    r0 = np.where(ovf_inf, 0.0, _ratio(got, val, cond * np.abs(val)))
    alt = None
    bad = ~np.isfinite(got) & np.isfinite(val) & ~ovf_inf
    if bad.any():
        failures.append("%s%d non-finite pdfs where the reference is finite" % (label, bad.sum()))
    for name, idx in I.classes.items():
        r, aside = r0[idx], (knot | amb)[idx]
        if name.endswith(THRESHOLD_MARK):
            if alt is None:
                alt = []
                for t in (-1, 1):
                    v2, c2, _, _ = R.pdf_luminaire(T, p, l, lp, ln, ld, tie=t)
                    alt.append(_ratio(got, v2, c2 * np.abs(v2)))
            r = np.minimum(r, np.minimum(alt[0][idx], alt[1][idx]))
            aside = amb[idx]
        elif aside.sum() > cf.MAX_AMBIGUOUS * len(idx):
            failures.append("%s%s: %d of %d records undecidable in binary32 -- the class tests too little" % (label, name, aside.sum(), len(idx)))
        r = np.where(aside, 0.0, r)
        report[name] = (float(r.max()), 0.0, int(aside.sum()), len(idx))
        if (r > cf.K_VALUE).any():
            i = int(idx[np.argmax(r)])
            failures.append("%s%s: worst ratio %.3g > %g at p %s lp %s ln %s ld %s: got %.9g ref %.9g cond %.3g"
                            % (label, name, r.max(), cf.K_VALUE, p[i].tolist(), lp[i].tolist(), ln[i].tolist(), ld[i].tolist(), got[i], val[i], cond[i]))
    return failures, report


def check_le(T, I, got):
    """op 2 read-outs `got` [n][3] -> (failures, report)"""
    (dirs,) = I.cols
    failures, report = [], {}
    val, cond, amb = R.background_le(T, dirs)
    cf._non_finite(failures, "Le", got, val)
    r0 = _ratio(got, val, cond * np.abs(val)).max(axis=1)
    for name, idx in I.classes.items():
        r = np.where(amb[idx], 0.0, r0[idx])
        if amb[idx].sum() > cf.MAX_AMBIGUOUS * len(idx):
            failures.append("%s: %d of %d records undecidable" % (name, amb[idx].sum(), len(idx)))
        report[name] = (float(r.max()), 0.0, int(amb[idx].sum()), len(idx))
        if (r > cf.K_VALUE).any():
            i = int(idx[np.argmax(r)])
            failures.append("%s: worst ratio %.3g > %g at %s: got %s ref %s cond %s" % (name, r.max(), cf.K_VALUE, dirs[i].tolist(), got[i].tolist(), val[i].tolist(), cond[i].tolist()))
    return failures, report


def round_trip(T, I, got, evaluate):
    """for every op 0 record with found = 1 on a non-delta luminaire: op 1 on what it returned gives the same pdf, within the
    value tolerance of the two (the sample's bound plus the pdf's at the returned record).  Envmap records the restatement
    flags for a cell border or the pole clamp are left out -> (failures, report)"""
    p, s = I.cols
    failures, report = [], {}
    ref = R.sample_luminaire(T, p, s)
    found = got[:, 0] != 0
    glum = got[:, 1].astype(np.int64)
    for l in np.unique(glum[found]):
        if int(T.A["lum_type"][l]) not in R.NON_DELTA:
            continue
        m = np.nonzero(found & (glum == l) & np.isfinite(got[:, 11]))[0]
        if not len(m):
            continue
        q = np.zeros((len(m), 16), dtype=np.float32)
        q[:, 0:3] = p[m]; q[:, 3:12] = got[m, 2:11]; q[:, 12] = l
        back = evaluate(1, q)[:, 0].astype(np.float64)
        val, cond, knot, amb = R.pdf_luminaire(T, p[m], l, got[m, 2:5], got[m, 5:8], got[m, 8:11])
        bound = cond * np.abs(val) + np.where(ref.found[m] & (ref.lum[m] == l), ref.pdf_err[m], 0.0)
        r = _ratio(back, got[m, 11], bound)
        # sample() divides by sin(theta), pdf() by sqrt(max(Epsilon, 1 - d.y^2)): within 0.01 rad of a pole the reference's own
        # two functions disagree
        out = knot | amb | ref.amb[m] | R.pdf_luminaire.clamp
        r = np.where(out, 0.0, r)
        report["round trip, lum %d" % l] = (float(r.max()), 0.0, int(out.sum()), len(m))
        if (r > cf.K_VALUE).any():
            i = int(np.argmax(r))
            failures.append("round trip, lum %d: worst ratio %.3g > %g at p %s s %s: sample pdf %.9g, pdf() of its record %.9g"
                            % (l, r.max(), cf.K_VALUE, p[m[i]].tolist(), s[m[i]].tolist(), got[m[i], 11], back[i]))
    return failures, report


def check_scene(evaluate, A, seed, parts=("sample", "pdf", "le", "round trip")):
    """every class of every operation for the scene with arrays A through `evaluate(op, queries [n][16]) -> [n][16]`"""
    T = R.tables(A)
    rng = np.random.RandomState(seed)
    failures, report = [], {}
    I = sample_inputs(A, rng)
    q = np.zeros((I.n, 16), dtype=np.float32)
    q[:, 0:3], q[:, 3:5] = I.cols
    got = evaluate(0, q)
    if "sample" in parts:
        f, r = check_sample(T, I, got); failures += f; report.update(r)
    if "round trip" in parts:
        f, r = round_trip(T, I, got, evaluate); failures += f; report.update(r)
    if "pdf" in parts:
        for l, J in pdf_inputs(A, rng).items():
            q = np.zeros((J.n, 16), dtype=np.float32)
            q[:, 0:3], q[:, 3:6], q[:, 6:9], q[:, 9:12] = J.cols
            q[:, 12] = l
            f, r = check_pdf(T, l, J, evaluate(1, q)[:, 0], "lum %d " % l); failures += f
            report.update({"lum %d %s" % (l, k): v for k, v in r.items()})
    J = le_inputs(A, rng)
    if "le" in parts and J is not None:
        q = np.zeros((J.n, 16), dtype=np.float32)
        q[:, 0:3] = J.cols[0]
        f, r = check_le(T, J, evaluate(2, q)[:, 0:3]); failures += f; report.update(r)
    return failures, report


def format_report(report):
    return "\n".join("  %-95s value %7.3g / %g  vector %7.3g / %g  set aside %d of %d" % (k, v[0], cf.K_VALUE, v[1], cf.K_DIR, v[2], v[3])
                     for k, v in report.items())


# Worst ratios the oracle reached on the CPU when this list was written (units of 2^-23 x the derived bound; a value may
# reach K_VALUE = 16, a vector K_DIR = 64), by class family over the nine scenes:
#   selection (random, s0 = 0, s0 = 1 - 2^-24, the knots and a step either side)      value 0.55   vector 0.56
#   mesh: in front / behind / distance 1e-3 / 1e4 / corners / triangle-cdf knots      value 0.33   vector 0.59
#   mesh: p in the plane of the emitter (set aside where dp is within reach of 0)     value 0.33   vector 0.43
#   sphere: radius / distance 0.5 .. 3e-2, the cone axis, towards the tangent          value 0.49   vector 0.30
#   sphere: either side of and on the 1 - Epsilon switch                               value 0.39   vector 0.82
#   sphere: 3e-2 .. 1e-4 (pdf if found; below 2.4e-4 the reference's own inf)          value 0.50   vector 0.27
#   constant / envmap: inside, outside, on the bounding sphere                         value 0.56   vector 0.56
#   envmap: cdf knots, first and last row, y = 0                                       value 0.52   vector 0.46
#   round trip                                                                          value 0.98 (envmap), 0.07 (mesh), 0 (sphere, constant)
#   pdf queries                                                                         value 0.49
#   Le queries                                                                          value 0.22
# The bounds are worst-case first-order sums, so a faithful binary32 evaluation sits near 1 at most; test_lum_truth.py holds
# the oracle below WORST_ORACLE so that a drift of the restatement's bounds shows before it eats the margin.
WORST_ORACLE = (2.0, 2.0)
