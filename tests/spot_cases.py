"""Inputs shared by tests/test_spot.py (CPU) and tests/test_gpu_spot.py (device): spot luminaires in four poses (one with a
toWorld that is aligned to no axis) under the cutoff / beam pairs 20 / 15, 60 / 60 and 89 / 10 degrees; as projection textures a
checkerboard and a grid under three Texture2D transforms (the identity; scale 4 with offset 0.25; a negative scale), the bitmaps of
tests/bmp_cases.py for the nearest lookup, and power-of-two bitmaps of 1 x 1, 2 x 2, 1 x 8 and 16 x 16 texels (width x height) under
all four wrap modes for the bilinear one; and points: random ones in and around the cone, points bisected onto cosTheta ==
cosCutoff and == cosBeamWidth with the binary32 neighbours of each, the axis, points whose uv sits on a texel edge, a checker edge
or the xPos == 0 column of the bilinear lookup, and points whose uv lies at 0 or 1 up to rounding.  Test infrastructure."""
import numpy as np

import bmp_cases
import ref64_bmp as B
import ref64_spot as R
import ref64_tex as T

F = np.float32
POSES = [((0.0, 2.0, 0.0), (0.0, 0.0, 0.0)),             # straight down
         ((1.0, 2.5, 1.0), (0.0, 0.0, 0.0)),             # aligned to no axis
         ((-0.8, 1.8, 0.8), (0.4, 0.0, -0.3)),
         ((0.3, 0.2, -2.0), (0.3, 0.2, 1.0))]            # along +z
ANGLES = [(20.0, 15.0), (60.0, 60.0), (89.0, 10.0)]      # cutoff, beam width (degrees)
TRANSFORMS = {"id": (0.0, 0.0, 1.0, 1.0), "scale4": (0.25, 0.25, 4.0, 4.0), "neg": (0.3, -0.2, -2.5, -3.0)}      # uoffset, voffset, uscale, vscale
BILINEAR_SIZES = {"1x1": (1, 1), "2x2": (2, 2), "1x8": (1, 8), "16x16": (16, 16)}      # width, height


def description(mts):
    """one triangle and the twelve spots, pose-major: luminaire 3 * pose + pair"""
    S = mts.scenes
    sd = S.SceneDescription("spot_cases")
    b = sd.lambertian(0.5)
    sd.add_mesh(np.float32([[-1, 0, -1], [1, 0, -1], [0, 0, 1]]), np.uint32([[0, 1, 2]]), bsdf=b, face_normals=True, name="floor")
    for k, (pos, tgt) in enumerate(POSES):
        for j, (cut, beam) in enumerate(ANGLES):
            sd.spot_light(pos, tgt, (3.0 + k, 2.0 + j, 1.5), cutoff_deg=cut, beam_deg=beam)
    sd.camera = dict(origin=(0.0, 3.0, 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), fov=40.0)
    return sd


_blocks = {}


def spots(mts):
    """the twelve ref64_spot.Spot objects, from the blocks the flattener completes (configure(), spot.cpp:55-61)"""
    if "b" not in _blocks:
        sc = mts.Scene(description(mts))
        _blocks["b"] = np.array(sc.arrays()["lum_params"], dtype=np.float32).reshape(-1, mts.abi.LUM_NPARAMS).copy()
    return [R.Spot(P) for P in _blocks["b"]]


def bilinear_texels(name):
    w, h = BILINEAR_SIZES[name]
    return np.random.RandomState(300 + 31 * w + h).uniform(0.05, 1.0, (h, w, 3)).astype(np.float32)


def textures():
    """name -> ref64_spot.SpotTex"""
    out = {}
    for tn, tr in TRANSFORMS.items():
        out["checker/" + tn] = R.SpotTex(T.Tex(T.CHECKERBOARD, *tr, bright=(1.0, 0.9, 0.8), dark=(0.25, 0.2, 0.1)))
        out["grid/" + tn] = R.SpotTex(T.Tex(T.GRID, *tr, bright=(0.7, 0.8, 0.9), dark=(0.1, 0.05, 0.2), line_width=0.06))
    for name, t in bmp_cases.textures().items():
        out["nearest/" + name] = R.SpotTex(t, False)
    for size in BILINEAR_SIZES:
        tx = bilinear_texels(size)
        for wrap, wname in enumerate(B.WRAP_NAMES):
            for tn in ("id", "neg"):
                out["bilinear/%s/%s/%s" % (size, wname, tn)] = R.SpotTex(B.Bmp(tx, wrap, *TRANSFORMS[tn]), True)
    return out


def scene_texture(S, st):
    """the scenes texture object of a ref64_spot.SpotTex"""
    t = st.tex
    if st.kind == R.BITMAP:
        return bmp_cases.scene_texture(S, t)
    cls = S.Checkerboard if st.kind == R.CHECKERBOARD else S.GridTexture
    kw = dict(bright=t.bright, dark=t.dark, uoffset=t.uoffset, voffset=t.voffset, uscale=t.uscale, vscale=t.vscale)
    if st.kind == R.GRID:
        kw["line_width"] = t.line_width
    return cls(**kw)


def cases(mts):
    """[(name, Spot, SpotTex)]: every texture with one of the spots, in turn, so that every spot meets every kind of texture"""
    sp = spots(mts)
    out = []
    for i, (name, st) in enumerate(sorted(textures().items())):
        j = (5 * i + i // len(sp)) % len(sp)
        out.append(("%s @ spot %d" % (name, j), sp[j], st))
    return out


def _world(spot, local, dist):
    """points at distance dist [n] along the luminaire-space directions local [n][3] (binary64) -> binary32 [n][3]"""
    W = spot.w2l.astype(np.float64)
    d = local @ W                                       # the rows of W are the luminaire's axes in world space
    d /= np.linalg.norm(d, axis=1)[:, None]
    return (spot.position.astype(np.float64) + d * np.asarray(dist)[:, None]).astype(np.float32)


def _from_uv(spot, uvx, uvy, dist):
    f = np.tan(np.float64(spot.cutoff))
    local = np.stack([(np.asarray(uvx) - 0.5) * 2 * f, (np.asarray(uvy) - 0.5) * 2 * f, np.ones(len(uvx))], axis=1)
    return _world(spot, local, dist)


def _on_cone(spot, theta, phi, dist):
    local = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)], axis=1)
    return _world(spot, local, dist)


def threshold_points(spot, n_phi=1, seed=0):
    """points bisected onto the two cone thresholds of the mirror: for each azimuth the last angle on one side and the first on the
    other, and the binary32 neighbours of both in every coordinate"""
    out = []
    rng = np.random.RandomState(2000 + seed)
    phi, dist = rng.uniform(0.0, 2 * np.pi, n_phi), rng.uniform(0.5, 3.0, n_phi)
    for which, angle in (("inside", float(spot.cutoff)), ("in_beam", float(spot.beam))):
        lo, hi = np.full(n_phi, angle - 1e-3), np.full(n_phi, angle + 1e-3)
        for _ in range(50):
            mid = 0.5 * (lo + hi)
            flag = getattr(R.mirror(spot, None, _on_cone(spot, mid, phi, dist)), which)
            lo, hi = np.where(flag, mid, lo), np.where(flag, hi, mid)
        for th in (lo, hi):
            p = _on_cone(spot, th, phi, dist)
            out.append(p)
            for k in range(3):
                for s in (np.inf, -np.inf):
                    q = p.copy(); q[:, k] = np.nextafter(q[:, k], F(s)); out.append(q)
    return np.concatenate(out)


def edge_uvs(st):
    """uv values that put uv' on a texel edge, a checker edge, a grid line's rim or the xPos == 0 column, and at 0 and 1"""
    t = st.tex
    if st.kind == R.BITMAP:
        xs = [k / t.width for k in range(-1, t.width + 2)] + [(k + 0.5) / t.width for k in (-1, 0, 1, t.width - 1, t.width)]
        ys = [k / t.height for k in range(-1, t.height + 2)] + [(k + 0.5) / t.height for k in (-1, 0, t.height - 1, t.height)]
    else:
        xs = ys = [k / 2.0 for k in range(-2, 5)] + [float(t.line_width), 1.0 - float(t.line_width), 0.5]
    us, uo, vs, vo = float(t.uscale), float(t.uoffset), float(t.vscale), float(t.voffset)
    ux = np.array([(x - uo) / us for x in xs] + [0.0, 1.0, 0.5])
    uy = np.array([(y - vo) / vs for y in ys] + [0.0, 1.0, 0.5])
    ux, uy = ux[(ux > -0.02) & (ux < 1.02)], uy[(uy > -0.02) & (uy < 1.02)]
    gx, gy = np.meshgrid(ux, uy[:: max(1, len(uy) // 5)], indexing="ij")
    return np.clip(gx.ravel(), 0.0, 1.0), np.clip(gy.ravel(), 0.0, 1.0)


N_EDGE, N_RIM = 6, 2


def points(spot, st, n_random=2000, seed=0, thresholds=None):
    """the points of one case, binary32 [n][3].  The points that sit on a decision by construction -- the bisected ones (every
    fourth case has them unless `thresholds` says otherwise), N_EDGE edge points, N_RIM rim points -- are fragile by design; the
    random ones are there in such numbers that the fragile share of all records stays below 1 %"""
    if thresholds is None:
        thresholds = seed % 4 == 0
    rng = np.random.RandomState(1000 + seed)
    cut = float(spot.cutoff)
    theta = np.concatenate([rng.uniform(0.0, cut, n_random * 3 // 4), rng.uniform(cut, min(cut * 1.3, 3.0), n_random // 4)])
    parts = [_on_cone(spot, theta, rng.uniform(0, 2 * np.pi, len(theta)), rng.uniform(0.3, 4.0, len(theta))),
             _on_cone(spot, np.zeros(2), np.zeros(2), np.array([0.5, 2.0])),                      # the axis
             ] + ([threshold_points(spot, seed=seed)] if thresholds else [])
    if st is not None:
        ux, uy = edge_uvs(st)
        # the cutoff cone is the disc inscribed in the unit square of uv: keep what lies inside it
        inside = (ux - 0.5) ** 2 + (uy - 0.5) ** 2 < 0.2499
        pick = rng.permutation(int(inside.sum()))[:N_EDGE]
        ux, uy = ux[inside][pick], uy[inside][pick]
        parts.append(_from_uv(spot, ux, uy, rng.uniform(0.5, 3.0, len(ux))))
        # uv at 0 or 1 up to rounding: the rim of the cone along the luminaire's axes
        rim = np.array([0.0, 1.0])[[seed % 2]]; mid = np.array([0.5])
        parts.append(_from_uv(spot, 0.5 + (rim - 0.5) * (1.0 - 1e-7), mid, np.full(1, 1.3)))
        parts.append(_from_uv(spot, mid, 0.5 + (rim - 0.5) * (1.0 - 1e-6), np.full(1, 0.9)))
    return np.concatenate(parts).astype(np.float32)


# --- hand-computed records -----------------------------------------------------------------------------------------------------
def down_spot(mts, cutoff=45.0, beam=45.0, intensity=(2.0, 4.0, 8.0)):
    """a spot at (0, 2, 0) that looks straight down, with the axes spot_light gives it and the block the flattener completes"""
    S = mts.scenes
    sd = S.SceneDescription("spot_hand")
    b = sd.lambertian(0.5)
    sd.add_mesh(np.float32([[-1, 0, -1], [1, 0, -1], [0, 0, 1]]), np.uint32([[0, 1, 2]]), bsdf=b, face_normals=True, name="floor")
    sd.spot_light((0.0, 2.0, 0.0), (0.0, 0.0, 0.0), intensity, cutoff_deg=cutoff, beam_deg=beam)
    sd.camera = dict(origin=(0.0, 3.0, 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), fov=40.0)
    P = np.array(mts.Scene(sd).arrays()["lum_params"], dtype=np.float32).reshape(-1, mts.abi.LUM_NPARAMS)[0]
    return R.Spot(P)


# --- the end-to-end scenes -----------------------------------------------------------------------------------------------------
E2E_CUTOFF, E2E_BEAM = 30.0, 22.5


def e2e_description(mts, texture=None, bilinear=False, shape="floor", tilted=False, extra_light=False):
    """a two-triangle floor (or a sphere on it) under a spot with cutoff 30 and beam 22.5 degrees, seen from above"""
    S = mts.scenes
    sd = S.SceneDescription("spot_e2e_%s%s" % (shape, "_tilted" if tilted else ""))
    b = sd.lambertian(0.5)
    sd.add_mesh(np.float32([[-2, 0, -2], [2, 0, -2], [2, 0, 2], [-2, 0, 2]]), np.uint32([[0, 2, 1], [0, 3, 2]]), bsdf=b, face_normals=True, name="floor")
    if shape == "sphere":
        sd.add_sphere((0.1, 0.45, -0.05), 0.45, bsdf=b)
    pos, tgt = ((0.9, 2.2, 0.6), (0.05, 0.0, -0.1)) if tilted else ((0.0, 2.5, 0.0), (0.0, 0.0, 0.0))
    sd.spot_light(pos, tgt, (8.0, 8.0, 8.0), cutoff_deg=E2E_CUTOFF, beam_deg=E2E_BEAM, texture=texture, bilinear=bilinear)
    if extra_light:
        sd.point_light((1.5, 1.0, -1.0), (0.5, 0.25, 0.125))
    sd.camera = dict(origin=(0.0, 4.0, 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), fov=35.0)
    sd.max_depth = 2
    return sd


def floor_hits(rays):
    """the binary64 hit points on the plane y = 0 of camera rays [n][>=6] = origin, direction -> [n][3]"""
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    t = -o[:, 1] / d[:, 1]
    return o + d * t[:, None]


def sphere_hits(rays, center=(0.1, 0.45, -0.05), radius=0.45):
    """(hit [n] bool, points [n][3]) of the rays on the sphere, binary64; the inputs are the binary32 values the scene holds"""
    c = np.asarray(center, dtype=np.float32).astype(np.float64); r = float(F(radius))
    o, d = rays[:, 0:3].astype(np.float64), rays[:, 3:6].astype(np.float64)
    oc = o - c
    a, b, cc = (d * d).sum(axis=1), 2 * (oc * d).sum(axis=1), (oc * oc).sum(axis=1) - r * r
    disc = b * b - 4 * a * cc
    hit = disc > 1e-9
    t = (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2 * a)
    return hit, o + d * t[:, None]
