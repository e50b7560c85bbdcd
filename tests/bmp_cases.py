"""Inputs shared by tests/test_bmp.py (CPU) and tests/test_gpu_bmp.py (device), as small as they can be and still go wrong:
bitmaps of 1 x 1, 1 x 7, 5 x 3 and 16 x 16 texels (width x height) under all four wrap modes and three transforms (the identity,
and scales of +-3.7 with offsets of +-0.3, one of them with a negative vscale); tests/tex_cases.py's floor grid, whose texcoords
jump across every edge and reach below zero; a strip of triangles whose first vertex carries uv exactly -- on texel edges of
every bitmap, at 0 and 1, negative, and one binary32 step to either side; a second strip with magnitudes just inside the limit of
the (int) cast; one sphere.  Also the closed-form geometry of the end-to-end scenes under their orthographic camera
(tex_cases' derivation with the bitmap's decision), so that what the device test leaves out is decided by the CPU side and the
restatement alone.  Test infrastructure."""
import numpy as np

import ref64_bmp as R
import tex_cases

F = np.float32
SIZES = {"1x1": (1, 1), "1x7": (1, 7), "5x3": (5, 3), "16x16": (16, 16)}       # width, height
TRANSFORMS = {"id": (0.0, 0.0, 1.0, 1.0), "scaled": (0.3, -0.3, 3.7, -3.7), "neg": (-0.3, 0.3, -3.7, 3.7)}      # uoffset, voffset, uscale, vscale
CAST_LIMIT = 2147483648.0 - 65536.0
# the largest |uv| of the second strip: times 16 texels it is 2^31 - 2^17, inside the limit; every product on the way is exact
HUGE = F((2147483648.0 - 131072.0) / 16.0)
PALETTE_N = 12
# the end-to-end runs: shape, wrap mode, transform.  One black and one white, so that the column-0 constant is seen in a frame; the
# sphere's uv lies in [0, 1], so under the identity column 0 is its first sixteenth
E2E = [("grid", R.REPEAT, "scaled"), ("grid", R.BLACK_MODE, "id"), ("sphere", R.WHITE_MODE, "id"), ("sphere", R.REPEAT, "neg")]


def texels(name):
    """distinct values per texel and channel, exact in binary32"""
    w, h = SIZES[name]
    rng = np.random.RandomState(100 + 17 * w + h)
    return rng.uniform(0.05, 1.0, (h, w, 3)).astype(np.float32)


def textures():
    """name -> ref64_bmp.Bmp: every bitmap x wrap mode x transform; textures of one bitmap share its texels array"""
    out = {}
    for size in SIZES:
        tx = texels(size)
        for wrap, wname in enumerate(R.WRAP_NAMES):
            for tname, tr in TRANSFORMS.items():
                out["%s/%s/%s" % (size, wname, tname)] = R.Bmp(tx, wrap, *tr)
    return out


def scene_texture(S, t):
    """the scenes.BitmapTexture of a ref64_bmp.Bmp"""
    return S.BitmapTexture(texels=t.texels, wrap=R.WRAP_NAMES[t.wrap], uoffset=t.uoffset, voffset=t.voffset, uscale=t.uscale, vscale=t.vscale)


def boundary_values():
    """uv on the texel edges of the shared bitmaps (k/16, k/5, k/3, k/7, k/1), negative ones among them, and one binary32 step to
    either side"""
    base = [0.0, -0.0, 1.0, -1.0, 2.0, -3.0]
    base += [k / 16.0 for k in (1, 3, 8, 15, 17, -1, -5, -16, -17)]
    base += [k / 5.0 for k in (1, 2, 4, 6, -1, -3)] + [k / 3.0 for k in (1, 2, 4, -1, -2)] + [k / 7.0 for k in (1, 3, 6, 8, -2)]
    out = []
    for b in base:
        b = F(b)
        out += [b, np.nextafter(b, F(np.inf)), np.nextafter(b, F(-np.inf))]
    return np.array(out, dtype=np.float32)


def _strip(t0, origin):
    """one small triangle per row of t0 [n][2]: vertex 0 carries that texcoord, so that the record (u, v) = (0, 0) gives its.uv =
    t0 exactly (b = (1, 0, 0)) -> positions, triangles, texcoords"""
    n = t0.shape[0]
    k = np.arange(n, dtype=np.float32)
    base = np.stack([F(origin) + F(0.01) * k, np.zeros(n, dtype=np.float32), np.full(n, F(origin))], axis=1)
    pos = np.stack([base, base + np.float32([0.008, 0, 0]), base + np.float32([0, 0, 0.008])], axis=1).reshape(-1, 3)
    uv = np.stack([t0, t0 + np.float32([0.3, 0.1]), t0 + np.float32([-0.2, 0.4])], axis=1).reshape(-1, 2)
    return pos.astype(np.float32), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), uv.astype(np.float32)


def boundary_strip():
    b = boundary_values()
    bx, by = np.meshgrid(b, b[::3], indexing="ij")
    return _strip(np.stack([bx.ravel(), by.ravel()], axis=1).astype(np.float32), 5.0)


def huge_strip():
    """magnitudes just inside the cast limit, in every sign pattern, next to small ones; only the identity transform keeps them
    inside it"""
    h = [HUGE, -HUGE, np.nextafter(HUGE, F(0)), -np.nextafter(HUGE, F(0)), F(HUGE / 2), F(0.3), F(-0.7)]
    bx, by = np.meshgrid(np.float32(h), np.float32(h), indexing="ij")
    return _strip(np.stack([bx.ravel(), by.ravel()], axis=1).astype(np.float32), -60.0)


def hook_scene(mts):
    """shape 0: the floor grid, 1: the boundary strip, 2: the huge strip, 3: a mesh WITHOUT texcoords, 4: the sphere"""
    S = mts.scenes
    sd = S.SceneDescription("bmp_hook")
    white = sd.lambertian(0.5)
    pos, tri, uv = S.tex_grid_mesh(tex_cases.CELLS)
    sd.add_mesh(pos, tri, bsdf=white, face_normals=True, name="floor", texcoords=uv)
    pos, tri, uv = boundary_strip()
    sd.add_mesh(pos, tri, bsdf=white, face_normals=True, name="strip", texcoords=uv)
    pos, tri, uv = huge_strip()
    sd.add_mesh(pos, tri, bsdf=white, face_normals=True, name="huge strip", texcoords=uv)
    g = S.vcol_grid(2, colors=None).meshes[0]
    sd.add_mesh(g.positions - F(4), g.triangles, bsdf=white, face_normals=True, name="no texcoords")
    sd.add_sphere(tex_cases.SPHERE_CENTER, tex_cases.SPHERE_RADIUS, bsdf=white)
    sd.point_light((0.3, 1.5, -0.2), (5.0, 4.0, 3.0))
    sd.camera = dict(origin=(0.0, 2.0, 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), ortho_scale=1.0)
    sd.max_depth = 2
    return sd


# --- the end-to-end bitmap ---------------------------------------------------------------------------------------------------
def palette():
    """PALETTE_N colours, each channel a power of two that no other entry has in that channel, none of them 1 (white's) -> [n][3]"""
    k = np.arange(1, PALETTE_N + 1)
    return np.stack([2.0 ** -k, 2.0 ** -np.roll(k, 5), 2.0 ** -np.roll(k[::-1], 3)], axis=1).astype(np.float32)


def palette_bitmap(wrap, transform="scaled"):
    """a 16 x 16 bitmap whose texels are drawn from the palette -> (ref64_bmp.Bmp, entry [16][16])"""
    entry = np.random.RandomState(77).randint(0, PALETTE_N, (16, 16))
    return R.Bmp(palette()[entry], wrap, *TRANSFORMS[transform]), entry


def _unstable(t, uvx, uvy, dx, dy):
    """the binary64 decision changes somewhere on the corners of the box uv +- (dx, dy)"""
    base = R.lookup(t, uvx, uvy, np.float64)
    out = np.zeros(len(base), dtype=bool)
    for sx in (-1, 1):
        for sy in (-1, 1):
            out |= R.lookup(t, uvx + sx * dx, uvy + sy * dy, np.float64) != base
    return base, out


class FloorGeometry(tex_cases._Ortho):
    """tex_cases.FloorGeometry with the bitmap's decision: scenes.tex_scene(shape="grid") under a bitmap.  out.cell is the
    binary64 cell of the exact hit; a sample is FRAGILE under tex_cases' bounds (the hit within the device's reach of a triangle
    edge, or the cell changing within the reach of its uv)"""

    def __init__(self, mts, t):
        S = mts.scenes
        tex_cases._Ortho.__init__(self, mts, S.tex_scene(scene_texture(S, t), shape="grid", cells=tex_cases.CELLS))
        self.tex = t
        self.mesh = self.sd.meshes[0]
        self.pos, self.tri = self.mesh.positions.astype(np.float64), self.mesh.triangles.astype(np.int64)
        self.uv = self.mesh.texcoords.astype(np.float64)
        self.s = 2.0 / tex_cases.CELLS

    def locate(self, raster):
        U24 = tex_cases.U24
        o, d_o = self.origin(raster)
        n, s, c = o.shape[0], self.s, tex_cases.CELLS
        px, pz = o[:, 0], o[:, 2]
        i = np.clip(np.floor((px + 1) / s), 0, c - 1).astype(np.int64)
        j = np.clip(np.floor((pz + 1) / s), 0, c - 1).astype(np.int64)
        out = tex_cases.Hit()
        out.p = np.stack([px, np.zeros(n), pz], axis=1)
        out.prim = np.zeros(n, dtype=np.int64); out.u = np.zeros(n); out.v = np.zeros(n)
        best = np.full(n, -np.inf)
        for k in range(2):
            prim = 2 * (i * c + j) + k
            A, B, C = (self.pos[self.tri[prim, m]] for m in range(3))
            e1, e2, q = B - A, C - A, out.p - A
            det = e1[:, 0] * e2[:, 2] - e1[:, 2] * e2[:, 0]
            u = (q[:, 0] * e2[:, 2] - q[:, 2] * e2[:, 0]) / det
            v = (e1[:, 0] * q[:, 2] - e1[:, 2] * q[:, 0]) / det
            inside = np.minimum(np.minimum(u, v), 1 - u - v)
            take = inside > best
            best = np.where(take, inside, best)
            out.prim[take] = prim[take]; out.u[take] = u[take]; out.v[take] = v[take]
        d_b = (d_o[:, 0] + d_o[:, 2] + 2 * U24 * s) / s + 3 * U24
        T = self.uv[self.tri[out.prim]]                                       # [n][3][2]
        out.uv = T[:, 0] * (1 - out.u - out.v)[:, None] + T[:, 1] * out.u[:, None] + T[:, 2] * out.v[:, None]
        spread = np.abs(T[:, 1] - T[:, 0]) + np.abs(T[:, 2] - T[:, 0])
        d_uv = d_b[:, None] * spread + 3 * U24 * np.abs(T).max(axis=1)
        out.cell, unstable = _unstable(self.tex, out.uv[:, 0], out.uv[:, 1], d_uv[:, 0], d_uv[:, 1])
        out.fragile = unstable | (best <= 2 * d_b)
        out.hit = np.ones(n, dtype=bool)
        return out


class SphereGeometry(tex_cases._Ortho):
    """tex_cases.SphereGeometry with the bitmap's decision: scenes.tex_scene(shape="sphere") under a bitmap"""

    def __init__(self, mts, t):
        S = mts.scenes
        tex_cases._Ortho.__init__(self, mts, S.tex_scene(scene_texture(S, t), shape="sphere"))
        self.tex = t
        self.c = np.asarray(tex_cases.SPHERE_CENTER, dtype=np.float32).astype(np.float64)
        self.r = float(F(tex_cases.SPHERE_RADIUS))

    def locate(self, raster):
        U24 = tex_cases.U24
        o, d_o = self.origin(raster)
        dx, dz = o[:, 0] - self.c[0], o[:, 2] - self.c[2]
        h2 = self.r ** 2 - dx * dx - dz * dz
        out = tex_cases.Hit()
        out.hit = h2 > 0
        h = np.sqrt(np.where(out.hit, h2, 1.0))
        reach = np.maximum(d_o[:, 0], d_o[:, 2]) + 4 * U24 * 2.0
        d_h = (np.abs(dx) + np.abs(dz)) * reach / h + 4 * U24 * 2.0
        base = None
        unstable = np.zeros(len(h), dtype=bool)
        for sx in (0, -1, 1):
            for sy in (0, -1, 1):
                for sz in (0, -1, 1):
                    p = np.stack([o[:, 0] + sx * reach, self.c[1] + h + sy * d_h, o[:, 2] + sz * reach], axis=1)
                    pc = p - self.c
                    theta = np.arccos(np.clip(pc[:, 2] / self.r, -1, 1))
                    phi = np.arctan2(pc[:, 1], pc[:, 0]); phi = np.where(phi < 0, phi + 2 * np.pi, phi)
                    b = R.lookup(self.tex, phi * (0.5 / np.pi), theta / np.pi, np.float64)
                    if base is None:
                        base, out.p = b, p
                    unstable |= b != base
        out.cell = base
        out.fragile = out.hit & (unstable | (h < self.r / 100))
        out.fragile |= np.abs(h2) <= 2 * self.r * 2 * reach          # the silhouette: hit or miss is undecided
        return out
