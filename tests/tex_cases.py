"""Inputs shared by tests/test_tex.py (CPU) and tests/test_gpu_tex.py (device), as small as they can be and still go wrong:
a 4 x 4-cell planar grid with per-triangle vertices and texcoords that jump across every edge and reach below zero, a strip
of triangles whose first vertex carries the boundary texcoords (0, +-0.5, +-1, the edges of a grid line, and their binary32
neighbours), one sphere, and textures with scales of +-3.7 and offsets of +-0.3.  Also the closed-form geometry of the
end-to-end scenes under their orthographic camera, so that what the device test leaves out is decided by the CPU side and the
restatement alone.  Test infrastructure."""
import numpy as np

import ref64_tex as R

F = np.float32
CELLS, E2E_RES, E2E_SPP = 4, 48, 4
MAX_FRAGILE = 1.0e-3              # the film truth's cap
U24 = 2.0 ** -24
LINE_WIDTH = F(0.125)             # exact in binary32, so that a texcoord can sit exactly on a line's edge
SPHERE_CENTER, SPHERE_RADIUS = (0.05, -0.1, -0.02), 0.8      # scenes.tex_scene(shape="sphere")


def textures():
    """name -> ref64_tex.Tex: both kinds with uscale, vscale = +-3.7 and offsets = +-0.3 in all four sign patterns that
    matter, and the identity transform for the boundary records"""
    pow2 = dict(bright=(1.0, 0.5, 0.25), dark=(0.125, 0.25, 0.5))
    return {
        "checker": R.Tex(R.CHECKERBOARD, 0.3, -0.3, 3.7, -3.7, **pow2),
        "checker_neg": R.Tex(R.CHECKERBOARD, -0.3, 0.3, -3.7, 3.7, **pow2),
        "checker_id": R.Tex(R.CHECKERBOARD, **pow2),
        "grid": R.Tex(R.GRID, -0.3, 0.3, 3.7, -3.7, line_width=LINE_WIDTH, **pow2),
        "grid_neg": R.Tex(R.GRID, 0.3, -0.3, -3.7, 3.7, line_width=LINE_WIDTH, **pow2),
        "grid_id": R.Tex(R.GRID, line_width=LINE_WIDTH, **pow2),
    }


def scene_texture(S, t):
    """the scenes.Checkerboard / GridTexture of a ref64_tex.Tex"""
    kw = dict(bright=t.bright, dark=t.dark, uoffset=t.uoffset, voffset=t.voffset, uscale=t.uscale, vscale=t.vscale)
    return S.Checkerboard(**kw) if t.kind == R.CHECKERBOARD else S.GridTexture(line_width=t.line_width, **kw)


def boundary_values():
    """texcoords on the decisions' boundaries and one binary32 step to either side"""
    lw = float(LINE_WIDTH)
    base = [0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, lw, -lw, 1.0 - lw, 1.0 + lw, -1.0 + lw, -1.0 - lw, 0.25, -0.25]
    out = []
    for b in base:
        b = F(b)
        out += [b, np.nextafter(b, F(np.inf)), np.nextafter(b, F(-np.inf))]
    return np.array(out, dtype=np.float32)


def boundary_strip():
    """one small triangle per pair of boundary values (x, y), far from the floor: vertex 0 carries the texcoord (x, y), so
    that the record (u, v) = (0, 0) gives its.uv = (x, y) exactly (b = (1, 0, 0)) -> positions, triangles, texcoords"""
    b = boundary_values()
    bx, by = np.meshgrid(b, b[:18], indexing="ij")
    t0 = np.stack([bx.ravel(), by.ravel()], axis=1).astype(np.float32)
    n = t0.shape[0]
    k = np.arange(n, dtype=np.float32)
    base = np.stack([F(5) + F(0.01) * k, np.zeros(n, dtype=np.float32), np.full(n, F(5))], axis=1)
    pos = np.stack([base, base + np.float32([0.008, 0, 0]), base + np.float32([0, 0, 0.008])], axis=1).reshape(-1, 3)
    uv = np.stack([t0, t0 + np.float32([0.3, 0.1]), t0 + np.float32([-0.2, 0.4])], axis=1).reshape(-1, 2)
    return pos.astype(np.float32), np.arange(3 * n, dtype=np.uint32).reshape(-1, 3), uv.astype(np.float32)


def hook_scene(mts):
    """shape 0: the floor grid, shape 1: the boundary strip, shape 2: a mesh WITHOUT texcoords, shape 3: the sphere"""
    S = mts.scenes
    sd = S.SceneDescription("tex_hook")
    white = sd.lambertian(0.5)
    pos, tri, uv = S.tex_grid_mesh(CELLS)
    sd.add_mesh(pos, tri, bsdf=white, face_normals=True, name="floor", texcoords=uv)
    pos, tri, uv = boundary_strip()
    sd.add_mesh(pos, tri, bsdf=white, face_normals=True, name="strip", texcoords=uv)
    g = S.vcol_grid(2, colors=None).meshes[0]
    sd.add_mesh(g.positions - F(4), g.triangles, bsdf=white, face_normals=True, name="no texcoords")
    sd.add_sphere(SPHERE_CENTER, SPHERE_RADIUS, bsdf=white)
    sd.point_light((0.3, 1.5, -0.2), (5.0, 4.0, 3.0))
    sd.camera = dict(origin=(0.0, 2.0, 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), ortho_scale=1.0)
    sd.max_depth = 2
    return sd


def triangle_records(rng, first, count, n):
    """vcol_cases.barycentric_records for the primitives first .. first + count"""
    import vcol_cases
    prim, u, v = vcol_cases.barycentric_records(rng, count, n)
    return (prim + np.uint32(first)).astype(np.uint32), u, v


def sphere_points(rng, n, center=SPHERE_CENTER, radius=SPHERE_RADIUS):
    """binary32 world points on the sphere: random ones, the poles, the seam phi = 0 | 2 pi from both sides, the equator"""
    d = rng.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1, keepdims=True)
    special = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [1, 1e-7, 0], [1, -1e-7, 0],
                        [-1, 1e-7, 0], [-1, -1e-7, 0], [0.6, 0, 0.8], [0.6, -0.0, -0.8]], dtype=np.float64)
    d[:len(special)] = special
    return (np.asarray(center, dtype=np.float32) + (F(radius) * d.astype(np.float32))).astype(np.float32)


# --- the end-to-end scenes under their camera ------------------------------------------------------------------------------
class Hit:
    pass


class _Ortho:
    """raster position -> the ray's x and z (the camera looks straight down, orthographic.cpp:104-118) in binary64, and a
    bound on how far the device's binary32 transforms can move them (vcol_cases.GridGeometry derives it)"""

    def __init__(self, mts, sd):
        self.sd = sd
        cam = mts.PerspectiveCamera.for_description(sd, E2E_RES, E2E_RES)
        self.M1 = np.array(list(cam.c.raster_to_camera), dtype=np.float64).reshape(4, 4)
        self.M2 = np.array(list(cam.c.camera_to_world), dtype=np.float64).reshape(4, 4)
        assert cam.c.kind == 1 and self.M2[:3, 2].tolist() == [0.0, -1.0, 0.0]

    def origin(self, raster):
        r = np.asarray(raster, dtype=np.float32).astype(np.float64)
        n = r.shape[0]
        h4 = np.concatenate([r, np.zeros((n, 1)), np.ones((n, 1))], axis=1)
        ic = h4 @ self.M1.T
        d_ic = 5 * U24 * (np.abs(h4) @ np.abs(self.M1).T)[:, :3]
        ic[:, 3] = 1.0
        o = ic @ self.M2.T
        d_o = d_ic @ np.abs(self.M2[:3, :3]).T + 5 * U24 * (np.abs(ic) @ np.abs(self.M2).T)[:, :3]
        return o[:, :3], d_o


def _unstable(tex, uvx, uvy, dx, dy):
    """the binary64 decision changes somewhere on the corners of the box uv +- (dx, dy)"""
    base = R.at_uv(tex, uvx, uvy, np.float64)
    out = np.zeros(len(base), dtype=bool)
    for sx in (-1, 1):
        for sy in (-1, 1):
            out |= R.at_uv(tex, uvx + sx * dx, uvy + sy * dy, np.float64) != base
    return base, out


class FloorGeometry(_Ortho):
    """scenes.tex_scene(shape="grid"): the ray of a raster position meets the plane y = 0 below it.  A sample is FRAGILE when
    its exact hit lies within the device's reach of a triangle edge (the texcoords jump there), or when the binary64 decision
    changes within the reach of its uv: the hit moves by at most d_o, the barycentrics by that over the cell size plus three
    roundings (vcol_cases), uv by that times the texcoord spread of the triangle plus the three roundings of the
    interpolation."""

    def __init__(self, mts, tex):
        S = mts.scenes
        _Ortho.__init__(self, mts, S.tex_scene(scene_texture(S, tex), shape="grid", cells=CELLS))
        self.tex = tex
        self.mesh = self.sd.meshes[0]
        self.pos, self.tri = self.mesh.positions.astype(np.float64), self.mesh.triangles.astype(np.int64)
        self.uv = self.mesh.texcoords.astype(np.float64)
        self.s = 2.0 / CELLS

    def locate(self, raster):
        o, d_o = self.origin(raster)
        n, s, c = o.shape[0], self.s, CELLS
        px, pz = o[:, 0], o[:, 2]
        i = np.clip(np.floor((px + 1) / s), 0, c - 1).astype(np.int64)
        j = np.clip(np.floor((pz + 1) / s), 0, c - 1).astype(np.int64)
        out = Hit()
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
        out.bright, unstable = _unstable(self.tex, out.uv[:, 0], out.uv[:, 1], d_uv[:, 0], d_uv[:, 1])
        out.fragile = unstable | (best <= 2 * d_b)
        out.hit = np.ones(n, dtype=bool)
        return out


class SphereGeometry(_Ortho):
    """scenes.tex_scene(shape="sphere"): the ray of a raster position meets the sphere at y = c.y + sqrt(r^2 - dx^2 - dz^2).
    The device's point has the ray's x and z (d_o off at most) and y = o.y - t with t from Sphere::rayIntersect's binary64
    quadratic rounded once; the exact height moves by (|dx| + |dz|) d_o / h with the footpoint.  A sample is FRAGILE when the
    binary64 decision changes on the box of that size around the hit, when the ray passes within d_o of the silhouette, or
    when h < r / 100 (the bound on the height is first order only)."""

    def __init__(self, mts, tex):
        S = mts.scenes
        _Ortho.__init__(self, mts, S.tex_scene(scene_texture(S, tex), shape="sphere"))
        self.tex = tex
        self.c = np.asarray(SPHERE_CENTER, dtype=np.float32).astype(np.float64)
        self.r = float(F(SPHERE_RADIUS))

    def locate(self, raster):
        o, d_o = self.origin(raster)
        dx, dz = o[:, 0] - self.c[0], o[:, 2] - self.c[2]
        h2 = self.r ** 2 - dx * dx - dz * dz
        out = Hit()
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
                    # binary64 throughout: sphere_uv takes the points as they are when dtype is float64
                    pc = p - self.c
                    theta = np.arccos(np.clip(pc[:, 2] / self.r, -1, 1))
                    phi = np.arctan2(pc[:, 1], pc[:, 0]); phi = np.where(phi < 0, phi + 2 * np.pi, phi)
                    b = R.at_uv(self.tex, phi * (0.5 / np.pi), theta / np.pi, np.float64)
                    if base is None:
                        base, out.p = b, p
                    unstable |= b != base
        out.bright = base
        out.fragile = out.hit & (unstable | (h < self.r / 100))
        out.fragile |= np.abs(h2) <= 2 * self.r * 2 * reach          # the silhouette: hit or miss is undecided
        return out
