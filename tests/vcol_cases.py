"""Inputs shared by tests/test_vcol.py (CPU) and tests/test_gpu_vcol.py (device): the (primitive, u, v) records of the
interpolation check, and the closed-form geometry of the end-to-end scene (scenes.vcol_grid under its orthographic camera),
so that what the device test excludes is decided by the CPU side and the restatement alone.  Test infrastructure."""
import numpy as np

F = np.float32
E2E_CELLS, E2E_RES, E2E_SPP = 4, 32, 4
MAX_EXCLUDED = 0.01
U24 = 2.0 ** -24                  # unit roundoff of binary32


def barycentric_records(rng, n_prims, n):
    """random (prim, u, v) inside the triangle, with the three edges and the three corners among them: u = 0, v = 0,
    u + v = 1 (u a multiple of 2^-12, so that 1 - u is exact), (0, 0), (1, 0), (0, 1)"""
    prim = rng.randint(0, n_prims, n).astype(np.uint32)
    a, b = rng.rand(n), rng.rand(n)
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    u, v = a.astype(np.float32), b.astype(np.float32)
    over = u + v > F(1)                     # the rounding to binary32 may push a point over the edge: pull it back in
    v[over] = F(1) - u[over]
    k = np.arange(n) % 16
    u[k == 0] = 0; v[k == 1] = 0
    e = k == 2
    u[e] = (np.floor(u[e] * 4096) / 4096).astype(np.float32); v[e] = F(1) - u[e]
    u[k == 3] = 0; v[k == 3] = 0
    u[k == 4] = 1; v[k == 4] = 0
    u[k == 5] = 0; v[k == 5] = 1
    return prim, u, v


class Hit:
    pass


class GridGeometry:
    """scenes.vcol_grid(E2E_CELLS) seen by its orthographic camera at E2E_RES x E2E_RES: raster position -> the hit.

    The camera looks straight down: the ray of raster position (x, y) is o = cameraToWorld(rasterToCamera(x, y, 0)),
    d = (0, -1, 0) (orthographic.cpp:104-118), and it meets the plane y = 0 at (o.x, 0, o.z) whatever t is.  The device
    evaluates the two transforms in binary32 (three products and three sums per coordinate each) and TriAccel::rayIntersect
    (triaccel.h:139-157); how far its (u, v) can lie from the exact barycentrics of the exact point is bounded like this:

      transform 1   |d ic| <= 5 U * (|M1| |(x, y, 0, 1)|)                 (a 4-term dot product: gamma_5 of its absolute terms)
      transform 2   |d o|  <= |M2| |d ic| + 5 U * (|M2| |(ic, 1)|)
      hu = o_u + t * 0 - a_u, hv likewise: one rounding each, |hu|, |hv| <= the cell size s
      u = hv * b_nu + hu * b_nv, v = hu * c_nu + hv * c_nv with |b_n*|, |c_n*| <= 1 / s (legs along the axes): three roundings
      =>  |du|, |dv| <= (|d o_x| + |d o_z| + 2 U s) / s + 3 U

    with U = 2^-24.  `reach` is that bound; a sample is excluded when its exact hit lies within `reach` of an edge of its
    triangle (the device may then find the neighbour)."""

    def __init__(self, mts, material="lambertian"):
        self.sd = mts.scenes.vcol_grid(E2E_CELLS, material=material)
        self.mesh = self.sd.meshes[0]
        cam = mts.PerspectiveCamera.for_description(self.sd, E2E_RES, E2E_RES)
        self.camera = cam
        self.M1 = np.array(list(cam.c.raster_to_camera), dtype=np.float64).reshape(4, 4)
        self.M2 = np.array(list(cam.c.camera_to_world), dtype=np.float64).reshape(4, 4)
        assert cam.c.kind == 1
        # straight down, exactly: d = cameraToWorld(0, 0, 1)
        assert self.M2[:3, 2].tolist() == [0.0, -1.0, 0.0], self.M2
        assert (self.M1[3] == [0, 0, 0, 1]).all() and (self.M2[3] == [0, 0, 0, 1]).all()
        self.s = 2.0 / E2E_CELLS
        self.pos = self.mesh.positions.astype(np.float64)
        self.tri = self.mesh.triangles.astype(np.int64)

    def locate(self, raster):
        """raster [n][2] float32 -> Hit with p [n][3], prim, u, v (binary64), du = dv = reach [n], excluded [n]"""
        r = np.asarray(raster, dtype=np.float32).astype(np.float64)
        n = r.shape[0]
        h4 = np.concatenate([r, np.zeros((n, 1)), np.ones((n, 1))], axis=1)
        ic = h4 @ self.M1.T
        d_ic = 5 * U24 * (np.abs(h4) @ np.abs(self.M1).T)[:, :3]
        ic[:, 3] = 1.0
        o = ic @ self.M2.T
        d_o = d_ic @ np.abs(self.M2[:3, :3]).T + 5 * U24 * (np.abs(ic) @ np.abs(self.M2).T)[:, :3]
        s, c = self.s, E2E_CELLS
        px, pz = o[:, 0], o[:, 2]
        i = np.clip(np.floor((px + 1) / s), 0, c - 1).astype(np.int64)
        j = np.clip(np.floor((pz + 1) / s), 0, c - 1).astype(np.int64)
        out = Hit()
        out.p = np.stack([px, np.zeros(n), pz], axis=1)
        out.prim = np.zeros(n, dtype=np.int64); out.u = np.zeros(n); out.v = np.zeros(n)
        best = np.full(n, -np.inf)
        for k in range(2):                   # the two triangles of the cell: the one that holds the point
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
        out.du = (d_o[:, 0] + d_o[:, 2] + 2 * U24 * s) / s + 3 * U24
        out.dv = out.du
        out.excluded = best <= 2 * out.du       # 1 - u - v moves by du + dv
        return out

    def point(self, prim, u, v):
        A, B, C = (self.pos[self.tri[prim, m]] for m in range(3))
        return A * (1 - u - v)[:, None] + B * u[:, None] + C * v[:, None]
