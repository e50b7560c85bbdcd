"""Inputs shared by tests/test_tan.py (CPU) and tests/test_gpu_tan.py (device), the smallest that reach every branch of
TriMesh::computeTangentSpaceBasis and of the tangent frame: a 4 x 4-quad floor whose uv is rotated by 27 degrees and sheared
(so that s is no axis), an 8 x 4 quarter-cylinder patch with smooth normals and uv = (angle, height), one small mesh that
collects the degenerate cases in exactly representable coordinates, and a scene that mixes a tangent mesh, an isotropic mesh
with texcoords, a mesh without texcoords and a sphere.  Test infrastructure."""
import numpy as np

F = np.float32
UV_ANGLE, UV_SHEAR = np.deg2rad(27.0), 0.35


def _grid(nu, nv):
    """vertex parameters [(nu + 1) * (nv + 1)][2] in [0, 1]^2 and the triangles of an nu x nv quad grid with shared vertices"""
    a, b = np.meshgrid(np.arange(nu + 1) / nu, np.arange(nv + 1) / nv, indexing="ij")
    idx = np.arange((nu + 1) * (nv + 1)).reshape(nu + 1, nv + 1)
    tri = []
    for i in range(nu):
        for j in range(nv):
            q = idx[i, j], idx[i + 1, j], idx[i + 1, j + 1], idx[i, j + 1]
            tri += [[q[0], q[2], q[1]], [q[0], q[3], q[2]]]
    return np.stack([a.ravel(), b.ravel()], axis=1), np.array(tri, dtype=np.uint32)


def floor(extent=1.0):
    """-> positions, triangles, normals, texcoords: the plane y = 0 over [-extent, extent]^2, normal +y,
    uv = R(27 deg) * [[1, 0.35], [0, 1]] * (x, z) / extent"""
    p, tri = _grid(4, 4)
    xz = (2 * p - 1)
    pos = np.stack([xz[:, 0] * extent, 0 * xz[:, 0], xz[:, 1] * extent], axis=1).astype(np.float32)
    c, s = np.cos(UV_ANGLE), np.sin(UV_ANGLE)
    M = np.array([[c, -s], [s, c]]) @ np.array([[1.0, UV_SHEAR], [0.0, 1.0]])
    uv = (xz @ M.T).astype(np.float32)
    nrm = np.tile(np.float32([0, 1, 0]), (len(pos), 1))
    return pos, tri, nrm, uv


def floor_tangent(extent=1.0):
    """the floor's exact dp/du (binary64, world space): constant, and no axis"""
    c, s = np.cos(UV_ANGLE), np.sin(UV_ANGLE)
    M = np.array([[c, -s], [s, c]]) @ np.array([[1.0, UV_SHEAR], [0.0, 1.0]])
    col = np.linalg.inv(M)[:, 0] * extent
    return np.array([col[0], 0.0, col[1]])


CYL_T0, CYL_T1, CYL_H = np.pi / 4, 3 * np.pi / 4, 1.0


def cylinder(radius=1.0):
    """-> positions, triangles, normals, texcoords: the quarter of a cylinder around the z axis that faces +y,
    p = (r cos a, r sin a, h), smooth normals (cos a, sin a, 0), uv = (a, h)"""
    p, tri = _grid(8, 4)
    a = CYL_T0 + (CYL_T1 - CYL_T0) * p[:, 0]
    h = CYL_H * (2 * p[:, 1] - 1)
    pos = np.stack([radius * np.cos(a), radius * np.sin(a), h], axis=1).astype(np.float32)
    nrm = np.stack([np.cos(a), np.sin(a), 0 * a], axis=1).astype(np.float32)
    return pos, tri[:, [0, 2, 1]].copy(), nrm, np.stack([a, h], axis=1).astype(np.float32)


def degenerate():
    """-> positions, triangles, normals, texcoords, names: one triangle (of its own three vertices) per case, small integers
    and halves throughout, so that binary32 and binary64 take the same branch:
      0 regular               a reference point
      1 zero uv determinant   collinear texcoords along u: dpdu comes out zero, recovered as cross(n, dpdv)
      2 dpdv zero             collinear texcoords along v: dpdv comes out zero, recovered as cross(dpdu, n)
      3 one texcoord          dpdu = dpdv = 0 and cross(n, 0) = 0: coordinateSystem(n)
      4 zero area, collinear  positions on a line, texcoords regular
      5 zero area, one point  dpdu = dpdv = 0 and no face normal: both stay zero, the vertices fall back to coordinateSystem
      6 zero vertex normal    a regular triangle whose first vertex has the normal (0, 0, 0)
    then vertex 21, which no triangle uses, and vertex 22, unused and with a zero normal"""
    names = ["regular", "zero uv determinant", "dpdv zero", "one texcoord", "zero area, collinear", "zero area, one point", "zero vertex normal"]
    base = lambda k: np.float32([4 * k, 0, 8])
    P = [[(0, 0, 0), (2, 0, 0), (0, 0, 2)]] * 4 + [[(0, 0, 0), (1, 0, 0), (3, 0, 0)], [(1, 0, 1), (1, 0, 1), (1, 0, 1)], [(0, 0, 0), (2, 0, 0), (0, 0, 2)]]
    T = [[(0, 0), (1, 0.5), (0.5, 2)], [(0, 0), (1, 0), (2, 0)], [(0, 0), (0, 1), (0, 2)], [(0.5, 0.25), (0.5, 0.25), (0.5, 0.25)],
         [(0, 0), (1, 0), (0, 1)], [(0, 0), (1, 0), (0, 1)], [(0, 0), (1, 0), (0, 1)]]
    pos = np.concatenate([np.float32(p) + base(k) for k, p in enumerate(P)] + [np.float32([[40, 0, 8], [44, 0, 8]])])
    uv = np.concatenate([np.float32(t) for t in T] + [np.float32([[0.25, 0.75], [0.5, 0.5]])])
    nrm = np.tile(np.float32([0, -1, 0]), (len(pos), 1))       # cross(+x, +z) of the reference = -y
    nrm[18] = 0
    nrm[21] = (0, 0.6, 0.8)
    nrm[22] = 0
    tri = np.arange(21, dtype=np.uint32).reshape(7, 3)
    return pos.astype(np.float32), tri, nrm.astype(np.float32), uv.astype(np.float32), names


WARD_ANISO = dict(alpha_x=0.1, alpha_y=0.3, rd=0.5, rs=0.5, kd=0.5, ks=0.5)
WARD_SWAPPED = dict(alpha_x=0.3, alpha_y=0.1, rd=0.5, rs=0.5, kd=0.5, ks=0.5)


def hook_scene(mts, isotropic=False):
    """shape 0: the floor (anisotropic Ward -> tangents), 1: the cylinder patch (a composite with an anisotropic Ward child),
    2: the degenerate mesh (twosided anisotropic Ward), 3: the floor again, lifted, with texcoords and an ISOTROPIC Ward,
    4: a mesh without texcoords, 5: a sphere with the anisotropic Ward, 6: the floor with face normals and the anisotropic Ward
    (texcoords, but no vertex normals: no tangents).  isotropic: every Ward with alphaU = alphaV, so no mesh has tangents"""
    S = mts.scenes
    sd = S.SceneDescription("tan_hook")
    kw = dict(WARD_ANISO, alpha_y=0.1) if isotropic else WARD_ANISO
    aniso = sd.ward(**kw)
    comp = sd.composite([0.4, 0.6], [sd.lambertian(0.5), sd.ward(**kw)])
    two = sd.twosided(sd.ward(**kw))
    iso = sd.ward(0.2, 0.2, rd=0.5, rs=0.5, kd=0.5, ks=0.5)
    white = sd.lambertian(0.5)
    pos, tri, nrm, uv = floor()
    sd.add_mesh(pos, tri, bsdf=aniso, face_normals=False, normals=nrm, texcoords=uv, name="floor")
    cp, ct, cn, cuv = cylinder()
    sd.add_mesh(cp + np.float32([0, 2, 0]), ct, bsdf=comp, face_normals=False, normals=cn, texcoords=cuv, name="cylinder")
    dp, dt, dn, duv, _ = degenerate()
    sd.add_mesh(dp, dt, bsdf=two, face_normals=False, normals=dn, texcoords=duv, name="degenerate")
    sd.add_mesh(pos + np.float32([0, -3, 0]), tri, bsdf=iso, face_normals=False, normals=nrm, texcoords=uv, name="isotropic")
    sd.add_mesh(pos + np.float32([0, -6, 0]), tri, bsdf=white, face_normals=False, normals=nrm, name="no texcoords")
    sd.add_sphere((5.0, 1.0, 0.0), 0.75, bsdf=aniso)
    sd.add_mesh(pos + np.float32([0, -9, 0]), tri, bsdf=aniso, face_normals=True, texcoords=uv, name="face normals")
    sd.point_light((0.3, 6.0, -0.2), (5.0, 4.0, 3.0))
    sd.camera = dict(origin=(0.0, 9.0, 0.0), target=(0.0, 0.0, 0.0), up=(0.0, 0.0, -1.0), fov=40.0)
    sd.max_depth = 2
    return sd


HOOK_FLAGS = [1, 1, 1, 0, 0, 0, 0]


def mixed_scene(mts, isotropic=False, sky=False, extra=None):
    """a small closed room for the film comparisons: the tangent floor (anisotropic Ward), a back wall with texcoords and an
    isotropic Ward, side walls without texcoords, a cylinder patch with a composite whose Ward child is anisotropic, a sphere
    with the anisotropic Ward, a glass sphere and a quad emitter.  extra: None, "checkerboard" (the left wall's reflectance)
    or "vertexcolors" (the right wall's)"""
    S = mts.scenes
    sd = S.SceneDescription("tan_mixed")
    kw = dict(WARD_ANISO, alpha_y=0.1) if isotropic else WARD_ANISO
    aniso = sd.ward(**kw)
    comp = sd.composite([0.4, 0.6], [sd.lambertian(0.7, 0.2, 0.2), sd.ward(**kw)])
    iso = sd.ward(0.15, 0.15, rd=(0.5, 0.4, 0.3), rs=0.4, kd=0.6, ks=0.4, model="ward-duer")
    left = sd.lambertian(S.Checkerboard(bright=(0.7, 0.6, 0.5), dark=0.1, uscale=2.5, vscale=2.5)) if extra == "checkerboard" else sd.lambertian(0.6)
    right = sd.lambertian(S.VERTEX_COLORS) if extra == "vertexcolors" else sd.lambertian(0.6)
    glass = sd.dielectric()
    pos, tri, nrm, uv = floor()
    sd.add_mesh(pos, tri, bsdf=aniso, face_normals=False, normals=nrm, texcoords=uv, name="floor")
    # the same grid turned into the walls: back (normal +z), left (+x), right (-x)
    back = np.stack([pos[:, 0], pos[:, 2] + 1, 0 * pos[:, 0] - 1], axis=1).astype(np.float32)
    sd.add_mesh(back, tri[:, [0, 2, 1]], bsdf=iso, face_normals=False, normals=np.tile(np.float32([0, 0, 1]), (len(pos), 1)), texcoords=uv, name="back")
    lw = np.stack([0 * pos[:, 0] - 1, pos[:, 2] + 1, pos[:, 0]], axis=1).astype(np.float32)
    sd.add_mesh(lw, tri, bsdf=left, face_normals=True, texcoords=uv if extra == "checkerboard" else None, name="left")
    rw = np.stack([0 * pos[:, 0] + 1, pos[:, 2] + 1, pos[:, 0]], axis=1).astype(np.float32)
    rng = np.random.RandomState(4)
    sd.add_mesh(rw, tri[:, [0, 2, 1]], bsdf=right, face_normals=True, colors=rng.uniform(0.2, 0.8, (len(pos), 3)) if extra == "vertexcolors" else None, name="right")
    cp, ct, cn, cuv = cylinder(0.3)
    sd.add_mesh(cp * np.float32([1, 1, 0.4]) + np.float32([-0.45, 0.0, 0.1]), ct, bsdf=comp, face_normals=False, normals=cn, texcoords=cuv, name="cylinder")
    sd.add_sphere((0.45, 0.3, 0.3), 0.3, bsdf=glass)
    sd.add_sphere((0.0, 0.25, -0.5), 0.25, bsdf=aniso)
    if sky:
        sd.sky(sun_direction=(0.3, 0.8, 0.5))
    lum = sd.add_lum(mts.abi.LUM_AREA, [12.0, 11.0, 9.0])
    lp, lt = S._quad((-0.3, 1.98, -0.3), (0.6, 0, 0), (0, 0, 0.6), (0, -1, 0))
    sd.add_mesh(lp, lt, bsdf=sd.lambertian(0.0), lum=lum, face_normals=True, name="light")
    sd.camera = dict(origin=(0.0, 1.0, 3.4), target=(0.0, 0.9, 0.0), up=(0.0, 1.0, 0.0), fov=39.3)
    return sd


MIXED_FLAGS = [1, 0, 0, 0, 1, 0, 0, 0]


def records(rng, first, count, n):
    """n records (prim, u, v) on the primitives first .. first + count: random interior points, then every primitive's corners
    and edge midpoints"""
    prim = rng.randint(0, count, n)
    a = rng.uniform(0, 1, (n, 2))
    flip = a.sum(axis=1) > 1
    a[flip] = 1 - a[flip]
    k = min(n, 6 * count)
    special = np.array([[0, 0], [1, 0], [0, 1], [0.5, 0], [0, 0.5], [0.5, 0.5]])
    prim[:k] = np.arange(k) // 6 % count
    a[:k] = special[np.arange(k) % 6]
    return (prim + first).astype(np.uint32), a[:, 0].astype(np.float32), a[:, 1].astype(np.float32)
