"""What analytic cylinders cost on a frame, tools/mask_frame.py style: a forest of n x n upright Lambertian cylinders over a floor under
a point light and a constant environment, rendered with the cylinders as `cylinder` shapes (one kd-tree primitive each, the CYL
instantiations of k_trace) and with every cylinder replaced by the 40-triangle mesh of Cylinder::createTriMesh
(src/shapes/cylinder.cpp:377-415: 20 steps of phi, smooth normals), which runs the kernels every other scene runs:
python3 tools/cyl_frame.py [n [res [spp]]]          (64 -> 4 096 cylinders, 512, 16)"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import _pkgload
pkg = _pkgload.load()
S = pkg.scenes
n, res, spp = (int(a) for a in (sys.argv[1:] + ["64", "512", "16"][len(sys.argv) - 1:])[:3])
F = np.float32


def tri_mesh(p1, height, radius):
    """createTriMesh of an upright cylinder: vertices 2k (bottom), 2k + 1 (top) at phi = k * 2 pi / 20, with their normals"""
    steps = 20
    phi = np.arange(steps) * (2 * np.pi / steps)
    c, s = np.cos(phi), np.sin(phi)
    pos = np.zeros((2 * steps, 3)); nrm = np.zeros((2 * steps, 3))
    pos[0::2] = np.stack([p1[0] + radius * c, np.full(steps, p1[1]), p1[2] + radius * s], axis=1)
    pos[1::2] = pos[0::2] + [0, height, 0]
    nrm[0::2] = nrm[1::2] = np.stack([c, np.zeros(steps), s], axis=1)
    tri = []
    for k in range(steps):
        i0, i1 = 2 * k, 2 * k + 1
        i2 = (2 * k + 2) % (2 * steps); i3 = i2 + 1
        tri += [(i0, i2, i1), (i1, i2, i3)]
    return pos, np.array(tri), nrm


def scene(analytic):
    rng = np.random.RandomState(1)
    sd = S.SceneDescription("cyl_forest")
    grey, bark = sd.lambertian(0.6), sd.lambertian((0.5, 0.35, 0.2))
    sd.add_mesh([(-1.2, 0, -1.2), (1.2, 0, -1.2), (1.2, 0, 1.2), (-1.2, 0, 1.2)], [(0, 1, 2), (0, 2, 3)], bsdf=grey, face_normals=True, name="floor")
    g = (np.arange(n) + 0.5) / n * 2 - 1
    for x in g:
        for z in g:
            h, r = 0.2 + 0.5 * rng.rand(), (0.25 + 0.2 * rng.rand()) / n
            p1 = (x + 0.3 / n * (rng.rand() - 0.5), 0.0, z + 0.3 / n * (rng.rand() - 0.5))
            if analytic:
                sd.add_cylinder(p1, (p1[0], h, p1[2]), r, bsdf=bark)
            else:
                pos, tri, nrm = tri_mesh(p1, h, r)
                sd.add_mesh(pos, tri, bsdf=bark, face_normals=False, normals=nrm, name="cylinder mesh")
    sd.point_light((0.4, 2.5, 0.6), (8.0, 8.0, 8.0))
    sd.add_lum(pkg.abi.LUM_CONSTANT, [0.3, 0.3, 0.3])
    sd.camera = dict(origin=(0.0, 1.6, 2.6), target=(0.0, 0.2, 0.0), up=(0.0, 1.0, 0.0), fov=40.0)
    sd.max_depth = 8
    return sd


for name in ("analytic", "meshes", "analytic", "meshes"):
    sd = scene(name == "analytic")
    t0 = time.perf_counter(); sc = pkg.Scene(sd); build_ms = (time.perf_counter() - t0) * 1e3
    assert sc.has_cylinders == (name == "analytic")
    cam = pkg.PerspectiveCamera.for_description(sd, res, res)
    it = pkg.MIPathTracer(maxDepth=sd.max_depth)
    it.preprocess(sc, cam, sampler="independent", sampleCount=spp, seed=0x5EED)
    assert it.render()
    film = it.film()
    times = []
    for timing in (False, False, False, True):
        it.set_options(time_kernels=timing)
        it.clear_film()
        t0 = time.perf_counter(); assert it.render(); dt = (time.perf_counter() - t0) * 1e3
        if not timing: times.append(dt)
    st = it.stats()
    print("%-8s (%d primitives, %d nodes, %d leaf entries, host build %.0f ms; %dx%d, %d spp): frames %s ms, best %.1f | traversal %.1f ms, "
          "shading %.1f ms, closest rays %d, shadow rays %d, avg path length %.2f, mean radiance %.4f"
          % (name, sc.sc.n_tris, sc.sc.n_nodes, sc.sc.n_indices, build_ms, res, res, spp, " ".join("%.1f" % t for t in times), min(times),
             st["trace_ms"], st["shade_ms"], st["rays_closest"], st["rays_shadow"], st["avg_path_length"],
             float((film[..., :3].sum(axis=2) / np.maximum(film[..., 4], 1e-9)).mean())), flush=True)
