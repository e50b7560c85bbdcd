"""What a tangent mesh costs on a frame, tools/tex_frame.py style: the bench's C3 scene (1 M triangles, 1024 x 1024, 64 spp, `path`)
with planar texcoords and smooth normals on its walls mesh and a Ward BSDF there whose diffuse reflectance is a checkerboard of
two equal colours, so that the scene runs through the texture kernels: once isotropic (alphaU = alphaV = 0.2: the texture family),
once with alphaU nudged off alphaV (0.2 * (1 + 2^-10): the tangent family, on nearly the same paths).  The difference is the cost
of the tangent kernels: 48 bytes more per hit on the mesh and the frame's arithmetic.
python3 tools/tan_frame.py [grid [res [spp]]]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import _pkgload
pkg = _pkgload.load()
S = pkg.scenes
grid, res, spp = (int(a) for a in (sys.argv[1:] + ["320", "1024", "64"][len(sys.argv) - 1:])[:3])


def scene(nudged):
    sd = S.cornell_c3(grid=grid)
    walls = sd.meshes[0]
    c = float(sd.bsdf_params[walls.bsdf][0])
    p = walls.positions
    walls.texcoords = np.stack([p[:, 0] + np.float32(0.5) * p[:, 1], p[:, 2] + np.float32(0.5) * p[:, 1]], axis=1).astype(np.float32)
    walls.face_normals, walls.normals = False, None          # tangents need vertex normals; the flattener computes them
    tex = S.Checkerboard(bright=c, dark=c, uscale=4.0, vscale=4.0, uoffset=0.3)
    walls.bsdf = sd.ward(0.2 * (1 + 2.0 ** -10) if nudged else 0.2, 0.2, rd=tex, rs=0.3, kd=0.7, ks=0.3)
    return sd


for name in ("isotropic", "nudged", "isotropic", "nudged"):
    sd = scene(name == "nudged")
    sc = pkg.Scene(sd)
    assert sc.wants_tangents == (name == "nudged") and sc.bsdf_slot_texture is not None
    cam = pkg.PerspectiveCamera.for_description(sd, res, res)
    it = pkg.MIPathTracer(maxDepth=sd.max_depth, rrDepth=sd.rr_depth)
    it.preprocess(sc, cam, sampler="ldsampler", sampleCount=spp, seed=0x5EED)
    assert it.render()
    times = []
    for timing in (False, False, False, True):
        it.set_options(time_kernels=timing)
        it.clear_film()
        t0 = time.perf_counter(); assert it.render(); dt = (time.perf_counter() - t0) * 1e3
        if not timing: times.append(dt)
    st = it.stats()
    print("%-9s (%d tris, %dx%d, %d spp): frames %s ms, best %.1f | traversal %.1f ms, shading %.1f ms, avg path length %.2f"
          % (name, sd.n_tris, res, res, spp, " ".join("%.1f" % t for t in times), min(times), st["trace_ms"], st["shade_ms"], st["avg_path_length"]), flush=True)
