"""What a uv-textured slot costs on a frame, tools/config_frames.py style: the bench's C3 scene (1 M triangles, 1024 x 1024, 64 spp,
`path`) with its walls mesh -- floor, ceiling and walls are one mesh with one Lambertian -- once with the constant reflectance, once
with a checkerboard whose bright and dark colours both equal that constant (the texture kernels on the SAME paths, bit for bit: the
difference is the kernels' own cost) and once with a real checkerboard (other albedos, other path lengths):
python3 tools/tex_frame.py [grid [res [spp]]]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import _pkgload
pkg = _pkgload.load()
S = pkg.scenes
grid, res, spp = (int(a) for a in (sys.argv[1:] + ["320", "1024", "64"][len(sys.argv) - 1:])[:3])


def scene(reflectance):
    sd = S.cornell_c3(grid=grid)
    walls = sd.meshes[0]
    c = float(sd.bsdf_params[walls.bsdf][0])
    p = walls.positions
    walls.texcoords = np.stack([p[:, 0] + np.float32(0.5) * p[:, 1], p[:, 2] + np.float32(0.5) * p[:, 1]], axis=1).astype(np.float32)
    tex = {"constant": None, "equal": S.Checkerboard(bright=c, dark=c, uscale=4.0, vscale=4.0, uoffset=0.3),
           "checker": S.Checkerboard(bright=min(1.0, 1.4 * c), dark=0.6 * c, uscale=4.0, vscale=4.0, uoffset=0.3)}[reflectance]
    if tex is not None:
        walls.bsdf = sd.lambertian(tex)
    return sd


films = {}
for name in ("constant", "equal", "checker", "constant", "equal"):
    sd = scene(name)
    sc = pkg.Scene(sd)
    cam = pkg.PerspectiveCamera.for_description(sd, res, res)
    it = pkg.MIPathTracer(maxDepth=sd.max_depth, rrDepth=sd.rr_depth)
    it.preprocess(sc, cam, sampler="ldsampler", sampleCount=spp, seed=0x5EED)
    assert it.render()
    films[name] = it.film().copy()
    times = []
    for timing in (False, False, False, True):
        it.set_options(time_kernels=timing)
        it.clear_film()
        t0 = time.perf_counter(); assert it.render(); dt = (time.perf_counter() - t0) * 1e3
        if not timing: times.append(dt)
    st = it.stats()
    print("%-8s (%d tris, %dx%d, %d spp): frames %s ms, best %.1f | traversal %.1f ms, shading %.1f ms, avg path length %.2f"
          % (name, sd.n_tris, res, res, spp, " ".join("%.1f" % t for t in times), min(times), st["trace_ms"], st["shade_ms"], st["avg_path_length"]), flush=True)
print("film of `equal` == film of `constant`, bit for bit:", bool(np.array_equal(films["equal"].view(np.uint32), films["constant"].view(np.uint32))))
