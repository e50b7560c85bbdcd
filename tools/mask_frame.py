"""What the mask kernels cost on a frame, tools/tex_frame.py style: the bench's C3 scene (1 M triangles, 1024 x 1024, 64 spp, `path`)
as it is, and with mask(1.0) on every BSDF -- opacity one takes the nested BSDF every time and multiplies and divides by 1, so the
mask kernels run on the SAME paths, bit for bit, and the difference is the family's own cost:
python3 tools/mask_frame.py [grid [res [spp]]]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import _pkgload
pkg = _pkgload.load()
S = pkg.scenes
grid, res, spp = (int(a) for a in (sys.argv[1:] + ["320", "1024", "64"][len(sys.argv) - 1:])[:3])


def scene(masked):
    sd = S.cornell_c3(grid=grid)
    if masked:
        for b in range(len(sd.bsdf_type)):
            sd.mask(b, 1.0)
    return sd


films = {}
for name in ("plain", "masked", "plain", "masked"):
    sd = scene(name == "masked")
    sc = pkg.Scene(sd)
    assert (sc.bsdf_mask is not None) == (name == "masked")
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
print("film of `masked` == film of `plain`, bit for bit:", bool(np.array_equal(films["masked"].view(np.uint32), films["plain"].view(np.uint32))))
