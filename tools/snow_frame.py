"""What the snow kernels cost on a frame, tools/mask_frame.py style: the bench's C3 scene (1 M triangles, 1024 x 1024, 64 spp, `path`)
as it is, and with the BSDF of its walls mesh -- the floor and the four walls are one mesh with one Lambertian -- replaced by a
Wiscombe and by a HanrahanKrueger with the reference's defaults, alternating in one process.  The films differ (another
material, other paths), so the comparison base is the Lambertian frame of the same run and the path lengths are printed:
python3 tools/snow_frame.py [grid [res [spp]]]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import _pkgload
pkg = _pkgload.load()
S = pkg.scenes
grid, res, spp = (int(a) for a in (sys.argv[1:] + ["320", "1024", "64"][len(sys.argv) - 1:])[:3])


def scene(material):
    sd = S.cornell_c3(grid=grid)
    if material != "lambertian":
        donor = S.SceneDescription("donor")
        b = donor.wiscombe() if material == "wiscombe" else donor.hanrahan_krueger()
        walls = sd.meshes[0].bsdf
        sd.bsdf_snow[walls] = donor.bsdf_snow[b]
        sd.bsdf_params[walls][:] = 0
    return sd


for name in ("lambertian", "wiscombe", "hk", "lambertian", "wiscombe", "hk"):
    sd = scene(name)
    sc = pkg.Scene(sd)
    assert (sc.bsdf_snow is not None) == (name != "lambertian")
    cam = pkg.PerspectiveCamera.for_description(sd, res, res)
    it = pkg.MIPathTracer(maxDepth=sd.max_depth, rrDepth=sd.rr_depth)
    it.preprocess(sc, cam, sampler="ldsampler", sampleCount=spp, seed=0x5EED)
    assert it.render()
    assert np.isfinite(it.film()).all()
    times = []
    for timing in (False, False, False, True):
        it.set_options(time_kernels=timing)
        it.clear_film()
        t0 = time.perf_counter(); assert it.render(); dt = (time.perf_counter() - t0) * 1e3
        if not timing: times.append(dt)
    st = it.stats()
    print("%-10s (%d tris, %dx%d, %d spp): frames %s ms, best %.1f | traversal %.1f ms, shading %.1f ms, avg path length %.2f, mean radiance %.4f"
          % (name, sd.n_tris, res, res, spp, " ".join("%.1f" % t for t in times), min(times), st["trace_ms"], st["shade_ms"], st["avg_path_length"],
             float(it.film()[..., :3].mean())), flush=True)
