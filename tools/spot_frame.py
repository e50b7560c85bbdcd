"""What the spot kernels cost on a frame, tools/cloth_frame.py style: C1's box under a spot luminaire with a 16 x 16 bitmap as its
projection texture (bilinear lookup), with a checkerboard, and with the constant texture -- the frame the plain kernels render --
alternating in one process.  The films differ (another light), so the comparison base is the constant-texture frame of the same run:
python3 tools/spot_frame.py [res [spp]]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import _pkgload
pkg = _pkgload.load()
S = pkg.scenes
res, spp = (int(a) for a in (sys.argv[1:3] + ["512", "16"][len(sys.argv[1:3]):])[:2])
TEXELS = np.random.RandomState(1).uniform(0.1, 1.0, (16, 16, 3)).astype(np.float32)


def scene(kind):
    sd = S.cornell_c1()
    sd.name = "spot frame " + kind
    tex = {"constant": None, "checkerboard": S.Checkerboard(bright=1.0, dark=0.2, uscale=6.0, vscale=6.0),
           "bitmap, bilinear": S.BitmapTexture(texels=TEXELS, wrap="repeat", uscale=2.0, vscale=2.0)}[kind]
    sd.spot_light((0.0, 1.9, 0.3), (0.0, 0.0, 0.0), 30.0, cutoff_deg=50.0, beam_deg=35.0, texture=tex, bilinear=kind.endswith("bilinear"))
    sd.max_depth = 5
    return sd


for name in ("constant", "checkerboard", "bitmap, bilinear") * 2:
    sd = scene(name)
    sc = pkg.Scene(sd)
    assert (sc.spot_texture_args() is not None) == (name != "constant")
    cam = pkg.PerspectiveCamera.for_description(sd, res, res)
    it = pkg.MIPathTracer(maxDepth=sd.max_depth)
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
    print("%-17s (%dx%d, %d spp): frames %s ms, best %.2f | traversal %.2f ms, shading %.2f ms, avg path length %.2f, mean radiance %.4f"
          % (name, res, res, spp, " ".join("%.2f" % t for t in times), min(times), st["trace_ms"], st["shade_ms"], st["avg_path_length"],
             float(it.film()[..., :3].mean())), flush=True)
