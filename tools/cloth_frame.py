"""What the cloth kernels cost on a frame, tools/snow_frame.py style: a box whose five faces and a sphere in it are draped in the
woven cloth of tests/golden/cloth_plain_2x2.weave (repeat 40 x 40), against the same box with those entries as plain Lambertians
of the yarns' mean kd, alternating in one process; and the cloth with period and fineness off against on, which is what the two
Random(seed) constructions per evaluation cost.  The films differ (another material), so the comparison base is the Lambertian
frame of the same run:
python3 tools/cloth_frame.py [res [spp [lambertian]]]      (with `lambertian` the base frame alone, which a tree without the cloth can run)"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import _pkgload
pkg = _pkgload.load()
S = pkg.scenes
res, spp = (int(a) for a in (sys.argv[1:3] + ["512", "16"][len(sys.argv[1:3]):])[:2])
only_base = len(sys.argv) > 3 and sys.argv[3] == "lambertian"
TEXT = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden", "cloth_plain_2x2.weave")).read()
UV = [(0, 0), (1, 0), (1, 1), (0, 1)]


def scene(material):
    sd = S.SceneDescription("cloth frame " + material)
    if material == "lambertian":
        bsdf = sd.lambertian(0.39, 0.39, 0.31)          # pi times the mean kd of the two yarns
    else:
        noise = material == "cloth, noise on"
        w = pkg.load_weave(TEXT, dict(fineness=2.0 if noise else 0.0, period=3.0 if noise else 0.0, weft_ks=(0.6, 0.7, 0.8)))
        bsdf = sd.irawan(w, repeat_u=40.0, repeat_v=40.0)
    for name, p0, e1, e2, nrm in S._box_faces():
        pos, tri = S._quad(p0, e1, e2, nrm)
        sd.add_mesh(pos, tri, bsdf=bsdf, face_normals=True, name=name, texcoords=UV)
    sd.add_sphere((0.3, 0.4, 0.1), 0.4, bsdf=bsdf)
    S._add_light(sd, intensity=4.0)
    sd.max_depth = 5
    return sd


for name in (("lambertian",) if only_base else ("lambertian", "cloth, noise off", "cloth, noise on")) * 2:
    sd = scene(name)
    sc = pkg.Scene(sd)
    assert (getattr(sc, "cloth", None) is not None) == (name != "lambertian")
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
