"""What an unfiltered bitmap in a slot costs on a frame, next to tools/tex_frame.py: the bench's C3 scene (1 M triangles, 1024 x 1024,
64 spp, `path`) with its walls mesh once with the constant reflectance, once with a checkerboard and once with a 1024 x 1024 bitmap
(16 MiB of texels in HBM) whose colours all equal that constant -- the same paths bit for bit, so the difference is the kernels' own
cost: the descriptor, the lookup and, for the bitmap, one 16-byte gather per textured hit from a pool that no cache holds.  `bitmap`
is the same bitmap with random texels around the constant (other albedos, other path lengths):
python3 tools/bmp_frame.py [grid [res [spp [texels]]]]"""
import os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import _pkgload
pkg = _pkgload.load()
S = pkg.scenes
grid, res, spp, size = (int(a) for a in (sys.argv[1:] + ["320", "1024", "64", "1024"][len(sys.argv) - 1:])[:4])


def scene(reflectance):
    sd = S.cornell_c3(grid=grid)
    walls = sd.meshes[0]
    c = float(sd.bsdf_params[walls.bsdf][0])
    p = walls.positions
    walls.texcoords = np.stack([p[:, 0] + np.float32(0.5) * p[:, 1], p[:, 2] + np.float32(0.5) * p[:, 1]], axis=1).astype(np.float32)
    if reflectance == "checker_equal":
        tex = S.Checkerboard(bright=c, dark=c, uscale=4.0, vscale=4.0, uoffset=0.3)
    elif reflectance == "bitmap_equal":
        tex = S.BitmapTexture(texels=np.full((size, size, 3), c, dtype=np.float32), uscale=4.0, vscale=4.0, uoffset=0.3)
    elif reflectance == "bitmap":
        tx = np.random.RandomState(1).uniform(0.6 * c, min(1.0, 1.4 * c), (size, size, 3)).astype(np.float32)
        tex = S.BitmapTexture(texels=tx, uscale=4.0, vscale=4.0, uoffset=0.3)
    else:
        return sd
    walls.bsdf = sd.lambertian(tex)
    return sd


films = {}
for name in ("constant", "checker_equal", "bitmap_equal", "bitmap", "constant", "checker_equal", "bitmap_equal"):
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
    print("%-13s (%d tris, %dx%d, %d spp): frames %s ms, best %.1f | traversal %.1f ms, shading %.1f ms, avg path length %.2f"
          % (name, sd.n_tris, res, res, spp, " ".join("%.1f" % t for t in times), min(times), st["trace_ms"], st["shade_ms"], st["avg_path_length"]), flush=True)
for name in ("checker_equal", "bitmap_equal"):
    print("film of `%s` == film of `constant`, bit for bit:" % name, bool(np.array_equal(films[name].view(np.uint32), films["constant"].view(np.uint32))))
