"""The recorder of tests/test_upload_plan.py: the calls a driver's preprocess() makes on the library, without a GPU.  A proxy
stands in for the cached library object; it forwards the context-free symbols (flattening, the flat scene's read-outs, the
*_configure calls, the cameras, mtsgpu_last_error), answers 0 to every create / destroy / set_* / upload_* call after writing
it down, and refuses everything else, so that no device is ever opened.  Test infrastructure.

A trace is a list of [call, args]: the C name without its mtsgpu_ / mtsgpu_group_ prefix, and for every argument after the
handle its value if it is a number, else "ptr" or "null".  (mtsgpu_create and mtsgpu_create_multi take no handle: all of their
arguments are written down.)

    python tests/upload_plan_cases.py > tests/golden/upload_plan.json

writes the fixture; that is done on the commit BEFORE a change to the drivers, never on the code under test."""
import contextlib
import ctypes as C
import json
import os
import sys

import numpy as np

FAKE_HANDLE = 0x1000       # what the proxy's create calls hand out; never passed to the library


def _holder(mts):
    """the module that holds the cached library object `_lib`"""
    return getattr(mts, "binding", mts)


def _strip(name):
    for prefix in ("mtsgpu_group_", "mtsgpu_"):
        if name.startswith(prefix):
            return name[len(prefix):]
    return name


def _context_free(name):
    return (name.startswith(("mtsgpu_flatten", "mtsgpu_flat_scene_", "mtsgpu_make_camera")) or name.endswith("_configure")
            or name == "mtsgpu_last_error")


def _recorded(name):
    call = _strip(name)
    return not _context_free(name) and (call in ("create", "create_multi", "destroy") or call.startswith(("set_", "upload_")))


def word(a):
    if isinstance(a, (bool, int, float, np.integer, np.floating)):
        return int(a) if int(a) == a else float(a)
    if a is None:
        return "null"
    if isinstance(a, C.c_void_p):
        return "ptr" if a.value else "null"
    if isinstance(a, C._Pointer):
        return "ptr" if a else "null"
    return "ptr"        # an array, a structure or a byref() of one


class Proxy:
    def __init__(self, real):
        self._real, self.trace = real, []

    def __getattr__(self, name):
        if _context_free(name):
            return getattr(self._real, name)
        if not _recorded(name):
            raise RuntimeError("%s needs a device: the recorder does not forward it" % name)
        getattr(self._real, name)       # the symbol exists
        call = _strip(name)

        def record(*args):
            makes = call in ("create", "create_multi")
            self.trace.append([call, [word(a) for a in (args if makes else args[1:])]])
            if makes:
                args[-1]._obj.value = FAKE_HANDLE
            return 0
        return record


@contextlib.contextmanager
def recording(mts):
    """the proxy in place of the library for the length of the block -> its trace"""
    real = mts.lib()
    holder = _holder(mts)
    assert holder._lib is real
    proxy = Proxy(real)
    holder._lib = proxy
    try:
        yield proxy.trace
    finally:
        holder._lib = real


def camera(mts):
    return mts.PerspectiveCamera((0.0, 1.0, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), 40.0, 16, 16)


def preprocess_trace(mts, make, scene):
    """(whole trace, the part preprocess() made) of make() ... preprocess(scene) ... close().  The driver is closed before the
    library comes back: its handle is the proxy's"""
    cam = camera(mts)
    with recording(mts) as trace:
        driver = make()
        try:
            first = len(trace)
            driver.preprocess(scene, cam, sampler="ldsampler", sampleCount=4, depth=3, seed=7)
            last = len(trace)
        finally:
            driver.close()
    return trace, trace[first:last]


BARE = "bare_pointer"       # the name of the case that hands preprocess() an abi.Scene pointer, not a Scene


def cloth_on_spheres(mts):
    """cloth on spheres only: no mesh has texcoords, so the uv-only texture call takes the zero pool"""
    import cloth_cases
    sd = mts.scenes.SceneDescription("cloth on spheres")
    sd.add_sphere((0.0, 0.4, 0.0), 0.4, bsdf=sd.irawan(cloth_cases.weaves(mts)[1][1], repeat_u=8.0, repeat_v=4.0))
    sd.add_sphere((0.9, 0.3, 0.0), 0.3, bsdf=sd.lambertian(0.5))
    sd.point_light((0.5, 1.5, 1.0), 4.0)
    sd.camera = dict(origin=(0.0, 1.0, 3.0), target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0), fov=40.0)
    return sd


def plan_scenes(mts):
    """[(name, description)]: the layout fixture's scenes, and what they lack for every branch of preprocess()"""
    import spot_cases
    import upload_cases
    S = mts.scenes
    chk = S.Checkerboard(bright=(1.0, 0.9, 0.8), dark=(0.25, 0.2, 0.1), uscale=4.0, vscale=4.0)
    out = [(n, sd[0] if isinstance(sd, tuple) else sd) for n, sd in upload_cases.layout_scenes(mts)]
    return out + [("spot_checker", spot_cases.e2e_description(mts, texture=chk)), ("cloth_on_spheres", cloth_on_spheres(mts))]


def record_all(mts):
    """name -> the trace of MIPathTracer.preprocess for every scene of plan_scenes(), and for the bare pointer"""
    out = {}
    for name, sd in plan_scenes(mts):
        scene = mts.Scene(sd)
        out[name] = preprocess_trace(mts, lambda: mts.MIPathTracer(maxDepth=5), scene)[1]
        if name == "cornell_c1":
            out[BARE] = preprocess_trace(mts, lambda: mts.MIPathTracer(maxDepth=5), scene.ptr)[1]
    return out


if __name__ == "__main__":
    import subprocess
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle")]
    import _pkgload
    rev = subprocess.check_output(["git", "-C", here, "rev-parse", "--short", "HEAD"]).decode().strip()
    rows = ['  "%s": %s' % (k, json.dumps(v, separators=(",", ":"))) for k, v in record_all(_pkgload.load()).items()]
    print('{\n "commit": "%s",\n "command": "python tests/upload_plan_cases.py",\n "traces": {\n%s\n }\n}' % (rev, ",\n".join(rows)))
