"""The device phases of the kd-tree build (csrc/kdbuild_bin.hip, csrc/kdbuild_exact.hip) held to the binary64 truth of
tests/ref64_kd.py with no oracle and no host tree in between: trees built with gpu_binning / gpu_exact in the three
combinations over every scene x parameter set of tests/kd_cases.py, through all six properties and the same caps as the CPU
suite.  Then the builder's product shown sound by use as well as by construction: the device-built `sah` tree of each scene
handed to mtsgpu_trace_rays with the ray classes of tests/geom_cases.py, against the brute force of tests/ref64_geom.py.
(fuzz_0 has no ray truth: ref64_geom refuses triangles whose projection axis binary32 cannot decide.)
Run on the GPU box: pytest -m gpu"""
import ctypes as C

import numpy as np
import pytest

import geom_cases as GC
import kd_cases as KC
import ref64_geom as G

pytestmark = pytest.mark.gpu

PHASES = {"binning": (True, False), "exact": (False, True), "both": (True, True)}


@pytest.mark.parametrize("phases", list(PHASES))
@pytest.mark.parametrize("pname", list(KC.PARAMS))
@pytest.mark.parametrize("sname", KC.SCENES)
def test_device_trees_hold_every_property(gpu_lib, mts, sname, pname, phases):
    sd, _ = KC.scene(mts, sname)
    binning, exact = PHASES[phases]
    dev = mts.Scene(sd, kd_params=KC.kd_params(mts, pname), gpu_binning=binning, gpu_exact=exact)
    rep = KC.report(mts, sname, pname, dev)
    print(sname, pname, phases, {k: v for k, v in rep.share.items()}, {k: v for k, v in rep.left_out.items() if v[0]})
    f = KC.failures(rep, "device %s / %s / %s" % (phases, sname, pname))
    assert not f, "\n".join(f)


_truth = {}


def _rays_and_truth(mts, sname, dev):
    """the rays of geom_cases and what they hit: the shared case of the nine scenes, the same classes for cornell_c1"""
    if sname in GC.SCENES:
        c = GC.case(mts, sname)
        return c.rays, c.closest, c.shadow
    if sname not in _truth:
        geom = G.Geometry(KC.scene(mts, sname)[0], list(dev.sc.aabb_min), list(dev.sc.aabb_max))
        rays = np.concatenate(list(GC.ray_classes(geom, [], seed=len(GC.SCENES) + 1).values()))
        _truth[sname] = (rays, G.trace(geom, rays, shadow=False), G.trace(geom, rays, shadow=True))
    return _truth[sname]


@pytest.mark.parametrize("sname", [s for s in KC.SCENES if s != "fuzz_0"])
def test_device_built_tree_traces_to_the_truth(gpu_lib, mts, sname):
    sd, _ = KC.scene(mts, sname)
    dev = mts.Scene(sd, gpu_binning=True, gpu_exact=True)
    f = KC.failures(KC.report(mts, sname, "defaults", dev), "device both / %s" % sname)
    rays, closest, shadow = _rays_and_truth(mts, sname, dev)
    it = mts.MIPathTracer(maxDepth=2)
    what = "%s / device-built sah tree" % sname
    try:
        rc = mts.lib().mtsgpu_upload_scene(it._ctx, C.byref(dev.sc))
        assert rc == 0, mts.lib().mtsgpu_last_error(it._ctx)
        more, worst = GC.check_closest(closest, it.trace_rays(rays), what)
        f += more + GC.check_shadow(shadow, it.trace_rays(rays, shadow=True), what)
    finally:
        it.close()
    print(what, "worst |device - truth| / bound", {k: round(v[0], 3) for k, v in worst.items()})
    assert not f, "\n".join(f)
