"""Scenes and parameter sets that hold the kd-tree builders (the oracle's and the host's in the CPU suite, the device phases in
the GPU suite) against tests/ref64_kd.py, and the planted errors the checker must name.  Test infrastructure.

Every scene holds a few hundred primitives at most.  The check is a pure function of the primitives, the tree and the
parameters: a tree that is word for word one already checked under the same parameters shares that report."""
import hashlib

import numpy as np

import geom_cases
import ref64_kd as K

SCENES = geom_cases.SCENES + ("cornell_c1", "fuzz_0")

# name -> KdParams fields.  small_exact / bins4: the binning phase runs on a dozen primitives (as in test_gpu_kdbuild.py)
PARAMS = {
    "defaults": {},
    "small_exact": dict(exact_prim_threshold=4, stop_prims=1),
    "bins4": dict(exact_prim_threshold=40, min_max_bins=4),
    "bins128": dict(min_max_bins=128),
    "noclip": dict(clip=-1),
    "noretract": dict(retract=-1),
    "depth3": dict(max_depth=3),
    "one_bad_refine": dict(max_bad_refines=1),
    "bonus_half": dict(empty_space_bonus=0.5),
    "dear_query": dict(traversal_cost=1, query_cost=40),
}

CAP = 0.01                       # the share of its cases a property may leave out as fragile, in any one scene
NO_FRAGILE = ("coverage", "tightness", "stats")

_scenes, _reports = {}, {}


def scene(mts, name):
    """-> (scene description, ref64_kd.Prims)"""
    if name not in _scenes:
        if name == "cornell_c1":
            sd = mts.scenes.cornell_c1()
        elif name == "fuzz_0":
            sd = mts.scenes.fuzz(0)
        else:
            sd = geom_cases.scene_description(mts, name)
        _scenes[name] = (sd, K.Prims(sd))
    return _scenes[name]


def add_triangles(sd, tris, bsdf):
    """triangles [n][3][3] as one mesh of the description, no vertex shared"""
    tris = np.asarray(tris, dtype=np.float64).reshape(-1, 3, 3)
    sd.add_mesh(tris.reshape(-1, 3), np.arange(3 * len(tris)).reshape(-1, 3), bsdf=bsdf, face_normals=True)


def kd_params(mts, pname, **more):
    kp = mts.abi.KdParams()
    for k, v in dict(PARAMS[pname], **more).items():
        setattr(kp, k, v)
    return kp


def tree_arrays(flat):
    a = flat.arrays()
    return {k: a[k].copy() for k in ("kd_nodes", "kd_indices", "aabb_min", "aabb_max")}


def report(mts, sname, pname, flat):
    """the checker's report on a built scene (mts.Scene or orc.FlatScene)"""
    prims = scene(mts, sname)[1]
    arrays, stats = tree_arrays(flat), K.stats_dict(flat.kdstats())
    h = hashlib.sha1()
    for k in sorted(arrays):
        h.update(np.ascontiguousarray(arrays[k]).tobytes())
    h.update(repr(sorted(stats.items())).encode())
    key = (sname, pname, h.hexdigest())
    if key not in _reports:
        _reports[key] = K.check(prims, arrays, K.Params(kd_params(mts, pname), prims.n), stats)
    return _reports[key]


def failures(rep, what):
    """violations of any property, and fragile shares past the caps, as lines of text"""
    out = ["%s: %s: %s" % (what, k, "; ".join(v[:3])) for k, v in rep.violations.items() if v]
    for k in K.PROPERTIES:
        n, of = rep.left_out[k]
        if n > (0 if k in NO_FRAGILE else CAP * of):
            out.append("%s: %s leaves out %d of %d cases as fragile" % (what, k, n, of))
    return out
