"""The device phases of the kd-tree build (csrc/kdbuild_bin.hip, csrc/kdbuild_exact.hip) at the smallest shapes at which
they can still go wrong: a dozen primitives (less than one wave, fewer than the host threads that fill the box and triangle
arrays), non-triangle primitives, walls that are flat along an axis (the overflow branch of binIndex), and the one refusal
that only a device build can reach.  The large shapes are in test_gpu_parity.py and test_gpu_round2.py."""
import numpy as np
import pytest

TREE = ("kd_nodes", "kd_indices", "aabb_min", "aabb_max", "triaccel")

# scene -> (description, kd parameters): the primitive count exceeds the threshold, so the binning kernels do run
CASES = {
    "cornell_c1": (lambda s: s.cornell_c1(), dict(exact_prim_threshold=4, stop_prims=1)),
    "spheres": (lambda s: s.spheres(), dict(exact_prim_threshold=4, stop_prims=1)),
    "fuzz_0": (lambda s: s.fuzz(0), dict(exact_prim_threshold=40, min_max_bins=4)),
    "c5_2560_bins": (lambda s: s.cornell_c5(sphere_subdiv=2), dict(exact_prim_threshold=300, min_max_bins=2560)),
}
_reference = {}


def _params(mts, fields, **more):
    kp = mts.abi.KdParams()
    for k, v in dict(fields, **more).items():
        setattr(kp, k, v)
    return kp


def _host_and_oracle(mts, orc, name):
    """the host build of this library and the oracle's builder, once per scene"""
    if name not in _reference:
        make, fields = CASES[name]
        sd = make(mts.scenes)
        host = mts.Scene(sd, kd_params=_params(mts, fields, n_threads=1))
        oa = orc.FlatScene(sd, kd_params=_params(mts, fields)).arrays()
        _reference[name] = (sd, {k: host.arrays()[k].view(np.uint32).copy() for k in TREE}, host.kdstats(),
                            oa["kd_nodes"].copy(), oa["kd_indices"].copy())
    return _reference[name]


def _assert_same_tree(mts, orc, name, dev):
    _, harr, hstats, onodes, oidx = _host_and_oracle(mts, orc, name)
    da = dev.arrays()
    for k in TREE:
        assert np.array_equal(harr[k], da[k].view(np.uint32)), k
    assert dev.kdstats() == hstats
    assert np.array_equal(onodes, da["kd_nodes"]) and np.array_equal(oidx, da["kd_indices"])


@pytest.mark.gpu
@pytest.mark.parametrize("n_threads", [1, 16])
@pytest.mark.parametrize("binning,exact", [(True, False), (False, True), (True, True)])
@pytest.mark.parametrize("name", ["cornell_c1", "spheres", "fuzz_0"])
def test_tiny_trees_through_every_phase_combination(gpu_lib, mts, orc, name, binning, exact, n_threads):
    """k_kd_* and k_x_* on a few primitives: nodes, index lists, bounding box, triaccel and statistics are the host build's
    word for word, nodes and index lists the oracle builder's as well"""
    sd = _host_and_oracle(mts, orc, name)[0]
    dev = mts.Scene(sd, kd_params=_params(mts, CASES[name][1], n_threads=n_threads), gpu_binning=binning, gpu_exact=exact)
    _assert_same_tree(mts, orc, name, dev)


@pytest.mark.gpu
def test_bin_count_limit_of_the_device_binning_phase(gpu_lib, mts, orc):
    """the histogram of a node lives in 60 KiB of LDS: 2560 bins build the host's tree, 2561 are refused by name"""
    name = "c5_2560_bins"
    sd = _host_and_oracle(mts, orc, name)[0]
    _assert_same_tree(mts, orc, name, mts.Scene(sd, kd_params=_params(mts, CASES[name][1]), gpu_binning=True))
    with pytest.raises(mts.MtsGpuError, match="at most 2560 bins"):
        mts.Scene(sd, kd_params=_params(mts, CASES[name][1], min_max_bins=2561), gpu_binning=True)
