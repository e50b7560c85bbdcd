"""mtsgpu_upload_scene checks before it commits: a refused upload leaves the scene in force as it was."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_refused_upload_keeps_the_scene(gpu_lib, mts):
    """cornell_c1 at 16 x 16, 1 spp: a frame, an upload that checkScene refuses (an orphan node), the same frame bit for bit; a
    cylinder scene through the entry point that does not take cylinders, the same frame again"""
    import cyl_cases
    L = gpu_lib
    sd = mts.scenes.cornell_c1()
    scene = mts.Scene(sd)
    it = mts.MIPathTracer(maxDepth=4, device=0)
    it.preprocess(scene, mts.PerspectiveCamera.for_description(sd, 16, 16), sampler="independent", sampleCount=1, seed=3)

    def frame():
        it.clear_film()
        assert it.render()
        return it.film().view(np.uint32)
    first = frame()
    assert first.any()
    leaf = [0x80000000, 0]
    orphan = np.array([[1 << 2, 0], leaf, leaf, leaf, leaf], dtype=np.uint32)       # the root's children are nodes 1 and 2
    broken = mts.abi.Scene.from_buffer_copy(scene.sc)
    broken.kd_nodes = mts.abi.ptr(orphan, mts.abi.u32p); broken.n_nodes = len(orphan)
    assert L.mtsgpu_upload_scene(it._ctx, C.byref(broken)) == -1
    assert b"unreachable" in L.mtsgpu_last_error(it._ctx)
    assert np.array_equal(frame(), first)
    cyl = mts.Scene(cyl_cases.scene_description(mts, "one"))
    assert L.mtsgpu_upload_scene(it._ctx, cyl.ptr) == -1
    assert b"upload it with mtsgpu_upload_scene_cylinders" in L.mtsgpu_last_error(it._ctx)
    assert np.array_equal(frame(), first)
