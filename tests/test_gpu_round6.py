"""GPU tests, sixth set: what round 6 added or left uncovered, each against the oracle."""
import numpy as np
import pytest

from test_gpu_parity import _setup

pytestmark = pytest.mark.gpu


def test_ld_apply_in_memory_with_many_slots_groups_and_chunked_launches(gpu_lib, mts, orc):
    """LowDiscrepancySampler::generate() above 16 384 samples per pixel (k_ld_scout + k_ld_apply: a lane per table, the 64
    slots of a wave interleaved in a scratch copy, the result transposed through LDS into the per-pixel rows) with everything
    the single-slot table read-out cannot reach: 384 pixels = six groups of 64 slots, 48 tables per pixel = 288 (group, table)
    pairs = two chunked launches (block0 > 0), and a second pass whose last group is ragged (200 + 184 slots).  The film
    equals the oracle's in crops from the first group, a middle group, the pass boundary and the ragged last group"""
    W, H, spp, depth = 24, 16, 32768, 24
    sd, scene, oscene, cam, ocam, it, op = _setup(mts, orc, "c1", W=W, H=H, sampler="ldsampler", spp=spp, max_depth=2)
    it.preprocess(scene, cam, sampler="ldsampler", sampleCount=spp, depth=depth, seed=0x5EED)
    op = orc.render_params(2, sampler=mts.abi.SAMPLER_LD_KEYED, spp=spp, ld_depth=depth, seed=0x5EED)
    it.set_options(max_paths=200 * spp)
    assert it.render()
    film = it.film()
    assert it.stats()["camera_samples"] == W * H * spp
    for x0, y0 in ((0, 0), (10, 5), (6, 8), (8, 8), (22, 15)):      # slot 200 = pixel (8, 8): the first of the second pass
        o, _ = orc.render(oscene.scene, ocam, op, rect=(x0, y0, x0 + 2, y0 + 1))
        assert np.array_equal(film[y0:y0 + 1, x0:x0 + 2].view(np.uint32), o[y0:y0 + 1, x0:x0 + 2].view(np.uint32)), (x0, y0)
        assert o[y0, x0, 4] > 0


def _group(mts, devices):
    sd = mts.scenes.cornell_c1()
    scene = mts.Scene(sd); cam = mts.PerspectiveCamera.for_description(sd, 64, 48)
    g = mts.DeviceGroup(devices, maxDepth=4)
    g.preprocess(scene, cam, sampler="independent", sampleCount=4)
    return g, scene, cam


def test_group_rccl_self_check_and_rank_count(gpu_lib, mts):
    """mtsgpu_group_render checks its communicator before the first frame depends on it (ncclCommInitAll gave every member a
    communicator, a one-float sum of ones arrives as the number of members) and reports the verified rank count; a probe
    that fails (injected) leaves the group on the ordered sum with the reason, and is an error when RCCL was demanded"""
    g, scene, cam = _group(mts, [0])
    assert g.rccl_ranks() == 0                           # no collective asked for yet
    assert g.render(ordered_reduce=2) and g.reduce_kind() == "rccl ncclReduce"
    assert g.rccl_ranks() == 1
    ref = g.film()
    g.set_tuning(rccl_fail=1)                            # the collective of the next frame fails: RCCL is given up
    assert g.render(ordered_reduce=2) and g.rccl_ranks() == 0 and np.array_equal(g.film().view(np.uint32), ref.view(np.uint32))
    g2, _, _ = _group(mts, [0])
    g2.set_tuning(rccl_fail=1)                           # the probe itself fails
    with pytest.raises(mts.MtsGpuError, match="self-check"):
        g2.render(ordered_reduce=2)
    assert g2.rccl_ranks() == 0
    g2.set_tuning(rccl_fail=0)
    assert g2.render() and np.array_equal(g2.film().view(np.uint32), ref.view(np.uint32))


def test_group_rccl_reduce_equals_the_ordered_sum_on_eight_gpus(gpu_lib, mts):
    """needs eight GPUs (skipped below): the node-sized form of the two-GPU test -- ncclCommInitAll over eight devices, the
    self-check, ONE ncclReduce of the films (renderproc.cpp:123-130 in one collective) against the ordered peer-copy sum and
    against the unsharded render; with the box filter every pixel has one writer, so all three films are equal bit for bit"""
    import torch
    if torch.cuda.device_count() < 8:
        pytest.skip("fewer than eight GPUs")
    g, scene, cam = _group(mts, list(range(8)))
    assert g.render(ordered_reduce=1) and g.reduce_kind() == "ordered peer-copy sum"
    a = g.film()
    try:
        assert g.render(ordered_reduce=2)
    except mts.MtsGpuError as e:
        pytest.skip("RCCL could not be initialised here: %s" % e)
    assert np.array_equal(g.film().view(np.uint32), a.view(np.uint32)), g.reduce_note()
    if g.reduce_kind() != "rccl ncclReduce":
        pytest.skip("the collective fell back to the ordered sum (film still equal): %s" % g.reduce_note())
    assert g.rccl_ranks() == 8
    one, _, _ = _group(mts, [0])
    assert one.render() and np.array_equal(one.film().view(np.uint32), a.view(np.uint32))


def test_host_driven_bounces_match_the_oracle_with_retry_and_ragged_passes(gpu_lib, mts, orc):
    """host-driven bounces (one stream: the any-hit launch of a bounce before the shading of the next one), also when every
    first closest-hit launch is repeated with static dealing and when the frame takes ragged passes: the oracle's film"""
    sd, scene, oscene, cam, ocam, it, op = _setup(mts, orc, "c5_small", W=48, H=40, sampler="ldsampler", spp=16, max_depth=8)
    ofilm, _ = orc.render(oscene.scene, ocam, op)
    for knobs in (dict(sync_free=0), dict(sync_free=0, test_retry=1)):
        it.set_tuning(**knobs)
        it.clear_film(); assert it.render()
        assert np.array_equal(it.film().view(np.uint32), ofilm.view(np.uint32)), knobs
    it.set_tuning(sync_free=0, test_retry=0)
    it.set_options(max_paths=16 * 500)                     # ragged passes
    it.clear_film(); assert it.render()
    assert np.array_equal(it.film().view(np.uint32), ofilm.view(np.uint32))


def test_tied_walls_match_the_oracle(gpu_lib, mts, orc):
    """the one case in which the hashed mailbox decides a closest hit: two primitives tied in t -- the later test wins, and which
    tests run depends on the mailbox (sahkdtree3.h:130-144, :278-283).  A box whose every wall exists twice, with different
    reflectances, makes every hit a tie: the film equals the oracle's bit for bit with host-driven bounces (also with the retry
    of the closest-hit launch) and with device-driven ones"""
    S = mts.scenes
    sd = S.SceneDescription("tied_walls")
    a, b = sd.lambertian(0.7, 0.2, 0.2), sd.lambertian(0.2, 0.7, 0.2)
    for name, p0, e1, e2, nrm in S._box_faces():
        pos, tri = S._quad(p0, e1, e2, nrm)
        sd.add_mesh(pos, tri, bsdf=a, face_normals=True, name=name)
        sd.add_mesh(pos.copy(), tri.copy(), bsdf=b, face_normals=True, name=name + "_again")
    pos, tri = S.icosphere(2, 0.35, (0.1, 0.45, 0.0))
    sd.add_mesh(pos, tri, bsdf=sd.dielectric(), face_normals=False, name="glass")
    S._add_light(sd)
    sd.max_depth = 6
    W, H, spp = 48, 40, 16
    scene = mts.Scene(sd); oscene = orc.FlatScene(sd)
    cam = mts.PerspectiveCamera.for_description(sd, W, H); ocam = orc.make_camera(sd, W, H)
    ofilm, _ = orc.render(oscene.scene, ocam, orc.render_params(6, sampler=mts.abi.SAMPLER_LD_KEYED, spp=spp, seed=5))
    it = mts.MIPathTracer(maxDepth=6)
    it.preprocess(scene, cam, sampler="ldsampler", sampleCount=spp, seed=5)
    for knobs in (dict(sync_free=0), dict(sync_free=0, test_retry=1), dict(sync_free=1, test_retry=0)):
        it.set_tuning(**knobs)
        it.clear_film(); assert it.render()
        assert np.array_equal(it.film().view(np.uint32), ofilm.view(np.uint32)), knobs
    # an ordinary scene
    sd2, scene2, oscene2, cam2, ocam2, it2, op2 = _setup(mts, orc, "c5_small", W=48, H=40, sampler="ldsampler", spp=16, max_depth=8)
    it2.set_tuning(sync_free=0)
    assert it2.render()
    assert np.array_equal(it2.film().view(np.uint32), orc.render(oscene2.scene, ocam2, op2)[0].view(np.uint32))
