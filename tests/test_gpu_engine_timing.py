"""The bookkeeping of the bounce engine (csrc/render.cpp): what a frame reports with time_kernels on -- per-class traversal
times, shading time, launch counts -- next to the same frame without it, in every drive of the engine; and one context taken
through every grow-only buffer it owns, twice in one process.  Films are compared bit for bit with the oracle's.

Scene and size are those of test_host_driven_bounces_match_the_oracle_with_retry_and_ragged_passes (c5_small, 48 x 40,
ldsampler, 16 spp, maxDepth 8).

The 1e-4 of the time inequalities is derived, not fitted: the times of a frame are at most a few hundred binary32 event
intervals that lie inside the frame's interval (or, per class, inside the sum they are part of), each rounded once to
2^-24 relative, so their sum can exceed what contains it by a few hundred x 6e-8 < 1e-4 relative and no more."""
import numpy as np
import pytest

from test_gpu_parity import _setup
import test_gpu_miss_settled as rounds

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH = 48, 40, 16, 8
EPS = 1e-4
COUNTS = ("rays_closest", "rays_shadow", "camera_samples", "trace_launches")
# (knobs, max_paths, host-driven): the four drives of the engine
DRIVES = [
    (dict(sync_free=1, shade_fused=1), 0, False),
    (dict(sync_free=1, shade_fused=0), 0, False),
    (dict(sync_free=0), 0, True),
    (dict(sync_free=0), SPP * (W * H // 3 + 1), True),      # ragged passes
]
_cache = {}


def _frame(mts, orc):
    """scene, cameras and the oracle's film of the frame: built once, shared, never changed"""
    if "frame" not in _cache:
        sd, scene, oscene, cam, ocam, it, op = _setup(mts, orc, "c5_small", W=W, H=H, sampler="ldsampler", spp=SPP, max_depth=DEPTH)
        it.close()
        _cache["frame"] = dict(sd=sd, scene=scene, oscene=oscene, cam=cam, ocam=ocam, op=op, film=orc.render(oscene.scene, ocam, op)[0])
    return _cache["frame"]


def _tracer(mts, f):
    it = mts.MIPathTracer(maxDepth=DEPTH)
    it.preprocess(f["scene"], f["cam"], sampler="ldsampler", sampleCount=SPP, seed=0x5EED)
    return it


def _render(it, max_paths, timed):
    it.set_options(max_paths=max_paths, time_kernels=timed)
    it.clear_film()
    assert it.render()
    return it.film(), it.stats(), it.bin_entries()


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("drive", range(len(DRIVES)))
def test_timing_on_changes_no_film_and_no_count(gpu_lib, mts, orc, drive):
    knobs, max_paths, host_driven = DRIVES[drive]
    f = _frame(mts, orc)
    it = _tracer(mts, f)
    it.set_tuning(**knobs)
    film0, st0, bins0 = _render(it, max_paths, False)
    film1, st1, bins1 = _render(it, max_paths, True)
    print(drive, {k: st1[k] for k in ("trace_ms", "shade_ms", "trace_first_ms", "trace_shadow_ms", "trace_union_ms", "total_ms", "trace_launches")})
    assert _same(film0, f["film"]) and _same(film1, f["film"])
    for k in COUNTS:
        assert st0[k] == st1[k], k
    assert bins0 == bins1 and sum(bins0) > 0
    assert st0["camera_samples"] == W * H * SPP and st0["trace_launches"] > 0
    assert st0["trace_ms"] == 0 and st0["shade_ms"] == 0
    assert st1["trace_ms"] > 0 and st1["shade_ms"] > 0
    assert st1["trace_first_ms"] > 0
    assert st1["trace_first_ms"] + st1["trace_shadow_ms"] <= st1["trace_ms"] * (1 + EPS)
    assert 0 < st1["trace_union_ms"] <= st1["trace_ms"] * (1 + EPS)
    if host_driven:      # everything on one stream
        assert st1["trace_ms"] + st1["shade_ms"] <= st1["total_ms"] * (1 + EPS)
        assert st1["trace_shadow_ms"] > 0
    # the events of the frame before serve again
    film2, st2, _ = _render(it, max_paths, True)
    assert _same(film2, f["film"]) and st2["trace_launches"] == st0["trace_launches"] and st2["trace_ms"] > 0
    it.close()


def test_timing_with_the_retry_of_the_closest_hit_launch(gpu_lib, mts, orc):
    f = _frame(mts, orc)
    it = _tracer(mts, f)
    it.set_tuning(sync_free=0, test_retry=1)
    film0, st0, _ = _render(it, 0, False)
    film1, st1, _ = _render(it, 0, True)
    print({k: st1[k] for k in ("trace_ms", "trace_launches", "bin_overflow_retries")})
    assert _same(film0, f["film"]) and _same(film1, f["film"])
    assert st1["bin_overflow_retries"] > 0 and st1["bin_overflow_retries"] == st0["bin_overflow_retries"]
    assert st1["trace_launches"] == st0["trace_launches"] > st1["bin_overflow_retries"]
    it.close()


def test_timing_of_the_direct_integrators_rounds(gpu_lib, mts, orc):
    c = rounds._scene(mts, orc, "floor")
    it = mts.MIDirectIntegrator(luminaireSamples=2, bsdfSamples=2)
    it.preprocess(c["scene"], c["cam"], sampler="ldsampler", sampleCount=rounds.SPP, seed=rounds.SEED)
    film0, st0, bins0 = _render(it, 0, False)
    film1, st1, bins1 = _render(it, 0, True)
    print({k: st1[k] for k in ("trace_ms", "shade_ms", "trace_first_ms", "trace_shadow_ms", "trace_launches")})
    assert _same(film0, film1) and film0[..., :3].max() > 0
    for k in COUNTS:
        assert st0[k] == st1[k], k
    assert bins0 == bins1
    assert st0["rays_shadow"] > 0 and st0["trace_launches"] >= 3      # the camera rays, a shadow round, a round of sampled rays
    assert st0["trace_ms"] == 0 and st1["trace_ms"] > 0 and st1["shade_ms"] > 0
    assert st1["trace_shadow_ms"] > 0
    it.close()


def _grow_references(mts, orc, f):
    """the oracle's films of the four frames of test_one_context_through_every_grow_only_buffer, computed once"""
    if "grow" not in _cache:
        gauss = orc.tabulate_filter("gaussian")
        wide_cam = mts.PerspectiveCamera.for_description(f["sd"], 2 * W, H)
        wide_ocam = orc.make_camera(f["sd"], 2 * W, H)
        direct = orc.render_params(-1, sampler=mts.abi.SAMPLER_STRATIFIED_KEYED, spp=4, seed=0x5EED, integrator="direct",
                                   luminaire_samples=2, bsdf_samples=2)
        _cache["grow"] = dict(
            wide_cam=wide_cam,
            filtered=orc.render_tiles(f["oscene"].scene, f["ocam"], f["op"], gauss)[0],
            direct=orc.render(f["oscene"].scene, f["ocam"], direct)[0],
            wide=orc.render_tiles(f["oscene"].scene, wide_ocam, f["op"], gauss)[0])
    return _cache["grow"]


def test_one_context_through_every_grow_only_buffer(gpu_lib, mts, orc):
    """blocks and tile records (gaussian filter), film statistics, the sample arrays of a stratified direct frame, then every
    buffer again at twice the size; closed, and all of it once more in the same process"""
    f = _frame(mts, orc)
    g = _grow_references(mts, orc, f)
    for again in range(2):
        it = _tracer(mts, f)
        it.set_rfilter("gaussian")
        assert _same(_render(it, 0, False)[0], g["filtered"]), again
        it.set_rfilter("box"); it.set_film_statistics(True)
        assert _same(_render(it, 0, False)[0], f["film"]), again
        var, n = it.film_statistics()
        assert (n == SPP).all() and var.max() > 0
        it.set_film_statistics(False)
        it.preprocess(f["scene"], f["cam"], sampler="stratified", sampleCount=4, seed=0x5EED)
        assert gpu_lib.mtsgpu_set_direct_integrator(it._ctx, 2, 2) == 0
        assert _same(_render(it, 0, False)[0], g["direct"]), again
        it.preprocess(f["scene"], g["wide_cam"], sampler="ldsampler", sampleCount=SPP, seed=0x5EED)
        it.set_rfilter("gaussian")
        assert _same(_render(it, 0, False)[0], g["wide"]), again
        it.close()
