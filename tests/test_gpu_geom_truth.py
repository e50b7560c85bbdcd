"""k_trace (closest hit and any hit) held against the binary64 restatement of tests/ref64_geom.py with no oracle in
between: every scene x tree x ray class of tests/geom_cases.py, product kernel and counting kernel, with the counters
proving that each hand-built tree drove the kernel down the path it was shaped for; then the scheduling knobs that small
launches never reach, which must not move an answer by a bit.  Run on the GPU box: pytest -m gpu"""
import ctypes as C

import numpy as np
import pytest

import geom_cases as GC

pytestmark = pytest.mark.gpu


def _tracer(mts, c, tree, count=False, **knobs):
    it = mts.MIPathTracer(maxDepth=2)
    sc = c.scene.sc if tree == "sah" else GC.with_tree(mts, c.scene.sc, c.trees[tree])
    rc = mts.lib().mtsgpu_upload_scene(it._ctx, C.byref(sc))
    assert rc == 0, mts.lib().mtsgpu_last_error(it._ctx)
    it.set_options(count_traversal=count)
    it.set_tuning(**knobs)
    return it


@pytest.mark.parametrize("tree", GC.TREES)
@pytest.mark.parametrize("scene", GC.SCENES)
def test_device_agrees_with_the_truth(gpu_lib, mts, scene, tree):
    c = GC.case(mts, scene)
    failures, first = [], {}
    for count in (False, True):                            # two instantiations of k_trace
        it = _tracer(mts, c, tree, count=count)
        what = "%s / %s / %s" % (scene, tree, "counting kernel" if count else "product kernel")
        hits = it.trace_rays(c.rays)
        stats = it.stats()
        f, worst = GC.check_closest(c.closest, hits, what)
        shadow = it.trace_rays(c.rays, shadow=True)
        failures += f + GC.check_shadow(c.shadow, shadow, what)
        print(what, "worst |device - truth| / bound", {k: round(v[0], 3) for k, v in worst.items()})
        if not count:
            first = dict(hits=hits, shadow=shadow)
            continue
        assert np.array_equal(hits, first["hits"]) and np.array_equal(shadow[:, 3], first["shadow"][:, 3]), what
        keys = ("n_inner", "n_leaf", "n_idx", "req_pair_global", "req_pair_lds", "req_node_global", "req_node_lds", "req_spill")
        print(what, "counters", {k: stats[k] for k in keys})
        if tree == "chain":
            assert stats["req_spill"] > 0, stats
        elif tree == "one_leaf":
            s = c.slices["interior"]
            assert c.closest.enters[s].all() and not c.closest.clip_ambiguous[s].any()
            it.trace_rays(c.rays[s])
            st = it.stats()
            print(what, "interior rays:", {k: st[k] for k in keys})
            assert st["n_inner"] == 0 and st["n_idx"] == (s.stop - s.start) * c.geom.n_prims, st
            assert stats["n_inner"] == 0
        elif tree == "median_small":
            assert stats["req_pair_global"] == 0 and stats["req_pair_lds"] > 0, stats
        elif tree == "median_large":
            assert stats["req_pair_global"] > 0 and stats["req_pair_lds"] > 0, stats
        it.close()
    assert not failures, "\n".join(failures)


def test_one_level_more_than_the_chain_is_refused(gpu_lib, mts):
    c = GC.case(mts, "soup")
    it = mts.MIPathTracer(maxDepth=2)
    L = mts.lib()
    ok = GC.with_tree(mts, c.scene.sc, c.trees["chain"])
    assert L.mtsgpu_upload_scene(it._ctx, C.byref(ok)) == 0
    deeper = GC.with_tree(mts, c.scene.sc, GC.chain(c.geom, GC.chain_levels() + 1))
    assert L.mtsgpu_upload_scene(it._ctx, C.byref(deeper)) == -1
    assert b"deeper than" in L.mtsgpu_last_error(it._ctx)


def _plan(n, n_cus, block, batch, blocks_per_cu, dyn_min_rounds, dyn_div):
    """trace_plan (kernels.h) for a closest-hit launch of n rays with these knobs -> (rounds, static_n)"""
    waves = block // 64
    per_cu = min(blocks_per_cu, 24 // waves)
    max_blocks = n_cus * per_cu
    need = (n + batch * waves - 1) // (batch * waves)
    blocks = min(need, max_blocks)
    per_round = blocks * waves * batch
    rounds = n // per_round
    dynamic = rounds >= dyn_min_rounds
    dyn_rounds = max(1, rounds // dyn_div) if dynamic else 0
    return rounds, ((rounds - dyn_rounds) * per_round if dynamic else n)


KNOBS = [dict(batch=8, blocks_per_cu=1, dyn_min_rounds=1), dict(batch=8, blocks_per_cu=1, dyn_min_rounds=1, dyn_div=1),
         dict(plain_below=1), dict(plain_below=1, refill_min=8), dict(plain_below=1, desc_min=1, leaf_min=1),
         dict(plain_below=1, desc_min=32, leaf_min=32), dict(plain_below=1, desc_min=32, leaf_min=32, refill_min=8, batch=8,
                                                            blocks_per_cu=1, dyn_min_rounds=1, dyn_div=1)]


@pytest.mark.parametrize("tree", ["median_large", "chain"])
def test_scheduling_knobs_do_not_move_an_answer(gpu_lib, mts, tree):
    import torch
    c = GC.case(mts, "twins")
    reps = -(-40000 // len(c.rays))
    rays = np.tile(c.rays, (reps, 1))
    n = len(rays)
    assert n >= 40000
    it = _tracer(mts, c, tree)
    ref, ref_shadow = it.trace_rays(rays), it.trace_rays(rays, shadow=True)
    it.close()
    for r in range(reps):
        s = slice(r * len(c.rays), (r + 1) * len(c.rays))
        f = GC.check_closest(c.closest, ref[s], "twins / %s" % tree)[0] + GC.check_shadow(c.shadow, ref_shadow[s], "twins / %s" % tree)
        assert not f, "\n".join(f)
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    block = GC.kernel_constants()["block"]
    for knobs in KNOBS:
        if "dyn_min_rounds" in knobs:
            rounds, static_n = _plan(n, n_cus, block, knobs["batch"], knobs["blocks_per_cu"], knobs["dyn_min_rounds"], knobs.get("dyn_div", 4))
            assert rounds > 1 and static_n < n, "the launch is not dynamic on %d CUs: rounds %d static %d of %d" % (n_cus, rounds, static_n, n)
        it = _tracer(mts, c, tree, **knobs)
        assert np.array_equal(it.trace_rays(rays), ref), knobs
        assert np.array_equal(it.trace_rays(rays, shadow=True)[:, 3], ref_shadow[:, 3]), knobs
        it.close()
