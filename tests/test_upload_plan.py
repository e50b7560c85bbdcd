"""The upload protocol and the signature table, without a GPU.

 * The calls MIPathTracer.preprocess and DeviceGroup.preprocess make on the library for the scenes of
   upload_plan_cases.plan_scenes() -- written down by a proxy in place of the library (tests/upload_plan_cases.py) -- equal
   tests/golden/upload_plan.json, which was recorded from the commit the file names: the one BEFORE both drivers came to run
   Scene.upload_plan(), when each spelled the protocol out itself.  The plan names the same calls.
 * The scene list takes every branch of that protocol; the test says so itself, from the fixture and the scenes.
 * binding.TABLE: every name of the six lists has a row, a symbol and, after lib(), a signature."""
import json
import os

import pytest

import upload_plan_cases as R

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "upload_plan.json")))["traces"]


@pytest.fixture(scope="module")
def flat(mts):
    """name -> Scene, and the bare pointer of one of them"""
    out = {name: mts.Scene(sd) for name, sd in R.plan_scenes(mts)}
    out[R.BARE] = out["cornell_c1"].ptr
    return out


def test_the_fixture_and_the_scene_list_name_the_same_cases(flat):
    assert sorted(GOLDEN) == sorted(flat)


def test_the_scene_list_takes_every_branch(flat):
    """every upload call, every setter, the texture call without textures ahead of the cloth call once over real texcoords and
    once over the zero pool, and the bare pointer"""
    calls = {name: [c for c, _ in trace] for name, trace in GOLDEN.items()}
    taken = set().union(*calls.values())
    assert {"upload_scene", "upload_scene_tangents", "upload_scene_cylinders", "set_vertex_colors", "set_uv_textures", "set_uv_bitmap_textures",
            "set_uv_masked_textures", "set_snow_bsdfs", "set_cloth_bsdfs", "set_spot_textures"} <= taken
    uv = {name: args for name, trace in GOLDEN.items() for c, args in trace if c == "set_uv_textures"}
    assert any(args[2] > 0 and args[3] == "ptr" for args in uv.values()), "set_uv_textures with textures"
    uv_only = [name for name, args in uv.items() if args[2:] == [0, "null", "null"]]
    for name in uv_only:
        assert calls[name][calls[name].index("set_uv_textures") + 1] == "set_cloth_bsdfs", name
    pools = {name: flat[name].vertex_texcoords()[0] is not None for name in uv_only}
    assert True in pools.values(), "the uv-only call over real texcoords"
    assert False in pools.values(), "the uv-only call over the zero pool of a scene whose cloth sits on spheres only"
    assert GOLDEN[R.BARE][1] == ["upload_scene", ["ptr"]] and not isinstance(flat[R.BARE], type(flat["cornell_c1"]))


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_both_drivers_and_the_plan_follow_the_recorded_protocol(mts, flat, name):
    scene, want = flat[name], GOLDEN[name]
    whole, got = R.preprocess_trace(mts, lambda: mts.MIPathTracer(maxDepth=5), scene)
    assert got == want
    assert [whole[0][0], whole[-1][0]] == ["create", "destroy"] and len(whole) == len(got) + 2
    whole, got = R.preprocess_trace(mts, lambda: mts.DeviceGroup([0], maxDepth=5), scene)
    assert got == want
    assert [whole[0][0], whole[-1][0]] == ["create_multi", "destroy"] and len(whole) == len(got) + 2
    # the attachment part: between set_integrator and set_camera
    assert [want[0][0], want[-2][0], want[-1][0]] == ["set_integrator", "set_camera", "set_sampler"]
    if name == R.BARE:
        assert mts.flatscene.upload_plan(scene) == [("upload_scene", (scene,))]
    else:
        plan = scene.upload_plan()
        assert [c for c, _ in plan] == [c for c, _ in want[1:-2]]
        assert [[R.word(a) for a in args] for _, args in plan] == [args for _, args in want[1:-2]]


def test_the_recorder_opens_no_device(mts, flat):
    """what is neither context-free nor written down is refused, not forwarded"""
    with R.recording(mts):
        it = mts.MIPathTracer()
        try:
            with pytest.raises(RuntimeError, match="needs a device"):
                it.render()
        finally:
            it.close()
    assert mts.binding._lib is mts.lib() and not isinstance(mts.lib(), R.Proxy)


def test_signature_table(mts):
    B = mts.binding
    lists = [B.EXPORTS, B.MASK_EXPORTS, B.SNOW_EXPORTS, B.CLOTH_EXPORTS, B.SPOT_EXPORTS, B.CYLINDER_EXPORTS]
    assert [len(names) for names in lists] == [94, 3, 5, 6, 4, 7]
    rows = {row[0]: row for header, group in B.TABLE.items() for row in group}
    assert len(rows) == sum(len(group) for group in B.TABLE.values()), "a symbol with two rows"
    L = mts.lib()
    for name in sum(lists, []):
        assert name in rows, name
        assert getattr(L, name).argtypes is not None, name
        assert list(getattr(L, name).argtypes) == list(rows[name][1]), name
    for header, group in B.TABLE.items():
        for row in group:
            assert len(row) in (2, 3), row
            assert sum(names.count(row[0]) for names in lists) == (0 if header == "hooks" else 1), row[0]
            assert getattr(L, row[0]).argtypes is not None, row[0]
    assert [row[0] for row in B.TABLE["hooks"]] == ["mtsgpu_hook_rays_redone"]
    # the facade hands out the same objects
    assert mts.EXPORTS is B.EXPORTS and mts.CYLINDER_EXPORTS is B.CYLINDER_EXPORTS and mts.lib is B.lib
