"""The launch matrix of the shading kernels against films recorded on another commit.

launch_shade / launch_shade_all send a material queue to one of four kernel families (k_shade, k_shade_vcol, k_shade_tex,
k_shade_tan), each instantiated per bin x ROUNDS x SKY, plus a fused k_shade_all* per family.  The other tests compare the
drivers with one another, so a wiring mistake that all drivers share -- a bin sent to another instantiation, ROUNDS and SKY
swapped, an argument missing from a family's launch -- passes them.  Films do not depend on scheduling, so this module holds
every cell of the matrix to the SHA-256 of the film that tests/golden/shade_launch_matrix.json recorded on the commit named
there (tools/record_shade_matrix.py prints that file from the cells below).

Cells: family x sky x integrator x driver = 4 x 2 x 3 x 3 = 72 renders of 32 x 32 pixels, 4 spp, independent sampler,
maxDepth 6.  Scenes: the project's helper scenes plus one small sphere per BSDF type the helper lacks, so that every bin a
family has kernels for holds a shape -- a type missing from a scene is a wiring this test cannot see.  That condition and the
family each scene makes the launcher pick are checked here, on the CPU (test_every_family_scene_fills_every_bin_of_its_kernels);
the renders are in tests/test_gpu_shade_matrix.py."""
import hashlib
import json
import os

import numpy as np
import pytest

import tan_cases

RES, SPP, MAX_DEPTH, SEED = 32, 4, 6, 5
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "shade_launch_matrix.json")

# family -> the bins (= BSDF types) it has kernels for; plain has the terminal bin as well, which needs rays that escape
FAMILY_BINS = {"plain": range(10), "vcol": range(9), "tex": range(9), "tan": range(10)}
INTEGRATORS = {"path": "path", "direct11": (1, 1), "direct23": (2, 3)}
# device-driven with the fused k_shade_all*, device-driven with one k_shade* per type, host-driven
DRIVERS = {"fused": dict(sync_free=1, shade_fused=1), "pertype": dict(sync_free=1, shade_fused=0), "host": dict(sync_free=0)}
GROUPS = [(family, sky) for family in FAMILY_BINS for sky in (False, True)]
CELLS = [(family, sky, integ, drive) for family, sky in GROUPS for integ in INTEGRATORS for drive in DRIVERS]


def cell_id(family, sky, integ, drive):
    return "%s-%s-%s-%s" % (family, "sky" if sky else "nosky", integ, drive)


def _one_of_each_type(sd, composite):
    """a row of small spheres in mid-air, one per BSDF type 0..8 and, composite = True, a composite of two earlier blocks"""
    blocks = [sd.lambertian(0.5, 0.6, 0.4), sd.dielectric(), sd.roughmetal(0.3), sd.microfacet(0.2), sd.mirror(0.7),
              sd.phong(15.0, 0.4, 0.3), sd.roughglass(0.2), sd.difftrans(0.6), sd.ward(0.15, 0.15)]
    if composite:
        blocks.append(sd.composite([0.5, 0.5], [blocks[0], blocks[8]]))
    for k, b in enumerate(blocks):
        sd.add_sphere((-0.81 + 0.18 * k, 1.0, 0.3), 0.08, bsdf=b)


def scene_description(mts, family, sky):
    S = mts.scenes
    if family == "plain":
        sd = S.spheres()                    # an open box: paths leave it, with and without a sky behind
        if sky:
            sd.sky(sun_direction=(0.3, 0.2, 0.8), turbidity=3.0, sky_scale=0.2)
    elif family == "vcol":
        sd = S.cornell_vcol(sky=sky)
    elif family == "tex":
        sd = S.cornell_tex(sky=sky)
    else:
        sd = tan_cases.mixed_scene(mts, sky=sky)
    _one_of_each_type(sd, composite=9 in FAMILY_BINS[family])
    return sd


def bins_of(sd):
    """the material queues the shapes' hits are sorted to: the BSDF type of each shape that has a BSDF"""
    return {sd.bsdf_type[m.bsdf] & 0xFF for m in sd.meshes if m.bsdf >= 0}


def family_of(scene):
    """the family launch_shade / launch_shade_all pick, in their order of precedence"""
    if scene.wants_tangents:
        return "tan"
    if scene.bsdf_slot_texture is not None:
        return "tex"
    if scene.bsdf_color_slots is not None:
        return "vcol"
    return "plain"


def render(mts, scene, cam, integ, drive):
    it = mts.MIPathTracer(maxDepth=MAX_DEPTH) if INTEGRATORS[integ] == "path" else mts.MIDirectIntegrator(*INTEGRATORS[integ])
    it.preprocess(scene, cam, sampler="independent", sampleCount=SPP, seed=SEED)
    it.set_tuning(**DRIVERS[drive])
    assert it.render()
    return it.film()


def film_hash(film):
    return hashlib.sha256(np.ascontiguousarray(film).tobytes()).hexdigest()


def render_group(mts, family, sky):
    """{cell id: film} of the nine cells of one (family, sky)"""
    sd = scene_description(mts, family, sky)
    scene = mts.Scene(sd)
    assert family_of(scene) == family
    cam = mts.PerspectiveCamera.for_description(sd, RES, RES)
    return {cell_id(family, sky, integ, drive): render(mts, scene, cam, integ, drive) for integ in INTEGRATORS for drive in DRIVERS}


@pytest.mark.parametrize("family, sky", GROUPS)
def test_every_family_scene_fills_every_bin_of_its_kernels(mts, family, sky):
    sd = scene_description(mts, family, sky)
    assert set(FAMILY_BINS[family]) <= bins_of(sd), "a BSDF type is missing: its kernels of this family would never be launched"
    scene = mts.Scene(sd)
    assert family_of(scene) == family
    assert scene.wants_tangents == (family == "tan")
    if family == "vcol":
        assert scene.bsdf_color_slots is not None and scene.bsdf_slot_texture is None
    if family == "tex":
        assert scene.bsdf_slot_texture is not None
    if family == "plain":
        assert scene.bsdf_color_slots is None and scene.bsdf_slot_texture is None
    assert (len(sd.lum_type) > 0 and any(t == mts.abi.LUM_SKY for t in sd.lum_type)) == sky


def test_the_fixture_holds_every_cell_and_one_hash_per_driver_triple():
    golden = json.load(open(GOLDEN))
    assert len(CELLS) == 72 and sorted(golden["films"]) == sorted(cell_id(*c) for c in CELLS)
    assert golden["commit"] and golden["command"]
    per_render = set()
    for family, sky in GROUPS:
        for integ in INTEGRATORS:
            hashes = {golden["films"][cell_id(family, sky, integ, drive)] for drive in DRIVERS}
            assert len(hashes) == 1, (family, sky, integ, "the drivers' films differ in the fixture")
            per_render |= hashes
    assert len(per_render) == 24, "two of the 24 (family, sky, integrator) films are the same film"
