"""Per-vertex colours and the `vertexcolors` texture, host side (no GPU): the `.serialized` loader hands the EHasColors block
over, the flat scene's colour pool follows the vertices, the ABI keeps its version and struct sizes, the new exports exist,
the scene-description mirror records slot masks and writes 1 into a coloured slot, and the inputs of the device's end-to-end
comparison (tests/test_gpu_vcol.py) stay decidable.  The device side is tests/test_gpu_vcol.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ref64_vcol
import serialized_io as sio
import vcol_cases

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["mtsgpu_set_vertex_colors", "mtsgpu_group_set_vertex_colors", "mtsgpu_flat_scene_set_mesh_colors",
               "mtsgpu_flat_scene_vertex_colors", "mtsgpu_flat_scene_shape_has_colors", "mtsgpu_loaded_mesh_colors",
               "mtsgpu_vertex_color_eval", "mtsgpu_bsdf_eval_colored"]


# --- the loader --------------------------------------------------------------------------------------------------------
def _mesh(rng, nv, nt, normals, texcoords, colors):
    m = dict(positions=rng.uniform(-1, 1, (nv, 3)).astype(np.float32), triangles=rng.randint(0, nv, (nt, 3)).astype(np.uint32))
    if normals:
        n = rng.normal(size=(nv, 3)); m["normals"] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    if texcoords:
        m["texcoords"] = rng.uniform(0, 1, (nv, 2)).astype(np.float32)
    if colors:
        m["colors"] = rng.uniform(0, 1, (nv, 3)).astype(np.float32)
    return m


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("normals, texcoords", [(False, False), (True, False), (False, True), (True, True)])
def test_loader_returns_the_colour_block(mts, tmp_path, double, normals, texcoords):
    """the colours come after the optional normals and texture coordinates (trimesh.cpp:207-229): every combination of the
    two, both precisions, and a shape index > 0 whose neighbour has no colours"""
    rng = np.random.RandomState(3 + 2 * normals + texcoords)
    meshes = [_mesh(rng, 7, 5, not normals, texcoords, False), _mesh(rng, 13, 9, normals, texcoords, True), _mesh(rng, 5, 4, False, False, True)]
    path = str(tmp_path / "c.serialized")
    sio.write(path, meshes, double=double)
    for index, m in enumerate(meshes):
        got = mts.load_serialized(path, index)
        assert np.array_equal(got.positions, m["positions"]) and np.array_equal(got.triangles, m["triangles"])
        if "colors" in m:
            # float32 -> file precision -> float32 is exact either way: the bytes come back
            assert got.colors is not None and got.colors.dtype == np.float32
            assert np.array_equal(got.colors.view(np.uint32), m["colors"].view(np.uint32)), (index, double)
        else:
            assert got.colors is None
        if "normals" in m:
            assert np.array_equal(got.normals, m["normals"])
    # the C call itself: NULL without the flag, and mtsgpu_load_serialized / mtsgpu_mesh as they were
    h = C.c_void_p(); cm = mts.abi.Mesh()
    assert mts.lib().mtsgpu_load_serialized(os.fsencode(path), 0, C.byref(h), C.byref(cm)) == 0
    assert not mts.lib().mtsgpu_loaded_mesh_colors(h) and cm.n_verts == 7
    mts.lib().mtsgpu_loaded_mesh_free(h)
    assert not mts.lib().mtsgpu_loaded_mesh_colors(None)


def test_loader_of_a_file_without_colours_is_unchanged(mts):
    m = mts.load_serialized(os.path.join(ROOT, "tests", "golden", "matpreview.serialized"), 1)
    assert m.colors is None and m.positions.shape[0] > 0


# --- the flat scene's colour pool --------------------------------------------------------------------------------------
@pytest.mark.parametrize("face_normals", [True, False])
def test_colour_pool_follows_the_vertices(mts, face_normals):
    """two shared-vertex meshes, the first without colours, a sphere in between: row v of the pool is the colour of the vertex
    whose position is row v of vtx_pos, whatever `face_normals` makes the flattener do with the normals"""
    S = mts.scenes
    sd = S.SceneDescription("pool")
    white = sd.lambertian(0.5)
    plain = S.vcol_grid(3, colors=None).meshes[0]
    sd.add_mesh(plain.positions + F(3), plain.triangles, bsdf=white, face_normals=face_normals)
    sd.add_sphere((0, 5, 0), 0.5, bsdf=white)
    g = S.vcol_grid(4, seed=5).meshes[0]
    sd.add_mesh(g.positions, g.triangles, bsdf=sd.lambertian(S.VERTEX_COLORS), face_normals=face_normals, colors=g.colors)
    sd.point_light((0, 3, 0), 1.0)
    scene = mts.Scene(sd)
    A = scene.arrays()
    col, has = scene.vertex_colors()
    assert has.tolist() == [0, 0, 1] and col.shape == A["vtx_pos"].shape
    nv0 = plain.positions.shape[0]
    assert not col[:nv0].any()
    assert np.array_equal(A["vtx_pos"][nv0:], g.positions)
    assert np.array_equal(col[nv0:].view(np.uint32), g.colors.view(np.uint32))
    # through the triangles: corner k of primitive t has the colour its own mesh gave that vertex
    off = A["shape_tri_offset"]
    tri = A["tri_idx"][off[2]:off[3]]
    assert np.array_equal(col[tri], g.colors[g.triangles])
    assert scene.bsdf_color_slots.tolist() == [0, 1]
    # taking the colours away again: the getters return NULL
    assert mts.lib().mtsgpu_flat_scene_set_mesh_colors(scene._h, 2, None) == 0
    assert scene.vertex_colors() == (None, None)
    # what the call refuses
    assert mts.lib().mtsgpu_flat_scene_set_mesh_colors(scene._h, 3, mts.abi.ptr(g.colors, mts.abi.f32p)) == -1
    assert "out of range" in mts.lib().mtsgpu_last_error(None).decode()
    assert mts.lib().mtsgpu_flat_scene_set_mesh_colors(scene._h, 1, mts.abi.ptr(g.colors, mts.abi.f32p)) == -1
    assert "only a triangle mesh" in mts.lib().mtsgpu_last_error(None).decode()


def test_scene_without_colours_has_no_pool(mts):
    scene = mts.Scene(mts.scenes.cornell_c1())
    assert scene.vertex_colors() == (None, None) and scene.vertex_color_args() is None and scene.bsdf_color_slots is None


def test_mesh_description_wants_one_colour_per_vertex(mts):
    with pytest.raises(ValueError, match="one colour per vertex"):
        mts.scenes.MeshDesc(np.zeros((4, 3)), [[0, 1, 2]], colors=np.zeros((3, 3)))


# --- ABI ---------------------------------------------------------------------------------------------------------------
def test_abi_is_unchanged_and_the_exports_exist(mts):
    L, a = mts.lib(), mts.abi
    assert L.mtsgpu_abi_version() == a.ABI_VERSION == 8
    assert [L.mtsgpu_abi_sizeof(i) for i in range(6)] == [288, 172, 184, 72, 96, 48]
    header = open(os.path.join(ROOT, "include", "mtsgpu.h")).read()
    declared = set(re.findall(r"\b(mtsgpu_[a-z0-9_]+)\s*\(", header))
    for name in NEW_EXPORTS:
        assert name in declared and name in mts.EXPORTS and hasattr(L, name), name
    for line in ("#define MTSGPU_ABI_VERSION 8", "MTSGPU_BSDF_NTYPES = 10", "#define MTSGPU_BSDF_NPARAMS 16"):
        assert line in header, line
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_EXPORTS:
        assert name in doc, name


# --- the scene-description mirror --------------------------------------------------------------------------------------
def test_constructors_record_slot_masks_and_write_ones(mts):
    """VERTEX_COLORS in slot s sets bit s and leaves the block of the constant (1, 1, 1), bit for bit: Phong::configure and
    Ward::configure then derive the reference's sampling weights from getAverage() = 1 (vertexcolors.cpp:49-55)"""
    S = mts.scenes
    V = S.VERTEX_COLORS
    pairs = [
        (lambda sd, a, b: sd.lambertian(a), 1), (lambda sd, a, b: sd.dielectric(1.5, 1.0, refl=a, trans=b), 2),
        (lambda sd, a, b: sd.roughmetal(0.2, refl=a), 1), (lambda sd, a, b: sd.microfacet(0.2, 0.4, 0.3, rd=a, rs=b), 2),
        (lambda sd, a, b: sd.mirror(a), 1), (lambda sd, a, b: sd.phong(17.0, rd=a, rs=b, kd=0.6, ks=0.7), 2),
        (lambda sd, a, b: sd.roughglass(0.2, refl=a, trans=b), 2), (lambda sd, a, b: sd.difftrans(a), 1),
        (lambda sd, a, b: sd.ward(0.2, 0.2, rd=a, rs=b, kd=0.8, ks=0.9), 2)]
    for btype, (make, n_slots) in enumerate(pairs):
        assert len(mts.abi.BSDF_COLOR_SLOTS[btype]) == n_slots
        for mask in range(1 << n_slots):
            sd = S.SceneDescription("m")
            one = make(sd, 1.0, 1.0)
            col = make(sd, V if mask & 1 else 1.0, V if mask & 2 else 1.0)
            assert sd.bsdf_type[col] == btype and sd.bsdf_color_slots == [0, mask], (btype, mask)
            assert np.array_equal(sd.bsdf_params[one].view(np.uint32), sd.bsdf_params[col].view(np.uint32)), (btype, mask)
            for s in range(n_slots):
                o = mts.abi.BSDF_COLOR_SLOTS[btype][s]
                assert sd.bsdf_params[col][o:o + 3].tolist() == [1.0, 1.0, 1.0]
    sd = S.SceneDescription("m")
    with pytest.raises(ValueError, match="alpha"):
        sd.roughglass(V)
    # a constant next to a coloured slot keeps its value, and existing constructors give what they gave
    assert sd.bsdf_params[sd.phong(9.0, rd=0.25, rs=V)][5:11].tolist() == [0.25, 0.25, 0.25, 1.0, 1.0, 1.0]
    c = sd.composite([0.5, 0.5], [0, 0])
    assert sd.bsdf_color_slots[c] == 0 and len(sd.bsdf_color_slots) == len(sd.bsdf_type)


# --- the restatement and the inputs of the device comparison -----------------------------------------------------------
def test_restatement_at_the_corners_and_against_its_mirror():
    rng = np.random.RandomState(2)
    col = rng.uniform(0, 1, (25, 3)).astype(np.float32)
    tri = rng.randint(0, 25, (32, 3)).astype(np.uint32)
    prim, u, v = vcol_cases.barycentric_records(rng, 32, 4000)
    val, bound = ref64_vcol.color64(col, tri, prim, u, v)
    m = ref64_vcol.color32(col, tri, prim, u, v)
    assert m.dtype == np.float32 and ref64_vcol.within_bound(m, val, bound).all()
    assert (bound <= 3.5 * np.abs(col).max() + 1e-12).all()      # a convex combination of numbers below 1: a few half units
    c0 = col[tri[prim][:, 0]]
    at0 = (u == 0) & (v == 0)
    assert at0.sum() >= 10 and np.array_equal(m[at0], c0[at0])
    # the bound is no blank cheque: one ulp of 0.5 on top of the mirror leaves it where the value is that large
    big = val > 0.5
    assert (~ref64_vcol.within_bound(m + F(2.0 ** -19), val, bound))[big].all()


def test_end_to_end_inputs_stay_under_the_exclusion_cap(mts):
    """tests/test_gpu_vcol.py excludes camera samples whose hit lies within the rounding reach of a cell edge or diagonal;
    the share is decided here, from the raster positions the samplers can produce, by the restatement alone"""
    for material in ("lambertian", "phong"):
        geo = vcol_cases.GridGeometry(mts, material)
        rng = np.random.RandomState(8)
        raster = rng.uniform(0, vcol_cases.E2E_RES, (20000, 2)).astype(np.float32)
        hit = geo.locate(raster)
        assert hit.excluded.mean() <= vcol_cases.MAX_EXCLUDED, hit.excluded.mean()
        assert (hit.prim < 2 * vcol_cases.E2E_CELLS ** 2).all()
        # the closed form is consistent: the point rebuilt from (prim, u, v) is the point below the raster position
        p = geo.point(hit.prim, hit.u, hit.v)
        assert np.abs(p - hit.p).max() < 1e-12
