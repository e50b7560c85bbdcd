"""Texture coordinates and the checkerboard / grid textures, host side (no GPU): the `.serialized` loader hands the
EHasTexcoords block over, the flat scene's uv pool follows the vertices, the ABI keeps its version and struct sizes, the new
exports exist and are documented, the scene-description mirror records the slot table and writes getAverage() into the block,
the restatement (tests/ref64_tex.py) agrees with its mirror and with hand-computed points, reports every mutation, and the
inputs of the device's end-to-end comparison stay under the cap on fragile samples.  The device side is tests/test_gpu_tex.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ref64_tex as R
import serialized_io as sio
import tex_cases

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["mtsgpu_set_uv_textures", "mtsgpu_group_set_uv_textures", "mtsgpu_flat_scene_set_mesh_texcoords",
               "mtsgpu_flat_scene_vertex_texcoords", "mtsgpu_flat_scene_shape_has_texcoords", "mtsgpu_loaded_mesh_texcoords",
               "mtsgpu_uv_texture_eval", "mtsgpu_bsdf_eval_slots"]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# --- the loader --------------------------------------------------------------------------------------------------------
def _mesh(rng, nv, nt, normals, texcoords, colors):
    m = dict(positions=rng.uniform(-1, 1, (nv, 3)).astype(np.float32), triangles=rng.randint(0, nv, (nt, 3)).astype(np.uint32))
    if normals:
        n = rng.normal(size=(nv, 3)); m["normals"] = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(np.float32)
    if texcoords:
        m["texcoords"] = rng.uniform(-2, 2, (nv, 2)).astype(np.float32)
    if colors:
        m["colors"] = rng.uniform(0, 1, (nv, 3)).astype(np.float32)
    return m


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("normals, colors", [(False, False), (True, False), (False, True), (True, True)])
def test_loader_returns_the_texcoord_block(mts, tmp_path, double, normals, colors):
    """the texcoords sit between the optional normals and the optional colours (trimesh.cpp:207-229): every combination of
    the two, both precisions, and a shape index > 0 whose neighbour has no texcoords"""
    rng = np.random.RandomState(13 + 2 * normals + colors)
    meshes = [_mesh(rng, 7, 5, not normals, False, colors), _mesh(rng, 13, 9, normals, True, colors), _mesh(rng, 5, 4, False, True, False)]
    path = str(tmp_path / "t.serialized")
    sio.write(path, meshes, double=double)
    for index, m in enumerate(meshes):
        got = mts.load_serialized(path, index)
        assert np.array_equal(got.positions, m["positions"]) and np.array_equal(got.triangles, m["triangles"])
        if "texcoords" in m:
            assert got.texcoords is not None and got.texcoords.dtype == np.float32 and got.texcoords.shape == (len(m["positions"]), 2)
            assert np.array_equal(bits(got.texcoords), bits(m["texcoords"])), (index, double)
        else:
            assert got.texcoords is None
        for key in ("normals", "colors"):
            if key in m:
                assert np.array_equal(bits(getattr(got, key)), bits(m[key])), (index, key)
            else:
                assert getattr(got, key) is None
    h = C.c_void_p(); cm = mts.abi.Mesh()
    assert mts.lib().mtsgpu_load_serialized(os.fsencode(path), 0, C.byref(h), C.byref(cm)) == 0
    assert not mts.lib().mtsgpu_loaded_mesh_texcoords(h) and cm.n_verts == 7
    mts.lib().mtsgpu_loaded_mesh_free(h)
    assert not mts.lib().mtsgpu_loaded_mesh_texcoords(None)


def test_loader_of_a_file_without_texcoords_is_unchanged(mts):
    path = os.path.join(ROOT, "tests", "golden", "matpreview.serialized")
    m = mts.load_serialized(path, 1)
    ref = sio.read(path, 1)
    assert (m.texcoords is None) == (ref["texcoords"] is None)
    if ref["texcoords"] is not None:
        assert np.array_equal(bits(m.texcoords), bits(ref["texcoords"]))
    assert np.array_equal(m.positions, ref["positions"]) and np.array_equal(m.triangles, ref["triangles"])


# --- the flat scene's uv pool ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("face_normals", [True, False])
def test_uv_pool_follows_the_vertices(mts, face_normals):
    S = mts.scenes
    sd = S.SceneDescription("pool")
    white = sd.lambertian(0.5)
    plain = S.vcol_grid(3, colors=None).meshes[0]
    sd.add_mesh(plain.positions + F(3), plain.triangles, bsdf=white, face_normals=face_normals)
    sd.add_sphere((0, 5, 0), 0.5, bsdf=white)
    pos, tri, uv = S.tex_grid_mesh(4)
    sd.add_mesh(pos, tri, bsdf=sd.lambertian(S.Checkerboard()), face_normals=face_normals, texcoords=uv)
    sd.point_light((0, 3, 0), 1.0)
    scene = mts.Scene(sd)
    A = scene.arrays()
    pool, has = scene.vertex_texcoords()
    assert has.tolist() == [0, 0, 1] and pool.shape == (A["vtx_pos"].shape[0], 2)
    nv0 = plain.positions.shape[0]
    assert not pool[:nv0].any()
    assert np.array_equal(A["vtx_pos"][nv0:], pos) and np.array_equal(bits(pool[nv0:]), bits(uv))
    off = A["shape_tri_offset"]
    assert np.array_equal(pool[A["tri_idx"][off[2]:off[3]]], uv[tri])
    assert scene.bsdf_slot_texture.tolist() == [[-1, -1], [0, -1]] and len(scene.textures) == 1
    assert scene.uv_texture_args() is not None
    assert mts.lib().mtsgpu_flat_scene_set_mesh_texcoords(scene._h, 2, None) == 0
    assert scene.vertex_texcoords() == (None, None)
    assert mts.lib().mtsgpu_flat_scene_set_mesh_texcoords(scene._h, 3, mts.abi.ptr(uv, mts.abi.f32p)) == -1
    assert "out of range" in mts.lib().mtsgpu_last_error(None).decode()
    assert mts.lib().mtsgpu_flat_scene_set_mesh_texcoords(scene._h, 1, mts.abi.ptr(uv, mts.abi.f32p)) == -1
    assert "only a triangle mesh" in mts.lib().mtsgpu_last_error(None).decode()


def test_scene_without_textures_has_no_pool_and_no_call(mts):
    scene = mts.Scene(mts.scenes.cornell_c1())
    assert scene.vertex_texcoords() == (None, None) and scene.uv_texture_args() is None and scene.bsdf_slot_texture is None
    with pytest.raises(ValueError, match="one texcoord per vertex"):
        mts.scenes.MeshDesc(np.zeros((4, 3)), [[0, 1, 2]], texcoords=np.zeros((3, 2)))


# --- ABI ---------------------------------------------------------------------------------------------------------------
def test_abi_is_unchanged_and_the_exports_exist(mts):
    L, a = mts.lib(), mts.abi
    assert L.mtsgpu_abi_version() == a.ABI_VERSION == 8
    assert [L.mtsgpu_abi_sizeof(i) for i in range(6)] == [288, 172, 184, 72, 96, 48]
    header = open(os.path.join(ROOT, "include", "mtsgpu.h")).read()
    declared = set(re.findall(r"\b(mtsgpu_[a-z0-9_]+)\s*\(", header))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW_EXPORTS:
        assert name in declared and name in mts.EXPORTS and hasattr(L, name), name
        assert name in doc, name
    assert C.sizeof(a.UvTexture) == 48 and a.UvTexture.line_width.offset == 44
    assert "#define MTSGPU_ABI_VERSION 8" in header and "MTSGPU_TEX_CHECKERBOARD = 0, MTSGPU_TEX_GRID = 1" in header


# --- the scene-description mirror --------------------------------------------------------------------------------------
def test_constructors_record_the_slot_table_and_write_the_average(mts):
    """a texture in slot s puts its index into bsdf_slot_texture[b][s] and getAverage() into the block: dark * 0.5f for the
    checkerboard (sic), bright for the grid; the rest of the block is what the constant getAverage() gives, except that
    verifyEnergyConservation reads getMaximum() = bright (phong.cpp:81-90)"""
    S = mts.scenes
    check = S.Checkerboard(bright=(0.8, 0.6, 0.4), dark=(0.2, 0.1, 0.3), uscale=3.7)
    grid = S.GridTexture(bright=(0.5, 0.25, 0.75), dark=0.1, line_width=0.05)
    assert np.array_equal(check.average(), np.float32([0.2, 0.1, 0.3]) * F(0.5)) and np.array_equal(check.maximum(), check.bright)
    assert np.array_equal(grid.average(), grid.bright) and np.array_equal(grid.maximum(), grid.bright)
    makes = [(lambda sd, a, b: sd.lambertian(a), 1), (lambda sd, a, b: sd.dielectric(1.5, 1.0, refl=a, trans=b), 2),
             (lambda sd, a, b: sd.roughmetal(0.2, refl=a), 1), (lambda sd, a, b: sd.microfacet(0.2, 0.4, 0.3, rd=a, rs=b), 2),
             (lambda sd, a, b: sd.mirror(a), 1), (lambda sd, a, b: sd.phong(17.0, rd=a, rs=b, kd=0.3, ks=0.2), 2),
             (lambda sd, a, b: sd.roughglass(0.2, refl=a, trans=b), 2), (lambda sd, a, b: sd.difftrans(a), 1),
             (lambda sd, a, b: sd.ward(0.2, 0.2, rd=a, rs=b, kd=0.3, ks=0.2), 2)]
    for btype, (make, n_slots) in enumerate(makes):
        offs = mts.abi.BSDF_COLOR_SLOTS[btype]
        assert len(offs) == n_slots
        for pick in range(3 ** n_slots):
            choice = [(pick // 3 ** s) % 3 for s in range(2)]
            args = [[0.5, check, grid][c] for c in choice]
            sd = S.SceneDescription("m")
            b = make(sd, *args)
            # the same BSDF from the constants the textures average to (kd, ks chosen so that no normalisation happens)
            ref = make(sd, *[a if not isinstance(a, S._UvTexture) else tuple(a.average()) for a in args]) if btype != 0 else \
                sd.lambertian(*(tuple(args[0].average()) if isinstance(args[0], S._UvTexture) else (args[0],)))
            assert sd.bsdf_type[b] == btype and sd.bsdf_color_slots[b] == 0
            assert np.array_equal(bits(sd.bsdf_params[b]), bits(sd.bsdf_params[ref])), (btype, choice)
            row = sd.bsdf_slot_texture[b]
            for s in range(2):
                t = args[s] if s < n_slots and isinstance(args[s], S._UvTexture) else None
                assert (row[s] == -1) if t is None else (sd.textures[row[s]] is t), (btype, choice)
                if t is not None:
                    assert np.array_equal(sd.bsdf_params[b][offs[s]:offs[s] + 3], t.average())
            assert sd.bsdf_slot_texture[ref] == [-1, -1] and len(sd.bsdf_slot_texture) == len(sd.bsdf_type)
    sd = S.SceneDescription("m")
    # one instance in two BSDFs is one entry of the texture list; vertex colours next to a texture keep their bit
    a, b = sd.lambertian(check), sd.phong(9.0, rd=check, rs=S.VERTEX_COLORS, kd=0.3, ks=0.2)
    assert sd.textures == [check] and sd.bsdf_slot_texture == [[0, -1], [0, -1]] and sd.bsdf_color_slots == [0, 2]
    # energy conservation reads getMaximum(): bright 0.8 * kd 1 + 0.5 * ks 1 > 1 scales kd and ks, the average 0.1 would not
    p = sd.bsdf_params[sd.phong(9.0, rd=check, rs=0.5, kd=1.0, ks=1.0)]
    assert p[1] == F(1) * (F(1) / (F(1) * F(0.8) + F(1) * F(0.5))) and p[1] < 1
    with pytest.raises(ValueError, match="alpha"):
        sd.roughglass(check)
    d = check.descriptor()
    assert (d.kind, d.uscale, d.vscale, d.uoffset, list(d.dark)) == (0, F(3.7), 1.0, 0.0, [F(0.2), F(0.1), F(0.3)])
    assert grid.descriptor().kind == 1 and grid.descriptor().line_width == F(0.05)


# --- the restatement ---------------------------------------------------------------------------------------------------
def test_hand_computed_points():
    """truncation towards zero: the cell around 0 is twice as wide, and a negative coordinate keeps a negative fraction"""
    ck = R.Tex(R.CHECKERBOARD)
    gr = R.Tex(R.GRID, line_width=0.125)
    pts = [  # uv, checkerboard bright?, grid bright?
        ((0.25, 0.25), True, True), ((0.75, 0.25), False, True), ((-0.25, 0.25), True, True), ((-0.75, 0.25), False, True),
        ((-0.25, -0.25), True, True), ((-0.75, -0.75), True, True), ((0.5, 0.25), False, True), ((-0.5, 0.25), False, True),
        ((0.1, 0.5), False, False), ((-0.1, 0.5), False, False), ((0.95, 0.5), True, False), ((-0.95, 0.5), True, True),
        ((0.5, 0.5), True, True), ((0.125, 0.5), False, True), ((0.875, 0.5), True, True), ((0.88, 0.5), True, False),
        ((1.0, 0.5), False, False), ((-1.0, 0.5), False, False), ((-1.05, 0.5), False, False), ((-1.95, 0.5), True, True)]
    for dtype in (np.float32, np.float64):
        for (x, y), cb, gb in pts:
            ux, uy = np.array([x], dtype=np.float32), np.array([y], dtype=np.float32)
            assert bool(R.at_uv(ck, ux, uy, dtype)[0]) == cb, ("checkerboard", x, y)
            assert bool(R.at_uv(gr, ux, uy, dtype)[0]) == gb, ("grid", x, y)
    # where floor and the cast differ, the mutation gives the other answer
    for x in (-0.25, -0.75):
        ux, uy = np.array([x], dtype=np.float32), np.array([0.25], dtype=np.float32)
        assert R.at_uv(ck, ux, uy, np.float64)[0] != R.at_uv(ck, ux, uy, np.float64, "floor")[0]
    ux, uy = np.array([-0.95], dtype=np.float32), np.array([0.5], dtype=np.float32)
    assert R.at_uv(gr, ux, uy, np.float64)[0] and not R.at_uv(gr, ux, uy, np.float64, "floor")[0]
    # the transform: the product is rounded before the sum, and offsets follow the scale
    t = R.Tex(R.CHECKERBOARD, 0.3, -0.3, 3.7, -3.7)
    x, y = R.transform(t, np.float32([0.7]), np.float32([0.2]), np.float32)
    assert x[0] == F(F(0.7) * F(3.7)) + F(0.3) and y[0] == F(F(0.2) * F(-3.7)) + F(-0.3)
    # interpolation at the corners, and the sphere's poles and seam
    tc = np.float32([[0.1, 0.2], [0.9, -0.4], [-0.7, 0.6]])
    for dtype in (np.float32, np.float64):
        ux, uy = R.triangle_uv(tc, [[0, 1, 2]], [0, 0, 0], [0, 1, 0], [0, 0, 1], dtype)
        assert np.array_equal(np.stack([ux, uy], 1).astype(np.float32), tc)
        p = np.float32([[0, 0, 2], [0, 0, -2], [2, 0, 0], [0, 2, 0], [-2, 0, 0], [0, -2, 0]]) + np.float32([1, 2, 3])
        ux, uy = R.sphere_uv((1, 2, 3), 2.0, np.eye(3), p, dtype)
        assert np.allclose(uy, [0, 1, 0.5, 0.5, 0.5, 0.5], atol=1e-7) and np.allclose(ux[2:], [0, 0.25, 0.5, 0.75], atol=1e-7)


def _shared_decisions(mts, name, mutation=None):
    """the decisions of texture `name` on the shared inputs: random and boundary records on the floor and the strip"""
    S = mts.scenes
    tex = tex_cases.textures()[name]
    rng = np.random.RandomState(31)
    out = []
    pos, tri, uv = S.tex_grid_mesh(tex_cases.CELLS)
    prim, u, v = tex_cases.triangle_records(rng, 0, len(tri), 4096)
    out.append(R.decide_triangles(tex, uv, tri, prim, u, v, mutation))
    pos, tri, uv = tex_cases.boundary_strip()
    prim = np.arange(len(tri)); z = np.zeros(len(tri), dtype=np.float32)
    out.append(R.decide_triangles(tex, uv, tri, prim, z, z, mutation))
    return out


@pytest.mark.parametrize("name", sorted(tex_cases.textures()))
def test_restatement_agrees_with_its_mirror(mts, name):
    tex = tex_cases.textures()[name]
    floor, strip = _shared_decisions(mts, name)
    assert floor.uv32.min() < -0.5 and floor.uv32.max() > 0.5, "the texcoords reach below zero"
    for d in (floor, strip):
        assert np.abs(d.uv32 - d.uv64).max() < 1e-6
        keep = ~d.fragile
        assert np.array_equal(d.bright32[keep], d.bright64[keep])
    assert floor.fragile.mean() <= tex_cases.MAX_FRAGILE
    assert 0.05 < floor.bright32.mean() < 0.95, "both colours occur"
    if name.endswith("_id"):
        # the strip's texcoords ARE the boundary values, untransformed: nothing is rounded, nothing is fragile, both colours occur
        assert not strip.fragile.any() and 0.1 < strip.bright32.mean() < 0.9
    sp = tex_cases.sphere_points(np.random.RandomState(5), 4096)
    d = R.decide_sphere(tex, tex_cases.SPHERE_CENTER, tex_cases.SPHERE_RADIUS, np.eye(3), sp)
    assert d.uv32.min() >= 0 and d.uv32.max() <= 1
    assert np.array_equal(d.bright32[~d.fragile], d.bright64[~d.fragile]) and d.fragile.mean() <= 4 * tex_cases.MAX_FRAGILE


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_mutations_are_reported(mts, mutation):
    """each mutated restatement disagrees with the mirror on records that are not fragile, for at least one of the shared
    textures of the kind it touches: in the decision, or (grid) in the wrapped fractions x, y the decision is taken on"""
    kinds = {"invert": ("checker", "grid"), "ge_half": ("grid_id",), "le_width": ("grid_id",), "floor": ("checker", "grid", "checker_id", "grid_id"),
             "offset_first": ("checker", "grid"), "swap_uv": ("checker", "grid"), "b_order": ("checker", "grid")}[mutation]
    reported = 0
    for name in kinds:
        for d in _shared_decisions(mts, name, mutation):
            keep = ~d.fragile
            reported += int((d.bright32[keep] != d.bright64[keep]).sum())
            if d.frac32 is not None:
                # `>= .5` cannot change a colour (|x| is the same either way); it shows in the wrapped fraction itself
                reported += int((np.abs(d.frac32 - d.frac64)[keep] > 1e-5).any(axis=1).sum())
    print("%s: %d records reported" % (mutation, reported))
    assert reported > 0


# --- the inputs of the device's end-to-end comparison ------------------------------------------------------------------
@pytest.mark.parametrize("shape, name", [("grid", "checker"), ("grid", "grid"), ("sphere", "checker")])
def test_end_to_end_inputs_stay_under_the_cap(mts, shape, name):
    tex = tex_cases.textures()[name]
    geo = (tex_cases.FloorGeometry if shape == "grid" else tex_cases.SphereGeometry)(mts, tex)
    raster = np.random.RandomState(8).uniform(0, tex_cases.E2E_RES, (40000, 2)).astype(np.float32)
    hit = geo.locate(raster)
    print("%s / %s: fragile %.3g, hit %.3g, bright %.3g" % (shape, name, hit.fragile.mean(), hit.hit.mean(), hit.bright[hit.hit].mean()))
    assert hit.fragile.mean() <= tex_cases.MAX_FRAGILE
    assert hit.hit.mean() > 0.4 and 0.1 < hit.bright[hit.hit].mean() < 0.9
