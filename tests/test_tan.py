"""Vertex tangents from texture coordinates, host side (no GPU): mtsgpu_flatten_tangents computes what the float32 mirror of
tests/ref64_tan.py computes, bit for bit, on the regular and the degenerate meshes, and lies within the derived bound of the
binary64 restatement on the regular ones; every mutation of the restatement is reported; the per-shape flags, the refusals and
acceptances of the new flatten call, the unchanged refusals of the old one, and the ABI.  The device side is
tests/test_gpu_tan.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ref64_tan as R
import tan_cases

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["mtsgpu_flatten_tangents", "mtsgpu_flat_scene_vertex_tangents", "mtsgpu_flat_scene_shape_has_tangents",
               "mtsgpu_upload_scene_tangents", "mtsgpu_group_upload_scene_tangents", "mtsgpu_shading_frame_eval"]
MESHES = {"floor": 0, "cylinder": 1, "degenerate": 2}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def hook(mts):
    """the flat hook scene, its description, and per mesh the mirror's tangents, normals and decisions (computed once)"""
    sd = tan_cases.hook_scene(mts)
    scene = mts.Scene(sd)
    mirror = {}
    for name, s in MESHES.items():
        m = sd.meshes[s]
        mirror[name] = R.tangents32(m.positions, m.normals, m.texcoords, m.triangles)
    return sd, scene, mirror


def _rows(scene, s):
    sd = scene.description
    first = sum(len(m.positions) for m in sd.meshes[:s])
    return first, first + len(sd.meshes[s].positions)


@pytest.mark.parametrize("name", sorted(MESHES))
def test_tangents_equal_the_mirror_bit_for_bit(mts, hook, name):
    sd, scene, mirror = hook
    pool, has = scene.vertex_tangents()
    a, b = _rows(scene, MESHES[name])
    want, nrm, _ = mirror[name]
    got = pool[a:b]
    assert got.shape == want.shape
    diff = np.argwhere(bits(got) != bits(want))
    assert len(diff) == 0, (name, diff[:4], got[diff[0][0]], want[diff[0][0]])
    # the zero normals became (1, 0, 0) in the scene's normals as well
    assert np.array_equal(bits(scene.arrays()["vtx_nrm"][a:b]), bits(nrm))


def test_degenerate_mesh_reaches_every_branch(hook):
    """the decisions the mirror took on the degenerate mesh: every `== 0` of the reference came out both ways"""
    sd, scene, mirror = hook
    tan, nrm, made = mirror["degenerate"]
    assert True in made and False in made
    pos, tri, n0, uv, names = tan_cases.degenerate()
    assert np.isfinite(tan).all()
    assert (nrm[18] == (1, 0, 0)).all() and (nrm[22] == (1, 0, 0)).all()
    # an unused vertex gets coordinateSystem(normal): (0, .6, .8) -> s = (0, -.8, .6) up to rounding
    assert np.allclose(tan[21, :3], [0, -0.8, 0.6], atol=1e-6) and np.allclose(tan[22, :3], [0, 0, 1], atol=0)
    # zero uv determinant: dpdu recovered as cross(n, dpdv), not zero; one point: both from coordinateSystem of the vertex normal
    for k in (1, 2, 3, 4, 5):
        v = tri[k]
        assert (np.abs(tan[v, :3]).sum(axis=1) > 0).all() and (np.abs(tan[v, 3:]).sum(axis=1) > 0).all(), names[k]


@pytest.mark.parametrize("name", ["floor", "cylinder"])
def test_tangents_within_the_bound_of_binary64(mts, hook, name):
    """no vertex of a regular mesh is left out: its bound stays under 1e-3 of |dpdu|"""
    sd, scene, mirror = hook
    m = sd.meshes[MESHES[name]]
    want32, _, made = mirror[name]
    val, bound = R.tangents64(m.positions, m.normals, m.texcoords, m.triangles, made)
    pool, _ = scene.vertex_tangents()
    a, b = _rows(scene, MESHES[name])
    got = pool[a:b]
    size = np.linalg.norm(val[:, :3], axis=1)
    left_out = (bound[:, :3].max(axis=1) * R.TOL32 > 1e-3 * size)
    print("%s: worst bound %.3g of |dpdu|, worst error %.3g of the bound" % (name, (bound[:, :3].max(axis=1) * R.TOL32 / size).max(),
          (np.abs(got - val) / (bound * R.TOL32 + R.DENORM)).max()))
    assert not left_out.any()
    ok = R.within_bound(got, val, bound)
    assert ok.all(), (name, np.argwhere(~ok)[:4])
    if name == "floor":
        # the floor's dp/du is one constant vector, and no axis
        exact = tan_cases.floor_tangent()
        assert np.abs(val[:, :3] - exact).max() < 1e-5 and (np.abs(exact[[0, 2]]) > 0.2).all()
    else:
        # the cylinder's dp/du is the circumferential direction of length r = 1, up to the chords: a vertex on the patch's
        # rim sees segments on one side only, whose chord leans by half a segment's angle (pi / 32); at the 7 x 3 vertices
        # inside the patch the two sides cancel
        nrm = m.normals.astype(np.float64)
        lean = np.abs((val[:, :3] * nrm).sum(axis=1))
        assert lean.max() < np.sin(np.pi / 32) * 1.001 and np.sort(lean)[20] < 1e-6 and np.abs(val[:, 2]).max() < 1e-6
        assert np.abs(np.linalg.norm(val[:, :3], axis=1) - 1).max() < 0.01


def _frames(m, dpdu, bound, rng, n, dtype, mutation=None):
    prim, u, v = tan_cases.records(rng, 0, len(m.triangles), n)
    return R.frame(dpdu, m.normals, m.triangles, prim, u, v, dtype, mutation, bound)


@pytest.mark.parametrize("mutation", R.MUTATIONS)
def test_mutations_are_reported(mts, hook, mutation):
    """each mutated restatement leaves the mirror's bound on at least one value of the regular meshes (tangents or frames), or,
    for the one that is about which meshes get tangents, changes the flag table of the hook scene"""
    sd, scene, mirror = hook
    if mutation == "tangents_on_isotropic_mesh":
        assert R.shape_flags(sd) == tan_cases.HOOK_FLAGS and R.shape_flags(sd, mutation) != tan_cases.HOOK_FLAGS
        return
    reported = 0
    for name in ("floor", "cylinder"):
        m = sd.meshes[MESHES[name]]
        want32, _, made = mirror[name]
        val, bound = R.tangents64(m.positions, m.normals, m.texcoords, m.triangles, made, mutation)
        plain, pbound = R.tangents64(m.positions, m.normals, m.texcoords, m.triangles, made)
        reported += int((~R.within_bound(want32, val, np.maximum(bound, pbound))).sum())
        f32, _ = _frames(m, want32[:, :3], None, np.random.RandomState(3), 512, np.float32)
        f64, fb = _frames(m, val[:, :3], bound[:, :3], np.random.RandomState(3), 512, np.float64, mutation)
        p64, pb = _frames(m, plain[:, :3], pbound[:, :3], np.random.RandomState(3), 512, np.float64)
        reported += int((~R.within_bound(f32, f64, np.maximum(fb, pb))).sum())
    print("%s: %d values reported" % (mutation, reported))
    assert reported > 0


@pytest.mark.parametrize("name", ["floor", "cylinder"])
def test_frame_mirror_within_the_bound_and_orthonormal(mts, hook, name):
    sd, scene, mirror = hook
    m = sd.meshes[MESHES[name]]
    want32, _, made = mirror[name]
    val, bound = R.tangents64(m.positions, m.normals, m.texcoords, m.triangles, made)
    f32, _ = _frames(m, want32[:, :3], None, np.random.RandomState(3), 2048, np.float32)
    f64, fb = _frames(m, val[:, :3], bound[:, :3], np.random.RandomState(3), 2048, np.float64)
    assert R.within_bound(f32, f64, fb).all()
    gram = np.einsum("nij,nkj->nik", f64, f64)
    assert np.abs(gram - np.eye(3)).max() < 1e-12
    # right-handed in the reference's sense: t = cross(n, s), so cross(s, t) = n
    assert np.abs(np.cross(f64[:, 0], f64[:, 1]) - f64[:, 2]).max() < 1e-12
    plain = R.plain_frame(f64[:, 2])
    assert np.abs(plain[:, 0] - f64[:, 0]).max() > 0.1, "the tangent frame must differ from Frame(n) on this mesh"


def test_flag_table_and_untouched_meshes(mts, hook):
    sd, scene, mirror = hook
    pool, has = scene.vertex_tangents()
    assert has.tolist() == tan_cases.HOOK_FLAGS == R.shape_flags(sd)
    assert scene.wants_tangents and pool.shape == (scene.sc.n_verts, 6)
    for s in (3, 4, 6):
        a, b = _rows(scene, s)
        assert not pool[a:b].any(), sd.meshes[s].name
    # the texcoords were recorded as mtsgpu_flat_scene_set_mesh_texcoords records them
    uvp, uvh = scene.vertex_texcoords()
    assert uvh.tolist() == [1, 1, 1, 1, 0, 0, 1]
    a, b = _rows(scene, 1)
    assert np.array_equal(bits(uvp[a:b]), bits(sd.meshes[1].texcoords))
    # every array of the scene but the replaced zero normals is what mtsgpu_flatten builds for the isotropic twin
    twin = mts.Scene(tan_cases.hook_scene(mts, isotropic=True))
    assert not twin.wants_tangents and twin.vertex_tangents() == (None, None) and twin.tangent_args() is None
    A, B = scene.arrays(), twin.arrays()
    for key in ("vtx_pos", "tri_idx", "kd_nodes", "kd_indices", "triaccel", "shape_flags", "shape_type"):
        assert np.array_equal(A[key], B[key]), key
    same = np.ones(len(A["vtx_nrm"]), dtype=bool)
    a, b = _rows(scene, 2)
    same[a + 18] = same[a + 22] = False
    assert np.array_equal(bits(A["vtx_nrm"][same]), bits(B["vtx_nrm"][same]))


def _flatten_tangents(mts, sd, texcoords):
    d, keep = sd.to_ctypes()
    tcs = (mts.abi.f32p * len(sd.meshes))()
    for i, t in enumerate(texcoords):
        if t is not None:
            tcs[i] = mts.abi.ptr(t, mts.abi.f32p)
    h = C.c_void_p()
    rc = mts.lib().mtsgpu_flatten_tangents(C.byref(d), C.byref(mts.abi.KdParams()), tcs, C.byref(h))
    msg = mts.lib().mtsgpu_last_error(None).decode()
    if rc == 0:
        has = mts.lib().mtsgpu_flat_scene_shape_has_tangents(h)
        flags = [has[i] for i in range(len(sd.meshes))] if has else None
        mts.lib().mtsgpu_flat_scene_free(h)
        return 0, flags
    return rc, msg


def _one_mesh(mts, make, face_normals, sphere=False):
    sd = mts.scenes.SceneDescription("one")
    b = make(sd)
    pos, tri, nrm, uv = tan_cases.floor()
    if sphere:
        sd.add_sphere((0, 0, 0), 1.0, bsdf=b)
    else:
        sd.add_mesh(pos, tri, bsdf=b, face_normals=face_normals, normals=None if face_normals else nrm)
    sd.point_light((0, 2, 0), 1.0)
    return sd, uv


ANISO = [lambda sd: sd.ward(0.1, 0.3), lambda sd: sd.composite([0.5, 0.5], [sd.lambertian(0.5), sd.ward(0.1, 0.3)]),
         lambda sd: sd.twosided(sd.ward(0.1, 0.3))]


@pytest.mark.parametrize("k", range(3))
def test_new_flatten_call_accepts_and_refuses(mts, k):
    # texcoords and vertex normals: tangents
    sd, uv = _one_mesh(mts, ANISO[k], False)
    assert _flatten_tangents(mts, sd, [uv]) == (0, [1])
    # without texcoords: the reference's message
    rc, msg = _flatten_tangents(mts, sd, [None])
    assert rc != 0 and "texture coordinates are required to generate tangent vectors" in msg and "anisotropic" in msg
    # face normals: accepted, no tangents (trimesh.cpp:562-565); without texcoords still refused
    sd, uv = _one_mesh(mts, ANISO[k], True)
    assert _flatten_tangents(mts, sd, [uv]) == (0, None)
    assert _flatten_tangents(mts, sd, [None])[0] != 0
    # a sphere needs none; an isotropic Ward gets none
    sd, uv = _one_mesh(mts, ANISO[k], False, sphere=True)
    assert _flatten_tangents(mts, sd, [None]) == (0, None)
    sd, uv = _one_mesh(mts, lambda sd: sd.ward(0.2, 0.2), False)
    assert _flatten_tangents(mts, sd, [uv]) == (0, None)
    # non-finite texcoords of a tangent mesh
    sd, uv = _one_mesh(mts, ANISO[k], False)
    bad = uv.copy(); bad[3, 1] = np.nan
    rc, msg = _flatten_tangents(mts, sd, [bad])
    assert rc != 0 and "non-finite" in msg
    assert mts.lib().mtsgpu_flatten_tangents(None, None, None, None) != 0


@pytest.mark.parametrize("k", range(3))
@pytest.mark.parametrize("face_normals", [False, True])
def test_old_flatten_call_refuses_as_before(mts, k, face_normals):
    sd, uv = _one_mesh(mts, ANISO[k], face_normals)
    d, keep = sd.to_ctypes()
    h = C.c_void_p()
    assert mts.lib().mtsgpu_flatten(C.byref(d), C.byref(mts.abi.KdParams()), C.byref(h)) != 0
    msg = mts.lib().mtsgpu_last_error(None).decode()
    assert "texture coordinates are required to generate tangent vectors" in msg and "anisotropic" in msg
    # and Scene(sd) goes through it when no mesh has texcoords
    with pytest.raises(mts.MtsGpuError, match="texture coordinates are required"):
        mts.Scene(sd)


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
    assert "#define MTSGPU_ABI_VERSION 8" in header
