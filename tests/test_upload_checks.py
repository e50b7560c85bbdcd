"""The pure half of the upload calls (csrc/scene_layout.cpp, csrc/host.h: checkScene, layoutScene, planTextures, planCloth,
claimRefusal) without a GPU: tests/upload_harness/harness.cpp, a stand-alone program built once per session with
AddressSanitizer and UBSan, reads a scene flattened on the CPU (tests/upload_cases.py) with one planted fault and prints the
refusal, or the digests of everything the calls would copy to the device.

 * every refusal is asserted by a substring of its text; the unplanted scenes are accepted;
 * the digests equal tests/golden/upload_layout.json, which was recorded from the upload() of the commit BEFORE the split
   (a throw-away log line in its ctx.h, run on an MI355X over layout_scenes), not from these functions;
 * a non-zero exit status or anything on stderr -- a sanitizer report -- fails the test."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import geom_cases
import upload_cases as U

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
pytestmark = pytest.mark.skipif(HIPCC is None, reason="no hipcc to build the harness with")
F = np.float32
NAN = np.float32(np.nan)
COLORS, TEXTURES, MASKS, SNOW, CLOTH = 1, 2, 4, 8, 16       # host.h: Family


@pytest.fixture(scope="session")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("upload_harness") / "harness")
    subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(HERE, "upload_harness", "harness.cpp"), os.path.join(ROOT, "mitsuba-renderer_amd", "csrc", "scene_layout.cpp"),
                    "-o", exe], check=True, capture_output=True)
    return exe


@pytest.fixture(scope="session")
def run(harness, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("upload_cases")
    count = [0]

    def call(verb, case=None, *more):
        args = [harness, verb]
        if case is not None:
            count[0] += 1
            path = str(tmp / ("case%d.bin" % count[0]))
            U.write_case(path, case)
            args.append(path)
        p = subprocess.run(args + [str(m) for m in more], capture_output=True, text=True)
        assert p.returncode == 0 and p.stderr == "", "harness %s: exit %d\n%s" % (verb, p.returncode, p.stderr[-3000:])
        return p.stdout
    return call


@pytest.fixture(scope="session")
def cases(mts):
    """name -> a function that returns a fresh copy of the case of that scene (the flattening is done once)"""
    import cyl_cases
    import tan_cases
    import test_gpu_cloth
    import test_gpu_mask
    import test_gpu_snow
    K = geom_cases.kernel_constants()
    S = mts.scenes
    makers = dict(U.layout_scenes(mts))
    makers.update(cyl_one=cyl_cases.scene_description(mts, "one"), snow_refusals=test_gpu_snow._refusal_scene(mts),
                  cloth_refusals=test_gpu_cloth._refusal_scene(mts))
    made = {}

    def get(name):
        if name not in made:
            sd = makers[name]
            sd = sd[0] if isinstance(sd, tuple) else sd
            made[name] = U.case_of(mts, mts.Scene(sd), K["stack_levels"] - 2, K["top_nodes"])
        c = made[name]
        return {k: (dict(v) if k == "hdr" else np.array(v, copy=True)) for k, v in c.items()}
    get.top_nodes = K["top_nodes"]
    return get


def _first(case, pred):
    return next(s for s in range(case["hdr"]["n_shapes"]) if pred(s))


def _shape_of_type(case, t):
    return _first(case, lambda s: case["shape_type"][s] == t)


def _prim(case, s):
    return int(case["shape_tri_offset"][s])


# --- the trees of test_malformed_trees_are_refused ---------------------------------------------------------------------
def _inner(i, left, axis=0):
    return [((left - i) << 2) | axis, 0]


LEAF = [0x80000000, 0]


def _tree(c, nodes):
    c["kd_nodes"] = np.array(nodes, dtype=np.uint32)
    c["hdr"]["n_nodes"] = len(nodes)


def _chain(c, depth=60):
    n = 2 * depth + 1
    chain = np.zeros((n, 2), dtype=np.uint32)
    for k in range(depth):
        i = 0 if k == 0 else 2 * k - 1
        chain[i, 0] = ((2 * k + 1 - i) << 2) | 0
        chain[2 * k + 2, 0] = 0x80000000
    chain[2 * depth - 1, 0] = 0x80000000
    c["kd_nodes"] = chain
    c["hdr"]["n_nodes"] = n


def _set(name, index, value):
    def f(c):
        c[name][index] = value
    return f


def _hdr(**kw):
    return lambda c: c["hdr"].update(kw)


def _drop(*names):
    def f(c):
        for n in names:
            del c[n]
    return f


def _both(*fs):
    def f(c):
        for g in fs:
            g(c)
    return f


def _leaf_out_of_range(c):
    i = int(np.nonzero(c["kd_nodes"][:, 0] & 0x80000000)[0][0])
    c["kd_nodes"][i, 1] = c["hdr"]["n_indices"] + 1


def _mesh_as_sphere(c):
    s = _first(c, lambda s: c["shape_type"][s] == 0 and c["shape_tri_offset"][s + 1] - c["shape_tri_offset"][s] > 1)
    c["shape_type"][s] = 1


def _on(t, name, col, value):
    """set column `col` of row (the first shape of type t) of a per-shape array"""
    def f(c):
        s = _shape_of_type(c, t)
        if col is None:
            c[name][s] = value
        else:
            c[name][s, col] = value
    return f


def _prim_word(t, word, value):
    return lambda c: c["triaccel"].__setitem__((_prim(c, _shape_of_type(c, t)), word), value)


def _cyl_bsdf_type(c):
    c["bsdf_type"][c["shape_bsdf"][_shape_of_type(c, 2)]] = 2 | 0x100


def _tangents_on(pred):
    def f(c):
        n = c["hdr"]["n_shapes"]
        c["vtx_dpdu"] = np.zeros((max(c["hdr"]["n_verts"], 1), 3), dtype=F)
        c["shape_has_tangents"] = np.zeros(n, dtype=np.uint32)
        c["shape_has_tangents"][_first(c, lambda s: pred(c, s))] = 1
        c["hdr"]["with_tangents"] = 1
    return f


def _anisotropic_mesh(c):
    s = _first(c, lambda s: c["shape_type"][s] == 0 and c["shape_bsdf"][s] >= 0)
    b = c["shape_bsdf"][s]
    c["bsdf_type"][b] = 8
    c["bsdf_params"][b, 1:3] = (0.1, 0.3)


def _nan_tangent(c):
    s = _first(c, lambda s: c["shape_has_tangents"][s])
    c["vtx_dpdu"][c["tri_idx"][_prim(c, s), 0], 1] = NAN


def _area(c):
    """an area luminaire and its shape"""
    l = int(c["shape_lum"].max())
    return l, int(c["lum_shape"][l])


def _unlink(c):
    l, s = _area(c)
    c["shape_lum"][s] = -1
    return l


def _relink(c):
    l, s = _area(c)
    c["lum_shape"][l] = (s + 1) % c["hdr"]["n_shapes"]


def _bad_lum_shape(c):
    c["lum_shape"][_unlink(c)] = c["hdr"]["n_shapes"]


def _unknown_lum(c):
    c["lum_type"][_unlink(c)] = 99


def _cdf_size(c):
    l, _ = _area(c)
    c["lum_cdf_offset"][l + 1:] += 1


def _sphere_emitter_cdf(c):
    """a sphere that emits is given a triangle CDF; or a sphere becomes the emitter of a mesh's luminaire, which keeps its CDF"""
    l, s = _area(c)
    if c["shape_type"][s] == 1:
        c["lum_cdf_offset"][l + 1:] += 1
        return
    t = _shape_of_type(c, 1)
    c["shape_lum"][s] = -1
    c["shape_lum"][t] = l
    c["lum_shape"][l] = t


def _env(c):
    return int(c["hdr"]["background_lum"])


def _hole_before_shape_0(c):
    c["shape_tri_offset"][0] = 1
    c["triaccel"][0, 10] = c["hdr"]["n_shapes"]


SCENE_REFUSALS = [
    ("cornell_c1", _hdr(n_nodes=0), "scene has no kd-tree"),
    ("cornell_c1", _hdr(n_lums=0), "scene has no luminaire"),
    ("cornell_c1", _leaf_out_of_range, "index range out of bounds"),
    ("cornell_c1", lambda c: c["kd_nodes"].__setitem__((0, 0), c["kd_nodes"][0, 0] | 0x40000000), "indirection nodes are not supported"),
    ("cornell_c1", lambda c: c["kd_nodes"].__setitem__((0, 0), c["kd_nodes"][0, 0] | 3), "bad axis/child offset"),
    ("cornell_c1", lambda c: _tree(c, [_inner(0, 1), _inner(1, 3), _inner(2, 3), LEAF, LEAF, LEAF, LEAF]), "child of two nodes"),
    ("cornell_c1", lambda c: _tree(c, [_inner(0, 1), LEAF, LEAF, LEAF, LEAF]), "2 of 5 nodes are unreachable from the root"),
    ("cornell_c1", _chain, "kd-tree deeper than"),
    ("cornell_c1", lambda c: c["kd_indices"].__setitem__(0, c["hdr"]["n_tris"]), "kd index 0 out of range"),
    ("cornell_c1", _drop("shape_params"), "shape_type and shape_params must both be given or both be NULL"),
    ("cyl_mixed", _hdr(accepts_cylinders=0), "is a cylinder: its derived block travels beside the scene"),
    ("cyl_mixed", _drop("cylinders"), "was given no cylinder blocks"),
    ("cornell_c1", _set("shape_type", 0, 7), "unknown shape type"),
    ("cornell_c1", lambda c: c["shape_tri_offset"].__setitem__(0, c["shape_tri_offset"][1] + 1), "shape_tri_offset not monotone"),
    ("cornell_c1", lambda c: c["shape_tri_offset"].__setitem__(1, c["hdr"]["n_tris"] + 1), "shape_tri_offset not monotone"),
    ("cornell_c1", _mesh_as_sphere, "a non-mesh shape must own exactly one primitive"),
    ("spheres", _on(1, "shape_params", 0, NAN), "non-finite parameter"),
    ("cyl_mixed", _on(2, "cylinders", 3, NAN), "non-finite cylinder parameter"),
    ("cyl_mixed", _on(2, "cylinders", 24, -1.0), "a cylinder needs radius > 0 and length > 0"),
    ("cyl_one", _on(2, "shape_bsdf", None, -1), "a cylinder without a BSDF is not served yet"),
    ("cyl_mixed", _cyl_bsdf_type, "is of type 2 under twosided, not served on a cylinder yet"),
    ("cyl_mixed", _on(2, "shape_lum", None, 0), "a cylinder cannot carry an area luminaire"),
    ("spheres", _on(1, "shape_params", 3, 0.0), "zero radius"),
    ("cornell_c1", _prim_word(0, 0, 0xFFFFFFFF), "a mesh triangle is marked as a shape"),
    ("cornell_c1", lambda c: c["tri_idx"].__setitem__((0, 0), c["hdr"]["n_verts"]), "triangle vertex index out of range"),
    ("spheres", _prim_word(1, 0, 0), "must have k = KNoTriangleFlag"),
    ("cornell_c1", _set("triaccel", (0, 10), 1), "TriAccel 0: shape index does not match shape_tri_offset"),
    ("cornell_c1", lambda c: c["shape_bsdf"].__setitem__(0, c["hdr"]["n_bsdfs"]), "bad BSDF/luminaire index"),
    ("cornell_c1", lambda c: c["shape_lum"].__setitem__(0, c["hdr"]["n_lums"]), "bad BSDF/luminaire index"),
    ("cornell_c1", _relink, "luminaire link is inconsistent"),
    ("cornell_c1", lambda c: c["shape_tri_offset"].__setitem__(-1, c["hdr"]["n_tris"] - 1), "shape_tri_offset does not cover all triangles"),
    ("cornell_c1", _hole_before_shape_0, "TriAccel 0: shape index out of range"),
    ("cornell_c1", _set("bsdf_type", 0, 99), "BSDF 0: unknown type"),
    ("spheres", _tangents_on(lambda c, s: c["shape_type"][s] == 1), "only a triangle mesh can carry tangents"),
    ("cornell_c1", _tangents_on(lambda c, s: c["shape_type"][s] == 0 and not c["shape_flags"][s] & 1), "tangents need vertex normals"),
    ("cornell_c1", _anisotropic_mesh, "texture coordinates are required to generate tangent vectors"),
    ("tan_mixed", _nan_tangent, "non-finite tangent at vertex"),
    ("cornell_c1", _bad_lum_shape, "luminaire 0: bad shape"),
    ("spheres", _sphere_emitter_cdf, "a non-mesh emitter has no triangle CDF"),
    ("cornell_c1", _cdf_size, "CDF size mismatch"),
    ("envlit", _hdr(background_lum=0xFFFFFFFF), "the envmap must be the background luminaire"),
    ("envlit", _drop("env_cdf"), "missing or oversized environment map"),
    ("envlit", _hdr(env_width=16385), "missing or oversized environment map"),
    ("envlit", _set("env_cdf", 0, 1e9), "the environment map's CDF is not monotone"),
    ("envlit", lambda c: c["lum_params"].__setitem__((_env(c), 0), NAN), "non-finite parameter"),
    ("cornell_tex_sky", _hdr(background_lum=0xFFFFFFFF), "the sky must be the background luminaire"),
    ("cornell_tex_sky", lambda c: c["lum_params"].__setitem__((_env(c), 1), NAN), "non-finite sky parameter"),
    ("cornell_c1", _unknown_lum, "luminaire 0: unknown type"),
    ("cornell_c1", lambda c: c["hdr"].update(background_lum=c["hdr"]["n_lums"]), "background luminaire out of range"),
]


@pytest.mark.parametrize("scene,plant,text", SCENE_REFUSALS, ids=["%02d %s" % (i, r[2][:40]) for i, r in enumerate(SCENE_REFUSALS)])
def test_scene_refusals(run, cases, scene, plant, text):
    """one planted fault, the refusal of checkScene in its present words"""
    c = cases(scene)
    plant(c)
    assert text in run("check", c)


def test_intact_scenes_are_accepted(run, cases, mts):
    for name, _ in U.layout_scenes(mts):
        c = cases(name)
        assert run("check", c) == "\n", name
        assert run("textures", c) == "\n", name
        assert run("cloth", c) == "\n", name
    for name in ("cyl_one", "snow_refusals", "cloth_refusals"):
        assert run("check", cases(name)) == "\n", name


# --- the texture calls -------------------------------------------------------------------------------------------------
def _tex(c, k):
    """the twelve words of texture k as float32 and as uint32 views of the section"""
    return c["textures"].view(F).reshape(-1, 12), c["textures"].view(np.uint32).reshape(-1, 12)


def _tex_word(k, word, value, as_float=True):
    def f(c):
        _tex(c, k)[0 if as_float else 1][k, word] = value
    return f


def _masks(c):
    return c["bsdf_mask"].view(np.uint32).reshape(-1, 6)


def _mask_word(pred, word, value, as_float=False):
    def f(c):
        m = _masks(c)
        b = next(b for b in range(len(m)) if pred(c, m, b))
        (m.view(F) if as_float else m)[b, word] = value
    return f


def _textured_bsdf(c):
    return int(np.nonzero(c["bsdf_slot_texture"].reshape(-1, 2)[:, 0] >= 0)[0][0])


def _held(section, value, n="n_bsdfs", dtype=np.uint32, width=1):
    """entry b (chosen by the case) in the hands of another family"""
    def f(c, b):
        a = np.full((c["hdr"][n], width), -1 if dtype == np.int32 else 0, dtype=dtype)
        a[b] = value
        c[section] = a
    return f


def _with_mask_table(c, kind=1):
    c["bsdf_mask"] = np.zeros((c["hdr"]["n_bsdfs"], 6), dtype=np.uint32)
    c["bsdf_mask"][0, 0] = kind
    c["tex_call"] = np.zeros(1, dtype=np.uint32)
    c["hdr"]["with_bitmaps"] = 1


def _composite(c):
    return int(np.nonzero((c["bsdf_type"] & 0xFF) == 9)[0][0])


def _composite_child(c):
    p = c["bsdf_params"][_composite(c)]
    return int(p[1 + int(p[0])])


def _slot_on_composite_child(c):
    t = np.full((c["hdr"]["n_bsdfs"], 2), -1, dtype=np.int32)
    t[_composite_child(c), 0] = 0
    c["bsdf_slot_texture"] = t


def _unused_masked_bsdf(c):
    """one more BSDF that no shape uses, with a textured mask whose texture's offset leaves the range of the cast"""
    n = c["hdr"]["n_bsdfs"]
    c["hdr"]["n_bsdfs"] = n + 1
    c["bsdf_type"] = np.append(c["bsdf_type"], np.uint32(0))
    c["bsdf_params"] = np.concatenate([c["bsdf_params"], np.full((1, 16), 0.5, dtype=F)])
    if "bsdf_slot_texture" in c:
        c["bsdf_slot_texture"] = np.concatenate([c["bsdf_slot_texture"].reshape(-1, 2), np.full((1, 2), -1, dtype=np.int32)])
    if "bsdf_color_slots" in c:
        c["bsdf_color_slots"] = np.append(c["bsdf_color_slots"], np.uint32(0))
    extra = np.zeros((1, 6), dtype=np.uint32)
    extra[0, 0], extra[0, 1] = 2, c["hdr"]["n_textures"]
    c["bsdf_mask"] = np.concatenate([_masks(c), extra])
    t = np.zeros((1, 12), dtype=F)
    t.view(np.uint32)[0, 0] = 0
    t[0, 1], t[0, 3], t[0, 4] = 2e9, 1.0, 1.0
    c["textures"] = np.concatenate([c["textures"].view(F).reshape(-1, 12), t]).view(np.uint8).ravel() if "textures" in c else t
    c["hdr"]["n_textures"] += 1


def _snow_holds_textured(c):
    _held("in_snow_kind", 1)(c, _textured_bsdf(c))


def _snow_holds_masked(c):
    _held("in_snow_kind", 1)(c, next(b for b in range(len(_masks(c))) if _masks(c)[b, 0]))
    c.pop("bsdf_slot_texture", None)


TEXTURE_REFUSALS = [
    ("cornell_tex_sky", _drop("shape_has_uv"), "vtx_uv and shape_has_uv must both be given or both be NULL"),
    ("cornell_tex_sky", _drop("textures"), "n_textures without textures"),
    ("cornell_tex_sky", _hdr(n_textures=(1 << 20) + 1), "at most 2^20 textures"),
    ("cornell_bmp", _drop("bitmaps"), "n_bitmaps without bitmaps"),
    ("cornell_bmp", _hdr(n_bitmaps=(1 << 20) + 1), "at most 2^20 bitmaps"),
    ("cornell_tex_sky", _tex_word(0, 0, 2, False), "texture 0: unknown kind 2"),
    ("cornell_bmp", _tex_word(0, 0, 3, False), "texture 0: unknown kind 3"),
    ("cornell_tex_sky", _tex_word(0, 11, NAN), "texture 0: non-finite parameter"),
    ("cornell_bmp", _set("bitmaps", (0, 0), 0), "bitmap 0: zero dimension (0 x"),
    ("cornell_bmp", _set("bitmaps", (0, 2), 4), "bitmap 0: unknown wrap mode 4"),
    ("cornell_bmp", _set("bitmaps", (0, 3), 1), "bitmap 0: reserved word is not zero"),
    ("cornell_bmp", _both(_set("bitmaps", (0, 0), 65536), _set("bitmaps", (0, 1), 65536)), "texels in all (the pool is indexed with one uint32)"),
    ("cornell_bmp", _drop("bitmap_texels"), "bitmap 0: no texels"),
    ("cornell_bmp", _set("bitmap_texels", 4, -0.5), "bitmap 0: texel (1, 0) is negative or not finite"),
    ("cornell_bmp", lambda c: c["texture_bitmap"].__setitem__(int(np.nonzero(c["texture_bitmap"] >= 0)[0][0]), 99), "bitmap index 99 out of range"),
    ("cornell_tex_sky", lambda c: c["bsdf_slot_texture"].__setitem__((_textured_bsdf(c), 0), 99), "slot 0 names texture 99 of"),
    ("cornell_tex_sky", lambda c: c["bsdf_slot_texture"].__setitem__((_textured_bsdf(c), 1), 0), "uv texture in slot 1, beyond the 1 texture slot(s) of its type"),
    ("cornell_tex_sky", lambda c: _held("in_color_slots", 1)(c, _textured_bsdf(c)), "slot 0 has a uv texture and takes vertex colours as well"),
    ("mask_mixed", _slot_on_composite_child, "has a uv texture: a composite's children keep constant parameters"),
    ("cyl_mixed", _with_mask_table, "the mask BSDF is not served in a scene with a cylinder yet"),
    ("mask_mixed", _mask_word(lambda c, m, b: True, 0, 3), "unknown mask kind 3"),
    ("mask_mixed", _mask_word(lambda c, m, b: True, 5, 1), "the reserved word of its mask is not zero"),
    ("mask_mixed", _mask_word(lambda c, m, b: True, 2, NAN, True), "the opacity of its mask is not finite"),
    ("mask_mixed", _mask_word(lambda c, m, b: m[b, 0] == 2, 1, 99), "its mask names texture 99 of"),
    ("mask_mixed", _mask_word(lambda c, m, b: b == _composite(c), 0, 1), "a mask around a composite is not supported"),
    ("mask_mixed", _mask_word(lambda c, m, b: b == _composite_child(c), 0, 1), "has a mask: a mask is the outermost adapter"),
    ("cornell_tex_sky", _snow_holds_textured, "the entry has a uv texture and a snow record, whose BRDF has no texture slot"),
    ("mask_mixed", _snow_holds_masked, "the entry has a mask and a snow record: a mask around a snow BRDF is not supported"),
    ("spheres", lambda c: (_with_mask_table(c, 0), c.update(vtx_uv=np.zeros((max(c["hdr"]["n_verts"], 1), 2), dtype=F),
                                                              shape_has_uv=(c["shape_type"] == 1).astype(np.uint32))), "only a triangle mesh can carry texture coordinates"),
    ("cornell_tex_sky", lambda c: c["vtx_uv"].__setitem__((c["tri_idx"][_prim(c, _first(c, lambda s: c["shape_has_uv"][s])), 0], 0), NAN), "non-finite texcoord at vertex"),
    ("cornell_tex_sky", _tex_word(0, 3, 1e30), "maps a texcoord outside the range of the (int) cast (|2 uv'| >= 2^31 - 2^16)"),
    ("cornell_bmp", lambda c: _tex_word(int(np.nonzero(c["texture_bitmap"] >= 0)[0][0]), 1, 1e30)(c), "(|uv' * size| >= 2^31 - 2^16)"),
    ("mask_mixed", lambda c: _tex_word(int(next(m[1] for m in _masks(c) if m[0] == 2)), 1, 1e30)(c), ": the opacity of its mask: texture"),
    ("mask_mixed", _unused_masked_bsdf, "the opacity of its mask: texture"),
]


@pytest.mark.parametrize("scene,plant,text", TEXTURE_REFUSALS, ids=["%02d %s" % (i, r[2][:40]) for i, r in enumerate(TEXTURE_REFUSALS)])
def test_texture_refusals(run, cases, scene, plant, text):
    """one planted fault, the refusal of the texture calls after their free (planTextures) in its present words"""
    c = cases(scene)
    plant(c)
    out = run("textures", c)
    assert text in out
    if text == "the opacity of its mask: texture":       # the BSDF no shape uses: reported by BSDF, not by shape
        assert out.startswith("BSDF ")


# --- mtsgpu_set_cloth_bsdfs --------------------------------------------------------------------------------------------
def _woven(c):
    return int(np.nonzero(c["bsdf_weave"] >= 0)[0][0])


def _weave_on_composite_child(c):
    c["bsdf_weave"][_composite_child(c)] = 0


def _cloth_on(c):
    """a cloth table on a scene that has none: one plain weave on BSDF 0"""
    c["hdr"]["n_weaves"] = 1
    w = np.zeros((1, 20), dtype=np.uint32)
    w.view(F)[0, [0, 1, 2, 3, 4, 5]] = (0.01, 4.0, 0.0, 0.5, 1.0, 1.0)
    w[0, 6], w[0, 7] = 1, 1
    w.view(F)[0, 14:18] = 1.0
    w[0, 18], w[0, 19] = 1, 1
    y = np.zeros(14, dtype=np.uint32)
    y.view(F)[1:8] = (0.0, 0.5, 0.0, 1.0, 1.0, 0.5, 0.5)
    c.update(weaves=w, weave_patterns=np.ones(1, dtype=np.uint32), weave_yarns=y)
    c["bsdf_weave"] = np.full(c["hdr"]["n_bsdfs"], -1, dtype=np.int32)
    c["bsdf_weave"][0] = 0


def _woven_mesh(c, pred):
    return _first(c, lambda s: c["shape_type"][s] == 0 and c["shape_bsdf"][s] >= 0 and c["bsdf_weave"][c["shape_bsdf"][s]] >= 0 and pred(s))


def _no_texcoords(c):
    s = _woven_mesh(c, lambda s: True)
    c["shape_has_uv"][s] = 0


def _no_tangents(c):
    s = _woven_mesh(c, lambda s: c["shape_flags"][s] & 1)
    c["shape_has_tangents"][s] = 0


def _huge_uv(c):
    n = c["hdr"]["n_shapes"]
    c["in_shape_has_uv"] = np.ones(n, dtype=np.uint32)
    c["in_uv_range"] = np.tile(np.float64([0.0, 1e12, 0.0, 1.0]), (n, 1))


CLOTH_REFUSALS = [
    ("cyl_mixed", _cloth_on, "the cloth BRDF is not served in a scene with a cylinder yet"),
    ("cloth_film", _drop("weaves", "weave_patterns", "weave_yarns"), "n_weaves without weaves"),
    ("cloth_film", _hdr(n_weaves=(1 << 20) + 1), "at most 2^20 weaves"),
    ("cloth_film", _set("weaves", (0, 6), 0), "weave 0: zero tile dimension"),
    ("cloth_film", lambda c: c["bsdf_weave"].__setitem__(_woven(c), 99), "weave index 99 out of range"),
    ("cloth_film", lambda c: c["bsdf_type"].__setitem__(_woven(c), 2), "a weave sits on a Lambertian entry (twosided allowed), not on type word 2"),
    ("cloth_film", lambda c: _held("in_color_slots", 1)(c, _woven(c)), "a cloth BRDF has no texture slot, and the entry takes vertex colours"),
    ("cloth_film", lambda c: _held("in_slot_tex", 0, dtype=np.int32, width=2)(c, _woven(c)), "a cloth BRDF has no texture slot, and the entry has a uv texture"),
    ("cloth_film", lambda c: _held("in_mask_kind", 1)(c, _woven(c)), "a mask around a cloth BRDF is not supported"),
    ("cloth_film", lambda c: _held("in_snow_kind", 1)(c, _woven(c)), "the entry has a snow record and a weave"),
    ("cloth_refusals", _both(_cloth_on, _weave_on_composite_child), "has a weave: the composite's loop would run it as a Lambertian"),
    ("cloth_film", _no_texcoords, "needs texture coordinates: a mesh without them must be given some"),
    ("cloth_film", _no_tangents, "is anisotropic: a mesh with vertex normals needs its tangents"),
    ("cloth_film", _huge_uv, "a texcoord maps outside the range of the (int) cast (|xy| >= 2^31 - 2^16)"),
]


@pytest.mark.parametrize("scene,plant,text", CLOTH_REFUSALS, ids=["%02d %s" % (i, r[2][:40]) for i, r in enumerate(CLOTH_REFUSALS)])
def test_cloth_refusals(run, cases, scene, plant, text):
    """one planted fault, the refusal of mtsgpu_set_cloth_bsdfs after its free (planCloth) in its present words"""
    c = cases(scene)
    plant(c)
    assert text in run("cloth", c)


# --- the claims function -----------------------------------------------------------------------------------------------
CLAIMS = {      # (claimant, holder) -> the refusal, in the words of the claiming call; every other ordered pair is granted
    (COLORS, TEXTURES): "slot 0 takes vertex colours and has a uv texture as well",
    (COLORS, SNOW): "the entry takes vertex colours and has a snow record, whose BRDF has no texture slot",
    (COLORS, CLOTH): "the entry takes vertex colours and has a weave, whose BRDF has no texture slot",
    (TEXTURES, COLORS): "slot 0 has a uv texture and takes vertex colours as well",
    (TEXTURES, SNOW): "the entry has a uv texture and a snow record, whose BRDF has no texture slot",
    (TEXTURES, CLOTH): "the entry has a uv texture and a weave, whose BRDF has no texture slot",
    (MASKS, SNOW): "the entry has a mask and a snow record: a mask around a snow BRDF is not supported",
    (MASKS, CLOTH): "the entry has a mask and a weave: a mask around a cloth BRDF is not supported",
    (SNOW, COLORS): "a snow BRDF has no texture slot, and the entry takes vertex colours",
    (SNOW, TEXTURES): "a snow BRDF has no texture slot, and the entry has a uv texture",
    (SNOW, MASKS): "a mask around a snow BRDF is not supported",
    (SNOW, CLOTH): "the entry has a weave and a snow record",
    (CLOTH, COLORS): "a cloth BRDF has no texture slot, and the entry takes vertex colours",
    (CLOTH, TEXTURES): "a cloth BRDF has no texture slot, and the entry has a uv texture",
    (CLOTH, MASKS): "a mask around a cloth BRDF is not supported",
    (CLOTH, SNOW): "the entry has a snow record and a weave",
}
FAMILIES = (COLORS, TEXTURES, MASKS, SNOW, CLOTH)


@pytest.mark.parametrize("claimant", FAMILIES)
def test_claims(run, claimant):
    """claimRefusal for every ordered pair of families: each family claims entry 0 while each other one holds it"""
    for holder in FAMILIES:
        if holder == claimant:
            continue
        out = run("claim", None, claimant, holder, 1)
        want = CLAIMS.get((claimant, holder))
        assert out == ("BSDF 0: %s\n" % want if want else "\n"), (claimant, holder)
        assert run("claim", None, claimant, holder, 0) == "\n"          # nothing claimed, nothing refused
    if claimant in (COLORS, TEXTURES):       # the second slot is named as such
        other = TEXTURES if claimant == COLORS else COLORS
        assert "BSDF 0: slot 1 " in run("claim", None, claimant, other, 2)


# --- the layout --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def golden():
    with open(os.path.join(HERE, "golden", "upload_layout.json")) as fh:
        return json.load(fh)


def _digests(out):
    return [(n, int(c), h) for n, c, h in (line.split() for line in out.splitlines())]


def test_layout_equals_the_recording(run, cases, golden, mts):
    """every array the upload call and the setters copy to the device, for every scene of the list: element count and FNV-1a 64
    as the parent commit's upload() saw them"""
    names = [n for n, _ in U.layout_scenes(mts)]
    assert sorted(names) == sorted(golden)
    for name in names:
        c = cases(name)
        assert c["hdr"]["n_nodes"] == golden[name]["n_nodes"], name
        got = [[cnt, h] for _, cnt, h in _digests(run("layout", c))]
        assert got == golden[name]["arrays"], name
    assert cases("cornell_c1")["hdr"]["n_nodes"] < cases.top_nodes < cases("cornell_c3_40_3")["hdr"]["n_nodes"]       # padding; treelets
    fuzz = cases("fuzz_0")
    assert (fuzz["shape_bsdf"] < 0).any()


def test_layout_digest_sees_one_word(run, cases):
    """the planted error: one word of one laid-out array changes that array's digest and no other"""
    c = cases("mask_mixed")
    base = _digests(run("layout", c))
    for i in (0, 1, 2, 8, len(base) - 1):
        got = _digests(run("layout", c, i, 5))
        assert [k for k in range(len(base)) if got[k] != base[k]] == [i]
