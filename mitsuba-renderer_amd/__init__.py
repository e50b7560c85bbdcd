"""mitsuba-renderer_amd: MI355X-native path-tracing hot path behind Mitsuba 0.2.1's
integrator interface.

Host-side mirror of the reference's objects for this path, over the C ABI of
include/mtsgpu.h (libmtsgpu.so, built by csrc/Makefile):

    Scene          <- Scene + ShapeKDTree after Scene::initialize()   (src/librender/scene.cpp:291-332)
    PerspectiveCamera  <- PerspectiveCameraImpl                      (src/cameras/perspective.cpp)
    MIPathTracer   <- the `path` integrator plugin                   (src/integrators/path/path.cpp)

There is no CPU fallback: every compute call raises if libmtsgpu.so or a gfx950
device is missing.  (The CPU oracle lives in oracle/ and is test infrastructure.)"""
import ctypes as C
import os
import subprocess

import numpy as np

from . import abi, scenes, filmreduce, testmode  # noqa: F401
from .testmode import write_mfile, analyze  # noqa: F401
from .scenes import load_weave, Weave, Yarn  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
# MTSGPU_LIB selects an experiment build (tools/build_variant.sh); the product is libmtsgpu.so next to this file
LIB_PATH = os.environ.get("MTSGPU_LIB") or os.path.join(_HERE, "libmtsgpu.so")

EXPORTS = [
    "mtsgpu_create", "mtsgpu_destroy", "mtsgpu_last_error", "mtsgpu_abi_version", "mtsgpu_source_hash", "mtsgpu_abi_sizeof", "mtsgpu_set_stream",
    "mtsgpu_upload_scene", "mtsgpu_set_camera", "mtsgpu_set_integrator", "mtsgpu_set_direct_integrator", "mtsgpu_set_sampler",
    "mtsgpu_set_tiles", "mtsgpu_set_rfilter", "mtsgpu_set_film_edges", "mtsgpu_tabulate_filter", "mtsgpu_set_film_buffer", "mtsgpu_set_options", "mtsgpu_render", "mtsgpu_sync",
    "mtsgpu_read_film", "mtsgpu_clear_film", "mtsgpu_get_stats", "mtsgpu_trace_rays", "mtsgpu_ld_tables",
    "mtsgpu_li_samples", "mtsgpu_flatten", "mtsgpu_flat_scene_get", "mtsgpu_flat_scene_free",
    "mtsgpu_flat_scene_kdstats", "mtsgpu_make_camera", "mtsgpu_make_camera_ortho", "mtsgpu_load_serialized", "mtsgpu_loaded_mesh_free",
    "mtsgpu_make_camera_crop", "mtsgpu_hbm_triad", "mtsgpu_sampler_values", "mtsgpu_random_values", "mtsgpu_set_tuning", "mtsgpu_gather_roof",
    "mtsgpu_create_multi", "mtsgpu_group_destroy", "mtsgpu_group_size", "mtsgpu_group_ctx", "mtsgpu_group_last_error",
    "mtsgpu_group_upload_scene", "mtsgpu_group_set_camera", "mtsgpu_group_set_integrator", "mtsgpu_group_set_sampler",
    "mtsgpu_group_set_rfilter", "mtsgpu_group_render", "mtsgpu_group_last_reduce_kind", "mtsgpu_group_rccl_ranks", "mtsgpu_group_reduce_note", "mtsgpu_bsdf_eval", "mtsgpu_bsdf_eval_table", "mtsgpu_replay_roof", "mtsgpu_group_set_tuning",
    "mtsgpu_sky_configure", "mtsgpu_lum_eval", "mtsgpu_scene_lum_eval", "mtsgpu_pass_samples",
    "mtsgpu_set_film_statistics", "mtsgpu_read_film_statistics", "mtsgpu_film_statistics_form", "mtsgpu_group_set_film_statistics",
    "mtsgpu_set_vertex_colors", "mtsgpu_group_set_vertex_colors", "mtsgpu_flat_scene_set_mesh_colors", "mtsgpu_flat_scene_vertex_colors",
    "mtsgpu_flat_scene_shape_has_colors", "mtsgpu_loaded_mesh_colors", "mtsgpu_vertex_color_eval", "mtsgpu_bsdf_eval_colored",
    "mtsgpu_set_uv_textures", "mtsgpu_group_set_uv_textures", "mtsgpu_flat_scene_set_mesh_texcoords", "mtsgpu_flat_scene_vertex_texcoords",
    "mtsgpu_flat_scene_shape_has_texcoords", "mtsgpu_loaded_mesh_texcoords", "mtsgpu_uv_texture_eval", "mtsgpu_bsdf_eval_slots",
    "mtsgpu_flatten_tangents", "mtsgpu_flat_scene_vertex_tangents", "mtsgpu_flat_scene_shape_has_tangents", "mtsgpu_upload_scene_tangents",
    "mtsgpu_group_upload_scene_tangents", "mtsgpu_shading_frame_eval", "mtsgpu_bin_entries",
    "mtsgpu_set_uv_bitmap_textures", "mtsgpu_group_set_uv_bitmap_textures", "mtsgpu_bitmap_texture_eval", "mtsgpu_ldr_texels",
    "mtsgpu_camera_rays",
]
# the mask BSDF's entry points: an extension declared in include/mtsgpu_mask.h, next to the list of mtsgpu.h that ABI version 8 fixes
MASK_EXPORTS = ["mtsgpu_set_uv_masked_textures", "mtsgpu_group_set_uv_masked_textures", "mtsgpu_bsdf_eval_masked"]
# the snow BRDFs' entry points (wiscombe, hanrahankrueger): the extension declared in include/mtsgpu_snow.h
SNOW_EXPORTS = ["mtsgpu_wiscombe_configure", "mtsgpu_hk_configure", "mtsgpu_set_snow_bsdfs", "mtsgpu_group_set_snow_bsdfs",
                "mtsgpu_bsdf_eval_snow"]
# the woven-cloth BRDF's entry points (irawan): the extension declared in include/mtsgpu_cloth.h
CLOTH_EXPORTS = ["mtsgpu_set_cloth_bsdfs", "mtsgpu_group_set_cloth_bsdfs", "mtsgpu_flatten_tangents_flagged", "mtsgpu_bsdf_eval_cloth",
                 "mtsgpu_cloth_check", "mtsgpu_devmath"]


# the cylinder shape's entry points: the extension declared in include/mtsgpu_cylinder.h
# the projection textures of the spot luminaire: the extension declared in include/mtsgpu_spot.h
SPOT_EXPORTS = ["mtsgpu_set_spot_textures", "mtsgpu_group_set_spot_textures", "mtsgpu_spot_textures_check", "mtsgpu_spot_eval"]
CYLINDER_EXPORTS = ["mtsgpu_cylinder_configure", "mtsgpu_flatten_cylinders", "mtsgpu_flat_scene_cylinders", "mtsgpu_upload_scene_cylinders",
                    "mtsgpu_group_upload_scene_cylinders", "mtsgpu_cylinder_aabb", "mtsgpu_cylinder_clip"]


class MtsGpuError(RuntimeError):
    pass


def load_serialized(path, shape_index=0, bsdf=-1, lum=-1, name=None):
    """<shape type="serialized"> (TriMesh::TriMesh(Stream *, int), src/librender/trimesh.cpp:156-236) -> MeshDesc"""
    h = C.c_void_p(); m = abi.Mesh()
    rc = lib().mtsgpu_load_serialized(os.fsencode(path), int(shape_index), C.byref(h), C.byref(m))
    if rc != 0:
        raise MtsGpuError("mtsgpu_load_serialized: %s" % lib().mtsgpu_last_error(None).decode())
    try:
        pos = abi.np_from(m.positions, (m.n_verts, 3), np.float32)
        tri = abi.np_from(m.triangles, (m.n_tris, 3), np.uint32)
        nrm = abi.np_from(m.normals, (m.n_verts, 3), np.float32) if m.normals else None
        cp = lib().mtsgpu_loaded_mesh_colors(h)             # the EHasColors block, or NULL
        col = abi.np_from(cp, (m.n_verts, 3), np.float32) if cp else None
        tp = lib().mtsgpu_loaded_mesh_texcoords(h)          # the EHasTexcoords block, or NULL
        uv = abi.np_from(tp, (m.n_verts, 2), np.float32) if tp else None
        return scenes.MeshDesc(pos, tri, bsdf=bsdf, lum=lum, face_normals=bool(m.face_normals), normals=nrm,
                               name=name or "%s#%d" % (os.path.basename(path), shape_index), colors=col, texcoords=uv)
    finally:
        lib().mtsgpu_loaded_mesh_free(h)


def sources():
    """csrc/sources.txt: the hashed inputs of the library in hash order, relative to csrc/ -- the one list that csrc/Makefile,
    tools/build_variant.sh and tools/kernel_resources.sh read as well"""
    return open(os.path.join(_HERE, "csrc", "sources.txt")).read().split()


def source_hash():
    """the hash csrc/Makefile stamps into the library (csrc/stamp.cpp), recomputed from the sources on disk"""
    import hashlib
    h = hashlib.sha256()
    for f in sources():
        h.update(open(os.path.join(_HERE, "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def built_hash(path=None):
    """mtsgpu_source_hash() of a built library, None if it cannot be loaded or predates the stamp"""
    try:
        L = C.CDLL(path or os.path.join(_HERE, "libmtsgpu.so"))
        L.mtsgpu_source_hash.restype = C.c_char_p
        return L.mtsgpu_source_hash().decode()
    except (OSError, AttributeError):
        return None


def _probe_hash(lib_path):
    """mtsgpu_source_hash() of the file at lib_path, asked in a child process (a library already loaded here would answer
    for the OLD file).  Returns (hash, None) or (None, why the library could not be loaded or asked)."""
    probe = "import ctypes as C; L = C.CDLL(%r); L.mtsgpu_source_hash.restype = C.c_char_p; print(L.mtsgpu_source_hash().decode())" % lib_path
    r = subprocess.run([os.sys.executable, "-c", probe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        return None, r.stderr.decode(errors="replace").strip().splitlines()[-1:] or ["exit code %d" % r.returncode]
    return r.stdout.decode().strip(), None


def _make_jobs():
    """the -j of build(): MAX_JOBS when it is set (16 at the most), otherwise 4"""
    try:
        return "-j%d" % max(1, min(16, int(os.environ["MAX_JOBS"])))
    except (KeyError, ValueError):
        return "-j4"


def build(force=False):
    """Compile libmtsgpu.so for gfx950 (hipcc cross-compiles without a GPU).  make is incremental; a binary whose stamped
    source hash differs from the sources on disk (e.g. a copied-in .so newer than the files) is rebuilt from scratch.  A
    library that cannot be LOADED is reported as such (with the loader's message), not mistaken for a stale one."""
    csrc = os.path.join(_HERE, "csrc")
    lib_path = os.path.join(_HERE, "libmtsgpu.so")          # what csrc/Makefile builds; MTSGPU_LIB variants are built by tools/build_variant.sh
    subprocess.check_call(["make", "-C", csrc, _make_jobs()] + (["-B"] if force else []), stdout=subprocess.DEVNULL)
    got, why = _probe_hash(lib_path)
    if why is not None:
        raise MtsGpuError("libmtsgpu.so was built but cannot be loaded: %s" % "; ".join(why))
    if got != source_hash():
        subprocess.check_call(["make", "-C", csrc, _make_jobs(), "-B"], stdout=subprocess.DEVNULL)
        got, why = _probe_hash(lib_path)
        if why is not None:
            raise MtsGpuError("libmtsgpu.so cannot be loaded after a full rebuild: %s" % "; ".join(why))
        if got != source_hash():
            raise MtsGpuError("libmtsgpu.so reports source hash %r after a full rebuild, the sources hash to %r" % (got, source_hash()))
    return lib_path


_lib = None


def lib():
    """Load libmtsgpu.so; fails loudly when it is missing (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MtsGpuError("libmtsgpu.so not built: run __graft_entry__.build() or `make -C mitsuba-renderer_amd/csrc`")
    L = C.CDLL(LIB_PATH)
    vp, f32p, u32p = C.c_void_p, abi.f32p, abi.u32p
    L.mtsgpu_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.mtsgpu_destroy.argtypes = [vp]; L.mtsgpu_destroy.restype = None
    L.mtsgpu_last_error.argtypes = [vp]; L.mtsgpu_last_error.restype = C.c_char_p
    L.mtsgpu_abi_version.argtypes = []
    L.mtsgpu_source_hash.argtypes = []; L.mtsgpu_source_hash.restype = C.c_char_p
    L.mtsgpu_abi_sizeof.argtypes = [C.c_int]; L.mtsgpu_abi_sizeof.restype = C.c_size_t
    L.mtsgpu_set_stream.argtypes = [vp, vp]
    L.mtsgpu_upload_scene.argtypes = [vp, C.POINTER(abi.Scene)]
    L.mtsgpu_set_camera.argtypes = [vp, C.POINTER(abi.Camera)]
    L.mtsgpu_set_integrator.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.mtsgpu_set_sampler.argtypes = [vp, C.c_int, C.c_uint32, C.c_int, C.c_uint64]
    L.mtsgpu_set_direct_integrator.argtypes = [vp, C.c_int, C.c_int]
    L.mtsgpu_set_tiles.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.mtsgpu_set_film_buffer.argtypes = [vp, vp]
    L.mtsgpu_set_rfilter.argtypes = [vp, C.c_float, C.c_float, f32p]
    L.mtsgpu_set_film_edges.argtypes = [vp, C.c_int]
    L.mtsgpu_tabulate_filter.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float, f32p, f32p]
    L.mtsgpu_set_options.argtypes = [vp, C.c_uint64, C.c_int, C.c_int]
    L.mtsgpu_render.argtypes = [vp, C.POINTER(C.c_int)]
    L.mtsgpu_sync.argtypes = [vp]
    L.mtsgpu_read_film.argtypes = [vp, f32p]
    L.mtsgpu_clear_film.argtypes = [vp]
    L.mtsgpu_get_stats.argtypes = [vp, C.POINTER(abi.Stats)]
    L.mtsgpu_trace_rays.argtypes = [vp, f32p, C.c_uint32, C.c_int, u32p]
    L.mtsgpu_ld_tables.argtypes = [vp, C.c_uint32, f32p, f32p]
    L.mtsgpu_li_samples.argtypes = [vp, u32p, C.c_uint32, f32p]
    L.mtsgpu_pass_samples.argtypes = [vp, C.c_uint32, C.c_uint32, f32p]
    L.mtsgpu_camera_rays.argtypes = [vp, abi.i32p, C.c_uint32, C.c_uint32, f32p]
    L.mtsgpu_bin_entries.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.mtsgpu_hook_rays_redone.argtypes = [vp, C.POINTER(C.c_uint64)]      # a hook outside the ABI (csrc/ctx.h), not in EXPORTS
    L.mtsgpu_flatten.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.KdParams), C.POINTER(vp)]
    L.mtsgpu_flat_scene_get.argtypes = [vp]; L.mtsgpu_flat_scene_get.restype = C.POINTER(abi.Scene)
    L.mtsgpu_flat_scene_free.argtypes = [vp]; L.mtsgpu_flat_scene_free.restype = None
    L.mtsgpu_flat_scene_kdstats.argtypes = [vp, C.POINTER(C.c_double)]
    L.mtsgpu_make_camera.argtypes = [f32p, f32p, f32p, C.c_float, C.c_int, C.c_int, C.POINTER(abi.Camera)]
    L.mtsgpu_make_camera_ortho.argtypes = [f32p, f32p, f32p, C.c_float, C.c_float, C.c_int, C.c_int, C.POINTER(abi.Camera)]
    L.mtsgpu_load_serialized.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp), C.POINTER(abi.Mesh)]
    L.mtsgpu_loaded_mesh_free.argtypes = [vp]; L.mtsgpu_loaded_mesh_free.restype = None
    L.mtsgpu_make_camera_crop.argtypes = [f32p, f32p, f32p, C.c_float] + [C.c_int] * 6 + [C.POINTER(abi.Camera)]
    L.mtsgpu_gather_roof.argtypes = [C.c_int, C.c_size_t, C.POINTER(C.c_double)]
    L.mtsgpu_set_tuning.argtypes = [vp, C.c_char_p, C.c_long]
    L.mtsgpu_sampler_values.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, f32p]
    L.mtsgpu_random_values.argtypes = [vp, C.c_int, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    L.mtsgpu_bsdf_eval.argtypes = [vp, C.c_uint32, f32p, C.c_int, C.c_uint32, f32p, f32p]
    L.mtsgpu_bsdf_eval_table.argtypes = [vp, C.c_uint32, u32p, f32p, C.c_uint32, C.c_int, C.c_uint32, f32p, f32p]
    L.mtsgpu_sky_configure.argtypes = [f32p, f32p]
    L.mtsgpu_lum_eval.argtypes = [vp, C.c_uint32, f32p, C.c_int, C.c_uint32, f32p, f32p]
    L.mtsgpu_scene_lum_eval.argtypes = [vp, C.c_int, C.c_uint32, f32p, f32p]
    L.mtsgpu_hbm_triad.argtypes = [C.c_int, C.c_size_t, C.c_int, C.POINTER(C.c_double)]
    L.mtsgpu_replay_roof.argtypes = [vp, C.c_int, C.c_uint32, C.c_uint32, C.c_int, C.POINTER(C.c_double)]
    L.mtsgpu_create_multi.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(vp)]
    L.mtsgpu_group_destroy.argtypes = [vp]; L.mtsgpu_group_destroy.restype = None
    L.mtsgpu_group_size.argtypes = [vp]
    L.mtsgpu_group_ctx.argtypes = [vp, C.c_int]; L.mtsgpu_group_ctx.restype = vp
    L.mtsgpu_group_last_error.argtypes = [vp]; L.mtsgpu_group_last_error.restype = C.c_char_p
    L.mtsgpu_group_upload_scene.argtypes = [vp, C.POINTER(abi.Scene)]
    L.mtsgpu_group_set_camera.argtypes = [vp, C.POINTER(abi.Camera)]
    L.mtsgpu_group_set_integrator.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.mtsgpu_group_set_sampler.argtypes = [vp, C.c_int, C.c_uint32, C.c_int, C.c_uint64]
    L.mtsgpu_group_set_rfilter.argtypes = [vp, C.c_float, C.c_float, f32p]
    L.mtsgpu_group_render.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.mtsgpu_group_last_reduce_kind.argtypes = [vp]
    L.mtsgpu_group_rccl_ranks.argtypes = [vp]
    L.mtsgpu_group_reduce_note.argtypes = [vp]; L.mtsgpu_group_reduce_note.restype = C.c_char_p
    L.mtsgpu_group_set_tuning.argtypes = [vp, C.c_char_p, C.c_long]
    L.mtsgpu_set_film_statistics.argtypes = [vp, C.c_int]
    L.mtsgpu_read_film_statistics.argtypes = [vp, f32p, u32p]
    L.mtsgpu_film_statistics_form.argtypes = [vp]
    L.mtsgpu_group_set_film_statistics.argtypes = [vp, C.c_int]
    L.mtsgpu_set_vertex_colors.argtypes = [vp, f32p, u32p, u32p]
    L.mtsgpu_group_set_vertex_colors.argtypes = [vp, f32p, u32p, u32p]
    L.mtsgpu_flat_scene_set_mesh_colors.argtypes = [vp, C.c_uint32, f32p]
    L.mtsgpu_flat_scene_vertex_colors.argtypes = [vp]; L.mtsgpu_flat_scene_vertex_colors.restype = f32p
    L.mtsgpu_flat_scene_shape_has_colors.argtypes = [vp]; L.mtsgpu_flat_scene_shape_has_colors.restype = u32p
    L.mtsgpu_loaded_mesh_colors.argtypes = [vp]; L.mtsgpu_loaded_mesh_colors.restype = f32p
    L.mtsgpu_vertex_color_eval.argtypes = [vp, C.c_uint32, u32p, f32p, f32p]
    L.mtsgpu_bsdf_eval_colored.argtypes = [vp, C.c_uint32, f32p, C.c_uint32, f32p, C.c_int, C.c_uint32, f32p, f32p]
    texp = C.POINTER(abi.UvTexture)
    L.mtsgpu_set_uv_textures.argtypes = [vp, f32p, u32p, C.c_uint32, texp, abi.i32p]
    L.mtsgpu_group_set_uv_textures.argtypes = [vp, f32p, u32p, C.c_uint32, texp, abi.i32p]
    L.mtsgpu_flat_scene_set_mesh_texcoords.argtypes = [vp, C.c_uint32, f32p]
    L.mtsgpu_flat_scene_vertex_texcoords.argtypes = [vp]; L.mtsgpu_flat_scene_vertex_texcoords.restype = f32p
    L.mtsgpu_flat_scene_shape_has_texcoords.argtypes = [vp]; L.mtsgpu_flat_scene_shape_has_texcoords.restype = u32p
    L.mtsgpu_loaded_mesh_texcoords.argtypes = [vp]; L.mtsgpu_loaded_mesh_texcoords.restype = f32p
    L.mtsgpu_uv_texture_eval.argtypes = [vp, texp, C.c_uint32, u32p, f32p, f32p]
    L.mtsgpu_bsdf_eval_slots.argtypes = [vp, C.c_uint32, f32p, abi.i32p, f32p, f32p, C.c_int, C.c_uint32, f32p, f32p]
    L.mtsgpu_flatten_tangents.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.KdParams), C.POINTER(f32p), C.POINTER(vp)]
    L.mtsgpu_flat_scene_vertex_tangents.argtypes = [vp]; L.mtsgpu_flat_scene_vertex_tangents.restype = f32p
    L.mtsgpu_flat_scene_shape_has_tangents.argtypes = [vp]; L.mtsgpu_flat_scene_shape_has_tangents.restype = u32p
    L.mtsgpu_upload_scene_tangents.argtypes = [vp, C.POINTER(abi.Scene), f32p, u32p]
    L.mtsgpu_group_upload_scene_tangents.argtypes = [vp, C.POINTER(abi.Scene), f32p, u32p]
    L.mtsgpu_shading_frame_eval.argtypes = [vp, C.c_uint32, u32p, f32p, f32p]
    cylp = C.POINTER(abi.Cylinder)
    L.mtsgpu_cylinder_configure.argtypes = [cylp, f32p]
    L.mtsgpu_flatten_cylinders.argtypes = [C.POINTER(abi.SceneDesc), C.POINTER(abi.KdParams), C.POINTER(f32p), u32p, cylp, C.POINTER(vp)]
    L.mtsgpu_flat_scene_cylinders.argtypes = [vp]; L.mtsgpu_flat_scene_cylinders.restype = f32p
    L.mtsgpu_upload_scene_cylinders.argtypes = [vp, C.POINTER(abi.Scene), f32p, u32p, f32p]
    L.mtsgpu_group_upload_scene_cylinders.argtypes = [vp, C.POINTER(abi.Scene), f32p, u32p, f32p]
    L.mtsgpu_cylinder_aabb.argtypes = [f32p, f32p]
    L.mtsgpu_cylinder_clip.argtypes = [f32p, C.c_uint32, f32p, C.c_int, f32p, u32p]
    bmpp = C.POINTER(abi.Bitmap)
    L.mtsgpu_set_uv_bitmap_textures.argtypes = [vp, f32p, u32p, C.c_uint32, texp, abi.i32p, C.c_uint32, bmpp, abi.i32p]
    L.mtsgpu_group_set_uv_bitmap_textures.argtypes = [vp, f32p, u32p, C.c_uint32, texp, abi.i32p, C.c_uint32, bmpp, abi.i32p]
    L.mtsgpu_bitmap_texture_eval.argtypes = [vp, texp, bmpp, C.c_uint32, u32p, f32p, f32p]
    mskp = C.POINTER(abi.BsdfMask)
    L.mtsgpu_set_uv_masked_textures.argtypes = [vp, f32p, u32p, C.c_uint32, texp, abi.i32p, C.c_uint32, bmpp, abi.i32p, mskp]
    L.mtsgpu_group_set_uv_masked_textures.argtypes = [vp, f32p, u32p, C.c_uint32, texp, abi.i32p, C.c_uint32, bmpp, abi.i32p, mskp]
    L.mtsgpu_bsdf_eval_masked.argtypes = [vp, C.c_uint32, f32p, f32p, C.c_int, C.c_uint32, f32p, f32p]
    snwp = C.POINTER(abi.BsdfSnow)
    L.mtsgpu_wiscombe_configure.argtypes = [f32p, snwp]
    L.mtsgpu_hk_configure.argtypes = [f32p, snwp]
    L.mtsgpu_set_snow_bsdfs.argtypes = [vp, snwp]
    L.mtsgpu_group_set_snow_bsdfs.argtypes = [vp, snwp]
    L.mtsgpu_bsdf_eval_snow.argtypes = [vp, C.c_uint32, snwp, C.c_int, C.c_uint32, f32p, f32p]
    wvp = C.POINTER(abi.Weave)
    L.mtsgpu_set_cloth_bsdfs.argtypes = [vp, C.c_uint32, wvp, abi.i32p]
    L.mtsgpu_group_set_cloth_bsdfs.argtypes = [vp, C.c_uint32, wvp, abi.i32p]
    L.mtsgpu_bsdf_eval_cloth.argtypes = [vp, C.c_uint32, wvp, C.c_int, C.c_uint32, f32p, f32p]
    L.mtsgpu_cloth_check.argtypes = [wvp, f32p]
    L.mtsgpu_devmath.argtypes = [C.c_int, C.c_uint32, f32p, f32p, f32p]
    L.mtsgpu_flatten_tangents_flagged.argtypes = L.mtsgpu_flatten_tangents.argtypes[:3] + [u32p] + L.mtsgpu_flatten_tangents.argtypes[3:]
    L.mtsgpu_ldr_texels.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8), C.c_float, f32p]
    L.mtsgpu_set_spot_textures.argtypes = [vp, C.c_uint32, texp, C.c_uint32, bmpp, abi.i32p, u32p, abi.i32p]
    L.mtsgpu_group_set_spot_textures.argtypes = [vp, C.c_uint32, texp, C.c_uint32, bmpp, abi.i32p, u32p, abi.i32p]
    L.mtsgpu_spot_textures_check.argtypes = [C.c_uint32, u32p, f32p, C.c_uint32, texp, C.c_uint32, bmpp, abi.i32p, u32p, abi.i32p, C.c_uint32, f32p]
    L.mtsgpu_spot_eval.argtypes = [vp, f32p, texp, bmpp, C.c_uint32, C.c_uint32, f32p, f32p]
    _lib = L
    return L


def _f(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def bsdf_mask_array(masks):
    """rows (kind, texture, opacity rgb) or abi.BsdfMask objects -> the ctypes array mtsgpu_set_uv_masked_textures takes"""
    arr = (abi.BsdfMask * max(len(masks), 1))()
    for i, m in enumerate(masks):
        if isinstance(m, abi.BsdfMask):
            arr[i] = m
        else:
            kind, tex, op = m
            arr[i] = abi.BsdfMask(int(kind), int(tex), (C.c_float * 3)(*[float(x) for x in op]), 0)
    return arr


def snow_configure(kind, raw):
    """the reference's configure() of a snow BRDF on the host: kind abi.SNOW_WISCOMBE with raw = g, depth, w0 rgb, sigmaT rgb
    (mtsgpu_wiscombe_configure), or abi.SNOW_HK with raw = sigmaA rgb, sigmaS rgb, g, etaInt, etaExt, ssFactor rgb, drFactor rgb,
    useDiffuseReflectance (mtsgpu_hk_configure) -> abi.BsdfSnow"""
    n, call = {abi.SNOW_WISCOMBE: (8, lib().mtsgpu_wiscombe_configure), abi.SNOW_HK: (16, lib().mtsgpu_hk_configure)}[int(kind)]
    r = np.ascontiguousarray(raw, dtype=np.float32)
    if r.shape != (n,):
        raise ValueError("snow_configure: %d raw values, not %d" % (r.size, n))
    out = abi.BsdfSnow()
    if call(abi.ptr(r, abi.f32p), C.byref(out)) != 0:
        raise MtsGpuError("snow_configure: %s" % lib().mtsgpu_last_error(None).decode())
    return out


def bsdf_snow_array(rows):
    """abi.BsdfSnow objects, rows (kind, derived) or None (no snow record) -> the ctypes array mtsgpu_set_snow_bsdfs takes"""
    arr = (abi.BsdfSnow * max(len(rows), 1))()
    for i, m in enumerate(rows):
        if isinstance(m, abi.BsdfSnow):
            arr[i] = m
        elif m is not None:
            kind, derived = m
            d = np.zeros(abi.SNOW_NDERIVED, dtype=np.float32); d[:len(derived)] = derived
            arr[i] = abi.BsdfSnow(int(kind), 0, (C.c_float * abi.SNOW_NDERIVED)(*[float(x) for x in d]))
    return arr


def weave_array(weaves):
    """scenes.Weave objects -> (the ctypes array of mtsgpu_weave that mtsgpu_set_cloth_bsdfs takes, the arrays it points into)"""
    arr = (abi.Weave * max(len(weaves), 1))()
    keep = []
    for i, w in enumerate(weaves):
        for n in abi.WEAVE_SCALARS:
            setattr(arr[i], n, getattr(w, n))
        pat = (C.c_uint32 * max(len(w.pattern), 1))(*[int(p) & 0xFFFFFFFF for p in w.pattern])
        yarns = (abi.Yarn * max(len(w.yarns), 1))()
        for j, y in enumerate(w.yarns):
            yarns[j] = abi.Yarn(int(y.type), float(y.psi), float(y.umax), float(y.kappa), float(y.width), float(y.length), float(y.centerU),
                                float(y.centerV), (C.c_float * 3)(*[float(x) for x in y.kd]), (C.c_float * 3)(*[float(x) for x in y.ks]))
        arr[i].n_pattern, arr[i].n_yarns = len(w.pattern), len(w.yarns)
        arr[i].pattern, arr[i].yarns = C.cast(pat, C.POINTER(C.c_uint32)), C.cast(yarns, C.POINTER(abi.Yarn))
        keep += [pat, yarns]
    return arr, keep


def cloth_check(weave, uv_range=None):
    """mtsgpu_cloth_check: what the cloth setter requires of one scenes.Weave, and with uv_range = (uMin, uMax, vMin, vMax) the casts
    of f on such texcoords; raises MtsGpuError with the reason"""
    arr, keep = weave_array([weave])
    r = None if uv_range is None else np.ascontiguousarray(uv_range, dtype=np.float32)
    if lib().mtsgpu_cloth_check(arr, abi.ptr(r, abi.f32p)) != 0:
        raise MtsGpuError("cloth_check: %s" % lib().mtsgpu_last_error(None).decode())


DEVMATH = dict(sin=0, cos=1, tan=2, exp=3, log=4, atan=5, acos=6, atan2=7, sinh=8, cosh=9, pow15=10)


def devmath(fn, x, y=None):
    """mtsgpu_devmath: the library's elementary function `fn` (a key of DEVMATH) of float32 arguments, on the host"""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    y = None if y is None else np.ascontiguousarray(y, dtype=np.float32).ravel()
    out = np.zeros_like(x)
    if lib().mtsgpu_devmath(DEVMATH[fn], len(x), abi.ptr(x, abi.f32p), abi.ptr(y, abi.f32p), abi.ptr(out, abi.f32p)) != 0:
        raise MtsGpuError("devmath: %s" % lib().mtsgpu_last_error(None).decode())
    return out


def uv_texture_array(textures):
    """a ctypes array of mtsgpu_uv_texture from scenes.Checkerboard / GridTexture objects (or abi.UvTexture values)"""
    items = [t if isinstance(t, abi.UvTexture) else t.descriptor() for t in textures]
    return (abi.UvTexture * max(len(items), 1))(*items) if items else (abi.UvTexture * 1)()


def bitmap_array(bitmaps):
    """a ctypes array of mtsgpu_bitmap from scenes.BitmapTexture objects (or abi.Bitmap values)"""
    items = [b if isinstance(b, abi.Bitmap) else b.bitmap() for b in bitmaps]
    return (abi.Bitmap * max(len(items), 1))(*items) if items else (abi.Bitmap * 1)()


def spot_textures_check(lum_type, lum_params, textures, texture_bilinear, lum_texture, in_force=0, bitmaps=None, texture_bitmap=None):
    """mtsgpu_spot_textures_check: what mtsgpu_set_spot_textures requires, without a context.  textures: scenes texture objects (or
    abi.UvTexture values with `bitmaps` / `texture_bitmap` given); in_force: bit 0 a mask, 1 a snow table, 2 a cloth table.
    Returns uv_factor [n_lums]; raises MtsGpuError with the refusal"""
    lt = np.ascontiguousarray(lum_type, dtype=np.uint32).reshape(-1)
    lp = np.ascontiguousarray(lum_params, dtype=np.float32).reshape(-1, abi.LUM_NPARAMS)
    textures = list(textures) if textures is not None else None
    if textures is not None and bitmaps is None:
        bitmaps, texture_bitmap = bitmap_table(textures)
    tb = None if texture_bitmap is None else np.ascontiguousarray(texture_bitmap, dtype=np.int32)
    fl = None if texture_bilinear is None else np.ascontiguousarray(texture_bilinear, dtype=np.uint32)
    lx = None if lum_texture is None else np.ascontiguousarray(lum_texture, dtype=np.int32)
    out = np.zeros(max(len(lt), 1), dtype=np.float32)
    rc = lib().mtsgpu_spot_textures_check(len(lt), abi.ptr(lt, abi.u32p), abi.ptr(lp, abi.f32p), len(textures or []),
                                          uv_texture_array(textures) if textures else None, len(bitmaps or []),
                                          bitmap_array(bitmaps) if bitmaps else None, abi.ptr(tb, abi.i32p), abi.ptr(fl, abi.u32p),
                                          abi.ptr(lx, abi.i32p), int(in_force), abi.ptr(out, abi.f32p))
    if rc != 0:
        raise MtsGpuError("spot_textures_check: %s" % lib().mtsgpu_last_error(None).decode())
    return out[:len(lt)]


def bitmap_table(textures):
    """(bitmaps, texture_bitmap) for a list of texture objects: one entry of `bitmaps` per distinct (texels array, wrap mode)
    among the scenes.BitmapTexture objects, and for every texture the index of its bitmap, -1 for the other kinds"""
    bitmaps, index = [], []
    for t in textures:
        if getattr(t, "kind", None) != abi.TEX_BITMAP or isinstance(t, abi.UvTexture):
            index.append(-1)
            continue
        hit = [i for i, b in enumerate(bitmaps) if b.texels is t.texels and b.wrap == t.wrap]
        if not hit:
            bitmaps.append(t)
        index.append(hit[0] if hit else len(bitmaps) - 1)
    return bitmaps, np.asarray(index, dtype=np.int32)


def ldr_texels(pixels, gamma=-1.0, bpp=None, width=None, height=None):
    """mtsgpu_ldr_texels: the bytes of a decoded LDR file -> [height][width][3] linear RGB float32, as LDRTexture::initializeFrom
    and MIPMap::fromBitmap leave them.  pixels: uint8 [height][width] (8 bpp) or [height][width][2 | 3 | 4] (16, 24, 32); or
    flat bytes with bpp, width and height given (the only way to 1 bpp)"""
    a = np.ascontiguousarray(pixels, dtype=np.uint8)
    if bpp is None:
        if a.ndim not in (2, 3):
            raise ValueError("ldr_texels: pixels are [height][width] or [height][width][channels]")
        height, width = a.shape[:2]
        bpp = 8 * (a.shape[2] if a.ndim == 3 else 1)
    width, height, bpp = int(width), int(height), int(bpp)
    if bpp in (1, 8, 16, 24, 32) and a.size < (width * height * bpp + 7) // 8:
        raise ValueError("ldr_texels: %d bytes for %d x %d pixels of %d bits" % (a.size, width, height, bpp))
    out = np.zeros((height, width, 3), dtype=np.float32)
    rc = lib().mtsgpu_ldr_texels(bpp, width, height, a.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_float(gamma), abi.ptr(out, abi.f32p))
    if rc != 0:
        raise MtsGpuError("mtsgpu_ldr_texels: %s" % lib().mtsgpu_last_error(None).decode())
    return out


def cylinder_configure(cyl):
    """mtsgpu_cylinder_configure of a scenes.CylinderDesc or an abi.Cylinder -> the derived block [28]"""
    c = cyl.to_struct() if hasattr(cyl, "to_struct") else cyl
    out = np.zeros(abi.CYLINDER_NDERIVED, dtype=np.float32)
    if lib().mtsgpu_cylinder_configure(C.byref(c), abi.ptr(out, abi.f32p)) != 0:
        raise MtsGpuError(lib().mtsgpu_last_error(None).decode())
    return out


def cylinder_aabb(derived):
    """mtsgpu_cylinder_aabb -> [6] = min, max"""
    d = np.ascontiguousarray(derived, dtype=np.float32).reshape(abi.CYLINDER_NDERIVED)
    out = np.zeros(6, dtype=np.float32)
    if lib().mtsgpu_cylinder_aabb(abi.ptr(d, abi.f32p), abi.ptr(out, abi.f32p)) != 0:
        raise MtsGpuError(lib().mtsgpu_last_error(None).decode())
    return out


def cylinder_clip(derived, boxes, on_device=False):
    """mtsgpu_cylinder_clip: boxes [n][6] -> (clipped [n][6], valid [n])"""
    d = np.ascontiguousarray(derived, dtype=np.float32).reshape(abi.CYLINDER_NDERIVED)
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
    out = np.zeros_like(b); valid = np.zeros(b.shape[0], dtype=np.uint32)
    if lib().mtsgpu_cylinder_clip(abi.ptr(d, abi.f32p), b.shape[0], abi.ptr(b, abi.f32p), int(on_device), abi.ptr(out, abi.f32p), abi.ptr(valid, abi.u32p)) != 0:
        raise MtsGpuError(lib().mtsgpu_last_error(None).decode())
    return out, valid.astype(bool)


class Scene:
    """A flattened, render-ready scene: what Scene::initialize() leaves behind
    (kd-tree, TriAccel table, vertex normals, luminaire CDFs), built by mtsgpu_flatten()."""

    def __init__(self, description, kd_params=None, gpu_binning=False, gpu_exact=False):
        """gpu_binning: run the min-max binning phase of the kd-tree build (nodes of more than
        exactPrimThreshold primitives, gkdtree.h:1735-1867) on the current HIP device -- same tree, bit for bit.
        gpu_exact: the exact O(n log n) sweep below that threshold (gkdtree.h:1898-2345) on the device as well."""
        self.description = description
        self._desc, self._keep = description.to_ctypes()
        self._h = C.c_void_p()
        kp = kd_params if kd_params is not None else abi.KdParams()
        kp.gpu_binning = (kp.gpu_binning & ~3) | (1 if gpu_binning else 0) | (2 if gpu_exact else 0)
        # the _tangents calls only when a mesh with texcoords has an anisotropic BSDF (TriMesh::configure asks for tangents
        # then, trimesh.cpp:288-290); every other scene goes through the calls it always went through
        self.wants_tangents = any(m.shape_type == abi.SHAPE_TRIMESH and getattr(m, "texcoords", None) is not None and m.bsdf >= 0
                                  and (description.bsdf_is_anisotropic(m.bsdf) or m.bsdf in getattr(description, "bsdf_weave", {}))
                                  for m in description.meshes)
        # the cloth BSDFs of the scene (none: the scene never calls mtsgpu_set_cloth_bsdfs): IrawanClothBRDF is EAnisotropic and its
        # Lambertian entry is not, so its entries are flagged for the flattener
        self.cloth = None
        if getattr(description, "bsdf_weave", None):
            self.cloth = weave_array(description.weaves) + (description.weave_table(),)
        # a description with a cylinder goes through the cylinder calls (include/mtsgpu_cylinder.h), every other one through
        # the calls it always went through
        self.has_cylinders = any(m.shape_type == abi.SHAPE_CYLINDER for m in description.meshes)
        if self.has_cylinders:
            tcs = (abi.f32p * max(len(description.meshes), 1))()
            cyl = (abi.Cylinder * max(len(description.meshes), 1))()
            for i, m in enumerate(description.meshes):
                if m.shape_type == abi.SHAPE_TRIMESH and getattr(m, "texcoords", None) is not None:
                    tcs[i] = abi.ptr(m.texcoords, abi.f32p)
                if m.shape_type == abi.SHAPE_CYLINDER:
                    cyl[i] = m.to_struct()
            flags = None if self.cloth is None else np.ascontiguousarray(self.cloth[2] >= 0, dtype=np.uint32)
            rc = lib().mtsgpu_flatten_cylinders(C.byref(self._desc), C.byref(kp), tcs, abi.ptr(flags, abi.u32p), cyl, C.byref(self._h))
        elif self.wants_tangents:
            tcs = (abi.f32p * max(len(description.meshes), 1))()
            for i, m in enumerate(description.meshes):
                if m.shape_type == abi.SHAPE_TRIMESH and getattr(m, "texcoords", None) is not None:
                    tcs[i] = abi.ptr(m.texcoords, abi.f32p)
            if self.cloth is not None:
                flags = np.ascontiguousarray(self.cloth[2] >= 0, dtype=np.uint32)
                rc = lib().mtsgpu_flatten_tangents_flagged(C.byref(self._desc), C.byref(kp), tcs, abi.ptr(flags, abi.u32p), C.byref(self._h))
            else:
                rc = lib().mtsgpu_flatten_tangents(C.byref(self._desc), C.byref(kp), tcs, C.byref(self._h))
        else:
            rc = lib().mtsgpu_flatten(C.byref(self._desc), C.byref(kp), C.byref(self._h))
        if rc != 0:
            raise MtsGpuError("mtsgpu_flatten: %s" % lib().mtsgpu_last_error(None).decode())
        self.ptr = lib().mtsgpu_flat_scene_get(self._h)
        # per-vertex colours go into the flat scene's own pool; the slot masks of the BSDFs travel next to the blocks
        for i, m in enumerate(description.meshes):
            if getattr(m, "colors", None) is not None:
                rc = lib().mtsgpu_flat_scene_set_mesh_colors(self._h, i, abi.ptr(m.colors, abi.f32p))
                if rc != 0:
                    raise MtsGpuError("mtsgpu_flat_scene_set_mesh_colors: %s" % lib().mtsgpu_last_error(None).decode())
        slots = np.asarray(getattr(description, "bsdf_color_slots", []), dtype=np.uint32)
        self.bsdf_color_slots = slots if slots.any() else None
        # likewise the texture coordinates, the uv textures and the table that names one per BSDF slot
        for i, m in enumerate(description.meshes):
            if getattr(m, "texcoords", None) is not None:
                rc = lib().mtsgpu_flat_scene_set_mesh_texcoords(self._h, i, abi.ptr(m.texcoords, abi.f32p))
                if rc != 0:
                    raise MtsGpuError("mtsgpu_flat_scene_set_mesh_texcoords: %s" % lib().mtsgpu_last_error(None).decode())
        self.textures = uv_texture_array(getattr(description, "textures", []))
        # the bitmaps behind the BitmapTexture objects among them (none: the scene takes mtsgpu_set_uv_textures as ever)
        self._bitmap_objects, self.texture_bitmap = bitmap_table(getattr(description, "textures", []))
        self.bitmaps = bitmap_array(self._bitmap_objects)
        table = np.asarray(getattr(description, "bsdf_slot_texture", []), dtype=np.int32).reshape(-1, 2)
        self.bsdf_slot_texture = np.ascontiguousarray(table) if (table >= 0).any() else None
        # the masks around the BSDFs (none: the scene takes the texture calls as ever)
        self.bsdf_mask = bsdf_mask_array(description.mask_table()) if getattr(description, "bsdf_masks", None) else None
        # the snow records of the BSDFs (none: the scene never calls mtsgpu_set_snow_bsdfs)
        self.bsdf_snow = bsdf_snow_array(description.snow_table(snow_configure)) if getattr(description, "bsdf_snow", None) else None

        # the projection textures of the spot luminaires (none: the scene never calls mtsgpu_set_spot_textures)
        self.spot = None
        if getattr(description, "spot_textures", None):
            st, flags, lum = description.spot_texture_table()
            sb, stb = bitmap_table(st)
            self.spot = (st, uv_texture_array(st), sb, bitmap_array(sb), stb, flags, lum)

    @property
    def sc(self):
        return self.ptr.contents

    def spot_texture_args(self):
        """what mtsgpu_set_spot_textures takes for this scene: (n_textures, textures, n_bitmaps, bitmaps, texture_bitmap,
        texture_bilinear, lum_texture), or None when no spot luminaire of the scene has a projection texture"""
        if self.spot is None:
            return None
        st, ta, sb, ba, stb, flags, lum = self.spot
        return (len(st), ta, len(sb), ba if sb else None, abi.ptr(stb, abi.i32p) if sb else None, abi.ptr(flags, abi.u32p), abi.ptr(lum, abi.i32p))

    def cylinder_blocks(self):
        """the derived blocks mtsgpu_upload_scene_cylinders takes behind the scene, [n_shapes][28], or None without a cylinder"""
        p = lib().mtsgpu_flat_scene_cylinders(self._h)
        return abi.np_from(p, (self.sc.n_shapes, abi.CYLINDER_NDERIVED), np.float32) if p else None

    def vertex_color_args(self):
        """what mtsgpu_set_vertex_colors takes for this scene: (vtx_col, shape_has_colors, bsdf_color_slots) pointers, or
        None when the scene has neither coloured meshes nor coloured BSDF slots"""
        col = lib().mtsgpu_flat_scene_vertex_colors(self._h)
        has = lib().mtsgpu_flat_scene_shape_has_colors(self._h)
        if not col and self.bsdf_color_slots is None:
            return None
        return (col if col else None, has if has else None, abi.ptr(self.bsdf_color_slots, abi.u32p))

    def uv_texture_args(self):
        """what mtsgpu_set_uv_textures takes for this scene: (vtx_uv, shape_has_uv, n_textures, textures, bsdf_slot_texture),
        or None when no BSDF slot of the scene has a uv texture"""
        if self.bsdf_slot_texture is None:
            return None
        uv = lib().mtsgpu_flat_scene_vertex_texcoords(self._h)
        has = lib().mtsgpu_flat_scene_shape_has_texcoords(self._h)
        return (uv if uv else None, has if has else None, len(self.textures), self.textures, abi.ptr(self.bsdf_slot_texture, abi.i32p))

    def uv_only_args(self):
        """what mtsgpu_set_uv_textures takes to hand over the texcoords alone (a cloth scene without a uv texture)"""
        uv = lib().mtsgpu_flat_scene_vertex_texcoords(self._h)
        has = lib().mtsgpu_flat_scene_shape_has_texcoords(self._h)
        if not uv:       # no mesh has texcoords (spheres only): a zero pool, so that the call keeps a uv array
            n = max(int(self.sc.n_verts), 1)
            self._uv_zero = (np.zeros((n, 2), dtype=np.float32), np.zeros(max(int(self.sc.n_shapes), 1), dtype=np.uint32))
            return (abi.ptr(self._uv_zero[0], abi.f32p), abi.ptr(self._uv_zero[1], abi.u32p), 0, None, None)
        return (uv, has, 0, None, None)

    def uv_bitmap_texture_args(self):
        """what mtsgpu_set_uv_bitmap_textures takes for this scene: uv_texture_args() and (n_bitmaps, bitmaps, texture_bitmap), or
        None when no texture in a slot of the scene is a bitmap -- such a scene takes mtsgpu_set_uv_textures"""
        ut = self.uv_texture_args()
        if ut is None or not self._bitmap_objects:
            return None
        return ut + (len(self._bitmap_objects), self.bitmaps, abi.ptr(self.texture_bitmap, abi.i32p))

    def uv_masked_texture_args(self):
        """what mtsgpu_set_uv_masked_textures takes for this scene: the nine arguments of mtsgpu_set_uv_bitmap_textures (slot
        table, bitmaps and bitmap indices None where the scene has none) and bsdf_mask, or None when no BSDF of the scene has a
        mask -- such a scene takes the two older calls"""
        if self.bsdf_mask is None:
            return None
        uv = lib().mtsgpu_flat_scene_vertex_texcoords(self._h)
        has = lib().mtsgpu_flat_scene_shape_has_texcoords(self._h)
        nb, nt = len(self._bitmap_objects), len(getattr(self.description, "textures", []))
        return (uv if uv else None, has if has else None, nt, self.textures if nt else None,
                abi.ptr(self.bsdf_slot_texture, abi.i32p), nb, self.bitmaps if nb else None,
                abi.ptr(self.texture_bitmap, abi.i32p) if nb else None, self.bsdf_mask)

    def vertex_tangents(self):
        """(pool [n_verts][6] float32 = dpdu, dpdv; flags [n_shapes] uint32) of the flat scene, or (None, None) when no mesh has
        tangents (mtsgpu_flat_scene_vertex_tangents)"""
        tan = lib().mtsgpu_flat_scene_vertex_tangents(self._h)
        if not tan:
            return None, None
        return (abi.np_from(tan, (self.sc.n_verts, 6), np.float32),
                abi.np_from(lib().mtsgpu_flat_scene_shape_has_tangents(self._h), (self.sc.n_shapes,), np.uint32))

    def tangent_args(self):
        """what mtsgpu_upload_scene_tangents takes behind the scene: (vtx_dpdu [n_verts][3], shape_has_tangents) arrays, or None
        when the scene was flattened without the tangents call"""
        if not self.wants_tangents:
            return None
        tan, has = self.vertex_tangents()
        if tan is None:
            return (None, None)
        return (np.ascontiguousarray(tan[:, :3]), np.ascontiguousarray(has))

    def vertex_texcoords(self):
        """(pool [n_verts][2] float32, flags [n_shapes] uint32) of the flat scene, or (None, None)"""
        uv = lib().mtsgpu_flat_scene_vertex_texcoords(self._h)
        if not uv:
            return None, None
        return (abi.np_from(uv, (self.sc.n_verts, 2), np.float32),
                abi.np_from(lib().mtsgpu_flat_scene_shape_has_texcoords(self._h), (self.sc.n_shapes,), np.uint32))

    def vertex_colors(self):
        """(pool [n_verts][3] float32, flags [n_shapes] uint32) of the flat scene, or (None, None)"""
        col = lib().mtsgpu_flat_scene_vertex_colors(self._h)
        if not col:
            return None, None
        return (abi.np_from(col, (self.sc.n_verts, 3), np.float32),
                abi.np_from(lib().mtsgpu_flat_scene_shape_has_colors(self._h), (self.sc.n_shapes,), np.uint32))

    def arrays(self):
        return abi.scene_arrays(self.sc)

    def kdstats(self):
        out = (C.c_double * 6)()
        lib().mtsgpu_flat_scene_kdstats(self._h, out)
        return dict(zip(["inner", "leaf", "indices", "exp_traversals", "exp_leaves", "exp_prims"], list(out)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and _lib is not None:
            _lib.mtsgpu_flat_scene_free(h)
            self._h = None


class PerspectiveCamera:
    """`perspective` camera plugin: lookAt toWorld transform, fov along the smaller side, pinhole."""

    def __init__(self, origin, target, up, fov, width, height, apertureRadius=0.0, focusDepth=None):
        self.c = abi.Camera()
        rc = lib().mtsgpu_make_camera(abi.ptr(_f(origin), abi.f32p), abi.ptr(_f(target), abi.f32p), abi.ptr(_f(up), abi.f32p),
                                      C.c_float(fov), int(width), int(height), C.byref(self.c))
        if rc != 0:
            raise MtsGpuError("mtsgpu_make_camera: %s" % lib().mtsgpu_last_error(None).decode())
        if apertureRadius > 0:                       # thin lens (camera.cpp:164-166, perspective.cpp:90-103)
            self.c.aperture_radius = apertureRadius
            self.c.focus_depth = self.c.far_clip if focusDepth is None else focusDepth

    @classmethod
    def cropped(cls, desc, film_width, film_height, crop):
        """the camera of `desc` behind a film with a crop window (film.cpp:33-41): crop = (offsetX, offsetY, width, height)"""
        c = desc.camera
        self = cls.__new__(cls)
        self.c = abi.Camera()
        rc = lib().mtsgpu_make_camera_crop(abi.ptr(_f(c["origin"]), abi.f32p), abi.ptr(_f(c["target"]), abi.f32p), abi.ptr(_f(c["up"]), abi.f32p),
                                           C.c_float(c["fov"]), int(film_width), int(film_height), *[int(v) for v in crop], C.byref(self.c))
        if rc != 0:
            raise MtsGpuError("mtsgpu_make_camera_crop: %s" % lib().mtsgpu_last_error(None).decode())
        return self

    @classmethod
    def for_description(cls, desc, width, height):
        c = desc.camera
        if "ortho_scale" in c:
            return OrthographicCamera(c["origin"], c["target"], c["up"], c["ortho_scale"], width, height)
        return cls(c["origin"], c["target"], c["up"], c["fov"], width, height,
                   apertureRadius=c.get("aperture", 0.0), focusDepth=c.get("focus"))

    @property
    def width(self):
        return self.c.width

    @property
    def height(self):
        return self.c.height


class OrthographicCamera(PerspectiveCamera):
    """`orthographic` camera plugin (src/cameras/orthographic.cpp): toWorld = lookAt * scale(sx, sy, 1)"""

    def __init__(self, origin, target, up, scale, width, height):
        self.c = abi.Camera()
        sx, sy = (scale, scale) if np.isscalar(scale) else scale
        rc = lib().mtsgpu_make_camera_ortho(abi.ptr(_f(origin), abi.f32p), abi.ptr(_f(target), abi.f32p), abi.ptr(_f(up), abi.f32p),
                                            C.c_float(sx), C.c_float(sy), int(width), int(height), C.byref(self.c))
        if rc != 0:
            raise MtsGpuError("mtsgpu_make_camera_ortho: %s" % lib().mtsgpu_last_error(None).decode())


class MIPathTracer:
    """The `path` integrator (MIPathTracer : MonteCarloIntegrator) on one MI355X.

    Properties as in src/librender/integrator.cpp:272-292: maxDepth (-1 = unbounded),
    rrDepth (10), strictNormals (false).  The call order mirrors the host's:
    configure() -> preprocess(scene, camera, sampler...) -> render() [-> cancel()]."""

    def __init__(self, maxDepth=-1, rrDepth=10, strictNormals=False, device=0):
        self.maxDepth, self.rrDepth, self.strictNormals = int(maxDepth), int(rrDepth), bool(strictNormals)
        self._ctx = C.c_void_p()
        self._cancel = C.c_int(0)
        self._film_keep = None
        rc = lib().mtsgpu_create(int(device), C.byref(self._ctx))
        if rc != 0:
            raise MtsGpuError("mtsgpu_create: %s" % lib().mtsgpu_last_error(None).decode())
        self.camera = None

    def _chk(self, rc, what):
        if rc != 0:
            raise MtsGpuError("%s: %s (code %d)" % (what, lib().mtsgpu_last_error(self._ctx).decode(), rc))

    def configure(self):
        self._configure_integrator()
        return self

    def _configure_integrator(self):
        self._chk(lib().mtsgpu_set_integrator(self._ctx, self.maxDepth, self.rrDepth, int(self.strictNormals)), "set_integrator")

    def preprocess(self, scene, camera, sampler="independent", sampleCount=4, depth=3, seed=0x5EED):
        """Scene::preprocess -> Integrator::preprocess: upload the flattened scene, camera and sampler."""
        self.configure()
        sp = scene.ptr if isinstance(scene, Scene) else scene
        ta = scene.tangent_args() if isinstance(scene, Scene) else None
        cb = scene.cylinder_blocks() if isinstance(scene, Scene) else None
        if cb is not None:
            ta = ta if ta is not None else (None, None)
            self._chk(lib().mtsgpu_upload_scene_cylinders(self._ctx, sp, abi.ptr(ta[0], abi.f32p), abi.ptr(ta[1], abi.u32p), abi.ptr(cb, abi.f32p)), "upload_scene_cylinders")
        elif ta is not None:
            self._chk(lib().mtsgpu_upload_scene_tangents(self._ctx, sp, abi.ptr(ta[0], abi.f32p), abi.ptr(ta[1], abi.u32p)), "upload_scene_tangents")
        else:
            self._chk(lib().mtsgpu_upload_scene(self._ctx, sp), "upload_scene")
        vc = scene.vertex_color_args() if isinstance(scene, Scene) else None
        if vc is not None:
            self._chk(lib().mtsgpu_set_vertex_colors(self._ctx, *vc), "set_vertex_colors")
        ut = scene.uv_texture_args() if isinstance(scene, Scene) else None
        ub = scene.uv_bitmap_texture_args() if isinstance(scene, Scene) else None
        um = scene.uv_masked_texture_args() if isinstance(scene, Scene) else None
        if um is not None:
            self._chk(lib().mtsgpu_set_uv_masked_textures(self._ctx, *um), "set_uv_masked_textures")
        elif ub is not None:
            self._chk(lib().mtsgpu_set_uv_bitmap_textures(self._ctx, *ub), "set_uv_bitmap_textures")
        elif ut is not None:
            self._chk(lib().mtsgpu_set_uv_textures(self._ctx, *ut), "set_uv_textures")
        if isinstance(scene, Scene) and scene.bsdf_snow is not None:
            self._chk(lib().mtsgpu_set_snow_bsdfs(self._ctx, scene.bsdf_snow), "set_snow_bsdfs")
        if isinstance(scene, Scene) and scene.cloth is not None:
            if um is None and ub is None and ut is None:       # no texture call has handed the texcoords over: one without textures
                self._chk(lib().mtsgpu_set_uv_textures(self._ctx, *scene.uv_only_args()), "set_uv_textures")
            self._chk(lib().mtsgpu_set_cloth_bsdfs(self._ctx, len(scene.description.weaves), scene.cloth[0], abi.ptr(scene.cloth[2], abi.i32p)),
                      "set_cloth_bsdfs")
        sx = scene.spot_texture_args() if isinstance(scene, Scene) else None
        if sx is not None:
            self._chk(lib().mtsgpu_set_spot_textures(self._ctx, *sx), "set_spot_textures")
        self.camera = camera
        self._chk(lib().mtsgpu_set_camera(self._ctx, C.byref(camera.c if hasattr(camera, "c") else camera)), "set_camera")
        kind = {"independent": abi.SAMPLER_INDEPENDENT_KEYED, "ldsampler": abi.SAMPLER_LD_KEYED, "halton": abi.SAMPLER_HALTON,
                "hammersley": abi.SAMPLER_HAMMERSLEY, "stratified": abi.SAMPLER_STRATIFIED_KEYED}[sampler] if isinstance(sampler, str) else int(sampler)
        self._chk(lib().mtsgpu_set_sampler(self._ctx, kind, int(sampleCount), int(depth), int(seed)), "set_sampler")
        return True

    def set_tiles(self, block_size=32, part=0, n_parts=1):
        self._chk(lib().mtsgpu_set_tiles(self._ctx, block_size, part, n_parts), "set_tiles")

    def set_rfilter(self, kind="box", halfSize=-1.0, stddev=-1.0, B=-1.0, C=-1.0, cycles=-1.0):
        """Film reconstruction filter plugin (src/rfilters/{box,gaussian,mitchell,catmullrom,wsinc}.cpp); negative
        values select the plugin defaults"""
        if kind == "box":
            self._chk(lib().mtsgpu_set_rfilter(self._ctx, 0.5, 0.5, None), "set_rfilter")
            return
        size = np.zeros(2, dtype=np.float32); values = np.zeros(256, dtype=np.float32)
        k = {"gaussian": 1, "mitchell": 2, "catmullrom": 3, "wsinc": 4}[kind]
        p0, p1 = {1: (stddev, -1.0), 2: (B, C), 3: (-1.0, -1.0), 4: (cycles, -1.0)}[k]
        rc = lib().mtsgpu_tabulate_filter(k, halfSize, p0, p1, abi.ptr(size, abi.f32p), abi.ptr(values, abi.f32p))
        if rc != 0:
            raise MtsGpuError("mtsgpu_tabulate_filter: %s" % lib().mtsgpu_last_error(None).decode())
        self._chk(lib().mtsgpu_set_rfilter(self._ctx, float(size[0]), float(size[1]), abi.ptr(values, abi.f32p)), "set_rfilter")
        return size, values.reshape(16, 16)

    def set_film_edges(self, highQualityEdges=False):
        """Film property `highQualityEdges` (src/librender/film.cpp:51, renderproc.cpp:146-153)"""
        self._chk(lib().mtsgpu_set_film_edges(self._ctx, int(bool(highQualityEdges))), "set_film_edges")

    def set_options(self, max_paths=0, count_traversal=False, time_kernels=False):
        self._chk(lib().mtsgpu_set_options(self._ctx, int(max_paths), int(count_traversal), int(time_kernels)), "set_options")

    def set_tuning(self, **knobs):
        """scheduling knobs of the traversal kernel (mtsgpu_set_tuning); results never depend on them"""
        for k, v in knobs.items():
            self._chk(lib().mtsgpu_set_tuning(self._ctx, k.encode(), int(v)), "set_tuning")

    def set_stream(self, hip_stream):
        self._chk(lib().mtsgpu_set_stream(self._ctx, C.c_void_p(hip_stream)), "set_stream")

    def set_film_buffer(self, device_ptr, keepalive=None):
        self._film_keep = keepalive
        self._chk(lib().mtsgpu_set_film_buffer(self._ctx, C.c_void_p(device_ptr)), "set_film_buffer")

    def clear_film(self):
        self._chk(lib().mtsgpu_clear_film(self._ctx), "clear_film")

    def render(self):
        """SampleIntegrator::render: returns True, or False when cancelled (integrator.cpp:87-120)."""
        self._cancel.value = 0
        rc = lib().mtsgpu_render(self._ctx, C.byref(self._cancel))
        if rc == -4:
            return False
        self._chk(rc, "render")
        return True

    def cancel(self):
        self._cancel.value = 1

    def sync(self):
        self._chk(lib().mtsgpu_sync(self._ctx), "sync")

    def film(self):
        """[H][W][5] float32: spectrum rgb sum, alpha sum, weight sum (ImageBlock layout)"""
        cam = self.camera.c if hasattr(self.camera, "c") else self.camera
        out = np.zeros((cam.height, cam.width, 5), dtype=np.float32)
        self._chk(lib().mtsgpu_read_film(self._ctx, abi.ptr(out, abi.f32p)), "read_film")
        return out

    def stats(self):
        st = abi.Stats()
        self._chk(lib().mtsgpu_get_stats(self._ctx, C.byref(st)), "get_stats")
        d = st.as_dict()
        redone = C.c_uint64(0)      # not a field of mtsgpu_stats, whose layout is part of ABI version 8
        self._chk(lib().mtsgpu_hook_rays_redone(self._ctx, C.byref(redone)), "rays_redone")
        d["rays_redone"] = int(redone.value)
        return d

    def bin_entries(self):
        """entries the closest-hit launches of the last frame appended to every material queue (mtsgpu_bin_entries): one count per
        BSDF type, then the terminal queue"""
        out = (C.c_uint64 * (abi.BSDF_NTYPES + 1))()
        self._chk(lib().mtsgpu_bin_entries(self._ctx, out), "bin_entries")
        return [int(v) for v in out]

    # --- test-case mode (`mitsuba -t`, testmode.py) -----------------------------
    def set_film_statistics(self, on=True):
        """ImageBlocks with statistics (renderproc.cpp:44-50): render() also runs the per-pixel variance recurrence of
        SampleIntegrator::renderBlock (integrator.cpp:171-202).  Box filter only, as in the reference."""
        self._chk(lib().mtsgpu_set_film_statistics(self._ctx, int(bool(on))), "set_film_statistics")

    def film_statistics(self):
        """(variance [H][W][3] float32, nSamples [H][W] uint32) of the last render; pixels not rendered hold 0, 0"""
        cam = self.camera.c if hasattr(self.camera, "c") else self.camera
        var = np.zeros((cam.height, cam.width, 3), dtype=np.float32)
        n = np.zeros((cam.height, cam.width), dtype=np.uint32)
        self._chk(lib().mtsgpu_read_film_statistics(self._ctx, abi.ptr(var, abi.f32p), abi.ptr(n, abi.u32p)), "read_film_statistics")
        return var, n

    def film_statistics_form(self):
        """the form of the variance kernel the last pass ran: "lane", "wave" or None"""
        return {0: "lane", 1: "wave"}.get(lib().mtsgpu_film_statistics_form(self._ctx))

    # --- kernels exposed for parity tests --------------------------------------
    def trace_rays(self, rays, shadow=False):
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        hits = np.zeros((r.shape[0], 4), dtype=np.uint32)
        self._chk(lib().mtsgpu_trace_rays(self._ctx, abi.ptr(r, abi.f32p), r.shape[0], int(shadow), abi.ptr(hits, abi.u32p)), "trace_rays")
        return hits

    REPLAY_KINDS = {"deep": 0, "camera": 1, "shadow": 2}

    def replay_roof(self, n, stride=1, reps=3, kind="deep"):
        """mtsgpu_replay_roof: the request stream of n rays of the frame rendered last replayed without arithmetic, next to
        the product kernel on the same rays.  kind: "deep" = the last ray of every stride-th path (closest-hit kernel),
        "camera" = the camera rays of the last pass, generated again (closest-hit kernel, first-bounce launch shape),
        "shadow" = every stride-th slot of the shadow queue (any-hit kernel)"""
        out = (C.c_double * 12)()
        self._chk(lib().mtsgpu_replay_roof(self._ctx, self.REPLAY_KINDS[kind], int(n), int(stride), int(reps), out), "replay_roof")
        keys = ["rays", "requests", "truncated_rays", "product_ms", "replay_ms", "pair_global", "pair_lds", "node_global", "node_lds",
                "heads", "tails", "spills"]
        return dict(zip(keys, list(out)))

    def ld_tables(self, pixel_key, spp, depth):
        t1 = np.zeros((depth, spp), dtype=np.float32)
        t2 = np.zeros((depth, spp, 2), dtype=np.float32)
        self._chk(lib().mtsgpu_ld_tables(self._ctx, int(pixel_key), abi.ptr(t1, abi.f32p), abi.ptr(t2, abi.f32p)), "ld_tables")
        return t1, t2

    def sampler_values(self, pixel_key, sample_index, n, two_d=False):
        """generate() for the pixel, then n x next1D() (or next2D()) of camera sample `sample_index`, on the device"""
        out = np.zeros((n, 2) if two_d else (n,), dtype=np.float32)
        self._chk(lib().mtsgpu_sampler_values(self._ctx, int(pixel_key), int(sample_index), int(n), int(bool(two_d)),
                                              abi.ptr(out, abi.f32p)), "sampler_values")
        return out

    def random_values(self, op, n, seed=0, arg=0, clone=0):
        """the reference's Random (MT19937-64) on the device: op 0 nextULong, 1 nextFloat bits, 2 nextSize(arg), 3 shuffle(0..n-1)"""
        out = np.zeros(n, dtype=np.uint64)
        self._chk(lib().mtsgpu_random_values(self._ctx, int(op), int(seed), int(arg), int(clone), int(n),
                                             out.ctypes.data_as(C.POINTER(C.c_uint64))), "random_values")
        return out

    def bsdf_eval(self, bsdf_type, params, op, wi, aux):
        """BSDF::f (op 0), pdf (1), sample(bRec, pdf, sample) (2) on the device for n query records (mtsgpu_bsdf_eval):
        wi [n][3] or [3]; aux = wo [n][3] (op 0, 1) or the 2D sample [n][2] (op 2).  Returns [n][8]."""
        aux = np.atleast_2d(np.asarray(aux, dtype=np.float32))
        n = aux.shape[0]
        q = np.zeros((n, 6), dtype=np.float32)
        q[:, :3] = np.asarray(wi, dtype=np.float32).reshape(-1, 3)
        q[:, 3:3 + aux.shape[1]] = aux
        P = np.zeros(abi.BSDF_NPARAMS, dtype=np.float32); P[:len(params)] = params
        out = np.zeros((n, 8), dtype=np.float32)
        self._chk(lib().mtsgpu_bsdf_eval(self._ctx, int(bsdf_type), abi.ptr(P, abi.f32p), int(op), n, abi.ptr(q, abi.f32p),
                                         abi.ptr(out, abi.f32p)), "bsdf_eval")
        return out

    def bsdf_eval_table(self, types, params, index, op, wi, aux):
        """the same read-out for entry `index` of a BSDF table (mtsgpu_bsdf_eval_table): types [n_bsdfs], params
        [n_bsdfs][16] as a scene description holds them; a composite reads its children there"""
        aux = np.atleast_2d(np.asarray(aux, dtype=np.float32))
        n = aux.shape[0]
        q = np.zeros((n, 6), dtype=np.float32)
        q[:, :3] = np.asarray(wi, dtype=np.float32).reshape(-1, 3)
        q[:, 3:3 + aux.shape[1]] = aux
        T = np.ascontiguousarray(types, dtype=np.uint32).reshape(-1)
        P = np.ascontiguousarray(params, dtype=np.float32).reshape(len(T), abi.BSDF_NPARAMS)
        out = np.zeros((n, 8), dtype=np.float32)
        self._chk(lib().mtsgpu_bsdf_eval_table(self._ctx, len(T), abi.ptr(T, abi.u32p), abi.ptr(P, abi.f32p), int(index), int(op), n,
                                               abi.ptr(q, abi.f32p), abi.ptr(out, abi.f32p)), "bsdf_eval_table")
        return out

    def set_vertex_colors(self, vtx_col=None, shape_has_colors=None, bsdf_color_slots=None):
        """mtsgpu_set_vertex_colors on the uploaded scene: the colour pool [n_verts][3], one flag per shape, one slot mask
        per BSDF; all None switches the colours off"""
        a = None if vtx_col is None else np.ascontiguousarray(vtx_col, dtype=np.float32)
        b = None if shape_has_colors is None else np.ascontiguousarray(shape_has_colors, dtype=np.uint32)
        c = None if bsdf_color_slots is None else np.ascontiguousarray(bsdf_color_slots, dtype=np.uint32)
        self._chk(lib().mtsgpu_set_vertex_colors(self._ctx, abi.ptr(a, abi.f32p), abi.ptr(b, abi.u32p), abi.ptr(c, abi.u32p)), "set_vertex_colors")

    def set_uv_textures(self, vtx_uv=None, shape_has_uv=None, textures=None, bsdf_slot_texture=None):
        """mtsgpu_set_uv_textures on the uploaded scene: the texcoord pool [n_verts][2], one flag per shape, the textures
        (scenes.Checkerboard / GridTexture objects or abi.UvTexture), the table [n_bsdfs][2]; all None switches them off"""
        a = None if vtx_uv is None else np.ascontiguousarray(vtx_uv, dtype=np.float32)
        b = None if shape_has_uv is None else np.ascontiguousarray(shape_has_uv, dtype=np.uint32)
        t = None if textures is None else uv_texture_array(textures)
        s = None if bsdf_slot_texture is None else np.ascontiguousarray(bsdf_slot_texture, dtype=np.int32)
        self._chk(lib().mtsgpu_set_uv_textures(self._ctx, abi.ptr(a, abi.f32p), abi.ptr(b, abi.u32p), 0 if t is None else len(t), t,
                                               abi.ptr(s, abi.i32p)), "set_uv_textures")

    def set_uv_bitmap_textures(self, vtx_uv=None, shape_has_uv=None, textures=None, bsdf_slot_texture=None, bitmaps=None, texture_bitmap=None):
        """mtsgpu_set_uv_bitmap_textures on the uploaded scene: set_uv_textures() with bitmaps (scenes.BitmapTexture objects or
        abi.Bitmap) and the bitmap index per texture.  With bitmaps and texture_bitmap both None they are derived from the
        BitmapTexture objects among `textures` (none: n_bitmaps = 0)"""
        a = None if vtx_uv is None else np.ascontiguousarray(vtx_uv, dtype=np.float32)
        b = None if shape_has_uv is None else np.ascontiguousarray(shape_has_uv, dtype=np.uint32)
        if bitmaps is None and texture_bitmap is None and textures is not None:
            bitmaps, texture_bitmap = bitmap_table(textures)
        t = None if textures is None else uv_texture_array(textures)
        s = None if bsdf_slot_texture is None else np.ascontiguousarray(bsdf_slot_texture, dtype=np.int32)
        bm = None if not bitmaps else bitmap_array(bitmaps)
        tb = None if texture_bitmap is None else np.ascontiguousarray(texture_bitmap, dtype=np.int32)
        self._chk(lib().mtsgpu_set_uv_bitmap_textures(self._ctx, abi.ptr(a, abi.f32p), abi.ptr(b, abi.u32p), 0 if t is None else len(t), t,
                                                      abi.ptr(s, abi.i32p), 0 if bm is None else len(bitmaps), bm, abi.ptr(tb, abi.i32p)),
                  "set_uv_bitmap_textures")

    def set_uv_masked_textures(self, vtx_uv=None, shape_has_uv=None, textures=None, bsdf_slot_texture=None, bitmaps=None, texture_bitmap=None,
                               bsdf_mask=None):
        """mtsgpu_set_uv_masked_textures on the uploaded scene: set_uv_bitmap_textures() with one mask per BSDF, rows (kind,
        texture, opacity rgb) or abi.BsdfMask; all None switches masks and textures off"""
        a = None if vtx_uv is None else np.ascontiguousarray(vtx_uv, dtype=np.float32)
        b = None if shape_has_uv is None else np.ascontiguousarray(shape_has_uv, dtype=np.uint32)
        if bitmaps is None and texture_bitmap is None and textures is not None:
            bitmaps, texture_bitmap = bitmap_table(textures)
        t = None if textures is None else uv_texture_array(textures)
        s = None if bsdf_slot_texture is None else np.ascontiguousarray(bsdf_slot_texture, dtype=np.int32)
        bm = None if not bitmaps else bitmap_array(bitmaps)
        tb = None if texture_bitmap is None else np.ascontiguousarray(texture_bitmap, dtype=np.int32)
        m = None if bsdf_mask is None else bsdf_mask_array(bsdf_mask)
        self._chk(lib().mtsgpu_set_uv_masked_textures(self._ctx, abi.ptr(a, abi.f32p), abi.ptr(b, abi.u32p), 0 if t is None else len(t), t,
                                                      abi.ptr(s, abi.i32p), 0 if bm is None else len(bitmaps), bm, abi.ptr(tb, abi.i32p), m),
                  "set_uv_masked_textures")

    def set_snow_bsdfs(self, table=None):
        """mtsgpu_set_snow_bsdfs on the uploaded scene: one abi.BsdfSnow, row (kind, derived) or None per BSDF; None switches the
        table off"""
        self._chk(lib().mtsgpu_set_snow_bsdfs(self._ctx, None if table is None else bsdf_snow_array(table)), "set_snow_bsdfs")

    def bsdf_eval_snow(self, bsdf_type, entry, op, wi, aux):
        """bsdf_eval() of the snow record `entry`, an abi.BsdfSnow or a row (kind, derived) (mtsgpu_bsdf_eval_snow) -> [n][8]"""
        aux = np.atleast_2d(np.asarray(aux, dtype=np.float32))
        n = aux.shape[0]
        q = np.zeros((n, 6), dtype=np.float32)
        q[:, :3] = np.asarray(wi, dtype=np.float32).reshape(-1, 3)
        q[:, 3:3 + aux.shape[1]] = aux
        e = bsdf_snow_array([entry])
        out = np.zeros((n, 8), dtype=np.float32)
        self._chk(lib().mtsgpu_bsdf_eval_snow(self._ctx, int(bsdf_type), e, int(op), n, abi.ptr(q, abi.f32p), abi.ptr(out, abi.f32p)),
                  "bsdf_eval_snow")
        return out

    def set_cloth_bsdfs(self, weaves=None, bsdf_weave=None):
        """mtsgpu_set_cloth_bsdfs on the uploaded scene: scenes.Weave objects and one weave index (or -1) per BSDF; None switches
        the table off"""
        if bsdf_weave is None:
            self._chk(lib().mtsgpu_set_cloth_bsdfs(self._ctx, 0, None, None), "set_cloth_bsdfs")
            return
        arr, keep = weave_array(list(weaves or []))
        table = np.ascontiguousarray(bsdf_weave, dtype=np.int32)
        self._chk(lib().mtsgpu_set_cloth_bsdfs(self._ctx, len(weaves or []), arr, abi.ptr(table, abi.i32p)), "set_cloth_bsdfs")

    def bsdf_eval_cloth(self, bsdf_type, weave, op, wi, aux, uv):
        """bsdf_eval() of the cloth BRDF with the scenes.Weave `weave` at its.uv = uv (mtsgpu_bsdf_eval_cloth); op 3: the
        internals of f (yarn id, centre x, y, random1, random2, intensityVariation, u, v) -> [n][8]"""
        aux = np.atleast_2d(np.asarray(aux, dtype=np.float32))
        n = aux.shape[0]
        q = np.zeros((n, 8), dtype=np.float32)
        q[:, :3] = np.asarray(wi, dtype=np.float32).reshape(-1, 3)
        q[:, 3:3 + aux.shape[1]] = aux
        q[:, 6:8] = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
        arr, keep = weave_array([weave])
        out = np.zeros((n, 8), dtype=np.float32)
        self._chk(lib().mtsgpu_bsdf_eval_cloth(self._ctx, int(bsdf_type), arr, int(op), n, abi.ptr(q, abi.f32p), abi.ptr(out, abi.f32p)),
                  "bsdf_eval_cloth")
        return out

    def bsdf_eval_masked(self, bsdf_type, params, opacity, op, wi, aux):
        """bsdf_eval() through the mask adapter whose opacity is the spectrum `opacity` (mtsgpu_bsdf_eval_masked) -> [n][8]"""
        aux = np.atleast_2d(np.asarray(aux, dtype=np.float32))
        n = aux.shape[0]
        q = np.zeros((n, 6), dtype=np.float32)
        q[:, :3] = np.asarray(wi, dtype=np.float32).reshape(-1, 3)
        q[:, 3:3 + aux.shape[1]] = aux
        P = np.zeros(abi.BSDF_NPARAMS, dtype=np.float32); P[:len(params)] = params
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(opacity, dtype=np.float32), (3,)))
        out = np.zeros((n, 8), dtype=np.float32)
        self._chk(lib().mtsgpu_bsdf_eval_masked(self._ctx, int(bsdf_type), abi.ptr(P, abi.f32p), abi.ptr(o, abi.f32p), int(op), n,
                                                abi.ptr(q, abi.f32p), abi.ptr(out, abi.f32p)), "bsdf_eval_masked")
        return out

    def bitmap_texture_eval(self, texture, prim, rec, bitmap=None):
        """uv_texture_eval() for a scenes.BitmapTexture (or an abi.UvTexture of kind TEX_BITMAP with an abi.Bitmap)
        (mtsgpu_bitmap_texture_eval) -> [n][5] = uv, rgb"""
        p = np.ascontiguousarray(prim, dtype=np.uint32).reshape(-1)
        q = np.ascontiguousarray(rec, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((len(p), 5), dtype=np.float32)
        t = uv_texture_array([texture])
        bm = bitmap_array([texture if bitmap is None else bitmap])
        self._chk(lib().mtsgpu_bitmap_texture_eval(self._ctx, t, bm, len(p), abi.ptr(p, abi.u32p), abi.ptr(q, abi.f32p), abi.ptr(out, abi.f32p)),
                  "bitmap_texture_eval")
        return out

    def uv_texture_eval(self, texture, prim, rec):
        """its.uv and the texture's value on the device for records (primitive, (u, v, -) | world point) of the uploaded scene
        (mtsgpu_uv_texture_eval) -> [n][5] = uv, rgb"""
        p = np.ascontiguousarray(prim, dtype=np.uint32).reshape(-1)
        q = np.ascontiguousarray(rec, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((len(p), 5), dtype=np.float32)
        t = uv_texture_array([texture])
        self._chk(lib().mtsgpu_uv_texture_eval(self._ctx, t, len(p), abi.ptr(p, abi.u32p), abi.ptr(q, abi.f32p), abi.ptr(out, abi.f32p)), "uv_texture_eval")
        return out

    def bsdf_eval_slots(self, bsdf_type, params, source, color, values, op, wi, aux):
        """bsdf_eval() with texture slot s taking nothing (source[s] = 0), `color` (1) or values[s] (2) (mtsgpu_bsdf_eval_slots)
        -> [n][8]"""
        aux = np.atleast_2d(np.asarray(aux, dtype=np.float32))
        n = aux.shape[0]
        q = np.zeros((n, 6), dtype=np.float32)
        q[:, :3] = np.asarray(wi, dtype=np.float32).reshape(-1, 3)
        q[:, 3:3 + aux.shape[1]] = aux
        P = np.zeros(abi.BSDF_NPARAMS, dtype=np.float32); P[:len(params)] = params
        src = np.ascontiguousarray(source, dtype=np.int32).reshape(2)
        col = np.ascontiguousarray(color, dtype=np.float32).reshape(3)
        val = np.ascontiguousarray(values, dtype=np.float32).reshape(6)
        out = np.zeros((n, 8), dtype=np.float32)
        self._chk(lib().mtsgpu_bsdf_eval_slots(self._ctx, int(bsdf_type), abi.ptr(P, abi.f32p), abi.ptr(src, abi.i32p), abi.ptr(col, abi.f32p),
                                               abi.ptr(val, abi.f32p), int(op), n, abi.ptr(q, abi.f32p), abi.ptr(out, abi.f32p)), "bsdf_eval_slots")
        return out

    def upload_scene_tangents(self, scene, vtx_dpdu=None, shape_has_tangents=None):
        """mtsgpu_upload_scene_tangents with explicit arrays: vtx_dpdu [n_verts][3], shape_has_tangents [n_shapes] (both None =
        none); clears vertex colours and uv textures like every upload"""
        sp = scene.ptr if isinstance(scene, Scene) else scene
        a = None if vtx_dpdu is None else np.ascontiguousarray(vtx_dpdu, dtype=np.float32)
        b = None if shape_has_tangents is None else np.ascontiguousarray(shape_has_tangents, dtype=np.uint32)
        self._chk(lib().mtsgpu_upload_scene_tangents(self._ctx, sp, abi.ptr(a, abi.f32p), abi.ptr(b, abi.u32p)), "upload_scene_tangents")

    def shading_frame_eval(self, prim, rec):
        """the shading frame on the device for records (primitive, (u, v, -) | world point) of the uploaded scene
        (mtsgpu_shading_frame_eval) -> [n][9] = s, t, n"""
        p = np.ascontiguousarray(prim, dtype=np.uint32).reshape(-1)
        q = np.ascontiguousarray(rec, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((len(p), 9), dtype=np.float32)
        self._chk(lib().mtsgpu_shading_frame_eval(self._ctx, len(p), abi.ptr(p, abi.u32p), abi.ptr(q, abi.f32p), abi.ptr(out, abi.f32p)), "shading_frame_eval")
        return out

    def vertex_color_eval(self, prim, uv):
        """its.color on the device for records (primitive, u, v) of the uploaded scene (mtsgpu_vertex_color_eval) -> [n][3]"""
        p = np.ascontiguousarray(prim, dtype=np.uint32).reshape(-1)
        q = np.ascontiguousarray(uv, dtype=np.float32).reshape(-1, 2)
        out = np.zeros((len(p), 3), dtype=np.float32)
        self._chk(lib().mtsgpu_vertex_color_eval(self._ctx, len(p), abi.ptr(p, abi.u32p), abi.ptr(q, abi.f32p), abi.ptr(out, abi.f32p)), "vertex_color_eval")
        return out

    def bsdf_eval_colored(self, bsdf_type, params, slots, color, op, wi, aux):
        """bsdf_eval() with the texture slots of mask `slots` taking `color` (mtsgpu_bsdf_eval_colored) -> [n][8]"""
        aux = np.atleast_2d(np.asarray(aux, dtype=np.float32))
        n = aux.shape[0]
        q = np.zeros((n, 6), dtype=np.float32)
        q[:, :3] = np.asarray(wi, dtype=np.float32).reshape(-1, 3)
        q[:, 3:3 + aux.shape[1]] = aux
        P = np.zeros(abi.BSDF_NPARAMS, dtype=np.float32); P[:len(params)] = params
        col = np.ascontiguousarray(color, dtype=np.float32).reshape(3)
        out = np.zeros((n, 8), dtype=np.float32)
        self._chk(lib().mtsgpu_bsdf_eval_colored(self._ctx, int(bsdf_type), abi.ptr(P, abi.f32p), int(slots), abi.ptr(col, abi.f32p), int(op), n,
                                                 abi.ptr(q, abi.f32p), abi.ptr(out, abi.f32p)), "bsdf_eval_colored")
        return out

    def lum_eval(self, lum_type, block, op, a, b=None):
        """the luminaire plugins on the device for n query records (mtsgpu_lum_eval; the sky): op 0 Le(a = direction
        [n][3]); op 1 sample(a = p [n][3], b = the 2D sample [n][2]); op 2 pdf(a = p, b = lRec.d).  Returns [n][12]:
        Le.rgb | d.xyz, pdf, value.rgb, -, end point of the shadow ray xyz | pdf"""
        a = np.atleast_2d(np.asarray(a, dtype=np.float32))
        n = a.shape[0]
        q = np.zeros((n, 6), dtype=np.float32)
        q[:, :3] = a
        if b is not None:
            b = np.atleast_2d(np.asarray(b, dtype=np.float32))
            q[:, 3:3 + b.shape[1]] = b
        P = np.zeros(abi.LUM_NPARAMS, dtype=np.float32); P[:len(block)] = block
        out = np.zeros((n, 12), dtype=np.float32)
        self._chk(lib().mtsgpu_lum_eval(self._ctx, int(lum_type), abi.ptr(P, abi.f32p), int(op), n, abi.ptr(q, abi.f32p),
                                        abi.ptr(out, abi.f32p)), "lum_eval")
        return out

    def set_spot_textures(self, textures=None, texture_bilinear=None, lum_texture=None):
        """mtsgpu_set_spot_textures on the uploaded scene: scenes texture objects, one filter flag per texture and one texture index
        (or -1) per luminaire; all None switches the projection textures off"""
        if textures is None and lum_texture is None:
            self._chk(lib().mtsgpu_set_spot_textures(self._ctx, 0, None, 0, None, None, None, None), "set_spot_textures")
            return
        textures = list(textures or [])
        sb, stb = bitmap_table(textures)
        fl = None if texture_bilinear is None else np.ascontiguousarray(texture_bilinear, dtype=np.uint32)
        lx = np.ascontiguousarray(lum_texture, dtype=np.int32)
        self._chk(lib().mtsgpu_set_spot_textures(self._ctx, len(textures), uv_texture_array(textures) if textures else None, len(sb),
                                                 bitmap_array(sb) if sb else None, abi.ptr(stb, abi.i32p) if sb else None,
                                                 abi.ptr(fl, abi.u32p), abi.ptr(lx, abi.i32p)), "set_spot_textures")

    def spot_eval(self, block, texture, points, bilinear=False):
        """SpotLuminaire::sample with the projection texture `texture` on the device (mtsgpu_spot_eval) for the spot whose parameter
        block is `block` and points [n][3] -> [n][8] = lRec.d, uv, lRec.value"""
        b = np.ascontiguousarray(block, dtype=np.float32).reshape(abi.LUM_NPARAMS)
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((len(p), 8), dtype=np.float32)
        t = uv_texture_array([texture])
        bm = bitmap_array([texture]) if getattr(texture, "kind", None) == abi.TEX_BITMAP else None
        self._chk(lib().mtsgpu_spot_eval(self._ctx, abi.ptr(b, abi.f32p), t, bm, 1 if bilinear else 0, len(p), abi.ptr(p, abi.f32p),
                                         abi.ptr(out, abi.f32p)), "spot_eval")
        return out

    def scene_lum_eval(self, op, queries):
        """the luminaires of the uploaded scene on the device (mtsgpu_scene_lum_eval) for query records [n][16]: op 0
        sampleLuminaire(p, s) without the occlusion test, op 1 pdfLuminaire(p, lRec.p, lRec.n, lRec.d, index), op 2 the
        background's Le(direction).  Returns [n][16]: found, index, p, n, d, pdf, value | pdf | Le.rgb"""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 16)
        out = np.zeros((q.shape[0], 16), dtype=np.float32)
        self._chk(lib().mtsgpu_scene_lum_eval(self._ctx, int(op), q.shape[0], abi.ptr(q, abi.f32p), abi.ptr(out, abi.f32p)), "scene_lum_eval")
        return out

    def li_samples(self, pix_samples):
        ps = np.ascontiguousarray(pix_samples, dtype=np.uint32).reshape(-1, 3)
        out = np.zeros((ps.shape[0], 8), dtype=np.float32)
        self._chk(lib().mtsgpu_li_samples(self._ctx, abi.ptr(ps, abi.u32p), ps.shape[0], abi.ptr(out, abi.f32p)), "li_samples")
        return out

    def pass_samples(self, first=0, n=None):
        """records first .. first + n of the pass rendered last, as the film kernels read them (mtsgpu_pass_samples): [n][8]
        float32 laid out like li_samples(), the pixel key as a bit pattern in column 7.  n = None: up to the end of the pass
        (camera_samples of the last render when it took one pass)"""
        return _pass_samples(self._ctx, first, self.stats()["camera_samples"] - int(first) if n is None else n)

    def camera_rays(self, pix_samples=None, first=0, n=None):
        """the camera records as the camera kernel leaves them (mtsgpu_camera_rays): [n][14] float32 = o, mint, d, maxt, raster
        x, y, then as bit patterns the sampler counters d1, d2, the pixel key and the sample index.  pix_samples [n][3] int32
        (pixel x, y of the crop window -- the border pixels of highQualityEdges at negative coordinates included -- and the
        sample index), or None for records first .. first + n of the pass rendered last, generated once more.  Either way
        the last pass is invalid afterwards"""
        if pix_samples is None:
            ps, count = None, int(n)
        else:
            ps = np.ascontiguousarray(pix_samples, dtype=np.int32).reshape(-1, 3)
            count = ps.shape[0]
        out = np.zeros((count, abi.CAMERA_RAY_FLOATS), dtype=np.float32)
        self._chk(lib().mtsgpu_camera_rays(self._ctx, None if ps is None else abi.ptr(ps, abi.i32p), int(first), count, abi.ptr(out, abi.f32p)),
                  "camera_rays")
        return out

    def close(self):
        if self._ctx and _lib is not None:
            _lib.mtsgpu_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceGroup:
    """Several GPUs behind one host process (mtsgpu_create_multi): what the Mitsuba plugin uses, since Scene::render
    calls Integrator::render once (src/librender/scene.cpp:356-359).  devices may repeat (two contexts on one GPU)."""

    def __init__(self, devices, maxDepth=-1, rrDepth=10, strictNormals=False):
        self.maxDepth, self.rrDepth, self.strictNormals = int(maxDepth), int(rrDepth), bool(strictNormals)
        self._g = C.c_void_p()
        self._cancel = C.c_int(0)
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        rc = lib().mtsgpu_create_multi(len(devices), devs, C.byref(self._g))
        if rc != 0:
            raise MtsGpuError("mtsgpu_create_multi: %s" % lib().mtsgpu_last_error(None).decode())
        self.camera = None

    def _chk(self, rc, what):
        if rc != 0:
            raise MtsGpuError("%s: %s (code %d)" % (what, lib().mtsgpu_group_last_error(self._g).decode(), rc))

    def __len__(self):
        return lib().mtsgpu_group_size(self._g)

    def member(self, i):
        return lib().mtsgpu_group_ctx(self._g, int(i))

    def preprocess(self, scene, camera, sampler="independent", sampleCount=4, depth=3, seed=0x5EED):
        sp = scene.ptr if isinstance(scene, Scene) else scene
        self._chk(lib().mtsgpu_group_set_integrator(self._g, self.maxDepth, self.rrDepth, int(self.strictNormals)), "set_integrator")
        ta = scene.tangent_args() if isinstance(scene, Scene) else None
        cb = scene.cylinder_blocks() if isinstance(scene, Scene) else None
        if cb is not None:
            ta = ta if ta is not None else (None, None)
            self._chk(lib().mtsgpu_group_upload_scene_cylinders(self._g, sp, abi.ptr(ta[0], abi.f32p), abi.ptr(ta[1], abi.u32p), abi.ptr(cb, abi.f32p)), "upload_scene_cylinders")
        elif ta is not None:
            self._chk(lib().mtsgpu_group_upload_scene_tangents(self._g, sp, abi.ptr(ta[0], abi.f32p), abi.ptr(ta[1], abi.u32p)), "upload_scene_tangents")
        else:
            self._chk(lib().mtsgpu_group_upload_scene(self._g, sp), "upload_scene")
        vc = scene.vertex_color_args() if isinstance(scene, Scene) else None
        if vc is not None:
            self._chk(lib().mtsgpu_group_set_vertex_colors(self._g, *vc), "set_vertex_colors")
        ut = scene.uv_texture_args() if isinstance(scene, Scene) else None
        ub = scene.uv_bitmap_texture_args() if isinstance(scene, Scene) else None
        um = scene.uv_masked_texture_args() if isinstance(scene, Scene) else None
        if um is not None:
            self._chk(lib().mtsgpu_group_set_uv_masked_textures(self._g, *um), "set_uv_masked_textures")
        elif ub is not None:
            self._chk(lib().mtsgpu_group_set_uv_bitmap_textures(self._g, *ub), "set_uv_bitmap_textures")
        elif ut is not None:
            self._chk(lib().mtsgpu_group_set_uv_textures(self._g, *ut), "set_uv_textures")
        if isinstance(scene, Scene) and scene.bsdf_snow is not None:
            self._chk(lib().mtsgpu_group_set_snow_bsdfs(self._g, scene.bsdf_snow), "set_snow_bsdfs")
        if isinstance(scene, Scene) and scene.cloth is not None:
            if um is None and ub is None and ut is None:
                self._chk(lib().mtsgpu_group_set_uv_textures(self._g, *scene.uv_only_args()), "set_uv_textures")
            self._chk(lib().mtsgpu_group_set_cloth_bsdfs(self._g, len(scene.description.weaves), scene.cloth[0], abi.ptr(scene.cloth[2], abi.i32p)),
                      "set_cloth_bsdfs")
        sx = scene.spot_texture_args() if isinstance(scene, Scene) else None
        if sx is not None:
            self._chk(lib().mtsgpu_group_set_spot_textures(self._g, *sx), "set_spot_textures")
        self.camera = camera
        self._chk(lib().mtsgpu_group_set_camera(self._g, C.byref(camera.c)), "set_camera")
        kind = {"independent": abi.SAMPLER_INDEPENDENT_KEYED, "ldsampler": abi.SAMPLER_LD_KEYED, "halton": abi.SAMPLER_HALTON,
                "hammersley": abi.SAMPLER_HAMMERSLEY, "stratified": abi.SAMPLER_STRATIFIED_KEYED}[sampler]
        self._chk(lib().mtsgpu_group_set_sampler(self._g, kind, int(sampleCount), int(depth), int(seed)), "set_sampler")
        return True

    def set_rfilter(self, kind="box", halfSize=-1.0, stddev=-1.0):
        if kind == "box":
            self._chk(lib().mtsgpu_group_set_rfilter(self._g, 0.5, 0.5, None), "set_rfilter")
            return
        size = np.zeros(2, dtype=np.float32); values = np.zeros(256, dtype=np.float32)
        rc = lib().mtsgpu_tabulate_filter({"gaussian": 1, "mitchell": 2, "catmullrom": 3, "wsinc": 4}[kind], halfSize, stddev, -1.0,
                                          abi.ptr(size, abi.f32p), abi.ptr(values, abi.f32p))
        if rc != 0:
            raise MtsGpuError("mtsgpu_tabulate_filter: %s" % lib().mtsgpu_last_error(None).decode())
        self._chk(lib().mtsgpu_group_set_rfilter(self._g, float(size[0]), float(size[1]), abi.ptr(values, abi.f32p)), "set_rfilter")

    def render(self, block_size=32, ordered_reduce=False):
        """ordered_reduce: False / 0 = RCCL when possible, True / 1 = the ordered peer-copy sum, 2 = RCCL must initialise"""
        self._cancel.value = 0
        rc = lib().mtsgpu_group_render(self._g, int(block_size), int(ordered_reduce), C.byref(self._cancel))
        if rc == -4:
            return False
        self._chk(rc, "group_render")
        return True

    def cancel(self):
        self._cancel.value = 1

    def reduce_kind(self):
        return {0: "ordered peer-copy sum", 1: "rccl ncclReduce"}.get(lib().mtsgpu_group_last_reduce_kind(self._g))

    def rccl_ranks(self):
        """ranks of the group's RCCL communicator once it has passed its self-check, else 0"""
        return int(lib().mtsgpu_group_rccl_ranks(self._g))

    def set_tuning(self, **knobs):
        """mtsgpu_set_tuning on every member (and the group's own test knob rccl_fail)"""
        for k, v in knobs.items():
            self._chk(lib().mtsgpu_group_set_tuning(self._g, k.encode(), int(v)), "group_set_tuning")

    def reduce_note(self):
        """why the last render fell back to the ordered sum ("" when it did not)"""
        return lib().mtsgpu_group_reduce_note(self._g).decode()

    def film(self):
        out = np.zeros((self.camera.c.height, self.camera.c.width, 5), dtype=np.float32)
        rc = lib().mtsgpu_read_film(self.member(0), abi.ptr(out, abi.f32p))
        if rc != 0:
            raise MtsGpuError("read_film: %s" % lib().mtsgpu_last_error(self.member(0)).decode())
        return out

    def set_film_statistics(self, on=True):
        """test-case mode on every member; member 0 holds the merged statistics after render()"""
        self._chk(lib().mtsgpu_group_set_film_statistics(self._g, int(bool(on))), "group_set_film_statistics")

    def film_statistics(self):
        var = np.zeros((self.camera.c.height, self.camera.c.width, 3), dtype=np.float32)
        n = np.zeros((self.camera.c.height, self.camera.c.width), dtype=np.uint32)
        rc = lib().mtsgpu_read_film_statistics(self.member(0), abi.ptr(var, abi.f32p), abi.ptr(n, abi.u32p))
        if rc != 0:
            raise MtsGpuError("read_film_statistics: %s (code %d)" % (lib().mtsgpu_last_error(self.member(0)).decode(), rc))
        return var, n

    def member_pass_samples(self, i, first=0, n=None):
        """pass_samples() of member i, read through mtsgpu_group_ctx"""
        return _pass_samples(self.member(i), first, self.member_stats(i)["camera_samples"] - int(first) if n is None else n)

    def member_stats(self, i):
        st = abi.Stats()
        lib().mtsgpu_get_stats(self.member(i), C.byref(st))
        return st.as_dict()

    def close(self):
        if self._g and _lib is not None:
            _lib.mtsgpu_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _pass_samples(ctx, first, n):
    out = np.zeros((int(n), 8), dtype=np.float32)
    rc = lib().mtsgpu_pass_samples(ctx, int(first), int(n), abi.ptr(out, abi.f32p))
    if rc != 0:
        raise MtsGpuError("pass_samples: %s (code %d)" % (lib().mtsgpu_last_error(ctx).decode(), rc))
    return out


def sky_configure(block):
    """SkyLuminaire::configure() for one LUM_SKY block (mtsgpu_sky_configure, host only): zenith x / y / Y, the 3 x 5 Perez
    coefficients (x, y, Y), their three denominators, sin and cos of thetaS"""
    P = np.zeros(abi.LUM_NPARAMS, dtype=np.float32); P[:len(block)] = block
    out = np.zeros(abi.SKY_NDERIVED, dtype=np.float32)
    if lib().mtsgpu_sky_configure(abi.ptr(P, abi.f32p), abi.ptr(out, abi.f32p)) != 0:
        raise MtsGpuError("mtsgpu_sky_configure: %s" % lib().mtsgpu_last_error(None).decode())
    return out


def hbm_triad_gbs(device=0, gib=1.0, iters=5):
    """measured HBM triad bandwidth in GB/s (the practical roof next to the 8 TB/s specification), None on failure"""
    out = C.c_double(0)
    rc = lib().mtsgpu_hbm_triad(int(device), int(gib * (1 << 30)), int(iters), C.byref(out))
    return float(out.value) if rc == 0 and out.value > 0 else None


def gather_roof(device=0, footprint_mib=4):
    """measured lane-level 16-byte gather requests per second (the roof of the traversal kernel), None on failure"""
    out = C.c_double(0)
    rc = lib().mtsgpu_gather_roof(int(device), int(footprint_mib) << 20, C.byref(out))
    return float(out.value) if rc == 0 and out.value > 0 else None


class MIDirectIntegrator(MIPathTracer):
    """The `direct` integrator (src/integrators/direct/direct.cpp); more than one sample per strategy needs a sampler
    with sample arrays (independent, ldsampler, stratified), as in the reference"""

    def __init__(self, luminaireSamples=1, bsdfSamples=1, device=0):
        MIPathTracer.__init__(self, device=device)
        self.luminaireSamples, self.bsdfSamples = int(luminaireSamples), int(bsdfSamples)

    def _configure_integrator(self):
        self._chk(lib().mtsgpu_set_direct_integrator(self._ctx, self.luminaireSamples, self.bsdfSamples), "set_direct_integrator")


def develop(film):
    """Film::develop: pixel = spectrum * (1 / weight) (src/films/mfilm.cpp:108-116)"""
    w = film[..., 4:5]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(w > 0, np.float32(1.0) / w, np.float32(0)).astype(np.float32)
    return (film[..., :3] * inv).astype(np.float32)
