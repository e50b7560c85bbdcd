"""libmtsgpu.so: where it is, how it is built, and the one table of its symbols' signatures.

TABLE states every symbol the package calls once, under the header that declares it.  The name lists the tests hold
against the headers (EXPORTS, MASK_EXPORTS, ...) are read off it and lib() applies it, so a symbol with a name and no
signature -- called with ctypes' default conversions -- cannot occur."""
import ctypes as C
import os
import subprocess

from . import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# MTSGPU_LIB selects an experiment build (tools/build_variant.sh); the product is libmtsgpu.so next to this file
LIB_PATH = os.environ.get("MTSGPU_LIB") or os.path.join(_HERE, "libmtsgpu.so")


class MtsGpuError(RuntimeError):
    pass


P = C.POINTER
I, U, U64, F, Z, S, LONG = C.c_int, C.c_uint32, C.c_uint64, C.c_float, C.c_size_t, C.c_char_p, C.c_long
vp, f32p, u32p, i32p, f64p = C.c_void_p, abi.f32p, abi.u32p, abi.i32p, P(C.c_double)
scenep, camp, descp, kdp = P(abi.Scene), P(abi.Camera), P(abi.SceneDesc), P(abi.KdParams)
texp, bmpp, mskp, snwp, wvp, cylp = P(abi.UvTexture), P(abi.Bitmap), P(abi.BsdfMask), P(abi.BsdfSnow), P(abi.Weave), P(abi.Cylinder)
# the arguments after the handle that a context's call and its group's twin share
_COLORS = [f32p, u32p, u32p]
_UV = [f32p, u32p, U, texp, i32p]
_UV_BITMAPS = _UV + [U, bmpp, i32p]
_TANGENTS = [scenep, f32p, u32p]
_SPOT = [U, texp, U, bmpp, i32p, u32p, i32p]
_QUERY = [I, U, f32p, f32p]         # op, n, the query records, the results

# header -> rows (name, argtypes) or (name, argtypes, restype), in the order of the name list; restype: int unless given
TABLE = {
    "mtsgpu.h": [       # the list that ABI version 8 fixes
        ("mtsgpu_create", [I, P(vp)]),
        ("mtsgpu_destroy", [vp], None),
        ("mtsgpu_last_error", [vp], S),
        ("mtsgpu_abi_version", []),
        ("mtsgpu_source_hash", [], S),
        ("mtsgpu_abi_sizeof", [I], Z),
        ("mtsgpu_set_stream", [vp, vp]),
        ("mtsgpu_upload_scene", [vp, scenep]),
        ("mtsgpu_set_camera", [vp, camp]),
        ("mtsgpu_set_integrator", [vp, I, I, I]),
        ("mtsgpu_set_direct_integrator", [vp, I, I]),
        ("mtsgpu_set_sampler", [vp, I, U, I, U64]),
        ("mtsgpu_set_tiles", [vp, I, I, I]),
        ("mtsgpu_set_rfilter", [vp, F, F, f32p]),
        ("mtsgpu_set_film_edges", [vp, I]),
        ("mtsgpu_tabulate_filter", [I, F, F, F, f32p, f32p]),
        ("mtsgpu_set_film_buffer", [vp, vp]),
        ("mtsgpu_set_options", [vp, U64, I, I]),
        ("mtsgpu_render", [vp, P(I)]),
        ("mtsgpu_sync", [vp]),
        ("mtsgpu_read_film", [vp, f32p]),
        ("mtsgpu_clear_film", [vp]),
        ("mtsgpu_get_stats", [vp, P(abi.Stats)]),
        ("mtsgpu_trace_rays", [vp, f32p, U, I, u32p]),
        ("mtsgpu_ld_tables", [vp, U, f32p, f32p]),
        ("mtsgpu_li_samples", [vp, u32p, U, f32p]),
        ("mtsgpu_flatten", [descp, kdp, P(vp)]),
        ("mtsgpu_flat_scene_get", [vp], scenep),
        ("mtsgpu_flat_scene_free", [vp], None),
        ("mtsgpu_flat_scene_kdstats", [vp, f64p]),
        ("mtsgpu_make_camera", [f32p, f32p, f32p, F, I, I, camp]),
        ("mtsgpu_make_camera_ortho", [f32p, f32p, f32p, F, F, I, I, camp]),
        ("mtsgpu_load_serialized", [S, I, P(vp), P(abi.Mesh)]),
        ("mtsgpu_loaded_mesh_free", [vp], None),
        ("mtsgpu_make_camera_crop", [f32p, f32p, f32p, F] + [I] * 6 + [camp]),
        ("mtsgpu_hbm_triad", [I, Z, I, f64p]),
        ("mtsgpu_sampler_values", [vp, U, U, U, I, f32p]),
        ("mtsgpu_random_values", [vp, I, U64, U64, U, U, P(U64)]),
        ("mtsgpu_set_tuning", [vp, S, LONG]),
        ("mtsgpu_gather_roof", [I, Z, f64p]),
        ("mtsgpu_create_multi", [I, P(I), P(vp)]),
        ("mtsgpu_group_destroy", [vp], None),
        ("mtsgpu_group_size", [vp]),
        ("mtsgpu_group_ctx", [vp, I], vp),
        ("mtsgpu_group_last_error", [vp], S),
        ("mtsgpu_group_upload_scene", [vp, scenep]),
        ("mtsgpu_group_set_camera", [vp, camp]),
        ("mtsgpu_group_set_integrator", [vp, I, I, I]),
        ("mtsgpu_group_set_sampler", [vp, I, U, I, U64]),
        ("mtsgpu_group_set_rfilter", [vp, F, F, f32p]),
        ("mtsgpu_group_render", [vp, I, I, P(I)]),
        ("mtsgpu_group_last_reduce_kind", [vp]),
        ("mtsgpu_group_rccl_ranks", [vp]),
        ("mtsgpu_group_reduce_note", [vp], S),
        ("mtsgpu_bsdf_eval", [vp, U, f32p] + _QUERY),
        ("mtsgpu_bsdf_eval_table", [vp, U, u32p, f32p, U] + _QUERY),
        ("mtsgpu_replay_roof", [vp, I, U, U, I, f64p]),
        ("mtsgpu_group_set_tuning", [vp, S, LONG]),
        ("mtsgpu_sky_configure", [f32p, f32p]),
        ("mtsgpu_lum_eval", [vp, U, f32p] + _QUERY),
        ("mtsgpu_scene_lum_eval", [vp] + _QUERY),
        ("mtsgpu_pass_samples", [vp, U, U, f32p]),
        ("mtsgpu_set_film_statistics", [vp, I]),
        ("mtsgpu_read_film_statistics", [vp, f32p, u32p]),
        ("mtsgpu_film_statistics_form", [vp]),
        ("mtsgpu_group_set_film_statistics", [vp, I]),
        ("mtsgpu_set_vertex_colors", [vp] + _COLORS),
        ("mtsgpu_group_set_vertex_colors", [vp] + _COLORS),
        ("mtsgpu_flat_scene_set_mesh_colors", [vp, U, f32p]),
        ("mtsgpu_flat_scene_vertex_colors", [vp], f32p),
        ("mtsgpu_flat_scene_shape_has_colors", [vp], u32p),
        ("mtsgpu_loaded_mesh_colors", [vp], f32p),
        ("mtsgpu_vertex_color_eval", [vp, U, u32p, f32p, f32p]),
        ("mtsgpu_bsdf_eval_colored", [vp, U, f32p, U, f32p] + _QUERY),
        ("mtsgpu_set_uv_textures", [vp] + _UV),
        ("mtsgpu_group_set_uv_textures", [vp] + _UV),
        ("mtsgpu_flat_scene_set_mesh_texcoords", [vp, U, f32p]),
        ("mtsgpu_flat_scene_vertex_texcoords", [vp], f32p),
        ("mtsgpu_flat_scene_shape_has_texcoords", [vp], u32p),
        ("mtsgpu_loaded_mesh_texcoords", [vp], f32p),
        ("mtsgpu_uv_texture_eval", [vp, texp, U, u32p, f32p, f32p]),
        ("mtsgpu_bsdf_eval_slots", [vp, U, f32p, i32p, f32p, f32p] + _QUERY),
        ("mtsgpu_flatten_tangents", [descp, kdp, P(f32p), P(vp)]),
        ("mtsgpu_flat_scene_vertex_tangents", [vp], f32p),
        ("mtsgpu_flat_scene_shape_has_tangents", [vp], u32p),
        ("mtsgpu_upload_scene_tangents", [vp] + _TANGENTS),
        ("mtsgpu_group_upload_scene_tangents", [vp] + _TANGENTS),
        ("mtsgpu_shading_frame_eval", [vp, U, u32p, f32p, f32p]),
        ("mtsgpu_bin_entries", [vp, P(U64)]),
        ("mtsgpu_set_uv_bitmap_textures", [vp] + _UV_BITMAPS),
        ("mtsgpu_group_set_uv_bitmap_textures", [vp] + _UV_BITMAPS),
        ("mtsgpu_bitmap_texture_eval", [vp, texp, bmpp, U, u32p, f32p, f32p]),
        ("mtsgpu_ldr_texels", [I, U, U, P(C.c_uint8), F, f32p]),
        ("mtsgpu_camera_rays", [vp, i32p, U, U, f32p]),
    ],
    "mtsgpu_mask.h": [      # the mask BSDF: an extension next to the list of mtsgpu.h
        ("mtsgpu_set_uv_masked_textures", [vp] + _UV_BITMAPS + [mskp]),
        ("mtsgpu_group_set_uv_masked_textures", [vp] + _UV_BITMAPS + [mskp]),
        ("mtsgpu_bsdf_eval_masked", [vp, U, f32p, f32p] + _QUERY),
    ],
    "mtsgpu_snow.h": [      # the snow BRDFs (wiscombe, hanrahankrueger)
        ("mtsgpu_wiscombe_configure", [f32p, snwp]),
        ("mtsgpu_hk_configure", [f32p, snwp]),
        ("mtsgpu_set_snow_bsdfs", [vp, snwp]),
        ("mtsgpu_group_set_snow_bsdfs", [vp, snwp]),
        ("mtsgpu_bsdf_eval_snow", [vp, U, snwp] + _QUERY),
    ],
    "mtsgpu_cloth.h": [     # the woven-cloth BRDF (irawan)
        ("mtsgpu_set_cloth_bsdfs", [vp, U, wvp, i32p]),
        ("mtsgpu_group_set_cloth_bsdfs", [vp, U, wvp, i32p]),
        ("mtsgpu_flatten_tangents_flagged", [descp, kdp, P(f32p), u32p, P(vp)]),
        ("mtsgpu_bsdf_eval_cloth", [vp, U, wvp] + _QUERY),
        ("mtsgpu_cloth_check", [wvp, f32p]),
        ("mtsgpu_devmath", [I, U, f32p, f32p, f32p]),
    ],
    "mtsgpu_spot.h": [      # the projection textures of the spot luminaire
        ("mtsgpu_set_spot_textures", [vp] + _SPOT),
        ("mtsgpu_group_set_spot_textures", [vp] + _SPOT),
        ("mtsgpu_spot_textures_check", [U, u32p, f32p] + _SPOT + [U, f32p]),
        ("mtsgpu_spot_eval", [vp, f32p, texp, bmpp, U, U, f32p, f32p]),
    ],
    "mtsgpu_cylinder.h": [  # the cylinder shape
        ("mtsgpu_cylinder_configure", [cylp, f32p]),
        ("mtsgpu_flatten_cylinders", [descp, kdp, P(f32p), u32p, cylp, P(vp)]),
        ("mtsgpu_flat_scene_cylinders", [vp], f32p),
        ("mtsgpu_upload_scene_cylinders", [vp] + _TANGENTS + [f32p]),
        ("mtsgpu_group_upload_scene_cylinders", [vp] + _TANGENTS + [f32p]),
        ("mtsgpu_cylinder_aabb", [f32p, f32p]),
        ("mtsgpu_cylinder_clip", [f32p, U, f32p, I, f32p, u32p]),
    ],
    "hooks": [              # outside the ABI (csrc/ctx.h), in no name list
        ("mtsgpu_hook_rays_redone", [vp, P(U64)]),
    ],
}
EXPORTS, MASK_EXPORTS, SNOW_EXPORTS, CLOTH_EXPORTS, SPOT_EXPORTS, CYLINDER_EXPORTS = (
    [row[0] for row in TABLE["mtsgpu" + ext + ".h"]] for ext in ("", "_mask", "_snow", "_cloth", "_spot", "_cylinder"))


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
    for rows in TABLE.values():
        for name, argtypes, *restype in rows:
            fn = getattr(L, name)
            fn.argtypes = argtypes
            if restype:
                fn.restype = restype[0]
    _lib = L
    return L


def check(rc, what):
    """the result of a call that takes no context: raises with the library's own text"""
    if rc != 0:
        raise MtsGpuError("%s: %s" % (what, lib().mtsgpu_last_error(None).decode()))
