"""The integrators: MIPathTracer and MIDirectIntegrator on one context, DeviceGroup on several.  What they do alike --
running a scene's upload plan, camera, sampler, reconstruction filter, film read-back -- is Driver's."""
import ctypes as C

import numpy as np

from . import abi, binding
from .binding import MtsGpuError, check, lib
from .cameras import struct_of
from .flatscene import Scene, bitmap_array, bitmap_table, bsdf_mask_array, bsdf_snow_array, upload_plan, uv_texture_array, weave_array
from .hooks import ReadOuts, read_pass_samples


def _chk_ctx(ctx, rc, what):
    if rc != 0:
        raise MtsGpuError("%s: %s (code %d)" % (what, lib().mtsgpu_last_error(ctx).decode(), rc))


def _or_none(a, dtype):
    return None if a is None else np.ascontiguousarray(a, dtype=dtype)


class Driver:
    """One handle of the library behind the host's call order configure -> preprocess -> render [-> cancel].  A subclass
    creates _handle and names the prefix of its symbols (_prefix), its last-error symbol (_last_error) and its destructor
    (_destroy)."""
    SAMPLERS = {"independent": abi.SAMPLER_INDEPENDENT_KEYED, "ldsampler": abi.SAMPLER_LD_KEYED, "halton": abi.SAMPLER_HALTON,
                "hammersley": abi.SAMPLER_HAMMERSLEY, "stratified": abi.SAMPLER_STRATIFIED_KEYED}
    FILTERS = {"gaussian": 1, "mitchell": 2, "catmullrom": 3, "wsinc": 4}

    def _chk(self, rc, what):
        if rc != 0:
            raise MtsGpuError("%s: %s (code %d)" % (what, getattr(lib(), self._last_error)(self._handle).decode(), rc))

    def _call(self, name, *args):
        """<prefix><name>(handle, *args), checked"""
        self._chk(getattr(lib(), self._prefix + name)(self._handle, *args), name)

    def _configure_integrator(self):
        self._call("set_integrator", self.maxDepth, self.rrDepth, int(self.strictNormals))

    def _film_ctx(self):
        """the context whose film is the frame: a group overrides it"""
        return self._handle

    def preprocess(self, scene, camera, sampler="independent", sampleCount=4, depth=3, seed=0x5EED):
        """Scene::preprocess -> Integrator::preprocess: upload the flattened scene, camera and sampler."""
        self._configure_integrator()
        for call, args in upload_plan(scene):
            self._call(call, *args)
        self.camera = camera
        self._call("set_camera", C.byref(struct_of(camera)))
        kind = self.SAMPLERS[sampler] if isinstance(sampler, str) else int(sampler)
        self._call("set_sampler", kind, int(sampleCount), int(depth), int(seed))
        return True

    def set_rfilter(self, kind="box", halfSize=-1.0, stddev=-1.0, B=-1.0, C=-1.0, cycles=-1.0):
        """Film reconstruction filter plugin (src/rfilters/{box,gaussian,mitchell,catmullrom,wsinc}.cpp); negative
        values select the plugin defaults"""
        if kind == "box":
            self._call("set_rfilter", 0.5, 0.5, None)
            return
        size = np.zeros(2, dtype=np.float32); values = np.zeros(256, dtype=np.float32)
        k = self.FILTERS[kind]
        p0, p1 = {1: (stddev, -1.0), 2: (B, C), 3: (-1.0, -1.0), 4: (cycles, -1.0)}[k]
        check(lib().mtsgpu_tabulate_filter(k, halfSize, p0, p1, abi.ptr(size, abi.f32p), abi.ptr(values, abi.f32p)), "mtsgpu_tabulate_filter")
        self._call("set_rfilter", float(size[0]), float(size[1]), abi.ptr(values, abi.f32p))
        return size, values.reshape(16, 16)

    def set_tuning(self, **knobs):
        """scheduling knobs of the traversal kernel (mtsgpu_set_tuning; a group: on every member, and its own test knob
        rccl_fail); results never depend on them"""
        for k, v in knobs.items():
            self._call("set_tuning", k.encode(), int(v))

    def cancel(self):
        self._cancel.value = 1

    def film(self):
        """[H][W][5] float32: spectrum rgb sum, alpha sum, weight sum (ImageBlock layout)"""
        cam, ctx = struct_of(self.camera), self._film_ctx()
        out = np.zeros((cam.height, cam.width, 5), dtype=np.float32)
        _chk_ctx(ctx, lib().mtsgpu_read_film(ctx, abi.ptr(out, abi.f32p)), "read_film")
        return out

    # --- test-case mode (`mitsuba -t`, testmode.py) -----------------------------
    def set_film_statistics(self, on=True):
        """ImageBlocks with statistics (renderproc.cpp:44-50): render() also runs the per-pixel variance recurrence of
        SampleIntegrator::renderBlock (integrator.cpp:171-202).  Box filter only, as in the reference.  A group: on every
        member; member 0 holds the merged statistics after render()"""
        self._call("set_film_statistics", int(bool(on)))

    def film_statistics(self):
        """(variance [H][W][3] float32, nSamples [H][W] uint32) of the last render; pixels not rendered hold 0, 0"""
        cam, ctx = struct_of(self.camera), self._film_ctx()
        var = np.zeros((cam.height, cam.width, 3), dtype=np.float32)
        n = np.zeros((cam.height, cam.width), dtype=np.uint32)
        _chk_ctx(ctx, lib().mtsgpu_read_film_statistics(ctx, abi.ptr(var, abi.f32p), abi.ptr(n, abi.u32p)), "read_film_statistics")
        return var, n

    def close(self):
        if self._handle and binding._lib is not None:
            getattr(binding._lib, self._destroy)(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _uv_args(vtx_uv, shape_has_uv, textures, bsdf_slot_texture):
    """the five arguments of mtsgpu_set_uv_textures from arrays and texture objects, None for NULL"""
    t = None if textures is None else uv_texture_array(textures)
    return (abi.ptr(_or_none(vtx_uv, np.float32), abi.f32p), abi.ptr(_or_none(shape_has_uv, np.uint32), abi.u32p), 0 if t is None else len(t), t,
            abi.ptr(_or_none(bsdf_slot_texture, np.int32), abi.i32p))


def _bitmap_args(textures, bitmaps, texture_bitmap):
    """the three arguments mtsgpu_set_uv_bitmap_textures adds; bitmaps and texture_bitmap both None: derived from `textures`"""
    if bitmaps is None and texture_bitmap is None and textures is not None:
        bitmaps, texture_bitmap = bitmap_table(textures)
    bm = None if not bitmaps else bitmap_array(bitmaps)
    return (0 if bm is None else len(bitmaps), bm, abi.ptr(_or_none(texture_bitmap, np.int32), abi.i32p))


class MIPathTracer(Driver, ReadOuts):
    """The `path` integrator (MIPathTracer : MonteCarloIntegrator) on one MI355X.

    Properties as in src/librender/integrator.cpp:272-292: maxDepth (-1 = unbounded),
    rrDepth (10), strictNormals (false).  The call order mirrors the host's:
    configure() -> preprocess(scene, camera, sampler...) -> render() [-> cancel()]."""
    _prefix, _last_error, _destroy = "mtsgpu_", "mtsgpu_last_error", "mtsgpu_destroy"
    _ctx = property(lambda self: self._handle)      # the handle under the name the tests and tools know

    def __init__(self, maxDepth=-1, rrDepth=10, strictNormals=False, device=0):
        self.maxDepth, self.rrDepth, self.strictNormals = int(maxDepth), int(rrDepth), bool(strictNormals)
        self._handle = C.c_void_p()
        self._cancel = C.c_int(0)
        self._film_keep = None
        check(lib().mtsgpu_create(int(device), C.byref(self._handle)), "mtsgpu_create")
        self.camera = None

    def configure(self):
        self._configure_integrator()
        return self

    def set_tiles(self, block_size=32, part=0, n_parts=1):
        self._call("set_tiles", block_size, part, n_parts)

    def set_film_edges(self, highQualityEdges=False):
        """Film property `highQualityEdges` (src/librender/film.cpp:51, renderproc.cpp:146-153)"""
        self._call("set_film_edges", int(bool(highQualityEdges)))

    def set_options(self, max_paths=0, count_traversal=False, time_kernels=False):
        self._call("set_options", int(max_paths), int(count_traversal), int(time_kernels))

    def set_stream(self, hip_stream):
        self._call("set_stream", C.c_void_p(hip_stream))

    def set_film_buffer(self, device_ptr, keepalive=None):
        self._film_keep = keepalive
        self._call("set_film_buffer", C.c_void_p(device_ptr))

    def clear_film(self):
        self._call("clear_film")

    def render(self):
        """SampleIntegrator::render: returns True, or False when cancelled (integrator.cpp:87-120)."""
        self._cancel.value = 0
        rc = lib().mtsgpu_render(self._ctx, C.byref(self._cancel))
        if rc == -4:
            return False
        self._chk(rc, "render")
        return True

    def sync(self):
        self._call("sync")

    def stats(self):
        st = abi.Stats()
        self._call("get_stats", C.byref(st))
        d = st.as_dict()
        redone = C.c_uint64(0)      # not a field of mtsgpu_stats, whose layout is part of ABI version 8
        self._call("hook_rays_redone", C.byref(redone))
        d["rays_redone"] = int(redone.value)
        return d

    def bin_entries(self):
        """entries the closest-hit launches of the last frame appended to every material queue (mtsgpu_bin_entries): one count per
        BSDF type, then the terminal queue"""
        out = (C.c_uint64 * (abi.BSDF_NTYPES + 1))()
        self._call("bin_entries", out)
        return [int(v) for v in out]

    def film_statistics_form(self):
        """the form of the variance kernel the last pass ran: "lane", "wave" or None"""
        return {0: "lane", 1: "wave"}.get(lib().mtsgpu_film_statistics_form(self._ctx))

    # --- the tables of the uploaded scene, set by hand ---------------------------
    def upload_scene_tangents(self, scene, vtx_dpdu=None, shape_has_tangents=None):
        """mtsgpu_upload_scene_tangents with explicit arrays: vtx_dpdu [n_verts][3], shape_has_tangents [n_shapes] (both None =
        none); clears vertex colours and uv textures like every upload"""
        self._call("upload_scene_tangents", scene.ptr if isinstance(scene, Scene) else scene, abi.ptr(_or_none(vtx_dpdu, np.float32), abi.f32p),
                   abi.ptr(_or_none(shape_has_tangents, np.uint32), abi.u32p))

    def set_vertex_colors(self, vtx_col=None, shape_has_colors=None, bsdf_color_slots=None):
        """mtsgpu_set_vertex_colors on the uploaded scene: the colour pool [n_verts][3], one flag per shape, one slot mask
        per BSDF; all None switches the colours off"""
        self._call("set_vertex_colors", abi.ptr(_or_none(vtx_col, np.float32), abi.f32p), abi.ptr(_or_none(shape_has_colors, np.uint32), abi.u32p),
                   abi.ptr(_or_none(bsdf_color_slots, np.uint32), abi.u32p))

    def set_uv_textures(self, vtx_uv=None, shape_has_uv=None, textures=None, bsdf_slot_texture=None):
        """mtsgpu_set_uv_textures on the uploaded scene: the texcoord pool [n_verts][2], one flag per shape, the textures
        (scenes.Checkerboard / GridTexture objects or abi.UvTexture), the table [n_bsdfs][2]; all None switches them off"""
        self._call("set_uv_textures", *_uv_args(vtx_uv, shape_has_uv, textures, bsdf_slot_texture))

    def set_uv_bitmap_textures(self, vtx_uv=None, shape_has_uv=None, textures=None, bsdf_slot_texture=None, bitmaps=None, texture_bitmap=None):
        """mtsgpu_set_uv_bitmap_textures on the uploaded scene: set_uv_textures() with bitmaps (scenes.BitmapTexture objects or
        abi.Bitmap) and the bitmap index per texture.  With bitmaps and texture_bitmap both None they are derived from the
        BitmapTexture objects among `textures` (none: n_bitmaps = 0)"""
        self._call("set_uv_bitmap_textures", *_uv_args(vtx_uv, shape_has_uv, textures, bsdf_slot_texture),
                   *_bitmap_args(textures, bitmaps, texture_bitmap))

    def set_uv_masked_textures(self, vtx_uv=None, shape_has_uv=None, textures=None, bsdf_slot_texture=None, bitmaps=None, texture_bitmap=None,
                               bsdf_mask=None):
        """mtsgpu_set_uv_masked_textures on the uploaded scene: set_uv_bitmap_textures() with one mask per BSDF, rows (kind,
        texture, opacity rgb) or abi.BsdfMask; all None switches masks and textures off"""
        self._call("set_uv_masked_textures", *_uv_args(vtx_uv, shape_has_uv, textures, bsdf_slot_texture),
                   *_bitmap_args(textures, bitmaps, texture_bitmap), None if bsdf_mask is None else bsdf_mask_array(bsdf_mask))

    def set_snow_bsdfs(self, table=None):
        """mtsgpu_set_snow_bsdfs on the uploaded scene: one abi.BsdfSnow, row (kind, derived) or None per BSDF; None switches the
        table off"""
        self._call("set_snow_bsdfs", None if table is None else bsdf_snow_array(table))

    def set_cloth_bsdfs(self, weaves=None, bsdf_weave=None):
        """mtsgpu_set_cloth_bsdfs on the uploaded scene: scenes.Weave objects and one weave index (or -1) per BSDF; None switches
        the table off"""
        if bsdf_weave is None:
            self._call("set_cloth_bsdfs", 0, None, None)
            return
        arr, keep = weave_array(list(weaves or []))
        self._call("set_cloth_bsdfs", len(weaves or []), arr, abi.ptr(np.ascontiguousarray(bsdf_weave, dtype=np.int32), abi.i32p))

    def set_spot_textures(self, textures=None, texture_bilinear=None, lum_texture=None):
        """mtsgpu_set_spot_textures on the uploaded scene: scenes texture objects, one filter flag per texture and one texture index
        (or -1) per luminaire; all None switches the projection textures off"""
        if textures is None and lum_texture is None:
            self._call("set_spot_textures", 0, None, 0, None, None, None, None)
            return
        textures = list(textures or [])
        sb, stb = bitmap_table(textures)
        self._call("set_spot_textures", len(textures), uv_texture_array(textures) if textures else None, len(sb), bitmap_array(sb) if sb else None,
                   abi.ptr(stb, abi.i32p) if sb else None, abi.ptr(_or_none(texture_bilinear, np.uint32), abi.u32p),
                   abi.ptr(np.ascontiguousarray(lum_texture, dtype=np.int32), abi.i32p))


class MIDirectIntegrator(MIPathTracer):
    """The `direct` integrator (src/integrators/direct/direct.cpp); more than one sample per strategy needs a sampler
    with sample arrays (independent, ldsampler, stratified), as in the reference"""

    def __init__(self, luminaireSamples=1, bsdfSamples=1, device=0):
        MIPathTracer.__init__(self, device=device)
        self.luminaireSamples, self.bsdfSamples = int(luminaireSamples), int(bsdfSamples)

    def _configure_integrator(self):
        self._call("set_direct_integrator", self.luminaireSamples, self.bsdfSamples)


class DeviceGroup(Driver):
    """Several GPUs behind one host process (mtsgpu_create_multi): what the Mitsuba plugin uses, since Scene::render
    calls Integrator::render once (src/librender/scene.cpp:356-359).  devices may repeat (two contexts on one GPU)."""
    _prefix, _last_error, _destroy = "mtsgpu_group_", "mtsgpu_group_last_error", "mtsgpu_group_destroy"
    _g = property(lambda self: self._handle)        # the handle under the name the tests know

    def __init__(self, devices, maxDepth=-1, rrDepth=10, strictNormals=False):
        self.maxDepth, self.rrDepth, self.strictNormals = int(maxDepth), int(rrDepth), bool(strictNormals)
        self._handle = C.c_void_p()
        self._cancel = C.c_int(0)
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        check(lib().mtsgpu_create_multi(len(devices), devs, C.byref(self._handle)), "mtsgpu_create_multi")
        self.camera = None

    def _film_ctx(self):
        return self.member(0)

    def __len__(self):
        return lib().mtsgpu_group_size(self._g)

    def member(self, i):
        return lib().mtsgpu_group_ctx(self._g, int(i))

    def render(self, block_size=32, ordered_reduce=False):
        """ordered_reduce: False / 0 = RCCL when possible, True / 1 = the ordered peer-copy sum, 2 = RCCL must initialise"""
        self._cancel.value = 0
        rc = lib().mtsgpu_group_render(self._g, int(block_size), int(ordered_reduce), C.byref(self._cancel))
        if rc == -4:
            return False
        self._chk(rc, "group_render")
        return True

    def reduce_kind(self):
        return {0: "ordered peer-copy sum", 1: "rccl ncclReduce"}.get(lib().mtsgpu_group_last_reduce_kind(self._g))

    def rccl_ranks(self):
        """ranks of the group's RCCL communicator once it has passed its self-check, else 0"""
        return int(lib().mtsgpu_group_rccl_ranks(self._g))

    def reduce_note(self):
        """why the last render fell back to the ordered sum ("" when it did not)"""
        return lib().mtsgpu_group_reduce_note(self._g).decode()

    def member_pass_samples(self, i, first=0, n=None):
        """pass_samples() of member i, read through mtsgpu_group_ctx"""
        return read_pass_samples(self.member(i), first, self.member_stats(i)["camera_samples"] - int(first) if n is None else n)

    def member_stats(self, i):
        st = abi.Stats()
        lib().mtsgpu_get_stats(self.member(i), C.byref(st))
        return st.as_dict()


def develop(film):
    """Film::develop: pixel = spectrum * (1 / weight) (src/films/mfilm.cpp:108-116)"""
    w = film[..., 4:5]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(w > 0, np.float32(1.0) / w, np.float32(0)).astype(np.float32)
    return (film[..., :3] * inv).astype(np.float32)
