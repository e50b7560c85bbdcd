"""Read-outs for tests and measurements: device functions and host-side steps of the library, called one at a time.

ReadOuts is the mixin MIPathTracer inherits: each method borrows the context to run one device function on query records.
The functions below it need no context."""
import ctypes as C

import numpy as np

from . import abi
from .binding import MtsGpuError, check, lib
from .flatscene import bitmap_array, bitmap_table, bsdf_snow_array, uv_texture_array, weave_array


def _fp(a):
    return abi.ptr(a, abi.f32p)


def _up(a):
    return abi.ptr(a, abi.u32p)


def _queries(wi, aux, uv=None, params=None):
    """(n, q, out, P) of a bsdf_eval* call: the query records q [n][6] = wi, aux -- [n][8] with uv behind them --, the
    results out [n][8], and params padded to BSDF_NPARAMS (None without params)"""
    aux = np.atleast_2d(np.asarray(aux, dtype=np.float32))
    n = aux.shape[0]
    q = np.zeros((n, 6 if uv is None else 8), dtype=np.float32)
    q[:, :3] = np.asarray(wi, dtype=np.float32).reshape(-1, 3)
    q[:, 3:3 + aux.shape[1]] = aux
    if uv is not None:
        q[:, 6:8] = np.asarray(uv, dtype=np.float32).reshape(-1, 2)
    P = None
    if params is not None:
        P = np.zeros(abi.BSDF_NPARAMS, dtype=np.float32); P[:len(params)] = params
    return n, q, np.zeros((n, 8), dtype=np.float32), P


def _records(prim, rec, width, out_width):
    """(p, q, out) of a call on records (primitive, rec [width]) of the uploaded scene"""
    p = np.ascontiguousarray(prim, dtype=np.uint32).reshape(-1)
    return p, np.ascontiguousarray(rec, dtype=np.float32).reshape(-1, width), np.zeros((len(p), out_width), dtype=np.float32)


def read_pass_samples(ctx, first, n):
    out = np.zeros((int(n), 8), dtype=np.float32)
    rc = lib().mtsgpu_pass_samples(ctx, int(first), int(n), _fp(out))
    if rc != 0:
        raise MtsGpuError("pass_samples: %s (code %d)" % (lib().mtsgpu_last_error(ctx).decode(), rc))
    return out


class ReadOuts:
    """kernels exposed for parity tests; _call(name, *args) is the driver's: mtsgpu_<name>(context, *args), checked"""

    def trace_rays(self, rays, shadow=False):
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 8)
        hits = np.zeros((r.shape[0], 4), dtype=np.uint32)
        self._call("trace_rays", _fp(r), r.shape[0], int(shadow), _up(hits))
        return hits

    REPLAY_KINDS = {"deep": 0, "camera": 1, "shadow": 2}

    def replay_roof(self, n, stride=1, reps=3, kind="deep"):
        """mtsgpu_replay_roof: the request stream of n rays of the frame rendered last replayed without arithmetic, next to
        the product kernel on the same rays.  kind: "deep" = the last ray of every stride-th path (closest-hit kernel),
        "camera" = the camera rays of the last pass, generated again (closest-hit kernel, first-bounce launch shape),
        "shadow" = every stride-th slot of the shadow queue (any-hit kernel)"""
        out = (C.c_double * 12)()
        self._call("replay_roof", self.REPLAY_KINDS[kind], int(n), int(stride), int(reps), out)
        keys = ["rays", "requests", "truncated_rays", "product_ms", "replay_ms", "pair_global", "pair_lds", "node_global", "node_lds",
                "heads", "tails", "spills"]
        return dict(zip(keys, list(out)))

    def ld_tables(self, pixel_key, spp, depth):
        t1 = np.zeros((depth, spp), dtype=np.float32)
        t2 = np.zeros((depth, spp, 2), dtype=np.float32)
        self._call("ld_tables", int(pixel_key), _fp(t1), _fp(t2))
        return t1, t2

    def sampler_values(self, pixel_key, sample_index, n, two_d=False):
        """generate() for the pixel, then n x next1D() (or next2D()) of camera sample `sample_index`, on the device"""
        out = np.zeros((n, 2) if two_d else (n,), dtype=np.float32)
        self._call("sampler_values", int(pixel_key), int(sample_index), int(n), int(bool(two_d)), _fp(out))
        return out

    def random_values(self, op, n, seed=0, arg=0, clone=0):
        """the reference's Random (MT19937-64) on the device: op 0 nextULong, 1 nextFloat bits, 2 nextSize(arg), 3 shuffle(0..n-1)"""
        out = np.zeros(n, dtype=np.uint64)
        self._call("random_values", int(op), int(seed), int(arg), int(clone), int(n), out.ctypes.data_as(C.POINTER(C.c_uint64)))
        return out

    def bsdf_eval(self, bsdf_type, params, op, wi, aux):
        """BSDF::f (op 0), pdf (1), sample(bRec, pdf, sample) (2) on the device for n query records (mtsgpu_bsdf_eval):
        wi [n][3] or [3]; aux = wo [n][3] (op 0, 1) or the 2D sample [n][2] (op 2).  Returns [n][8]."""
        n, q, out, P = _queries(wi, aux, params=params)
        self._call("bsdf_eval", int(bsdf_type), _fp(P), int(op), n, _fp(q), _fp(out))
        return out

    def bsdf_eval_table(self, types, params, index, op, wi, aux):
        """the same read-out for entry `index` of a BSDF table (mtsgpu_bsdf_eval_table): types [n_bsdfs], params
        [n_bsdfs][16] as a scene description holds them; a composite reads its children there"""
        n, q, out, _ = _queries(wi, aux)
        T = np.ascontiguousarray(types, dtype=np.uint32).reshape(-1)
        P = np.ascontiguousarray(params, dtype=np.float32).reshape(len(T), abi.BSDF_NPARAMS)
        self._call("bsdf_eval_table", len(T), _up(T), _fp(P), int(index), int(op), n, _fp(q), _fp(out))
        return out

    def bsdf_eval_snow(self, bsdf_type, entry, op, wi, aux):
        """bsdf_eval() of the snow record `entry`, an abi.BsdfSnow or a row (kind, derived) (mtsgpu_bsdf_eval_snow) -> [n][8]"""
        n, q, out, _ = _queries(wi, aux)
        self._call("bsdf_eval_snow", int(bsdf_type), bsdf_snow_array([entry]), int(op), n, _fp(q), _fp(out))
        return out

    def bsdf_eval_cloth(self, bsdf_type, weave, op, wi, aux, uv):
        """bsdf_eval() of the cloth BRDF with the scenes.Weave `weave` at its.uv = uv (mtsgpu_bsdf_eval_cloth); op 3: the
        internals of f (yarn id, centre x, y, random1, random2, intensityVariation, u, v) -> [n][8]"""
        n, q, out, _ = _queries(wi, aux, uv=uv)
        arr, keep = weave_array([weave])
        self._call("bsdf_eval_cloth", int(bsdf_type), arr, int(op), n, _fp(q), _fp(out))
        return out

    def bsdf_eval_masked(self, bsdf_type, params, opacity, op, wi, aux):
        """bsdf_eval() through the mask adapter whose opacity is the spectrum `opacity` (mtsgpu_bsdf_eval_masked) -> [n][8]"""
        n, q, out, P = _queries(wi, aux, params=params)
        o = np.ascontiguousarray(np.broadcast_to(np.asarray(opacity, dtype=np.float32), (3,)))
        self._call("bsdf_eval_masked", int(bsdf_type), _fp(P), _fp(o), int(op), n, _fp(q), _fp(out))
        return out

    def bsdf_eval_slots(self, bsdf_type, params, source, color, values, op, wi, aux):
        """bsdf_eval() with texture slot s taking nothing (source[s] = 0), `color` (1) or values[s] (2) (mtsgpu_bsdf_eval_slots)
        -> [n][8]"""
        n, q, out, P = _queries(wi, aux, params=params)
        src = np.ascontiguousarray(source, dtype=np.int32).reshape(2)
        col = np.ascontiguousarray(color, dtype=np.float32).reshape(3)
        val = np.ascontiguousarray(values, dtype=np.float32).reshape(6)
        self._call("bsdf_eval_slots", int(bsdf_type), _fp(P), abi.ptr(src, abi.i32p), _fp(col), _fp(val), int(op), n, _fp(q), _fp(out))
        return out

    def bsdf_eval_colored(self, bsdf_type, params, slots, color, op, wi, aux):
        """bsdf_eval() with the texture slots of mask `slots` taking `color` (mtsgpu_bsdf_eval_colored) -> [n][8]"""
        n, q, out, P = _queries(wi, aux, params=params)
        col = np.ascontiguousarray(color, dtype=np.float32).reshape(3)
        self._call("bsdf_eval_colored", int(bsdf_type), _fp(P), int(slots), _fp(col), int(op), n, _fp(q), _fp(out))
        return out

    def bitmap_texture_eval(self, texture, prim, rec, bitmap=None):
        """uv_texture_eval() for a scenes.BitmapTexture (or an abi.UvTexture of kind TEX_BITMAP with an abi.Bitmap)
        (mtsgpu_bitmap_texture_eval) -> [n][5] = uv, rgb"""
        p, q, out = _records(prim, rec, 3, 5)
        self._call("bitmap_texture_eval", uv_texture_array([texture]), bitmap_array([texture if bitmap is None else bitmap]), len(p), _up(p),
                   _fp(q), _fp(out))
        return out

    def uv_texture_eval(self, texture, prim, rec):
        """its.uv and the texture's value on the device for records (primitive, (u, v, -) | world point) of the uploaded scene
        (mtsgpu_uv_texture_eval) -> [n][5] = uv, rgb"""
        p, q, out = _records(prim, rec, 3, 5)
        self._call("uv_texture_eval", uv_texture_array([texture]), len(p), _up(p), _fp(q), _fp(out))
        return out

    def shading_frame_eval(self, prim, rec):
        """the shading frame on the device for records (primitive, (u, v, -) | world point) of the uploaded scene
        (mtsgpu_shading_frame_eval) -> [n][9] = s, t, n"""
        p, q, out = _records(prim, rec, 3, 9)
        self._call("shading_frame_eval", len(p), _up(p), _fp(q), _fp(out))
        return out

    def vertex_color_eval(self, prim, uv):
        """its.color on the device for records (primitive, u, v) of the uploaded scene (mtsgpu_vertex_color_eval) -> [n][3]"""
        p, q, out = _records(prim, uv, 2, 3)
        self._call("vertex_color_eval", len(p), _up(p), _fp(q), _fp(out))
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
        self._call("lum_eval", int(lum_type), _fp(P), int(op), n, _fp(q), _fp(out))
        return out

    def spot_eval(self, block, texture, points, bilinear=False):
        """SpotLuminaire::sample with the projection texture `texture` on the device (mtsgpu_spot_eval) for the spot whose parameter
        block is `block` and points [n][3] -> [n][8] = lRec.d, uv, lRec.value"""
        b = np.ascontiguousarray(block, dtype=np.float32).reshape(abi.LUM_NPARAMS)
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        out = np.zeros((len(p), 8), dtype=np.float32)
        bm = bitmap_array([texture]) if getattr(texture, "kind", None) == abi.TEX_BITMAP else None
        self._call("spot_eval", _fp(b), uv_texture_array([texture]), bm, 1 if bilinear else 0, len(p), _fp(p), _fp(out))
        return out

    def scene_lum_eval(self, op, queries):
        """the luminaires of the uploaded scene on the device (mtsgpu_scene_lum_eval) for query records [n][16]: op 0
        sampleLuminaire(p, s) without the occlusion test, op 1 pdfLuminaire(p, lRec.p, lRec.n, lRec.d, index), op 2 the
        background's Le(direction).  Returns [n][16]: found, index, p, n, d, pdf, value | pdf | Le.rgb"""
        q = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, 16)
        out = np.zeros((q.shape[0], 16), dtype=np.float32)
        self._call("scene_lum_eval", int(op), q.shape[0], _fp(q), _fp(out))
        return out

    def li_samples(self, pix_samples):
        ps = np.ascontiguousarray(pix_samples, dtype=np.uint32).reshape(-1, 3)
        out = np.zeros((ps.shape[0], 8), dtype=np.float32)
        self._call("li_samples", _up(ps), ps.shape[0], _fp(out))
        return out

    def pass_samples(self, first=0, n=None):
        """records first .. first + n of the pass rendered last, as the film kernels read them (mtsgpu_pass_samples): [n][8]
        float32 laid out like li_samples(), the pixel key as a bit pattern in column 7.  n = None: up to the end of the pass
        (camera_samples of the last render when it took one pass)"""
        return read_pass_samples(self._ctx, first, self.stats()["camera_samples"] - int(first) if n is None else n)

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
        self._call("camera_rays", None if ps is None else abi.ptr(ps, abi.i32p), int(first), count, _fp(out))
        return out


def cloth_check(weave, uv_range=None):
    """mtsgpu_cloth_check: what the cloth setter requires of one scenes.Weave, and with uv_range = (uMin, uMax, vMin, vMax) the casts
    of f on such texcoords; raises MtsGpuError with the reason"""
    arr, keep = weave_array([weave])
    r = None if uv_range is None else np.ascontiguousarray(uv_range, dtype=np.float32)
    check(lib().mtsgpu_cloth_check(arr, _fp(r)), "cloth_check")


DEVMATH = dict(sin=0, cos=1, tan=2, exp=3, log=4, atan=5, acos=6, atan2=7, sinh=8, cosh=9, pow15=10)


def devmath(fn, x, y=None):
    """mtsgpu_devmath: the library's elementary function `fn` (a key of DEVMATH) of float32 arguments, on the host"""
    x = np.ascontiguousarray(x, dtype=np.float32).ravel()
    y = None if y is None else np.ascontiguousarray(y, dtype=np.float32).ravel()
    out = np.zeros_like(x)
    check(lib().mtsgpu_devmath(DEVMATH[fn], len(x), _fp(x), _fp(y), _fp(out)), "devmath")
    return out


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
    check(lib().mtsgpu_spot_textures_check(len(lt), _up(lt), _fp(lp), len(textures or []), uv_texture_array(textures) if textures else None,
                                           len(bitmaps or []), bitmap_array(bitmaps) if bitmaps else None, abi.ptr(tb, abi.i32p), _up(fl),
                                           abi.ptr(lx, abi.i32p), int(in_force), _fp(out)), "spot_textures_check")
    return out[:len(lt)]


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
    check(lib().mtsgpu_ldr_texels(bpp, width, height, a.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_float(gamma), _fp(out)), "mtsgpu_ldr_texels")
    return out


def cylinder_configure(cyl):
    """mtsgpu_cylinder_configure of a scenes.CylinderDesc or an abi.Cylinder -> the derived block [28]"""
    c = cyl.to_struct() if hasattr(cyl, "to_struct") else cyl
    out = np.zeros(abi.CYLINDER_NDERIVED, dtype=np.float32)
    check(lib().mtsgpu_cylinder_configure(C.byref(c), _fp(out)), "cylinder_configure")
    return out


def cylinder_aabb(derived):
    """mtsgpu_cylinder_aabb -> [6] = min, max"""
    d = np.ascontiguousarray(derived, dtype=np.float32).reshape(abi.CYLINDER_NDERIVED)
    out = np.zeros(6, dtype=np.float32)
    check(lib().mtsgpu_cylinder_aabb(_fp(d), _fp(out)), "cylinder_aabb")
    return out


def cylinder_clip(derived, boxes, on_device=False):
    """mtsgpu_cylinder_clip: boxes [n][6] -> (clipped [n][6], valid [n])"""
    d = np.ascontiguousarray(derived, dtype=np.float32).reshape(abi.CYLINDER_NDERIVED)
    b = np.ascontiguousarray(boxes, dtype=np.float32).reshape(-1, 6)
    out = np.zeros_like(b); valid = np.zeros(b.shape[0], dtype=np.uint32)
    check(lib().mtsgpu_cylinder_clip(_fp(d), b.shape[0], _fp(b), int(on_device), _fp(out), _up(valid)), "cylinder_clip")
    return out, valid.astype(bool)


def sky_configure(block):
    """SkyLuminaire::configure() for one LUM_SKY block (mtsgpu_sky_configure, host only): zenith x / y / Y, the 3 x 5 Perez
    coefficients (x, y, Y), their three denominators, sin and cos of thetaS"""
    P = np.zeros(abi.LUM_NPARAMS, dtype=np.float32); P[:len(block)] = block
    out = np.zeros(abi.SKY_NDERIVED, dtype=np.float32)
    check(lib().mtsgpu_sky_configure(_fp(P), _fp(out)), "mtsgpu_sky_configure")
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
