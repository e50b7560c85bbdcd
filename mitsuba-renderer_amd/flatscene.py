"""Scene: a description flattened by the library, the tables that travel next to it, and upload_plan() -- the one statement
of which calls hand a scene to a context, in which order.  With it the ctypes arrays those calls take, and what feeds a
description: load_serialized() and snow_configure()."""
import ctypes as C
import os

import numpy as np

from . import abi, binding, scenes
from .binding import check, lib


def load_serialized(path, shape_index=0, bsdf=-1, lum=-1, name=None):
    """<shape type="serialized"> (TriMesh::TriMesh(Stream *, int), src/librender/trimesh.cpp:156-236) -> MeshDesc"""
    h = C.c_void_p(); m = abi.Mesh()
    check(lib().mtsgpu_load_serialized(os.fsencode(path), int(shape_index), C.byref(h), C.byref(m)), "mtsgpu_load_serialized")
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
    check(call(abi.ptr(r, abi.f32p), C.byref(out)), "snow_configure")
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


def uv_texture_array(textures):
    """a ctypes array of mtsgpu_uv_texture from scenes.Checkerboard / GridTexture objects (or abi.UvTexture values)"""
    items = [t if isinstance(t, abi.UvTexture) else t.descriptor() for t in textures]
    return (abi.UvTexture * max(len(items), 1))(*items) if items else (abi.UvTexture * 1)()


def bitmap_array(bitmaps):
    """a ctypes array of mtsgpu_bitmap from scenes.BitmapTexture objects (or abi.Bitmap values)"""
    items = [b if isinstance(b, abi.Bitmap) else b.bitmap() for b in bitmaps]
    return (abi.Bitmap * max(len(items), 1))(*items) if items else (abi.Bitmap * 1)()


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
        meshes = description.meshes
        kp = kd_params if kd_params is not None else abi.KdParams()
        kp.gpu_binning = (kp.gpu_binning & ~3) | (1 if gpu_binning else 0) | (2 if gpu_exact else 0)
        # the _tangents calls only when a mesh with texcoords has an anisotropic BSDF (TriMesh::configure asks for tangents
        # then, trimesh.cpp:288-290); every other scene goes through the calls it always went through
        self.wants_tangents = any(m.shape_type == abi.SHAPE_TRIMESH and getattr(m, "texcoords", None) is not None and m.bsdf >= 0
                                  and (description.bsdf_is_anisotropic(m.bsdf) or m.bsdf in getattr(description, "bsdf_weave", {}))
                                  for m in meshes)
        # the cloth BSDFs of the scene (none: the scene never calls mtsgpu_set_cloth_bsdfs): IrawanClothBRDF is EAnisotropic and its
        # Lambertian entry is not, so its entries are flagged for the flattener
        self.cloth = None
        if getattr(description, "bsdf_weave", None):
            self.cloth = weave_array(description.weaves) + (description.weave_table(),)
        flags = None if self.cloth is None else np.ascontiguousarray(self.cloth[2] >= 0, dtype=np.uint32)
        tcs = (abi.f32p * max(len(meshes), 1))()       # per mesh its texcoords, NULL without
        for i, m in enumerate(meshes):
            if m.shape_type == abi.SHAPE_TRIMESH and getattr(m, "texcoords", None) is not None:
                tcs[i] = abi.ptr(m.texcoords, abi.f32p)
        # a description with a cylinder goes through the cylinder calls (include/mtsgpu_cylinder.h), every other one through
        # the calls it always went through
        self.has_cylinders = any(m.shape_type == abi.SHAPE_CYLINDER for m in meshes)
        desc, h = C.byref(self._desc), C.byref(self._h)
        if self.has_cylinders:
            cyl = (abi.Cylinder * max(len(meshes), 1))()
            for i, m in enumerate(meshes):
                if m.shape_type == abi.SHAPE_CYLINDER:
                    cyl[i] = m.to_struct()
            rc = lib().mtsgpu_flatten_cylinders(desc, C.byref(kp), tcs, abi.ptr(flags, abi.u32p), cyl, h)
        elif self.wants_tangents and flags is not None:
            rc = lib().mtsgpu_flatten_tangents_flagged(desc, C.byref(kp), tcs, abi.ptr(flags, abi.u32p), h)
        elif self.wants_tangents:
            rc = lib().mtsgpu_flatten_tangents(desc, C.byref(kp), tcs, h)
        else:
            rc = lib().mtsgpu_flatten(desc, C.byref(kp), h)
        check(rc, "mtsgpu_flatten")
        self.ptr = lib().mtsgpu_flat_scene_get(self._h)
        # per-vertex colours go into the flat scene's own pool; the slot masks of the BSDFs travel next to the blocks
        for i, m in enumerate(meshes):
            if getattr(m, "colors", None) is not None:
                check(lib().mtsgpu_flat_scene_set_mesh_colors(self._h, i, abi.ptr(m.colors, abi.f32p)), "mtsgpu_flat_scene_set_mesh_colors")
        slots = np.asarray(getattr(description, "bsdf_color_slots", []), dtype=np.uint32)
        self.bsdf_color_slots = slots if slots.any() else None
        # likewise the texture coordinates, the uv textures and the table that names one per BSDF slot
        for i, m in enumerate(meshes):
            if getattr(m, "texcoords", None) is not None:
                check(lib().mtsgpu_flat_scene_set_mesh_texcoords(self._h, i, abi.ptr(m.texcoords, abi.f32p)), "mtsgpu_flat_scene_set_mesh_texcoords")
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

    def upload_plan(self):
        """the upload of this scene: the ordered list of (call, args), call being the C name without its mtsgpu_ /
        mtsgpu_group_ prefix and args everything after the handle.  One of the three upload calls; then colours, one of the
        three texture calls, snow, cloth (behind a texture call without textures when none has handed the texcoords over),
        spot textures -- the order csrc/scene_attach.cpp insists on"""
        ta, cb = self.tangent_args(), self.cylinder_blocks()
        self._plan_keep = (ta, cb)          # the pointers below point into these
        if cb is not None:
            ta = ta if ta is not None else (None, None)
            plan = [("upload_scene_cylinders", (self.ptr, abi.ptr(ta[0], abi.f32p), abi.ptr(ta[1], abi.u32p), abi.ptr(cb, abi.f32p)))]
        elif ta is not None:
            plan = [("upload_scene_tangents", (self.ptr, abi.ptr(ta[0], abi.f32p), abi.ptr(ta[1], abi.u32p)))]
        else:
            plan = [("upload_scene", (self.ptr,))]
        vc = self.vertex_color_args()
        if vc is not None:
            plan.append(("set_vertex_colors", vc))
        textures = [(call, args) for call, args in (("set_uv_masked_textures", self.uv_masked_texture_args()),
                                                    ("set_uv_bitmap_textures", self.uv_bitmap_texture_args()),
                                                    ("set_uv_textures", self.uv_texture_args())) if args is not None]
        plan += textures[:1]
        if self.bsdf_snow is not None:
            plan.append(("set_snow_bsdfs", (self.bsdf_snow,)))
        if self.cloth is not None:
            if not textures:
                plan.append(("set_uv_textures", self.uv_only_args()))
            plan.append(("set_cloth_bsdfs", (len(self.description.weaves), self.cloth[0], abi.ptr(self.cloth[2], abi.i32p))))
        sx = self.spot_texture_args()
        if sx is not None:
            plan.append(("set_spot_textures", sx))
        return plan

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

    def _uv_pool(self):
        """(vtx_uv, shape_has_uv) pointers of the flat scene, None where no mesh has texcoords"""
        uv = lib().mtsgpu_flat_scene_vertex_texcoords(self._h)
        has = lib().mtsgpu_flat_scene_shape_has_texcoords(self._h)
        return (uv if uv else None, has if has else None)

    def uv_texture_args(self):
        """what mtsgpu_set_uv_textures takes for this scene: (vtx_uv, shape_has_uv, n_textures, textures, bsdf_slot_texture),
        or None when no BSDF slot of the scene has a uv texture"""
        if self.bsdf_slot_texture is None:
            return None
        return self._uv_pool() + (len(self.textures), self.textures, abi.ptr(self.bsdf_slot_texture, abi.i32p))

    def uv_only_args(self):
        """what mtsgpu_set_uv_textures takes to hand over the texcoords alone (a cloth scene without a uv texture)"""
        uv, has = self._uv_pool()
        if uv is None:      # no mesh has texcoords (spheres only): a zero pool, so that the call keeps a uv array
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
        nb, nt = len(self._bitmap_objects), len(getattr(self.description, "textures", []))
        return self._uv_pool() + (nt, self.textures if nt else None, abi.ptr(self.bsdf_slot_texture, abi.i32p), nb,
                                  self.bitmaps if nb else None, abi.ptr(self.texture_bitmap, abi.i32p) if nb else None, self.bsdf_mask)

    def _pool(self, pool, flags, width):
        """(pool [n_verts][width] float32, flags [n_shapes] uint32) behind two pointers of the flat scene, or (None, None)"""
        p = pool(self._h)
        if not p:
            return None, None
        return abi.np_from(p, (self.sc.n_verts, width), np.float32), abi.np_from(flags(self._h), (self.sc.n_shapes,), np.uint32)

    def vertex_tangents(self):
        """(pool [n_verts][6] float32 = dpdu, dpdv; flags [n_shapes] uint32) of the flat scene, or (None, None) when no mesh has
        tangents (mtsgpu_flat_scene_vertex_tangents)"""
        return self._pool(lib().mtsgpu_flat_scene_vertex_tangents, lib().mtsgpu_flat_scene_shape_has_tangents, 6)

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
        return self._pool(lib().mtsgpu_flat_scene_vertex_texcoords, lib().mtsgpu_flat_scene_shape_has_texcoords, 2)

    def vertex_colors(self):
        """(pool [n_verts][3] float32, flags [n_shapes] uint32) of the flat scene, or (None, None)"""
        return self._pool(lib().mtsgpu_flat_scene_vertex_colors, lib().mtsgpu_flat_scene_shape_has_colors, 3)

    def arrays(self):
        return abi.scene_arrays(self.sc)

    def kdstats(self):
        out = (C.c_double * 6)()
        lib().mtsgpu_flat_scene_kdstats(self._h, out)
        return dict(zip(["inner", "leaf", "indices", "exp_traversals", "exp_leaves", "exp_prims"], list(out)))

    def __del__(self):
        h = getattr(self, "_h", None)
        if h and binding._lib is not None:
            binding._lib.mtsgpu_flat_scene_free(h)
            self._h = None


def upload_plan(scene):
    """Scene.upload_plan(), or the one call a bare abi.Scene pointer in place of a Scene consists of"""
    return scene.upload_plan() if isinstance(scene, Scene) else [("upload_scene", (scene,))]
