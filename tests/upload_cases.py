"""Scenes and case files of tests/upload_harness: the scene list whose device layout tests/golden/upload_layout.json pins, and
the flat binary file the harness reads -- everything preprocess() hands to the upload call and to the setters for a scene,
taken from a mts.Scene on the CPU.  Which calls a case has is read off Scene.upload_plan().  Test infrastructure.

The file: for every section, in any order, u32 length of the name, the name, u64 byte count, the bytes.  A section that is
absent is a NULL pointer of the call.  "hdr" holds the counts (HDR); the rest are the arrays under the names of the C ABI."""
import struct

import numpy as np

HDR = ("abi_version", "n_nodes", "n_indices", "n_tris", "n_verts", "n_shapes", "n_bsdfs", "n_lums", "background_lum", "env_width",
       "env_height", "env_pdf_width", "env_pdf_height", "with_tangents", "accepts_cylinders", "depth_limit", "top_slots",
       "n_textures", "n_bitmaps", "with_bitmaps", "n_weaves")


def layout_scenes(mts):
    """[(name, description)]: the scene list of the layout fixture"""
    import cloth_cases
    import cyl_cases
    import tan_cases
    import test_gpu_cloth
    import test_gpu_mask
    import test_gpu_snow
    S = mts.scenes
    fuzz = S.fuzz(0)
    if all(m.bsdf >= 0 for m in fuzz.meshes):       # a shape without a BSDF: the non-occluder bit of the leaf records
        fuzz.add_sphere((0.1, 0.2, 0.3), 0.05, bsdf=-1)
    return [("cornell_c1", S.cornell_c1()), ("cornell_c3_40_3", S.cornell_c3(grid=40, sphere_subdiv=3)),
            ("cornell_c5_2", S.cornell_c5(sphere_subdiv=2)), ("spheres", S.spheres()), ("fuzz_0", fuzz), ("envlit", S.envlit()),
            ("cornell_tex_sky", S.cornell_tex(sky=True)), ("cyl_mixed", cyl_cases.scene_description(mts, "mixed")),
            ("cyl_cross", cyl_cases.scene_description(mts, "cross")), ("tan_mixed", tan_cases.mixed_scene(mts)),
            ("cornell_vcol", S.cornell_vcol()), ("cornell_bmp", S.cornell_bmp()), ("mask_mixed", test_gpu_mask._mixed(mts, False)),
            ("snow_film", test_gpu_snow._one_film_scene(mts, False)),
            ("cloth_film", test_gpu_cloth._one_film_scene(mts, False, cloth_cases.weaves(mts)))]


def _struct_bytes(arr, n):
    return np.frombuffer(bytes(arr), dtype=np.uint8)[:n * (len(bytes(arr)) // max(len(arr), 1))].copy()


def case_of(mts, scene, depth_limit, top_slots):
    """the sections of one case: {name: numpy array}; "hdr" is a dict until write_case packs it"""
    A = mts.abi
    sc = scene.sc
    a = scene.arrays()
    hdr = dict.fromkeys(HDR, 0)
    hdr.update(abi_version=sc.abi_version, n_nodes=sc.n_nodes, n_indices=sc.n_indices, n_tris=sc.n_tris, n_verts=sc.n_verts, n_shapes=sc.n_shapes,
               n_bsdfs=sc.n_bsdfs, n_lums=sc.n_lums, background_lum=sc.background_lum & 0xFFFFFFFF, env_width=sc.env_width, env_height=sc.env_height,
               env_pdf_width=sc.env_pdf_width, env_pdf_height=sc.env_pdf_height, depth_limit=depth_limit, top_slots=top_slots)
    out = {"hdr": hdr}
    for k in ("kd_nodes", "kd_indices", "triaccel", "tri_idx", "vtx_pos", "vtx_nrm", "shape_tri_offset", "shape_bsdf", "shape_lum", "shape_flags",
              "bsdf_type", "bsdf_params", "lum_type", "lum_params", "lum_shape", "lum_inv_area", "lum_cdf_offset", "lum_tri_cdf", "lum_sel_cdf",
              "lum_sel_pdf"):
        out[k] = a[k]
    if sc.shape_type:
        out["shape_type"], out["shape_params"] = a["shape_type"], a["shape_params"]
    if sc.env_pixels:
        out["env_pixels"], out["env_pdf"], out["env_cdf"] = a["env_pixels"], a["env_pdf"], a["env_cdf"]
    # which calls the scene takes, in which order, is the plan's to say; the arrays are read from the scene
    plan = scene.upload_plan()
    calls = [c for c, _ in plan]
    ta, cb = scene.tangent_args(), scene.cylinder_blocks()
    if calls[0] == "upload_scene_cylinders":
        hdr.update(with_tangents=1, accepts_cylinders=1)
        out["cylinders"] = cb
    if calls[0] == "upload_scene_tangents":
        hdr.update(with_tangents=1)
    if ta is not None and ta[0] is not None:
        out["vtx_dpdu"], out["shape_has_tangents"] = ta
    col, has = scene.vertex_colors()
    if "set_vertex_colors" in calls:
        if col is not None:
            out["vtx_col"], out["shape_has_colors"] = col, has
        if scene.bsdf_color_slots is not None:
            out["bsdf_color_slots"] = scene.bsdf_color_slots
    uv, has = scene.vertex_texcoords()
    tex, args = next(((c, a) for c, a in plan if c in ("set_uv_masked_textures", "set_uv_bitmap_textures", "set_uv_textures")), (None, None))
    if tex == "set_uv_textures" and args[3] is None:
        # no texture call has handed the texcoords over: one without textures, after the snow call
        out["tex_call"] = np.ones(1, dtype=np.uint32)
        out["vtx_uv"], out["shape_has_uv"] = (uv, has) if uv is not None else scene._uv_zero
    elif tex is not None:
        masked, nb = tex == "set_uv_masked_textures", len(scene._bitmap_objects)
        out["tex_call"] = np.zeros(1, dtype=np.uint32)
        if uv is not None:
            out["vtx_uv"], out["shape_has_uv"] = uv, has
        hdr.update(n_textures=args[2], with_bitmaps=int(tex != "set_uv_textures"))
        if not masked or args[2]:
            out["textures"] = _struct_bytes(scene.textures, args[2])
        if scene.bsdf_slot_texture is not None:
            out["bsdf_slot_texture"] = scene.bsdf_slot_texture
        if nb and tex != "set_uv_textures":
            hdr.update(n_bitmaps=nb)
            out["bitmaps"] = np.asarray([[b.width, b.height, b.wrap, 0] for b in scene._bitmap_objects], dtype=np.uint32)
            out["bitmap_texels"] = np.concatenate([np.ascontiguousarray(b.texels, dtype=np.float32).ravel() for b in scene._bitmap_objects])
            out["texture_bitmap"] = scene.texture_bitmap
        if masked:
            out["bsdf_mask"] = _struct_bytes(scene.bsdf_mask, sc.n_bsdfs)
    if "set_snow_bsdfs" in calls:
        out["bsdf_snow"] = _struct_bytes(scene.bsdf_snow, sc.n_bsdfs)
    if "set_cloth_bsdfs" in calls:
        W = scene.description.weaves
        hdr.update(n_weaves=len(W))
        out.update(weave_sections(A, W))
        out["bsdf_weave"] = np.ascontiguousarray(scene.cloth[2], dtype=np.int32)
    return out


def weave_sections(A, weaves):
    """the weaves as the harness reads them: 20 words of scalars and counts each, then all patterns, then all yarns"""
    head, pat, yarns = [], [], []
    for w in weaves:
        row = [np.uint32(getattr(w, n)) if n in ("tileWidth", "tileHeight") else np.float32(getattr(w, n)).view(np.uint32) for n in A.WEAVE_SCALARS]
        head.append(row + [len(w.pattern), len(w.yarns)])
        pat += [int(p) & 0xFFFFFFFF for p in w.pattern]
        for y in w.yarns:
            yarns.append(bytes(A.Yarn(int(y.type), float(y.psi), float(y.umax), float(y.kappa), float(y.width), float(y.length), float(y.centerU),
                                      float(y.centerV), (A.C.c_float * 3)(*[float(x) for x in y.kd]), (A.C.c_float * 3)(*[float(x) for x in y.ks]))))
    return {"weaves": np.asarray(head, dtype=np.uint32).reshape(-1, 20), "weave_patterns": np.asarray(pat, dtype=np.uint32),
            "weave_yarns": np.frombuffer(b"".join(yarns), dtype=np.uint32).copy()}


def write_case(path, case):
    with open(path, "wb") as fh:
        for name, arr in case.items():
            if arr is None:
                continue
            if name == "hdr":
                arr = np.asarray([int(arr[k]) & 0xFFFFFFFF for k in HDR], dtype=np.uint32)
            data = np.ascontiguousarray(arr).tobytes()
            fh.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<Q", len(data)) + data)
