// scene_attach.cpp -- what comes and goes between two uploads (ctx.h: one record per family): vertex colours, uv textures with
// bitmaps and masks, snow records, cloth weaves, the projection textures of spot luminaires.  Every setter has one shape: the shared prologue, the family's clear(), the pure
// checks and plan (host.h: claimRefusal, planTextures, planCloth; scene_layout.cpp), then upload and commit.  A refused call
// leaves its family switched off.
#include "ctx.h"
#include <cmath>
#include <cstring>

using namespace mg;

// the slot tables of the host (host.h) and of the kernels (kernels.h) are one table
constexpr bool colorSlotTablesAgree() {
	for (int t = 0; t < MTSGPU_BSDF_NTYPES; ++t)
		for (int k = 0; k < 2; ++k)
			if (kBsdfColorSlotOffset[t][k] != bsdf_color_slot_offset(t, k)) return false;
	return true;
}
static_assert(colorSlotTablesAgree(), "BSDF colour slot tables differ");
static_assert(sizeof(mtsgpu_bsdf_mask) == sizeof(DMask) && offsetof(mtsgpu_bsdf_mask, opacity) == offsetof(DMask, opacity)
              && offsetof(mtsgpu_bsdf_mask, texture) == offsetof(DMask, texture), "mtsgpu_bsdf_mask and DMask are one layout");
static_assert(MTSGPU_MASK_NONE == (int) kMaskNone && MTSGPU_MASK_CONSTANT == (int) kMaskConstant && MTSGPU_MASK_TEXTURE == (int) kMaskTexture,
              "mask kinds differ");
static_assert(sizeof(mtsgpu_bsdf_snow) == 64 && sizeof(mtsgpu_bsdf_snow) == sizeof(DSnow) && offsetof(mtsgpu_bsdf_snow, derived) == offsetof(DSnow, derived)
              && offsetof(mtsgpu_bsdf_snow, derived) == 8, "mtsgpu_bsdf_snow and DSnow are one layout");
static_assert(MTSGPU_SNOW_NONE == (int) kSnowNone && MTSGPU_SNOW_WISCOMBE == (int) kSnowWiscombe && MTSGPU_SNOW_HK == (int) kSnowHK, "snow kinds differ");

// The prologue of every setter `me`: a context with a scene, then -- unless `early`, what the call refuses before anything is
// freed, says otherwise -- no pass to replay, the context's device, and nothing still reading the arrays that go (the shading
// launches of a render that was not synchronised).  The caller's next line is its family's clear().
template <typename Early> static int beginAttach(mtsgpu_ctx *c, const char *me, Early early) {
	if (!c) return fail(c, MTSGPU_EINVAL, "null argument");
	if (!c->haveScene) return fail(c, MTSGPU_ESTATE, "%s before mtsgpu_upload_scene", me);
	const std::string why = early();
	if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
	c->lastPass.valid = false;
	HIPCHK(c, hipSetDevice(c->device));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
	return 0;
}
static int beginAttach(mtsgpu_ctx *c, const char *me) { return beginAttach(c, me, [] { return std::string(); }); }

extern "C" {

int mtsgpu_set_vertex_colors(mtsgpu_ctx *c, const float *vtx_col, const uint32_t *shape_has_colors, const uint32_t *bsdf_color_slots) {
	if (int rc = beginAttach(c, "mtsgpu_set_vertex_colors")) return rc;
	c->colors.clear();
	if (!vtx_col && !shape_has_colors && !bsdf_color_slots) return 0;
	if ((vtx_col == nullptr) != (shape_has_colors == nullptr))
		return fail(c, MTSGPU_EINVAL, "vtx_col and shape_has_colors must both be given or both be NULL");
	const HostScene &h = c->host;
	const InForce in = c->inForce();
	const uint32_t nShapes = (uint32_t) h.shapeBsdf.size(), nBsdfs = (uint32_t) h.bsdfType.size();
	bool anySlot = false;
	if (bsdf_color_slots) {
		std::string why = checkBsdfColorSlots(nBsdfs, h.bsdfType.data(), h.bsdfParams.data(), bsdf_color_slots);
		for (uint32_t holder : { kFamTextures, kFamSnow, kFamCloth })      // a slot or an entry one of the other calls has taken
			for (uint32_t b = 0; b < nBsdfs && why.empty(); ++b) why = claimRefusal(kFamColors, b, bsdf_color_slots[b], in, holder);
		if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
		for (uint32_t s = 0; s < nShapes; ++s) {
			const int32_t b = h.shapeBsdf[s];
			if (b < 0 || !bsdf_color_slots[b]) continue;
			if (h.shapeType[s] != MTSGPU_SHAPE_TRIMESH)
				return fail(c, MTSGPU_EINVAL, "shape %u: BSDF %d takes vertex colours, but a sphere has none (its.color would be read unwritten, shape.h:162-163)", s, b);
			if (!shape_has_colors || !shape_has_colors[s])
				return fail(c, MTSGPU_EINVAL, "shape %u: BSDF %d takes vertex colours, but the mesh has none (its.color would be read unwritten, shape.h:162-163)", s, b);
		}
		for (uint32_t b = 0; b < nBsdfs; ++b) anySlot |= bsdf_color_slots[b] != 0;
	}
	if (!vtx_col) return 0;       // masks that are all zero and no colours: nothing to keep
	// the gather array: the colours of the three vertices of every primitive of a coloured mesh, zero elsewhere
	std::vector<float> triCol(4 * (size_t) kTriColStride * ((size_t) c->nTris + 1), 0.0f);
	bool anyColors = false;
	for (uint32_t s = 0; s < nShapes; ++s) {
		if (!shape_has_colors[s]) continue;
		if (h.shapeType[s] != MTSGPU_SHAPE_TRIMESH) return fail(c, MTSGPU_EINVAL, "shape %u: only a triangle mesh can carry vertex colours", s);
		anyColors = true;
		uint32_t v;
		if (!gatherMeshRows(h.triIdx.data(), h.shapeTriOffset[s], h.shapeTriOffset[s + 1], vtx_col, 3, kTriColStride, triCol.data(), &v))
			return fail(c, MTSGPU_EINVAL, "shape %u: non-finite colour at vertex %u", s, v);
	}
	if (!anyColors) return 0;
	const float *dCol = nullptr; const uint32_t *dSlots = nullptr;
	int rc = upload(c, &dCol, triCol.data(), triCol.size(), &c->colors.allocs);
	if (!rc && anySlot) rc = upload(c, &dSlots, bsdf_color_slots, nBsdfs, &c->colors.allocs);
	if (rc) { c->colors.clear(); return rc; }
	c->colors.d = DColors{ reinterpret_cast<const float4 *>(dCol), dSlots };
	if (anySlot) c->colors.slots.assign(bsdf_color_slots, bsdf_color_slots + nBsdfs);
	return 0;
}

// mtsgpu_set_uv_textures, mtsgpu_set_uv_bitmap_textures and mtsgpu_set_uv_masked_textures (me: the caller's name)
static int setUvTextures(mtsgpu_ctx *c, const TextureArgs &a, const char *me) {
	// an entry mtsgpu_set_cloth_bsdfs has given a weave takes neither a textured slot nor a mask; and the cloth table was
	// checked against the texcoords that go with this call, so a texture call while one is in force is refused before anything
	// is freed (the cloth kernels read the uv array): the order is the texture call first (mtsgpu_cloth.h)
	const int rc0 = beginAttach(c, me, [&]() -> std::string {
		const InForce in = c->inForce();
		if (!in.clothWeave) return std::string();
		for (uint32_t b = 0; b < (uint32_t) c->host.bsdfType.size(); ++b) {
			std::string held = claimRefusal(kFamTextures, b, textureSlotsClaimed(a.bsdf_slot_texture, b), in, kFamCloth);
			if (held.empty()) held = claimRefusal(kFamMasks, b, a.bsdf_mask && a.bsdf_mask[b].kind != (uint32_t) MTSGPU_MASK_NONE, in, kFamCloth);
			if (!held.empty()) return held;
		}
		return std::string(me) + " while a cloth table is in force: the texture call comes first (switch the table off with mtsgpu_set_cloth_bsdfs(ctx, 0, NULL, NULL))";
	});
	if (rc0) return rc0;
	c->tex.clear();
	if (c->inForce().spotTextures && a.bsdf_mask)
		for (uint32_t b = 0; b < (uint32_t) c->host.bsdfType.size(); ++b)
			if (a.bsdf_mask[b].kind != (uint32_t) MTSGPU_MASK_NONE) return fail(c, MTSGPU_EINVAL, "BSDF %u: %s", b, spotBesideRefusal("the mask BSDF").c_str());
	TexturePlan p;
	const std::string why = planTextures(c->host, c->inForce(), a, p);
	if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
	if (!p.keep) return 0;
	const uint32_t nBsdfs = (uint32_t) c->host.bsdfType.size();
	std::vector<void *> *owner = &c->tex.allocs;
	const float *dUv = nullptr, *dTexels = nullptr; const DTexture *dTex = nullptr; const int32_t *dSlots = nullptr; const DMask *dMask = nullptr;
	int rc = upload(c, &dUv, p.triUv.data(), p.triUv.size(), owner);
	// (a mask keeps the textures and the bitmaps when no slot uses them)
	if (!rc && !p.desc.empty()) rc = upload(c, &dTex, p.desc.data(), p.desc.size(), owner);
	if (!rc && p.anySlot) rc = upload(c, &dSlots, a.bsdf_slot_texture, 2 * (size_t) nBsdfs, owner);
	if (!rc && p.anyMask) rc = upload(c, &dMask, reinterpret_cast<const DMask *>(a.bsdf_mask), nBsdfs, owner);
	if (!rc && !p.pool.empty()) rc = upload(c, &dTexels, p.pool.data(), p.pool.size(), owner);
	if (rc) { c->tex.clear(); return rc; }
	c->tex.d = DTextures{ reinterpret_cast<const float4 *>(dUv), dTex, dSlots, reinterpret_cast<const float4 *>(dTexels) };
	c->tex.msk = DMasks{ dMask };
	if (p.anySlot) c->tex.slotTex.assign(a.bsdf_slot_texture, a.bsdf_slot_texture + 2 * (size_t) nBsdfs);
	c->tex.shapeHasUv = std::move(p.shapeHasUv);
	c->tex.uvRange = std::move(p.uvRange);
	for (uint32_t b = 0; b < nBsdfs && p.anyMask; ++b) c->tex.maskKind.push_back(a.bsdf_mask[b].kind);
	return 0;
}

int mtsgpu_set_uv_textures(mtsgpu_ctx *c, const float *vtx_uv, const uint32_t *shape_has_uv, uint32_t n_textures,
                           const mtsgpu_uv_texture *textures, const int32_t *bsdf_slot_texture) {
	return setUvTextures(c, TextureArgs{ vtx_uv, shape_has_uv, n_textures, textures, bsdf_slot_texture, 0, nullptr, nullptr, false, nullptr },
	                     "mtsgpu_set_uv_textures");
}

int mtsgpu_set_uv_bitmap_textures(mtsgpu_ctx *c, const float *vtx_uv, const uint32_t *shape_has_uv, uint32_t n_textures,
                                  const mtsgpu_uv_texture *textures, const int32_t *bsdf_slot_texture, uint32_t n_bitmaps,
                                  const mtsgpu_bitmap *bitmaps, const int32_t *texture_bitmap) {
	return setUvTextures(c, TextureArgs{ vtx_uv, shape_has_uv, n_textures, textures, bsdf_slot_texture, n_bitmaps, bitmaps, texture_bitmap, true, nullptr },
	                     "mtsgpu_set_uv_bitmap_textures");
}

int mtsgpu_set_uv_masked_textures(mtsgpu_ctx *c, const float *vtx_uv, const uint32_t *shape_has_uv, uint32_t n_textures,
                                  const mtsgpu_uv_texture *textures, const int32_t *bsdf_slot_texture, uint32_t n_bitmaps,
                                  const mtsgpu_bitmap *bitmaps, const int32_t *texture_bitmap, const mtsgpu_bsdf_mask *bsdf_mask) {
	return setUvTextures(c, TextureArgs{ vtx_uv, shape_has_uv, n_textures, textures, bsdf_slot_texture, n_bitmaps, bitmaps, texture_bitmap, true, bsdf_mask },
	                     "mtsgpu_set_uv_masked_textures");
}

int mtsgpu_set_snow_bsdfs(mtsgpu_ctx *c, const mtsgpu_bsdf_snow *table) {
	if (int rc = beginAttach(c, "mtsgpu_set_snow_bsdfs")) return rc;
	c->snow.clear();
	if (!table) return 0;
	if (c->inForce().spotTextures)
		for (uint32_t b = 0; b < (uint32_t) c->host.bsdfType.size(); ++b)
			if (table[b].kind != (uint32_t) MTSGPU_SNOW_NONE) return fail(c, MTSGPU_EINVAL, "BSDF %u: %s", b, spotBesideRefusal("a snow BRDF").c_str());
	if (c->host.hasShapes == kHasCylinders)
		return fail(c, MTSGPU_EINVAL, "the snow BRDFs are not served in a scene with a cylinder yet (the snow kernels do not build a cylinder's record)");
	const HostScene &h = c->host;
	const InForce in = c->inForce();
	const uint32_t nBsdfs = (uint32_t) h.bsdfType.size();
	std::string why = checkBsdfSnow(nBsdfs, h.bsdfType.data(), h.bsdfParams.data(), table, in);
	for (uint32_t b = 0; b < nBsdfs && why.empty(); ++b)      // an entry mtsgpu_set_cloth_bsdfs has given a weave
		why = claimRefusal(kFamSnow, b, table[b].kind != (uint32_t) MTSGPU_SNOW_NONE, in, kFamCloth);
	if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
	bool any = false;
	for (uint32_t b = 0; b < nBsdfs; ++b) any |= table[b].kind != (uint32_t) MTSGPU_SNOW_NONE;
	if (!any) return 0;           // nothing to keep: the context launches what it launches without a table
	const DSnow *dSnow = nullptr;
	if (int rc = upload(c, &dSnow, reinterpret_cast<const DSnow *>(table), nBsdfs, &c->snow.allocs)) { c->snow.clear(); return rc; }
	c->snow.d = DSnows{ dSnow };
	for (uint32_t b = 0; b < nBsdfs; ++b) c->snow.kind.push_back(table[b].kind);
	return 0;
}

int mtsgpu_set_cloth_bsdfs(mtsgpu_ctx *c, uint32_t n_weaves, const mtsgpu_weave *weaves, const int32_t *bsdf_weave) {
	if (int rc = beginAttach(c, "mtsgpu_set_cloth_bsdfs")) return rc;
	c->cloth.clear();
	if (bsdf_weave && c->inForce().spotTextures)
		for (uint32_t b = 0; b < (uint32_t) c->host.bsdfType.size(); ++b)
			if (bsdf_weave[b] >= 0) return fail(c, MTSGPU_EINVAL, "BSDF %u: %s", b, spotBesideRefusal("the cloth BRDF").c_str());
	ClothPlan p;
	const std::string why = planCloth(c->host, c->inForce(), n_weaves, weaves, bsdf_weave, p);
	if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
	if (!p.keep) return 0;
	const uint32_t nBsdfs = (uint32_t) c->host.bsdfType.size();
	std::vector<void *> *owner = &c->cloth.allocs;
	const DWeave *dW = nullptr; const uint32_t *dP = nullptr; const DYarn *dY = nullptr; const int32_t *dB = nullptr;
	int rc = upload(c, &dW, p.weaves.data(), p.weaves.size(), owner);
	if (!rc) rc = upload(c, &dP, p.pattern.data(), p.pattern.size(), owner);
	if (!rc) rc = upload(c, &dY, p.yarns.data(), p.yarns.size(), owner);
	if (!rc) rc = upload(c, &dB, bsdf_weave, nBsdfs, owner);
	if (rc) { c->cloth.clear(); return rc; }
	c->cloth.d = DCloths{ dW, dP, dY, dB };
	c->cloth.weave.assign(bsdf_weave, bsdf_weave + nBsdfs);
	return 0;
}

int mtsgpu_set_spot_textures(mtsgpu_ctx *c, uint32_t n_textures, const mtsgpu_uv_texture *textures, uint32_t n_bitmaps, const mtsgpu_bitmap *bitmaps,
                             const int32_t *texture_bitmap, const uint32_t *texture_bilinear, const int32_t *lum_texture) {
	if (int rc = beginAttach(c, "mtsgpu_set_spot_textures")) return rc;
	c->spots.clear();
	const HostScene &h = c->host;
	const InForce in = c->inForce();
	const uint32_t nLums = (uint32_t) h.lumType.size();
	SpotPlan p;
	const SpotArgs a{ n_textures, textures, n_bitmaps, bitmaps, texture_bitmap, texture_bilinear, lum_texture };
	const std::string why = planSpots(nLums, h.lumType.data(), h.lumParams.data(), a, in.maskKind != nullptr, in.snowKind != nullptr, in.clothWeave != nullptr, p);
	if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
	if (!p.keep) return 0;
	std::vector<void *> *owner = &c->spots.allocs;
	const DTexture *dTex = nullptr; const float *dTexels = nullptr, *dFactor = nullptr; const int32_t *dLum = nullptr;
	int rc = upload(c, &dTex, p.desc.data(), p.desc.size(), owner);
	if (!rc && !p.pool.empty()) rc = upload(c, &dTexels, p.pool.data(), p.pool.size(), owner);
	if (!rc) rc = upload(c, &dLum, lum_texture, nLums, owner);
	if (!rc) rc = upload(c, &dFactor, p.uvFactor.data(), nLums, owner);
	if (rc) { c->spots.clear(); return rc; }
	c->spots.d = DSpots{ dTex, reinterpret_cast<const float4 *>(dTexels), dLum, dFactor };
	return 0;
}

int mtsgpu_spot_textures_check(uint32_t n_lums, const uint32_t *lum_type, const float *lum_params, uint32_t n_textures, const mtsgpu_uv_texture *textures,
                               uint32_t n_bitmaps, const mtsgpu_bitmap *bitmaps, const int32_t *texture_bitmap, const uint32_t *texture_bilinear,
                               const int32_t *lum_texture, uint32_t in_force, float *uv_factor) {
	if (n_lums && (!lum_type || !lum_params)) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	if (in_force > 7u) return fail(nullptr, MTSGPU_EINVAL, "unknown in_force bits %u", in_force);
	SpotPlan p;
	const SpotArgs a{ n_textures, textures, n_bitmaps, bitmaps, texture_bitmap, texture_bilinear, lum_texture };
	const std::string why = planSpots(n_lums, lum_type, lum_params, a, (in_force & 1u) != 0, (in_force & 2u) != 0, (in_force & 4u) != 0, p);
	if (!why.empty()) return fail(nullptr, MTSGPU_EINVAL, "%s", why.c_str());
	for (uint32_t l = 0; uv_factor && l < n_lums; ++l) uv_factor[l] = p.keep ? p.uvFactor[l] : 0.0f;
	return 0;
}

// LDRTexture::initializeFrom (ldrtexture.cpp:116-202) and MIPMap::fromBitmap (mipmap.cpp:156-177)
int mtsgpu_ldr_texels(int bpp, uint32_t width, uint32_t height, const uint8_t *data, float gamma, float *out) {
	if (!data || !out) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	if (width == 0 || height == 0) return fail(nullptr, MTSGPU_EINVAL, "zero dimension (%u x %u)", width, height);
	if (bpp != 1 && bpp != 8 && bpp != 16 && bpp != 24 && bpp != 32)
		return fail(nullptr, MTSGPU_EINVAL, "%i bpp images are currently not supported!", bpp);
	float tbl[256];
	if (gamma == -1.0f) {
		for (int i = 0; i < 256; ++i) {      // fromSRGBComponent (:116-121)
			const float value = (float) i / 255.0f;
			tbl[i] = value <= 0.04045f ? value / 12.92f : std::pow((value + 0.055f) / (float) (1.0 + 0.055), 2.4f);
		}
	} else {
		for (int i = 0; i < 256; ++i) tbl[i] = std::pow((float) i / 255.0f, gamma);
	}
	for (int i = 0; i < 256; ++i) tbl[i] = std::max(tbl[i], 0.0f);      // clampNegative (a NaN of pow stays one: the upload refuses it)
	const size_t n = (size_t) width * height;
	for (size_t pos = 0; pos < n; ++pos) {
		float *o = out + 3 * pos;
		if (bpp == 32 || bpp == 24) {
			const uint8_t *p = data + (size_t) (bpp / 8) * pos;
			o[0] = tbl[p[0]]; o[1] = tbl[p[1]]; o[2] = tbl[p[2]];
		} else {
			const int value = bpp == 16 ? data[2 * pos] : bpp == 8 ? data[pos] : (data[pos / 8] & (1 << (pos % 8))) ? 255 : 0;
			o[0] = o[1] = o[2] = tbl[value];
		}
	}
	return 0;
}

} // extern "C"
