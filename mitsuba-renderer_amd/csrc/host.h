// host.h -- host-side pieces of libmtsgpu shared between translation units.
#pragma once
#include "../../include/mtsgpu.h"
#include "../../include/mtsgpu_mask.h"
#include "../../include/mtsgpu_snow.h"
#include "../../include/mtsgpu_cloth.h"
#include "../../include/mtsgpu_cylinder.h"
#include "../../include/mtsgpu_spot.h"
#include "devmath.h"
#include "kdtree.h"
#include "kernels.h"
#include <cmath>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace mg {

// Owns every array a mtsgpu_scene points to
struct FlatScene {
	mtsgpu_scene sc;
	KdTree kd;
	std::vector<float> envPixels, envPdf, envCdf;
	std::vector<float> vtxPos, vtxNrm, shapeParams, bsdfParams, lumParams, lumInvArea, lumTriCdf, lumSelCdf, lumSelPdf;
	std::vector<uint32_t> triIdx, shapeTriOffset, shapeFlags, shapeType, triaccel, bsdfType, lumType, lumCdfOffset;
	std::vector<int32_t> shapeBsdf, shapeLum, lumShape;
	// per-vertex colours (mtsgpu_flat_scene_set_mesh_colors): the pool [n_verts][3] in the order of vtxPos and one flag per
	// shape, both empty until a mesh receives colours; shapeVtxOffset[s] = the first pool row of shape s
	std::vector<float> vtxCol;
	std::vector<uint32_t> shapeHasColors, shapeVtxOffset;
	// texture coordinates (mtsgpu_flat_scene_set_mesh_texcoords): the pool [n_verts][2] and the flags, kept like the colours
	std::vector<float> vtxUv;
	std::vector<uint32_t> shapeHasUv;
	// tangents (mtsgpu_flatten_tangents): the pool [n_verts][6] = dpdu, dpdv and one flag per shape, both empty unless a mesh
	// with texcoords has an anisotropic BSDF (TriMesh::computeTangentSpaceBasis)
	std::vector<float> vtxTan;
	std::vector<uint32_t> shapeHasTan;
	// the derived blocks of the cylinders (mtsgpu_flatten_cylinders): [n_shapes + 1][MTSGPU_CYLINDER_NDERIVED], zero rows for the
	// other shapes; empty without a cylinder
	std::vector<float> cylinders;
};

// Texture-typed spectrum slots per BSDF type, in slot order (include/mtsgpu.h): the first float of each slot's three in the
// parameter block, -1 = no such slot.  The composite has none of its own.
constexpr int kBsdfColorSlotOffset[MTSGPU_BSDF_NTYPES][2] = {
	{ 0, -1 }, { 2, 5 }, { 7, -1 }, { 5, 8 }, { 0, -1 }, { 5, 8 }, { 4, 7 }, { 0, -1 }, { 7, 10 }, { -1, -1 } };
inline int bsdfColorSlotCount(uint32_t type) {
	const uint32_t t = type & 0xFFu;
	if (t >= MTSGPU_BSDF_NTYPES) return 0;
	return (kBsdfColorSlotOffset[t][0] >= 0) + (kBsdfColorSlotOffset[t][1] >= 0);
}
// The attachment families that can claim a BSDF entry between two uploads, and the tables in force: host copies of what each
// family's setter accepted last, NULL while the family is off.  colorSlots [n_bsdfs] (mtsgpu_set_vertex_colors), slotTex
// [n_bsdfs][2] and maskKind [n_bsdfs] (the texture calls), snowKind [n_bsdfs], clothWeave [n_bsdfs]; and, from the texture
// call, shapeHasUv [n_shapes] with the extremes uvRange [n_shapes][4] = uMin, uMax, vMin, vMax of every shape's texcoords
enum Family : uint32_t { kFamColors = 1u, kFamTextures = 2u, kFamMasks = 4u, kFamSnow = 8u, kFamCloth = 16u, kFamAll = 31u };
struct InForce {
	const uint32_t *colorSlots = nullptr;
	const int32_t *slotTex = nullptr;
	const uint32_t *maskKind = nullptr, *snowKind = nullptr;
	const int32_t *clothWeave = nullptr;
	const uint32_t *shapeHasUv = nullptr;
	const double *uvRange = nullptr;
	bool spotTextures = false;           // mtsgpu_set_spot_textures has given a luminaire a texture: masks, snow and cloth stay out
};
// The refusal of a mask, snow or cloth call (`what`) in a context that has a textured spot, and of the spot call in a context that
// has one of the three: the kernels of a textured spot carry colours, uv textures and tangents only.  Whichever call comes second refuses
inline std::string spotBesideRefusal(const char *what) {
	return std::string(what) + " is not served in a context with a textured spot luminaire (the spot kernels do not carry it); "
	       "switch the projection textures off with mtsgpu_set_spot_textures(ctx, 0, NULL, 0, NULL, NULL, NULL, NULL)";
}
// the slots of entry b that a slot table [n_bsdfs][2] (or NULL) gives a texture, as bits
inline uint32_t textureSlotsClaimed(const int32_t *slotTex, uint32_t b) {
	return slotTex ? (slotTex[2 * (size_t) b] >= 0 ? 1u : 0u) | (slotTex[2 * (size_t) b + 1] >= 0 ? 2u : 0u) : 0u;
}
// May family `f` claim BSDF entry b, given what is in force?  The one place of the pairwise rules: a texture slot takes vertex
// colours or a uv texture, not both; a snow or cloth entry has no texture slot, no mask, and is one of the two.  want: the
// slots claimed (bit s; colours, textures) or non-zero (masks, snow, cloth); holders: the families asked, in the order colours,
// textures, masks, snow, cloth (the setters report in their own order and ask for them one at a time where that differs).
// Returns the refusal in the words of the claiming call, or an empty string.
inline std::string claimRefusal(Family f, uint32_t b, uint32_t want, const InForce &in, uint32_t holders = kFamAll) {
	if (!want) return std::string();
	const std::string who = "BSDF " + std::to_string(b) + ": ";
	const uint32_t colors = (holders & kFamColors) && in.colorSlots ? in.colorSlots[b] : 0u;
	const uint32_t tex = (holders & kFamTextures) ? textureSlotsClaimed(in.slotTex, b) : 0u;
	const bool mask = (holders & kFamMasks) && in.maskKind && in.maskKind[b] != (uint32_t) MTSGPU_MASK_NONE;
	const bool snow = (holders & kFamSnow) && in.snowKind && in.snowKind[b] != (uint32_t) MTSGPU_SNOW_NONE;
	const bool cloth = (holders & kFamCloth) && in.clothWeave && in.clothWeave[b] >= 0;
	auto slot = [](uint32_t bits) { return std::to_string((bits & 1u) ? 0 : 1); };
	switch (f) {
	case kFamColors:
		if (want & tex) return who + "slot " + slot(want & tex) + " takes vertex colours and has a uv texture as well";
		if (snow) return who + "the entry takes vertex colours and has a snow record, whose BRDF has no texture slot";
		if (cloth) return who + "the entry takes vertex colours and has a weave, whose BRDF has no texture slot";
		break;
	case kFamTextures:
		if (want & colors) return who + "slot " + slot(want & colors) + " has a uv texture and takes vertex colours as well";
		if (snow) return who + "the entry has a uv texture and a snow record, whose BRDF has no texture slot";
		if (cloth) return who + "the entry has a uv texture and a weave, whose BRDF has no texture slot";
		break;
	case kFamMasks:
		if (snow) return who + "the entry has a mask and a snow record: a mask around a snow BRDF is not supported";
		if (cloth) return who + "the entry has a mask and a weave: a mask around a cloth BRDF is not supported";
		break;
	case kFamSnow:
		if (colors) return who + "a snow BRDF has no texture slot, and the entry takes vertex colours";
		if (tex) return who + "a snow BRDF has no texture slot, and the entry has a uv texture";
		if (mask) return who + "a mask around a snow BRDF is not supported";
		if (cloth) return who + "the entry has a weave and a snow record";
		break;
	case kFamCloth:
		if (colors) return who + "a cloth BRDF has no texture slot, and the entry takes vertex colours";
		if (tex) return who + "a cloth BRDF has no texture slot, and the entry has a uv texture";
		if (mask) return who + "a mask around a cloth BRDF is not supported";
		if (snow) return who + "the entry has a snow record and a weave";
		break;
	default: break;
	}
	return std::string();
}
// What mtsgpu_set_vertex_colors requires of the slot masks against a checked BSDF table: no bit beyond the slots of the
// type, none on a composite's child.  Returns the reason, or an empty string.
inline std::string checkBsdfColorSlots(uint32_t n_bsdfs, const uint32_t *type, const float *params, const uint32_t *slots) {
	auto msg = [](uint32_t b, const std::string &what) { return "BSDF " + std::to_string(b) + ": " + what; };
	for (uint32_t b = 0; b < n_bsdfs; ++b) {
		const int n = bsdfColorSlotCount(type[b]);
		if (slots[b] >> n)
			return msg(b, "vertex-colour slot mask " + std::to_string(slots[b]) + " names a slot beyond the " + std::to_string(n) + " texture slot(s) of its type");
	}
	for (uint32_t b = 0; b < n_bsdfs; ++b) {
		if ((type[b] & 0xFFu) != MTSGPU_BSDF_COMPOSITE) continue;
		const float *P = params + (size_t) MTSGPU_BSDF_NPARAMS * b;
		const int n = (int) P[0];
		for (int i = 0; i < n; ++i)
			if (slots[(uint32_t) P[1 + n + i]])
				return msg(b, "composite child " + std::to_string(i) + " takes vertex colours: a composite's children keep constant parameters, not supported");
	}
	return std::string();
}

// What mtsgpu_set_uv_textures requires of the slot table [n_bsdfs][2] (a texture index, or -1) against a checked BSDF table
// and the colour masks in force: indices inside the texture list, no slot beyond those of the type, none that
// is coloured as well, none on a composite's child.  Returns the reason, or an empty string.
inline std::string checkBsdfSlotTextures(uint32_t n_bsdfs, const uint32_t *type, const float *params, const int32_t *slotTex, uint32_t n_textures,
                                         const InForce &in) {
	auto msg = [](uint32_t b, const std::string &what) { return "BSDF " + std::to_string(b) + ": " + what; };
	for (uint32_t b = 0; b < n_bsdfs; ++b) {
		const int n = bsdfColorSlotCount(type[b]);
		for (int s = 0; s < 2; ++s) {
			const int32_t k = slotTex[2 * (size_t) b + s];
			if (k < -1 || k >= (int64_t) n_textures)
				return msg(b, "slot " + std::to_string(s) + " names texture " + std::to_string(k) + " of " + std::to_string(n_textures));
			if (k < 0) continue;
			if (s >= n)
				return msg(b, "uv texture in slot " + std::to_string(s) + ", beyond the " + std::to_string(n) + " texture slot(s) of its type");
			const std::string held = claimRefusal(kFamTextures, b, 1u << s, in, kFamColors);
			if (!held.empty()) return held;
		}
	}
	for (uint32_t b = 0; b < n_bsdfs; ++b) {
		if ((type[b] & 0xFFu) != MTSGPU_BSDF_COMPOSITE) continue;
		const float *P = params + (size_t) MTSGPU_BSDF_NPARAMS * b;
		const int n = (int) P[0];
		for (int i = 0; i < n; ++i) {
			const uint32_t ch = (uint32_t) P[1 + n + i];
			if (slotTex[2 * (size_t) ch] >= 0 || slotTex[2 * (size_t) ch + 1] >= 0)
				return msg(b, "composite child " + std::to_string(i) + " has a uv texture: a composite's children keep constant parameters, not supported");
		}
	}
	return std::string();
}

// What mtsgpu_set_uv_masked_textures requires of the mask table [n_bsdfs] against a checked BSDF table: known kinds, zero
// reserved words, finite opacities, texture indices inside the texture list, none on a composite or on a composite's child.
// Returns the reason, or an empty string.
inline std::string checkBsdfMasks(uint32_t n_bsdfs, const uint32_t *type, const float *params, const mtsgpu_bsdf_mask *mask, uint32_t n_textures) {
	auto msg = [](uint32_t b, const std::string &what) { return "BSDF " + std::to_string(b) + ": " + what; };
	for (uint32_t b = 0; b < n_bsdfs; ++b) {
		const mtsgpu_bsdf_mask &m = mask[b];
		if (m.kind > (uint32_t) MTSGPU_MASK_TEXTURE) return msg(b, "unknown mask kind " + std::to_string(m.kind));
		if (m.reserved != 0) return msg(b, "the reserved word of its mask is not zero");
		for (int k = 0; k < 3; ++k)
			if (!(std::fabs(m.opacity[k]) <= 3.4028235e38f)) return msg(b, "the opacity of its mask is not finite");
		if (m.kind == (uint32_t) MTSGPU_MASK_TEXTURE && (m.texture < 0 || m.texture >= (int64_t) n_textures))
			return msg(b, "its mask names texture " + std::to_string(m.texture) + " of " + std::to_string(n_textures));
		if (m.kind != (uint32_t) MTSGPU_MASK_NONE && (type[b] & 0xFFu) == MTSGPU_BSDF_COMPOSITE)
			return msg(b, "a mask around a composite is not supported");
	}
	for (uint32_t b = 0; b < n_bsdfs; ++b) {
		if ((type[b] & 0xFFu) != MTSGPU_BSDF_COMPOSITE) continue;
		const float *P = params + (size_t) MTSGPU_BSDF_NPARAMS * b;
		const int n = (int) P[0];
		for (int i = 0; i < n; ++i)
			if (mask[(uint32_t) P[1 + n + i]].kind != (uint32_t) MTSGPU_MASK_NONE)
				return msg(b, "composite child " + std::to_string(i) + " has a mask: a mask is the outermost adapter (mask.cpp), not supported inside a composite");
	}
	return std::string();
}

// Wiscombe::configure (wiscombe.cpp:70-101) in binary32, in the reference's operation order and with its operators as compiled
// (spectrum.h): Float * Spectrum and Float / Spectrum are the friends that return spd * f and spd / f, and Spectrum / Float
// multiplies by 1.0f / f.  raw = g, depth, w0 rgb, sigmaT rgb.  m_tau, m_tauStar, m_gamma1 and m_gamma2 are computed there and
// never read.  derived: wStar, bStar, xi, P.
inline void snowWiscombeConfigure(const float *raw, float *derived) {
	const float g = raw[0];
	const float gSq = g * g;
	const float gStar = g / (1.0f + g);
	const float recipGStar = 1.0f / gStar;
	for (int k = 0; k < 3; ++k) {
		const float w0 = raw[2 + k];
		const float wStar = (w0 * (1.0f - gSq)) / (1.0f - w0 * gSq);
		const float bTmp = 1.0f - wStar * gStar;
		const float bStar = bTmp * recipGStar;                        // m_gStar / bTmp: operator/(Float, Spectrum &) = bTmp / gStar
		const float xiSq = ((1.0f - wStar * gStar) * (1.0f - wStar)) * 3.0f;
		const float xi = sqrtf(xiSq);
		const float P = (xi * 2.0f) / ((1.0f - wStar * gStar) * 3.0f);
		derived[k] = wStar; derived[3 + k] = bStar; derived[6 + k] = xi; derived[9 + k] = P;
	}
	derived[12] = derived[13] = 0.0f;
}

// HanrahanKrueger::configure (hanrahan-krueger.cpp:89-132) likewise; exp is dexp.  raw = sigmaA rgb, sigmaS
// rgb, g, etaInt, etaExt, ssFactor rgb, drFactor rgb, useDiffuseReflectance.  (4.0 / 3.0) * A is a binary64 product, rounded
// once when the friend operator*(Float, Spectrum &) takes it; reducedAlbedo / 2.0 is Spectrum / Float = * (1.0f / 2.0f).
// derived: sigmaS / sigmaT, ssFactor, the diffuse reflectance times drFactor, g, eta, the flag as 0 / 1.
inline void snowHkConfigure(const float *raw, float *derived) {
	const float g = raw[6], eta = raw[7] / raw[8];
	float Fdr;
	if (eta > 1)
		Fdr = -1.440f / (eta * eta) + 0.710f / eta + 0.668f + 0.0636f * eta;                       // [Groenhuis et al. 1983]
	else
		Fdr = -0.4399f + 0.7099f / eta - 0.3319f / (eta * eta) + 0.0636f / (eta * eta * eta);      // [Egan et al. 1973]
	float Fdt = 1.0f - Fdr;
	if (eta == 1.0f) { Fdr = 0.0f; Fdt = 1.0f; }
	const float A = (1 + Fdr) / Fdt;
	const float fourThirdsA = (float) ((4.0 / 3.0) * (double) A);
	for (int k = 0; k < 3; ++k) {
		const float sigmaA = raw[k], sigmaS = raw[3 + k];
		const float sigmaT = sigmaA + sigmaS;
		const float sigmaSPrime = sigmaS * (1 - g);
		const float sigmaTPrime = sigmaA + sigmaSPrime;
		const float reducedAlbedo = sigmaSPrime / sigmaTPrime;
		const float var1 = -sqrtf((1.0f - reducedAlbedo) * 3.0f);
		const float dr = ((reducedAlbedo * (1.0f / 2.0f)) * (1.0f + mg::dexp(var1 * fourThirdsA))) * mg::dexp(var1);
		derived[k] = sigmaS / sigmaT;
		derived[3 + k] = raw[9 + k];
		derived[6 + k] = dr * raw[12 + k];
	}
	derived[9] = g; derived[10] = eta; derived[11] = raw[15] != 0.0f ? 1.0f : 0.0f;
	derived[12] = derived[13] = 0.0f;
}

// the first word of `derived` that is not finite, or -1
inline int snowFirstNonFinite(const mtsgpu_bsdf_snow &e) {
	for (int k = 0; k < 14; ++k)
		if (!(std::fabs(e.derived[k]) <= 3.4028235e38f)) return k;
	return -1;
}

// What mtsgpu_set_snow_bsdfs and mtsgpu_bsdf_eval_snow require of one snow record on an entry of type word `type`: a known kind,
// a zero reserved word, finite derived words, and for a snow kind a Lambertian under at most the twosided adapter.  Returns the
// reason, or an empty string.
inline std::string checkSnowEntry(const mtsgpu_bsdf_snow &e, uint32_t type) {
	if (e.kind > (uint32_t) MTSGPU_SNOW_HK) return "unknown snow kind " + std::to_string(e.kind);
	if (e.reserved != 0) return "the reserved word of its snow record is not zero";
	const int bad = snowFirstNonFinite(e);
	if (bad >= 0) return "derived word " + std::to_string(bad) + " of its snow record is not finite";
	if (e.kind != (uint32_t) MTSGPU_SNOW_NONE && (type & ~(uint32_t) MTSGPU_BSDF_TWOSIDED) != (uint32_t) MTSGPU_BSDF_LAMBERTIAN)
		return "a snow record sits on a Lambertian entry (twosided allowed), not on type word " + std::to_string(type);
	return std::string();
}

// ... and of the table [n_bsdfs] against a checked BSDF table and the tables in force: every record as above, none on an entry
// with a coloured slot, a textured slot or a mask, none on a composite's child.
inline std::string checkBsdfSnow(uint32_t n_bsdfs, const uint32_t *type, const float *params, const mtsgpu_bsdf_snow *snow, const InForce &in) {
	auto msg = [](uint32_t b, const std::string &what) { return "BSDF " + std::to_string(b) + ": " + what; };
	for (uint32_t b = 0; b < n_bsdfs; ++b) {
		const std::string why = checkSnowEntry(snow[b], type[b]);
		if (!why.empty()) return msg(b, why);
		const std::string held = claimRefusal(kFamSnow, b, snow[b].kind != (uint32_t) MTSGPU_SNOW_NONE, in, kFamColors | kFamTextures | kFamMasks);
		if (!held.empty()) return held;
	}
	for (uint32_t b = 0; b < n_bsdfs; ++b) {
		if ((type[b] & 0xFFu) != MTSGPU_BSDF_COMPOSITE) continue;
		const float *P = params + (size_t) MTSGPU_BSDF_NPARAMS * b;
		const int n = (int) P[0];
		for (int i = 0; i < n; ++i)
			if (snow[(uint32_t) P[1 + n + i]].kind != (uint32_t) MTSGPU_SNOW_NONE)
				return msg(b, "composite child " + std::to_string(i) + " has a snow record: the composite's loop would run it as a Lambertian, not supported");
	}
	return std::string();
}

// What mtsgpu_set_cloth_bsdfs and mtsgpu_bsdf_eval_cloth require of one weave: the reference's SAsserts (irawan.cpp:73-77), known
// yarn types, finite parameters, and positive width, length, umax and areas, non-negative fineness and period (narrower than the
// reference, which divides by them).  Returns the reason, or an empty string.
inline std::string checkWeave(const mtsgpu_weave &w) {
	auto finite = [](float x) { return std::fabs(x) <= 3.4028235e38f; };
	if (w.tileWidth == 0 || w.tileHeight == 0) return "zero tile dimension (" + std::to_string(w.tileWidth) + " x " + std::to_string(w.tileHeight) + ")";
	if (w.tileWidth > 32768u || w.tileHeight > 32768u) return "a tile dimension above 32768";
	if ((uint64_t) w.n_pattern != (uint64_t) w.tileWidth * w.tileHeight)
		return "pattern size " + std::to_string(w.n_pattern) + " is not tileWidth * tileHeight = " + std::to_string((uint64_t) w.tileWidth * w.tileHeight);
	if (!w.pattern || !w.yarns || w.n_yarns == 0) return "no pattern or no yarns";
	for (uint32_t i = 0; i < w.n_pattern; ++i)
		if (w.pattern[i] == 0 || w.pattern[i] > w.n_yarns)
			return "pattern entry " + std::to_string(i) + " = " + std::to_string(w.pattern[i]) + " is outside 1.." + std::to_string(w.n_yarns);
	const float scalars[16] = { w.alpha, w.beta, w.ss, w.hWidth, w.warpArea, w.weftArea, w.dWarpUmaxOverDWarp, w.dWarpUmaxOverDWeft,
	                            w.dWeftUmaxOverDWarp, w.dWeftUmaxOverDWeft, w.fineness, w.period, w.repeatU, w.repeatV, w.kdMultiplier, w.ksMultiplier };
	static const char *const names[16] = { "alpha", "beta", "ss", "hWidth", "warpArea", "weftArea", "dWarpUmaxOverDWarp", "dWarpUmaxOverDWeft",
	                                       "dWeftUmaxOverDWarp", "dWeftUmaxOverDWeft", "fineness", "period", "repeatU", "repeatV", "kdMultiplier", "ksMultiplier" };
	for (int i = 0; i < 16; ++i)
		if (!finite(scalars[i])) return std::string(names[i]) + " is not finite";
	if (!(w.warpArea > 0) || !(w.weftArea > 0)) return "warpArea and weftArea must be positive";
	if (w.fineness < 0 || w.period < 0) return "fineness and period must not be negative";
	for (uint32_t y = 0; y < w.n_yarns; ++y) {
		const mtsgpu_yarn &Y = w.yarns[y];
		const std::string me = "yarn " + std::to_string(y) + ": ";
		if (Y.type > (uint32_t) MTSGPU_YARN_WEFT) return me + "unknown type " + std::to_string(Y.type);
		const float p[13] = { Y.psi, Y.umax, Y.kappa, Y.width, Y.length, Y.centerU, Y.centerV, Y.kd[0], Y.kd[1], Y.kd[2], Y.ks[0], Y.ks[1], Y.ks[2] };
		for (int i = 0; i < 13; ++i)
			if (!finite(p[i])) return me + "a parameter is not finite";
		if (!(Y.width > 0) || !(Y.length > 0) || !(Y.umax > 0)) return me + "width, length and umax must be positive";
	}
	return std::string();
}

// The casts of IrawanClothBRDF::f (irawan.cpp:114-125, 170-181, 206-208; noise.cpp:66) on a surface whose texcoords reach
// (u, v) in [uMin, uMax] x [vMin, vMax]: every one must stay inside its type's range with the margin of the texture calls,
// L = 2^31 - 2^16.  In binary64, from the extremes:
//   X = max |u repeatU tileWidth|, Y = max |(1 - v) repeatV tileHeight|          the two (int) casts: X, Y < L
//   Cx = max |center.x|: (int) xy.x / tileWidth is unsigned, so Cx <= 2^32 + |centerU| tileWidth where xy.x can be negative,
//        and X + |centerU| tileWidth otherwise (any negative extreme counts: an interpolated texcoord may round past -1); Cy likewise with |1 - centerV| tileHeight
//   period > 0: the seed factors (uint64_t) center.x, (uint64_t) (tileHeight repeatV), (uint64_t) center.y need Cx, Cy,
//        |tileHeight repeatV| < 2^63 -- held to L for the last one, 2^33 bounds the others; the two floorToInt arguments are at most
//        (Cx (|tileHeight repeatV| + 1) + Cy) / period and (Cy (|tileWidth repeatU| + 1) + Cx) / period (nextFloat() < 1): < L
//   fineness > 0: the local xy after the translation (and the weft's rotation, which swaps the axes) is at most
//        S = max(X + Cx, Y + Cy), so |center + xy| <= max(Cx, Cy) + S; times fineness < L, and |tileHeight repeatV fineness| < L
// Returns the reason, or an empty string.
inline std::string clothCastRange(const mtsgpu_weave &w, double uMin, double uMax, double vMin, double vMax) {
	const double L = 2147483648.0 - 65536.0;
	const double tw = w.tileWidth, th = w.tileHeight, ru = w.repeatU, rv = w.repeatV;
	const double x0 = uMin * ru * tw, x1 = uMax * ru * tw, y0 = (1.0 - vMin) * rv * th, y1 = (1.0 - vMax) * rv * th;
	const double X = std::max(std::fabs(x0), std::fabs(x1)), Y = std::max(std::fabs(y0), std::fabs(y1));
	if (!(X < L) || !(Y < L)) return "a texcoord maps outside the range of the (int) cast (|xy| >= 2^31 - 2^16)";
	double cu = 0, cv = 0;
	for (uint32_t y = 0; y < w.n_yarns; ++y) {
		cu = std::max(cu, std::fabs((double) w.yarns[y].centerU) * tw);
		cv = std::max(cv, std::fabs(1.0 - (double) w.yarns[y].centerV) * th);
	}
	const double Cx = (std::min(x0, x1) < 0.0 ? 4294967296.0 : X) + cu, Cy = (std::min(y0, y1) < 0.0 ? 4294967296.0 : Y) + cv;
	if (w.period > 0) {
		if (!(std::fabs(th * rv) < L)) return "tileHeight * repeatV leaves the range of the seed's cast";
		const double a = (Cx * (std::fabs(th * rv) + 1.0) + Cy) / w.period, b = (Cy * (std::fabs(tw * ru) + 1.0) + Cx) / w.period;
		if (!(a < L) || !(b < L)) return "a noise argument can leave the range of floorToInt (>= 2^31 - 2^16)";
	}
	if (w.fineness > 0) {
		const double S = std::max(X + Cx, Y + Cy);
		if (!((std::max(Cx, Cy) + S) * w.fineness < L) || !(std::fabs(th * rv * w.fineness) < L))
			return "a fineness seed factor can leave the range of its cast (>= 2^31 - 2^16)";
	}
	return std::string();
}

// What the kernels require of a BSDF table (mtsgpu_upload_scene, mtsgpu_bsdf_eval_table and the flattener all ask here):
// known types, and for a composite (block: [0] n, [1..n] weights, [1+n..2n] child indices as floats) 1 <= n <=
// MTSGPU_COMPOSITE_MAX, no negative weight (composite.cpp:45-46), children that exist and are neither composites nor delta
// BSDFs.  Returns the reason, or an empty string.
inline std::string checkBsdfTable(uint32_t n_bsdfs, const uint32_t *type, const float *params) {
	auto msg = [](uint32_t b, const std::string &what) { return "BSDF " + std::to_string(b) + ": " + what; };
	for (uint32_t b = 0; b < n_bsdfs; ++b) {
		if ((type[b] & ~(uint32_t) MTSGPU_BSDF_TWOSIDED) >= MTSGPU_BSDF_NTYPES) return msg(b, "unknown type");
		if ((type[b] & 0xFFu) != MTSGPU_BSDF_COMPOSITE) continue;
		const float *P = params + (size_t) MTSGPU_BSDF_NPARAMS * b;
		if (!(P[0] >= 1.0f && P[0] <= (float) MTSGPU_COMPOSITE_MAX) || P[0] != (float) (int) P[0])
			return msg(b, "a composite needs between 1 and " + std::to_string(MTSGPU_COMPOSITE_MAX) + " children");
		const int n = (int) P[0];
		for (int i = 0; i < n; ++i) {
			const float w = P[1 + i], ci = P[1 + n + i];
			const std::string child = "composite child " + std::to_string(i);
			if (!(w >= 0.0f) || !(w <= 3.4028235e38f)) return msg(b, child + ": invalid BRDF weight (negative or not finite, composite.cpp:45-46)");
			if (!(ci >= 0.0f && ci < (float) n_bsdfs) || ci != (float) (uint32_t) ci) return msg(b, child + ": index out of range");
			const uint32_t ct = type[(uint32_t) ci] & 0xFFu;
			if (ct >= MTSGPU_BSDF_NTYPES) return msg(b, child + ": unknown type");
			if (ct == MTSGPU_BSDF_COMPOSITE) return msg(b, child + " is a composite: nested composites are not supported");
			if (ct == MTSGPU_BSDF_DIELECTRIC || ct == MTSGPU_BSDF_MIRROR)
				return msg(b, child + " is a delta BSDF (dielectric, mirror): a composite would need fDelta / pdfDelta, not supported");
		}
		// DiscretePDF::build divides by the sum of the weights (pdf.h:87-91): all zero makes every pdf and knot NaN
		float sum = 0.0f;
		for (int i = 0; i < n; ++i) sum = sum + P[1 + i];
		if (!(sum > 0.0f) || !(sum <= 3.4028235e38f)) return msg(b, "the weights of a composite must have a positive, finite sum");
	}
	return std::string();
}
// BSDF::EAnisotropic of entry b of a checked table: a Ward with alphaX != alphaY (ward.cpp:84-85), alone or inside a composite
inline bool bsdfIsAnisotropic(const uint32_t *type, const float *params, uint32_t b) {
	const float *P = params + (size_t) MTSGPU_BSDF_NPARAMS * b;
	const uint32_t t = type[b] & 0xFFu;
	if (t == MTSGPU_BSDF_WARD) return P[1] != P[2];
	if (t != MTSGPU_BSDF_COMPOSITE) return false;
	const int n = (int) P[0];
	for (int i = 0; i < n; ++i) {
		const uint32_t c = (uint32_t) P[1 + n + i];
		if ((type[c] & 0xFFu) == MTSGPU_BSDF_WARD && bsdfIsAnisotropic(type, params, c)) return true;
	}
	return false;
}
// Shapes that give the shading frame a tangent an anisotropic BSDF can use on their own: spheres (dpdu / dpdv).  A triangle
// mesh has one when tangents were computed from its texture coordinates (mtsgpu_flatten_tangents,
// mtsgpu_upload_scene_tangents); any shape type added later has none until it says so here.
// cylinders have one too (cylinder.cpp:165-171)
inline bool shapeHasTangentFrame(uint32_t shape_type) { return shape_type == MTSGPU_SHAPE_SPHERE || shape_type == MTSGPU_SHAPE_CYLINDER; }
// the reference's refusal of an anisotropic BSDF on a mesh without texture coordinates (trimesh.cpp:288-290, :547-556)
inline std::string anisotropicOnMeshMessage(uint32_t shape) {
	return "shape " + std::to_string(shape) + ": computeTangentSpace(): texture coordinates are required to generate tangent vectors. "
	       "If you want to render with an anisotropic material, please make sure that all associated shapes have valid texture "
	       "coordinates (a triangle mesh has none here unless mtsgpu_flatten_tangents / mtsgpu_upload_scene_tangents supplied them)";
}

// SkyLuminaire::configure() (src/luminaires/sky.cpp:139-179) and the parts of getDistribution() that depend on the
// parameters alone (:458-461), from a MTSGPU_LUM_SKY block: derived[MTSGPU_SKY_NDERIVED] =
//   [0] zenithX [1] zenithY [2] zenithL [3..7] perezX [8..12] perezY [13..17] perezL [18..20] the Perez denominators of
//   x, y, L [21] sin(thetaS) [22] cos(thetaS) (getAngleBetween, :431-432).
// Types as the reference's single-precision build: double literals promote each expression to binary64, every store into a Float member rounds to
// binary32.  The denominators and [21], [22] use the elementary functions of devmath.h in the operation order of
// getDistribution / getAngleBetween, so the kernels that read them see the bits they would have computed themselves.
inline void skyConfigure(const float *LP, float *derived) {
	const float turbidity = LP[1], thetaS = LP[16];
	const float k[5] = { LP[18], LP[19], LP[20], LP[21], LP[22] };
	const float theta2 = thetaS * thetaS;
	const float theta3 = theta2 * thetaS;
	const float turb2 = turbidity * turbidity;
	derived[0] = (float) (
		(+0.00165 * theta3 - 0.00374 * theta2 + 0.00208 * thetaS + 0) * turb2 +
		(-0.02902 * theta3 + 0.06377 * theta2 - 0.03202 * thetaS + 0.00394) * turbidity +
		(+0.11693 * theta3 - 0.21196 * theta2 + 0.06052 * thetaS + 0.25885));
	derived[1] = (float) (
		(+0.00275 * theta3 - 0.00610 * theta2 + 0.00316 * thetaS + 0) * turb2 +
		(-0.04214 * theta3 + 0.08970 * theta2 - 0.04153 * thetaS + 0.00515) * turbidity +
		(+0.15346 * theta3 - 0.26756 * theta2 + 0.06669 * thetaS + 0.26688));
	const float chi = (float) ((4.0 / 9.0 - turbidity / 120.0) * (kPi - 2 * thetaS));      // M_PI is a binary32 literal (constants.h:45-46)
	double sChi, cChi;
	sincos_d((double) chi, sChi, cChi);      // tan(chi): the binary64 sine over the binary64 cosine
	derived[2] = (float) ((4.0453 * turbidity - 4.9710) * (sChi / cChi) - 0.2155 * turbidity + 2.4192);
	float *perezX = derived + 3, *perezY = derived + 8, *perezL = derived + 13;
	perezL[0] = (float) (( 0.17872 * turbidity - 1.46303) * k[0]);
	perezL[1] = (float) ((-0.35540 * turbidity + 0.42749) * k[1]);
	perezL[2] = (float) ((-0.02266 * turbidity + 5.32505) * k[2]);
	perezL[3] = (float) (( 0.12064 * turbidity - 2.57705) * k[3]);
	perezL[4] = (float) ((-0.06696 * turbidity + 0.37027) * k[4]);
	perezX[0] = (float) ((-0.01925 * turbidity - 0.25922) * k[0]);
	perezX[1] = (float) ((-0.06651 * turbidity + 0.00081) * k[1]);
	perezX[2] = (float) ((-0.00041 * turbidity + 0.21247) * k[2]);
	perezX[3] = (float) ((-0.06409 * turbidity - 0.89887) * k[3]);
	perezX[4] = (float) ((-0.00325 * turbidity + 0.04517) * k[4]);
	perezY[0] = (float) ((-0.01669 * turbidity - 0.26078) * k[0]);
	perezY[1] = (float) ((-0.09495 * turbidity + 0.00921) * k[1]);
	perezY[2] = (float) ((-0.00792 * turbidity + 0.21023) * k[2]);
	perezY[3] = (float) ((-0.04405 * turbidity - 1.65369) * k[3]);
	perezY[4] = (float) ((-0.01092 * turbidity + 0.05291) * k[4]);
	float sinThetaS, cosThetaS;
	dsincos(thetaS, sinThetaS, cosThetaS);
	for (int i = 0; i < 3; ++i) {
		const float *lam = derived + 3 + 5 * i;
		derived[18 + i] = (1 + lam[0] * dexp(lam[1])) * (1 + lam[2] * dexp(lam[3] * thetaS) + lam[4] * cosThetaS * cosThetaS);
	}
	derived[21] = sinThetaS; derived[22] = cosThetaS;
	derived[23] = 0.0f;
}
// What the kernels require of a sky luminaire (the flattener and mtsgpu_upload_scene both ask here): it is the scene's
// background luminaire, its parameters are finite, its bounding sphere has a positive radius, and the two divisions of
// getSkySpectralRadiance / getDistribution (Y / y, num / den; sky.cpp:463,484) have non-zero divisors.  Returns the reason,
// or an empty string; derivedOut (MTSGPU_SKY_NDERIVED floats, optional) receives what skyConfigure derived on the way.
inline std::string checkSkyLuminaire(uint32_t l, const float *LP, int32_t background_lum, float *derivedOut = nullptr) {
	const std::string who = "luminaire " + std::to_string(l) + ": ";
	if ((int32_t) l != background_lum) return who + "the sky must be the background luminaire";
	for (int i = 0; i <= 22; ++i) if (!std::isfinite(LP[i])) return who + "non-finite sky parameter";
	if (!(LP[6] > 0.0f)) return who + "the sky's bounding sphere needs a positive radius";
	float own[MTSGPU_SKY_NDERIVED];
	float *derived = derivedOut ? derivedOut : own;
	skyConfigure(LP, derived);
	for (int i = 0; i < MTSGPU_SKY_NDERIVED; ++i) if (!std::isfinite(derived[i])) return who + "non-finite derived sky quantity (sky.cpp:139-179)";
	if (derived[1] == 0.0f) return who + "the sky's zenith y is zero (Y / y, sky.cpp:484)";
	for (int i = 0; i < 3; ++i) if (derived[18 + i] == 0.0f) return who + "a Perez denominator of the sky is zero (sky.cpp:463)";
	return std::string();
}

// meshTexcoords [n_meshes] (mtsgpu_flatten_tangents): the texcoords [that mesh's n_verts][2] of each mesh or NULL; with them a
// mesh whose BSDF is anisotropic is accepted and receives tangents (fs.vtxTan, fs.shapeHasTan).  NULL: no mesh has any.
// bsdfAnisotropic [n_bsdfs] (mtsgpu_flatten_tangents_flagged): non-zero = treat the entry as anisotropic as well; NULL: none.
void flattenScene(const mtsgpu_scene_desc &d, const mtsgpu_kd_params *kp, FlatScene &fs, const float *const *meshTexcoords = nullptr,
                  const uint32_t *bsdfAnisotropic = nullptr, const mtsgpu_cylinder *cylinders = nullptr);
// mtsgpu_cylinder_configure: both constructors of cylinder.cpp:34-64; the reason it refuses, or an empty string
std::string cylinderConfigure(const mtsgpu_cylinder &in, float *derived);
// What the upload requires of a derived block; the reason, or an empty string (scene_layout.cpp)
std::string checkCylinderBlock(const float *derived);
// Cylinder::getAABB (cylinder.cpp:187-208) of a derived block: out6 = min, max
void cylinderAabb(const float *derived, float *out6);
// the row of the kd-tree builder's cylinder table (kdtree.h) of a derived block
void cylinderBuilderRow(const float *derived, float *row8);
// The per-vertex colours of shape `mesh` of a flattened scene (mtsgpu_flat_scene_set_mesh_colors): colors [that mesh's
// n_verts][3] copied into fs.vtxCol at the mesh's rows, NULL takes them away again.  Returns the reason it refuses, or an
// empty string.
std::string setMeshColors(FlatScene &fs, uint32_t mesh, const float *colors);
// the same for texture coordinates: texcoords [that mesh's n_verts][2] into fs.vtxUv
std::string setMeshTexcoords(FlatScene &fs, uint32_t mesh, const float *texcoords);

// One shape of a `.serialized` file (TriMesh::TriMesh(Stream *, int), src/librender/trimesh.cpp:156-236)
struct LoadedMesh {
	std::vector<float> positions, normals;     // normals empty when the file has none
	std::vector<float> colors;                 // [n_verts][3], empty without the EHasColors block (trimesh.cpp:113-118,223-229)
	std::vector<float> texcoords;              // [n_verts][2], empty without the EHasTexcoords block (trimesh.cpp:105-111,214-221)
	std::vector<uint32_t> triangles;
	bool faceNormals = false;
};
void loadSerializedMesh(const char *path, int index, LoadedMesh &out);   // throws std::runtime_error
// TabulatedFilter of the box / gaussian / mitchell / catmullrom / wsinc plugins (kinds 0..4): sizeXY[2], values[16*16]
void tabulateFilter(int kind, float halfSize, float p0, float p1, float *sizeXY, float *values);
void makeCamera(const float origin[3], const float target[3], const float up[3], float fovDeg, int width, int height,
                mtsgpu_camera &out);
void makeCameraOrtho(const float origin[3], const float target[3], const float up[3], float scaleX, float scaleY,
                     int width, int height, mtsgpu_camera &out);

// --- scene_layout.cpp: the pure half of the upload calls (no context, no HIP call): what they check and what they lay out ---
// the arguments that travel beside the scene: mtsgpu_upload_scene passes none, mtsgpu_upload_scene_tangents the first three,
// mtsgpu_upload_scene_cylinders all (cylinders = the derived blocks [n_shapes][MTSGPU_CYLINDER_NDERIVED] or NULL)
struct UploadExtras {
	const float *vtxDpdu = nullptr;
	const uint32_t *shapeHasTangents = nullptr;
	bool withTangents = false;
	const float *cylinders = nullptr;
	bool acceptsCylinders = false;
};
// Everything the kernels index with, checked before anything is laid out or freed (an out-of-range index would fault the GPU);
// no array is read through an index that has not been checked.  depthLimit: the deepest branch the traversal stack holds
// (trace_stack_levels() - 2); skyDerived [MTSGPU_SKY_NDERIVED] receives SkyLuminaire::configure() of a background sky.
// Returns the reason, or an empty string.
std::string checkScene(const mtsgpu_scene &sc, const UploadExtras &x, uint32_t depthLimit, float *skyDerived);
// What the upload derives from a checked scene, in the order it is uploaded (DScene, DTangents)
struct SceneLayout {
	std::vector<uint32_t> nodes;         // the kd-tree in device order, 2 words per slot
	std::vector<uint32_t> leafTa;        // TriAccel records in leaf order, then the cylinders' rows
	std::vector<float> triRec;           // per-primitive position / normal records
	std::vector<uint32_t> shapeBin, shapeType;      // [n_shapes + 1]
	std::vector<float> shapeParams;      // [n_shapes + 1][MTSGPU_SHAPE_NPARAMS], a cylinder's row as the shading reads it
	std::vector<float> triDpdu;          // the gather array of the tangents, empty without a tangent mesh
	std::vector<uint32_t> hasTan;        // ... and its flags [n_shapes + 1]
	uint32_t hasShapes = 0, binMask = 0; // DScene::has_shapes; the material queues that can ever be non-empty
};
// topSlots: trace_top_nodes().  Returns a size refusal, or an empty string.
std::string layoutScene(const mtsgpu_scene &sc, const UploadExtras &x, uint32_t topSlots, SceneLayout &out);

// What the setters need of the uploaded scene once the caller's arrays may be gone: host copies, taken by the upload
struct HostScene {
	uint32_t nVerts = 0, hasShapes = 0;      // hasShapes: DScene::has_shapes
	std::vector<uint32_t> triIdx, shapeTriOffset, shapeType, bsdfType, lumType;      // triIdx: [n_tris][3]
	std::vector<int32_t> shapeBsdf;
	std::vector<float> bsdfParams, lumParams;     // lumParams: [n_lums][MTSGPU_LUM_NPARAMS]
	std::vector<uint32_t> shapeNormals, shapeTangents;      // per shape: has vertex normals / uploaded tangents (0 / 1)
};
void keepHostScene(const mtsgpu_scene &sc, const UploadExtras &x, const SceneLayout &lay, HostScene &out);
// The rows of one mesh in a per-primitive gather array: for each of its primitives [t0, t1) the attribute of the three
// vertices (`comps` floats per vertex: 4 floats apart for tangents and colours, 2 for texcoords), in rows of 4 * stride
// floats.  A non-finite component is refused: false, and *bad names the vertex.
bool gatherMeshRows(const uint32_t *triIdx, uint32_t t0, uint32_t t1, const float *vtx, int comps, size_t stride, float *rows, uint32_t *bad);
std::string checkUvTexture(const mtsgpu_uv_texture &t, bool bitmaps = false);
std::string checkBitmap(const mtsgpu_bitmap &b, uint64_t *total);
void packBitmapTexels(const mtsgpu_bitmap &b, float *dst);
// the arguments of the three texture calls (withBitmaps = false: kind MTSGPU_TEX_BITMAP is unknown; bsdf_mask: the masked call's)
struct TextureArgs {
	const float *vtx_uv = nullptr; const uint32_t *shape_has_uv = nullptr;
	uint32_t n_textures = 0; const mtsgpu_uv_texture *textures = nullptr; const int32_t *bsdf_slot_texture = nullptr;
	uint32_t n_bitmaps = 0; const mtsgpu_bitmap *bitmaps = nullptr; const int32_t *texture_bitmap = nullptr;
	bool withBitmaps = false;
	const mtsgpu_bsdf_mask *bsdf_mask = nullptr;
};
// ... and what they upload and keep (keep = false: the call switches the family off and keeps nothing)
struct TexturePlan {
	bool keep = false, anySlot = false, anyMask = false, anyMaskTex = false, anyBitmap = false;
	std::vector<float> triUv;            // the gather array of the texcoords
	std::vector<DTexture> desc;          // the descriptors, a bitmap's with its place in the pool (empty when neither a slot nor a mask reads one)
	std::vector<float> pool;             // the bitmaps one behind the other, 16 bytes per texel (only when a kept texture shows one)
	std::vector<uint32_t> shapeHasUv;    // what mtsgpu_set_cloth_bsdfs checks its casts on: the flags and the extremes of every
	std::vector<double> uvRange;         // shape's texcoords (both empty without vtx_uv)
};
// the refusals of a texture call after its free, in its order, then the plan; the reason, or an empty string
std::string planTextures(const HostScene &h, const InForce &in, const TextureArgs &a, TexturePlan &out);
// the arguments of mtsgpu_set_spot_textures
struct SpotArgs {
	uint32_t n_textures = 0; const mtsgpu_uv_texture *textures = nullptr;
	uint32_t n_bitmaps = 0; const mtsgpu_bitmap *bitmaps = nullptr; const int32_t *texture_bitmap = nullptr;
	const uint32_t *texture_bilinear = nullptr;
	const int32_t *lum_texture = nullptr;
};
// ... and what it uploads (keep = false: the call switches the family off and keeps nothing)
struct SpotPlan {
	bool keep = false;
	std::vector<DTexture> desc;          // a bitmap's with its place in the pool and its filter flag (DSpots)
	std::vector<float> pool;             // the bitmaps one behind the other, 16 bytes per texel
	std::vector<float> uvFactor;         // [n_lums]: tan(cutoffAngle) of a luminaire with a texture, 0 otherwise
};
// SpotLuminaire::configure()'s m_uvFactor = std::tan(m_cutoffAngle) (spot.cpp:59) in binary32, the tangent of DESIGN.md section 5
inline float spotUvFactor(float cutoffAngle) { return dtan(cutoffAngle); }
// the refusals of mtsgpu_set_spot_textures after its free, in its order, then the plan; the reason, or an empty string.
// lumType [nLums], lumParams [nLums][MTSGPU_LUM_NPARAMS]; haveMask / haveSnow / haveCloth: what is in force in the context
std::string planSpots(uint32_t nLums, const uint32_t *lumType, const float *lumParams, const SpotArgs &a, bool haveMask, bool haveSnow,
                      bool haveCloth, SpotPlan &out);
struct ClothPlan {
	bool keep = false;
	std::vector<DWeave> weaves;
	std::vector<uint32_t> pattern;
	std::vector<DYarn> yarns;
};
// likewise mtsgpu_set_cloth_bsdfs after its free
std::string planCloth(const HostScene &h, const InForce &in, uint32_t n_weaves, const mtsgpu_weave *weaves, const int32_t *bsdf_weave, ClothPlan &out);

} // namespace mg
