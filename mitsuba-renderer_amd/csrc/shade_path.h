// shade_path.h -- K3+K5: one iteration of MIPathTracer::Li per material queue, and the kernel templates of the eight families
// (k_shade*, k_shade_all*).  Each family is instantiated by the unit that launches it: shade_plain / _vcol / _tex / _tan / _mask / _snow /
// _cloth / _spot.hip.
#pragma once
#include "shade_bsdf.h"
#include "shade_cloth.h"

namespace mg {

// BsdfCloth2 on weave k of the cloth tables: the stage of f that depends on its.uv alone, once per hit, and the two evaluations
__device__ __forceinline__ BsdfCloth::Hit cloth_prepare(const DCloths &clo, int k, float uvx, float uvy) {
	const DWeave W = clo.weaves[k];
	return BsdfCloth::prepare(W, clo.pattern + W.first_pattern, clo.yarns + W.first_yarn, uvx, uvy);
}
__device__ __forceinline__ V3 cloth_f(const DCloths &clo, int k, const BsdfCloth::Hit &H, bool two, V3 wi, V3 wo) {
	const DWeave W = clo.weaves[k];
	return BsdfCloth2::eval(two, W, clo.yarns + W.first_yarn, H, wi, wo);
}
__device__ __forceinline__ V3 cloth_sample(const DCloths &clo, int k, const BsdfCloth::Hit &H, bool two, V3 wi, float sx, float sy, V3 &wo,
                                           float &pdf, uint32_t &st) {
	const DWeave W = clo.weaves[k];
	return BsdfCloth2::sample(two, W, clo.yarns + W.first_yarn, H, wi, sx, sy, wo, pdf, st);
}

// ===========================================================================
// K3+K5: one iteration of the loop of MIPathTracer::Li (path.cpp:61-209) for
// all paths whose current hit has BSDF type BT.  The tail of the previous
// iteration (emitter hit by the BSDF sample, Russian roulette, throughput
// update; path.cpp:171-208) runs first because it needs the new hit.
// ===========================================================================
// ROUNDS: the instantiation the rounds of MIDirectIntegrator use (DConfig::dr_mode != 0); the path tracer and the
// one-sample direct integrator run the one without that code
// The iteration for ONE path (id): what it leaves behind in registers is whether the path continues and its pending
// direct-light term with the shadow ray that guards it.
// The path's 128-byte record is staged in LDS by k_shade (`row`, slot k = record slot k): ro / rd / h / T4 / L4 were
// read from it already and, for a valid hit, slots 0, 1, 3 now hold the primitive's position chunks (see k_shade).
// What changes is written back to `row`: ray_o, ray_d, bsdf when the path continues; thr, Li, misc always.
// A staged path record in LDS: slot k of lane l lives at column k ^ (l & 7) of the lane's 8-slot row when the rows
// are packed (MG_SHADE_PACKED: 128 B per lane, what 5 waves per SIMD can afford; two lanes share a bank group), or at
// column k of a 9-slot row (144 B per lane, conflict-free)
#ifndef MG_SHADE_PACKED
#define MG_SHADE_PACKED 0
#endif
constexpr int kRowStride = MG_SHADE_PACKED ? kPathSlots : kPathSlots + 1;
struct ShadeRow {
	float4 *base; uint32_t x;
	__device__ __forceinline__ float4 &operator[](int k) const { return base[MG_SHADE_PACKED ? ((uint32_t) k ^ x) : (uint32_t) k]; }
};
__device__ __forceinline__ uint32_t shade_row_index(uint32_t lane, uint32_t k) { return lane * kRowStride + (MG_SHADE_PACKED ? (k ^ (lane & 7u)) : k); }

// VCOL: kSlotColor = the instantiation for scenes with a coloured BSDF slot (DColors::bsdf_color_slots != NULL): the block the
// BSDF reads is built per hit by bsdf_block_with_color.  kSlotTexture = the one for scenes with a uv-textured slot
// (DTextures::bsdf_slot_texture != NULL), which serves coloured slots as well: bsdf_block_with_slots.  Every other scene
// (kSlotBlock) runs the instantiation without that code.  TAN: the instantiation for scenes with a tangent mesh
// (DTangents::tri_dpdu != NULL), on top of kSlotTexture: the record comes from fill_its_tan, and the texture table may be NULL.
// MSK: the instantiation for scenes with a mask adapter (DMasks::bsdf_mask != NULL), on top of TAN: the BSDF is evaluated through
// BsdfMasked with the opacity's luminance at the hit, and the tangent table may be NULL as well.
// SNW: the instantiation of bin 0 for scenes with a snow BRDF (DSnows::bsdf_snow != NULL), on top of MSK: a hit whose BSDF has a
// snow record is evaluated through BsdfSnow2, every other one as in the mask kernel, and the mask table may be NULL as well.
// SPT: the instantiation for scenes in which a spot luminaire has a projection texture (DSpots::lum_texture != NULL), on top of
// TAN and beside MSK: the luminaire sampling evaluates the texture (sample_luminaire<SKY, true>), and the tangent table may be NULL.
// CLO: the instantiation of bin 0 for scenes with a woven-cloth BRDF (DCloths::bsdf_weave != NULL), on top of SNW: a hit whose
// BSDF has a weave is evaluated through BsdfCloth2 at its.uv, every other one as in the snow kernel, and the snow table may be NULL.
template <int BT, bool ROUNDS, bool SKY, int VCOL, bool TAN = false, bool MSK = false, bool SNW = false, bool CLO = false, bool SPT = false>
__device__ __forceinline__ void shade_path(const DScene &sc, const DPaths &ps, const DConfig &cfg, const uint32_t id,
                                           const float4 ro, const float4 rd, const uint4 h, const float4 T4, const float4 L4,
                                           const ShadeRow row, bool &continues, bool &wantShadow, V3 &neeV, V3 &shO, V3 &shD, const DColors &col,
                                           const DTextures &tex, const DTangents &tan = DTangents{ nullptr, nullptr },
                                           const DMasks &msk = DMasks{ nullptr }, const DSnows &snw = DSnows{ nullptr },
                                           const DCloths &clo = DCloths{ nullptr, nullptr, nullptr, nullptr },
                                           const DSpots &spt = DSpots{ nullptr, nullptr, nullptr, nullptr }) {
	{
		// rounds of MIDirectIntegrator (DConfig::dr_mode): later BSDF samples start again from the camera hit
		const int mode = ROUNDS ? cfg.dr_mode : 0;
		const bool skipToNee = ROUNDS && mode == 1 && cfg.dr_index > 0, skipToBsdf = ROUNDS && mode == 2;
		const V3 rayO(ro.x, ro.y, ro.z), rayD(rd.x, rd.y, rd.z);
		const bool valid = h.w != kNoPrim;
		V3 thr(T4.x, T4.y, T4.z), Li(L4.x, L4.y, L4.z);
		int depth = __float_as_int(T4.w);
		uint32_t flags = __float_as_uint(L4.w);
		PathSampler smp;
		uint2 misc_zw;
		{
			const uint4 r = reinterpret_cast<const uint4 &>(row[6]);
			smp.stream = (uint64_t) r.x | ((uint64_t) r.y << 32);
			smp.slot = cfg.slot_per_path ? id : (id / cfg.spp);
			smp.j = r.z;
			misc_zw = make_uint2(r.z, r.w);
			smp.d1 = (flags >> F_D1_SHIFT) & 0xFFu; smp.d2 = (flags >> F_D2_SHIFT) & 0xFFu;
		}
		const bool direct = cfg.integrator == 1;
		// DConfig::miss_settled: while its ray was in flight the record held depth + 1, what a miss would have left.  The ray of
		// this shading hit something, so in the tail below `depth` is one ahead until the place of its depth++ (the camera ray's
		// record holds depth 1 either way)
		const bool settled = !ROUNDS && cfg.miss_settled && !direct;
		// the kernels a cylinder's hit can reach (fill_its: CYL)
		constexpr bool kCyl = BT == 0 && !MSK && !SNW && !CLO;
		Its its;
		if (valid) {
			// (a scene that is here for its masks or its textured spot alone has no tangent table)
			if (TAN && !((MSK || SPT) && tan.shape_has_tan == nullptr)) fill_its_tan<kCyl>(sc, tan, rayO, rayD, __uint_as_float(h.x), h.w, __uint_as_float(h.y), __uint_as_float(h.z), row[0], row[1], row[3], its);
			else fill_its<kCyl>(sc, rayO, rayD, __uint_as_float(h.x), h.w, __uint_as_float(h.y), __uint_as_float(h.z), row[0], row[1], row[3], its);
		}
		const int shapeLum = valid ? sc.shape_lum[its.shape] : -1;

		do {
			if (skipToNee || skipToBsdf) {
				// nothing before the sampling loops runs again
			} else if (flags & F_FIRST) {
				// rRec.rayIntersect (records.inl:89-105): alpha = 1 on a hit
				flags &= ~F_FIRST;
				if (valid) flags |= F_ALPHA;
				// while (rRec.depth <= m_maxDepth || m_maxDepth < 0) with depth == 1 (path.cpp:61): maxDepth == 0 never
				// enters the loop, the sample is black with the alpha of the camera ray
				if (!direct && !(depth <= cfg.max_depth || cfg.max_depth < 0))
					break;
			} else {
				// ---- tail of the previous iteration (path.cpp:147-208) ----
				const float4 B4 = row[5];
				const V3 bsdfVal(B4.x, B4.y, B4.z);
				const float bsdfPdf = B4.w;
				const uint32_t sampledType = flags >> F_ST_SHIFT;
				bool hitLuminaire = false;
				V3 lvalue(0, 0, 0), lp(0, 0, 0), ln(0, 0, 0);
				int llum = -1;
				if (valid) {
					if (shapeLum >= 0) {
						// LuminaireSamplingRecord(its, -ray.d); value = its.Le(-ray.d) (area.cpp:62-66)
						const float *LP = sc.lum_params + kLumStride * (size_t) shapeLum;
						lp = its.p; ln = its.geoN; llum = shapeLum;
						lvalue = (dot(-rayD, its.geoN) <= 0) ? V3(0, 0, 0) : V3(LP[0], LP[1], LP[2]);
						hitLuminaire = true;
					}
				} else {
					if (sc.background_lum >= 0) {
						llum = sc.background_lum;
						lvalue = background_le<SKY>(sc, rayD);
						hitLuminaire = true;
					} else {
						if (!direct && !settled) depth++;       // settled: the record counted this ray already
						break;
					}
				}
				if (hitLuminaire) {
					const float lumPdf = (!(sampledType & T_DELTA)) ? pdf_luminaire(sc, rayO, llum, lp, ln, -rayD) : 0.0f;
					// direct.cpp:189-191 weighs the two strategies by their sample counts
					const float weight = direct ? mi_weight(bsdfPdf * cfg.frac_bsdf, lumPdf * cfg.frac_lum) * cfg.weight_bsdf
					                            : mi_weight(bsdfPdf, lumPdf);
					Li.x += thr.x * lvalue.x * bsdfVal.x * weight;
					Li.y += thr.y * lvalue.y * bsdfVal.y * weight;
					Li.z += thr.z * lvalue.z * bsdfVal.z * weight;
				}
				if (!valid || direct)
					break;                                  // MIDirectIntegrator stops after its BSDF sample (direct.cpp:193)
				flags &= ~F_EMITTED;                       // rRec.type = ERadianceNoEmission
				if (depth >= cfg.rr_depth + (settled ? 1 : 0) && !(sampledType & T_TRANSMISSION)) {
					const float approxAlbedo = smin(0.9f, smax(smax(bsdfVal.x, bsdfVal.y), bsdfVal.z));
					if (sampler_next1d(cfg, smp) > approxAlbedo) {
						if (settled) depth--;                   // the path ends before the depth++ the record had counted
						break;
					}
					thr = thr * (1.0f / approxAlbedo);
				}
				thr = thr * bsdfVal;
				if (!settled) depth++;
				if (!(depth <= cfg.max_depth || cfg.max_depth < 0))
					break;
			}

			// ---- head of the iteration (path.cpp:62-98) ----
			if (!valid) {
				if (skipToNee || skipToBsdf) break;
				if ((flags & F_EMITTED) && sc.background_lum >= 0) {
					const V3 le = background_le<SKY>(sc, rayD);
					Li.x += thr.x * le.x; Li.y += thr.y * le.y; Li.z += thr.z * le.z;
				}
				break;
			}
			if (BT == kNumBsdfTypes)
				break;                                      // bsdf == NULL (path.cpp:72-77)
			const int bsdfIdx = sc.shape_bsdf[its.shape];
			const float *BP = sc.bsdf_params + 16 * (size_t) bsdfIdx;
			float colouredBlock[kBsdfNParams];
			// mask kernels: the Mask around this BSDF, p = opacity.getLuminance() at the hit, 1 without one (what BsdfMasked takes)
			float maskP = 1.0f;
			// snow kernels: the record of this BSDF (BsdfSnow2), kSnowNone without one
			uint32_t snowKind = kSnowNone;
			const float *snowD = nullptr;
			if (SNW && snw.bsdf_snow != nullptr) { snowKind = snw.bsdf_snow[bsdfIdx].kind; snowD = snw.bsdf_snow[bsdfIdx].derived; }
			// cloth kernels: the weave of this BSDF (BsdfCloth2) and its.uv, -1 without one
			int weaveIdx = -1;
			BsdfCloth::Hit clothHit{};
			if (CLO) {
				weaveIdx = clo.bsdf_weave[bsdfIdx];
				if (weaveIdx >= 0) {
					float clothU = 0, clothV = 0;
					its_uv<false>(sc, tex.tri_uv, h.w, its.shape, __uint_as_float(h.y), __uint_as_float(h.z), its.p, clothU, clothV);
					clothHit = cloth_prepare(clo, weaveIdx, clothU, clothV);
				}
			}
			if (VCOL == kSlotTexture && BT < 9) {
				// a checkerboard, a grid texture or a bitmap in a slot of this BSDF: that slot holds the texture's value at its.uv; a
				// `vertexcolors` texture in the other one its.color
				// (a scene that is here for its tangents alone has no texture table)
				const bool noTex = TAN && tex.bsdf_slot_texture == nullptr;
				const int k0 = noTex ? -1 : tex.bsdf_slot_texture[2 * (size_t) bsdfIdx], k1 = noTex ? -1 : tex.bsdf_slot_texture[2 * (size_t) bsdfIdx + 1];
				const uint32_t slots = col.bsdf_color_slots ? col.bsdf_color_slots[bsdfIdx] : 0u;
				float uvx = 0, uvy = 0;
				// (mask kernels: the opacity first, with its.uv computed once for the mask and the slots)
				DMask m{ kMaskNone, -1, { 0, 0, 0 }, 0u };
				// (a scene that is here for its snow alone has no mask table)
				if (MSK && !(SNW && msk.bsdf_mask == nullptr)) m = msk.bsdf_mask[bsdfIdx];
				if (k0 >= 0 || k1 >= 0 || (MSK && m.kind == kMaskTexture))
					its_uv<kCyl>(sc, tex.tri_uv, h.w, its.shape, __uint_as_float(h.y), __uint_as_float(h.z), its.p, uvx, uvy);
				if (MSK && m.kind == kMaskConstant) maskP = luminance(V3(m.opacity[0], m.opacity[1], m.opacity[2]));
				else if (MSK && m.kind == kMaskTexture) maskP = luminance(tex_eval(tex.textures[m.texture], tex.texels, uvx, uvy));
				// one slot after the other, so that only one value is alive next to the block
				const V3 zero(0, 0, 0);
				bsdf_block_with_slots<BT>(BP, kSlotBlock, kSlotBlock, zero, zero, zero, colouredBlock);
				{
					const int src = k0 >= 0 ? kSlotTexture : (slots & 1u) ? kSlotColor : kSlotBlock;
					const V3 w = src == kSlotTexture ? tex_eval(tex.textures[k0], tex.texels, uvx, uvy)
					           : src == kSlotColor ? its_color(col.tri_col, h.w, __uint_as_float(h.y), __uint_as_float(h.z)) : zero;
					bsdf_block_set_slot<BT, 0>(colouredBlock, src, w);
				}
				{
					const int src = k1 >= 0 ? kSlotTexture : (slots & 2u) ? kSlotColor : kSlotBlock;
					const V3 w = src == kSlotTexture ? tex_eval(tex.textures[k1], tex.texels, uvx, uvy)
					           : src == kSlotColor ? its_color(col.tri_col, h.w, __uint_as_float(h.y), __uint_as_float(h.z)) : zero;
					bsdf_block_set_slot<BT, 1>(colouredBlock, src, w);
				}
				BP = colouredBlock;
			} else if (VCOL == kSlotColor && BT < 9) {
				// a `vertexcolors` texture in a slot of this BSDF: that slot holds its.color for this hit
				const uint32_t slots = col.bsdf_color_slots[bsdfIdx];
				const V3 color = slots ? its_color(col.tri_col, h.w, __uint_as_float(h.y), __uint_as_float(h.z)) : V3(0, 0, 0);
				bsdf_block_with_color<BT>(BP, slots, color, colouredBlock);
				BP = colouredBlock;
			}
			const bool twoSided = (sc.bsdf_type[bsdfIdx] & 0x100u) != 0;
			const BsdfTable tab{ sc.bsdf_type, sc.bsdf_params };
			if (shapeLum >= 0 && (flags & F_EMITTED) && !(skipToNee || skipToBsdf)) {
				// Li += pathThroughput * its.Le(-ray.d) (path.cpp:80-81, area.cpp:62-66)
				const float *LP = sc.lum_params + kLumStride * (size_t) shapeLum;
				const V3 le = (dot(-rayD, its.geoN) <= 0) ? V3(0.0f, 0.0f, 0.0f) : V3(LP[0], LP[1], LP[2]);
				Li.x += thr.x * le.x; Li.y += thr.y * le.y; Li.z += thr.z * le.z;
			}
			if (!direct) {      // MonteCarloIntegrator properties; the direct integrator has neither (direct.cpp:33-41)
				if (cfg.max_depth > 0 && depth >= cfg.max_depth)
					break;
				const float wiDotGeoN = -dot(its.geoN, rayD), wiDotShN = its.wi.z;
				if (wiDotGeoN * wiDotShN < 0 && cfg.strict_normals)
					break;
			}
			const bool strict = cfg.strict_normals && !direct;

			// ---- luminaire sampling (path.cpp:100-126) ----
			if (!skipToBsdf) {
				float s0, s1;
				if (ROUNDS && direct && cfg.n_lum > 1) sampler_array2d(cfg, smp, misc_zw.y, 0, (uint32_t) cfg.dr_index, s0, s1);   // direct.cpp:122-123
				else sampler_next2d(cfg, smp, s0, s1);
				LRec lRec;
				if ((!direct || cfg.n_lum > 0) && sample_luminaire<SKY, SPT>(sc, its.p, s0, s1, lRec, spt)) {
					const V3 wo = -lRec.d;
					const V3 woL(dot(wo, its.shS), dot(wo, its.shT), dot(wo, its.shN));
					V3 bsdfVal = ((CLO && weaveIdx >= 0) ? cloth_f(clo, weaveIdx, clothHit, twoSided, its.wi, woL)
					                  : SNW ? BsdfSnow2::f(twoSided, snowKind, snowD, BP, maskP, its.wi, woL)
					                  : MSK ? BsdfMasked<BT>::f(tab, twoSided, BP, maskP, its.wi, woL) : Bsdf2<BT>::f(tab, twoSided, BP, its.wi, woL)) * fabsf(woL.z);
					const float woDotGeoN = dot(its.geoN, wo);
					if (!isZero(bsdfVal) && (!strict || woDotGeoN * woL.z > 0)) {
						// isIntersectable() || isBackgroundLuminaire() (path.cpp:118-120): 0 for delta luminaires
						const uint32_t lt = sc.lum_type[lRec.lum];      // area, constant, envmap and sky luminaires can be hit by BSDF samples
						const float bsdfPdf = (lt <= 1u || lt == 5u || (SKY && lt == 7u)) ? ((CLO && weaveIdx >= 0) ? BsdfCloth2::pdf(twoSided, its.wi, woL)
						                                                                             : SNW ? BsdfSnow2::pdf(twoSided, snowKind, snowD, BP, maskP, its.wi, woL)
						                                                                             : MSK ? BsdfMasked<BT>::pdf(tab, twoSided, BP, maskP, its.wi, woL) : Bsdf2<BT>::pdf(tab, twoSided, BP, its.wi, woL)) : 0.0f;
						const float weight = direct ? mi_weight(lRec.pdf * cfg.frac_lum, bsdfPdf * cfg.frac_bsdf) * cfg.weight_lum
						                            : mi_weight(lRec.pdf, bsdfPdf);          // direct.cpp:143-145
						// added to Li iff the segment is unoccluded: parked in the record by shade_block and cancelled by
						// k_trace<shadow>, or sent along with the shadow ray (DQueues::nee_parked)
						neeV = V3(thr.x * lRec.value.x * bsdfVal.x * weight,
						          thr.y * lRec.value.y * bsdfVal.y * weight,
						          thr.z * lRec.value.z * bsdfVal.z * weight);
						shO = its.p;
						shD = lRec.p - its.p;               // Ray(p1, p2 - p1) (scene.h:241-246)
						wantShadow = true;
					}
				}
			}

			if (mode == 1)
				break;                                      // a luminaire round ends here

			// ---- BSDF sampling (path.cpp:128-146) ----
			float s0, s1;
			if (ROUNDS && direct && cfg.n_bsdf > 1) sampler_array2d(cfg, smp, misc_zw.y, cfg.n_lum > 1 ? 1 : 0, (uint32_t) cfg.dr_index, s0, s1);   // direct.cpp:156-157
			else sampler_next2d(cfg, smp, s0, s1);
			if (direct && cfg.n_bsdf <= 0)
				break;                                      // the sample is drawn even when it is not used (direct.cpp:156-161)
			V3 woL; float bsdfPdf; uint32_t sampledType;
			V3 bsdfVal = (CLO && weaveIdx >= 0) ? cloth_sample(clo, weaveIdx, clothHit, twoSided, its.wi, s0, s1, woL, bsdfPdf, sampledType)
			           : SNW ? BsdfSnow2::sample(twoSided, snowKind, snowD, BP, maskP, its.wi, s0, s1, woL, bsdfPdf, sampledType)
			           : MSK ? BsdfMasked<BT>::sample(tab, twoSided, BP, maskP, its.wi, s0, s1, woL, bsdfPdf, sampledType)
			                 : Bsdf2<BT>::sample(tab, twoSided, BP, its.wi, s0, s1, woL, bsdfPdf, sampledType);
			if (!isZero(bsdfVal))
				bsdfVal = bsdfVal * fabsf(woL.z);          // sampleCos (bsdf.h:273-279)
			if (isZero(bsdfVal))
				break;
			bsdfVal = bsdfVal * (1.0f / bsdfPdf);
			const V3 wo(its.shS.x * woL.x + its.shT.x * woL.y + its.shN.x * woL.z,
			            its.shS.y * woL.x + its.shT.y * woL.y + its.shN.y * woL.z,
			            its.shS.z * woL.x + its.shT.z * woL.y + its.shN.z * woL.z);
			const float woDotGeoN = dot(its.geoN, wo);
			if (woDotGeoN * woL.z <= 0 && strict)
				break;
			// ray = Ray(its.p, wo, time): mint = Epsilon, maxt = inf
			row[0] = make_float4(its.p.x, its.p.y, its.p.z, kEpsilon);
			row[1] = make_float4(wo.x, wo.y, wo.z, MG_INF);
			row[5] = make_float4(bsdfVal.x, bsdfVal.y, bsdfVal.z, bsdfPdf);
			flags = (flags & 0x00FFFFFFu) | (sampledType << F_ST_SHIFT);
			continues = true;
		} while (false);
		if (!continues) { row[0] = ro; row[1] = rd; }      // a path that ends keeps its last ray (the slots held triangle data)

		flags = (flags & ~((0xFFu << F_D1_SHIFT) | (0xFFu << F_D2_SHIFT))) | (smp.d1 << F_D1_SHIFT) | (smp.d2 << F_D2_SHIFT);
		row[3] = make_float4(thr.x, thr.y, thr.z, __int_as_float(depth + ((settled && continues) ? 1 : 0)));
		row[4] = make_float4(Li.x, Li.y, Li.z, __uint_as_float(flags));
		reinterpret_cast<uint4 &>(row[6]) = make_uint4((uint32_t) (smp.stream & 0xFFFFFFFFull), (uint32_t) (smp.stream >> 32), misc_zw.x, misc_zw.y);
	}

}

#ifndef MG_SHADE_WAVES
#define MG_SHADE_WAVES 0
#endif
#if MG_SHADE_WAVES
#define MG_SHADE_BOUNDS __launch_bounds__(kShadeBlock, MG_SHADE_WAVES)
#else
#define MG_SHADE_BOUNDS __launch_bounds__(kShadeBlock)
#endif
// the workgroup's LDS: per-wave counts and the two queue offsets of the stream compaction, the staged path records
struct ShadeShared {
	uint32_t cnt[2][kShadeBlock / 64];
	uint32_t base[2];
	float4 rows[kShadeBlock / 64][64 * kRowStride];
};
// One workgroup of k_shade: the paths block * kShadeBlock .. of the material queue whose segment sizes are `prefix`
// (prefix[kBinShards] entries in kBinShards segments of bin_ids)
template <int BT, bool ROUNDS, bool SKY, int VCOL, bool TAN = false, bool MSK = false, bool SNW = false, bool CLO = false, bool SPT = false>
__device__ __forceinline__ void shade_block(const DScene &sc, const DPaths &ps, const DConfig &cfg, const DQueues &q, const uint32_t *prefix,
                                            const uint32_t *bin_ids, const uint32_t block, ShadeShared &sh, const DColors &col,
                                            const DTextures &tex = DTextures{ nullptr, nullptr, nullptr, nullptr }, const DTangents &tan = DTangents{ nullptr, nullptr },
                                            const DMasks &msk = DMasks{ nullptr }, const DSnows &snw = DSnows{ nullptr },
                                            const DCloths &clo = DCloths{ nullptr, nullptr, nullptr, nullptr },
                                            const DSpots &spt = DSpots{ nullptr, nullptr, nullptr, nullptr }) {
	uint32_t (&s_cnt)[2][kShadeBlock / 64] = sh.cnt;
	uint32_t (&s_base)[2] = sh.base;
	float4 (&s_rows)[kShadeBlock / 64][64 * kRowStride] = sh.rows;
	const uint32_t gtid = block * kShadeBlock + threadIdx.x;
	const uint32_t total = prefix[kBinShards];
	if (block * kShadeBlock >= total)
		return;                            // (uniform) a grid sized for the worst case
	const bool active = gtid < total;
	uint32_t id = 0u;
	uint4 binHit = make_uint4(0u, 0u, 0u, kNoPrim); bool haveBinHit = false;
	if (active) {
		int seg = 0;
		#pragma unroll
		for (int k = 1; k < kBinShards; ++k)
			if (gtid >= prefix[k]) seg = k;
		const size_t at = (size_t) seg * q.bin_seg_cap + (gtid - prefix[seg]);
		id = bin_ids[at];
		// the hit came with the id when the closest-hit kernel filled this bin (DQueues::bin_hits)
		if (q.bin_hits && bin_ids >= q.bins_base && bin_ids < q.bins_base + (size_t) kNumBins * q.bin_stride) {
			binHit = q.bin_hits[(size_t) (bin_ids - q.bins_base) + at]; haveBinHit = true;
		}
	}
	// ---- the path records of the wave, staged through LDS ----
	// The ids come from a material-sorted queue, so every lane owns a different 128-byte line.  Read field by field
	// that is seven 16-byte gathers per lane which each occupy the texture-address unit for 64 lines and -- the L1
	// holds 32 KB, the CU's waves hold far more lines -- mostly go to the L2 again.  Instead eight lanes fetch one
	// record together (one fully used line per request, eight records per instruction), rows of 9 float4 keep the
	// LDS accesses free of bank conflicts, and the rows are written back the same way: whole lines, coalesced.
	// All LDS traffic is private to the wave (program order suffices, no barrier).
	float4 *rows = s_rows[threadIdx.x >> 6];
	const ShadeRow row{ rows + lane_id() * kRowStride, lane_id() & 7u };
	const uint32_t sub = lane_id() & 7u, grp = lane_id() >> 3;
	const uint64_t actMask = __ballot(active);
	#pragma unroll
	for (int r = 0; r < 8; ++r) {
		const uint32_t src = grp + 8u * r;
		const uint32_t sid = (uint32_t) __shfl((int) id, (int) src);
		// whole 128-byte lines in both directions, slot 7 (the raster position, only read by the film kernels) included: only
		// the slots needed (7 read, 6 written, 3 of the triangle) cost 66 ms instead of 44 ms per frame (partial-line writes)
		if ((actMask >> src) & 1ull) rows[shade_row_index(src, sub)] = ld_stream<4>(&ps.base[(size_t) sid * kPathSlots + sub]);
	}
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
	bool continues = false, wantShadow = false;
	V3 neeV(0, 0, 0), shO(0, 0, 0), shD(0, 0, 0);      // pending direct-light term and its shadow ray
	float4 ro = make_float4(0, 0, 0, 0), rd = ro, T4 = ro, L4 = ro;
	uint4 h = make_uint4(0u, 0u, 0u, kNoPrim);
	if (active) {
		// a direct-light term the previous shading parked in slot 2 and the any-hit kernel did not cancel (DQueues::nee_parked)
		// is added before anything else of this Li iteration, where the sequential loop adds it (path.cpp:124)
		const float4 slot2 = row[2];
		L4 = settled_Li(row[4], slot2);
		h = haveBinHit ? binHit : reinterpret_cast<const uint4 &>(slot2);
		// what the write-back below leaves in slot 2: nothing while terms are parked there (unless this shading parks one,
		// see below), otherwise the hit
		if (q.nee_parked) row[2] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		else reinterpret_cast<uint4 &>(row[2]) = h;
		ro = row[0]; rd = row[1]; T4 = row[3];
		if (ROUNDS && cfg.dr_mode == 2) {
			// rounds of MIDirectIntegrator: later BSDF samples start again from the camera hit (kept in ps.prim)
			if (cfg.dr_index > 0) {
				ro = ps.prim[3 * (size_t) id]; rd = ps.prim[3 * (size_t) id + 1];
				h = reinterpret_cast<const uint4 &>(ps.prim[3 * (size_t) id + 2]);
			} else if (cfg.n_bsdf > 1) {
				ps.prim[3 * (size_t) id] = ro; ps.prim[3 * (size_t) id + 1] = rd;
				ps.prim[3 * (size_t) id + 2] = reinterpret_cast<const float4 &>(h);
			}
		}
	}
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
	// the first 64 bytes of the hit primitives' gather records (three position chunks + one of the normals), four lanes
	// per record, into row slots 0, 1, 3, 4 -- whose contents sit in registers now
	{
		const uint32_t prim = h.w;
		const uint64_t validMask = __ballot(active && prim != kNoPrim);
		const uint32_t sub4 = lane_id() & 3u, grp4 = lane_id() >> 2;
		const uint32_t slotOf = sub4 < 2u ? sub4 : sub4 + 1u;      // chunks 0, 1, 2, 3 -> slots 0, 1, 3, 4
		#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const uint32_t src = grp4 + 16u * r;
			const uint32_t sprim = (uint32_t) __shfl((int) prim, (int) src);
			if ((validMask >> src) & 1ull) rows[shade_row_index(src, slotOf)] = sc.tri_pos[(size_t) sprim * kTriStride + sub4];
		}
	}
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
	if (active)
		shade_path<BT, ROUNDS, SKY, VCOL, TAN, MSK, SNW, CLO, SPT>(sc, ps, cfg, id, ro, rd, h, T4, L4, row, continues, wantShadow, neeV, shO, shD, col, tex, tan, msk, snw, clo, spt);
	// the pending direct-light term is parked in the record with the write-back below (the line is written whole anyway):
	// the any-hit kernel clears the slot if the shadow ray is occluded, the record's next reader adds what is still there
	if (q.nee_parked && wantShadow) row[2] = make_float4(neeV.x, neeV.y, neeV.z, __uint_as_float(kNeeTag));
	__builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier();
	#pragma unroll
	for (int r = 0; r < 8; ++r) {
		const uint32_t src = grp + 8u * r;
		const uint32_t sid = (uint32_t) __shfl((int) id, (int) src);
		// whole lines again: slot 7 does not change here; slot 2 does when direct-light terms are parked in it (the term this
		// shading added has to go: every later reader would add it again; the term it parks arrives), otherwise it holds the
		// hit, unchanged
		if ((actMask >> src) & 1ull) st_stream<4>(&ps.base[(size_t) sid * kPathSlots + sub], rows[shade_row_index(src, sub)]);
	}

	// stream compaction: survivors -> next closest-hit queue, shadow rays -> shadow queue.
	// ballot + prefix popcount inside each wave, an LDS scan across the waves, ONE atomic per workgroup and queue
	// (a queue counter is a single word: every atomic on it serialises, which is why the workgroups are as large as
	// they can be: 1024 threads, 43.6 -> 41.9 ms per 64-spp frame against 512).  Measured and rejected: both queues
	// reserved with one 64-bit atomic on a shared word (43.4 ms); the reservation issued before the records are written
	// back so that its round trip hides under those stores (45 ms: the extra barrier delays the stores of every wave)
	const uint32_t wave = threadIdx.x >> 6, lane = lane_id();
	const unsigned long long mN = __ballot(continues), mS = __ballot(wantShadow);
	if (lane == 0) { s_cnt[0][wave] = (uint32_t) __popcll(mN); s_cnt[1][wave] = (uint32_t) __popcll(mS); }
	__syncthreads();
	if (threadIdx.x < 2) {
		uint32_t total = 0;
		for (int w = 0; w < kShadeBlock / 64; ++w) total += s_cnt[threadIdx.x][w];
		s_base[threadIdx.x] = total ? atomicAdd(&q.counters[threadIdx.x == 0 ? kNextWord : kShadowWord], total) : 0u;
	}
	__syncthreads();
	uint32_t offN = s_base[0], offS = s_base[1];
	for (uint32_t w = 0; w < wave; ++w) { offN += s_cnt[0][w]; offS += s_cnt[1][w]; }
	const unsigned long long below = (1ull << lane) - 1ull;
	if (continues) {
		const uint32_t pos = offN + (uint32_t) __popcll(mN & below);
		q.next[pos] = id;
		if (ps.rqn_o) {       // the new ray once more, in the order of the queue it was appended to
			st_stream<4>(&ps.rqn_o[pos], rows[shade_row_index(lane, 0)]);
			st_stream<4>(&ps.rqn_d[pos], rows[shade_row_index(lane, 1)]);
		}
	}
	if (wantShadow) {
		// the shadow ray lives in queue order (coalesced for both kernels); the path id rides in the origin's w.  The term
		// goes with it only when it is not parked in the record (DQueues::nee_parked)
		const uint32_t pos = offS + (uint32_t) __popcll(mS & below);
		st_stream<4>(&ps.shq_o[pos], make_float4(shO.x, shO.y, shO.z, __uint_as_float(id)));
		st_stream<4>(&ps.shq_d[pos], make_float4(shD.x, shD.y, shD.z, 0.0f));
		if (!q.nee_parked) st_stream<4>(&ps.shq_nee[pos], make_float4(neeV.x, neeV.y, neeV.z, __uint_as_float(id)));
	}
}

template <int BT, bool ROUNDS, bool SKY>
__global__ MG_SHADE_BOUNDS void k_shade(DScene sc, DPaths ps, DConfig cfg, DQueues q, BinView view_host,
                                                       const BinView *views_dev, const uint32_t *bin_ids) {
	__shared__ ShadeShared sh;
	// the bin's segment sizes: a kernel argument when the host read the counters back, otherwise what k_prep wrote
	shade_block<BT, ROUNDS, SKY, kSlotBlock>(sc, ps, cfg, q, views_dev ? views_dev[BT].prefix : view_host.prefix, bin_ids, blockIdx.x, sh, DColors{ nullptr, nullptr });
}
// the same for scenes with a coloured BSDF slot: the only kernels that take the colours
template <int BT, bool ROUNDS, bool SKY>
__global__ MG_SHADE_BOUNDS void k_shade_vcol(DScene sc, DPaths ps, DConfig cfg, DQueues q, BinView view_host,
                                                            const BinView *views_dev, const uint32_t *bin_ids, DColors col) {
	__shared__ ShadeShared sh;
	shade_block<BT, ROUNDS, SKY, kSlotColor>(sc, ps, cfg, q, views_dev ? views_dev[BT].prefix : view_host.prefix, bin_ids, blockIdx.x, sh, col);
}
// and for scenes with a uv-textured BSDF slot: the only kernels that take the textures
template <int BT, bool ROUNDS, bool SKY>
__global__ MG_SHADE_BOUNDS void k_shade_tex(DScene sc, DPaths ps, DConfig cfg, DQueues q, BinView view_host,
                                                           const BinView *views_dev, const uint32_t *bin_ids, DColors col, DTextures tex) {
	__shared__ ShadeShared sh;
	shade_block<BT, ROUNDS, SKY, kSlotTexture>(sc, ps, cfg, q, views_dev ? views_dev[BT].prefix : view_host.prefix, bin_ids, blockIdx.x, sh, col, tex);
}
// and for scenes with a tangent mesh (DTangents), built on the texture kernels: the only ones that take the tangents.  Bins
// 0..9: a composite (bin 9) reads no colours or textures, but its anisotropic Ward child needs the frame
template <int BT, bool ROUNDS, bool SKY>
__global__ MG_SHADE_BOUNDS void k_shade_tan(DScene sc, DPaths ps, DConfig cfg, DQueues q, BinView view_host,
                                                           const BinView *views_dev, const uint32_t *bin_ids, DColors col, DTextures tex, DTangents tan) {
	__shared__ ShadeShared sh;
	shade_block<BT, ROUNDS, SKY, kSlotTexture, true>(sc, ps, cfg, q, views_dev ? views_dev[BT].prefix : view_host.prefix, bin_ids, blockIdx.x, sh, col, tex, tan);
}
// and for scenes with a mask adapter (DMasks), built on the tangent kernels: the only ones that take the masks.  Bins 0..8: a
// composite takes no mask.  Any of the colour, texture-slot and tangent tables may be NULL here
template <int BT, bool ROUNDS, bool SKY>
__global__ MG_SHADE_BOUNDS void k_shade_msk(DScene sc, DPaths ps, DConfig cfg, DQueues q, BinView view_host,
                                                           const BinView *views_dev, const uint32_t *bin_ids, DColors col, DTextures tex, DTangents tan,
                                                           DMasks msk) {
	__shared__ ShadeShared sh;
	shade_block<BT, ROUNDS, SKY, kSlotTexture, true, true>(sc, ps, cfg, q, views_dev ? views_dev[BT].prefix : view_host.prefix, bin_ids, blockIdx.x, sh, col, tex, tan, msk);
}
// and for scenes with a snow BRDF (DSnows), built on the mask kernels: the only ones that take the snow table, its last
// argument.  Bin 0 only: a snow record sits on a Lambertian entry.  Any of the other tables may be NULL here.  Device-driven
// bounces launch this kernel next to the fused one, which then leaves bin 0 out (the composite's bin 9 is launched likewise)
template <int BT, bool ROUNDS, bool SKY>
__global__ MG_SHADE_BOUNDS void k_shade_snw(DScene sc, DPaths ps, DConfig cfg, DQueues q, BinView view_host,
                                                           const BinView *views_dev, const uint32_t *bin_ids, DColors col, DTextures tex, DTangents tan,
                                                           DMasks msk, DSnows snw) {
	static_assert(BT == 0, "a snow record sits on a Lambertian entry");
	__shared__ ShadeShared sh;
	shade_block<BT, ROUNDS, SKY, kSlotTexture, true, true, true>(sc, ps, cfg, q, views_dev ? views_dev[BT].prefix : view_host.prefix, bin_ids, blockIdx.x, sh, col, tex, tan, msk, snw);
}
// and for scenes with a woven-cloth BRDF (DCloths), built on the snow kernels: the only ones that take the cloth tables, their
// last argument.  Bin 0 only: a weave sits on a Lambertian entry.  The uv array of DTextures is never NULL here (the host
// refuses a cloth mesh without texcoords, and a table before the texture call); any other table may be.  Launched like k_shade_snw
template <int BT, bool ROUNDS, bool SKY>
__global__ MG_SHADE_BOUNDS void k_shade_clo(DScene sc, DPaths ps, DConfig cfg, DQueues q, BinView view_host,
                                                           const BinView *views_dev, const uint32_t *bin_ids, DColors col, DTextures tex, DTangents tan,
                                                           DMasks msk, DSnows snw, DCloths clo) {
	static_assert(BT == 0, "a weave sits on a Lambertian entry");
	__shared__ ShadeShared sh;
	shade_block<BT, ROUNDS, SKY, kSlotTexture, true, true, true, true>(sc, ps, cfg, q, views_dev ? views_dev[BT].prefix : view_host.prefix, bin_ids, blockIdx.x, sh, col, tex, tan, msk, snw, clo);
}
// and for scenes in which a spot luminaire has a projection texture (DSpots), built on the tangent kernels: the only ones that take
// the spot tables, their last argument.  Bins 0..9 (the terminal bin samples no luminaire).  One superset family: any of the
// colour, texture-slot and tangent tables may be NULL here.  Masks, snow and cloth are refused beside a textured spot.
// Device-driven bounces launch these kernels bin by bin instead of the fused one
template <int BT, bool ROUNDS, bool SKY>
__global__ MG_SHADE_BOUNDS void k_shade_spt(DScene sc, DPaths ps, DConfig cfg, DQueues q, BinView view_host,
                                                           const BinView *views_dev, const uint32_t *bin_ids, DColors col, DTextures tex, DTangents tan,
                                                           DSpots spt) {
	static_assert(BT < kNumBsdfTypes, "the terminal bin samples no luminaire");
	__shared__ ShadeShared sh;
	shade_block<BT, ROUNDS, SKY, kSlotTexture, true, false, false, false, true>(sc, ps, cfg, q, views_dev ? views_dev[BT].prefix : view_host.prefix, bin_ids, blockIdx.x, sh, col, tex, tan,
	                                                                            DMasks{ nullptr }, DSnows{ nullptr }, DCloths{ nullptr, nullptr, nullptr, nullptr }, spt);
}

// All material queues of a bounce in ONE launch (device-driven bounces): the workgroups are dealt to the bins in bin order,
// ceil(size / kShadeBlock) each, the sizes read from what k_prep left in device memory.  A frame of few paths is a chain of
// short launches, and a launch of k_shade -- 1024 threads and 148 KB of LDS per workgroup -- costs 10-20 us even when
// nearly all of its worst-case grid exits at once: one launch per bounce instead of one per BSDF type present.
// SKY: the launch for scenes whose background is a sky (launch_shade_all picks it): every other scene runs the instantiation
// without that code, whose registers are what they were before the sky existed.  VCOL: likewise for scenes with a coloured
// BSDF slot; the bins that cannot have one (composite, terminal) run the same code either way
template <bool SKY, int VCOL, bool TAN = false, bool MSK = false>
__device__ __forceinline__ void shade_all(const DScene &sc, const DPaths &ps, const DConfig &cfg, const DQueues &q, const BinView *views_dev, uint32_t bin_mask,
                                          ShadeShared &sh, const DColors &col, const DTextures &tex = DTextures{ nullptr, nullptr, nullptr, nullptr },
                                          const DTangents &tan = DTangents{ nullptr, nullptr }, const DMasks &msk = DMasks{ nullptr }) {
	uint32_t block = blockIdx.x;
	int bin = -1;
	for (int b = 0; b < kNumBins; ++b) {
		if (!((bin_mask >> b) & 1u)) continue;
		const uint32_t nb = (views_dev[b].prefix[kBinShards] + kShadeBlock - 1u) / kShadeBlock;
		if (block < nb) { bin = b; break; }
		block -= nb;
	}
	if (bin < 0) return;
	const uint32_t *prefix = views_dev[bin].prefix, *ids = q.bin(bin);
	switch (bin) {
		case 0: shade_block<0, false, SKY, VCOL, TAN, MSK>(sc, ps, cfg, q, prefix, ids, block, sh, col, tex, tan, msk); break;
		case 1: shade_block<1, false, SKY, VCOL, TAN, MSK>(sc, ps, cfg, q, prefix, ids, block, sh, col, tex, tan, msk); break;
		case 2: shade_block<2, false, SKY, VCOL, TAN, MSK>(sc, ps, cfg, q, prefix, ids, block, sh, col, tex, tan, msk); break;
		case 3: shade_block<3, false, SKY, VCOL, TAN, MSK>(sc, ps, cfg, q, prefix, ids, block, sh, col, tex, tan, msk); break;
		case 4: shade_block<4, false, SKY, VCOL, TAN, MSK>(sc, ps, cfg, q, prefix, ids, block, sh, col, tex, tan, msk); break;
		case 5: shade_block<5, false, SKY, VCOL, TAN, MSK>(sc, ps, cfg, q, prefix, ids, block, sh, col, tex, tan, msk); break;
		case 6: shade_block<6, false, SKY, VCOL, TAN, MSK>(sc, ps, cfg, q, prefix, ids, block, sh, col, tex, tan, msk); break;
		case 7: shade_block<7, false, SKY, VCOL, TAN, MSK>(sc, ps, cfg, q, prefix, ids, block, sh, col, tex, tan, msk); break;
		case 8: shade_block<8, false, SKY, VCOL, TAN, MSK>(sc, ps, cfg, q, prefix, ids, block, sh, col, tex, tan, msk); break;
		case 9: return;      // the composite's loop over its children is launched on its own (kShadeAllBins)
		default: shade_block<kNumBsdfTypes, false, SKY, kSlotBlock>(sc, ps, cfg, q, prefix, ids, block, sh, col); break;
	}
}
template <bool SKY>
__global__ MG_SHADE_BOUNDS void k_shade_all(DScene sc, DPaths ps, DConfig cfg, DQueues q, const BinView *views_dev, uint32_t bin_mask) {
	__shared__ ShadeShared sh;
	shade_all<SKY, kSlotBlock>(sc, ps, cfg, q, views_dev, bin_mask, sh, DColors{ nullptr, nullptr });
}
template <bool SKY>
__global__ MG_SHADE_BOUNDS void k_shade_all_vcol(DScene sc, DPaths ps, DConfig cfg, DQueues q, const BinView *views_dev, uint32_t bin_mask, DColors col) {
	__shared__ ShadeShared sh;
	shade_all<SKY, kSlotColor>(sc, ps, cfg, q, views_dev, bin_mask, sh, col);
}
template <bool SKY>
__global__ MG_SHADE_BOUNDS void k_shade_all_tex(DScene sc, DPaths ps, DConfig cfg, DQueues q, const BinView *views_dev, uint32_t bin_mask, DColors col,
                                                DTextures tex) {
	__shared__ ShadeShared sh;
	shade_all<SKY, kSlotTexture>(sc, ps, cfg, q, views_dev, bin_mask, sh, col, tex);
}
template <bool SKY>
__global__ MG_SHADE_BOUNDS void k_shade_all_tan(DScene sc, DPaths ps, DConfig cfg, DQueues q, const BinView *views_dev, uint32_t bin_mask, DColors col,
                                                DTextures tex, DTangents tan) {
	__shared__ ShadeShared sh;
	shade_all<SKY, kSlotTexture, true>(sc, ps, cfg, q, views_dev, bin_mask, sh, col, tex, tan);
}
template <bool SKY>
__global__ MG_SHADE_BOUNDS void k_shade_all_msk(DScene sc, DPaths ps, DConfig cfg, DQueues q, const BinView *views_dev, uint32_t bin_mask, DColors col,
                                                DTextures tex, DTangents tan, DMasks msk) {
	__shared__ ShadeShared sh;
	shade_all<SKY, kSlotTexture, true, true>(sc, ps, cfg, q, views_dev, bin_mask, sh, col, tex, tan, msk);
}

} // namespace mg
