// shade_bsdf.h -- device code of the shading units: intersection record, luminaires, BSDFs.  The K3+K5 kernels (shade_path.h)
// and the read-out hooks (shade_hooks.hip) run exactly this code.
#pragma once
#include "sampler.h"

namespace mg {

// ===========================================================================
// Intersection record, luminaires, BSDFs
// ===========================================================================
struct Its {
	V3 p, geoN, shS, shT, shN, wi;
	uint32_t shape;
};

// fillIntersectionRecord<true> (include/mitsuba/render/skdtree.h:352-432)
// t0, t1, t2: the first three chunks of the primitive's gather record (sc.tri_pos), fetched by the caller
// CYL: the form that knows the cylinder's record.  Only the kernels a cylinder's hit can reach have it (shade_path: the Lambertian
// bin of the families without mask, snow and cloth; the upload and those calls refuse everything else on a cylinder) and the
// read-out hooks; every other kernel is compiled without the branch and keeps the registers it had
template <bool CYL = true>
__device__ __forceinline__ void fill_its(const DScene &sc, V3 rayO, V3 rayD, float t, uint32_t prim, float u, float v,
                                         const float4 t0, const float4 t1, const float4 t2, Its &its) {
	V3 sS, sT;
	if (CYL && (__float_as_uint(t2.w) & 0xC0000000u) == 0xC0000000u) {
		// Cylinder::fillIntersectionRecord (src/shapes/cylinder.cpp:154-176): its.p = ray(t); CP = the cylinder's row of
		// shape_params: [0..11] worldToObject 3x4, [12..20] the 3x3 of objectToWorld, [21] length
		its.shape = __float_as_uint(t2.z);
		const float *CP = sc.shape_params + 24 * (size_t) its.shape;
		const float *O2W = CP + 12;
		its.p = V3(rayO.x + t * rayD.x, rayO.y + t * rayD.y, rayO.z + t * rayD.z);
		const float lx = CP[0] * its.p.x + CP[1] * its.p.y + CP[2] * its.p.z + CP[3];
		const float ly = CP[4] * its.p.x + CP[5] * its.p.y + CP[6] * its.p.z + CP[7];
		const V3 du(-ly * (2 * kPi), lx * (2 * kPi), 0 * (2 * kPi));
		const V3 dv(0.0f, 0.0f, CP[21]);
		const V3 dpdu(O2W[0] * du.x + O2W[1] * du.y + O2W[2] * du.z, O2W[3] * du.x + O2W[4] * du.y + O2W[5] * du.z,
		              O2W[6] * du.x + O2W[7] * du.y + O2W[8] * du.z);
		const V3 dpdv(O2W[0] * dv.x + O2W[1] * dv.y + O2W[2] * dv.z, O2W[3] * dv.x + O2W[4] * dv.y + O2W[5] * dv.z,
		              O2W[6] * dv.x + O2W[7] * dv.y + O2W[8] * dv.z);
		// the normal: cross(dpdu, dpdv) of the LOCAL vectors, pushed through objectToWorld as a Vector, then normalised (:169)
		const V3 cr = cross(du, dv);
		const V3 n = normalize(V3(O2W[0] * cr.x + O2W[1] * cr.y + O2W[2] * cr.z, O2W[3] * cr.x + O2W[4] * cr.y + O2W[5] * cr.z,
		                          O2W[6] * cr.x + O2W[7] * cr.y + O2W[8] * cr.z));
		sS = normalize(dpdu);
		sT = normalize(dpdv);
		its.geoN = n; its.shN = n;
	} else if (__float_as_uint(t2.w) & 0x80000000u) {
		// Sphere::fillIntersectionRecord (src/shapes/sphere.cpp:136-178): its.p = ray(t), frame from dpdu / dpdv
		its.shape = __float_as_uint(t2.z);
		const float *SP = sc.shape_params + 24 * (size_t) its.shape;
		const float *O2W = SP + 5, *W2O = SP + 14;
		const V3 center(SP[0], SP[1], SP[2]);
		const float radius = SP[3];
		its.p = V3(rayO.x + t * rayD.x, rayO.y + t * rayD.y, rayO.z + t * rayD.z);
		const V3 pc = its.p - center;
		const V3 local(W2O[0] * pc.x + W2O[1] * pc.y + W2O[2] * pc.z, W2O[3] * pc.x + W2O[4] * pc.y + W2O[5] * pc.z,
		               W2O[6] * pc.x + W2O[7] * pc.y + W2O[8] * pc.z);
		const float theta = dacos(smin(smax(local.z / radius, -1.0f), 1.0f));
		const V3 du(-local.y * (2 * kPi), local.x * (2 * kPi), 0 * (2 * kPi));
		const V3 dpdu(O2W[0] * du.x + O2W[1] * du.y + O2W[2] * du.z, O2W[3] * du.x + O2W[4] * du.y + O2W[5] * du.z,
		              O2W[6] * du.x + O2W[7] * du.y + O2W[8] * du.z);
		V3 n = normalize(pc);
		const float zrad = sqrtf(local.x * local.x + local.y * local.y);
		if (zrad > 0) {
			const float invZRad = 1.0f / zrad, cosPhi = local.x * invZRad, sinPhi = local.y * invZRad;
			float st, ct;
			dsincos(theta, st, ct);
			const V3 dv((local.z * cosPhi) * kPi, (local.z * sinPhi) * kPi, (-st * radius) * kPi);
			const V3 dpdv(O2W[0] * dv.x + O2W[1] * dv.y + O2W[2] * dv.z, O2W[3] * dv.x + O2W[4] * dv.y + O2W[5] * dv.z,
			              O2W[6] * dv.x + O2W[7] * dv.y + O2W[8] * dv.z);
			sS = normalize(dpdu);
			sT = normalize(dpdv);
		} else {
			coordinateSystem(n, sS, sT);
		}
		if (SP[4] != 0.0f)
			n = V3(n.x * -1, n.y * -1, n.z * -1);
		its.geoN = n; its.shN = n;
	} else {
	const V3 p0(t0.x, t0.y, t0.z), p1(t0.w, t1.x, t1.y), p2(t1.z, t1.w, t2.x);
	const float bx = 1 - u - v, by = u, bz = v;
	its.p = V3(p0.x * bx + p1.x * by + p2.x * bz, p0.y * bx + p1.y * by + p2.y * bz, p0.z * bx + p1.z * by + p2.z * bz);
	V3 faceNormal = cross(p1 - p0, p2 - p0);
	const float len = length(faceNormal);
	if (!isZero(faceNormal))
		faceNormal = divs(faceNormal, len);
	its.geoN = faceNormal;
	its.shape = __float_as_uint(t2.z);
	if (__float_as_uint(t2.w) & 1u) {
		const float4 *TN = sc.tri_nrm + kTriStride * (size_t) prim;
		const float4 m0 = TN[0], m1 = TN[1], m2 = TN[2];
		const V3 n0(m0.x, m0.y, m0.z), n1(m0.w, m1.x, m1.y), n2(m1.z, m1.w, m2.x);
		its.shN = normalize(V3(n0.x * bx + n1.x * by + n2.x * bz, n0.y * bx + n1.y * by + n2.y * bz, n0.z * bx + n1.z * by + n2.z * bz));
	} else {
		its.shN = its.geoN;
	}
	coordinateSystem(its.shN, sS, sT);
	}
	its.shS = sS; its.shT = sT;
	const V3 md = -rayD;
	its.wi = V3(dot(md, its.shS), dot(md, its.shT), dot(md, its.shN));
}

// The intersection record of scenes with a tangent mesh (DTangents): fill_its, and on a mesh that has tangents the shading
// frame of skdtree.h:392-399 in its operation order -- dpdu = (t0.dpdu * b.x + t1.dpdu * b.y) + t2.dpdu * b.z from the three
// vertex tangents of the primitive (DTangents::tri_dpdu), n the normalised interpolated normal fill_its has left in its.shN,
// s = normalize(dpdu - n * dot(n, dpdu)), t = cross(n, s) -- and its.wi in that frame.  Every other shape (spheres, meshes
// without tangents) keeps what fill_its wrote.  The shading kernels and the read-out hook (k_shading_frame_eval) both call this.
template <bool CYL = true>
__device__ __forceinline__ void fill_its_tan(const DScene &sc, const DTangents &tan, V3 rayO, V3 rayD, float t, uint32_t prim, float u, float v,
                                             const float4 t0, const float4 t1, const float4 t2, Its &its) {
	fill_its<CYL>(sc, rayO, rayD, t, prim, u, v, t0, t1, t2, its);
	if (!tan.shape_has_tan[its.shape]) return;
	const float4 *TD = tan.tri_dpdu + kTriDpduStride * (size_t) prim;
	const float4 d0 = TD[0], d1 = TD[1], d2 = TD[2];
	const float bx = 1 - u - v, by = u, bz = v;
	const V3 dpdu(d0.x * bx + d1.x * by + d2.x * bz, d0.y * bx + d1.y * by + d2.y * bz, d0.z * bx + d1.z * by + d2.z * bz);
	const V3 n = its.shN;
	its.shS = normalize(dpdu - n * dot(n, dpdu));
	its.shT = cross(n, its.shS);
	const V3 md = -rayD;
	its.wi = V3(dot(md, its.shS), dot(md, its.shT), dot(md, its.shN));
}

// its.color of fillIntersectionRecord (skdtree.h:364,417-421): the three vertex colours of the primitive (DColors::tri_col)
// weighted with b = ((1 - u) - v, u, v), in the reference's operation order: (c0 * b.x + c1 * b.y) + c2 * b.z per channel
__device__ __forceinline__ V3 its_color(const float4 *tri_col, uint32_t prim, float u, float v) {
	const float4 *TC = tri_col + kTriColStride * (size_t) prim;
	const float4 c0 = TC[0], c1 = TC[1], c2 = TC[2];
	const float bx = 1 - u - v, by = u, bz = v;
	return V3(c0.x * bx + c1.x * by + c2.x * bz, c0.y * bx + c1.y * by + c2.y * bz, c0.z * bx + c1.z * by + c2.z * bz);
}
// The parameter block of one hit: Q = the BSDF's block P with the texture slots named by `slots` (bit s = slot s of type BT,
// bsdf_color_slot_offset) replaced by `color` -- what a `vertexcolors` texture in that slot returns (vertexcolors.cpp:41-43).
// Every index is a compile-time constant, so Q lives in registers.  The shading kernels and the read-out hook
// (k_bsdf_eval_colored) both build their blocks here.
template <int BT>
__device__ __forceinline__ void bsdf_block_with_color(const float *P, uint32_t slots, V3 color, float (&Q)[kBsdfNParams]) {
	#pragma unroll
	for (int k = 0; k < kBsdfNParams; ++k) Q[k] = P[k];
	constexpr int o0 = bsdf_color_slot_offset(BT, 0), o1 = bsdf_color_slot_offset(BT, 1);
	if (o0 >= 0 && (slots & 1u)) { Q[o0 < 0 ? 0 : o0] = color.x; Q[o0 < 0 ? 0 : o0 + 1] = color.y; Q[o0 < 0 ? 0 : o0 + 2] = color.z; }
	if (o1 >= 0 && (slots & 2u)) { Q[o1 < 0 ? 0 : o1] = color.x; Q[o1 < 0 ? 0 : o1 + 1] = color.y; Q[o1 < 0 ? 0 : o1 + 2] = color.z; }
}

// its.uv of a hit.  Triangle mesh (skdtree.h:364,408-415): the three texcoords of the primitive (DTextures::tri_uv) weighted
// with b = ((1 - u) - v, u, v) as (t0 * b.x + t1 * b.y) + t2 * b.z per component; a mesh without texcoords has zero rows and
// gets (0, 0), the reference's value.  Sphere (sphere.cpp:136-145): spherical coordinates of the hit point p in object space,
// `local` formed as fill_its forms it.
template <bool CYL = true>
__device__ __forceinline__ void its_uv(const DScene &sc, const float4 *tri_uv, uint32_t prim, uint32_t shape, float u, float v, V3 p,
                                       float &uvx, float &uvy) {
	if (CYL && sc.shape_type[shape] == 2u) {
		// Cylinder (cylinder.cpp:158-163): uv = (local.z / length, phi / (2 * M_PI)), a division
		const float *CP = sc.shape_params + 24 * (size_t) shape;
		const float lx = CP[0] * p.x + CP[1] * p.y + CP[2] * p.z + CP[3];
		const float ly = CP[4] * p.x + CP[5] * p.y + CP[6] * p.z + CP[7];
		const float lz = CP[8] * p.x + CP[9] * p.y + CP[10] * p.z + CP[11];
		float phi = datan2(ly, lx);
		if (phi < 0) phi += 2 * kPi;
		uvx = lz / CP[21];
		uvy = phi / (2 * kPi);
	} else if (sc.shape_type[shape] == 1u) {
		const float *SP = sc.shape_params + 24 * (size_t) shape;
		const float *W2O = SP + 14;
		const V3 center(SP[0], SP[1], SP[2]);
		const float radius = SP[3];
		const V3 pc = p - center;
		const V3 local(W2O[0] * pc.x + W2O[1] * pc.y + W2O[2] * pc.z, W2O[3] * pc.x + W2O[4] * pc.y + W2O[5] * pc.z,
		               W2O[6] * pc.x + W2O[7] * pc.y + W2O[8] * pc.z);
		const float theta = dacos(smin(smax(local.z / radius, -1.0f), 1.0f));
		float phi = datan2(local.y, local.x);
		if (phi < 0) phi += 2 * kPi;
		uvx = phi * (0.5f * kInvPi);
		uvy = theta * kInvPi;
	} else {
		const float4 *TU = tri_uv + kTriUvStride * (size_t) prim;
		const float4 a = TU[0], c = TU[1];
		const float bx = 1 - u - v, by = u, bz = v;
		uvx = a.x * bx + a.z * by + c.x * bz;
		uvy = a.y * bx + a.w * by + c.y * bz;
	}
}
// MIPMap::triangle with filterType none (mipmap.cpp:228-231) and MIPMap::getTexel (:203-225) as written: the texel that holds
// uv' = (x, y), floors in binary32, integers from there on.  The out-of-range test has `x <= 0`, so column 0 counts as outside:
// harmless under repeat and clamp (modulo(0, w) = clamp(0, 0, w - 1) = 0), the constant under black and white.  modulo is the
// non-negative remainder (util.cpp:424-427).  The host has checked that the casts stay inside the int range.
__device__ __forceinline__ V3 bitmap_eval(const DTexture &t, const float4 *texels, float x, float y) {
	const int w = (int) t.width, h = (int) t.height;
	int xPos = (int) floorf(x * (float) w), yPos = (int) floorf(y * (float) h);
	if (xPos <= 0 || yPos < 0 || xPos >= w || yPos >= h) {
		if (t.wrap == kWrapRepeat) {
			xPos = xPos - (xPos / w) * w; if (xPos < 0) xPos += w;
			yPos = yPos - (yPos / h) * h; if (yPos < 0) yPos += h;
		} else if (t.wrap == kWrapClamp) {
			xPos = xPos < 0 ? 0 : xPos > w - 1 ? w - 1 : xPos;
			yPos = yPos < 0 ? 0 : yPos > h - 1 ? h - 1 : yPos;
		} else {
			const float c = t.wrap == kWrapBlack ? 0.0f : 1.0f;
			return V3(c, c, c);
		}
	}
	const float4 v = texels[(size_t) t.first + (size_t) xPos + (size_t) w * (size_t) yPos];
	return V3(v.x, v.y, v.z);
}
// MIPMap::triangle(0, x, y) of a filtered bitmap (mipmap.cpp:232-242), what LDRTexture::getValue(uv) is for filterType trilinear
// and ewa (ldrtexture.cpp:230-232): the bilinear lookup on level 0.  Four getTexel taps, each with the `x <= 0` column quirk and
// the wrap mode of bitmap_eval, summed left to right per channel.  env_triangle is this function for the envmap (repeat only).
__device__ __forceinline__ V3 bitmap_triangle(const DTexture &t, const float4 *texels, float x, float y) {
	const int w = (int) t.width, h = (int) t.height;
	x = x * w - 0.5f;
	y = y * h - 0.5f;
	const int xPos = (int) floorf(x), yPos = (int) floorf(y);
	const float dx = x - xPos, dy = y - yPos;
	V3 acc(0, 0, 0);
	#pragma unroll
	for (int k = 0; k < 4; ++k) {
		// T00 (1-dx)(1-dy) + T01 (1-dx) dy + T10 dx (1-dy) + T11 dx dy, Txy = getTexel(0, xPos + x, yPos + y)
		int tx = xPos + (k >> 1), ty = yPos + (k & 1);
		V3 texel;
		bool constant = false;
		if (tx <= 0 || ty < 0 || tx >= w || ty >= h) {
			if (t.wrap == kWrapRepeat) {
				tx = tx - (tx / w) * w; if (tx < 0) tx += w;
				ty = ty - (ty / h) * h; if (ty < 0) ty += h;
			} else if (t.wrap == kWrapClamp) {
				tx = tx < 0 ? 0 : tx > w - 1 ? w - 1 : tx;
				ty = ty < 0 ? 0 : ty > h - 1 ? h - 1 : ty;
			} else {
				const float c = t.wrap == kWrapBlack ? 0.0f : 1.0f;
				texel = V3(c, c, c);
				constant = true;
			}
		}
		if (!constant) {
			const float4 v = texels[(size_t) t.first + (size_t) tx + (size_t) w * (size_t) ty];
			texel = V3(v.x, v.y, v.z);
		}
		const float a = (k < 2) ? (1.0f - dx) : dx, b = (k & 1) ? dy : (1.0f - dy);
		const V3 term(texel.x * a * b, texel.y * a * b, texel.z * a * b);
		acc = (k == 0) ? term : V3(acc.x + term.x, acc.y + term.y, acc.z + term.z);
	}
	return acc;
}
// Texture2D::getValue(its) (texture.cpp:73-82) of a checkerboard (checkerboard.cpp:48-56), a grid texture
// (gridtexture.cpp:51-64) or an unfiltered bitmap (ldrtexture.cpp:230-232) at its.uv = (uvx, uvy).  The casts truncate towards
// zero as the reference's (int) does; the host has checked that they stay inside the int range for every texcoord of the scene
// (mtsgpu_set_uv_textures, mtsgpu_set_uv_bitmap_textures).  texels: DTextures::texels, read for a bitmap only.
__device__ __forceinline__ V3 tex_eval(const DTexture &t, const float4 *texels, float uvx, float uvy) {
	const float x = uvx * t.uscale + t.uoffset, y = uvy * t.vscale + t.voffset;
	if (t.kind == kTexBitmap) return bitmap_eval(t, texels, x, y);
	bool bright;
	if (t.kind == kTexCheckerboard) {
		// 2 * modulo(i, 2) - 1 with the non-negative remainder: +1 for an odd i, -1 for an even one
		const int cx = 2 * (((int) (x * 2)) & 1) - 1, cy = 2 * (((int) (y * 2)) & 1) - 1;
		bright = cx * cy == 1;
	} else {
		float fx = x - (float) (int) x, fy = y - (float) (int) y;
		if (fx > .5f) fx -= 1;
		if (fy > .5f) fy -= 1;
		bright = !(fabsf(fx) < t.line_width || fabsf(fy) < t.line_width);
	}
	return bright ? V3(t.bright[0], t.bright[1], t.bright[2]) : V3(t.dark[0], t.dark[1], t.dark[2]);
}
// bsdf_block_with_color for scenes with uv textures: slot S of type BT takes nothing (src = kSlotBlock) or w, which is its.color
// (kSlotColor) or the value of the slot's texture at its.uv (kSlotTexture).  Every index is a compile-time constant.  The shading
// kernels copy the block (bsdf_block_with_slots with both sources kSlotBlock) and then write one slot after the other, so that one
// value is alive at a time; the read-out hook (k_bsdf_eval_slots) hands both over at once.  Both write through bsdf_block_set_slot.
template <int BT, int S>
__device__ __forceinline__ void bsdf_block_set_slot(float (&Q)[kBsdfNParams], int src, V3 w) {
	constexpr int o = bsdf_color_slot_offset(BT, S);
	if (o >= 0 && src != kSlotBlock) { Q[o < 0 ? 0 : o] = w.x; Q[o < 0 ? 0 : o + 1] = w.y; Q[o < 0 ? 0 : o + 2] = w.z; }
}
template <int BT>
__device__ __forceinline__ void bsdf_block_with_slots(const float *P, int src0, int src1, V3 color, V3 val0, V3 val1, float (&Q)[kBsdfNParams]) {
	#pragma unroll
	for (int k = 0; k < kBsdfNParams; ++k) Q[k] = P[k];
	bsdf_block_set_slot<BT, 0>(Q, src0, src0 == kSlotColor ? color : val0);
	bsdf_block_set_slot<BT, 1>(Q, src1, src1 == kSlotColor ? color : val1);
}

struct LRec { V3 p, n, d, value; float pdf; int lum; };

// DiscretePDF::sample / sampleReuse (include/mitsuba/core/pdf.h:102-133)
__device__ __forceinline__ int dpdf_sample_reuse(const float *cdf, uint32_t n, float &sampleValue) {
	uint32_t lo = 0, count = n + 1;       // std::lower_bound over n + 1 knots
	while (count > 0) {
		const uint32_t step = count / 2, it = lo + step;
		if (cdf[it] < sampleValue) { lo = it + 1; count -= step + 1; }
		else count = step;
	}
	int index = (int) lo - 1;
	if (index < 0) index = 0;
	if (index > (int) n - 1) index = (int) n - 1;
	sampleValue = (sampleValue - cdf[index]) / (cdf[index + 1] - cdf[index]);
	return index;
}

// BSphere::rayIntersect (include/mitsuba/core/bsphere.h:85-118)
__device__ __forceinline__ bool bsphere_ray_intersect(V3 center, float radius, V3 o, V3 d, float &nearHit, float &farHit) {
	const V3 originToCenter = center - o;
	const float distToRayClosest = dot(originToCenter, d);
	const float tmp1 = dot(originToCenter, originToCenter) - radius * radius;
	if (tmp1 <= 0.0f) {
		nearHit = farHit = sqrtf(distToRayClosest * distToRayClosest - tmp1) + distToRayClosest;
		return true;
	}
	if (distToRayClosest < 0.0f)
		return false;
	const float sqrOriginToCenterLength = dot(originToCenter, originToCenter);
	const float sqrHalfChordDist = radius * radius - sqrOriginToCenterLength + distToRayClosest * distToRayClosest;
	if (sqrHalfChordDist < 0)
		return false;
	const float hitDistance = sqrtf(sqrHalfChordDist);
	nearHit = distToRayClosest - hitDistance;
	farHit = distToRayClosest + hitDistance;
	if (nearHit == 0)
		nearHit = farHit;
	return true;
}

// ---- EnvMapLuminaire (src/luminaires/envmap.cpp) ----
// MIPMap::triangle(0, x, y) with ERepeat (mipmap.cpp:226-243, getTexel :203-224)
__device__ __forceinline__ V3 env_triangle(const DScene &sc, float x, float y) {
	const int W = (int) sc.env_width, H = (int) sc.env_height;
	x = x * W - 0.5f;
	y = y * H - 0.5f;
	const int xPos = (int) floorf(x), yPos = (int) floorf(y);
	const float dx = x - xPos, dy = y - yPos;
	V3 acc(0, 0, 0);
	#pragma unroll
	for (int k = 0; k < 4; ++k) {
		int tx = xPos + (k >> 1), ty = yPos + (k & 1);
		if (tx <= 0 || ty < 0 || tx >= W || ty >= H) {
			int r = tx - (tx / W) * W; tx = (r < 0) ? r + W : r;               // modulo (util.cpp:424-427)
			r = ty - (ty / H) * H; ty = (r < 0) ? r + H : r;
		}
		const float *t = sc.env_pixels + 3 * ((size_t) tx + (size_t) W * ty);
		const float a = (k < 2) ? (1.0f - dx) : dx, b = (k & 1) ? dy : (1.0f - dy);
		const V3 term(t[0] * a * b, t[1] * a * b, t[2] * a * b);
		acc = (k == 0) ? term : V3(acc.x + term.x, acc.y + term.y, acc.z + term.z);
	}
	return acc;
}
// Le(direction) (envmap.cpp:147-153); LP = luminaire parameter block
__device__ __forceinline__ V3 env_le(const DScene &sc, const float *LP, V3 dir) {
	const float *M = LP + 7;
	const V3 d(M[0] * dir.x + M[1] * dir.y + M[2] * dir.z, M[3] * dir.x + M[4] * dir.y + M[5] * dir.z, M[6] * dir.x + M[7] * dir.y + M[8] * dir.z);
	const float u = .5f * (1 + datan2(d.x, -d.z) / kPi);
	const float v = dacos(smax(-1.0f, smin(1.0f, d.y))) / kPi;
	const V3 t = env_triangle(sc, u, v);
	return V3(t.x * LP[0], t.y * LP[0], t.z * LP[0]);
}
// pdf(p, lRec, delta) (envmap.cpp:176-193); ld = lRec.d
__device__ __forceinline__ float env_pdf(const DScene &sc, const float *LP, V3 ld) {
	const float *M = LP + 7;
	const V3 nd = -ld;
	const V3 d(M[0] * nd.x + M[1] * nd.y + M[2] * nd.z, M[3] * nd.x + M[4] * nd.y + M[5] * nd.z, M[6] * nd.x + M[7] * nd.y + M[8] * nd.z);
	const int rx = (int) sc.env_pdf_width, ry = (int) sc.env_pdf_height;
	const float x = .5f * (1 + datan2(d.x, -d.z) / kPi) * rx;
	const float y = dacos(smax(-1.0f, smin(1.0f, d.y))) / kPi * ry;
	int xPos = (int) floorf(x); xPos = xPos < 0 ? 0 : (xPos > rx - 1 ? rx - 1 : xPos);
	int yPos = (int) floorf(y); yPos = yPos < 0 ? 0 : (yPos > ry - 1 ? ry - 1 : yPos);
	const float pdf = sc.env_pdf[xPos + yPos * rx];
	const float sinTheta = sqrtf(smax(kEpsilon, 1 - d.y * d.y));
	const float psx = 2 * kPi / rx, psy = kPi / ry;
	return pdf / (psx * psy * sinTheta);
}

// ---- SkyLuminaire (src/luminaires/sky.cpp): the Preetham / Perez daylight model ----
// getDistribution (sky.cpp:451-464) with the terms all three calls share passed in: cos(theta_fin), gamma, cos(gamma);
// lam = five Perez coefficients, den = their denominator (a function of the parameters alone, derived on the host)
__device__ __forceinline__ float sky_distribution(const float *lam, float den, float cosThetaFin, float gamma, float cosGamma) {
	const float num = (1 + lam[0] * dexp(lam[1] / cosThetaFin)) * (1 + lam[2] * dexp(lam[3] * gamma) + lam[4] * cosGamma * cosGamma);
	return num / den;
}
// Le(direction) (sky.cpp:235-267, getSkySpectralRadiance :469-495, getAngleBetween :429-439); LP = the luminaire's
// parameter block, SD = what SkyLuminaire::configure() derives from it (skyConfigure, host.h).  Both are wave-uniform.
__device__ __forceinline__ V3 sky_le(const float *LP, const float *SD, V3 dir) {
	const float *M = LP + 7;
	V3 d = normalize(V3(M[0] * dir.x + M[1] * dir.y + M[2] * dir.z, M[3] * dir.x + M[4] * dir.y + M[5] * dir.z, M[6] * dir.x + M[7] * dir.y + M[8] * dir.z));
	if (LP[2] != 0.0f && d.z < 0.0f)
		return V3(0.0f, 0.0f, 0.0f);
	if (d.z < 0.001f)
		d = normalize(V3(d.x, d.y, 0.001f));
	// toSphericalCoordinates (util.cpp:618-626)
	const float theta = dacos(d.z);
	float phi = datan2(d.y, d.x);
	if (phi < 0) phi += 2 * kPi;                          // M_PI is a binary32 literal here (constants.h:45-46)
	const float thetaFin = smin(theta, (kPi * 0.5f) - 0.001f);
	// getAngleBetween(theta, phi, thetaS, phiS)
	float sinTheta, cosTheta;
	dsincos(theta, sinTheta, cosTheta);
	const float cospsi = sinTheta * SD[21] * dcos(LP[17] - phi) + cosTheta * SD[22];
	float gamma;
	if (cospsi > 1.0f) gamma = 0.0f;
	else if (cospsi < -1.0f) gamma = kPi;
	else gamma = dacos(cospsi);
	const float cosGamma = dcos(gamma), cosThetaFin = dcos(thetaFin);
	const float x = SD[0] * sky_distribution(SD + 3, SD[18], cosThetaFin, gamma, cosGamma);
	const float y = SD[1] * sky_distribution(SD + 8, SD[19], cosThetaFin, gamma, cosGamma);
	const float Y = SD[2] * sky_distribution(SD + 13, SD[20], cosThetaFin, gamma, cosGamma);
	// xyY -> XYZ
	const float yFrac = Y / y;
	const float X = yFrac * x;
	const float z = smax(0.0f, 1.0f - x - y);
	const float Z = yFrac * z;
	// Spectrum::fromXYZ, RGB (spectrum.cpp:94-98), clampNegative (spectrum.h:331-334), L *= m_skyScale
	const float r = 3.240479f * X + -1.537150f * Y + -0.498535f * Z;
	const float g = -0.969256f * X + 1.875991f * Y + 0.041556f * Z;
	const float b = 0.055648f * X + -0.204043f * Y + 1.057311f * Z;
	return V3(smax(0.0f, r) * LP[0], smax(0.0f, g) * LP[0], smax(0.0f, b) * LP[0]);
}
// SkyLuminaire::sample + sampleDirection (sky.cpp:277-281, :415-421): a uniform direction, pdf 1 / (4 pi), value Le(-d), the
// shadow ray ends at p - d * (2 radius); no bounding-sphere test, no normal.  Used by sample_luminaire and by the read-out hook.
__device__ __forceinline__ void sky_sample(const float *LP, const float *SD, V3 p, float sx, float sy, V3 &d, float &pdf, V3 &value, V3 &end) {
	d = squareToSphere(sx, sy);
	const float k = 2 * LP[6];
	pdf = 1.0f / (4 * kPi);
	value = sky_le(LP, SD, -d);
	end = V3(p.x - d.x * k, p.y - d.y * k, p.z - d.z * k);
}
// the radiance of the background luminaire along a ray that left the scene: constant.cpp:65-67, envmap.cpp:147-153, sky
template <bool SKY>
__device__ __forceinline__ V3 background_le(const DScene &sc, V3 rayD) {
	const float *LP = sc.lum_params + kLumStride * (size_t) sc.background_lum;
	if (SKY) return sky_le(LP, sc.sky, normalize(rayD));
	return (sc.lum_type[sc.background_lum] == 5u) ? env_le(sc, LP, normalize(rayD)) : V3(LP[0], LP[1], LP[2]);
}

// SpotLuminaire::falloffCurve with a projection texture (spot.cpp:87-108) for the unit direction d from the luminaire: LP = its
// parameter block, t = the texture (DSpots), uvFactor = tan(cutoffAngle).  The host has checked cutoffAngle < 90 degrees, so
// localDir.z > cosCutoff > 0 where the division happens, and that the casts of the lookup stay inside the int range.  The
// texture's value multiplies the intensity before the falloff factor does.  uvx, uvy: its.uv (0 outside the cone), for the hook
__device__ __forceinline__ V3 spot_falloff_textured(const float *LP, const DTexture &t, const float4 *texels, float uvFactor, V3 d,
                                                    float &uvx, float &uvy) {
	V3 result(LP[0], LP[1], LP[2]);
	const V3 localDir(LP[10] * d.x + LP[11] * d.y + LP[12] * d.z, LP[13] * d.x + LP[14] * d.y + LP[15] * d.z,
	                  LP[16] * d.x + LP[17] * d.y + LP[18] * d.z);
	const float cosTheta = localDir.z;
	uvx = uvy = 0.0f;
	if (cosTheta <= LP[7]) return V3(0, 0, 0);
	uvx = 0.5f + 0.5f * localDir.x / (localDir.z * uvFactor);
	uvy = 0.5f + 0.5f * localDir.y / (localDir.z * uvFactor);
	// Texture2D::getValue(its) without uv partials = getValue(uv') (texture.cpp:73-82); an ldrtexture's is MIPMap::triangle(0, ., .)
	V3 value;
	if (t.kind == kTexBitmap && t.reserved[0] == kSpotBilinear) value = bitmap_triangle(t, texels, uvx * t.uscale + t.uoffset, uvy * t.vscale + t.voffset);
	else value = tex_eval(t, texels, uvx, uvy);
	result = result * value;
	if (cosTheta >= LP[6]) return result;
	return result * ((LP[8] - dacos(cosTheta)) * LP[9]);
}

// Scene::sampleLuminaire without the visibility test (scene.cpp:396-415):
// returns true when a shadow ray has to be traced; value is already divided by pdf.
// SKY: the instantiation for scenes whose background luminaire is a sky (the only one that carries its code)
// SPT: the instantiation for scenes in which a spot luminaire has a projection texture (DSpots::lum_texture != NULL), likewise
template <bool SKY, bool SPT = false>
__device__ __forceinline__ bool sample_luminaire(const DScene &sc, V3 p, float s0, float s1, LRec &lRec,
                                                 const DSpots &spt = DSpots{ nullptr, nullptr, nullptr, nullptr }) {
	float sx = s0, sy = s1;
	const int l = dpdf_sample_reuse(sc.lum_sel_cdf, sc.n_lums, sx);
	const float lumPdf = sc.lum_sel_pdf[l];
	const float *LP = sc.lum_params + kLumStride * (size_t) l;
	if (sc.lum_type[l] == 0u && sc.shape_type[sc.lum_shape[l]] == 1u) {
		// AreaLuminaire::sample (area.cpp:68-79) -> Sphere::sampleSolidAngle (src/shapes/sphere.cpp:196-237)
		const float *SP = sc.shape_params + 24 * (size_t) sc.lum_shape[l];
		const V3 center(SP[0], SP[1], SP[2]);
		const float radius = SP[3];
		const V3 w = center - p;
		const float invDistW = 1 / length(w);
		const float squareTerm = fabsf(radius * invDistW);
		if (squareTerm >= 1 - kEpsilon) {
			// inside the sphere: uniform sampling
			const V3 d = squareToSphere(sx, sy);
			lRec.p = V3(center.x + d.x * radius, center.y + d.y * radius, center.z + d.z * radius);
			lRec.n = d;
			const V3 lumToPoint = p - lRec.p;
			const float distSquared = dot(lumToPoint, lumToPoint), dp = dot(lumToPoint, lRec.n);
			lRec.pdf = (dp > 0) ? (SP[23] * distSquared * sqrtf(distSquared) / dp) : 0.0f;
		} else {
			const float cosThetaMax = sqrtf(smax(0.0f, 1 - squareTerm * squareTerm));
			// squareToCone (util.cpp:656-662)
			const float cosTheta = (1 - sx) + sx * cosThetaMax;
			const float sinTheta = sqrtf(1 - cosTheta * cosTheta);
			const float phi = sy * (2 * kPi);
			float sphi, cphi;
			dsincos(phi, sphi, cphi);
			const V3 cone(cphi * sinTheta, sphi * sinTheta, cosTheta);
			// Frame(w * invDistW).toWorld(cone)
			const V3 fn = w * invDistW;
			V3 fs, ft;
			coordinateSystem(fn, fs, ft);
			const V3 d(fs.x * cone.x + ft.x * cone.y + fn.x * cone.z, fs.y * cone.x + ft.y * cone.y + fn.y * cone.z,
			           fs.z * cone.x + ft.z * cone.y + fn.z * cone.z);
			float t;
			if (!sphere_intersect(center, radius, p, d, 0.0f, MG_INF, t)) {
				lRec.pdf = 0.0f;         // roundoff: no sample
			} else {
				lRec.p = V3(p.x + t * d.x, p.y + t * d.y, p.z + t * d.z);
				lRec.n = normalize(lRec.p - center);
				lRec.pdf = 1 / ((2 * kPi) * (1 - cosThetaMax));
			}
		}
		lRec.d = p - lRec.p;
		if (lRec.pdf > 0 && dot(lRec.d, lRec.n) > 0) {
			lRec.value = V3(LP[0], LP[1], LP[2]);
			lRec.d = normalize(lRec.d);
		} else {
			lRec.pdf = 0;
		}
	} else if (sc.lum_type[l] == 0u) {
		// AreaLuminaire::sample (area.cpp:68-79) -> Shape::sampleSolidAngle (shape.cpp:65-75)
		// -> TriMesh::sampleArea (trimesh.cpp:297-302) -> Triangle::sample (triangle.cpp:23-47)
		const uint32_t s = (uint32_t) sc.lum_shape[l];
		const uint32_t t0 = sc.shape_tri_offset[s], nT = sc.shape_tri_offset[s + 1] - t0;
		const int index = dpdf_sample_reuse(sc.lum_tri_cdf + sc.lum_cdf_offset[l], nT, sy);
		const size_t tri = (size_t) t0 + (uint32_t) index;
		const float4 *TP = sc.tri_pos + kTriStride * tri;
		const float4 q0 = TP[0], q1 = TP[1], q2 = TP[2];
		const V3 p0(q0.x, q0.y, q0.z), p1(q0.w, q1.x, q1.y), p2(q1.z, q1.w, q2.x);
		float bx, by;
		squareToTriangle(sx, sy, bx, by);
		const V3 sideA = p1 - p0, sideB = p2 - p0;
		lRec.p = V3(p0.x + (sideA.x * bx) + (sideB.x * by), p0.y + (sideA.y * bx) + (sideB.y * by), p0.z + (sideA.z * bx) + (sideB.z * by));
		if (__float_as_uint(q2.w) & 1u) {
			const float4 *TN = sc.tri_nrm + kTriStride * tri;
			const float4 m0 = TN[0], m1 = TN[1], m2 = TN[2];
			const V3 n0(m0.x, m0.y, m0.z), n1(m0.w, m1.x, m1.y), n2(m1.z, m1.w, m2.x);
			const float b0 = 1.0f - bx - by;
			lRec.n = normalize(V3(n0.x * b0 + n1.x * bx + n2.x * by, n0.y * b0 + n1.y * bx + n2.y * by, n0.z * b0 + n1.z * bx + n2.z * by));
		} else {
			lRec.n = normalize(cross(sideA, sideB));
		}
		const float pdfArea = sc.lum_inv_area[l];
		const V3 lumToPoint = p - lRec.p;
		const float distSquared = dot(lumToPoint, lumToPoint), dp = dot(lumToPoint, lRec.n);
		lRec.pdf = (dp > 0) ? (pdfArea * distSquared * sqrtf(distSquared) / dp) : 0.0f;
		lRec.d = p - lRec.p;
		if (lRec.pdf > 0 && dot(lRec.d, lRec.n) > 0) {
			lRec.value = V3(LP[0], LP[1], LP[2]);
			lRec.d = normalize(lRec.d);
		} else {
			lRec.pdf = 0;
		}
	} else if (sc.lum_type[l] == 2u || sc.lum_type[l] == 4u) {
		// PointLuminaire::sample (point.cpp:55-63) / SpotLuminaire::sample (spot.cpp:110-118)
		const V3 pos(LP[3], LP[4], LP[5]);
		const V3 lumToP = p - pos;
		const float invDist = 1.0f / length(lumToP);
		lRec.p = pos;
		lRec.d = lumToP * invDist;
		lRec.n = V3(0, 0, 0);
		lRec.pdf = 1.0f;
		V3 result(LP[0], LP[1], LP[2]);
		if (SPT && sc.lum_type[l] == 4u && spt.lum_texture[l] >= 0) {
			float uvx, uvy;
			result = spot_falloff_textured(LP, spt.textures[spt.lum_texture[l]], spt.texels, spt.lum_uv_factor[l], lRec.d, uvx, uvy);
		} else if (sc.lum_type[l] == 4u) {
			// falloffCurve (spot.cpp:84-103), constant texture; cosTheta = m_worldToLuminaire(d).z
			const float cosTheta = LP[16] * lRec.d.x + LP[17] * lRec.d.y + LP[18] * lRec.d.z;
			if (cosTheta <= LP[7]) result = V3(0, 0, 0);
			else if (!(cosTheta >= LP[6])) result = result * ((LP[8] - dacos(cosTheta)) * LP[9]);
		}
		lRec.value = result * (invDist * invDist);
	} else if (sc.lum_type[l] == 5u) {
		// EnvMapLuminaire::sampleDirection + sample (envmap.cpp:123-145, :159-172)
		const int rx = (int) sc.env_pdf_width, ry = (int) sc.env_pdf_height;
		const int idx = dpdf_sample_reuse(sc.env_cdf, (uint32_t) (rx * ry), sx);
		float pdf = sc.env_pdf[idx];
		const int row = idx / rx, col = idx - rx * row;
		const float x = col + sx, y = row + sy;
		const V3 tv = env_triangle(sc, x * (1.0f / rx), y * (1.0f / ry));
		const float psx = 2 * kPi / rx, psy = kPi / ry;
		const float theta = psy * y, phi = psx * x - kPi;
		float sinTheta, cosTheta, sinPhi, cosPhi;
		dsincos(theta, sinTheta, cosTheta); dsincos(phi, sinPhi, cosPhi);
		pdf = pdf / (psx * psy * sinTheta);
		const float *L2W = LP + 16;
		const V3 v(-sinTheta * sinPhi, -cosTheta, sinTheta * cosPhi);
		const V3 d(L2W[0] * v.x + L2W[1] * v.y + L2W[2] * v.z, L2W[3] * v.x + L2W[4] * v.y + L2W[5] * v.z, L2W[6] * v.x + L2W[7] * v.y + L2W[8] * v.z);
		lRec.pdf = pdf;
		lRec.value = V3(tv.x * LP[0], tv.y * LP[0], tv.z * LP[0]);
		const V3 center(LP[3], LP[4], LP[5]);
		const float radius = LP[6];
		float nearHit, farHit;
		if (length(p - center) <= radius && bsphere_ray_intersect(center, radius, p, -d, nearHit, farHit)) {
			lRec.p = V3(p.x - d.x * nearHit, p.y - d.y * nearHit, p.z - d.z * nearHit);
			lRec.n = normalize(center - lRec.p);
			lRec.d = d;
		} else {
			lRec.pdf = 0.0f;
		}
	} else if (sc.lum_type[l] == 6u) {
		// CollimatedBeamLuminaire::sample (src/luminaires/collimated.cpp:62-76)
		const float *Wm = LP + 4, *Lm = LP + 16;
		const V3 local(Wm[0] * p.x + Wm[1] * p.y + Wm[2] * p.z + Wm[3], Wm[4] * p.x + Wm[5] * p.y + Wm[6] * p.z + Wm[7],
		               Wm[8] * p.x + Wm[9] * p.y + Wm[10] * p.z + Wm[11]);
		if (sqrtf(local.x * local.x + local.y * local.y) > LP[3] || local.z < 0) {
			lRec.pdf = 0.0f;
		} else {
			lRec.p = V3(Lm[0] * local.x + Lm[1] * local.y + Lm[2] * 0.0f + Lm[3], Lm[4] * local.x + Lm[5] * local.y + Lm[6] * 0.0f + Lm[7],
			            Lm[8] * local.x + Lm[9] * local.y + Lm[10] * 0.0f + Lm[11]);
			lRec.d = V3(Lm[0] * 0.0f + Lm[1] * 0.0f + Lm[2] * 1.0f, Lm[4] * 0.0f + Lm[5] * 0.0f + Lm[6] * 1.0f, Lm[8] * 0.0f + Lm[9] * 0.0f + Lm[10] * 1.0f);
			lRec.n = V3(0, 0, 0);
			lRec.pdf = 1.0f;
			lRec.value = V3(LP[0], LP[1], LP[2]);
		}
	} else if (SKY && sc.lum_type[l] == 7u) {
		sky_sample(LP, sc.sky, p, sx, sy, lRec.d, lRec.pdf, lRec.value, lRec.p);
		lRec.n = V3(0, 0, 0);
	} else if (sc.lum_type[l] == 3u) {
		// DirectionalLuminaire::sample (directional.cpp:84-91)
		const V3 dir(LP[3], LP[4], LP[5]);
		const float k = 2 * LP[6];
		lRec.p = V3(p.x - dir.x * k, p.y - dir.y * k, p.z - dir.z * k);
		lRec.d = dir;
		lRec.n = V3(0, 0, 0);
		lRec.pdf = 1.0f;
		lRec.value = V3(LP[0], LP[1], LP[2]);
	} else {
		// ConstantLuminaire::sample (constant.cpp:73-87)
		const V3 d = squareToSphere(sx, sy);
		const V3 center(LP[3], LP[4], LP[5]);
		const float radius = LP[6];
		float nearHit, farHit;
		if (length(p - center) <= radius && bsphere_ray_intersect(center, radius, p, d, nearHit, farHit)) {
			lRec.p = V3(p.x + d.x * nearHit, p.y + d.y * nearHit, p.z + d.z * nearHit);
			lRec.pdf = 1.0f / (4 * kPi);
			lRec.n = normalize(center - lRec.p);
			lRec.d = -d;
			lRec.value = V3(LP[0], LP[1], LP[2]);
		} else {
			lRec.pdf = 0.0f;
		}
	}
	if (lRec.pdf != 0) {
		lRec.pdf *= lumPdf;
		const float recip = 1.0f / lRec.pdf;
		lRec.value = lRec.value * recip;
		lRec.lum = l;
		return true;
	}
	return false;
}

// Scene::pdfLuminaire (scene.cpp:381-394); Shape::pdfSolidAngle (shape.cpp:77-83); constant.cpp:89-91
__device__ __forceinline__ float pdf_luminaire(const DScene &sc, V3 p, int lum, V3 lp, V3 ln, V3 ld) {
	const float fraction = 1.0f / sc.lum_sel_sum;
	float pdf;
	if (sc.lum_type[lum] == 0u && sc.shape_type[sc.lum_shape[lum]] == 1u) {
		// Sphere::pdfSolidAngle (sphere.cpp:239-255)
		const float *SP = sc.shape_params + 24 * (size_t) sc.lum_shape[lum];
		const V3 w = p - V3(SP[0], SP[1], SP[2]);
		const float invDistW = 1 / length(w);
		const float squareTerm = fabsf(SP[3] * invDistW);
		if (squareTerm >= 1 - kEpsilon) {
			const V3 lumToPoint = p - lp;
			const float distSquared = dot(lumToPoint, lumToPoint), dp = dot(lumToPoint, ln);
			pdf = (dp > 0) ? (SP[23] * distSquared * sqrtf(distSquared) / dp) : 0.0f;
		} else {
			const float cosThetaMax = sqrtf(smax(0.0f, 1 - squareTerm * squareTerm));
			pdf = 1 / (2 * kPi * (1 - cosThetaMax));          // squareToConePdf (util.cpp:652-654)
		}
	} else if (sc.lum_type[lum] == 0u) {
		const V3 lumToPoint = p - lp;
		const float distSquared = dot(lumToPoint, lumToPoint);
		const float invDP = smax(0.0f, sqrtf(distSquared) / dot(lumToPoint, ln));
		pdf = sc.lum_inv_area[lum] * distSquared * invDP;
	} else if (sc.lum_type[lum] == 5u) {
		pdf = env_pdf(sc, sc.lum_params + kLumStride * (size_t) lum, ld);
	} else {
		pdf = 1.0f / (4 * kPi);      // ConstantLuminaire::pdf (constant.cpp:89-91), SkyLuminaire::pdf (sky.cpp:288-292)
	}
	return pdf * fraction;
}

// --- BSDF building blocks (roughmetal.cpp:75-117 == microfacet.cpp:95-136) ---
enum : uint32_t { T_DIFFUSE_REFL = 0x1, T_DIFFUSE_TRANS = 0x2, T_DELTA_REFL = 0x4, T_DELTA_TRANS = 0x8, T_GLOSSY_REFL = 0x10, T_GLOSSY_TRANS = 0x20,
                  T_DELTA = 0xC, T_TRANSMISSION = 0x2A };

__device__ __forceinline__ float frame_tan_theta(V3 v) {      // frame.h:98-103
	const float temp = 1 - v.z * v.z;
	if (temp <= 0.0f) return 0.0f;
	return sqrtf(temp) / v.z;
}
__device__ __forceinline__ float beckmann_d(float alphaB, V3 m) {
	const float ex = frame_tan_theta(m) / alphaB;
	return dexp(-(ex * ex)) / (kPi * alphaB * alphaB * dpow4(m.z));
}
__device__ __forceinline__ V3 sample_beckmann_d(float alphaB, float sx, float sy) {
	const float thetaM = datan(sqrtf(-alphaB * alphaB * dlog(1.0f - sx)));
	const float phiM = (2.0f * kPi) * sy;
	float st, ct, sp, cp;
	dsincos(thetaM, st, ct); dsincos(phiM, sp, cp);
	return V3(st * cp, st * sp, ct);                           // sphericalDirection (util.cpp:543-550)
}
__device__ __forceinline__ float smith_g1(float alphaB, V3 v, V3 m) {
	if (dot(v, m) * v.z <= 0) return 0.0f;
	const float tanTheta = frame_tan_theta(v);
	if (tanTheta == 0.0f) return 1.0f;
	const float a = 1.0f / (alphaB * tanTheta);
	const float aSqr = a * a;
	if (a >= 1.6f) return 1.0f;
	return (3.535f * a + 2.181f * aSqr) / (1.0f + 2.276f * a + 2.577f * aSqr);
}
__device__ __forceinline__ V3 mf_reflect(V3 wi, V3 n) {
	const float s = 2.0f * dot(n, wi);
	return V3(n.x * s - wi.x, n.y * s - wi.y, n.z * s - wi.z);
}

template <int BT> struct Bsdf;

// Lambertian (src/bsdfs/lambertian.cpp:95-126)
template <> struct Bsdf<0> {
	static __device__ __forceinline__ V3 f(const float *P, V3 wi, V3 wo) {
		if (wi.z <= 0 || wo.z <= 0) return V3(0, 0, 0);
		return V3(P[0] * kInvPi, P[1] * kInvPi, P[2] * kInvPi);
	}
	static __device__ __forceinline__ float pdf(const float *P, V3 wi, V3 wo) {
		if (wi.z <= 0 || wo.z <= 0) return 0.0f;
		return wo.z * kInvPi;
	}
	static __device__ __forceinline__ V3 sample(const float *P, V3 wi, float sx, float sy, V3 &wo, float &pdf, uint32_t &st) {
		pdf = 0; st = 0; wo = V3(0, 0, 0);
		if (wi.z <= 0) return V3(0, 0, 0);
		wo = squareToHemispherePSA(sx, sy);
		st = T_DIFFUSE_REFL;
		pdf = wo.z * kInvPi;
		return V3(P[0] * kInvPi, P[1] * kInvPi, P[2] * kInvPi);
	}
};

// Dielectric (src/bsdfs/dielectric.cpp:101-107, :200-261): f = pdf = 0, delta sampling
template <> struct Bsdf<1> {
	static __device__ __forceinline__ V3 f(const float *, V3, V3) { return V3(0, 0, 0); }
	static __device__ __forceinline__ float pdf(const float *, V3, V3) { return 0.0f; }
	static __device__ __forceinline__ V3 sample(const float *P, V3 wi, float sx, float sy, V3 &wo, float &pdf, uint32_t &st) {
		const float cosThetaI = wi.z;
		float etaI = P[1], etaT = P[0];
		const bool entering = cosThetaI > 0.0f;
		if (!entering) { const float t = etaI; etaI = etaT; etaT = t; }
		const float eta = etaI / etaT, sinThetaTSqr = eta * eta * (1.0f - wi.z * wi.z);
		float Fr, cosThetaT = 0;
		if (sinThetaTSqr >= 1.0f) {
			Fr = 1.0f;
		} else {
			cosThetaT = sqrtf(1.0f - sinThetaTSqr);
			Fr = fresnelDielectric(fabsf(cosThetaI), cosThetaT, etaI, etaT);
			if (entering) cosThetaT = -cosThetaT;
		}
		if (sx <= Fr) {
			st = T_DELTA_REFL;
			wo = V3(-wi.x, -wi.y, wi.z);
			pdf = Fr * fabsf(wo.z);
			return V3(P[2] * Fr, P[3] * Fr, P[4] * Fr);
		} else {
			st = T_DELTA_TRANS;
			wo = V3(-eta * wi.x, -eta * wi.y, cosThetaT);
			pdf = (1 - Fr) * fabsf(wo.z);
			return V3(P[5] * (1 - Fr) * (eta * eta), P[6] * (1 - Fr) * (eta * eta), P[7] * (1 - Fr) * (eta * eta));
		}
	}
};

// RoughMetal (src/bsdfs/roughmetal.cpp:119-167) through BSDF::sample(bRec, pdf, s) (bsdf.cpp:37-48)
template <> struct Bsdf<2> {
	static __device__ __forceinline__ V3 f(const float *P, V3 wi, V3 wo) {
		if (wi.z <= 0 || wo.z <= 0) return V3(0, 0, 0);
		const V3 Hr = normalize(wi + wo);
		const float c = dot(wi, Hr);
		const V3 F(fresnelConductor1(c, P[1], P[4]), fresnelConductor1(c, P[2], P[5]), fresnelConductor1(c, P[3], P[6]));
		const float D = beckmann_d(P[0], Hr);
		const float G = smith_g1(P[0], wi, Hr) * smith_g1(P[0], wo, Hr);
		const float k = D * G / (4.0f * wi.z * wo.z);
		return V3(P[7] * (F.x * k), P[8] * (F.y * k), P[9] * (F.z * k));
	}
	static __device__ __forceinline__ float pdf(const float *P, V3 wi, V3 wo) {
		if (wi.z <= 0 || wo.z <= 0) return 0.0f;
		const V3 Hr = normalize(wi + wo);
		const float dwhr_dwo = 1.0f / (4.0f * fabsf(dot(wo, Hr)));
		return beckmann_d(P[0], Hr) * Hr.z * dwhr_dwo;
	}
	static __device__ __forceinline__ V3 sample(const float *P, V3 wi, float sx, float sy, V3 &wo, float &pdfv, uint32_t &st) {
		pdfv = 0; st = 0; wo = V3(0, 0, 0);
		if (wi.z <= 0) return V3(0, 0, 0);
		const V3 m = sample_beckmann_d(P[0], sx, sy);
		wo = mf_reflect(wi, m);
		st = T_GLOSSY_REFL;
		if (wo.z <= 0) return V3(0, 0, 0);
		const V3 fv = f(P, wi, wo);
		const float p = pdf(P, wi, wo);
		const V3 qv = fv * (1.0f / p);          // sample() = f / pdf; zero -> pdf 0, value 0
		if (isZero(qv)) return V3(0, 0, 0);
		pdfv = p;
		return fv;
	}
};

// Microfacet (src/bsdfs/microfacet.cpp:151-269) through BSDF::sample(bRec, pdf, s)
template <> struct Bsdf<3> {
	static __device__ __forceinline__ V3 f(const float *P, V3 wi, V3 wo) {
		if (wi.z <= 0 || wo.z <= 0) return V3(0, 0, 0);
		const float alphaB = P[0], kd = P[1], ks = P[2], intIOR = P[3], extIOR = P[4];
		const V3 Hr = normalize(wi + wo);
		const float F = fresnel(dot(wi, Hr), extIOR, intIOR);
		const float D = beckmann_d(alphaB, Hr);
		const float G = smith_g1(alphaB, wi, Hr) * smith_g1(alphaB, wo, Hr);
		const float specRef = D * G / (4.0f * wi.z * wo.z);
		const float fk = F * ks;
		V3 r(0.0f + (P[8] * specRef) * fk, 0.0f + (P[9] * specRef) * fk, 0.0f + (P[10] * specRef) * fk);
		const float dk = kInvPi * (1 - F) * kd;
		r.x += P[5] * dk; r.y += P[6] * dk; r.z += P[7] * dk;
		return r;
	}
	static __device__ __forceinline__ float pdf_spec(const float *P, V3 wi, V3 wo) {
		const V3 Hr = normalize(wi + wo);
		return beckmann_d(P[0], Hr) * Hr.z / (4.0f * fabsf(dot(wo, Hr)));
	}
	static __device__ __forceinline__ float pdf(const float *P, V3 wi, V3 wo) {
		if (wi.z <= 0 || wo.z <= 0) return 0.0f;
		const float kd = P[1], ks = P[2], intIOR = P[3], extIOR = P[4];
		float fr = fresnel(wi.z, extIOR, intIOR);
		fr = smin(smax(fr, 0.05f), 0.95f);
		const float diffuseSamplingWeight = (1 - fr) * kd;
		const float specularSamplingWeight = fr * ks;
		const float normalization = 1 / (diffuseSamplingWeight + specularSamplingWeight);
		return (specularSamplingWeight * pdf_spec(P, wi, wo) + diffuseSamplingWeight * (wo.z * kInvPi)) * normalization;
	}
	static __device__ __forceinline__ V3 sample(const float *P, V3 wi, float sx, float sy, V3 &wo, float &pdfv, uint32_t &st) {
		pdfv = 0; st = 0; wo = V3(0, 0, 0);
		if (wi.z <= 0) return V3(0, 0, 0);
		const float kd = P[1], ks = P[2], intIOR = P[3], extIOR = P[4];
		float fr = fresnel(wi.z, extIOR, intIOR);
		fr = smin(smax(fr, 0.05f), 0.95f);
		float diffuseSamplingWeight = (1 - fr) * kd;
		float specularSamplingWeight = fr * ks;
		const float normalization = 1 / (diffuseSamplingWeight + specularSamplingWeight);
		specularSamplingWeight *= normalization;
		diffuseSamplingWeight *= normalization;
		V3 qv(0, 0, 0);
		if (sx < specularSamplingWeight) {
			sx /= specularSamplingWeight;
			const V3 m = sample_beckmann_d(P[0], sx, sy);      // sampleSpecular (:203-218)
			wo = mf_reflect(wi, m);
			st = T_GLOSSY_REFL;
			if (wo.z <= 0) return V3(0, 0, 0);
			const float pdfValue = pdf(P, wi, wo);
			if (pdfValue == 0) return V3(0, 0, 0);
			qv = f(P, wi, wo) * (1.0f / pdfValue);
		} else {
			sx = (sx - specularSamplingWeight) / diffuseSamplingWeight;
			wo = squareToHemispherePSA(sx, sy);                // sampleLambertian (:224-229)
			st = T_DIFFUSE_REFL;
			qv = f(P, wi, wo) * (1.0f / pdf(P, wi, wo));
		}
		if (isZero(qv)) return V3(0, 0, 0);
		pdfv = pdf(P, wi, wo);
		return f(P, wi, wo);
	}
};

// Mirror (src/bsdfs/mirror.cpp:60-86): f = pdf = 0, delta reflection
template <> struct Bsdf<4> {
	static __device__ __forceinline__ V3 f(const float *, V3, V3) { return V3(0, 0, 0); }
	static __device__ __forceinline__ float pdf(const float *, V3, V3) { return 0.0f; }
	static __device__ __forceinline__ V3 sample(const float *P, V3 wi, float, float, V3 &wo, float &pdf, uint32_t &st) {
		wo = V3(-wi.x, -wi.y, wi.z);
		st = T_DELTA_REFL;
		pdf = fabsf(wo.z);
		return V3(P[0], P[1], P[2]);
	}
};

// Phong (src/bsdfs/phong.cpp:104-212), parameters after Phong::configure, through BSDF::sample(bRec, pdf, s)
template <> struct Bsdf<5> {
	static constexpr float kInvTwoPi = 0.15915494309189533577f;
	static __device__ __forceinline__ V3 f(const float *P, V3 wi, V3 wo) {
		if (wi.z <= 0 || wo.z <= 0) return V3(0, 0, 0);
		const V3 R(-wi.x, -wi.y, wi.z);
		const float alpha = dot(R, wo);
		float specRef;
		if (alpha <= 0.0f) specRef = 0.0f;
		else specRef = (P[0] + 2) * kInvTwoPi * dpow(alpha, P[0]) * P[2];
		V3 r(0.0f + P[8] * specRef, 0.0f + P[9] * specRef, 0.0f + P[10] * specRef);
		const float dk = kInvPi * P[1];
		r.x += P[5] * dk; r.y += P[6] * dk; r.z += P[7] * dk;
		return r;
	}
	static __device__ __forceinline__ float pdf_spec(const float *P, V3 wi, V3 wo) {
		const V3 R(-wi.x, -wi.y, wi.z);
		const float alpha = dot(R, wo);
		float specPdf = dpow(alpha, P[0]) * (P[0] + 1.0f) / (2.0f * kPi);
		if (alpha <= 0) specPdf = 0;
		return specPdf;
	}
	static __device__ __forceinline__ float pdf(const float *P, V3 wi, V3 wo) {
		if (wo.z <= 0 || wi.z <= 0) return 0.0f;
		return P[3] * pdf_spec(P, wi, wo) + P[4] * (wo.z * kInvPi);
	}
	static __device__ __forceinline__ V3 sample(const float *P, V3 wi, float sx, float sy, V3 &wo, float &pdfv, uint32_t &st) {
		pdfv = 0; st = 0; wo = V3(0, 0, 0);
		if (wi.z <= 0) return V3(0, 0, 0);
		V3 qv(0, 0, 0);
		if (sx <= P[3]) {
			sx /= P[3];
			const V3 R(-wi.x, -wi.y, wi.z);                     // sampleSpecular (:157-182)
			const float sinAlpha = sqrtf(1 - dpow(sy, 2 / (P[0] + 1)));
			const float cosAlpha = dpow(sy, 1 / (P[0] + 1));
			const float phi = (2.0f * kPi) * sx;
			float sp, cp; dsincos(phi, sp, cp);
			const V3 l(sinAlpha * cp, sinAlpha * sp, cosAlpha);
			V3 fs, ft;
			coordinateSystem(R, fs, ft);                         // Frame(R).toWorld(localDir)
			wo = V3(fs.x * l.x + ft.x * l.y + R.x * l.z, fs.y * l.x + ft.y * l.y + R.y * l.z, fs.z * l.x + ft.z * l.y + R.z * l.z);
			st = T_GLOSSY_REFL;
			if (wo.z <= 0) return V3(0, 0, 0);
			const float pdfVal = pdf(P, wi, wo);
			if (pdfVal == 0) return V3(0, 0, 0);
			qv = f(P, wi, wo) * (1.0f / pdfVal);
		} else {
			sx = (sx - P[3]) / P[4];
			wo = squareToHemispherePSA(sx, sy);                  // sampleDiffuse (:188-193)
			st = T_DIFFUSE_REFL;
			qv = f(P, wi, wo) * (1.0f / pdf(P, wi, wo));
		}
		if (isZero(qv)) return V3(0, 0, 0);
		pdfv = pdf(P, wi, wo);
		return f(P, wi, wo);
	}
};

// RoughGlass (src/bsdfs/roughglass.cpp) through BSDF::sample(bRec, pdf, s) (bsdf.cpp:37-48): the plugin's own
// 3-argument sample() takes its pdf by value (roughglass.cpp:619) and therefore does not override the virtual.
// path.cpp leaves bRec.sampler NULL (clamped Fresnel term of the surface normal), quantity = ERadiance.
// P: [0] distribution (0 beckmann, 1 phong, 2 ggx) [1] alpha [2] intIOR [3] extIOR [4..6] specRefl [7..9] specTrans
template <> struct Bsdf<6> {
	static constexpr float kInvTwoPi = 0.15915494309189533577f;
	static __device__ __forceinline__ float signum(float v) { return (v < 0) ? -1.0f : 1.0f; }
	// evalD (roughglass.cpp:213-257)
	static __device__ __forceinline__ float evalD(int distr, V3 m, float alpha) {
		if (m.z <= 0) return 0.0f;
		float result;
		if (distr == 0) {
			const float ex = frame_tan_theta(m) / alpha;
			result = dexp(-(ex * ex)) / (kPi * alpha * alpha * dpow4(m.z));
		} else if (distr == 1) {
			result = (alpha + 2) * kInvTwoPi * dpow(m.z, alpha);
		} else {
			const float tanTheta = frame_tan_theta(m), cosTheta = m.z;
			const float root = alpha / (cosTheta * cosTheta * (alpha * alpha + tanTheta * tanTheta));
			result = kInvPi * (root * root);
		}
		if ((double) result < 1e-40) result = 0;
		return result;
	}
	// sampleD (roughglass.cpp:266-293) + sphericalDirection (util.cpp:543-550)
	static __device__ __forceinline__ V3 sampleD(int distr, float sx, float sy, float alpha) {
		const float phiM = (2.0f * kPi) * sy;
		float thetaM;
		if (distr == 0) thetaM = datan(sqrtf(-alpha * alpha * dlog(1.0f - sx)));
		else if (distr == 1) thetaM = dacos(dpow(sx, (float) 1 / (alpha + 2)));
		else thetaM = datan(alpha * sqrtf(sx) / sqrtf(1.0f - sx));
		float st, ct, sp, cp;
		dsincos(thetaM, st, ct); dsincos(phiM, sp, cp);
		return V3(st * cp, st * sp, ct);
	}
	// smithG1 (roughglass.cpp:303-343)
	static __device__ __forceinline__ float smithG1(int distr, V3 v, V3 m, float alpha) {
		const float tanTheta = fabsf(frame_tan_theta(v));
		if (tanTheta == 0.0f) return 1.0f;
		if (dot(v, m) * v.z <= 0) return 0.0f;
		if (distr == 2) {
			const float root = alpha * tanTheta;
			return 2.0f / (1.0f + sqrtf(1.0f + root * root));
		}
		if (distr == 1) alpha = sqrtf(0.5f * alpha + 1) / tanTheta;     // falls through to the Beckmann case
		const float a = 1.0f / (alpha * tanTheta);
		const float aSqr = a * a;
		if (a >= 1.6f) return 1.0f;
		return (3.535f * a + 2.181f * aSqr) / (1.0f + 2.276f * a + 2.577f * aSqr);
	}
	// the half-vector of f() and pdf() (roughglass.cpp:355-377 == :417-446)
	static __device__ __forceinline__ V3 halfVector(const float *P, V3 wi, V3 wo, bool reflect, float etaI, float etaT) {
		if (reflect)
			return normalize(wo + wi) * signum(wo.z);
		const V3 n = normalize(V3(wi.x * etaI + wo.x * etaT, wi.y * etaI + wo.y * etaT, wi.z * etaI + wo.z * etaT));
		const float sgn = (P[3] > P[2]) ? 1.0f : -1.0f;
		return V3(sgn * n.x, sgn * n.y, sgn * n.z);
	}
	static __device__ __forceinline__ V3 f(const float *P, V3 wi, V3 wo) {
		const int distr = (int) P[0];
		const bool reflect = wi.z * wo.z > 0;
		float etaI = P[3], etaT = P[2];
		if (wi.z < 0) { const float t = etaI; etaI = etaT; etaT = t; }
		const V3 H = halfVector(P, wi, wo, reflect, etaI, etaT);
		const float alpha = P[1];
		const float D = evalD(distr, H, alpha);
		if (D == 0) return V3(0, 0, 0);
		const float F = fresnel(dot(wi, H), P[3], P[2]);
		const float G = smithG1(distr, wi, H, alpha) * smithG1(distr, wo, H, alpha);
		if (reflect) {
			const float value = F * D * G / (4.0f * wi.z * wo.z);
			return V3(P[4] * value, P[5] * value, P[6] * value);
		}
		const float sqrtDenom = etaI * dot(wi, H) + etaT * dot(wo, H);
		float value = ((1 - F) * D * G * etaT * etaT * dot(wi, H) * dot(wo, H)) / (wi.z * wo.z * sqrtDenom * sqrtDenom);
		value *= (etaI * etaI) / (etaT * etaT);                     // bRec.quantity == ERadiance
		const float av = fabsf(value);
		return V3(P[7] * av, P[8] * av, P[9] * av);
	}
	static __device__ __forceinline__ float pdf(const float *P, V3 wi, V3 wo) {
		const int distr = (int) P[0];
		const bool reflect = wi.z * wo.z > 0;
		float etaI = P[3], etaT = P[2];
		if (wi.z < 0) { const float t = etaI; etaI = etaT; etaT = t; }
		const V3 H = halfVector(P, wi, wo, reflect, etaI, etaT);
		float dwh_dwo;
		if (reflect) {
			dwh_dwo = 1.0f / (4.0f * dot(wo, H));
		} else {
			const float sqrtDenom = etaI * dot(wi, H) + etaT * dot(wo, H);
			dwh_dwo = (etaT * etaT * dot(wo, H)) / (sqrtDenom * sqrtDenom);
		}
		float alpha = P[1];
		alpha = alpha * (1.2f - 0.2f * sqrtf(fabsf(wi.z)));
		float prob = evalD(distr, H, alpha);
		const float F = smin(0.9f, smax(0.1f, fresnel(wi.z, P[3], P[2])));
		prob *= reflect ? F : (1 - F);
		return fabsf(prob * H.z * dwh_dwo);
	}
	// sample(bRec, sample) (roughglass.cpp:487-617), then pdf() and f() as BSDF::sample(bRec, pdf, s) does
	static __device__ __forceinline__ V3 sample(const float *P, V3 wi, float sx, float sy, V3 &wo, float &pdfv, uint32_t &st) {
		pdfv = 0; st = 0; wo = V3(0, 0, 0);
		const int distr = (int) P[0];
		bool choseReflection = true;
		float sampleF = smin(0.9f, smax(0.1f, fresnel(wi.z, P[3], P[2])));
		if (sx < sampleF) {
			sx /= sampleF;
		} else {
			sx = (sx - sampleF) / (1 - sampleF);
			choseReflection = false;
		}
		const float alpha = P[1];
		const float sampleAlpha = alpha * (1.2f - 0.2f * sqrtf(fabsf(wi.z)));
		const V3 m = sampleD(distr, sx, sy, sampleAlpha);
		V3 result;
		if (choseReflection) {
			const float k = 2 * dot(wi, m);                          // reflect (roughglass.cpp:180-182)
			wo = V3(k * m.x - wi.x, k * m.y - wi.y, k * m.z - wi.z);
			st = T_GLOSSY_REFL;
			if (wi.z * wo.z <= 0) return V3(0, 0, 0);
			result = V3(P[4], P[5], P[6]);
		} else {
			float etaI = P[3], etaT = P[2];
			if (wi.z < 0) { const float t = etaI; etaI = etaT; etaT = t; }
			const float eta = etaI / etaT, c = dot(wi, m);           // refract (roughglass.cpp:185-201)
			const float cosThetaTSqr = 1 + eta * eta * (c * c - 1);
			if (cosThetaTSqr < 0) return V3(0, 0, 0);
			const float k = eta * c - signum(wi.z) * sqrtf(cosThetaTSqr);
			wo = V3(m.x * k - wi.x * eta, m.y * k - wi.y * eta, m.z * k - wi.z * eta);
			st = T_GLOSSY_TRANS;
			if (wi.z * wo.z >= 0) return V3(0, 0, 0);
			const float scale = (etaI * etaI) / (etaT * etaT);
			result = V3(P[7] * scale, P[8] * scale, P[9] * scale);
		}
		float numerator = evalD(distr, m, alpha) * smithG1(distr, wi, m, alpha) * smithG1(distr, wo, m, alpha) * dot(wi, m);
		float denominator = evalD(distr, m, sampleAlpha) * m.z * wi.z * wo.z;
		float F = fresnel(dot(wi, m), P[3], P[2]);
		if (!choseReflection) {
			sampleF = 1 - sampleF;
			F = 1 - F;
		}
		numerator *= F;
		denominator *= sampleF;
		const float w = fabsf(numerator / denominator);
		const V3 qv(result.x * w, result.y * w, result.z * w);
		if (isZero(qv)) return V3(0, 0, 0);
		pdfv = pdf(P, wi, wo);
		return f(P, wi, wo);
	}
};

// DiffuseTransmitter (src/bsdfs/difftrans.cpp:92-131)
template <> struct Bsdf<7> {
	static __device__ __forceinline__ V3 f(const float *P, V3 wi, V3 wo) {
		if (wi.z * wo.z >= 0) return V3(0, 0, 0);
		return V3(P[0] * kInvPi, P[1] * kInvPi, P[2] * kInvPi);
	}
	static __device__ __forceinline__ float pdf(const float *, V3 wi, V3 wo) {
		if (wi.z * wo.z >= 0) return 0.0f;
		return fabsf(wo.z) * kInvPi;
	}
	static __device__ __forceinline__ V3 sample(const float *P, V3 wi, float sx, float sy, V3 &wo, float &pdfv, uint32_t &st) {
		wo = squareToHemispherePSA(sx, sy);
		if (wi.z > 0) wo.z *= -1;
		st = T_DIFFUSE_TRANS;
		pdfv = fabsf(wo.z) * kInvPi;
		if (wo.z == 0) return V3(0, 0, 0);
		return V3(P[0] * kInvPi, P[1] * kInvPi, P[2] * kInvPi);
	}
};

// Ward (src/bsdfs/ward.cpp:142-285), parameters after Ward::configure (:118-136), through BSDF::sample(bRec, pdf, s)
// (bsdf.cpp:37-48).  wi / wo are in the local frame, so alphaX != alphaY needs nothing here: the tangent comes from the shape.
// P: [0] model type (0 ward, 1 ward-duer, 2 balanced) [1] alphaX [2] alphaY [3] kd [4] ks [5] specularSamplingWeight
//    [6] diffuseSamplingWeight [7..9] diffuseReflectance [10..12] specularReflectance
template <> struct Bsdf<8> {
	static __device__ __forceinline__ V3 f(const float *P, V3 wi, V3 wo) {
		if (wi.z <= 0 || wo.z <= 0) return V3(0, 0, 0);
		const float alphaX = P[1], alphaY = P[2];
		const V3 H = wi + wo;
		const int model = (int) P[0];
		float factor1;
		if (model == 0) factor1 = 1.0f / (4.0f * kPi * alphaX * alphaY * sqrtf(wi.z * wo.z));
		else if (model == 1) factor1 = 1.0f / (4.0f * kPi * alphaX * alphaY * wi.z * wo.z);
		else factor1 = dot(H, H) / (kPi * alphaX * alphaY * dpow4(H.z));
		const float factor2 = H.x / alphaX, factor3 = H.y / alphaY;
		const float exponent = -(factor2 * factor2 + factor3 * factor3) / (H.z * H.z);
		const float specRef = factor1 * dexp(exponent) * P[4];
		V3 r(0, 0, 0);
		if (specRef > 1e-10f) r = V3(0.0f + P[10] * specRef, 0.0f + P[11] * specRef, 0.0f + P[12] * specRef);
		const float dk = kInvPi * P[3];
		r.x += P[7] * dk; r.y += P[8] * dk; r.z += P[9] * dk;
		return r;
	}
	static __device__ __forceinline__ float pdf_spec(const float *P, V3 wi, V3 wo) {       // pdfSpec (:190-199)
		const float alphaX = P[1], alphaY = P[2];
		const V3 H = normalize(wi + wo);
		const float factor1 = 1.0f / (4.0f * kPi * alphaX * alphaY * dot(H, wi) * dpow3(H.z));
		const float factor2 = H.x / alphaX, factor3 = H.y / alphaY;
		const float exponent = -(factor2 * factor2 + factor3 * factor3) / (H.z * H.z);
		return factor1 * dexp(exponent);
	}
	static __device__ __forceinline__ float pdf(const float *P, V3 wi, V3 wo) {
		if (wi.z <= 0 || wo.z <= 0) return 0.0f;
		return P[5] * pdf_spec(P, wi, wo) + P[6] * (wo.z * kInvPi);
	}
	static __device__ __forceinline__ V3 sample(const float *P, V3 wi, float sx, float sy, V3 &wo, float &pdfv, uint32_t &st) {
		pdfv = 0; st = 0; wo = V3(0, 0, 0);
		if (wi.z <= 0) return V3(0, 0, 0);
		V3 qv(0, 0, 0);
		if (sx <= P[5]) {
			sx = sx / P[5];
			const float alphaX = P[1], alphaY = P[2];                  // sampleSpecular (:222-246)
			float phiH = datan(alphaY / alphaX * dtan(2.0f * kPi * sy));
			if (sy > 0.5f) phiH += kPi;
			const float cosPhiH = dcos(phiH);
			const float sinPhiH = sqrtf(smax(0.0f, 1.0f - cosPhiH * cosPhiH));
			const float thetaH = datan(sqrtf(smax(0.0f, -dlog(sx) / ((cosPhiH * cosPhiH) / (alphaX * alphaX) + (sinPhiH * sinPhiH) / (alphaY * alphaY)))));
			float sth, cth, sph, cph;
			dsincos(thetaH, sth, cth); dsincos(phiH, sph, cph);
			const V3 H(sth * cph, sth * sph, cth);                      // sphericalDirection (util.cpp:543-550)
			const float k = 2.0f * dot(wi, H);
			wo = V3(H.x * k - wi.x, H.y * k - wi.y, H.z * k - wi.z);
			st = T_GLOSSY_REFL;
			if (wo.z <= 0.0f) return V3(0, 0, 0);
			qv = f(P, wi, wo) * (1.0f / pdf(P, wi, wo));
		} else {
			sx = (sx - P[5]) / P[6];
			wo = squareToHemispherePSA(sx, sy);                        // sampleLambertian (:252-257)
			st = T_DIFFUSE_REFL;
			qv = f(P, wi, wo) * (1.0f / pdf(P, wi, wo));
		}
		if (isZero(qv)) return V3(0, 0, 0);
		pdfv = pdf(P, wi, wo);
		return f(P, wi, wo);
	}
};

// (type 9, the composite, needs the BSDF table: BsdfT<9> below)
// "terminal" bin: never evaluated
template <> struct Bsdf<kNumBsdfTypes> {
	static __device__ __forceinline__ V3 f(const float *, V3, V3) { return V3(0, 0, 0); }
	static __device__ __forceinline__ float pdf(const float *, V3, V3) { return 0.0f; }
	static __device__ __forceinline__ V3 sample(const float *, V3, float, float, V3 &wo, float &pdf, uint32_t &st) {
		wo = V3(0, 0, 0); pdf = 0; st = 0; return V3(0, 0, 0);
	}
};

// The scene's BSDF table (DScene::bsdf_type / bsdf_params): what a composite reaches its children through
struct BsdfTable { const uint32_t *type; const float *params; };

// One interface for all types: every plugin but the composite ignores the table
template <int BT> struct BsdfT {
	static __device__ __forceinline__ V3 f(const BsdfTable &, const float *P, V3 wi, V3 wo) { return Bsdf<BT>::f(P, wi, wo); }
	static __device__ __forceinline__ float pdf(const BsdfTable &, const float *P, V3 wi, V3 wo) { return Bsdf<BT>::pdf(P, wi, wo); }
	static __device__ __forceinline__ V3 sample(const BsdfTable &, const float *P, V3 wi, float sx, float sy, V3 &wo, float &pdf, uint32_t &st) {
		return Bsdf<BT>::sample(P, wi, sx, sy, wo, pdf, st);
	}
};

// f and / or pdf of one child of a composite, with the child's own twosided adapter (twosided.cpp:80-98).  Children are
// non-delta entries of the table (mtsgpu_upload_scene checks it); anything else evaluates to zero.
template <bool WF, bool WP>
__device__ __forceinline__ void child_eval(uint32_t type, const float *P, V3 wi, V3 wo, V3 &f, float &pdf) {
	if ((type & 0x100u) && wi.z < 0) { wi.z *= -1; wo.z *= -1; }
	f = V3(0, 0, 0); pdf = 0.0f;
	#define MG_CHILD(BT) case BT: if (WF) f = Bsdf<BT>::f(P, wi, wo); if (WP) pdf = Bsdf<BT>::pdf(P, wi, wo); break
	switch (type & 0xFFu) {
		MG_CHILD(0); MG_CHILD(2); MG_CHILD(3); MG_CHILD(5); MG_CHILD(6); MG_CHILD(7); MG_CHILD(8);
		default: break;
	}
	#undef MG_CHILD
}
// sample(bRec, sample) of one child (the two-argument form composite.cpp:216 calls): the returned spectrum is zero exactly
// when that form's is (it returns f / pdf of what the three-argument form returns), the adapter flips wo back when it is
// not (twosided.cpp:100-113)
__device__ __forceinline__ V3 child_sample(uint32_t type, const float *P, V3 wi, float sx, float sy, V3 &wo, uint32_t &st) {
	bool flipped = false;
	if ((type & 0x100u) && wi.z < 0) { wi.z *= -1; flipped = true; }
	V3 r(0, 0, 0); float pdf = 0.0f;
	wo = V3(0, 0, 0); st = 0;
	#define MG_CHILD(BT) case BT: r = Bsdf<BT>::sample(P, wi, sx, sy, wo, pdf, st); break
	switch (type & 0xFFu) {
		MG_CHILD(0); MG_CHILD(2); MG_CHILD(3); MG_CHILD(5); MG_CHILD(6); MG_CHILD(7); MG_CHILD(8);
		default: break;
	}
	#undef MG_CHILD
	if (flipped && !isZero(r)) wo.z *= -1;
	return r;
}

// Composite (src/bsdfs/composite.cpp:144-229), bRec.component == -1.
// P: [0] child count n (1..MTSGPU_COMPOSITE_MAX = 7) [1..n] weights [1+n..2n] the children's indices into the BSDF table, as floats
template <> struct BsdfT<9> {
	// m_pdf.getOriginalSum(): the last knot of the running sum (pdf.h:84-87)
	static __device__ __forceinline__ float weight_sum(const float *P, int n) {
		float sum = 0.0f;
		for (int i = 0; i < n; ++i) sum = sum + P[1 + i];
		return sum;
	}
	// f = sum of w_i f_i (:144-159), pdf = sum of m_pdf[i] pdf_i (:178-193), children in table order
	template <bool WF, bool WP>
	static __device__ __forceinline__ void eval(const BsdfTable &tab, const float *P, V3 wi, V3 wo, V3 &f, float &pdf) {
		const int n = (int) P[0];
		const float sum = weight_sum(P, n);
		f = V3(0, 0, 0); pdf = 0.0f;
		#pragma unroll 1
		for (int i = 0; i < n; ++i) {
			const uint32_t c = (uint32_t) P[1 + n + i];
			const float w = P[1 + i];
			V3 cf; float cp;
			child_eval<WF, WP>(tab.type[c], tab.params + kBsdfNParams * (size_t) c, wi, wo, cf, cp);
			if (WF) { f.x += cf.x * w; f.y += cf.y * w; f.z += cf.z * w; }
			if (WP) pdf += cp * (w / sum);                          // m_pdf[i] after DiscretePDF::build (pdf.h:88-91)
		}
	}
	static __device__ __forceinline__ V3 f(const BsdfTable &tab, const float *P, V3 wi, V3 wo) {
		V3 fv; float pv; eval<true, false>(tab, P, wi, wo, fv, pv); return fv;
	}
	static __device__ __forceinline__ float pdf(const BsdfTable &tab, const float *P, V3 wi, V3 wo) {
		V3 fv; float pv; eval<false, true>(tab, P, wi, wo, fv, pv); return pv;
	}
	// sample(bRec, pdf, sample) (:212-229): sampleReuse picks the child, its sample() the direction, then pdf and f of the WHOLE
	static __device__ __forceinline__ V3 sample(const BsdfTable &tab, const float *P, V3 wi, float sx, float sy, V3 &wo, float &pdfv, uint32_t &st) {
		pdfv = 0; st = 0; wo = V3(0, 0, 0);
		const int n = (int) P[0];
		const float sum = weight_sum(P, n);
		// DiscretePDF::sample (pdf.h:102-107): std::lower_bound over the n + 1 knots m_cdf[i] = (w_0 + .. + w_(i-1)) / sum, m_cdf[n] = 1
		int it = n + 1;
		float acc = 0.0f;
		for (int i = 0; i <= n; ++i) {
			const float knot = (i == n) ? 1.0f : acc / sum;
			if (it > n && !(knot < sx)) it = i;
			if (i < n) acc = acc + P[1 + i];
		}
		int entry = it - 1;
		if (entry < 0) entry = 0;
		if (entry > n - 1) entry = n - 1;
		// sampleReuse (pdf.h:128-133)
		float lo = 0.0f;
		for (int i = 0; i < entry; ++i) lo = lo + P[1 + i];
		const float hi = (entry + 1 == n) ? 1.0f : (lo + P[1 + entry]) / sum;
		lo = lo / sum;
		sx = (sx - lo) / (hi - lo);
		const uint32_t c = (uint32_t) P[1 + n + entry];
		const V3 r = child_sample(tab.type[c], tab.params + kBsdfNParams * (size_t) c, wi, sx, sy, wo, st);
		if (isZero(r)) { wo = V3(0, 0, 0); st = 0; return V3(0, 0, 0); }      // sampling failed (:218-219)
		V3 fv;
		eval<true, true>(tab, P, wi, wo, fv, pdfv);
		return fv;
	}
};

// TwoSidedBRDF adapter (src/bsdfs/twosided.cpp:80-130) around any BSDF whose type carries MTSGPU_BSDF_TWOSIDED
template <int BT> struct Bsdf2 {
	static __device__ __forceinline__ V3 f(const BsdfTable &tab, bool two, const float *P, V3 wi, V3 wo) {
		if (two && wi.z < 0) { wi.z *= -1; wo.z *= -1; }
		return BsdfT<BT>::f(tab, P, wi, wo);
	}
	static __device__ __forceinline__ float pdf(const BsdfTable &tab, bool two, const float *P, V3 wi, V3 wo) {
		if (two && wi.z < 0) { wi.z *= -1; wo.z *= -1; }
		return BsdfT<BT>::pdf(tab, P, wi, wo);
	}
	static __device__ __forceinline__ V3 sample(const BsdfTable &tab, bool two, const float *P, V3 wi, float sx, float sy, V3 &wo, float &pdf, uint32_t &st) {
		bool flipped = false;
		if (two && wi.z < 0) { wi.z *= -1; flipped = true; }
		const V3 result = BsdfT<BT>::sample(tab, P, wi, sx, sy, wo, pdf, st);
		if (flipped && !isZero(result) && pdf != 0) wo.z *= -1;
		return result;
	}
};

// Spectrum::getLuminance of an RGB build (spectrum.h:387-389)
__device__ __forceinline__ float luminance(V3 c) {
	return (c.x * 0.212671f + c.y * 0.715160f) + c.z * 0.072169f;
}
// Mask adapter (src/bsdfs/mask.cpp:73-161) around Bsdf2<BT>, typeMask = EAll and component = -1: with probability p =
// opacity.getLuminance() the nested BSDF, otherwise the ray passes straight through as a delta transmission.  Nothing clamps p;
// p == 0 with sx == 0 divides 0 by 0 as the reference does.  The mask kernels (k_shade_msk, k_shade_all_msk) and the read-out
// hook (k_bsdf_eval_masked) both call this.
template <int BT> struct BsdfMasked {
	static __device__ __forceinline__ V3 f(const BsdfTable &tab, bool two, const float *P, float p, V3 wi, V3 wo) {
		return Bsdf2<BT>::f(tab, two, P, wi, wo) * p;
	}
	static __device__ __forceinline__ float pdf(const BsdfTable &tab, bool two, const float *P, float p, V3 wi, V3 wo) {
		return Bsdf2<BT>::pdf(tab, two, P, wi, wo) * p;
	}
	static __device__ __forceinline__ V3 sample(const BsdfTable &tab, bool two, const float *P, float p, V3 wi, float sx, float sy, V3 &wo, float &pdf,
	                                            uint32_t &st) {
		if (sx <= p) {
			const V3 result = Bsdf2<BT>::sample(tab, two, P, wi, sx / p, sy, wo, pdf, st) * p;
			pdf *= p;
			return result;
		}
		wo = V3(-wi.x, -wi.y, -wi.z);
		st = T_DELTA_TRANS;
		pdf = (1 - p) * fabsf(wo.z);
		return V3(1 - p, 1 - p, 1 - p);
	}
};

// The snow BRDFs of the reference, Wiscombe (src/bsdfs/wiscombe.cpp:108-166) and HanrahanKrueger
// (src/bsdfs/hanrahan-krueger.cpp:134-214), as written, quirks included.  Both sample like the Lambertian; D is the record's
// `derived` (mtsgpu_snow.h has the layout).  kSnowNone is Bsdf<0> on the block P, so a queue may mix Lambertian and snow hits.
// f, pdf and the sample-with-pdf form are what the integrators call (path.cpp:109,120,135).  The snow kernels (k_shade_snw) and
// the read-out hook (k_bsdf_eval_snow) both call this.
struct BsdfSnow {
	// Wiscombe::reflectance (:122-127) = albedo(mu0) * fBar * INV_PI; albedo (:133-135) is two component-wise divisions.
	// b = 1.07 * mu0 - 0.84 is binary64 (the literals), rounded once
	static __device__ __forceinline__ V3 wiscombe_reflectance(const float *D, float mu0, float muPrime) {
		const float b = (float) (1.07 * (double) mu0 - 0.84);
		const float fBar = (3.0f / (3.0f - b)) * (1.0f + b * (muPrime - 1.0f));
		float R[3];
		#pragma unroll
		for (int k = 0; k < 3; ++k) {
			const float wStar = D[k], bStar = D[3 + k], xi = D[6 + k], Pk = D[9 + k];
			const float albedo = (wStar / (1.0f + Pk)) * ((1.0f - xi * mu0 * bStar) / (1.0f + xi * mu0));
			R[k] = albedo * fBar * kInvPi;
		}
		return V3(R[0], R[1], R[2]);
	}
	// HanrahanKrueger::radiance (:171-193) with hgPhaseFunction (:140-147).  std::pow(base, 1.5) is base * sqrt(base) in
	// binary64 with the correctly rounded sqrt, rounded once to binary32
	static __device__ __forceinline__ V3 hk_radiance(const float *D, V3 wi, V3 wo) {
		const float cos_wi = wi.z, cos_wo = wo.z;
		const float g = D[9], eta = D[10];
		const float Ft1 = 1.0f - fresnel(cos_wo, 1.0f, eta);
		const float Ft2 = 1.0f - fresnel(cos_wi, 1.0f, eta);
		const float F = Ft1 * Ft2;
		const float costheta = dot(-wi, wo);
		const float gSq = g * g;
		const float num = (float) (1.0 - (double) gSq);
		const double base = 1.0 + (double) gSq - 2.0 * (double) g * (double) costheta;
		const float den = (float) (base * sqrt(base));
		const float p = (float) (0.5 * (double) (num / den));
		const float recip = 1.0f / (fabsf(cos_wi) + fabsf(cos_wo));      // Spectrum / Float (spectrum.h:229-243)
		float Lo[3];
		#pragma unroll
		for (int k = 0; k < 3; ++k) {
			const float f1 = D[k] * F * p * recip;
			Lo[k] = D[3 + k] * f1;
			if (D[11] != 0.0f) Lo[k] += D[6 + k] * F * kInvPi;
		}
		return V3(Lo[0], Lo[1], Lo[2]);
	}
	static __device__ __forceinline__ V3 f(uint32_t kind, const float *D, const float *P, V3 wi, V3 wo) {
		if (kind == kSnowNone) return Bsdf<0>::f(P, wi, wo);
		if (wi.z <= 0 || wo.z <= 0) return V3(0, 0, 0);
		// Wiscombe: mu0 = cosTheta(wo), muPrime = cosTheta(wi), and a second 1 / pi (:113-115)
		if (kind == kSnowWiscombe) return wiscombe_reflectance(D, wo.z, wi.z) * kInvPi;
		return hk_radiance(D, wi, wo) * kInvPi;
	}
	static __device__ __forceinline__ float pdf(uint32_t kind, const float *D, const float *P, V3 wi, V3 wo) {
		return Bsdf<0>::pdf(P, wi, wo);      // wiscombe.cpp:137-141, hanrahan-krueger.cpp:162-166: the Lambertian's
	}
	static __device__ __forceinline__ V3 sample(uint32_t kind, const float *D, const float *P, V3 wi, float sx, float sy, V3 &wo, float &pdf,
	                                            uint32_t &st) {
		if (kind == kSnowNone) return Bsdf<0>::sample(P, wi, sx, sy, wo, pdf, st);
		pdf = 0; st = 0; wo = V3(0, 0, 0);
		if (wi.z <= 0) return V3(0, 0, 0);
		wo = squareToHemispherePSA(sx, sy);
		st = T_DIFFUSE_REFL;
		pdf = wo.z * kInvPi;
		// Wiscombe: muPrime = |cosTheta(wi)|, one 1 / pi (:163-165); HanrahanKrueger: radiance * INV_PI (:213)
		if (kind == kSnowWiscombe) return wiscombe_reflectance(D, wo.z, fabsf(wi.z));
		return hk_radiance(D, wi, wo) * kInvPi;
	}
};
// BsdfSnow behind the TwoSidedBRDF adapter of Bsdf2 and the Mask adapter of BsdfMasked (p = 1 without a mask: a snow entry
// has none, a Lambertian of the same queue may)
struct BsdfSnow2 {
	static __device__ __forceinline__ V3 f(bool two, uint32_t kind, const float *D, const float *P, float p, V3 wi, V3 wo) {
		if (two && wi.z < 0) { wi.z *= -1; wo.z *= -1; }
		return BsdfSnow::f(kind, D, P, wi, wo) * p;
	}
	static __device__ __forceinline__ float pdf(bool two, uint32_t kind, const float *D, const float *P, float p, V3 wi, V3 wo) {
		if (two && wi.z < 0) { wi.z *= -1; wo.z *= -1; }
		return BsdfSnow::pdf(kind, D, P, wi, wo) * p;
	}
	static __device__ __forceinline__ V3 sample(bool two, uint32_t kind, const float *D, const float *P, float p, V3 wi, float sx, float sy, V3 &wo,
	                                            float &pdf, uint32_t &st) {
		if (sx <= p) {
			bool flipped = false;
			if (two && wi.z < 0) { wi.z *= -1; flipped = true; }
			const V3 result = BsdfSnow::sample(kind, D, P, wi, sx / p, sy, wo, pdf, st);
			if (flipped && !isZero(result) && pdf != 0) wo.z *= -1;
			pdf *= p;
			return result * p;
		}
		wo = V3(-wi.x, -wi.y, -wi.z);
		st = T_DELTA_TRANS;
		pdf = (1 - p) * fabsf(wo.z);
		return V3(1 - p, 1 - p, 1 - p);
	}
};

__device__ __forceinline__ float mi_weight(float pdfA, float pdfB) {     // path.cpp:218-222
	pdfA *= pdfA;
	pdfB *= pdfB;
	return pdfA / (pdfA + pdfB);
}

} // namespace mg
