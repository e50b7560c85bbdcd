// shade_hooks.hip -- the code of shade_bsdf.h read out for tests: the mtsgpu_*_eval hooks, one record per thread.
#include "shade_bsdf.h"
#include "shade_cloth.h"

namespace mg {

// BSDF::f / BSDF::pdf / BSDF::sample(bRec, pdf, sample) read out for tests (mtsgpu_bsdf_eval): the chi-square procedure of
// src/tests/test_chisquare.cpp:299-420 runs against exactly the code k_shade runs.  One query record per thread:
// wi = q[i][0..2]; op 0 / 1: wo = q[i][3..5]; op 2: sample = q[i][3..4].
template <int BT>
__device__ __forceinline__ void bsdf_eval_one(const BsdfTable &tab, bool two, const float *P, int op, const float *q, float *o) {
	const V3 wi(q[0], q[1], q[2]);
	if (op == 0) {
		const V3 f = Bsdf2<BT>::f(tab, two, P, wi, V3(q[3], q[4], q[5]));
		o[0] = f.x; o[1] = f.y; o[2] = f.z;
	} else if (op == 1) {
		o[0] = Bsdf2<BT>::pdf(tab, two, P, wi, V3(q[3], q[4], q[5]));
	} else {
		V3 wo; float pdf; uint32_t st;
		const V3 f = Bsdf2<BT>::sample(tab, two, P, wi, q[3], q[4], wo, pdf, st);
		o[0] = wo.x; o[1] = wo.y; o[2] = wo.z; o[3] = pdf; o[4] = f.x; o[5] = f.y; o[6] = f.z; o[7] = __uint_as_float(st);
	}
}
struct BsdfParams { float v[kBsdfNParams]; };
__global__ void k_bsdf_eval(uint32_t type, BsdfParams params, int op, uint32_t n, const float *queries, float *out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const bool two = (type & 0x100u) != 0;
	const float *P = params.v, *q = queries + 6 * (size_t) i;
	float o[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	const BsdfTable tab{ nullptr, nullptr };       // a single block has no table: the host refuses the composite here
	switch (type & 0xFFu) {
		case 0: bsdf_eval_one<0>(tab, two, P, op, q, o); break;
		case 1: bsdf_eval_one<1>(tab, two, P, op, q, o); break;
		case 2: bsdf_eval_one<2>(tab, two, P, op, q, o); break;
		case 3: bsdf_eval_one<3>(tab, two, P, op, q, o); break;
		case 4: bsdf_eval_one<4>(tab, two, P, op, q, o); break;
		case 5: bsdf_eval_one<5>(tab, two, P, op, q, o); break;
		case 6: bsdf_eval_one<6>(tab, two, P, op, q, o); break;
		case 7: bsdf_eval_one<7>(tab, two, P, op, q, o); break;
		default: bsdf_eval_one<8>(tab, two, P, op, q, o); break;
	}
	#pragma unroll
	for (int k = 0; k < 8; ++k) out[8 * (size_t) i + k] = o[k];
}
// The same read-out for entry `index` of a BSDF table in device memory (mtsgpu_bsdf_eval_table): what a composite needs
__global__ void k_bsdf_eval_table(const uint32_t *types, const float *params, uint32_t index, int op, uint32_t n, const float *queries, float *out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t type = types[index];
	const bool two = (type & 0x100u) != 0;
	const float *P = params + kBsdfNParams * (size_t) index, *q = queries + 6 * (size_t) i;
	float o[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	const BsdfTable tab{ types, params };
	switch (type & 0xFFu) {
		case 0: bsdf_eval_one<0>(tab, two, P, op, q, o); break;
		case 1: bsdf_eval_one<1>(tab, two, P, op, q, o); break;
		case 2: bsdf_eval_one<2>(tab, two, P, op, q, o); break;
		case 3: bsdf_eval_one<3>(tab, two, P, op, q, o); break;
		case 4: bsdf_eval_one<4>(tab, two, P, op, q, o); break;
		case 5: bsdf_eval_one<5>(tab, two, P, op, q, o); break;
		case 6: bsdf_eval_one<6>(tab, two, P, op, q, o); break;
		case 7: bsdf_eval_one<7>(tab, two, P, op, q, o); break;
		case 8: bsdf_eval_one<8>(tab, two, P, op, q, o); break;
		default: bsdf_eval_one<9>(tab, two, P, op, q, o); break;
	}
	#pragma unroll
	for (int k = 0; k < 8; ++k) out[8 * (size_t) i + k] = o[k];
}

// mtsgpu_bsdf_eval_colored: k_bsdf_eval on the block bsdf_block_with_color builds from (params, slots, color)
template <int BT>
__device__ __forceinline__ void bsdf_eval_colored_one(bool two, const float *P, uint32_t slots, V3 color, int op, const float *q, float *o) {
	float Q[kBsdfNParams];
	bsdf_block_with_color<BT>(P, slots, color, Q);
	bsdf_eval_one<BT>(BsdfTable{ nullptr, nullptr }, two, Q, op, q, o);
}
__global__ void k_bsdf_eval_colored(uint32_t type, BsdfParams params, uint32_t slots, float cr, float cg, float cb, int op, uint32_t n,
                                    const float *queries, float *out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const bool two = (type & 0x100u) != 0;
	const float *P = params.v, *q = queries + 6 * (size_t) i;
	const V3 color(cr, cg, cb);
	float o[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	switch (type & 0xFFu) {
		case 0: bsdf_eval_colored_one<0>(two, P, slots, color, op, q, o); break;
		case 1: bsdf_eval_colored_one<1>(two, P, slots, color, op, q, o); break;
		case 2: bsdf_eval_colored_one<2>(two, P, slots, color, op, q, o); break;
		case 3: bsdf_eval_colored_one<3>(two, P, slots, color, op, q, o); break;
		case 4: bsdf_eval_colored_one<4>(two, P, slots, color, op, q, o); break;
		case 5: bsdf_eval_colored_one<5>(two, P, slots, color, op, q, o); break;
		case 6: bsdf_eval_colored_one<6>(two, P, slots, color, op, q, o); break;
		case 7: bsdf_eval_colored_one<7>(two, P, slots, color, op, q, o); break;
		default: bsdf_eval_colored_one<8>(two, P, slots, color, op, q, o); break;
	}
	#pragma unroll
	for (int k = 0; k < 8; ++k) out[8 * (size_t) i + k] = o[k];
}
// mtsgpu_vertex_color_eval: its_color for n records; the host has checked prim < n_tris
__global__ void k_vertex_color_eval(const float4 *tri_col, uint32_t n, const uint32_t *prim, const float *uv, float *out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const V3 c = its_color(tri_col, prim[i], uv[2 * (size_t) i], uv[2 * (size_t) i + 1]);
	out[3 * (size_t) i] = c.x; out[3 * (size_t) i + 1] = c.y; out[3 * (size_t) i + 2] = c.z;
}

// mtsgpu_bsdf_eval_slots: k_bsdf_eval on the block bsdf_block_with_slots builds
struct SlotValues { int src[2]; float color[3]; float val[2][3]; };
template <int BT>
__device__ __forceinline__ void bsdf_eval_slots_one(bool two, const float *P, const SlotValues &sv, int op, const float *q, float *o) {
	float Q[kBsdfNParams];
	bsdf_block_with_slots<BT>(P, sv.src[0], sv.src[1], V3(sv.color[0], sv.color[1], sv.color[2]), V3(sv.val[0][0], sv.val[0][1], sv.val[0][2]),
	                          V3(sv.val[1][0], sv.val[1][1], sv.val[1][2]), Q);
	bsdf_eval_one<BT>(BsdfTable{ nullptr, nullptr }, two, Q, op, q, o);
}
__global__ void k_bsdf_eval_slots(uint32_t type, BsdfParams params, SlotValues sv, int op, uint32_t n, const float *queries, float *out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const bool two = (type & 0x100u) != 0;
	const float *P = params.v, *q = queries + 6 * (size_t) i;
	float o[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	switch (type & 0xFFu) {
		case 0: bsdf_eval_slots_one<0>(two, P, sv, op, q, o); break;
		case 1: bsdf_eval_slots_one<1>(two, P, sv, op, q, o); break;
		case 2: bsdf_eval_slots_one<2>(two, P, sv, op, q, o); break;
		case 3: bsdf_eval_slots_one<3>(two, P, sv, op, q, o); break;
		case 4: bsdf_eval_slots_one<4>(two, P, sv, op, q, o); break;
		case 5: bsdf_eval_slots_one<5>(two, P, sv, op, q, o); break;
		case 6: bsdf_eval_slots_one<6>(two, P, sv, op, q, o); break;
		case 7: bsdf_eval_slots_one<7>(two, P, sv, op, q, o); break;
		default: bsdf_eval_slots_one<8>(two, P, sv, op, q, o); break;
	}
	#pragma unroll
	for (int k = 0; k < 8; ++k) out[8 * (size_t) i + k] = o[k];
}
// mtsgpu_bsdf_eval_masked: k_bsdf_eval through BsdfMasked, p = the luminance of the opacity (luminance)
template <int BT>
__device__ __forceinline__ void bsdf_eval_masked_one(bool two, const float *P, float p, int op, const float *q, float *o) {
	const BsdfTable tab{ nullptr, nullptr };
	const V3 wi(q[0], q[1], q[2]);
	if (op == 0) {
		const V3 f = BsdfMasked<BT>::f(tab, two, P, p, wi, V3(q[3], q[4], q[5]));
		o[0] = f.x; o[1] = f.y; o[2] = f.z;
	} else if (op == 1) {
		o[0] = BsdfMasked<BT>::pdf(tab, two, P, p, wi, V3(q[3], q[4], q[5]));
	} else {
		V3 wo; float pdf; uint32_t st;
		const V3 f = BsdfMasked<BT>::sample(tab, two, P, p, wi, q[3], q[4], wo, pdf, st);
		o[0] = wo.x; o[1] = wo.y; o[2] = wo.z; o[3] = pdf; o[4] = f.x; o[5] = f.y; o[6] = f.z; o[7] = __uint_as_float(st);
	}
}
__global__ void k_bsdf_eval_masked(uint32_t type, BsdfParams params, float cr, float cg, float cb, int op, uint32_t n, const float *queries,
                                   float *out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const bool two = (type & 0x100u) != 0;
	const float *P = params.v, *q = queries + 6 * (size_t) i;
	const float p = luminance(V3(cr, cg, cb));
	float o[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	switch (type & 0xFFu) {
		case 0: bsdf_eval_masked_one<0>(two, P, p, op, q, o); break;
		case 1: bsdf_eval_masked_one<1>(two, P, p, op, q, o); break;
		case 2: bsdf_eval_masked_one<2>(two, P, p, op, q, o); break;
		case 3: bsdf_eval_masked_one<3>(two, P, p, op, q, o); break;
		case 4: bsdf_eval_masked_one<4>(two, P, p, op, q, o); break;
		case 5: bsdf_eval_masked_one<5>(two, P, p, op, q, o); break;
		case 6: bsdf_eval_masked_one<6>(two, P, p, op, q, o); break;
		case 7: bsdf_eval_masked_one<7>(two, P, p, op, q, o); break;
		default: bsdf_eval_masked_one<8>(two, P, p, op, q, o); break;
	}
	#pragma unroll
	for (int k = 0; k < 8; ++k) out[8 * (size_t) i + k] = o[k];
}
// mtsgpu_bsdf_eval_snow: k_bsdf_eval through BsdfSnow2 without a mask (p = 1); kSnowNone: the Lambertian whose block is derived[0..2]
__global__ void k_bsdf_eval_snow(uint32_t type, DSnow e, int op, uint32_t n, const float *queries, float *out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const bool two = (type & 0x100u) != 0;
	const float *q = queries + 6 * (size_t) i, *D = e.derived;
	const V3 wi(q[0], q[1], q[2]);
	float o[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	if (op == 0) {
		const V3 f = BsdfSnow2::f(two, e.kind, D, D, 1.0f, wi, V3(q[3], q[4], q[5]));
		o[0] = f.x; o[1] = f.y; o[2] = f.z;
	} else if (op == 1) {
		o[0] = BsdfSnow2::pdf(two, e.kind, D, D, 1.0f, wi, V3(q[3], q[4], q[5]));
	} else {
		V3 wo; float pdf; uint32_t st;
		const V3 f = BsdfSnow2::sample(two, e.kind, D, D, 1.0f, wi, q[3], q[4], wo, pdf, st);
		o[0] = wo.x; o[1] = wo.y; o[2] = wo.z; o[3] = pdf; o[4] = f.x; o[5] = f.y; o[6] = f.z; o[7] = __uint_as_float(st);
	}
	#pragma unroll
	for (int k = 0; k < 8; ++k) out[8 * (size_t) i + k] = o[k];
}
// mtsgpu_bsdf_eval_cloth: k_bsdf_eval through BsdfCloth2; a query is wi, wo or the sample, its.uv; op 3: the internals of f
__global__ void k_bsdf_eval_cloth(uint32_t type, DWeave W, const uint32_t *pattern, const DYarn *yarns, int op, uint32_t n, const float *queries,
                                  float *out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const bool two = (type & 0x100u) != 0;
	const float *q = queries + 8 * (size_t) i;
	const V3 wi(q[0], q[1], q[2]);
	float o[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
	if (op == 0) {
		const V3 f = BsdfCloth2::f(two, W, pattern, yarns, wi, V3(q[3], q[4], q[5]), q[6], q[7]);
		o[0] = f.x; o[1] = f.y; o[2] = f.z;
	} else if (op == 1) {
		o[0] = BsdfCloth2::pdf(two, wi, V3(q[3], q[4], q[5]));
	} else if (op == 2) {
		V3 wo; float pdf; uint32_t st;
		const BsdfCloth::Hit H = BsdfCloth::prepare(W, pattern, yarns, q[6], q[7]);
		const V3 f = BsdfCloth2::sample(two, W, yarns, H, wi, q[3], q[4], wo, pdf, st);
		o[0] = wo.x; o[1] = wo.y; o[2] = wo.z; o[3] = pdf; o[4] = f.x; o[5] = f.y; o[6] = f.z; o[7] = __uint_as_float(st);
	} else {
		(void) BsdfCloth2::f(two, W, pattern, yarns, wi, V3(q[3], q[4], q[5]), q[6], q[7], o);
	}
	#pragma unroll
	for (int k = 0; k < 8; ++k) out[8 * (size_t) i + k] = o[k];
}
// mtsgpu_uv_texture_eval: its_uv and tex_eval for n records; the host has checked prim < n_tris
__global__ void k_uv_texture_eval(DScene sc, const float4 *tri_uv, DTexture tex, uint32_t n, const uint32_t *prim, const float *rec, float *out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t shape = __float_as_uint(sc.tri_pos[kTriStride * (size_t) prim[i] + 2].z);
	const float *r = rec + 3 * (size_t) i;
	float uvx, uvy;
	its_uv(sc, tri_uv, prim[i], shape, r[0], r[1], V3(r[0], r[1], r[2]), uvx, uvy);
	const V3 c = tex_eval(tex, nullptr, uvx, uvy);      // the host refuses a bitmap here
	float *o = out + 5 * (size_t) i;
	o[0] = uvx; o[1] = uvy; o[2] = c.x; o[3] = c.y; o[4] = c.z;
}

// mtsgpu_bitmap_texture_eval: the same for a bitmap descriptor, whose texels lie at texels[tex.first ...]
__global__ void k_bitmap_texture_eval(DScene sc, const float4 *tri_uv, DTexture tex, const float4 *texels, uint32_t n, const uint32_t *prim,
                                      const float *rec, float *out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t shape = __float_as_uint(sc.tri_pos[kTriStride * (size_t) prim[i] + 2].z);
	const float *r = rec + 3 * (size_t) i;
	float uvx, uvy;
	its_uv(sc, tri_uv, prim[i], shape, r[0], r[1], V3(r[0], r[1], r[2]), uvx, uvy);
	const V3 c = tex_eval(tex, texels, uvx, uvy);
	float *o = out + 5 * (size_t) i;
	o[0] = uvx; o[1] = uvy; o[2] = c.x; o[3] = c.y; o[4] = c.z;
}

// mtsgpu_shading_frame_eval: the shading frame fill_its_tan leaves for n records; the host has checked prim < n_tris.  rec =
// (u, v, -) on a triangle, the world-space hit point on a sphere (then the ray starts there with t = 0)
__global__ void k_shading_frame_eval(DScene sc, DTangents tan, uint32_t n, const uint32_t *prim, const float *rec, float *out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float4 *TP = sc.tri_pos + kTriStride * (size_t) prim[i];
	const float *r = rec + 3 * (size_t) i;
	Its its;
	fill_its_tan(sc, tan, V3(r[0], r[1], r[2]), V3(0.0f, 0.0f, 1.0f), 0.0f, prim[i], r[0], r[1], TP[0], TP[1], TP[2], its);
	float *o = out + 9 * (size_t) i;
	o[0] = its.shS.x; o[1] = its.shS.y; o[2] = its.shS.z;
	o[3] = its.shT.x; o[4] = its.shT.y; o[5] = its.shT.z;
	o[6] = its.shN.x; o[7] = its.shN.y; o[8] = its.shN.z;
}

// The sky luminaire read out for n query records (mtsgpu_lum_eval): block = its parameters followed by the derived array
// (kLumStride + MTSGPU_SKY_NDERIVED floats in device memory); queries [n][6], out [n][12]
__global__ void k_sky_eval(const float *block, int op, uint32_t n, const float *queries, float *out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float *LP = block, *SD = block + kLumStride, *q = queries + 6 * (size_t) i;
	float o[12] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	if (op == 0) {
		const V3 le = sky_le(LP, SD, V3(q[0], q[1], q[2]));
		o[0] = le.x; o[1] = le.y; o[2] = le.z;
	} else if (op == 1) {
		// the call sample_luminaire<true> makes; the value is reported before that function divides it by the pdf
		V3 d, le, end; float pdf;
		sky_sample(LP, SD, V3(q[0], q[1], q[2]), q[3], q[4], d, pdf, le, end);
		o[0] = d.x; o[1] = d.y; o[2] = d.z; o[3] = pdf;
		o[4] = le.x; o[5] = le.y; o[6] = le.z;
		o[8] = end.x; o[9] = end.y; o[10] = end.z;
	} else {
		o[0] = 1.0f / (4 * kPi);      // sky.cpp:288-292
	}
	#pragma unroll
	for (int k = 0; k < 12; ++k) out[12 * (size_t) i + k] = o[k];
}

// The luminaires of the uploaded scene read out for n query records (mtsgpu_scene_lum_eval): queries [n][16], out [n][16].
// SKY is chosen the way the shading launches choose it (shade_launch.h): by DScene::sky.  The host has checked op, and for
// op 1 the luminaire index and type of every record, for op 2 that the scene has a background luminaire.
template <bool SKY>
__device__ __forceinline__ void scene_lum_eval_one(const DScene &sc, int op, const float *q, float *o) {
	const V3 p(q[0], q[1], q[2]);
	if (op == 0) {
		LRec r;
		r.p = r.n = r.d = r.value = V3(0.0f, 0.0f, 0.0f); r.pdf = 0.0f; r.lum = -1;
		const bool found = sample_luminaire<SKY>(sc, p, q[3], q[4], r);
		o[0] = found ? 1.0f : 0.0f; o[1] = (float) r.lum;
		o[2] = r.p.x; o[3] = r.p.y; o[4] = r.p.z;
		o[5] = r.n.x; o[6] = r.n.y; o[7] = r.n.z;
		o[8] = r.d.x; o[9] = r.d.y; o[10] = r.d.z;
		o[11] = r.pdf;
		o[12] = r.value.x; o[13] = r.value.y; o[14] = r.value.z;
	} else if (op == 1) {
		o[0] = pdf_luminaire(sc, p, (int) q[12], V3(q[3], q[4], q[5]), V3(q[6], q[7], q[8]), V3(q[9], q[10], q[11]));
	} else {
		const V3 le = background_le<SKY>(sc, p);
		o[0] = le.x; o[1] = le.y; o[2] = le.z;
	}
}
__global__ void k_scene_lum_eval(DScene sc, int op, uint32_t n, const float *queries, float *out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float *q = queries + 16 * (size_t) i;
	float o[16] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	if (sc.sky) scene_lum_eval_one<true>(sc, op, q, o);
	else scene_lum_eval_one<false>(sc, op, q, o);
	#pragma unroll
	for (int k = 0; k < 16; ++k) out[16 * (size_t) i + k] = o[k];
}

// the same for a scene with a textured spot (DSpots::lum_texture != NULL): op 0 runs sample_luminaire<SKY, true>, the
// instantiation the k_shade_spt kernels run; the other two operations do not depend on the table
__global__ void k_scene_lum_eval_spt(DScene sc, DSpots spt, int op, uint32_t n, const float *queries, float *out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float *q = queries + 16 * (size_t) i;
	float o[16] = { 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0 };
	if (op == 0) {
		LRec r;
		r.p = r.n = r.d = r.value = V3(0.0f, 0.0f, 0.0f); r.pdf = 0.0f; r.lum = -1;
		const V3 p(q[0], q[1], q[2]);
		const bool found = sc.sky ? sample_luminaire<true, true>(sc, p, q[3], q[4], r, spt) : sample_luminaire<false, true>(sc, p, q[3], q[4], r, spt);
		o[0] = found ? 1.0f : 0.0f; o[1] = (float) r.lum;
		o[2] = r.p.x; o[3] = r.p.y; o[4] = r.p.z;
		o[5] = r.n.x; o[6] = r.n.y; o[7] = r.n.z;
		o[8] = r.d.x; o[9] = r.d.y; o[10] = r.d.z;
		o[11] = r.pdf;
		o[12] = r.value.x; o[13] = r.value.y; o[14] = r.value.z;
	} else if (sc.sky) scene_lum_eval_one<true>(sc, op, q, o);
	else scene_lum_eval_one<false>(sc, op, q, o);
	#pragma unroll
	for (int k = 0; k < 16; ++k) out[16 * (size_t) i + k] = o[k];
}

// mtsgpu_spot_eval: SpotLuminaire::sample (spot.cpp:116-124) with a projection texture, as the spot branch of sample_luminaire runs
// it, for n points; block = the parameter block in device memory
__global__ void k_spot_eval(const float *block, DTexture tex, const float4 *texels, float uv_factor, uint32_t n, const float *p, float *out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const float *LP = block;
	const V3 lumToP = V3(p[3 * (size_t) i], p[3 * (size_t) i + 1], p[3 * (size_t) i + 2]) - V3(LP[3], LP[4], LP[5]);
	const float invDist = 1.0f / length(lumToP);
	const V3 d = lumToP * invDist;
	float uvx, uvy;
	const V3 value = spot_falloff_textured(LP, tex, texels, uv_factor, d, uvx, uvy) * (invDist * invDist);
	float *o = out + 8 * (size_t) i;
	o[0] = d.x; o[1] = d.y; o[2] = d.z; o[3] = uvx; o[4] = uvy; o[5] = value.x; o[6] = value.y; o[7] = value.z;
}

void launch_bsdf_eval(hipStream_t s, uint32_t type, const float *params, int op, uint32_t n, const float *queries, float *out) {
	BsdfParams p;
	for (int k = 0; k < kBsdfNParams; ++k) p.v[k] = params[k];
	if (n) hipLaunchKernelGGL(k_bsdf_eval, dim3(blocks_for(n, 256)), dim3(256), 0, s, type, p, op, n, queries, out);
}

void launch_bsdf_eval_table(hipStream_t s, const uint32_t *types, const float *params, uint32_t index, int op, uint32_t n,
                            const float *queries, float *out) {
	if (n) hipLaunchKernelGGL(k_bsdf_eval_table, dim3(blocks_for(n, 256)), dim3(256), 0, s, types, params, index, op, n, queries, out);
}

void launch_sky_eval(hipStream_t s, const float *block, int op, uint32_t n, const float *queries, float *out) {
	if (n) hipLaunchKernelGGL(k_sky_eval, dim3(blocks_for(n, 256)), dim3(256), 0, s, block, op, n, queries, out);
}

void launch_spot_eval(hipStream_t s, const float *block, const DTexture &tex, const float4 *texels, float uv_factor, uint32_t n,
                      const float *p, float *out) {
	if (n) hipLaunchKernelGGL(k_spot_eval, dim3(blocks_for(n, 256)), dim3(256), 0, s, block, tex, texels, uv_factor, n, p, out);
}

void launch_scene_lum_eval(hipStream_t s, const DScene &sc, int op, uint32_t n, const float *queries, float *out, const DSpots &spt) {
	if (n && spt.lum_texture) { hipLaunchKernelGGL(k_scene_lum_eval_spt, dim3(blocks_for(n, 256)), dim3(256), 0, s, sc, spt, op, n, queries, out); return; }
	if (n) hipLaunchKernelGGL(k_scene_lum_eval, dim3(blocks_for(n, 256)), dim3(256), 0, s, sc, op, n, queries, out);
}

void launch_bsdf_eval_colored(hipStream_t s, uint32_t type, const float *params, uint32_t slots, const float *color, int op, uint32_t n,
                              const float *queries, float *out) {
	BsdfParams p;
	for (int k = 0; k < kBsdfNParams; ++k) p.v[k] = params[k];
	if (n) hipLaunchKernelGGL(k_bsdf_eval_colored, dim3(blocks_for(n, 256)), dim3(256), 0, s, type, p, slots, color[0], color[1], color[2], op, n, queries, out);
}

void launch_bsdf_eval_slots(hipStream_t s, uint32_t type, const float *params, const int *source, const float *color, const float *values,
                            int op, uint32_t n, const float *queries, float *out) {
	BsdfParams p;
	for (int k = 0; k < kBsdfNParams; ++k) p.v[k] = params[k];
	SlotValues sv;
	for (int k = 0; k < 2; ++k) sv.src[k] = source[k];
	for (int k = 0; k < 3; ++k) sv.color[k] = color[k];
	for (int k = 0; k < 6; ++k) sv.val[k / 3][k % 3] = values[k];
	if (n) hipLaunchKernelGGL(k_bsdf_eval_slots, dim3(blocks_for(n, 256)), dim3(256), 0, s, type, p, sv, op, n, queries, out);
}

void launch_bsdf_eval_masked(hipStream_t s, uint32_t type, const float *params, const float *opacity, int op, uint32_t n,
                             const float *queries, float *out) {
	BsdfParams p;
	for (int k = 0; k < kBsdfNParams; ++k) p.v[k] = params[k];
	if (n) hipLaunchKernelGGL(k_bsdf_eval_masked, dim3(blocks_for(n, 256)), dim3(256), 0, s, type, p, opacity[0], opacity[1], opacity[2], op, n, queries, out);
}

void launch_bsdf_eval_snow(hipStream_t s, uint32_t type, const DSnow &entry, int op, uint32_t n, const float *queries, float *out) {
	if (n) hipLaunchKernelGGL(k_bsdf_eval_snow, dim3(blocks_for(n, 256)), dim3(256), 0, s, type, entry, op, n, queries, out);
}

void launch_bsdf_eval_cloth(hipStream_t s, uint32_t type, const DWeave &weave, const uint32_t *pattern, const DYarn *yarns, int op, uint32_t n,
                            const float *queries, float *out) {
	if (n) hipLaunchKernelGGL(k_bsdf_eval_cloth, dim3(blocks_for(n, 256)), dim3(256), 0, s, type, weave, pattern, yarns, op, n, queries, out);
}

void launch_uv_texture_eval(hipStream_t s, const DScene &sc, const float4 *tri_uv, const DTexture &tex, uint32_t n, const uint32_t *prim,
                            const float *rec, float *out) {
	if (n) hipLaunchKernelGGL(k_uv_texture_eval, dim3(blocks_for(n, 256)), dim3(256), 0, s, sc, tri_uv, tex, n, prim, rec, out);
}

void launch_bitmap_texture_eval(hipStream_t s, const DScene &sc, const float4 *tri_uv, const DTexture &tex, const float4 *texels, uint32_t n,
                                const uint32_t *prim, const float *rec, float *out) {
	if (n) hipLaunchKernelGGL(k_bitmap_texture_eval, dim3(blocks_for(n, 256)), dim3(256), 0, s, sc, tri_uv, tex, texels, n, prim, rec, out);
}

void launch_shading_frame_eval(hipStream_t s, const DScene &sc, const DTangents &tan, uint32_t n, const uint32_t *prim, const float *rec, float *out) {
	if (n) hipLaunchKernelGGL(k_shading_frame_eval, dim3(blocks_for(n, 256)), dim3(256), 0, s, sc, tan, n, prim, rec, out);
}

void launch_vertex_color_eval(hipStream_t s, const float4 *tri_col, uint32_t n, const uint32_t *prim, const float *uv, float *out) {
	if (n) hipLaunchKernelGGL(k_vertex_color_eval, dim3(blocks_for(n, 256)), dim3(256), 0, s, tri_col, n, prim, uv, out);
}

} // namespace mg
