// shade_cloth.h -- the Irawan-Marschner woven-cloth BRDF of the reference (src/bsdfs/irawan.cpp:105-517, irawan.h) in binary32, in
// the reference's operation order and as compiled: its value at (its.uv, wi, wo) from a weave record, a pattern and a yarn table
// (kernels.h: DWeave, DYarn).  The cloth kernels (k_shade_clo) and the read-out hook (k_bsdf_eval_cloth) both call this.
#pragma once
#include "shade_bsdf.h"

namespace mg {

// Noise::perlinNoise's permutation (noise.cpp:9-41: Ken Perlin's reference table, which the source lists twice so that an index
// of up to 511 needs no mask; here every index is masked).  256 bytes of constant memory: the shading kernels' LDS is taken by
// the path records, and a lookup is four dependent loads per corner that the vector L1 serves.
static __device__ __constant__ uint8_t kNoisePerm[256] = {
	151, 160, 137, 91, 90, 15, 131, 13, 201, 95, 96, 53, 194, 233, 7, 225, 140, 36, 103, 30, 69, 142, 8, 99, 37, 240, 21, 10, 23,
	190, 6, 148, 247, 120, 234, 75, 0, 26, 197, 62, 94, 252, 219, 203, 117, 35, 11, 32, 57, 177, 33, 88, 237, 149, 56, 87, 174,
	20, 125, 136, 171, 168, 68, 175, 74, 165, 71, 134, 139, 48, 27, 166, 77, 146, 158, 231, 83, 111, 229, 122, 60, 211, 133, 230,
	220, 105, 92, 41, 55, 46, 245, 40, 244, 102, 143, 54, 65, 25, 63, 161, 1, 216, 80, 73, 209, 76, 132, 187, 208, 89, 18, 169,
	200, 196, 135, 130, 116, 188, 159, 86, 164, 100, 109, 198, 173, 186, 3, 64, 52, 217, 226, 250, 124, 123, 5, 202, 38, 147, 118,
	126, 255, 82, 85, 212, 207, 206, 59, 227, 47, 16, 58, 17, 182, 189, 28, 42, 223, 183, 170, 213, 119, 248, 152, 2, 44, 154,
	163, 70, 221, 153, 101, 155, 167, 43, 172, 9, 129, 22, 39, 253, 19, 98, 108, 110, 79, 113, 224, 232, 178, 185, 112, 104, 218,
	246, 97, 228, 251, 34, 242, 193, 238, 210, 144, 12, 191, 179, 162, 241, 81, 51, 145, 235, 249, 14, 239, 107, 49, 192, 214, 31,
	181, 199, 106, 157, 184, 84, 204, 176, 115, 121, 50, 45, 127, 4, 150, 254, 138, 236, 205, 93, 222, 114, 67, 29, 24, 72, 243,
	141, 128, 195, 78, 66, 215, 61, 156, 180
};

struct BsdfCloth {
	// ---- Random(seed) and its first draws (random.cpp:99-103, 141-174, 218-227) ----
	// The first three outputs of a freshly seeded MT19937-64 are tempered mt'[0..2], and the first regeneration step forms
	// mt'[i] from mt[i], mt[i + 1] and mt[i + 156] alone: seven words of the 312-word seeding recurrence, which runs in
	// registers up to word 158.  Seed 0 is a seed like any other (mt[0] = 0).
	struct Mt3 { uint64_t w0, w1, w2, w3, m0, m1, m2; };
	static __device__ __forceinline__ Mt3 mt_seed(uint64_t s) {
		Mt3 r;
		uint64_t x = s;
		r.w0 = x;
		r.w1 = r.w2 = r.w3 = r.m0 = r.m1 = r.m2 = 0;
		for (uint32_t i = 1; i <= 158; ++i) {
			x = 6364136223846793005ULL * (x ^ (x >> 62)) + (uint64_t) i;
			if (i == 1) r.w1 = x;
			else if (i == 2) r.w2 = x;
			else if (i == 3) r.w3 = x;
			else if (i == 156) r.m0 = x;
			else if (i == 157) r.m1 = x;
			else if (i == 158) r.m2 = x;
		}
		return r;
	}
	static __device__ __forceinline__ uint64_t mt_word(uint64_t a, uint64_t b, uint64_t m) {
		const uint64_t x = (a & 0xFFFFFFFF80000000ULL) | (b & 0x7FFFFFFFULL);
		uint64_t y = m ^ (x >> 1) ^ ((x & 1ULL) ? 0xB5026F5AA96619E9ULL : 0ULL);
		y ^= (y >> 29) & 0x5555555555555555ULL;
		y ^= (y << 17) & 0x71D67FFFEDA60000ULL;
		y ^= (y << 37) & 0xFFF7EEE000000000ULL;
		y ^= (y >> 43);
		return y;
	}
	// nextULong() number k = 0, 1, 2 of Random(seed)
	static __device__ __forceinline__ uint64_t mt_ulong(const Mt3 &r, int k) {
		return k == 0 ? mt_word(r.w0, r.w1, r.m0) : k == 1 ? mt_word(r.w1, r.w2, r.m1) : mt_word(r.w2, r.w3, r.m2);
	}

	// ---- Noise::perlinNoise (noise.cpp:43-101), GRAD_PERLIN ----
	static __device__ __forceinline__ float grad(int x, int y, int z, float dx, float dy, float dz) {
		int h = kNoisePerm[(kNoisePerm[(kNoisePerm[x & 255] + y) & 255] + z) & 255];
		h &= 15;
		const float u = h < 8 ? dx : dy;
		const float v = h < 4 ? dy : (h == 12 || h == 14) ? dx : dz;
		return ((h & 1) ? -u : u) + ((h & 2) ? -v : v);
	}
	static __device__ __forceinline__ float noise_weight(float t) {
		const float t3 = t * t * t, t4 = t3 * t, t5 = t4 * t;
		return 6.0f * t5 - 15.0f * t4 + 10.0f * t3;
	}
	static __device__ __forceinline__ float lerp(float t, float v1, float v2) { return (1.0f - t) * v1 + t * v2; }      // util.h:323-325
	// the cloth passes (x, 0, 0); the full three-dimensional form is kept, so that the signs of its zeros are the reference's
	static __device__ __forceinline__ float perlin(float px) {
		const float py = 0.0f, pz = 0.0f;
		int ix = (int) floorf(px), iy = 0, iz = 0;
		const float dx = px - (float) ix, dy = py - (float) iy, dz = pz - (float) iz;
		ix &= 255;
		const float w000 = grad(ix, iy, iz, dx, dy, dz);
		const float w100 = grad(ix + 1, iy, iz, dx - 1, dy, dz);
		const float w010 = grad(ix, iy + 1, iz, dx, dy - 1, dz);
		const float w110 = grad(ix + 1, iy + 1, iz, dx - 1, dy - 1, dz);
		const float w001 = grad(ix, iy, iz + 1, dx, dy, dz - 1);
		const float w101 = grad(ix + 1, iy, iz + 1, dx - 1, dy, dz - 1);
		const float w011 = grad(ix, iy + 1, iz + 1, dx, dy - 1, dz - 1);
		const float w111 = grad(ix + 1, iy + 1, iz + 1, dx - 1, dy - 1, dz - 1);
		const float wx = noise_weight(dx), wy = noise_weight(dy), wz = noise_weight(dz);
		const float x00 = lerp(wx, w000, w100), x10 = lerp(wx, w010, w110), x01 = lerp(wx, w001, w101), x11 = lerp(wx, w011, w111);
		const float y0 = lerp(wy, x00, x10), y1 = lerp(wy, x01, x11);
		return lerp(wz, y0, y1);
	}

	// (uint64_t) of a Float that may be negative: what the reference's x86-64 build computes (mtsgpu_cloth.h)
	static __device__ __forceinline__ uint64_t to_u64(float x) { return (uint64_t) (long long) x; }
	static __device__ __forceinline__ float pow15(float x) { return dpow15(x); }      // std::pow(x, 1.5f)
	static __device__ __forceinline__ float atanh_ref(float arg) { return dlog((1.0f + arg) / (1.0f - arg)) / 2.0f; }      // irawan.cpp:485-487

	// irawan.cpp:453-483
	static __device__ __forceinline__ float radius_of_curvature(float u, float umax, float kappa, float w, float l) {
		const float rhat = 1.0f + kappa * (1.0f + 1.0f / dtan(umax));
		const float a = 0.5f * w;
		float R = 0;
		if (rhat == 1.0f) {                 // circle
			R = (0.5f * l - a * dsin(umax)) / dsin(umax);
		} else if (rhat > 0.0f) {           // ellipse
			const float tmax = datan(rhat * dtan(umax));
			const float bhat = (0.5f * l - a * dsin(umax)) / dsin(tmax);
			const float ahat = bhat / rhat;
			const float t = datan(rhat * dtan(u));
			float st, ct; dsincos(t, st, ct);
			R = pow15(bhat * bhat * ct * ct + ahat * ahat * st * st) / (ahat * bhat);
		} else if (rhat < 0.0f) {           // hyperbola
			const float tmax = -atanh_ref(rhat * dtan(umax));
			const float bhat = (0.5f * l - a * dsin(umax)) / dsinh(tmax);
			const float ahat = bhat / rhat;
			const float t = -atanh_ref(rhat * dtan(u));
			const float ch = dcosh(t), sh = dsinh(t);
			R = -pow15(bhat * bhat * ch * ch + ahat * ahat * sh * sh) / (ahat * bhat);
		} else {                            // rhat == 0 (or not a number): parabola
			const float tmax = dtan(umax);
			const float ahat = (0.5f * l - a * dsin(umax)) / (2 * tmax);
			const float t = dtan(u);
			R = 2 * ahat * pow15(1 + t * t);
		}
		return R;
	}
	// irawan.cpp:490-507; 2 * M_PI * I0 is binary64
	static __device__ __forceinline__ float von_mises(float cos_x, float b) {
		float I0;
		const float absB = fabsf(b);
		if (fabsf(b) <= 3.75f) {
			float t = absB / 3.75f;
			t = t * t;
			I0 = 1.0f + t * (3.5156229f + t * (3.0899424f + t * (1.2067492f + t * (0.2659732f + t * (0.0360768f + t * 0.0045813f)))));
		} else {
			const float t = 3.75f / absB;
			I0 = dexp(absB) / sqrtf(absB) * (0.39894228f + t * (0.01328592f + t * (0.00225319f + t * (-0.00157565f + t * (0.00916281f
			     + t * (-0.02057706f + t * (0.02635537f + t * (-0.01647633f + t * 0.00392377f))))))));
		}
		return (float) ((double) dexp(b * cos_x) / (2 * 3.14159265358979323846 * (double) I0));
	}
	// irawan.cpp:510-517 with sg_a = 0, sg_s = 1; al / (4.0f * M_PI) * c1 * c2 / (c1 + c2) is binary64 around the binary32 sum
	static __device__ __forceinline__ float seeliger(float cos_th1, float cos_th2) {
		const float al = 1.0f / (0.0f + 1.0f);
		const float c1 = smax(0.0f, cos_th1), c2 = smax(0.0f, cos_th2);
		if (c1 == 0.0f || c2 == 0.0f) return 0.0f;
		return (float) ((double) al / (4.0 * 3.14159265358979323846) * (double) c1 * (double) c2 / (double) (c1 + c2));
	}
	static __device__ __forceinline__ float smooth_step01(float value) {       // util.h:328-331 with min = 0, max = 1
		float v = (value - 0.0f) / (1.0f - 0.0f);
		v = v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
		return v * v * (-2 * v + 3);
	}

	// irawan.cpp:292-366
	static __device__ __forceinline__ float filament_integrand(const DWeave &W, float u, float v, V3 om_i, V3 om_r, float umax, float kappa,
	                                                           float w, float l) {
		const float alpha = W.alpha, beta = W.beta, ss = W.ss;
		if (ss < 0.0f || ss >= 1.0f) return 0.0f;
		if (w * dsin(umax) >= l) return 0.0f;
		if (kappa < -1.0f) return 0.0f;
		const V3 h = normalize(om_r + om_i);
		const float u_of_v = datan(h.y / h.z);
		if (fabsf(u_of_v) < umax) {
			float sv, cv, su, cu;
			dsincos(v, sv, cv); dsincos(u_of_v, su, cu);
			const V3 n = normalize(V3(sv, su * cv, cu * cv));
			const V3 t = normalize(V3(0.0f, cu, -su));
			const float R = radius_of_curvature(smin(fabsf(u_of_v), (1 - ss) * umax), (1 - ss) * umax, kappa, w, l);
			const float a = 0.5f * w;
			const V3 sum = om_i + om_r, t_cross_h = cross(t, h);
			const float Gu = a * (R + a * cv) / (length(sum) * fabsf(t_cross_h.x));
			const float fc = alpha + von_mises(-dot(om_i, om_r), beta);
			const float A = seeliger(dot(n, om_i), dot(n, om_r));
			float As;
			if (ss == 0.0f) As = A;
			else As = A * (1.0f - smooth_step01((fabsf(u_of_v) - (1.0f - ss) * umax) / (ss * umax)));
			float fs = Gu * fc * As;
			fs = (float) ((double) fs * 3.14159265358979323846 * (double) l);
			const float delta_y = l * W.hWidth;
			float y_of_v = u_of_v * 0.5f * l / umax;
			if (y_of_v > 0.5f * (l - delta_y)) y_of_v = 0.5f * (l - delta_y);
			else if (y_of_v < 0.5f * (delta_y - l)) y_of_v = 0.5f * (delta_y - l);
			if (fabsf(y_of_v - u * 0.5f * l / umax) < 0.5f * delta_y) return fs / delta_y;
		}
		return 0.0f;
	}
	// irawan.cpp:384-451.  The fibre tangent t the source forms there is never read.  v * w / M_PI stays binary64 inside the
	// window test; std::pow(x, 2.0f) is x * x (one rounding either way)
	static __device__ __forceinline__ float staple_integrand(const DWeave &W, float u, float v, V3 om_i, V3 om_r, float psi, float umax,
	                                                         float kappa, float w, float l) {
		const float alpha = W.alpha, beta = W.beta;
		if (w * dsin(umax) >= l) return 0.0f;
		if (kappa < -1.0f) return 0.0f;
		const V3 h = normalize(om_i + om_r);
		float su, cu; dsincos(u, su, cu);
		const float q = h.y * su + h.z * cu;
		const float D = (h.y * cu - h.z * su) / (sqrtf(h.x * h.x + q * q) * dtan(psi));
		const float v_of_u = datan2(-h.y * su - h.z * cu, h.x) + dacos(D);
		if (fabsf(D) < 1.0f && (double) fabsf(v_of_u) < 3.14159265358979323846 / 2.0) {
			float sv, cv; dsincos(v_of_u, sv, cv);
			const V3 n = normalize(V3(sv, su * cv, cu * cv));
			const float R = radius_of_curvature(fabsf(u), umax, kappa, w, l);
			const float a = 0.5f * w;
			const V3 sum = om_i + om_r;
			const float Gv = a * (R + a * cv) / (length(sum) * dot(n, h) * fabsf(dsin(psi)));
			const float fc = alpha + von_mises(-dot(om_i, om_r), beta);
			const float A = seeliger(dot(n, om_i), dot(n, om_r));
			float fs = Gv * fc * A;
			fs = fs * 2.0f * w * umax;
			const float delta_x = w * W.hWidth;
			float x_of_u = (float) ((double) (v_of_u * w) / 3.14159265358979323846);
			if (x_of_u > 0.5f * (w - delta_x)) x_of_u = 0.5f * (w - delta_x);
			else if (x_of_u < 0.5f * (delta_x - w)) x_of_u = 0.5f * (delta_x - w);
			if (fabs((double) x_of_u - (double) (v * w) / 3.14159265358979323846) < (double) (0.5f * delta_x)) return fs / delta_x;
		}
		return 0.0f;
	}

	// IrawanClothBRDF::f (irawan.cpp:105-223) in two stages.  Everything up to the integrand depends on its.uv alone -- the yarn
	// the pattern names, the segment's centre, the two Random(seed) constructions with the noise and the intensity variation, u
	// and v -- so a kernel computes that stage once per hit (prepare) and hands it to the evaluations of the luminaire sample and
	// of the BSDF sample (eval).  The operations and their order are those of the source.
	struct Hit {
		int yarnID;
		float cx, cy, umax, u, v, random1, random2, variation;
	};
	// pattern / yarns: the weave's own (already offset)
	static __device__ __forceinline__ Hit prepare(const DWeave &W, const uint32_t *pattern, const DYarn *yarns, float uvx, float uvy) {
		Hit H;
		const uint32_t tw = W.tileWidth, th = W.tileHeight;
		const float uvX = uvx * W.repeatU, uvY = (1 - uvy) * W.repeatV;
		float xyx = uvX * (float) tw, xyy = uvY * (float) th;
		const int ix = (int) xyx, iy = (int) xyy;
		// modulo(int, int) (util.cpp:424-427)
		int lx = ix - (ix / (int) tw) * (int) tw; if (lx < 0) lx += (int) tw;
		int ly = iy - (iy / (int) th) * (int) th; if (ly < 0) ly += (int) th;
		H.yarnID = (int) pattern[lx + ly * (int) tw] - 1;
		const DYarn &Y = yarns[H.yarnID];
		// ((int) xy.x / tileWidth) * tileWidth is unsigned arithmetic
		const float cx = (float) (((uint32_t) ix / tw) * tw) + Y.centerU * (float) tw;
		const float cy = (float) (((uint32_t) iy / th) * th) + (1 - Y.centerV) * (float) th;
		xyx = xyx - cx;
		xyy = -(xyy - cy);
		float umax = Y.umax;
		float dUmaxOverDWarp, dUmaxOverDWeft;
		if (Y.type == 0u) {
			dUmaxOverDWarp = W.dWarpUmaxOverDWarp; dUmaxOverDWeft = W.dWarpUmaxOverDWeft;
		} else {
			dUmaxOverDWarp = W.dWeftUmaxOverDWarp; dUmaxOverDWeft = W.dWeftUmaxOverDWeft;
			const float tmp = xyx; xyx = -xyy; xyy = tmp;      // the weft's rotation of xy; eval rotates the directions
		}
		H.random1 = 1.0f; H.random2 = 1.0f;
		if (W.period > 0.0f) {
			const uint64_t seed = to_u64(cx) * to_u64((float) th * W.repeatV) + to_u64(cy);
			const Mt3 r = mt_seed(seed);
			const float n1 = ulongToFloat(mt_ulong(r, 1)), n2 = ulongToFloat(mt_ulong(r, 2));      // the first nextFloat() is dropped
			H.random1 = perlin((cx * ((float) th * W.repeatV + n1) + cy) / W.period);
			H.random2 = perlin((cy * ((float) tw * W.repeatU + n2) + cx) / W.period);
			umax = umax + H.random1 * dUmaxOverDWarp + H.random2 * dUmaxOverDWeft;
		}
		H.u = xyy / (Y.length / 2.0f) * umax;
		H.v = (float) ((double) xyx * 3.14159265358979323846 / (double) Y.width);
		H.variation = 1.0f;
		if (W.ksMultiplier > 0.0f && W.fineness > 0.0f) {
			const uint64_t seed = to_u64((cx + xyx) * W.fineness) * to_u64((float) th * W.repeatV * W.fineness) + to_u64((cy + xyy) * W.fineness);
			const Mt3 r = mt_seed(seed);
			const float xi = ulongToFloat(mt_ulong(r, 0));
			H.variation = smin(-dlog(xi), 10.0f);
		}
		H.cx = cx; H.cy = cy; H.umax = umax;
		return H;
	}
	static __device__ __forceinline__ V3 eval(const DWeave &W, const DYarn *yarns, const Hit &H, V3 wi, V3 wo) {
		if (wi.z <= 0 || wo.z <= 0) return V3(0, 0, 0);
		const DYarn Y = yarns[H.yarnID];
		const float w = Y.width, l = Y.length, psi = Y.psi, kappa = Y.kappa;
		V3 om_i = wi, om_r = wo;
		const bool warp = Y.type == 0u;
		if (!warp) {
			float tmp = om_i.x; om_i.x = -om_i.y; om_i.y = tmp;
			tmp = om_r.x; om_r.x = -om_r.y; om_r.y = tmp;
		}
		V3 result(0, 0, 0);
		if (W.ksMultiplier > 0.0f) {
			float integrand;
			if (psi != 0.0f) integrand = staple_integrand(W, H.u, H.v, om_i, om_r, psi, H.umax, kappa, w, l);
			else integrand = filament_integrand(W, H.u, H.v, om_i, om_r, H.umax, kappa, w, l);
			const float s = H.variation * W.ksMultiplier * integrand;
			result = V3(Y.ks[0] * s, Y.ks[1] * s, Y.ks[2] * s);
			const float area = warp ? (W.warpArea + W.weftArea) / W.warpArea : (W.warpArea + W.weftArea) / W.weftArea;
			result = result * area;
		}
		return result + V3(Y.kd[0] * W.kdMultiplier, Y.kd[1] * W.kdMultiplier, Y.kd[2] * W.kdMultiplier);
	}
	// f at its.uv in one call (the read-out hook).  info, if not NULL, receives the eight internals mtsgpu_bsdf_eval_cloth's op 3
	// reports, zeros where f returns at once
	static __device__ __forceinline__ V3 f(const DWeave &W, const uint32_t *pattern, const DYarn *yarns, V3 wi, V3 wo, float uvx, float uvy,
	                                       float *info = nullptr) {
		if (wi.z <= 0 || wo.z <= 0) return V3(0, 0, 0);
		const Hit H = prepare(W, pattern, yarns, uvx, uvy);
		if (info) {
			info[0] = (float) H.yarnID; info[1] = H.cx; info[2] = H.cy; info[3] = H.random1; info[4] = H.random2; info[5] = H.variation;
			info[6] = H.u; info[7] = H.v;
		}
		return eval(W, yarns, H, wi, wo);
	}
	static __device__ __forceinline__ float pdf(V3 wi, V3 wo) {      // irawan.cpp:238-242
		if (wi.z <= 0 || wo.z <= 0) return 0.0f;
		return wo.z * kInvPi;
	}
	// sample(bRec, pdf, s) (irawan.cpp:254-263): the form the integrators call, which does not divide by the cosine
	static __device__ __forceinline__ V3 sample(const DWeave &W, const DYarn *yarns, const Hit &H, V3 wi, float sx, float sy, V3 &wo, float &pdf,
	                                            uint32_t &st) {
		pdf = 0; st = 0; wo = V3(0, 0, 0);
		if (wi.z <= 0) return V3(0, 0, 0);
		wo = squareToHemispherePSA(sx, sy);
		st = T_GLOSSY_REFL;
		pdf = wo.z * kInvPi;
		return eval(W, yarns, H, wi, wo);
	}
};
// BsdfCloth behind the TwoSidedBRDF adapter of Bsdf2
struct BsdfCloth2 {
	static __device__ __forceinline__ V3 f(bool two, const DWeave &W, const uint32_t *pattern, const DYarn *yarns, V3 wi, V3 wo, float uvx,
	                                       float uvy, float *info = nullptr) {
		if (two && wi.z < 0) { wi.z *= -1; wo.z *= -1; }
		return BsdfCloth::f(W, pattern, yarns, wi, wo, uvx, uvy, info);
	}
	static __device__ __forceinline__ V3 eval(bool two, const DWeave &W, const DYarn *yarns, const BsdfCloth::Hit &H, V3 wi, V3 wo) {
		if (two && wi.z < 0) { wi.z *= -1; wo.z *= -1; }
		return BsdfCloth::eval(W, yarns, H, wi, wo);
	}
	static __device__ __forceinline__ float pdf(bool two, V3 wi, V3 wo) {
		if (two && wi.z < 0) { wi.z *= -1; wo.z *= -1; }
		return BsdfCloth::pdf(wi, wo);
	}
	static __device__ __forceinline__ V3 sample(bool two, const DWeave &W, const DYarn *yarns, const BsdfCloth::Hit &H, V3 wi, float sx, float sy,
	                                            V3 &wo, float &pdf, uint32_t &st) {
		bool flipped = false;
		if (two && wi.z < 0) { wi.z *= -1; flipped = true; }
		const V3 result = BsdfCloth::sample(W, yarns, H, wi, sx, sy, wo, pdf, st);
		if (flipped && !isZero(result) && pdf != 0) wo.z *= -1;
		return result;
	}
};

} // namespace mg
