// readout.cpp -- the test and measurement hooks of the C ABI (include/mtsgpu.h): entry points that only borrow the context to
// run one device function over caller-supplied records and hand the results back, and the replay roof of k_trace.
#include "ctx.h"
#include <algorithm>
#include <cstring>

using namespace mg;

namespace {

// The device scratch of one read-out, on the context's device.  It keeps the first HIP error (every later step is skipped,
// finish() reports it) and frees what it handed out on every way out.  A pointer it returns after an error is NULL: launch
// only while ok().
class Scratch {
public:
	explicit Scratch(mtsgpu_ctx *c) : c(c) { check(hipSetDevice(c->device)); }
	~Scratch() { for (void *p : owned) (void) hipFree(p); }
	bool ok() const { return err == hipSuccess; }
	void check(hipError_t e) { if (ok()) err = e; }
	template <typename T> T *alloc(size_t count) {
		void *raw = nullptr;
		if (ok()) check(hipMalloc(&raw, count * sizeof(T)));
		if (raw) owned.push_back(raw);
		return static_cast<T *>(raw);
	}
	// ... zeroed on the context's stream
	template <typename T> T *zeros(size_t count) {
		T *p = alloc<T>(count);
		if (ok()) check(hipMemsetAsync(p, 0, count * sizeof(T), c->stream));
		return p;
	}
	// ... filled from host memory on the context's stream
	template <typename T> T *put(const T *host, size_t count) {
		T *p = alloc<T>(count);
		if (ok()) check(hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
		return p;
	}
	// the results of the launch before it, once that launch is known to have been accepted
	template <typename T> void get(T *host, const T *dev, size_t count) {
		if (ok()) check(hipGetLastError());
		if (ok()) check(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, c->stream));
	}
	int finish(const char *what) {
		if (ok()) check(hipGetLastError());
		if (ok()) check(hipStreamSynchronize(c->stream));
		return ok() ? 0 : fail(c, MTSGPU_EHIP, "%s failed: %s", what, hipGetErrorString(err));
	}
private:
	mtsgpu_ctx *c;
	hipError_t err = hipSuccess;
	std::vector<void *> owned;
};

int checkRecordCount(mtsgpu_ctx *c, uint32_t n) {
	return n > (1u << 24) ? fail(c, MTSGPU_EINVAL, "at most 2^24 query records per call") : 0;
}

// the kernels index the per-primitive arrays of the scene with it
int checkPrimitives(mtsgpu_ctx *c, uint32_t n, const uint32_t *prim) {
	for (uint32_t i = 0; i < n; ++i)
		if (prim[i] >= c->nTris) return fail(c, MTSGPU_EINVAL, "record %u: primitive %u out of range", i, prim[i]);
	return 0;
}

// a BSDF type word and an operation of the single-BSDF read-outs; composite: why this one takes no composite
int checkBsdfRequest(mtsgpu_ctx *c, uint32_t bsdf_type, int op, const char *composite) {
	if ((bsdf_type & 0xFFu) >= (uint32_t) MTSGPU_BSDF_NTYPES || (bsdf_type & ~(0xFFu | (uint32_t) MTSGPU_BSDF_TWOSIDED)) || op < 0 || op > 2)
		return fail(c, MTSGPU_EINVAL, "bad BSDF type or operation");
	if ((bsdf_type & 0xFFu) == (uint32_t) MTSGPU_BSDF_COMPOSITE) return fail(c, MTSGPU_EINVAL, "%s", composite);
	return 0;
}

// mtsgpu_replay_roof records what its rays ask for (DQueues::rec) during one launch only: off again on every way out
struct RecordingOff { mtsgpu_ctx *c; ~RecordingOff() { c->q.rec = c->q.rec_len = nullptr; c->q.rec_cap = 0; } };

} // namespace

extern "C" {

// The replay roof of the closest-hit traversal kernel (include/mtsgpu.h).
int mtsgpu_replay_roof(mtsgpu_ctx *c, int kind, uint32_t n, uint32_t stride, int reps, double *out) {
	if (!c) return fail(nullptr, MTSGPU_EINVAL, "null context");
	if (!c->haveScene) return fail(c, MTSGPU_ESTATE, "no scene uploaded");
	if (!out || n == 0 || stride == 0 || reps < 1 || kind < 0 || kind > 2) return fail(c, MTSGPU_EINVAL, "bad argument");
	const mtsgpu_ctx::LastPass lp = c->lastPass;
	if (kind == 1 && (!lp.valid || (uint64_t) n * stride > lp.nPaths))
		return fail(c, MTSGPU_EINVAL, "replay roof: %u camera rays x stride %u exceed the pass rendered last (%u paths)", n, stride, lp.valid ? lp.nPaths : 0u);
	if (kind == 2 && (!lp.valid || (uint64_t) n * stride > lp.shadowMax))
		return fail(c, MTSGPU_EINVAL, "replay roof: %u shadow rays x stride %u exceed the shadow queue of the pass rendered last (%u rays; host-driven passes only)",
		            n, stride, lp.valid ? lp.shadowMax : 0u);
	if ((uint64_t) n * stride > c->pathCap || ((uint64_t) (n - 1) * stride + 1) * kPathSlots > (1ull << 29))
		return fail(c, MTSGPU_EINVAL, "replay roof: %u rays x stride %u exceed the path records in memory (%zu) or the 2^29 slots a recorded index can name", n, stride, c->pathCap);
	HIPCHK(c, hipSetDevice(c->device));
	hipStream_t s = c->stream;
	const int mode = kind == 2 ? 1 : 0;
	const bool coherent = kind == 1, bin = kind != 2;      // as the bounces launch this class of rays
	const uint32_t cap = 256;                  // requests kept per ray (C3: 45 on average; longer lists are truncated and counted); % 4 == 0
	const uint32_t nBatches = (n + 63u) / 64u;
	Scratch scratch(c);
	RecordingOff recOff{ c };
	uint32_t *rec = scratch.alloc<uint32_t>((size_t) n * cap), *recLen = scratch.alloc<uint32_t>(n), *order = scratch.alloc<uint32_t>(n);
	uint32_t *tr = scratch.alloc<uint32_t>((size_t) nBatches * cap * 64), *batchLen = scratch.alloc<uint32_t>(nBatches), *sink = scratch.alloc<uint32_t>(1);
	float4 *tmp = kind == 2 ? scratch.alloc<float4>((size_t) n * 2) : nullptr;
	if (!scratch.ok()) return scratch.finish("replay roof allocation");
	EventPair ev;
	HIPCHK(c, hipEventCreate(&ev.a)); HIPCHK(c, hipEventCreate(&ev.b));
	c->q.counters = c->counterSets; c->q.spill = mode == 1 ? c->spillShadow : c->spillClosest; c->q.dev_stats = nullptr;
	c->q.next = c->queueB;
	// the rays of the sample
	if (kind == 1) {
		// the camera rays of the pass rendered last, once more (its sampler tables are still in place)
		launch_generate(s, c->dsc, c->paths, lp.cfg, c->pixelList + lp.base, lp.nSlots, nullptr, lp.nPaths, c->queueA);
		HIPCHK(c, hipGetLastError());
		c->lastPass.valid = false;             // the path records no longer hold that pass
	}
	if (kind == 2) {
		// any-hit rays are addressed by their queue position: the sampled slots move to the front of the shadow queue, origin
		// (with the path id in its w) and direction.  The launches below run as the bounces launch this class of rays, with
		// the direct-light terms parked in the records (DQueues::nee_parked): they write a cancel for every occluded ray of
		// the sample, into records of a frame that is already accumulated, and read no term
		launch_gather_strided(s, tmp, c->paths.shq_o, n, stride); launch_gather_strided(s, tmp + n, c->paths.shq_d, n, stride);
		HIPCHK(c, hipMemcpyAsync(c->paths.shq_o, tmp, (size_t) n * sizeof(float4), hipMemcpyDeviceToDevice, s));
		HIPCHK(c, hipMemcpyAsync(c->paths.shq_d, tmp + n, (size_t) n * sizeof(float4), hipMemcpyDeviceToDevice, s));
		c->lastPass.shadowMax = 0;             // the queue is no longer the frame's
	} else {
		// every stride-th path record, its ray copied into queue order the way the bounces hand rays to this kernel
		launch_iota_strided(s, c->queueA, n, stride);
		launch_gather_strided(s, c->rayqA[0], c->paths.base + 0, n, stride * kPathSlots);
		launch_gather_strided(s, c->rayqA[1], c->paths.base + 1, n, stride * kPathSlots);
		rayQueues(c, c->queueA, nullptr);
	}
	RayQueuesOff rqOff{ c };
	c->q.nee_parked = mode == 1 ? 1u : 0u;
	c->q.miss_settled = 0;
	const uint32_t *queue = mode == 1 ? c->q.shadow : c->queueA;
	// 1. the counting kernel records what every ray asks for
	HIPCHK(c, hipMemsetAsync(recLen, 0, (size_t) n * 4, s));
	HIPCHK(c, hipMemsetAsync(c->q.trace_counts, 0, kNumTraceCounts * sizeof(unsigned long long), s));
	HIPCHK(c, hipMemsetAsync(c->q.counters, 0, kCounterSetBytes, s));
	c->q.rec = rec; c->q.rec_len = recLen; c->q.rec_cap = cap;
	launch_trace(s, mode, true, bin, c->dsc, c->paths, c->q, queue, n, coherent);
	c->q.rec = c->q.rec_len = nullptr; c->q.rec_cap = 0;
	HIPCHK(c, hipGetLastError());
	std::vector<uint32_t> len(n);
	HIPCHK(c, hipMemcpyAsync(len.data(), recLen, (size_t) n * 4, hipMemcpyDeviceToHost, s));
	HIPCHK(c, hipStreamSynchronize(s));
	unsigned long long cnt[kNumTraceCounts];
	HIPCHK(c, hipMemcpy(cnt, c->q.trace_counts, sizeof(cnt), hipMemcpyDeviceToHost));
	// 2. rays by decreasing list length, 64 to a batch (lanes of a replay wave then finish together); a counting sort
	std::vector<uint32_t> ord(n), first(cap + 2, 0u);
	unsigned long long total = 0, truncated = 0;
	for (uint32_t i = 0; i < n; ++i) { const uint32_t l = std::min(len[i], cap); total += l; if (len[i] > cap) ++truncated; first[cap - l + 1]++; }
	for (uint32_t l = 0; l <= cap; ++l) first[l + 1] += first[l];
	for (uint32_t i = 0; i < n; ++i) ord[first[cap - std::min(len[i], cap)]++] = i;
	HIPCHK(c, hipMemcpyAsync(order, ord.data(), (size_t) n * 4, hipMemcpyHostToDevice, s));
	launch_build_replay(s, rec, recLen, order, n, cap, tr, batchLen);
	HIPCHK(c, hipGetLastError());
	// 3. the product kernel and the replay on the same rays, best of `reps`
	float prodMs = 1e30f, replayMs = 1e30f;
	for (int i = 0; i <= reps; ++i) {            // round 0 warms up
		HIPCHK(c, hipMemsetAsync(c->q.counters, 0, kCounterSetBytes, s));
		HIPCHK(c, hipEventRecord(ev.a, s));
		launch_trace(s, mode, false, bin, c->dsc, c->paths, c->q, queue, n, coherent);
		HIPCHK(c, hipEventRecord(ev.b, s));
		HIPCHK(c, hipEventSynchronize(ev.b));
		float ms = 0; HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
		if (i && ms < prodMs) prodMs = ms;
		HIPCHK(c, hipEventRecord(ev.a, s));
		launch_replay(s, c->dsc, c->paths, c->q, tr, batchLen, nBatches, cap, 0u, sink);
		HIPCHK(c, hipEventRecord(ev.b, s));
		HIPCHK(c, hipEventSynchronize(ev.b));
		HIPCHK(c, hipEventElapsedTime(&ms, ev.a, ev.b));
		if (i && ms < replayMs) replayMs = ms;
	}
	out[0] = (double) n; out[1] = (double) total; out[2] = (double) truncated;
	out[3] = prodMs; out[4] = replayMs;
	out[5] = (double) cnt[kCntPairGlobal]; out[6] = (double) cnt[kCntPairLds]; out[7] = (double) cnt[kCntNodeGlobal]; out[8] = (double) cnt[kCntNodeLds];
	out[9] = (double) cnt[kCntHead]; out[10] = (double) cnt[kCntTail]; out[11] = (double) cnt[kCntSpill];
	return 0;
}

int mtsgpu_ld_tables(mtsgpu_ctx *c, uint32_t pixel_key, float *out1d, float *out2d) {
	if (!c || !out1d || !out2d) return fail(c, MTSGPU_EINVAL, "null argument");
	if (c->samplerKind != MTSGPU_SAMPLER_LD_KEYED) return fail(c, MTSGPU_ESTATE, "sampler is not the low-discrepancy sampler");
	HIPCHK(c, hipSetDevice(c->device));
	const uint32_t spp = effectiveSpp(c);
	const int depth = c->ldDepth;
	int rc = c->ldScr.ensure(c, (size_t) 3 * depth); if (rc) return rc;
	rc = c->ldPerm.ensure(c, (size_t) 2 * depth * spp); if (rc) return rc;
	rc = ensureTableWork(c, 1, spp); if (rc) return rc;
	c->renderListValid = false; c->lastPass.valid = false;
	rc = c->pixelList.ensure(c, 1); if (rc) return rc;
	HIPCHK(c, hipMemcpyAsync(c->pixelList, &pixel_key, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	DConfig cfg{};
	cfg.spp = spp; cfg.ld_depth = depth; cfg.seed = c->seed; cfg.sampler_kind = 1;
	launch_ld_tables(c->stream, cfg, c->pixelList, 1, c->ldScr, c->ldPerm, c->ldState, c->ldScratch);
	HIPCHK(c, hipGetLastError());
	std::vector<uint32_t> scr((size_t) 3 * depth);
	std::vector<uint16_t> perm((size_t) 2 * depth * spp);
	HIPCHK(c, hipMemcpyAsync(scr.data(), c->ldScr, scr.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpyAsync(perm.data(), c->ldPerm, perm.size() * sizeof(uint16_t), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	// the u32 -> f32 step of ldsampler.cpp:111,117 on the device-generated integer tables
	for (int i = 0; i < depth; ++i)
		for (uint32_t k = 0; k < spp; ++k) {
			out1d[(size_t) i * spp + k] = u32ToUnit(vdcBits(perm[((size_t) 2 * i) * spp + k], scr[3 * i]));
			const uint32_t p = perm[((size_t) 2 * i + 1) * spp + k];
			out2d[((size_t) i * spp + k) * 2 + 0] = u32ToUnit(vdcBits(p, scr[3 * i + 1]));
			out2d[((size_t) i * spp + k) * 2 + 1] = u32ToUnit(sobol2Bits(p, scr[3 * i + 2]));
		}
	return 0;
}

int mtsgpu_random_values(mtsgpu_ctx *c, int op, uint64_t seed, uint64_t arg, uint32_t clone, uint32_t n, uint64_t *out) {
	if (!c || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	if (op < 0 || op > 3 || n == 0 || n > (1u << 20) || clone > 64 || (op == 2 && arg == 0)) return fail(c, MTSGPU_EINVAL, "bad Random request");
	Scratch s(c);
	void *state = s.alloc<unsigned char>(random_state_bytes());
	unsigned long long *dOut = s.alloc<unsigned long long>(n);
	if (s.ok()) launch_random_values(c->stream, state, op, seed, arg, clone, n, dOut);
	s.get((unsigned long long *) out, dOut, n);
	return s.finish("Random on the device");
}

int mtsgpu_sampler_values(mtsgpu_ctx *c, uint32_t pixel_key, uint32_t sample_index, uint32_t n, int two_d, float *out) {
	if (!c || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	if (n == 0) return 0;
	const uint32_t spp = effectiveSpp(c);
	if (n > 4096u || sample_index >= spp) return fail(c, MTSGPU_EINVAL, "sample index or count out of range");
	HIPCHK(c, hipSetDevice(c->device));
	c->renderListValid = false; c->lastPass.valid = false;
	int rc = c->pixelList.ensure(c, 1); if (rc) return rc;
	HIPCHK(c, hipMemcpyAsync(c->pixelList, &pixel_key, sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	if (samplerHasTables(c)) {
		rc = c->ldScr.ensure(c, (size_t) 3 * c->ldDepth); if (rc) return rc;
		rc = c->ldPerm.ensure(c, (size_t) 2 * c->ldDepth * spp); if (rc) return rc;
		rc = ensureTableWork(c, 1, spp); if (rc) return rc;
	}
	const int integratorSaved = c->integrator;
	c->integrator = 0;                               // no sample arrays: the plain next1D / next2D sequence
	const DConfig cfg = makeConfig(c, true);
	c->integrator = integratorSaved;
	if (samplerHasTables(c))
		launch_ld_tables(c->stream, cfg, c->pixelList, 1, c->ldScr, c->ldPerm, c->ldState, c->ldScratch);
	Scratch s(c);
	const size_t nOut = (size_t) n * (two_d ? 2 : 1);
	float *dOut = s.alloc<float>(nOut);
	if (s.ok()) launch_sampler_values(c->stream, cfg, pixel_key, sample_index, n, two_d, dOut);
	s.get(out, dOut, nOut);
	return s.finish("sampler read-out");
}

int mtsgpu_bsdf_eval(mtsgpu_ctx *c, uint32_t bsdf_type, const float *params, int op, uint32_t n, const float *queries, float *out) {
	if (!c || !params || !queries || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	if (int rc = checkBsdfRequest(c, bsdf_type, op, "a composite needs its children: use mtsgpu_bsdf_eval_table")) return rc;
	if (n == 0) return 0;
	if (int rc = checkRecordCount(c, n)) return rc;
	Scratch s(c);
	const float *dQ = s.put(queries, (size_t) n * 6);
	float *dOut = s.alloc<float>((size_t) n * 8);
	if (s.ok()) launch_bsdf_eval(c->stream, bsdf_type, params, op, n, dQ, dOut);
	s.get(out, dOut, (size_t) n * 8);
	return s.finish("BSDF read-out");
}

int mtsgpu_bsdf_eval_table(mtsgpu_ctx *c, uint32_t n_bsdfs, const uint32_t *types, const float *params, uint32_t index, int op,
                           uint32_t n, const float *queries, float *out) {
	if (!c || !types || !params || !queries || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	if (index >= n_bsdfs || n_bsdfs > (1u << 24) || op < 0 || op > 2) return fail(c, MTSGPU_EINVAL, "bad BSDF index or operation");
	const std::string why = checkBsdfTable(n_bsdfs, types, params);
	if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
	if (n == 0) return 0;
	if (int rc = checkRecordCount(c, n)) return rc;
	Scratch s(c);
	const float *dQ = s.put(queries, (size_t) n * 6);
	float *dOut = s.alloc<float>((size_t) n * 8);
	const float *dP = s.put(params, (size_t) n_bsdfs * MTSGPU_BSDF_NPARAMS);
	const uint32_t *dT = s.put(types, n_bsdfs);
	if (s.ok()) launch_bsdf_eval_table(c->stream, dT, dP, index, op, n, dQ, dOut);
	s.get(out, dOut, (size_t) n * 8);
	return s.finish("BSDF read-out");
}

int mtsgpu_bsdf_eval_colored(mtsgpu_ctx *c, uint32_t bsdf_type, const float *params, uint32_t slots, const float color[3], int op,
                             uint32_t n, const float *queries, float *out) {
	if (!c || !params || !color || !queries || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	if (int rc = checkBsdfRequest(c, bsdf_type, op, "a composite has no texture slot of its own, and its children take no vertex colours")) return rc;
	if (slots >> bsdfColorSlotCount(bsdf_type))
		return fail(c, MTSGPU_EINVAL, "vertex-colour slot mask %u names a slot beyond the %d texture slot(s) of BSDF type %u", slots, bsdfColorSlotCount(bsdf_type), bsdf_type & 0xFFu);
	if (n == 0) return 0;
	if (int rc = checkRecordCount(c, n)) return rc;
	Scratch s(c);
	const float *dQ = s.put(queries, (size_t) n * 6);
	float *dOut = s.alloc<float>((size_t) n * 8);
	if (s.ok()) launch_bsdf_eval_colored(c->stream, bsdf_type, params, slots, color, op, n, dQ, dOut);
	s.get(out, dOut, (size_t) n * 8);
	return s.finish("BSDF read-out");
}

int mtsgpu_vertex_color_eval(mtsgpu_ctx *c, uint32_t n, const uint32_t *prim, const float *uv, float *out) {
	if (!c || !prim || !uv || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	if (!c->haveScene || !c->colors.d.tri_col) return fail(c, MTSGPU_ESTATE, "no vertex colours are set (mtsgpu_set_vertex_colors)");
	if (int rc = checkRecordCount(c, n)) return rc;
	if (int rc = checkPrimitives(c, n, prim)) return rc;
	if (n == 0) return 0;
	Scratch s(c);
	const uint32_t *dP = s.put(prim, n);
	const float *dUV = s.put(uv, (size_t) n * 2);
	float *dOut = s.alloc<float>((size_t) n * 3);
	if (s.ok()) launch_vertex_color_eval(c->stream, c->colors.d.tri_col, n, dP, dUV, dOut);
	s.get(out, dOut, (size_t) n * 3);
	return s.finish("vertex-colour read-out");
}

int mtsgpu_bsdf_eval_slots(mtsgpu_ctx *c, uint32_t bsdf_type, const float *params, const int32_t slot_source[2], const float color[3],
                           const float *values, int op, uint32_t n, const float *queries, float *out) {
	if (!c || !params || !slot_source || !color || !values || !queries || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	if (int rc = checkBsdfRequest(c, bsdf_type, op, "a composite has no texture slot of its own, and its children take no textures")) return rc;
	int src[2];
	for (int s = 0; s < 2; ++s) {
		src[s] = slot_source[s];
		if (src[s] < kSlotBlock || src[s] > kSlotTexture) return fail(c, MTSGPU_EINVAL, "slot %d: unknown source %d", s, src[s]);
		if (src[s] != kSlotBlock && s >= bsdfColorSlotCount(bsdf_type))
			return fail(c, MTSGPU_EINVAL, "slot %d lies beyond the %d texture slot(s) of BSDF type %u", s, bsdfColorSlotCount(bsdf_type), bsdf_type & 0xFFu);
	}
	if (n == 0) return 0;
	if (int rc = checkRecordCount(c, n)) return rc;
	Scratch s(c);
	const float *dQ = s.put(queries, (size_t) n * 6);
	float *dOut = s.alloc<float>((size_t) n * 8);
	if (s.ok()) launch_bsdf_eval_slots(c->stream, bsdf_type, params, src, color, values, op, n, dQ, dOut);
	s.get(out, dOut, (size_t) n * 8);
	return s.finish("BSDF read-out");
}

int mtsgpu_bsdf_eval_masked(mtsgpu_ctx *c, uint32_t bsdf_type, const float *params, const float opacity[3], int op, uint32_t n,
                            const float *queries, float *out) {
	if (!c || !params || !opacity || !queries || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	if (int rc = checkBsdfRequest(c, bsdf_type, op, "a mask around a composite is not supported")) return rc;
	if (n == 0) return 0;
	if (int rc = checkRecordCount(c, n)) return rc;
	Scratch s(c);
	const float *dQ = s.put(queries, (size_t) n * 6);
	float *dOut = s.alloc<float>((size_t) n * 8);
	if (s.ok()) launch_bsdf_eval_masked(c->stream, bsdf_type, params, opacity, op, n, dQ, dOut);
	s.get(out, dOut, (size_t) n * 8);
	return s.finish("BSDF read-out");
}

int mtsgpu_bsdf_eval_snow(mtsgpu_ctx *c, uint32_t bsdf_type, const mtsgpu_bsdf_snow *entry, int op, uint32_t n, const float *queries, float *out) {
	if (!c || !entry || !queries || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	if ((bsdf_type & ~(uint32_t) MTSGPU_BSDF_TWOSIDED) != (uint32_t) MTSGPU_BSDF_LAMBERTIAN || op < 0 || op > 2)
		return fail(c, MTSGPU_EINVAL, "bad BSDF type or operation: a snow record sits on a Lambertian entry (twosided allowed)");
	{
		const std::string why = checkSnowEntry(*entry, bsdf_type);
		if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
	}
	if (n == 0) return 0;
	if (int rc = checkRecordCount(c, n)) return rc;
	Scratch s(c);
	const float *dQ = s.put(queries, (size_t) n * 6);
	float *dOut = s.alloc<float>((size_t) n * 8);
	DSnow e;
	std::memcpy(&e, entry, sizeof(e));
	if (s.ok()) launch_bsdf_eval_snow(c->stream, bsdf_type, e, op, n, dQ, dOut);
	s.get(out, dOut, (size_t) n * 8);
	return s.finish("BSDF read-out");
}

int mtsgpu_bsdf_eval_cloth(mtsgpu_ctx *c, uint32_t bsdf_type, const mtsgpu_weave *weave, int op, uint32_t n, const float *queries, float *out) {
	if (!c || !weave || !queries || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	if ((bsdf_type & ~(uint32_t) MTSGPU_BSDF_TWOSIDED) != (uint32_t) MTSGPU_BSDF_LAMBERTIAN || op < 0 || op > 3)
		return fail(c, MTSGPU_EINVAL, "bad BSDF type or operation: a weave sits on a Lambertian entry (twosided allowed)");
	{
		const std::string why = checkWeave(*weave);
		if (!why.empty()) return fail(c, MTSGPU_EINVAL, "weave: %s", why.c_str());
	}
	if (n == 0) return 0;
	if (int rc = checkRecordCount(c, n)) return rc;
	// the casts of f at the extremes of the queries' texcoords, as the setter checks them on a shape
	{
		double uMin = 0, uMax = 0, vMin = 0, vMax = 0;
		for (uint32_t i = 0; i < n; ++i) {
			const float u = queries[8 * (size_t) i + 6], v = queries[8 * (size_t) i + 7];
			if (!(std::fabs(u) <= 3.4028235e38f) || !(std::fabs(v) <= 3.4028235e38f)) return fail(c, MTSGPU_EINVAL, "query %u: non-finite texcoord", i);
			if (i == 0) { uMin = uMax = u; vMin = vMax = v; }
			uMin = std::min(uMin, (double) u); uMax = std::max(uMax, (double) u); vMin = std::min(vMin, (double) v); vMax = std::max(vMax, (double) v);
		}
		const std::string why = clothCastRange(*weave, uMin, uMax, vMin, vMax);
		if (!why.empty()) return fail(c, MTSGPU_EINVAL, "weave: %s", why.c_str());
	}
	Scratch s(c);
	const float *dQ = s.put(queries, (size_t) n * 8);
	const uint32_t *dP = s.put(weave->pattern, (size_t) weave->n_pattern);
	const DYarn *dY = s.put(reinterpret_cast<const DYarn *>(weave->yarns), (size_t) weave->n_yarns);
	float *dOut = s.alloc<float>((size_t) n * 8);
	DWeave w;
	std::memset(&w, 0, sizeof(w));
	std::memcpy(&w, weave, offsetof(mtsgpu_weave, pattern));
	if (s.ok()) launch_bsdf_eval_cloth(c->stream, bsdf_type, w, dP, dY, op, n, dQ, dOut);
	s.get(out, dOut, (size_t) n * 8);
	return s.finish("BSDF read-out");
}

int mtsgpu_cloth_check(const mtsgpu_weave *weave, const float *uv_range) {
	if (!weave) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	std::string why = checkWeave(*weave);
	if (why.empty() && uv_range) why = clothCastRange(*weave, uv_range[0], uv_range[1], uv_range[2], uv_range[3]);
	if (!why.empty()) return fail(nullptr, MTSGPU_EINVAL, "weave: %s", why.c_str());
	return 0;
}

int mtsgpu_devmath(int fn, uint32_t n, const float *x, const float *y, float *out) {
	if (!x || !out || (fn == 7 && !y)) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	if (fn < 0 || fn > 10) return fail(nullptr, MTSGPU_EINVAL, "unknown function %d", fn);
	for (uint32_t i = 0; i < n; ++i) {
		const float a = x[i];
		out[i] = fn == 0 ? dsin(a) : fn == 1 ? dcos(a) : fn == 2 ? dtan(a) : fn == 3 ? dexp(a) : fn == 4 ? dlog(a) : fn == 5 ? datan(a)
		       : fn == 6 ? dacos(a) : fn == 7 ? datan2(a, y[i]) : fn == 8 ? dsinh(a) : fn == 9 ? dcosh(a) : dpow15(a);
	}
	return 0;
}

int mtsgpu_uv_texture_eval(mtsgpu_ctx *c, const mtsgpu_uv_texture *tex, uint32_t n, const uint32_t *prim, const float *rec, float *out) {
	if (!c || !tex || !prim || !rec || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	if (!c->haveScene) return fail(c, MTSGPU_ESTATE, "mtsgpu_uv_texture_eval before mtsgpu_upload_scene");
	const std::string why = checkUvTexture(*tex);
	if (!why.empty()) return fail(c, MTSGPU_EINVAL, "texture: %s", why.c_str());
	if (int rc = checkRecordCount(c, n)) return rc;
	if (int rc = checkPrimitives(c, n, prim)) return rc;
	if (n == 0) return 0;
	Scratch s(c);
	const uint32_t *dP = s.put(prim, n);
	const float *dRec = s.put(rec, (size_t) n * 3);
	float *dOut = s.alloc<float>((size_t) n * 5);
	const float4 *triUv = c->tex.d.tri_uv;
	if (!triUv) triUv = s.zeros<float4>(kTriUvStride * ((size_t) c->nTris + 1));      // no texcoords set: every mesh reads zero rows
	if (s.ok()) {
		DTexture t;
		std::memcpy(&t, tex, sizeof t);
		launch_uv_texture_eval(c->stream, c->dsc, triUv, t, n, dP, dRec, dOut);
	}
	s.get(out, dOut, (size_t) n * 5);
	return s.finish("uv-texture read-out");
}

int mtsgpu_bitmap_texture_eval(mtsgpu_ctx *c, const mtsgpu_uv_texture *tex, const mtsgpu_bitmap *bitmap, uint32_t n, const uint32_t *prim,
                               const float *rec, float *out) {
	if (!c || !tex || !bitmap || !prim || !rec || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	if (!c->haveScene) return fail(c, MTSGPU_ESTATE, "mtsgpu_bitmap_texture_eval before mtsgpu_upload_scene");
	if (tex->kind != (uint32_t) MTSGPU_TEX_BITMAP) return fail(c, MTSGPU_EINVAL, "texture: kind %u is not a bitmap", tex->kind);
	std::string why = checkUvTexture(*tex, true);
	if (!why.empty()) return fail(c, MTSGPU_EINVAL, "texture: %s", why.c_str());
	uint64_t nTexels = 0;
	why = checkBitmap(*bitmap, &nTexels);
	if (!why.empty()) return fail(c, MTSGPU_EINVAL, "bitmap: %s", why.c_str());
	if (int rc = checkRecordCount(c, n)) return rc;
	if (int rc = checkPrimitives(c, n, prim)) return rc;
	if (n == 0) return 0;
	std::vector<float> pool(4 * (size_t) nTexels);
	packBitmapTexels(*bitmap, pool.data());
	Scratch s(c);
	const uint32_t *dP = s.put(prim, n);
	const float *dRec = s.put(rec, (size_t) n * 3);
	const float *dTexels = s.put(pool.data(), pool.size());
	float *dOut = s.alloc<float>((size_t) n * 5);
	const float4 *triUv = c->tex.d.tri_uv;
	if (!triUv) triUv = s.zeros<float4>(kTriUvStride * ((size_t) c->nTris + 1));      // no texcoords set: every mesh reads zero rows
	if (s.ok()) {
		DTexture t;
		std::memcpy(&t, tex, sizeof t);
		t.width = bitmap->width; t.height = bitmap->height; t.wrap = bitmap->wrap_mode; t.first = 0u;
		t.reserved[0] = t.reserved[1] = t.reserved[2] = 0u;
		launch_bitmap_texture_eval(c->stream, c->dsc, triUv, t, reinterpret_cast<const float4 *>(dTexels), n, dP, dRec, dOut);
	}
	s.get(out, dOut, (size_t) n * 5);
	return s.finish("bitmap-texture read-out");
}

int mtsgpu_shading_frame_eval(mtsgpu_ctx *c, uint32_t n, const uint32_t *prim, const float *rec, float *out) {
	if (!c || !prim || !rec || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	if (!c->haveScene) return fail(c, MTSGPU_ESTATE, "mtsgpu_shading_frame_eval before mtsgpu_upload_scene");
	if (int rc = checkRecordCount(c, n)) return rc;
	if (int rc = checkPrimitives(c, n, prim)) return rc;
	if (n == 0) return 0;
	Scratch s(c);
	const uint32_t *dP = s.put(prim, n);
	const float *dRec = s.put(rec, (size_t) n * 3);
	float *dOut = s.alloc<float>((size_t) n * 9);
	DTangents tan = c->tan.d;
	// no tangents uploaded: every shape reads a zero flag, and tri_dpdu is never touched
	if (!tan.shape_has_tan) tan.shape_has_tan = s.zeros<uint32_t>(c->host.shapeBsdf.size() + 1);
	if (s.ok()) launch_shading_frame_eval(c->stream, c->dsc, tan, n, dP, dRec, dOut);
	s.get(out, dOut, (size_t) n * 9);
	return s.finish("shading-frame read-out");
}

int mtsgpu_sky_configure(const float *block, float *derived) {
	if (!block || !derived) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	skyConfigure(block, derived);
	return 0;
}

int mtsgpu_wiscombe_configure(const float *raw, mtsgpu_bsdf_snow *out) {
	if (!raw || !out) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	std::memset(out, 0, sizeof(*out));
	out->kind = MTSGPU_SNOW_WISCOMBE;
	snowWiscombeConfigure(raw, out->derived);
	static const char *const names[4] = { "wStar", "bStar", "xi", "P" };
	const int bad = snowFirstNonFinite(*out);
	if (bad >= 0) return fail(nullptr, MTSGPU_EINVAL, "Wiscombe: %s[%d] is not finite (g = %g, w0 = %g %g %g)", names[bad / 3], bad % 3, raw[0], raw[2], raw[3], raw[4]);
	return 0;
}

int mtsgpu_hk_configure(const float *raw, mtsgpu_bsdf_snow *out) {
	if (!raw || !out) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	std::memset(out, 0, sizeof(*out));
	out->kind = MTSGPU_SNOW_HK;
	snowHkConfigure(raw, out->derived);
	static const char *const names[12] = { "albedo[0]", "albedo[1]", "albedo[2]", "ssFactor[0]", "ssFactor[1]", "ssFactor[2]",
	                                       "diffuseReflectance[0]", "diffuseReflectance[1]", "diffuseReflectance[2]", "g", "eta", "the flag" };
	const int bad = snowFirstNonFinite(*out);
	if (bad >= 0) return fail(nullptr, MTSGPU_EINVAL, "HanrahanKrueger: %s is not finite (sigmaA + sigmaS = %g %g %g, etaInt / etaExt = %g / %g)", names[bad],
	                          raw[0] + raw[3], raw[1] + raw[4], raw[2] + raw[5], raw[7], raw[8]);
	return 0;
}

int mtsgpu_lum_eval(mtsgpu_ctx *c, uint32_t lum_type, const float *block, int op, uint32_t n, const float *queries, float *out) {
	if (!c || !block || !queries || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	if (lum_type != (uint32_t) MTSGPU_LUM_SKY) return fail(c, MTSGPU_EINVAL, "luminaire type %u is not served by this read-out (sky only)", lum_type);
	if (op < 0 || op > 2) return fail(c, MTSGPU_EINVAL, "bad luminaire operation");
	float host[MTSGPU_LUM_NPARAMS + MTSGPU_SKY_NDERIVED];
	{
		const std::string why = checkSkyLuminaire(0, block, 0, host + MTSGPU_LUM_NPARAMS);
		if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
	}
	if (n == 0) return 0;
	if (int rc = checkRecordCount(c, n)) return rc;
	std::memcpy(host, block, sizeof(float) * MTSGPU_LUM_NPARAMS);
	Scratch s(c);
	const float *dQ = s.put(queries, (size_t) n * 6);
	float *dOut = s.alloc<float>((size_t) n * 12);
	const float *dB = s.put(host, sizeof(host) / sizeof(float));
	if (s.ok()) s.check(hipStreamSynchronize(c->stream));       // `host` lives on this stack
	if (s.ok()) launch_sky_eval(c->stream, dB, op, n, dQ, dOut);
	s.get(out, dOut, (size_t) n * 12);
	return s.finish("luminaire read-out");
}

int mtsgpu_spot_eval(mtsgpu_ctx *c, const float *block, const mtsgpu_uv_texture *tex, const mtsgpu_bitmap *bitmap, uint32_t bilinear, uint32_t n,
                     const float *p, float *out) {
	if (!c || !block || !tex || !p || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	const bool isBitmap = tex->kind == (uint32_t) MTSGPU_TEX_BITMAP;
	if (isBitmap != (bitmap != nullptr)) return fail(c, MTSGPU_EINVAL, "a bitmap goes with a texture of kind MTSGPU_TEX_BITMAP and with no other");
	// the block as the flattener completes it (SpotLuminaire::configure, spot.cpp:56-60), checked as the call on a scene checks it
	float host[MTSGPU_LUM_NPARAMS];
	std::memcpy(host, block, sizeof host);
	host[6] = std::cos(host[19]); host[7] = std::cos(host[8]); host[9] = 1.0f / (host[8] - host[19]);
	const uint32_t lumType = MTSGPU_LUM_SPOT, flag = bilinear;
	const int32_t zero = 0;
	SpotPlan plan;
	const SpotArgs a{ 1u, tex, isBitmap ? 1u : 0u, bitmap, &zero, &flag, &zero };
	const std::string why = planSpots(1u, &lumType, host, a, false, false, false, plan);
	if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
	if (int rc = checkRecordCount(c, n)) return rc;
	if (n == 0) return 0;
	Scratch s(c);
	const float *dB = s.put(host, (size_t) MTSGPU_LUM_NPARAMS);
	const float *dP = s.put(p, (size_t) n * 3);
	const float *dTexels = plan.pool.empty() ? nullptr : s.put(plan.pool.data(), plan.pool.size());
	float *dOut = s.alloc<float>((size_t) n * 8);
	if (s.ok()) s.check(hipStreamSynchronize(c->stream));       // `host` and the plan live on this stack
	if (s.ok()) launch_spot_eval(c->stream, dB, plan.desc[0], reinterpret_cast<const float4 *>(dTexels), plan.uvFactor[0], n, dP, dOut);
	s.get(out, dOut, (size_t) n * 8);
	return s.finish("spot read-out");
}

int mtsgpu_scene_lum_eval(mtsgpu_ctx *c, int op, uint32_t n, const float *queries, float *out) {
	if (!c || !queries || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	if (!c->haveScene) return fail(c, MTSGPU_ESTATE, "mtsgpu_scene_lum_eval before mtsgpu_upload_scene");
	if (op < 0 || op > 2) return fail(c, MTSGPU_EINVAL, "bad luminaire operation");
	if (int rc = checkRecordCount(c, n)) return rc;
	const std::vector<uint32_t> &lumType = c->host.lumType;
	if (op == 1)      // the kernel indexes the luminaire tables with it
		for (uint32_t i = 0; i < n; ++i) {
			const float lf = queries[16 * (size_t) i + 12];
			if (!(lf >= 0.0f && lf < (float) lumType.size()) || lf != (float) (uint32_t) lf)
				return fail(c, MTSGPU_EINVAL, "record %u: luminaire index %g out of range", i, (double) lf);
			const uint32_t t = lumType[(uint32_t) lf];
			if (t != (uint32_t) MTSGPU_LUM_AREA && t != (uint32_t) MTSGPU_LUM_CONSTANT && t != (uint32_t) MTSGPU_LUM_ENVMAP && t != (uint32_t) MTSGPU_LUM_SKY)
				return fail(c, MTSGPU_EINVAL, "record %u: luminaire %u is a delta luminaire (type %u), Scene::pdfLuminaire is never asked for one", i, (uint32_t) lf, t);
		}
	if (op == 2 && c->dsc.background_lum < 0) return fail(c, MTSGPU_EINVAL, "the scene has no background luminaire");
	if (n == 0) return 0;
	Scratch s(c);
	const float *dQ = s.put(queries, (size_t) n * 16);
	float *dOut = s.alloc<float>((size_t) n * 16);
	if (s.ok()) launch_scene_lum_eval(c->stream, c->dsc, op, n, dQ, dOut, c->spots.d);
	s.get(out, dOut, (size_t) n * 16);
	return s.finish("scene luminaire read-out");
}

} // extern "C"
