// render.cpp -- the wavefront engine behind mtsgpu_render (include/mtsgpu.h): the per-pass buffers, the host loops that
// drive the traversal and shading stages per bounce, and the entry points that run them (mtsgpu_render, mtsgpu_trace_rays,
// mtsgpu_li_samples), run their first stage alone (mtsgpu_camera_rays) or read their records back (mtsgpu_pass_samples,
// mtsgpu_bin_entries).
#include "ctx.h"
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <cstdlib>

using namespace mg;

namespace {

// size of the full film the crop window lies in (film.cpp:33-41); without a crop window the film itself
int filmWidth(const mtsgpu_ctx *c) { return c->cam.film_width > 0 ? c->cam.film_width : c->cam.width; }
int filmHeight(const mtsgpu_ctx *c) { return c->cam.film_height > 0 ? c->cam.film_height : c->cam.height; }

// Which part renders tile (tx, ty): the bits of tx and ty interleaved (tx lowest) modulo the number of parts, so the
// parts sample the image on a 2-D lattice (mtsgpu_set_tiles in include/mtsgpu.h; the same function lives in
// oracle/orc_render.c and filmreduce.py)
uint32_t tileMorton(uint32_t tx, uint32_t ty) {
	uint32_t m = 0;
	for (int b = 0; b < 16; ++b)
		m |= ((tx >> b) & 1u) << (2 * b) | ((ty >> b) & 1u) << (2 * b + 1);
	return m;
}

// The "lean_closest" knob when nobody set it (traceAndBin: which closest-hit launches run the kernel without the mailbox): the
// incoherent launches of at least plainBelow rays and the coherent first launch, which measured faster with it; the launches
// below plainBelow showed no difference and keep the kernel with the mailbox (profiles/r19_lean_closest_ab.txt)
constexpr long kLeanClosestDefault = 3;

long tuningOr(const mtsgpu_ctx *c, const char *key, long dflt) {
	auto it = c->tuning.find(key);
	return it == c->tuning.end() ? dflt : it->second;
}

} // namespace

// scheduling parameters of k_trace: the defaults, or what mtsgpu_set_tuning asked for
void mg::applyTuning(mtsgpu_ctx *c) {
	const auto get = [&](const char *key, long dflt) { return tuningOr(c, key, dflt); };
	c->q.refill_min = (uint32_t) get("refill_min", 32);
	c->q.desc_min = (uint32_t) get("desc_min", 8);
	c->q.leaf_min = (uint32_t) get("leaf_min", 8);
	c->q.tune_refill = c->tuning.count("refill_min") ? 1u : 0u;
	c->q.tune_batch = (uint32_t) get("batch", 0);
	c->q.tune_dyn_div = (uint32_t) get("dyn_div", 0);
	c->q.tune_blocks_per_cu = (uint32_t) get("blocks_per_cu", 0);
	c->q.tune_plain_below = (uint32_t) get("plain_below", 0);
	c->q.tune_dyn_min_rounds = (uint32_t) get("dyn_min_rounds", 0);
	c->q.bin_hits = c->binHits;
}

// the samplers whose generate() fills per-pixel tables (permutations, scrambles)
bool mg::samplerHasTables(const mtsgpu_ctx *c) {
	return c->samplerKind == MTSGPU_SAMPLER_LD_KEYED || c->samplerKind == MTSGPU_SAMPLER_STRATIFIED_KEYED;
}

// what launch_ld_tables needs besides the tables: one stream word per slot and, above 512 samples per pixel, the scratch
// copy the tables are shuffled in
int mg::ensureTableWork(mtsgpu_ctx *c, size_t nSlots, uint32_t spp) {
	int rc = c->ldState.ensure(c, nSlots); if (rc) return rc;
	return c->ldScratch.ensure(c, ld_table_scratch_entries((uint32_t) nSlots, spp, c->ldDepth));
}

DConfig mg::makeConfig(const mtsgpu_ctx *c, bool slotPerPath) {
	DConfig cfg{};
	std::memcpy(cfg.r2c, c->cam.raster_to_camera, sizeof(cfg.r2c));
	std::memcpy(cfg.c2w, c->cam.camera_to_world, sizeof(cfg.c2w));
	cfg.near_clip = c->cam.near_clip; cfg.far_clip = c->cam.far_clip;
	cfg.aperture_radius = c->cam.aperture_radius; cfg.focus_depth = c->cam.focus_depth; cfg.camera_kind = c->cam.kind;
	cfg.width = c->cam.width; cfg.height = c->cam.height;
	cfg.crop_x = c->cam.crop_offset_x; cfg.crop_y = c->cam.crop_offset_y;
	cfg.pix_w = filmWidth(c); cfg.pix_off = 0;
	cfg.max_depth = c->maxDepth; cfg.rr_depth = c->rrDepth; cfg.strict_normals = c->strictNormals;
	cfg.integrator = c->integrator; cfg.n_lum = c->nLumSamples; cfg.n_bsdf = c->nBsdfSamples;
	// MIDirectIntegrator::configure (direct.cpp:51-56)
	cfg.weight_bsdf = 1 / (float) c->nBsdfSamples; cfg.weight_lum = 1 / (float) c->nLumSamples;
	cfg.frac_bsdf = c->nBsdfSamples / (float) (c->nLumSamples + c->nBsdfSamples);
	cfg.frac_lum = c->nLumSamples / (float) (c->nLumSamples + c->nBsdfSamples);
	cfg.sampler_kind = c->samplerKind;
	cfg.spp = effectiveSpp(c); cfg.ld_depth = c->ldDepth; cfg.seed = c->seed;
	cfg.strat_res = 1; while ((uint32_t) cfg.strat_res * (uint32_t) cfg.strat_res < cfg.spp) ++cfg.strat_res;
	cfg.slot_per_path = slotPerPath ? 1 : 0;
	cfg.ld_scr = c->ldScr; cfg.ld_perm = c->ldPerm; cfg.primes = c->primes;
	// MIDirectIntegrator::configureSampler (direct.cpp:58-63): the luminaire array first
	if (c->integrator == 1) {
		if (c->nLumSamples > 1) cfg.arr_size[cfg.arr_n++] = (uint32_t) c->nLumSamples;
		if (c->nBsdfSamples > 1) cfg.arr_size[cfg.arr_n++] = (uint32_t) c->nBsdfSamples;
		for (int a = 0; a < cfg.arr_n; ++a) { cfg.arr_off[a] = cfg.arr_total; cfg.arr_total += cfg.spp * cfg.arr_size[a]; }
	}
	cfg.arr_scr = c->arrScr; cfg.arr_perm = c->arrPerm; cfg.arr_pts = c->arrPts;
	cfg.filt_size_x = c->filtSizeX; cfg.filt_size_y = c->filtSizeY; cfg.filt_border = c->filtBorder; cfg.filt_values = c->filtValues;
	// Without a background luminaire a ray that leaves the scene ends its path and adds nothing: the records are kept so that
	// such a ray needs no shading (kernels.h: DConfig::miss_settled).  The rounds of MIDirectIntegrator keep the shaded route,
	// and so does the "miss_shaded" knob at 1 (A/B runs, tests)
	const bool rounds = c->integrator == 1 && (c->nLumSamples > 1 || c->nBsdfSamples > 1);
	cfg.miss_settled = (c->dsc.background_lum < 0 && !rounds && tuningOr(c, "miss_shaded", 0) != 1) ? 1 : 0;
	return cfg;
}

// The rays of the two closest-hit queues in queue order (kernels.h: DPaths::rq_*): the traversal reads those of `cur`, the
// kernel that fills `nxt` writes them.  NULL (or the "ray_queues" knob at 0): records only.
void mg::rayQueues(mtsgpu_ctx *c, const uint32_t *cur, const uint32_t *nxt) {
	const bool on = tuningOr(c, "ray_queues", 1) != 0;
	auto of = [&](const uint32_t *q, int k) -> float4 * { return !on || !q ? nullptr : (q == c->queueA ? c->rayqA[k] : (q == c->queueB ? c->rayqB[k] : nullptr)); };
	c->paths.rq_o = of(cur, 0); c->paths.rq_d = of(cur, 1); c->paths.rqn_o = of(nxt, 0); c->paths.rqn_d = of(nxt, 1);
}

namespace {

// Device bytes ensurePaths() allocates per path of a pass: the 128-byte record, the shadow ray (2 x 16), the eleven material
// bins sized for the all-in-one-bin case with a quarter of headroom (id 4 + hit 16 bytes per entry), the two next queues
// (id 4 + ray 32 bytes each), the shadow queue's ids and the redo list's -- about 519 bytes, 37 GB for the default pass of 72 M paths.
// (A frame that does not park its direct-light terms adds 16 bytes per path for them: ensureNeeQueue.)
constexpr size_t kBytesPerPath = kPathSlots * 16 + 2 * 16 + (size_t) (kNumBins * (4 + 16) * 5 / 4) + 2 * (4 + 32) + 4 + 4 + 4;
// Paths per pass when the caller set none (mtsgpu_set_options max_paths == 0): 72 M, or what 60 % of the free device memory
// holds if that is less (the sampler tables, the film and the scene of a later upload need room too)
uint64_t defaultMaxPaths(mtsgpu_ctx *c) {
	uint64_t paths = 72ull << 20;
	size_t freeB = 0, totalB = 0;
	if (hipMemGetInfo(&freeB, &totalB) == hipSuccess) {
		// what this context already holds for its passes is free for the next one
		uint64_t avail = (uint64_t) freeB + (uint64_t) c->pathCap * kBytesPerPath;
		// test-case mode: 16 bytes of statistics per film pixel (variance 3 x f32, count u32), if not allocated yet
		if (c->filmStats && !c->statVar) avail -= std::min<uint64_t>(avail, 16ull * (uint64_t) c->cam.width * (uint64_t) c->cam.height);
		paths = std::min<uint64_t>(paths, std::max<uint64_t>(1ull << 16, avail * 6 / 10 / kBytesPerPath));
	}
	return paths;
}

int ensurePaths(mtsgpu_ctx *c, size_t cap) {
	if (cap <= c->pathCap)
		return 0;
	freeAll(c->pathAllocs);
	c->pathCap = 0;
	cap = (cap + 255) & ~(size_t) 255;
	auto &o = c->pathAllocs;
	int rc = 0;
	rc |= devAlloc(c, &c->paths.base, cap * kPathSlots, o);
	rc |= devAlloc(c, &c->paths.shq_o, cap, o); rc |= devAlloc(c, &c->paths.shq_d, cap, o);
	// With static dealing every shard (workgroups with blockIdx % kBinShards == s) sees at most 1/kBinShards of the
	// 256-ray batches plus one per workgroup, and all of them may land in one bin.  The dynamically claimed tail of a
	// large launch (a quarter of the queue) goes to whichever waves are free, so a shard can take more than its share:
	// a quarter of headroom covers what was ever observed; k_trace drops entries beyond the capacity and
	// traceAndBin() repeats such a launch with static dealing, for which the bound holds by construction.
	const unsigned gridBlocksMax = c->nCUs * kTraceBlocksPerCuMax;
	const size_t segCap = cap / kBinShards + cap / (4 * kBinShards) + (size_t) kTraceBlock * (gridBlocksMax / kBinShards + 2);
	rc |= devAlloc(c, &c->q.bins_base, segCap * kBinShards * kNumBins, o);
	rc |= devAlloc(c, &c->binHits, segCap * kBinShards * kNumBins, o);
	applyTuning(c);                  // DQueues::bin_hits follows the allocation
	c->q.bin_stride = (uint32_t) (segCap * kBinShards);
	if (segCap * kBinShards > 0xFFFFFFFFull) return fail(c, MTSGPU_EINVAL, "pass too large");
	c->q.bin_seg_cap = (uint32_t) segCap;
	rc |= devAlloc(c, &c->queueA, cap, o); rc |= devAlloc(c, &c->queueB, cap, o);
	for (int k = 0; k < 2; ++k) { rc |= devAlloc(c, &c->rayqA[k], cap, o); rc |= devAlloc(c, &c->rayqB[k], cap, o); }
	rc |= devAlloc(c, &c->q.shadow, cap, o);
	rc |= devAlloc(c, &c->q.redo, cap, o);          // closest-hit rays on which two primitives tied (k_trace LEAN): traced again with the mailbox
	rc |= devAlloc(c, &c->counterSets, (size_t) kCounterSets * kNumCounters * kCounterStride, o);
	rc |= devAlloc(c, &c->viewsDev, kNumBins, o);
	rc |= devAlloc(c, &c->devStats, kNumDevStats, o);
	rc |= devAlloc(c, &c->q.trace_counts, kNumTraceCounts, o);
	rc |= devAlloc(c, &c->spillClosest, (size_t) gridBlocksMax * kTraceBlock * trace_spill_levels(), o);
	rc |= devAlloc(c, &c->spillShadow, (size_t) gridBlocksMax * kTraceBlock * trace_spill_levels(), o);
	if (rc) return rc;
	c->q.counters = c->counterSets; c->q.spill = c->spillClosest; c->q.dev_stats = nullptr;
	c->q.spill_stride = gridBlocksMax * kTraceBlock;
	c->q.n_cus = c->nCUs; c->q.force_static = 0;
	applyTuning(c);
	HIPCHK(c, hipMemset(c->q.trace_counts, 0, kNumTraceCounts * sizeof(unsigned long long)));
	c->q.rec = c->q.rec_len = nullptr; c->q.rec_cap = 0;
	c->pathCap = cap;
	return 0;
}

// buffers of the sample arrays for nSlots sampler slots (and of the saved camera hits for nPaths paths)
int ensureSampleArrays(mtsgpu_ctx *c, size_t nSlots, size_t nPaths) {
	if (c->integrator != 1 || (c->nLumSamples <= 1 && c->nBsdfSamples <= 1))
		return 0;
	if (c->samplerKind == MTSGPU_SAMPLER_HALTON || c->samplerKind == MTSGPU_SAMPLER_HAMMERSLEY)
		return fail(c, MTSGPU_EINVAL, "request2DArray() is not supported by QMC samplers! (halton.cpp:102-104, hammersley.cpp:112-114)");
	const uint32_t spp = effectiveSpp(c);
	size_t total = 0; int nArr = 0;
	for (int n : { c->nLumSamples, c->nBsdfSamples })
		if (n > 1) {
			if ((uint64_t) spp * (uint64_t) n > 65536ull)
				return fail(c, MTSGPU_EINVAL, "sampleCount x samples per strategy = %llu exceeds 65536 points per pixel", (unsigned long long) spp * n);
			total += (size_t) spp * n; ++nArr;
		}
	int rc = 0;
	if (c->nBsdfSamples > 1) { rc = c->primSave.ensure(c, 3 * nPaths); if (rc) return rc; }
	c->paths.prim = c->primSave;
	if (!samplerHasTables(c)) return 0;
	rc = c->ldState.ensure(c, nSlots); if (rc) return rc;
	if (c->samplerKind == MTSGPU_SAMPLER_LD_KEYED) {
		rc = c->arrScr.ensure(c, nSlots * nArr * 2); if (rc) return rc;
		rc = c->arrPerm.ensure(c, nSlots * total); if (rc) return rc;
	} else {
		rc = c->arrPts.ensure(c, nSlots * total); if (rc) return rc;
	}
	return 0;
}

// What a timed launch is: a traversal launch of one of the classes of ctx.h's traceEvClass, or the shading of a bounce
enum LaunchKind { kClosest = 0, kClosestFirst = 1, kAnyHit = 2, kShading = 3 };

// The one way the engine launches a stage: `launch` (a kernel, or the kernels of one shading step) on stream s, then the
// check that the device accepted it.  With time_kernels on the launch runs between a pair of events from the pool of its
// kind, and a traversal launch files its class next to its pair (collectTimings sums the classes apart).  The host counts
// the traversal launches of a frame that keeps no statistics on the device (device-driven bounces count theirs in k_prep).
// An event that cannot be created is MTSGPU_EHIP: no launch goes untimed silently.
template <typename F> int timedLaunch(mtsgpu_ctx *c, hipStream_t s, LaunchKind kind, F &&launch) {
	const bool shading = kind == kShading;
	std::pair<hipEvent_t, hipEvent_t> ev{ nullptr, nullptr };
	if (c->timeKernels) {
		EventPool &pool = shading ? c->shadeEvents : c->traceEvents;
		size_t &used = shading ? c->shadeEvUsed : c->traceEvUsed;
		if (used == pool.size()) {
			if (hipEventCreate(&ev.first) != hipSuccess || hipEventCreate(&ev.second) != hipSuccess) {
				if (ev.first) (void) hipEventDestroy(ev.first);
				return fail(c, MTSGPU_EHIP, "hipEventCreate failed");
			}
			pool.push_back(ev);
		}
		if (!shading) {
			if (c->traceEvClass.size() <= used) c->traceEvClass.resize(used + 1);
			c->traceEvClass[used] = (unsigned char) kind;
		}
		ev = pool[used++];
		HIPCHK(c, hipEventRecord(ev.first, s));
	}
	launch();
	if (ev.second) HIPCHK(c, hipEventRecord(ev.second, s));
	HIPCHK(c, hipGetLastError());
	if (!shading && !c->q.dev_stats) c->stats.trace_launches++;
	return 0;
}

int readCounters(mtsgpu_ctx *c) {
	HIPCHK(c, hipMemcpyAsync(c->hostCounters, c->q.counters, kCounterSetBytes, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return 0;
}

// Closest-hit launch over queue[0..n) with the material sort, then the per-bin segment sizes (one blocking read of the
// counters).  A shard segment that overflowed (possible only with dynamically claimed batches, see ensurePaths) makes
// the launch run again with static dealing: tracing a ray twice writes the same hit twice.
// With the "lean_closest" knob the launch runs the kernel without the mailbox (trace.hip: LEAN, 8 waves per SIMD).  The rays on
// which two primitives tied come back as a list of path ids (q.redo) and go through the kernel with the mailbox, into the same
// bins and counters: every ray is binned once, by one of the two.  The redo deals its rays statically, but it appends to
// segments the first launch has filled already, so the proven bound of one static dealing (ensurePaths) does not cover the pair:
// the overflow retry runs the whole queue through the kernel with the mailbox, one static launch, for which it holds.
// Which launches (bits of the knob): 1 = the incoherent launches of at least plainBelow rays, 2 = the coherent first launch,
// 4 = the launches below plainBelow (kernels.h: trace_plan).  Counting frames keep the mailbox (the oracle counts with it).
bool leanClosest(const mtsgpu_ctx *c, uint32_t n, bool coherent) {
	const long knob = tuningOr(c, "lean_closest", kLeanClosestDefault);
	const uint32_t plainBelow = c->q.tune_plain_below ? c->q.tune_plain_below : 8u * (c->q.n_cus * kTraceBlocksPerCuMax) * kTraceBlock;
	return (knob & (coherent ? 2 : (n < plainBelow ? 4 : 1))) != 0 && !c->countTraversal;
}
// launches (may be NULL): how many launches the call made (1; 2 with a redo; more with the retry)
int traceAndBin(mtsgpu_ctx *c, const uint32_t *queue, uint32_t n, bool coherent, BinView *views, int *launches = nullptr) {
	hipStream_t s = c->stream;
	const bool testRetry = tuningOr(c, "test_retry", 0) != 0;      // exercises the retry (tests)
	const bool leanHere = leanClosest(c, n, coherent);
	for (int attempt = 0; attempt < 2; ++attempt) {
		if (attempt) HIPCHK(c, hipMemsetAsync(c->q.counters, 0, kCounterSetBytes, s));
		c->q.force_static = attempt ? 1u : 0u;
		const bool lean = leanHere && attempt == 0;
		if (launches) *launches += 1;
		int rc = timedLaunch(c, s, coherent ? kClosestFirst : kClosest, [&] {
			launch_trace(s, 0, c->countTraversal && attempt == 0, true, c->dsc, c->paths, c->q, queue, n, coherent, nullptr, lean); });
		if (!rc) rc = readCounters(c);
		const uint32_t nRedo = lean ? c->hostCounters[kRedoWord] : 0u;
		if (!rc && nRedo > n) rc = fail(c, MTSGPU_EHIP, "internal: redo list longer than the queue");
		if (!rc && nRedo) {
			// the list is not in queue order: its rays come from the path records.  Timed with the class of the launch it completes
			DPaths viaRecords = c->paths; viaRecords.rq_o = viaRecords.rq_d = nullptr;
			c->q.force_static = 1;
			if (launches) *launches += 1;
			rc = timedLaunch(c, s, coherent ? kClosestFirst : kClosest, [&] {
				launch_trace(s, 0, false, true, c->dsc, viaRecords, c->q, c->q.redo, nRedo, false); });
			if (!rc) rc = readCounters(c);
			c->raysRedone += nRedo;
		}
		c->q.force_static = 0;
		if (rc) return rc;
		bool overflow = attempt == 0 && testRetry;
		for (int b = 0; b < kNumBins; ++b) {
			uint32_t acc = 0;
			for (int k = 0; k < kBinShards; ++k) {
				views[b].prefix[k] = acc;
				const uint32_t cnt = c->hostCounters[(b * kBinShards + k) * kCounterStride];
				if (cnt > c->q.bin_seg_cap) overflow = true;
				acc += cnt;
			}
			views[b].prefix[kBinShards] = acc;
		}
		if (!overflow) {
			for (int b = 0; b < kNumBins; ++b) c->binEntries[b] += views[b].prefix[kBinShards];
			return 0;
		}
		c->stats.bin_overflow_retries++;
	}
	return fail(c, MTSGPU_EHIP, "internal: bin segment overflow with static dealing");
}

// The any-hit step of a bounce: the shadow queue, with a spill area of its own (a closest-hit launch may run beside it).
// n: the size of the queue, or, with `count`, a bound of the size the device keeps in that word.
int traceShadows(mtsgpu_ctx *c, hipStream_t s, uint32_t n, bool coherent, const uint32_t *count = nullptr) {
	DQueues q2 = c->q; q2.spill = c->spillShadow;
	return timedLaunch(c, s, kAnyHit, [&] { launch_trace(s, 1, c->countTraversal, false, c->dsc, c->paths, q2, q2.shadow, n, coherent, count); });
}

// What every shading launch of a frame takes: the stream, the frame's configuration and, from the context at the moment of
// the launch, the scene, the records, the queues and the three per-vertex families.
struct Shader {
	mtsgpu_ctx *c; hipStream_t s; DConfig cfg;
	bool fused;                            // the "shade_fused" knob: one kernel for the bins of kShadeAllBins (device-driven bounces)
	Shader(mtsgpu_ctx *c, hipStream_t s, const DConfig &cfg) : c(c), s(s), cfg(cfg), fused(tuningOr(c, "shade_fused", 1) != 0) {}
	// Bin b: over the view the host read back, or (viewsDev) over the one k_prep wrote, with a grid for `bound` paths.
	// ids: the queue to shade instead of the bin's (the ray queue, for the material-independent tail)
	void bin(int b, const BinView &view, const BinView *viewsDev = nullptr, uint32_t bound = 0, const uint32_t *ids = nullptr) const {
		launch_shade(s, b, c->dsc, c->paths, cfg, c->q, view, viewsDev, bound, ids, c->colors.d, c->tex.d, c->tan.d, c->tex.msk, c->snow.d, c->cloth.d, c->spots.d);
	}
	// the first nBins bins of a bounce whose sizes the host has read
	void bins(const BinView *views, int nBins = kNumBins) const { for (int b = 0; b < nBins; ++b) bin(b, views[b]); }
	// The bins of a bounce whose sizes only the device knows: the fused kernel where it applies, and one launch for every
	// other bin the scene can fill (the composite, which the fused kernel leaves out; every bin without it)
	void binsOnDevice(uint32_t bound) const {
		uint32_t each = c->binMask;
		// (a scene with a textured spot: every bin on its own, through the spot kernels; there is no fused form of them)
		if (cfg.dr_mode == 0 && fused && !c->spots.d.lum_texture) {
			// a scene with a snow or a cloth BRDF: the Lambertian's bin has kernels of its own (k_shade_snw, k_shade_clo) and is launched
			// like the composite's
			const uint32_t all = (c->snow.d.bsdf_snow || c->cloth.d.bsdf_weave) ? kShadeAllBins & ~1u : kShadeAllBins;
			launch_shade_all(s, c->dsc, c->paths, cfg, c->q, c->viewsDev, c->binMask & all, bound, c->colors.d, c->tex.d, c->tan.d, c->tex.msk);
			each &= ~all;
		}
		const BinView none{};
		for (int b = 0; b < kNumBins; ++b)
			if (each & (1u << b)) bin(b, none, c->viewsDev, bound);
	}
};

// the rounds of MIDirectIntegrator with more than one sample per strategy (runDirectRounds)
bool directRounds(const DConfig &cfg) { return cfg.integrator == 1 && (cfg.n_lum > 1 || cfg.n_bsdf > 1); }

// The direct-light terms of the shadow queue (DPaths::shq_nee), for a frame that runs with DQueues::nee_parked == 0; every
// other frame parks the terms in the path records and does without the 16 bytes per path
int ensureNeeQueue(mtsgpu_ctx *c) {
	const int rc = c->shqNee.ensure(c, c->pathCap);
	c->paths.shq_nee = c->shqNee;
	return rc;
}

// The queue flags of a frame, under the caller's RayQueuesOff: whether k_trace<closest> settles a miss (k_trace and k_shade
// agree on who does), and whether a direct-light term is parked in its path's record -- not in the rounds, which add their
// terms to Li one after the other, and not with the "nee_parked" knob at 0
int beginQueues(mtsgpu_ctx *c, const DConfig &cfg) {
	c->q.miss_settled = cfg.miss_settled ? 1u : 0u;
	c->q.nee_parked = !directRounds(cfg) && tuningOr(c, "nee_parked", 1) != 0 ? 1u : 0u;
	return c->q.nee_parked ? 0 : ensureNeeQueue(c);
}

// MIDirectIntegrator with more than one sample per strategy (direct.cpp:129-150,163-195): after the camera rays are
// traced and sorted by material, the two sampling loops run as rounds over those queues -- round j of the first loop
// shades with luminaire sample j and traces its shadow rays, round j of the second loop shades with BSDF sample j,
// traces the sampled rays and adds what they hit.  Li therefore receives its terms in the order of the reference
// (emission, luminaire samples 0.., BSDF samples 0..), which float addition needs for identical results.
int runDirectRounds(mtsgpu_ctx *c, const DConfig &cfg0, uint32_t nPaths, volatile const int *cancel) {
	hipStream_t s = c->stream;
	Shader shade(c, s, cfg0);
	RayQueuesOff rqOff{ c };
	int rc = beginQueues(c, cfg0); if (rc) return rc;
	HIPCHK(c, hipMemsetAsync(c->q.counters, 0, kCounterSetBytes, s));
	c->q.next = c->queueB;
	BinView views[kNumBins];
	rayQueues(c, c->queueA, nullptr);        // the camera rays; the rays of the sampling rounds are traced from the records
	rc = traceAndBin(c, c->queueA, nPaths, true, views); if (rc) return rc;
	rayQueues(c, nullptr, nullptr);
	c->stats.rays_closest += nPaths;
	auto shadeRound = [&](int mode, int index, int nBins) -> int {
		HIPCHK(c, hipMemsetAsync(c->q.counters, 0, kCounterSetBytes, s));     // the bins stay as they are; views[] holds their sizes
		shade.cfg.dr_mode = mode; shade.cfg.dr_index = index;
		const int rc = timedLaunch(c, s, kShading, [&] { shade.bins(views, nBins); });
		return rc ? rc : readCounters(c);
	};
	// direct.cpp:122-150
	for (int j = 0; j < std::max(1, c->nLumSamples); ++j) {
		if (cancel && *cancel) return fail(c, MTSGPU_ECANCEL, "render cancelled");
		rc = shadeRound(1, j, j == 0 ? kNumBins : kNumBsdfTypes); if (rc) return rc;      // the terminal bin once
		const uint32_t nShadow = c->hostCounters[kShadowWord];
		if (nShadow) {
			rc = traceShadows(c, s, nShadow, true); if (rc) return rc;
			c->stats.rays_shadow += nShadow;
		}
	}
	// direct.cpp:152-195
	for (int j = 0; j < std::max(1, c->nBsdfSamples); ++j) {
		if (cancel && *cancel) return fail(c, MTSGPU_ECANCEL, "render cancelled");
		rc = shadeRound(2, j, kNumBsdfTypes); if (rc) return rc;
		const uint32_t nNext = c->hostCounters[kNextWord];
		if (!nNext) continue;
		rc = timedLaunch(c, s, kClosest, [&] { launch_trace(s, 0, c->countTraversal, false, c->dsc, c->paths, c->q, c->queueB, nNext, false); });
		if (rc) return rc;
		c->stats.rays_closest += nNext;
		// what the sampled rays hit: the material-independent tail of the shading kernel over the ray queue
		BinView tail;
		tail.prefix[0] = 0;
		for (int k = 1; k <= kBinShards; ++k) tail.prefix[k] = nNext;
		shade.cfg.dr_mode = 3; shade.cfg.dr_index = j;
		rc = timedLaunch(c, s, kShading, [&] { shade.bin(kNumBsdfTypes, tail, nullptr, 0, c->queueB); }); if (rc) return rc;
	}
	return 0;
}

uint32_t *counterSet(mtsgpu_ctx *c, int bounce) { return c->counterSets + (size_t) (bounce & 1) * kNumCounters * kCounterStride; }

// Device-driven bounces: the whole chain of launches is enqueued without a single read-back of a queue size.
// k_trace reads its ray count from the counter the previous stage left in device memory, k_prep turns the shard
// counters of the closest-hit launch into the per-bin views k_shade reads, grids are sized for the upper bound
// (the number of paths of the pass) and surplus workgroups exit at once.  This is for frames whose launches are too
// short to hide a host round trip (a 1-spp frame: ~0.1-0.6 ms per launch, 2 round trips per bounce otherwise); large
// frames keep the host-sized grids of runBounces.  The host looks at a queue size once per chunk of bounces, to stop.
int runBouncesDevice(mtsgpu_ctx *c, const DConfig &cfg, uint32_t nPaths, volatile const int *cancel) {
	hipStream_t s1 = c->stream, s2 = c->stream2;
	HIPCHK(c, hipMemsetAsync(c->counterSets, 0, kCounterSets * kCounterSetBytes, s1));
	c->q.dev_stats = c->devStats;        // cleared by the caller (one frame may take several passes)
	c->devStatsUsed = true;
	// MIPathTracer traces at most maxDepth rays per path (path.cpp:87), the one-sample direct integrator two
	const int limit = cfg.integrator == 1 ? 2 : (cfg.max_depth > 0 ? cfg.max_depth : 0x7FFFFFFF);
	const int chunk = (int) tuningOr(c, "chunk", 8);
	uint32_t *cur = c->queueA, *nxt = c->queueB;
	uint32_t upper = nPaths;                   // what the host knows about the queue sizes
	bool shadowPending = false;
	int b = 0;
	// Every way out of this function -- cancel, a failed HIP call, the normal end -- leaves the context as the host-driven
	// loop expects it and the second stream joined: a shadow launch still running on it writes into the path records
	// (k_trace MODE 1: cancels, or a plain read-modify-write of Li), and the next frame's clear / generate kernels on
	// c->stream are not ordered against it otherwise (a GUI cancels and re-renders at once).
	struct Restore {
		mtsgpu_ctx *c; hipStream_t s2; const bool &pending;
		~Restore() {
			if (pending) (void) hipStreamSynchronize(s2);
			c->q.dev_stats = nullptr; c->q.counters = c->counterSets; c->q.spill = c->spillClosest;
		}
	} restore{ c, s2, shadowPending };
	RayQueuesOff rqOff{ c };
	{ int rc = beginQueues(c, cfg); if (rc) return rc; }
	const Shader shade(c, s1, cfg);
	while (b < limit && upper > 0) {
		if (cancel && *cancel) return fail(c, MTSGPU_ECANCEL, "render cancelled");
		const int end = (int) std::min<long long>((long long) b + chunk, limit);
		for (; b < end; ++b) {
			uint32_t *set = counterSet(c, b), *prev = counterSet(c, b - 1);
			c->q.counters = set; c->q.next = nxt; c->q.spill = c->spillClosest;
			rayQueues(c, cur, nxt);
			int rc = timedLaunch(c, s1, b == 0 ? kClosestFirst : kClosest, [&] {
				launch_trace(s1, 0, c->countTraversal, true, c->dsc, c->paths, c->q, cur, upper, b == 0,
				             b == 0 ? nullptr : prev + (size_t) kNextWord); });
			if (rc) return rc;
			// the shading of this bounce adds to Li after the shadow rays of the previous one have (path.cpp:124 before :80)
			if (shadowPending) HIPCHK(c, hipStreamWaitEvent(s1, c->evShadow[(b - 1) & 1], 0));
			rc = timedLaunch(c, s1, kShading, [&] {
				launch_prep(s1, set, prev, c->viewsDev, c->q.bin_seg_cap, c->devStats);
				shade.binsOnDevice(upper); });
			if (rc) return rc;
			HIPCHK(c, hipEventRecord(c->evShade[b & 1], s1));
			// shadow rays of this bounce on the second stream, next to the closest-hit launch of the next bounce
			HIPCHK(c, hipStreamWaitEvent(s2, c->evShade[b & 1], 0));
			rc = traceShadows(c, s2, upper, b == 0, set + (size_t) kShadowWord); if (rc) return rc;
			HIPCHK(c, hipEventRecord(c->evShadow[b & 1], s2));
			shadowPending = true;
			std::swap(cur, nxt);
		}
		// how many paths are left: the one read-back of the chunk
		uint32_t *hostNext = &c->hostCounters[kHostNextWord];
		HIPCHK(c, hipMemcpyAsync(hostNext, counterSet(c, b - 1) + (size_t) kNextWord, sizeof(uint32_t), hipMemcpyDeviceToHost, s1));
		HIPCHK(c, hipEventRecord(c->evCount, s1));
		HIPCHK(c, hipEventSynchronize(c->evCount));
		upper = *hostNext;
	}
	if (shadowPending) {
		HIPCHK(c, hipStreamWaitEvent(s1, c->evShadow[(b - 1) & 1], 0));      // the film kernels that follow wait on the device
		shadowPending = false;                                               // ... so the guard need not block the host
	}
	return 0;
}

// the statistics a device-driven frame kept on the device (the host-driven loop counts on the host)
int collectDeviceStats(mtsgpu_ctx *c) {
	if (!c->devStatsUsed) return 0;
	c->devStatsUsed = false;
	unsigned long long h[kNumDevStats];
	HIPCHK(c, hipMemcpy(h, c->devStats, sizeof(h), hipMemcpyDeviceToHost));
	c->stats.rays_closest += h[kStatClosest]; c->stats.rays_shadow += h[kStatShadow]; c->stats.trace_launches += h[kStatLaunches];
	for (int b = 0; b < kNumBins; ++b) c->binEntries[b] += h[kStatBin0 + b];
	if (h[kStatOverflow]) return fail(c, MTSGPU_EHIP, "internal: bin segment overflow in a device-driven frame");
	return 0;
}

// MTSGPU_DEBUG: what the launches of a host-driven bounce took, once they are done (tools/bounce_times.py); nClosestLaunches:
// the closest-hit launches of the bounce (the redo launch and a retry are part of its closest-hit time)
int printBounce(mtsgpu_ctx *c, uint32_t nClosest, uint32_t nShadow, int nClosestLaunches) {
	HIPCHK(c, hipStreamSynchronize(c->stream));
	float a = 0, b = 0, c2 = 0;
	if (c->timeKernels) {
		const size_t ti = c->traceEvUsed - (nShadow ? 2 : 1);
		for (int k = 0; k < nClosestLaunches && (size_t) k <= ti; ++k) {
			float ms = 0;
			(void) hipEventElapsedTime(&ms, c->traceEvents[ti - k].first, c->traceEvents[ti - k].second);
			a += ms;
		}
		(void) hipEventElapsedTime(&b, c->shadeEvents[c->shadeEvUsed - 1].first, c->shadeEvents[c->shadeEvUsed - 1].second);
		if (nShadow) (void) hipEventElapsedTime(&c2, c->traceEvents[ti + 1].first, c->traceEvents[ti + 1].second);
	}
	fprintf(stderr, "bounce: closest %u rays %.3f ms (%.2f Grays/s) | shade %.3f ms | shadow %u rays %.3f ms (%.2f Grays/s)\n",
	        nClosest, a, a > 0 ? nClosest / a / 1e6 : 0.0, b, nShadow, c2, c2 > 0 ? nShadow / c2 / 1e6 : 0.0);
	return 0;
}

// One wavefront pass: all bounces of the paths already generated into queueA[0..nPaths)
int runBounces(mtsgpu_ctx *c, const DConfig &cfg, uint32_t nPaths, volatile const int *cancel) {
	c->q.counters = c->counterSets; c->q.spill = c->spillClosest; c->q.dev_stats = nullptr;
	if (directRounds(cfg))
		return runDirectRounds(c, cfg, nPaths, cancel);
	{
		// frames of few paths are chains of launches too short to hide a host round trip
		const long sf = tuningOr(c, "sync_free", -1);
		if (sf == 1 || (sf < 0 && nPaths <= (8u << 20)))
			return runBouncesDevice(c, cfg, nPaths, cancel);
	}
	// Host-driven bounces, all on c->stream: stream order puts the shadow rays of bounce b before the shading of bounce
	// b + 1, which adds to Li after them (path.cpp:124 before :80)
	uint32_t nQ = nPaths;
	uint32_t *cur = c->queueA, *nxt = c->queueB;
	bool first = true;       // camera rays and their shadow rays are coherent: plain 64-ray batches win there
	hipStream_t s = c->stream;
	RayQueuesOff rqOff{ c };
	{ int rc = beginQueues(c, cfg); if (rc) return rc; }
	const Shader shade(c, s, cfg);
	for (int b = 0; nQ > 0; ++b) {
		if (cancel && *cancel)
			return fail(c, MTSGPU_ECANCEL, "render cancelled");
		// the counter set of this bounce; its last users (bounce b - 2) are done: the shading of bounce b - 1 waited for them
		c->q.counters = counterSet(c, b); c->q.spill = c->spillClosest;
		HIPCHK(c, hipMemsetAsync(c->q.counters, 0, kCounterSetBytes, s));
		c->q.next = nxt;
		rayQueues(c, cur, nxt);
		// closest hit + material sort
		BinView views[kNumBins];
		int closestLaunches = 0;
		int rc = traceAndBin(c, cur, nQ, first, views, &closestLaunches); if (rc) return rc;
		c->stats.rays_closest += nQ;
		// shade, one launch per BSDF type
		rc = timedLaunch(c, s, kShading, [&] { shade.bins(views); }); if (rc) return rc;
		rc = readCounters(c); if (rc) return rc;
		const uint32_t nNext = c->hostCounters[kNextWord], nShadow = c->hostCounters[kShadowWord];
		// shadow rays of this bounce (they cancel the parked direct-light terms of the occluded ones -- or, unparked, add the others' --
		// before the next bounce reads the records); the shading above has completed
		if (nShadow) {
			c->lastPass.shadowMax = std::max(c->lastPass.shadowMax, nShadow);
			rc = traceShadows(c, s, nShadow, first); if (rc) return rc;
			c->stats.rays_shadow += nShadow;
		}
		if (c->debug) { rc = printBounce(c, nQ, nShadow, closestLaunches); if (rc) return rc; }
		std::swap(cur, nxt);
		nQ = nNext;
		first = false;
	}
	c->q.counters = c->counterSets;
	return 0;
}

void collectTimings(mtsgpu_ctx *c) {
	float ms;
	// traversal launches may overlap (two streams): their summed durations and the length of the union of their intervals
	std::vector<std::pair<float, float>> iv;
	for (size_t i = 0; i < c->traceEvUsed; ++i) {
		if (hipEventElapsedTime(&ms, c->traceEvents[i].first, c->traceEvents[i].second) != hipSuccess) continue;
		c->stats.trace_ms += ms;
		const int cls = i < c->traceEvClass.size() ? c->traceEvClass[i] : 0;
		if (cls == 1) c->stats.trace_first_ms += ms;
		else if (cls == 2) c->stats.trace_shadow_ms += ms;
		float t0 = 0;
		if (i == 0 || hipEventElapsedTime(&t0, c->traceEvents[0].first, c->traceEvents[i].first) == hipSuccess)
			iv.emplace_back(t0, t0 + ms);
	}
	std::sort(iv.begin(), iv.end());
	float curA = 0, curB = -1;
	for (auto &p : iv) {
		if (curB < curA) { curA = p.first; curB = p.second; }
		else if (p.first <= curB) curB = std::max(curB, p.second);
		else { c->stats.trace_union_ms += curB - curA; curA = p.first; curB = p.second; }
	}
	if (curB >= curA) c->stats.trace_union_ms += curB - curA;
	for (size_t i = 0; i < c->shadeEvUsed; ++i)
		if (hipEventElapsedTime(&ms, c->shadeEvents[i].first, c->shadeEvents[i].second) == hipSuccess) c->stats.shade_ms += ms;
	c->traceEvUsed = c->shadeEvUsed = 0;
}

int fetchTraceCounts(mtsgpu_ctx *c) {
	unsigned long long h[kNumTraceCounts];
	HIPCHK(c, hipMemcpy(h, c->q.trace_counts, sizeof(h), hipMemcpyDeviceToHost));
	c->stats.n_inner = h[0]; c->stats.n_leaf = h[1]; c->stats.n_idx = h[2]; c->stats.n_tri_tested = h[3];
	c->stats.req_pair_global = h[kCntPairGlobal]; c->stats.req_pair_lds = h[kCntPairLds];
	c->stats.req_node_global = h[kCntNodeGlobal]; c->stats.req_node_lds = h[kCntNodeLds];
	c->stats.req_tail = h[kCntTail]; c->stats.req_spill = h[kCntSpill]; c->stats.req_head = h[kCntHead];
	if (c->debug)     // candidates whose tail was fetched with a plane distance outside the visited leaf's own interval
		fprintf(stderr, "[mtsgpu] record tails: %llu requests, %llu candidates of which %llu (%.3f) lie outside the leaf's interval\n",
		        h[kCntTail], h[kCntTail] / 2, h[15], h[kCntTail] ? 2.0 * h[15] / h[kCntTail] : 0.0);
	if (c->debug)     // SIMD utilisation of the traversal loops: lane steps / lane slots issued
		fprintf(stderr, "[mtsgpu] lanes: inner %llu/%llu (%.3f)  leaf-prims %llu/%llu (%.3f)  outer %llu/%llu (%.3f)  batch slots %llu\n",
		        h[0], h[4], h[4] ? (double) h[0] / h[4] : 0.0, h[2], h[5], h[5] ? (double) h[2] / h[5] : 0.0,
		        h[1], h[6], h[6] ? (double) h[1] / h[6] : 0.0, h[7]);
	return 0;
}

// The 8-float rows of mtsgpu_li_samples and mtsgpu_pass_samples for the n path records from `first` on: Li with the parked
// direct-light term settled, alpha, the sample position, the depth and, withKey, the record's pixel key (0 otherwise).
int readSampleRows(mtsgpu_ctx *c, size_t first, uint32_t n, bool withKey, float *out) {
	std::vector<float> Li(4 * (size_t) n), thr(4 * (size_t) n), spos(4 * (size_t) n), parked(4 * (size_t) n), misc(withKey ? 4 * (size_t) n : 0);
	const size_t pitch = kPathSlots * sizeof(float4);
	const float4 *rec = c->paths.base + first * kPathSlots;
	HIPCHK(c, hipMemcpy2DAsync(Li.data(), 16, rec + 4, pitch, 16, n, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpy2DAsync(parked.data(), 16, rec + 2, pitch, 16, n, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpy2DAsync(thr.data(), 16, rec + 3, pitch, 16, n, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpy2DAsync(spos.data(), 16, rec + 7, pitch, 16, n, hipMemcpyDeviceToHost, c->stream));
	if (withKey) HIPCHK(c, hipMemcpy2DAsync(misc.data(), 16, rec + 6, pitch, 16, n, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	for (size_t i = 0; i < n; ++i) {
		uint32_t flags; int depth;
		std::memcpy(&flags, &Li[4 * i + 3], 4); std::memcpy(&depth, &thr[4 * i + 3], 4);
		float *o = out + 8 * i;
		// a direct-light term still parked in the record of a path that has ended (DQueues::nee_parked), as the film kernels settle it
		const float4 L = settled_Li(make_float4(Li[4 * i], Li[4 * i + 1], Li[4 * i + 2], 0.0f),
		                            make_float4(parked[4 * i], parked[4 * i + 1], parked[4 * i + 2], parked[4 * i + 3]));
		o[0] = L.x; o[1] = L.y; o[2] = L.z; o[3] = (flags & F_ALPHA) ? 1.0f : 0.0f;
		o[4] = spos[4 * i]; o[5] = spos[4 * i + 1]; o[6] = (float) depth; o[7] = 0.0f;
		if (withKey) std::memcpy(&o[7], &misc[4 * i + 3], 4);           // the pixel key, as a bit pattern
	}
	return 0;
}

// The 14-float rows of mtsgpu_camera_rays for the n path records from `first` on, as k_generate left them: ray_o (o, mint),
// ray_d (d, maxt), the sample position, the sampler's counters from the flags word, the pixel key and the sample index.
int readCameraRows(mtsgpu_ctx *c, size_t first, uint32_t n, float *out) {
	std::vector<float> ro(4 * (size_t) n), rd(4 * (size_t) n), Li(4 * (size_t) n), misc(4 * (size_t) n), spos(4 * (size_t) n);
	const size_t pitch = kPathSlots * sizeof(float4);
	const float4 *rec = c->paths.base + first * kPathSlots;
	HIPCHK(c, hipMemcpy2DAsync(ro.data(), 16, rec + 0, pitch, 16, n, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpy2DAsync(rd.data(), 16, rec + 1, pitch, 16, n, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpy2DAsync(Li.data(), 16, rec + 4, pitch, 16, n, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpy2DAsync(misc.data(), 16, rec + 6, pitch, 16, n, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipMemcpy2DAsync(spos.data(), 16, rec + 7, pitch, 16, n, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	for (size_t i = 0; i < n; ++i) {
		uint32_t flags;
		std::memcpy(&flags, &Li[4 * i + 3], 4);
		float *o = out + 14 * i;
		std::memcpy(o, &ro[4 * i], 16); std::memcpy(o + 4, &rd[4 * i], 16);
		o[8] = spos[4 * i]; o[9] = spos[4 * i + 1];
		const uint32_t words[4] = { (flags >> F_D1_SHIFT) & 0xFFu, (flags >> F_D2_SHIFT) & 0xFFu, 0u, 0u };
		std::memcpy(o + 10, words, 8);
		std::memcpy(o + 12, &misc[4 * i + 3], 4);             // the pixel key
		std::memcpy(o + 13, &misc[4 * i + 2], 4);             // the sample index
	}
	return 0;
}

// A frame begins: statistics (bins: those of mtsgpu_bin_entries too), the timing events in use and the debug switch (read
// here, not per bounce)
void beginFrame(mtsgpu_ctx *c, bool bins = true) {
	std::memset(&c->stats, 0, sizeof(c->stats));
	if (bins) std::memset(c->binEntries, 0, sizeof(c->binEntries));
	c->raysRedone = 0;
	c->traceEvUsed = c->shadeEvUsed = 0;
	c->debug = getenv("MTSGPU_DEBUG") != nullptr;
}

// The work units of a frame: ImageBlock tiles (imageproc.cpp:43-78) owned by this context, tile (tx, ty) -> part
// morton(tx, ty) % n_parts, as pixel keys in tile order (renderPixels, and pixelList on the device) and tile rectangles
// (renderTiles).  They depend on the film geometry and the tile sharding only (renderKey) and are kept from frame to frame;
// the cached list holds while renderListValid (the hooks that borrow pixelList clear it) and pixelList still has its size.
// *offOut, *keyWOut: the grid the keys index -- the full film (the crop window only moves the rendered rectangle in it),
// grown by the filter border with Film::hasHighQualityEdges (renderproc.cpp:146-153)
int ensureWorkUnits(mtsgpu_ctx *c, int *offOut, int *keyWOut) {
	const int W = c->cam.width, H = c->cam.height, bs = c->blockSize, off = c->hqEdges ? -c->filtBorder : 0;
	const int RW = W - 2 * off, RH = H - 2 * off;
	const int tx = (RW + bs - 1) / bs, ty = (RH + bs - 1) / bs;
	const int cx = c->cam.crop_offset_x, cy = c->cam.crop_offset_y;
	const int keyW = filmWidth(c) - 2 * off;
	if ((uint64_t) keyW * (uint64_t) (filmHeight(c) - 2 * off) > 0xFFFFFFFFull) return fail(c, MTSGPU_EINVAL, "film too large");
	*offOut = off; *keyWOut = keyW;
	std::vector<uint32_t> &pixels = c->renderPixels;
	std::vector<TileMeta> &tiles = c->renderTiles;
	const std::vector<long long> key = { W, H, bs, off, cx, cy, keyW, c->nParts, c->part };
	if (c->renderListValid && key == c->renderKey && c->pixelList && c->pixelList.cap >= pixels.size()) return 0;
	pixels.clear(); tiles.clear();
	for (int t = 0; t < tx * ty; ++t) {
		if (tileMorton((uint32_t) (t % tx), (uint32_t) (t / tx)) % (uint32_t) c->nParts != (uint32_t) c->part) continue;
		const int x0 = off + (t % tx) * bs, y0 = off + (t / tx) * bs;            // inside the crop window
		TileMeta tm{};
		tm.x0 = x0 + cx; tm.y0 = y0 + cy; tm.w = std::min(bs, off + RW - x0); tm.h = std::min(bs, off + RH - y0);
		tm.slot_base = (uint32_t) pixels.size(); tm.block_index = (uint32_t) tiles.size();
		tm.colour = (uint32_t) (((t % tx) & 1) + 2 * ((t / tx) & 1));
		tiles.push_back(tm);
		for (int y = tm.y0; y < tm.y0 + tm.h; ++y)
			for (int x = tm.x0; x < tm.x0 + tm.w; ++x)
				pixels.push_back((uint32_t) (y - off) * (uint32_t) keyW + (uint32_t) (x - off));
	}
	c->renderKey = key; c->renderListValid = false;
	if (pixels.empty()) return 0;
	int rc = c->pixelList.ensure(c, pixels.size()); if (rc) return rc;
	HIPCHK(c, hipMemcpyAsync(c->pixelList, pixels.data(), pixels.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	// valid only once the copy has landed: a frame that leaves early (cancel, an error) and a caller that then switches
	// streams (mtsgpu_set_stream) must not find a list that is marked valid but not ordered before its next use
	HIPCHK(c, hipStreamSynchronize(c->stream));
	c->renderListValid = true;
	return 0;
}

// the sampler tables and sample arrays of nSlots sampler slots carrying nPaths paths (a pass, or the explicit samples of a hook)
int ensureSamplerBuffers(mtsgpu_ctx *c, size_t nSlots, size_t nPaths) {
	if (samplerHasTables(c)) {
		const uint32_t spp = effectiveSpp(c);
		int rc = c->ldScr.ensure(c, nSlots * 3 * c->ldDepth); if (rc) return rc;
		rc = c->ldPerm.ensure(c, nSlots * 2 * c->ldDepth * spp); if (rc) return rc;
		rc = ensureTableWork(c, nSlots, spp); if (rc) return rc;
	}
	return ensureSampleArrays(c, nSlots, nPaths);
}

// The buffers of a pass, and in *slotsPerPass how many sampler slots (pixels) one takes: the path records and queues, the
// sampler's tables and, with a filter wider than a pixel, the tile records and blocks of the whole frame
int ensurePassBuffers(mtsgpu_ctx *c, size_t *slotsPerPass) {
	const int bs = c->blockSize;
	const uint32_t spp = effectiveSpp(c);
	const bool wideFilter = c->filtBorder > 0;
	if (wideFilter && 2 * c->filtBorder > bs) return fail(c, MTSGPU_EINVAL, "filter border %d too wide for block size %d", c->filtBorder, bs);
	const uint64_t maxPaths = c->maxPaths ? c->maxPaths : defaultMaxPaths(c);
	size_t slots = (size_t) std::max<uint64_t>(1, std::min<uint64_t>(c->renderPixels.size(), maxPaths / spp));
	if (wideFilter) slots = std::max<size_t>(slots, (size_t) bs * bs);     // passes hold whole tiles
	if ((uint64_t) slots * spp > 0x7FFFFFFFull) return fail(c, MTSGPU_EINVAL, "pass too large");
	int rc = ensurePaths(c, slots * spp); if (rc) return rc;
	rc = ensureSamplerBuffers(c, slots, slots * spp); if (rc) return rc;
	if (wideFilter) {
		const size_t fullBlock = (size_t) (bs + 2 * c->filtBorder) * (bs + 2 * c->filtBorder) * 5;
		rc = c->tileMeta.ensure(c, c->renderTiles.size()); if (rc) return rc;
		rc = c->blocks.ensure(c, c->renderTiles.size() * fullBlock); if (rc) return rc;
	}
	*slotsPerPass = slots;
	return 0;
}

// The explicit samples of a hook on the device, one path each: n (x, y, sample index) triples and their pixel keys, which take
// the place of the frame's work units (the cached list and the last pass are gone), and the buffers their paths need
int putExplicitSamples(mtsgpu_ctx *c, const uint32_t *samples, const uint32_t *keys, uint32_t n) {
	int rc = ensurePaths(c, n); if (rc) return rc;
	rc = c->explicitSamples.ensure(c, 3 * (size_t) n); if (rc) return rc;
	c->renderListValid = false; c->lastPass.valid = false;
	rc = c->pixelList.ensure(c, n); if (rc) return rc;
	HIPCHK(c, hipMemcpyAsync(c->explicitSamples, samples, 3 * (size_t) n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	HIPCHK(c, hipMemcpyAsync(c->pixelList, keys, (size_t) n * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
	return ensureSamplerBuffers(c, n, n);
}

// sampler state and camera rays of nSlots slots from pixelList + base on, into queueA
int generatePaths(mtsgpu_ctx *c, const DConfig &cfg, size_t base, uint32_t nSlots, const uint32_t *explicitSamples, uint32_t nPaths) {
	if (samplerHasTables(c)) {
		launch_ld_tables(c->stream, cfg, c->pixelList + base, nSlots, c->ldScr, c->ldPerm, c->ldState, c->ldScratch);
		launch_sample_arrays(c->stream, cfg, nSlots, c->ldState);
	}
	rayQueues(c, nullptr, c->queueA);
	launch_generate(c->stream, c->dsc, c->paths, cfg, c->pixelList + base, nSlots, explicitSamples, nPaths, c->queueA);
	rayQueues(c, nullptr, nullptr);
	HIPCHK(c, hipGetLastError());
	return 0;
}

// The passes of a frame over the work units: generate, bounce, add to the film (or, with a filter wider than a pixel, to the
// tiles' blocks, which join the film when all passes are done).  Leaves total_ms and path_length_sum in the statistics.
int renderPasses(mtsgpu_ctx *c, const DConfig &cfg, size_t slotsPerPass, volatile const int *cancel) {
	const std::vector<uint32_t> &pixels = c->renderPixels;
	std::vector<TileMeta> &tiles = c->renderTiles;
	const int bs = c->blockSize;
	const uint32_t spp = cfg.spp;
	const bool wideFilter = c->filtBorder > 0;
	// frame timing events, released on every way out of this function
	EventPair frameEv;
	HIPCHK(c, hipEventCreate(&frameEv.a)); HIPCHK(c, hipEventCreate(&frameEv.b));
	HIPCHK(c, hipEventRecord(frameEv.a, c->stream));
	size_t tileCursor = 0;
	for (size_t base = 0; base < pixels.size();) {
		uint32_t nSlots;
		const size_t tileFirst = tileCursor;
		if (wideFilter) {
			// whole tiles only: a block gathers from all samples of its tile
			size_t acc = 0;
			while (tileCursor < tiles.size() && (acc == 0 || acc + (size_t) tiles[tileCursor].w * tiles[tileCursor].h <= slotsPerPass)) {
				// slot inside this pass.  The cached tile list is updated in place: every tile passes through this line in
				// every frame before its record is uploaded below, so nothing of an earlier frame's passes survives
				tiles[tileCursor].slot_base = (uint32_t) acc;
				acc += (size_t) tiles[tileCursor].w * tiles[tileCursor].h;
				++tileCursor;
			}
			nSlots = (uint32_t) acc;
		} else {
			nSlots = (uint32_t) std::min(slotsPerPass, pixels.size() - base);
		}
		const uint32_t nPaths = nSlots * spp;
		int rc = generatePaths(c, cfg, base, nSlots, nullptr, nPaths); if (rc) return rc;
		c->lastPass.valid = true; c->lastPass.cfg = cfg; c->lastPass.base = base;
		c->lastPass.nSlots = nSlots; c->lastPass.nPaths = nPaths; c->lastPass.shadowMax = 0;
		rc = runBounces(c, cfg, nPaths, cancel); if (rc) return rc;
		if (wideFilter) {
			const uint32_t nT = (uint32_t) (tileCursor - tileFirst);
			HIPCHK(c, hipMemcpyAsync(c->tileMeta + tileFirst, tiles.data() + tileFirst, nT * sizeof(TileMeta), hipMemcpyHostToDevice, c->stream));
			launch_splat_blocks(c->stream, c->paths, cfg, c->tileMeta + tileFirst, nT, spp, bs, c->blocks);
			launch_path_lengths(c->stream, c->paths, nPaths, c->pathLen);
		} else {
			launch_accumulate(c->stream, c->paths, cfg, nSlots, spp, c->film, c->pathLen);
			if (c->filmStats) {
				const long form = tuningOr(c, "stats_wave", -1);
				const bool wave = form < 0 ? variance_wave_rule(nSlots, spp) : form != 0;
				launch_variance(c->stream, wave, c->paths, cfg, c->pixelList + base, nSlots, spp, c->statVar, c->statN);
				c->statsForm = wave ? 1 : 0;
			}
		}
		HIPCHK(c, hipGetLastError());
		c->stats.camera_samples += nPaths;
		base += nSlots;
	}
	if (wideFilter)
		for (uint32_t colour = 0; colour < 4; ++colour)
			launch_add_blocks(c->stream, cfg, c->tileMeta, (uint32_t) tiles.size(), colour, bs, c->blocks, c->film);
	HIPCHK(c, hipGetLastError());
	HIPCHK(c, hipEventRecord(frameEv.b, c->stream));
	HIPCHK(c, hipMemcpyAsync(&c->hostCounters[kHostPathLenWord], c->pathLen, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	std::memcpy(&c->stats.path_length_sum, &c->hostCounters[kHostPathLenWord], sizeof(uint64_t));
	float ms = 0;
	HIPCHK(c, hipEventElapsedTime(&ms, frameEv.a, frameEv.b));
	c->stats.total_ms = ms;
	return 0;
}

} // namespace

extern "C" {

int mtsgpu_render(mtsgpu_ctx *c, volatile const int *cancel) {
	int rc = checkReady(c); if (rc) return rc;
	// refused before anything is touched: the context stays as it was
	if (c->filmStats && c->filtBorder > 0)
		return fail(c, MTSGPU_EINVAL, "film statistics need the box filter: the reference collects them only with a reconstruction "
		            "filter no wider than a pixel (renderjob.cpp:96-99, mfilm.cpp:145); this filter has a border of %d", c->filtBorder);
	rc = ensureFilm(c); if (rc) return rc;
	c->statsForm = -1;
	if (c->filmStats) { rc = ensureFilmStats(c); if (rc) return rc; }      // before defaultMaxPaths() asks for the free memory
	int off = 0, keyW = 0;
	rc = ensureWorkUnits(c, &off, &keyW); if (rc) return rc;
	beginFrame(c);
	if (c->renderPixels.empty()) return 0;
	size_t slotsPerPass = 0;
	rc = ensurePassBuffers(c, &slotsPerPass); if (rc) return rc;
	if (c->countTraversal) HIPCHK(c, hipMemsetAsync(c->q.trace_counts, 0, kNumTraceCounts * sizeof(unsigned long long), c->stream));
	DConfig cfg = makeConfig(c, false);
	cfg.pix_w = keyW; cfg.pix_off = off;
	HIPCHK(c, hipMemsetAsync(c->pathLen, 0, sizeof(unsigned long long), c->stream));
	HIPCHK(c, hipMemsetAsync(c->devStats, 0, kNumDevStats * sizeof(unsigned long long), c->stream));
	c->devStatsUsed = false;
	rc = renderPasses(c, cfg, slotsPerPass, cancel); if (rc) return rc;
	collectTimings(c);
	rc = collectDeviceStats(c); if (rc) return rc;
	if (c->countTraversal) { rc = fetchTraceCounts(c); if (rc) return rc; }
	return 0;
}

int mtsgpu_trace_rays(mtsgpu_ctx *c, const float *rays, uint32_t n, int shadow, uint32_t *hits) {
	if (!c) return fail(nullptr, MTSGPU_EINVAL, "null context");
	if (!c->haveScene) return fail(c, MTSGPU_ESTATE, "no scene uploaded");
	if (!rays || !hits) return fail(c, MTSGPU_EINVAL, "null argument");
	HIPCHK(c, hipSetDevice(c->device));
	beginFrame(c, false);
	if (n == 0) return 0;
	c->lastPass.valid = false;
	int rc = ensurePaths(c, n); if (rc) return rc;
	{
		// host rays -> ray_o / ray_d slots of the path records
		std::vector<float> od(8 * (size_t) n);
		std::memcpy(od.data(), rays, od.size() * sizeof(float));
		HIPCHK(c, hipMemcpy2DAsync(c->paths.base, kPathSlots * sizeof(float4), od.data(), 32, 32, n, hipMemcpyHostToDevice, c->stream));
		HIPCHK(c, hipStreamSynchronize(c->stream));
	}
	launch_iota(c->stream, c->queueA, n);
	if (c->countTraversal) HIPCHK(c, hipMemsetAsync(c->q.trace_counts, 0, kNumTraceCounts * sizeof(unsigned long long), c->stream));
	HIPCHK(c, hipMemsetAsync(c->q.counters, 0, kCounterSetBytes, c->stream));     // dynamic batch head
	if (!shadow && leanClosest(c, n, false)) {
		// As the bounces trace an incoherent queue of this size: through the material sort (the kernel without the mailbox, the
		// redo, the retry), every ray binned -- a miss in the terminal bin -- and the hits moved from the bins to the records
		const uint32_t settled = c->q.miss_settled;
		uint64_t bins[kNumBins];
		std::memcpy(bins, c->binEntries, sizeof(bins));
		c->q.miss_settled = 0;
		rayQueues(c, nullptr, nullptr);
		BinView views[kNumBins];
		rc = traceAndBin(c, c->queueA, n, false, views);
		c->q.miss_settled = settled;
		std::memcpy(c->binEntries, bins, sizeof(bins));      // a frame's statistic
		if (rc) return rc;
		launch_unbin_hits(c->stream, c->paths, c->q, n);
		HIPCHK(c, hipGetLastError());
	} else {
		rc = timedLaunch(c, c->stream, shadow ? kAnyHit : kClosest, [&] {
			launch_trace(c->stream, shadow ? 2 : 0, c->countTraversal, false, c->dsc, c->paths, c->q, c->queueA, n, false); });
		if (rc) return rc;
	}
	HIPCHK(c, hipMemcpy2DAsync(hits, 16, c->paths.base + 2, kPathSlots * sizeof(float4), 16, n, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (shadow) c->stats.rays_shadow = n; else c->stats.rays_closest = n;
	collectTimings(c);
	if (c->countTraversal) { rc = fetchTraceCounts(c); if (rc) return rc; }
	return 0;
}

int mtsgpu_li_samples(mtsgpu_ctx *c, const uint32_t *pix_samples, uint32_t n, float *out) {
	int rc = checkReady(c); if (rc) return rc;
	if (!pix_samples || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	beginFrame(c);
	if (n == 0) return 0;
	const uint32_t spp = effectiveSpp(c);
	std::vector<uint32_t> keys(n);
	for (uint32_t i = 0; i < n; ++i) {
		const uint32_t x = pix_samples[3 * (size_t) i], y = pix_samples[3 * (size_t) i + 1], j = pix_samples[3 * (size_t) i + 2];
		if (x >= (uint32_t) c->cam.width || y >= (uint32_t) c->cam.height || j >= spp)
			return fail(c, MTSGPU_EINVAL, "sample %u: pixel or sample index out of range", i);
		keys[i] = (y + (uint32_t) c->cam.crop_offset_y) * (uint32_t) filmWidth(c) + x + (uint32_t) c->cam.crop_offset_x;
	}
	rc = putExplicitSamples(c, pix_samples, keys.data(), n); if (rc) return rc;
	const DConfig cfg = makeConfig(c, true);
	rc = generatePaths(c, cfg, 0, n, c->explicitSamples, n); if (rc) return rc;
	HIPCHK(c, hipMemsetAsync(c->devStats, 0, kNumDevStats * sizeof(unsigned long long), c->stream));
	c->devStatsUsed = false;
	rc = runBounces(c, cfg, n, nullptr); if (rc) return rc;
	rc = readSampleRows(c, 0, n, false, out); if (rc) return rc;
	collectTimings(c);
	return collectDeviceStats(c);
}

// The records the film kernels of the last pass consumed (include/mtsgpu.h): the film kernels only read them, so they
// are still in place after mtsgpu_render.  Layout of mtsgpu_li_samples, plus the record's pixel key.
int mtsgpu_pass_samples(mtsgpu_ctx *c, uint32_t first, uint32_t n, float *out) {
	int rc = checkReady(c); if (rc) return rc;
	const mtsgpu_ctx::LastPass &lp = c->lastPass;
	if (!lp.valid) return fail(c, MTSGPU_ESTATE, "no pass to read: render first (setters, mtsgpu_li_samples and mtsgpu_trace_rays invalidate the last pass)");
	if ((uint64_t) first + n > lp.nPaths || (uint64_t) first + n > c->pathCap)
		return fail(c, MTSGPU_EINVAL, "records %u .. %llu lie past the end of the last pass (%u records)", first, (unsigned long long) first + n, lp.nPaths);
	if (n == 0) return 0;
	if (!out) return fail(c, MTSGPU_EINVAL, "null output");
	return readSampleRows(c, first, n, true, out);
}

// The camera records as k_generate leaves them (include/mtsgpu.h): one launch of the product's kernel and no bounce, for
// explicit samples (sampler state built as mtsgpu_li_samples builds it, keys in the grid mtsgpu_render uses) or for the pass
// rendered last once more (as mtsgpu_replay_roof kind 1 regenerates it).
int mtsgpu_camera_rays(mtsgpu_ctx *c, const int32_t *pix_samples, uint32_t first, uint32_t n, float *out) {
	int rc = checkReady(c); if (rc) return rc;
	if (n > (1u << 24)) return fail(c, MTSGPU_EINVAL, "at most 2^24 camera records per call");
	if (!pix_samples) {
		const mtsgpu_ctx::LastPass lp = c->lastPass;
		if (!lp.valid) return fail(c, MTSGPU_ESTATE, "no pass to regenerate: render first (setters, mtsgpu_li_samples, mtsgpu_trace_rays and this call invalidate the last pass)");
		if ((uint64_t) first + n > lp.nPaths || lp.nPaths > c->pathCap)
			return fail(c, MTSGPU_EINVAL, "records %u .. %llu lie past the end of the last pass (%u records)", first, (unsigned long long) first + n, lp.nPaths);
		if (n == 0) return 0;
		if (!out) return fail(c, MTSGPU_EINVAL, "null output");
		rayQueues(c, nullptr, nullptr);
		// its sampler tables and its part of the pixel list are still in place
		launch_generate(c->stream, c->dsc, c->paths, lp.cfg, c->pixelList + lp.base, lp.nSlots, nullptr, lp.nPaths, c->queueA);
		HIPCHK(c, hipGetLastError());
		c->lastPass.valid = false;             // the path records no longer hold that pass
		return readCameraRows(c, first, n, out);
	}
	if (first != 0) return fail(c, MTSGPU_EINVAL, "explicit samples start at record 0");
	if (n == 0) return 0;
	if (!out) return fail(c, MTSGPU_EINVAL, "null output");
	const uint32_t spp = effectiveSpp(c);
	// the grid of mtsgpu_render's keys: the full film, grown by the filter border with highQualityEdges
	const int border = c->hqEdges ? c->filtBorder : 0;
	const uint32_t keyW = (uint32_t) (filmWidth(c) + 2 * border);
	if ((uint64_t) keyW * (uint64_t) (filmHeight(c) + 2 * border) > 0xFFFFFFFFull) return fail(c, MTSGPU_EINVAL, "film too large");
	std::vector<uint32_t> keys(n), samples(3 * (size_t) n);
	for (uint32_t i = 0; i < n; ++i) {
		const int32_t x = pix_samples[3 * (size_t) i], y = pix_samples[3 * (size_t) i + 1], j = pix_samples[3 * (size_t) i + 2];
		if (x < -border || y < -border || x >= c->cam.width + border || y >= c->cam.height + border || j < 0 || (uint32_t) j >= spp)
			return fail(c, MTSGPU_EINVAL, "sample %u: pixel or sample index out of range", i);
		// k_generate adds the crop offset and forms the key; cfg.pix_off takes the border off again
		samples[3 * (size_t) i] = (uint32_t) (x + border); samples[3 * (size_t) i + 1] = (uint32_t) (y + border); samples[3 * (size_t) i + 2] = (uint32_t) j;
		keys[i] = ((uint32_t) (y + border) + (uint32_t) c->cam.crop_offset_y) * keyW + (uint32_t) (x + border) + (uint32_t) c->cam.crop_offset_x;
	}
	rc = putExplicitSamples(c, samples.data(), keys.data(), n); if (rc) return rc;
	DConfig cfg = makeConfig(c, true);
	cfg.pix_w = (int) keyW; cfg.pix_off = -border;
	rc = generatePaths(c, cfg, 0, n, c->explicitSamples, n); if (rc) return rc;
	// `samples` and `keys` live on this stack; the read-back below waits for the stream
	return readCameraRows(c, 0, n, out);
}

int mtsgpu_hook_rays_redone(mtsgpu_ctx *c, uint64_t *out) {
	if (!c || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	*out = c->raysRedone;
	return 0;
}

int mtsgpu_bin_entries(mtsgpu_ctx *c, uint64_t *out) {
	if (!c || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	for (int b = 0; b < kNumBins; ++b) out[b] = c->binEntries[b];
	return 0;
}

} // extern "C"
