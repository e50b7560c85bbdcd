// ctx.h -- the context behind the C ABI (include/mtsgpu.h) and the helpers its translation units share: api.cpp (context,
// setters, film), scene_upload.cpp, scene_attach.cpp, render.cpp (the wavefront engine), readout.cpp (test and measurement hooks),
// group.cpp.  scene_layout.cpp, the pure half of the upload calls, is declared in host.h and does not include this file.
// Device memory of a context has one owner per buffer: a DevBuf (grow-only, freed by its destructor) or one of the *Allocs
// lists; ~mtsgpu_ctx releases the lists, the pinned words, the events and the streams, so mtsgpu_destroy names no buffer.
#pragma once
#include "host.h"
#include "kernels.h"
#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>

namespace mg {
extern thread_local std::string g_lastError;
// records the message (thread-local and in the context) and returns `code`
int fail(mtsgpu_ctx *ctx, int code, const char *fmt, ...);
}

#define HIPCHK(ctx, expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
	return mg::fail(ctx, MTSGPU_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)

namespace mg {
// A device buffer with one owner.  ensure() only ever grows it (the contents are lost when it does); the destructor frees
// it, with the owner's device current (mtsgpu_destroy, mtsgpu_group_destroy).  Reads as the pointer it holds.
template <typename T> struct DevBuf {
	T *p = nullptr; size_t cap = 0;
	DevBuf() = default;
	DevBuf(const DevBuf &) = delete;
	DevBuf &operator=(const DevBuf &) = delete;
	~DevBuf() { release(); }
	operator T *() const { return p; }
	void release() { if (p) (void) hipFree(p); p = nullptr; cap = 0; }
	int ensure(mtsgpu_ctx *c, size_t need) {
		if (need <= cap) return 0;
		release();
		void *raw = nullptr;
		HIPCHK(c, hipMalloc(&raw, need * sizeof(T)));
		p = static_cast<T *>(raw); cap = need;
		return 0;
	}
};

// The pinned words of a context (mtsgpu_ctx::hostCounters): the counter set readCounters() fetches, then two scratch values
// behind it: the path-length sum of a frame (64 bits) and the queue size a chunk of device-driven bounces ends with
constexpr size_t kHostPathLenWord = (size_t) kNumCounters * kCounterStride;
constexpr size_t kHostNextWord = kHostPathLenWord + 2;
constexpr size_t kHostCounterWords = kHostPathLenWord + 4;
// bytes of one counter set (kCounterSets of them alternate between bounces)
constexpr size_t kCounterSetBytes = (size_t) kNumCounters * kCounterStride * sizeof(uint32_t);

using EventPool = std::vector<std::pair<hipEvent_t, hipEvent_t>>;
inline void freeAll(std::vector<void *> &v) { for (void *p : v) (void) hipFree(p); v.clear(); }

// One record per attachment family: the device arrays it owns apart from the scene's (they come and go between two uploads),
// the view its kernels take (all NULL while the family is off) and host copies of the tables in force (empty = none), by which
// the other families' calls refuse what this one holds (claimRefusal, host.h).  clear() is a setter's free and an upload's reset.
struct ColorFamily {                     // mtsgpu_set_vertex_colors
	std::vector<void *> allocs;
	DColors d{ nullptr, nullptr };
	std::vector<uint32_t> slots;         // bsdf_color_slots
	void clear() { freeAll(allocs); d = DColors{ nullptr, nullptr }; slots.clear(); }
};
struct TextureFamily {                   // mtsgpu_set_uv_textures, _bitmap_textures, _masked_textures: the masks are owned with the textures
	std::vector<void *> allocs;
	DTextures d{ nullptr, nullptr, nullptr, nullptr };
	DMasks msk{ nullptr };
	std::vector<int32_t> slotTex;        // bsdf_slot_texture
	std::vector<uint32_t> maskKind;
	std::vector<uint32_t> shapeHasUv;    // the shapes that have texcoords and the extremes of their texcoords (uMin, uMax, vMin, vMax
	std::vector<double> uvRange;         // per shape), which the cloth call checks its casts on
	void clear() {
		freeAll(allocs); d = DTextures{ nullptr, nullptr, nullptr, nullptr }; msk = DMasks{ nullptr };
		slotTex.clear(); maskKind.clear(); shapeHasUv.clear(); uvRange.clear();
	}
};
struct SnowFamily {                      // mtsgpu_set_snow_bsdfs
	std::vector<void *> allocs;
	DSnows d{ nullptr };
	std::vector<uint32_t> kind;
	void clear() { freeAll(allocs); d = DSnows{ nullptr }; kind.clear(); }
};
struct ClothFamily {                     // mtsgpu_set_cloth_bsdfs
	std::vector<void *> allocs;
	DCloths d{ nullptr, nullptr, nullptr, nullptr };
	std::vector<int32_t> weave;          // bsdf_weave
	void clear() { freeAll(allocs); d = DCloths{ nullptr, nullptr, nullptr, nullptr }; weave.clear(); }
};
struct SpotFamily {                      // mtsgpu_set_spot_textures
	std::vector<void *> allocs;
	DSpots d{ nullptr, nullptr, nullptr, nullptr };
	void clear() { freeAll(allocs); d = DSpots{ nullptr, nullptr, nullptr, nullptr }; }
};
struct TangentFamily {                   // mtsgpu_upload_scene_tangents: the arrays are the scene's (sceneAllocs) and go with it
	DTangents d{ nullptr, nullptr };
	void clear() { d = DTangents{ nullptr, nullptr }; }
};
}

struct mtsgpu_ctx {
	// with `device` current and idle (mtsgpu_destroy): everything no DevBuf member owns.  A caller's stream or film is not ours.
	~mtsgpu_ctx() {
		for (auto *list : { &sceneAllocs, &colors.allocs, &tex.allocs, &snow.allocs, &cloth.allocs, &spots.allocs, &pathAllocs }) mg::freeAll(*list);
		if (hostCounters) (void) hipHostFree(hostCounters);
		for (auto *pool : { &traceEvents, &shadeEvents })
			for (auto &e : *pool) { (void) hipEventDestroy(e.first); (void) hipEventDestroy(e.second); }
		for (hipEvent_t e : { evShade[0], evShade[1], evShadow[0], evShadow[1], evCount }) if (e) (void) hipEventDestroy(e);
		if (ownStream && stream) (void) hipStreamDestroy(stream);
		if (stream2) (void) hipStreamDestroy(stream2);
	}

	int device = 0;
	uint32_t nCUs = 256;                   // hipDeviceProp_t::multiProcessorCount
	hipStream_t stream = nullptr;
	bool ownStream = false;
	// second stream of device-driven bounces (runBouncesDevice): the shadow rays of bounce b are traced on it while `stream`
	// already traces the closest hits of bounce b + 1 (both only depend on the shading of bounce b); evShade / evShadow order
	// the two
	hipStream_t stream2 = nullptr;
	hipEvent_t evShade[2] = { nullptr, nullptr }, evShadow[2] = { nullptr, nullptr }, evCount = nullptr;
	std::string error;

	// scene
	bool haveScene = false;
	mg::DScene dsc{};
	std::vector<void *> sceneAllocs;
	uint32_t nTris = 0;
	mg::HostScene host;                     // what the setters need of it once the caller's arrays may be gone
	// what comes and goes between two uploads, one record per family (below)
	mg::ColorFamily colors;
	mg::TextureFamily tex;
	mg::SnowFamily snow;
	mg::ClothFamily cloth;
	mg::TangentFamily tan;
	mg::SpotFamily spots;
	// a new scene starts without any of them
	void clearAttachments() { colors.clear(); tex.clear(); snow.clear(); cloth.clear(); tan.clear(); spots.clear(); }
	// the tables in force, as the pure checks of host.h take them
	mg::InForce inForce() const {
		auto p = [](const auto &v) { return v.empty() ? nullptr : v.data(); };
		mg::InForce f;
		f.colorSlots = p(colors.slots); f.slotTex = p(tex.slotTex); f.maskKind = p(tex.maskKind); f.snowKind = p(snow.kind);
		f.clothWeave = p(cloth.weave); f.shapeHasUv = p(tex.shapeHasUv); f.uvRange = p(tex.uvRange);
		f.spotTextures = spots.d.lum_texture != nullptr;
		return f;
	}

	// configuration
	bool haveCamera = false;
	mtsgpu_camera cam{};
	int maxDepth = -1, rrDepth = 10, strictNormals = 0;
	int samplerKind = MTSGPU_SAMPLER_INDEPENDENT_KEYED;
	uint32_t spp = 4; int ldDepth = 3; uint64_t seed = 0;
	int blockSize = 32, part = 0, nParts = 1;
	uint64_t maxPaths = 0; bool countTraversal = false, timeKernels = false;
	std::map<std::string, long> tuning;      // mtsgpu_set_tuning

	// film
	float *film = nullptr;                 // the film in use: ownedFilm's, or the caller's (mtsgpu_set_film_buffer), never freed here
	mg::DevBuf<float> ownedFilm; bool ownFilm = false; size_t filmPixels = 0;
	float filtSizeX = 0.5f, filtSizeY = 0.5f; int filtBorder = 0;
	bool hqEdges = false;
	int integrator = 0, nLumSamples = 1, nBsdfSamples = 1;
	mg::DevBuf<float> filtValues;          // device [16][16]
	// test-case mode (mtsgpu_set_film_statistics): per-pixel variance [H][W][3] and sample count [H][W], allocated only while
	// the mode is on; statsForm = the form of the variance kernel the last pass ran (0 lane, 1 wave, -1 none)
	bool filmStats = false;
	mg::DevBuf<float> statVar; mg::DevBuf<uint32_t> statN; size_t statPixels = 0;
	int statsForm = -1;
	mg::DevBuf<mg::TileMeta> tileMeta;
	mg::DevBuf<float> blocks;

	// per-pass buffers
	size_t pathCap = 0;
	mg::DPaths paths{};
	mg::DQueues q{};
	uint32_t *queueA = nullptr, *queueB = nullptr;
	float4 *rayqA[2] = { nullptr, nullptr }, *rayqB[2] = { nullptr, nullptr };      // the rays of queueA / queueB in queue order (o, d)
	uint4 *binHits = nullptr;               // DQueues::bin_hits: the hits of binned paths, next to their ids
	mg::DevBuf<uint32_t> pixelList;
	// The work units of a frame (pixel keys in tile order + tile rectangles) depend on the film geometry and the tile
	// sharding only: they are kept from frame to frame (a 1-spp frame spent 0.55 of its 10.6 ms rebuilding and uploading
	// them).  renderKey is what they were built for; the test hooks that borrow pixelList clear renderListValid.
	std::vector<uint32_t> renderPixels; std::vector<mg::TileMeta> renderTiles;
	std::vector<long long> renderKey; bool renderListValid = false;
	mg::DevBuf<uint32_t> ldScr; mg::DevBuf<uint16_t> ldPerm;
	mg::DevBuf<uint16_t> ldScratch;        // the tables of a pass while they are shuffled (kernels.h)
	// Sampler::request2DArray arrays of the direct integrator (per pass, like the tables above)
	mg::DevBuf<unsigned long long> ldState;
	mg::DevBuf<uint32_t> arrScr; mg::DevBuf<uint16_t> arrPerm; mg::DevBuf<float2> arrPts;
	mg::DevBuf<float4> primSave;
	mg::DevBuf<float4> shqNee;             // DPaths::shq_nee, once a frame has run with DQueues::nee_parked == 0
	mg::DevBuf<uint16_t> primes;           // primeTable (util.cpp:64-122) on the device
	mg::DevBuf<uint32_t> explicitSamples;
	uint32_t *hostCounters = nullptr;       // pinned, kHostCounterWords words
	uint32_t *counterSets = nullptr;        // kCounterSets x kNumCounters lines, used by alternate bounces
	uint32_t *spillClosest = nullptr, *spillShadow = nullptr;   // the two traversal kernels run concurrently
	mg::BinView *viewsDev = nullptr;        // device-driven bounces: per-bin views written by k_prep
	unsigned long long *devStats = nullptr; // kStat* counters of a device-driven frame
	bool devStatsUsed = false;              // a device-driven pass ran since the statistics were cleared
	uint32_t binMask = 0x1FFu;              // bins that can be non-empty with the uploaded scene (BSDF types present + terminal)
	mg::DevBuf<unsigned long long> pathLen; // device: sum of the final path depths of a render (avgPathLength)
	std::vector<void *> pathAllocs;

	// stats
	mtsgpu_stats stats{};
	// entries the closest-hit launches of the last frame appended to every material queue (mtsgpu_bin_entries): counted by the
	// host where it reads the shard counters back, by k_prep otherwise
	uint64_t binEntries[mg::kNumBins] = {};
	// closest-hit rays of the last frame that the lean kernel handed to the kernel with the mailbox (mtsgpu_hook_rays_redone)
	uint64_t raysRedone = 0;
	mg::EventPool traceEvents, shadeEvents; // the timing events of a frame with time_kernels on, kept from frame to frame
	size_t traceEvUsed = 0, shadeEvUsed = 0;
	std::vector<unsigned char> traceEvClass;      // per traversal launch: 0 closest-hit, 1 closest-hit of a pass's first bounce, 2 any-hit
	bool debug = false;                     // MTSGPU_DEBUG was set when the frame began
	// what mtsgpu_replay_roof needs to know about the pass rendered last: how to generate its camera rays again, and
	// how many slots of the shadow queue hold rays (the largest shadow launch of the pass; 0 after device-driven bounces)
	struct LastPass { bool valid = false; mg::DConfig cfg{}; size_t base = 0; uint32_t nSlots = 0, nPaths = 0, shadowMax = 0; } lastPass;
};


// What the translation units behind the C ABI share besides the context.  Only what a second file uses is declared here;
// everything else is local to its file.
#pragma GCC visibility push(hidden)      // internal to the library: the exported names are the C ABI's
namespace mg {
template <typename T> int devAlloc(mtsgpu_ctx *ctx, T **p, size_t count, std::vector<void *> &owner) {
	void *raw = nullptr;
	HIPCHK(ctx, hipMalloc(&raw, std::max<size_t>(count, 1) * sizeof(T)));
	owner.push_back(raw);
	*p = static_cast<T *>(raw);
	return 0;
}

// owner: the list the allocation is filed under (NULL: the scene's)
template <typename T> int upload(mtsgpu_ctx *ctx, const T **dst, const T *src, size_t count, std::vector<void *> *owner = nullptr) {
	T *p = nullptr;
	int rc = devAlloc(ctx, &p, count, owner ? *owner : ctx->sceneAllocs);
	if (rc) return rc;
	if (count) HIPCHK(ctx, hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice));
	*dst = p;
	return 0;
}

// a pair of timing events, released on every way out of the function that holds it
struct EventPair {
	hipEvent_t a = nullptr, b = nullptr;
	~EventPair() { if (a) (void) hipEventDestroy(a); if (b) (void) hipEventDestroy(b); }
};

// api.cpp
uint32_t effectiveSpp(const mtsgpu_ctx *c);
int checkReady(mtsgpu_ctx *c);
int ensureFilm(mtsgpu_ctx *c);
int ensureFilmStats(mtsgpu_ctx *c);

// render.cpp
void applyTuning(mtsgpu_ctx *c);
bool samplerHasTables(const mtsgpu_ctx *c);
int ensureTableWork(mtsgpu_ctx *c, size_t nSlots, uint32_t spp);
DConfig makeConfig(const mtsgpu_ctx *c, bool slotPerPath);
void rayQueues(mtsgpu_ctx *c, const uint32_t *cur, const uint32_t *nxt);
// ... and outside the bounce loops nobody reads or writes them (test hooks and the replay measurement trace rays they put
// into the records)
struct RayQueuesOff { mtsgpu_ctx *c; ~RayQueuesOff() { rayQueues(c, nullptr, nullptr); c->q.nee_parked = 0; c->q.miss_settled = 0; } };

} // namespace mg
#pragma GCC visibility pop

// A measurement hook outside the C ABI of include/mtsgpu.h (ABI version 8 fixes mtsgpu_stats and the list of entry points): the
// closest-hit rays of the last frame, or mtsgpu_trace_rays call, that were traced a second time, with the mailbox, because two
// primitives tied in t on them (tuning key "lean_closest"; render.cpp: traceAndBin).  A redone ray counts once in rays_closest
// and once in mtsgpu_bin_entries.
extern "C" int mtsgpu_hook_rays_redone(mtsgpu_ctx *ctx, uint64_t *out);
