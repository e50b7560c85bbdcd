// api.cpp -- the C ABI of libmtsgpu (include/mtsgpu.h): the context, its configuration setters and its film, and the
// wrappers of the host-side loaders.  The scene goes to HBM in scene_upload.cpp (scene_attach.cpp: what comes and goes between
// two uploads; scene_layout.cpp: what both check and lay out, without a context), render.cpp drives the wavefront stages per
// bounce, readout.cpp holds the test and measurement hooks.
// There is no CPU fallback: every compute entry point needs a gfx950 device.
#include "ctx.h"
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <cmath>

using namespace mg;

namespace {

// The events that order the two streams of a context against each other (shading of bounce b -> its shadow rays on the
// second stream -> shading of bounce b + 1): both streams run on one device, so a device-scope release is all they need
#ifndef MG_EV_DEVICE
#define MG_EV_DEVICE 0
#endif
constexpr unsigned kOrderEventFlags = hipEventDisableTiming | (MG_EV_DEVICE ? hipEventReleaseToDevice : 0u);

uint32_t roundToPow2(uint32_t v) { uint32_t r = 1; while (r < v) r <<= 1; return r; }

uint32_t squareAtLeast(uint32_t v) { uint32_t i = 1; while ((uint64_t) i * i < v) ++i; return i * i; }

} // namespace

namespace mg {
thread_local std::string g_lastError;

int fail(mtsgpu_ctx *ctx, int code, const char *fmt, ...) {
	char buf[512];
	va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
	g_lastError = buf;
	if (ctx) ctx->error = buf;
	return code;
}

uint32_t effectiveSpp(const mtsgpu_ctx *c) {
	if (c->samplerKind == MTSGPU_SAMPLER_LD_KEYED) return roundToPow2(c->spp);                 // ldsampler.cpp:52-57
	if (c->samplerKind == MTSGPU_SAMPLER_STRATIFIED_KEYED) return squareAtLeast(c->spp);       // stratified.cpp:36-44
	return c->spp;
}

int checkReady(mtsgpu_ctx *c) {
	if (!c) return fail(nullptr, MTSGPU_EINVAL, "null context");
	if (!c->haveScene) return fail(c, MTSGPU_ESTATE, "no scene uploaded");
	if (!c->haveCamera) return fail(c, MTSGPU_ESTATE, "no camera set");
	if (hipSetDevice(c->device) != hipSuccess) return fail(c, MTSGPU_EHIP, "hipSetDevice failed");
	return 0;
}

int ensureFilm(mtsgpu_ctx *c) {
	const size_t px = (size_t) c->cam.width * c->cam.height;
	if (c->film && !c->ownFilm) return 0;
	if (c->film && c->filmPixels == px) return 0;
	// a film of another size is a new film, zeroed: released first, so that the buffer is not merely grown into
	c->film = nullptr; c->ownedFilm.release();
	if (int rc = c->ownedFilm.ensure(c, px * 5)) return rc;
	HIPCHK(c, hipMemset(c->ownedFilm, 0, px * 5 * sizeof(float)));
	c->film = c->ownedFilm; c->ownFilm = true; c->filmPixels = px;
	return 0;
}

// the statistics buffers of the test-case mode, zeroed when (re)allocated: sized like the film, owned by the context
static void freeFilmStats(mtsgpu_ctx *c) { c->statVar.release(); c->statN.release(); c->statPixels = 0; }
int ensureFilmStats(mtsgpu_ctx *c) {
	const size_t px = (size_t) c->cam.width * c->cam.height;
	if (c->statVar && c->statN && c->statPixels == px) return 0;
	HIPCHK(c, hipStreamSynchronize(c->stream));
	freeFilmStats(c);
	if (int rc = c->statVar.ensure(c, px * 3)) return rc;
	if (int rc = c->statN.ensure(c, px)) return rc;
	HIPCHK(c, hipMemset(c->statVar, 0, px * 3 * sizeof(float)));
	HIPCHK(c, hipMemset(c->statN, 0, px * sizeof(uint32_t)));
	c->statPixels = px;
	return 0;
}

} // namespace mg

extern "C" {

int mtsgpu_abi_version(void) { return MTSGPU_ABI_VERSION; }

size_t mtsgpu_abi_sizeof(int which) {
	switch (which) {
		case 0: return sizeof(mtsgpu_scene);
		case 1: return sizeof(mtsgpu_camera);
		case 2: return sizeof(mtsgpu_stats);
		case 3: return sizeof(mtsgpu_mesh);
		case 4: return sizeof(mtsgpu_scene_desc);
		case 5: return sizeof(mtsgpu_kd_params);
		default: return 0;
	}
}

const char *mtsgpu_last_error(const mtsgpu_ctx *ctx) { return ctx ? ctx->error.c_str() : g_lastError.c_str(); }

int mtsgpu_create(int device, mtsgpu_ctx **out) {
	if (!out) return fail(nullptr, MTSGPU_EINVAL, "out is null");
	*out = nullptr;
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
		return fail(nullptr, MTSGPU_ENODEV, "no HIP device visible; libmtsgpu has no CPU fallback");
	if (device < 0 || device >= n)
		return fail(nullptr, MTSGPU_EINVAL, "device %d out of range (%d visible)", device, n);
	hipDeviceProp_t prop;
	HIPCHK(nullptr, hipGetDeviceProperties(&prop, device));
	if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
		return fail(nullptr, MTSGPU_ENODEV, "device %d is %s; libmtsgpu is built for gfx950 only", device, prop.gcnArchName);
	HIPCHK(nullptr, hipSetDevice(device));
	mtsgpu_ctx *c = new mtsgpu_ctx();
	c->device = device;
	c->nCUs = (uint32_t) std::max(1, prop.multiProcessorCount);
	// from here on every failure goes through mtsgpu_destroy: whatever exists by then has its owner in the context
	auto give_up = [&](const char *what) { mtsgpu_destroy(c); return fail(nullptr, MTSGPU_EHIP, "%s failed", what); };
	if (hipStreamCreate(&c->stream) != hipSuccess) return give_up("hipStreamCreate");
	c->ownStream = true;
	{
		bool ok = hipStreamCreate(&c->stream2) == hipSuccess && hipEventCreateWithFlags(&c->evCount, hipEventDisableTiming) == hipSuccess;
		for (int i = 0; i < 2 && ok; ++i)
			ok = hipEventCreateWithFlags(&c->evShade[i], kOrderEventFlags) == hipSuccess
			  && hipEventCreateWithFlags(&c->evShadow[i], kOrderEventFlags) == hipSuccess;
		if (!ok) return give_up("stream / event creation");
	}
	if (hipHostMalloc((void **) &c->hostCounters, kHostCounterWords * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess)
		return give_up("hipHostMalloc");
	if (c->pathLen.ensure(c, 1)) return give_up("hipMalloc");
	{
		// the first 1000 primes (primeTable, src/libcore/util.cpp:64-122) for the halton / hammersley samplers
		std::vector<uint16_t> primes;
		for (uint32_t v = 2; primes.size() < 1000; ++v) {
			bool isPrime = true;
			for (uint32_t d = 2; d * d <= v; ++d) if (v % d == 0) { isPrime = false; break; }
			if (isPrime) primes.push_back((uint16_t) v);
		}
		if (c->primes.ensure(c, primes.size())
		    || hipMemcpy(c->primes, primes.data(), primes.size() * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess)
			return give_up("prime table upload");
	}
	*out = c;
	return 0;
}

void mtsgpu_destroy(mtsgpu_ctx *c) {
	if (!c) return;
	(void) hipSetDevice(c->device);       // memory is freed with the context's device current ...
	(void) hipDeviceSynchronize();        // ... and idle
	delete c;                             // ~mtsgpu_ctx and the DevBuf members release what the context owns
}

int mtsgpu_set_stream(mtsgpu_ctx *c, void *hip_stream) {
	if (!c) return fail(nullptr, MTSGPU_EINVAL, "null context");
	if (c->ownStream && c->stream) { (void) hipStreamSynchronize(c->stream); (void) hipStreamDestroy(c->stream); }
	if (hip_stream) { c->stream = (hipStream_t) hip_stream; c->ownStream = false; }
	else { HIPCHK(c, hipStreamCreate(&c->stream)); c->ownStream = true; }
	return 0;
}

int mtsgpu_set_camera(mtsgpu_ctx *c, const mtsgpu_camera *cam) {
	if (!c || !cam) return fail(c, MTSGPU_EINVAL, "null argument");
	c->lastPass.valid = false;
	if (cam->width <= 0 || cam->height <= 0 || (uint64_t) cam->width * (uint64_t) cam->height > 0x7FFFFFFFull)
		return fail(c, MTSGPU_EINVAL, "bad film size %dx%d", cam->width, cam->height);
	if (cam->kind != 0 && cam->kind != 1) return fail(c, MTSGPU_EINVAL, "unknown camera kind %d", cam->kind);
	if (cam->film_width != 0 || cam->film_height != 0 || cam->crop_offset_x != 0 || cam->crop_offset_y != 0) {
		// "Invalid crop window specification!" (film.cpp:41-45)
		if (cam->crop_offset_x < 0 || cam->crop_offset_y < 0 || cam->film_width <= 0 || cam->film_height <= 0
		    || (int64_t) cam->crop_offset_x + cam->width > cam->film_width || (int64_t) cam->crop_offset_y + cam->height > cam->film_height
		    || (uint64_t) cam->film_width * (uint64_t) cam->film_height > 0x7FFFFFFFull)
			return fail(c, MTSGPU_EINVAL, "invalid crop window %dx%d at (%d, %d) of a %dx%d film", cam->width, cam->height,
			            cam->crop_offset_x, cam->crop_offset_y, cam->film_width, cam->film_height);
	}
	c->cam = *cam; c->haveCamera = true;
	return 0;
}

int mtsgpu_set_integrator(mtsgpu_ctx *c, int max_depth, int rr_depth, int strict_normals) {
	if (!c) return fail(nullptr, MTSGPU_EINVAL, "null context");
	c->lastPass.valid = false;      // mtsgpu_replay_roof regenerates a pass from its saved configuration: not across a setter
	if (rr_depth <= 0) return fail(c, MTSGPU_EINVAL, "rrDepth == 0 breaks the computation of alpha values! (integrator.cpp:291)");
	c->maxDepth = max_depth; c->rrDepth = rr_depth; c->strictNormals = strict_normals ? 1 : 0;
	c->integrator = 0;
	return 0;
}

int mtsgpu_set_direct_integrator(mtsgpu_ctx *c, int luminaire_samples, int bsdf_samples) {
	if (!c) return fail(nullptr, MTSGPU_EINVAL, "null context");
	c->lastPass.valid = false;      // mtsgpu_replay_roof regenerates a pass from its saved configuration: not across a setter
	if (luminaire_samples < 0 || bsdf_samples < 0 || luminaire_samples + bsdf_samples <= 0)
		return fail(c, MTSGPU_EINVAL, "luminaireSamples + bsdfSamples must be > 0 (direct.cpp:41)");
	if (luminaire_samples > 65536 || bsdf_samples > 65536)
		return fail(c, MTSGPU_EINVAL, "at most 65536 samples per strategy");
	c->integrator = 1; c->nLumSamples = luminaire_samples; c->nBsdfSamples = bsdf_samples;
	return 0;
}

int mtsgpu_set_sampler(mtsgpu_ctx *c, int kind, uint32_t spp, int ld_depth, uint64_t seed) {
	if (!c) return fail(nullptr, MTSGPU_EINVAL, "null context");
	c->lastPass.valid = false;      // mtsgpu_replay_roof regenerates a pass from its saved configuration: not across a setter
	if (kind < MTSGPU_SAMPLER_INDEPENDENT_KEYED || kind > MTSGPU_SAMPLER_STRATIFIED_KEYED) return fail(c, MTSGPU_EINVAL, "unknown sampler kind %d", kind);
	if (spp == 0) return fail(c, MTSGPU_EINVAL, "sampleCount must be > 0");
	if (kind == MTSGPU_SAMPLER_LD_KEYED && (roundToPow2(spp) > 65536u || ld_depth < 1 || ld_depth > 64))
		return fail(c, MTSGPU_EINVAL, "ldsampler: sampleCount <= 65536 and 1 <= depth <= 64 required");
	if (kind == MTSGPU_SAMPLER_STRATIFIED_KEYED && (spp > 65536u || squareAtLeast(spp) > 65536u || ld_depth < 1 || ld_depth > 64))
		return fail(c, MTSGPU_EINVAL, "stratified: sampleCount <= 65536 and 1 <= depth <= 64 required");
	c->samplerKind = kind; c->spp = spp; c->ldDepth = ld_depth > 0 ? ld_depth : 3; c->seed = seed;
	return 0;
}

int mtsgpu_set_tiles(mtsgpu_ctx *c, int block_size, int part, int n_parts) {
	if (!c) return fail(nullptr, MTSGPU_EINVAL, "null context");
	c->lastPass.valid = false;      // mtsgpu_replay_roof regenerates a pass from its saved configuration: not across a setter
	if (block_size <= 0 || n_parts <= 0 || part < 0 || part >= n_parts) return fail(c, MTSGPU_EINVAL, "bad tile sharding %d/%d/%d", block_size, part, n_parts);
	c->blockSize = block_size; c->part = part; c->nParts = n_parts;
	return 0;
}

int mtsgpu_set_rfilter(mtsgpu_ctx *c, float size_x, float size_y, const float *values) {
	if (!c) return fail(nullptr, MTSGPU_EINVAL, "null context");
	c->lastPass.valid = false;      // mtsgpu_replay_roof regenerates a pass from its saved configuration: not across a setter
	if (!values) { c->filtSizeX = c->filtSizeY = 0.5f; c->filtBorder = 0; return 0; }
	if (!(size_x > 0) || !(size_y > 0) || size_x > 8 || size_y > 8) return fail(c, MTSGPU_EINVAL, "bad filter size");
	HIPCHK(c, hipSetDevice(c->device));
	if (int rc = c->filtValues.ensure(c, 256)) return rc;
	HIPCHK(c, hipMemcpy(c->filtValues, values, 256 * sizeof(float), hipMemcpyHostToDevice));
	c->filtSizeX = size_x; c->filtSizeY = size_y;
	c->filtBorder = (int) std::ceil(std::max(size_x, size_y) - 0.5f);       // renderproc.cpp:143-144
	return 0;
}

int mtsgpu_set_film_edges(mtsgpu_ctx *c, int high_quality_edges) {
	if (!c) return fail(nullptr, MTSGPU_EINVAL, "null context");
	c->lastPass.valid = false;      // mtsgpu_replay_roof regenerates a pass from its saved configuration: not across a setter
	c->hqEdges = high_quality_edges != 0;
	return 0;
}

struct mtsgpu_loaded_mesh { mg::LoadedMesh m; };

int mtsgpu_load_serialized(const char *path, int shape_index, mtsgpu_loaded_mesh **out, mtsgpu_mesh *mesh) {
	if (!path || !out || !mesh) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	*out = nullptr;
	mtsgpu_loaded_mesh *lm = new mtsgpu_loaded_mesh();
	try {
		loadSerializedMesh(path, shape_index, lm->m);
	} catch (const std::exception &e) {
		delete lm;
		return fail(nullptr, MTSGPU_EINVAL, "%s", e.what());
	}
	std::memset(mesh, 0, sizeof(*mesh));
	mesh->n_verts = (uint32_t) (lm->m.positions.size() / 3); mesh->n_tris = (uint32_t) (lm->m.triangles.size() / 3);
	mesh->positions = lm->m.positions.data();
	mesh->normals = lm->m.normals.empty() ? nullptr : lm->m.normals.data();
	mesh->triangles = lm->m.triangles.data();
	mesh->face_normals = lm->m.faceNormals ? 1 : 0;
	mesh->bsdf = -1; mesh->lum = -1; mesh->shape_type = MTSGPU_SHAPE_TRIMESH;
	*out = lm;
	return 0;
}

void mtsgpu_loaded_mesh_free(mtsgpu_loaded_mesh *m) { delete m; }

const float *mtsgpu_loaded_mesh_texcoords(const mtsgpu_loaded_mesh *m) { return (m && !m->m.texcoords.empty()) ? m->m.texcoords.data() : nullptr; }
const float *mtsgpu_loaded_mesh_colors(const mtsgpu_loaded_mesh *m) { return (m && !m->m.colors.empty()) ? m->m.colors.data() : nullptr; }

int mtsgpu_tabulate_filter(int kind, float half_size, float p0, float p1, float *size_xy, float *values) {
	if (!size_xy || !values || kind < 0 || kind > 4) return fail(nullptr, MTSGPU_EINVAL, "bad filter arguments");
	tabulateFilter(kind, half_size, p0, p1, size_xy, values);
	return 0;
}

int mtsgpu_set_film_buffer(mtsgpu_ctx *c, void *device_ptr) {
	if (!c) return fail(nullptr, MTSGPU_EINVAL, "null context");
	c->ownedFilm.release();
	c->film = (float *) device_ptr; c->ownFilm = false; c->filmPixels = 0;
	return 0;
}

int mtsgpu_set_tuning(mtsgpu_ctx *c, const char *key, long value) {
	if (!c || !key) return fail(c, MTSGPU_EINVAL, "null argument");
	struct Knob { const char *key; long lo, hi; };
	static const Knob knobs[] = { { "refill_min", 1, 64 }, { "desc_min", 1, 64 }, { "leaf_min", 1, 64 }, { "batch", 0, 64 },
	                              { "dyn_div", 0, 1 << 20 }, { "test_retry", 0, 1 }, { "sync_free", -1, 1 }, { "chunk", 1, 1024 }, { "blocks_per_cu", 0, (long) kTraceBlocksPerCuMax }, { "plain_below", 0, 1 << 30 }, { "dyn_min_rounds", 0, 1 << 20 }, { "shade_fused", 0, 1 }, { "ray_queues", 0, 1 }, { "nee_parked", 0, 1 }, { "stats_wave", -1, 1 }, { "miss_shaded", 0, 1 }, { "lean_closest", 0, 7 } };
	for (const Knob &k : knobs)
		if (std::strcmp(k.key, key) == 0) {
			if (value < k.lo || value > k.hi) return fail(c, MTSGPU_EINVAL, "tuning knob %s: %ld outside [%ld, %ld]", key, value, k.lo, k.hi);
			c->tuning[key] = value;
			applyTuning(c);
			return 0;
		}
	return fail(c, MTSGPU_EINVAL, "unknown tuning knob '%s'", key);
}

int mtsgpu_set_options(mtsgpu_ctx *c, uint64_t max_paths, int count_traversal, int time_kernels) {
	if (!c) return fail(nullptr, MTSGPU_EINVAL, "null context");
	c->maxPaths = max_paths; c->countTraversal = count_traversal != 0; c->timeKernels = time_kernels != 0;
	return 0;
}

int mtsgpu_set_film_statistics(mtsgpu_ctx *c, int on) {
	if (!c) return fail(nullptr, MTSGPU_EINVAL, "null context");
	HIPCHK(c, hipSetDevice(c->device));
	c->filmStats = on != 0;
	c->statsForm = -1;
	if (!c->filmStats) {
		HIPCHK(c, hipStreamSynchronize(c->stream));
		freeFilmStats(c);
	}
	return 0;
}

int mtsgpu_film_statistics_form(const mtsgpu_ctx *c) { return c ? c->statsForm : -1; }

int mtsgpu_read_film_statistics(mtsgpu_ctx *c, float *var3, uint32_t *nsamp) {
	int rc = checkReady(c); if (rc) return rc;
	if (!c->filmStats) return fail(c, MTSGPU_ESTATE, "film statistics are off (mtsgpu_set_film_statistics)");
	if (!var3 || !nsamp) return fail(c, MTSGPU_EINVAL, "null output");
	rc = ensureFilmStats(c); if (rc) return rc;
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipMemcpy(var3, c->statVar, c->statPixels * 3 * sizeof(float), hipMemcpyDeviceToHost));
	HIPCHK(c, hipMemcpy(nsamp, c->statN, c->statPixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return 0;
}

int mtsgpu_clear_film(mtsgpu_ctx *c) {
	int rc = checkReady(c); if (rc) return rc;
	rc = ensureFilm(c); if (rc) return rc;
	HIPCHK(c, hipMemsetAsync(c->film, 0, (size_t) c->cam.width * c->cam.height * 5 * sizeof(float), c->stream));
	if (c->filmStats) {
		rc = ensureFilmStats(c); if (rc) return rc;
		HIPCHK(c, hipMemsetAsync(c->statVar, 0, c->statPixels * 3 * sizeof(float), c->stream));
		HIPCHK(c, hipMemsetAsync(c->statN, 0, c->statPixels * sizeof(uint32_t), c->stream));
	}
	return 0;
}

int mtsgpu_sync(mtsgpu_ctx *c) {
	if (!c) return fail(nullptr, MTSGPU_EINVAL, "null context");
	HIPCHK(c, hipStreamSynchronize(c->stream));
	return 0;
}

int mtsgpu_read_film(mtsgpu_ctx *c, float *rgbaw) {
	int rc = checkReady(c); if (rc) return rc;
	if (!rgbaw) return fail(c, MTSGPU_EINVAL, "null output");
	rc = ensureFilm(c); if (rc) return rc;
	HIPCHK(c, hipStreamSynchronize(c->stream));
	HIPCHK(c, hipMemcpy(rgbaw, c->film, (size_t) c->cam.width * c->cam.height * 5 * sizeof(float), hipMemcpyDeviceToHost));
	return 0;
}

int mtsgpu_get_stats(mtsgpu_ctx *c, mtsgpu_stats *out) {
	if (!c || !out) return fail(c, MTSGPU_EINVAL, "null argument");
	*out = c->stats;
	return 0;
}

// --- host-side flattening ------------------------------------------------------
struct mtsgpu_flat_scene { FlatScene fs; };

int mtsgpu_flatten(const mtsgpu_scene_desc *desc, const mtsgpu_kd_params *kd, mtsgpu_flat_scene **out) {
	if (!desc || !out) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	*out = nullptr;
	try {
		std::unique_ptr<mtsgpu_flat_scene> p(new mtsgpu_flat_scene());
		flattenScene(*desc, kd, p->fs);
		*out = p.release();
	} catch (const std::exception &e) {
		return fail(nullptr, MTSGPU_EINVAL, "%s", e.what());
	}
	return 0;
}

int mtsgpu_flatten_tangents(const mtsgpu_scene_desc *desc, const mtsgpu_kd_params *kd, const float *const *mesh_texcoords, mtsgpu_flat_scene **out) {
	return mtsgpu_flatten_tangents_flagged(desc, kd, mesh_texcoords, nullptr, out);
}

int mtsgpu_flatten_tangents_flagged(const mtsgpu_scene_desc *desc, const mtsgpu_kd_params *kd, const float *const *mesh_texcoords,
                                    const uint32_t *bsdf_anisotropic, mtsgpu_flat_scene **out) {
	if (!desc || !out || !mesh_texcoords) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	*out = nullptr;
	try {
		std::unique_ptr<mtsgpu_flat_scene> p(new mtsgpu_flat_scene());
		flattenScene(*desc, kd, p->fs, mesh_texcoords, bsdf_anisotropic);
		for (uint32_t s = 0; s < desc->n_meshes; ++s)
			if (mesh_texcoords[s] && desc->meshes[s].shape_type == MTSGPU_SHAPE_TRIMESH) {
				const std::string why = setMeshTexcoords(p->fs, s, mesh_texcoords[s]);
				if (!why.empty()) throw std::runtime_error(why);
			}
		*out = p.release();
	} catch (const std::exception &e) {
		return fail(nullptr, MTSGPU_EINVAL, "%s", e.what());
	}
	return 0;
}
int mtsgpu_flatten_cylinders(const mtsgpu_scene_desc *desc, const mtsgpu_kd_params *kd, const float *const *mesh_texcoords,
                             const uint32_t *bsdf_anisotropic, const mtsgpu_cylinder *cylinders, mtsgpu_flat_scene **out) {
	if (!desc || !out) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	*out = nullptr;
	try {
		std::unique_ptr<mtsgpu_flat_scene> p(new mtsgpu_flat_scene());
		flattenScene(*desc, kd, p->fs, mesh_texcoords, bsdf_anisotropic, cylinders);
		for (uint32_t s = 0; mesh_texcoords && s < desc->n_meshes; ++s)
			if (mesh_texcoords[s] && desc->meshes[s].shape_type == MTSGPU_SHAPE_TRIMESH) {
				const std::string why = setMeshTexcoords(p->fs, s, mesh_texcoords[s]);
				if (!why.empty()) throw std::runtime_error(why);
			}
		*out = p.release();
	} catch (const std::exception &e) {
		return fail(nullptr, MTSGPU_EINVAL, "%s", e.what());
	}
	return 0;
}
const float *mtsgpu_flat_scene_cylinders(const mtsgpu_flat_scene *fs) { return (fs && !fs->fs.cylinders.empty()) ? fs->fs.cylinders.data() : nullptr; }

int mtsgpu_cylinder_configure(const mtsgpu_cylinder *in, float *derived) {
	if (!in || !derived) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	float D[MTSGPU_CYLINDER_NDERIVED];
	const std::string why = cylinderConfigure(*in, D);
	if (!why.empty()) return fail(nullptr, MTSGPU_EINVAL, "mtsgpu_cylinder_configure: %s", why.c_str());
	std::memcpy(derived, D, sizeof(D));
	return 0;
}
int mtsgpu_cylinder_aabb(const float *derived, float *out6) {
	if (!derived || !out6) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	const std::string why = checkCylinderBlock(derived);
	if (!why.empty()) return fail(nullptr, MTSGPU_EINVAL, "mtsgpu_cylinder_aabb: %s", why.c_str());
	cylinderAabb(derived, out6);
	return 0;
}
int mtsgpu_cylinder_clip(const float *derived, uint32_t n, const float *boxes, int on_device, float *out, uint32_t *valid) {
	if (!derived || !boxes || !out || !valid) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	const std::string why = checkCylinderBlock(derived);
	if (!why.empty()) return fail(nullptr, MTSGPU_EINVAL, "mtsgpu_cylinder_clip: %s", why.c_str());
	float own[6], row[8];
	cylinderAabb(derived, own);
	cylinderBuilderRow(derived, row);
	try {
		if (on_device) cylinderClipDevice(row, own, n, boxes, out, valid);
		else cylinderClipHost(row, own, n, boxes, out, valid);
	} catch (const std::exception &e) {
		return fail(nullptr, MTSGPU_EINVAL, "mtsgpu_cylinder_clip: %s", e.what());
	}
	return 0;
}

static bool flatSceneHasTangents(const mtsgpu_flat_scene *fs) {
	if (!fs) return false;
	for (uint32_t h : fs->fs.shapeHasTan) if (h) return true;
	return false;
}
const float *mtsgpu_flat_scene_vertex_tangents(const mtsgpu_flat_scene *fs) { return flatSceneHasTangents(fs) ? fs->fs.vtxTan.data() : nullptr; }
const uint32_t *mtsgpu_flat_scene_shape_has_tangents(const mtsgpu_flat_scene *fs) { return flatSceneHasTangents(fs) ? fs->fs.shapeHasTan.data() : nullptr; }

const mtsgpu_scene *mtsgpu_flat_scene_get(const mtsgpu_flat_scene *fs) { return fs ? &fs->fs.sc : nullptr; }
void mtsgpu_flat_scene_free(mtsgpu_flat_scene *fs) { delete fs; }

int mtsgpu_flat_scene_set_mesh_colors(mtsgpu_flat_scene *fs, uint32_t mesh_index, const float *colors) {
	if (!fs) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	const std::string why = setMeshColors(fs->fs, mesh_index, colors);
	if (!why.empty()) return fail(nullptr, MTSGPU_EINVAL, "%s", why.c_str());
	return 0;
}

static bool flatSceneHasColors(const mtsgpu_flat_scene *fs) {
	if (!fs) return false;
	for (uint32_t h : fs->fs.shapeHasColors) if (h) return true;
	return false;
}
const float *mtsgpu_flat_scene_vertex_colors(const mtsgpu_flat_scene *fs) { return flatSceneHasColors(fs) ? fs->fs.vtxCol.data() : nullptr; }
const uint32_t *mtsgpu_flat_scene_shape_has_colors(const mtsgpu_flat_scene *fs) { return flatSceneHasColors(fs) ? fs->fs.shapeHasColors.data() : nullptr; }

int mtsgpu_flat_scene_set_mesh_texcoords(mtsgpu_flat_scene *fs, uint32_t mesh_index, const float *texcoords) {
	if (!fs) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	const std::string why = setMeshTexcoords(fs->fs, mesh_index, texcoords);
	if (!why.empty()) return fail(nullptr, MTSGPU_EINVAL, "%s", why.c_str());
	return 0;
}
static bool flatSceneHasTexcoords(const mtsgpu_flat_scene *fs) {
	if (!fs) return false;
	for (uint32_t h : fs->fs.shapeHasUv) if (h) return true;
	return false;
}
const float *mtsgpu_flat_scene_vertex_texcoords(const mtsgpu_flat_scene *fs) { return flatSceneHasTexcoords(fs) ? fs->fs.vtxUv.data() : nullptr; }
const uint32_t *mtsgpu_flat_scene_shape_has_texcoords(const mtsgpu_flat_scene *fs) { return flatSceneHasTexcoords(fs) ? fs->fs.shapeHasUv.data() : nullptr; }

int mtsgpu_flat_scene_kdstats(const mtsgpu_flat_scene *fs, double *out6) {
	if (!fs || !out6) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	for (int i = 0; i < 6; ++i) out6[i] = fs->fs.kd.stats[i];
	return 0;
}

int mtsgpu_make_camera(const float origin[3], const float target[3], const float up[3],
                       float fov_deg, int width, int height, mtsgpu_camera *out) {
	if (!origin || !target || !up || !out || width <= 0 || height <= 0) return fail(nullptr, MTSGPU_EINVAL, "bad camera arguments");
	makeCamera(origin, target, up, fov_deg, width, height, *out);
	return 0;
}

int mtsgpu_make_camera_ortho(const float origin[3], const float target[3], const float up[3],
                             float scale_x, float scale_y, int width, int height, mtsgpu_camera *out) {
	if (!origin || !target || !up || !out || width <= 0 || height <= 0 || !(scale_x > 0) || !(scale_y > 0))
		return fail(nullptr, MTSGPU_EINVAL, "bad camera arguments");
	makeCameraOrtho(origin, target, up, scale_x, scale_y, width, height, *out);
	return 0;
}

} // extern "C"
