/*
 * mtsgpu.h -- C ABI of the MI355X path-tracing hot path (libmtsgpu.so).
 *
 * This is the drop-in boundary for Mitsuba 0.2.1's unidirectional path tracer
 * (reference: src/integrators/path/path.cpp:47-216 driven by
 * src/librender/integrator.cpp:131-170).  Everything that crosses it is a plain
 * pointer, a size or a POD struct; no C++/torch types, no exceptions.
 *
 * Two clients bind exactly these entry points:
 *   (1) the Mitsuba integrator plugin `gpupath`, which fills a
 *       mtsgpu_scene from Scene/ShapeKDTree/TriMesh and overrides
 *       Integrator::render() (include/mitsuba/render/integrator.h:57);
 *   (2) the host-side mirror in mitsuba-renderer_amd/ (ctypes), used by tests/ and bench.py.
 *
 * All functions return 0 on success or a negative MTSGPU_E* code;
 * mtsgpu_last_error() gives the text.  One ctx = one GPU = one host thread; a
 * device group (mtsgpu_create_multi, below) drives several ctx -- one per GPU of the node -- from ONE host
 * process and sums their films over xGMI, which is what a Mitsuba process needs
 * (Scene::render calls Integrator::render once, src/librender/scene.cpp:356-359).
 */
#ifndef MTSGPU_H
#define MTSGPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MTSGPU_ABI_VERSION 8

enum {
	MTSGPU_OK = 0,
	MTSGPU_EINVAL = -1,   /* bad argument / inconsistent scene                  */
	MTSGPU_EHIP = -2,     /* a HIP runtime call failed                          */
	MTSGPU_ENODEV = -3,   /* no usable gfx950 device                            */
	MTSGPU_ECANCEL = -4,  /* *cancel became non-zero (Integrator::cancel)       */
	MTSGPU_ESTATE = -5    /* call sequence error (e.g. render before upload)    */
};

/* BSDF plugins on the path (the plugins of src/bsdfs) */
enum {
	MTSGPU_BSDF_LAMBERTIAN = 0, /* params: [0..2] reflectance                                  */
	MTSGPU_BSDF_DIELECTRIC = 1, /* params: [0] intIOR [1] extIOR [2..4] specRefl [5..7] specTrans */
	MTSGPU_BSDF_ROUGHMETAL = 2, /* params: [0] alphaB [1..3] ior [4..6] k [7..9] specRefl        */
	MTSGPU_BSDF_MICROFACET = 3, /* params: [0] alphaB [1] kd [2] ks [3] intIOR [4] extIOR
	                                       [5..7] diffuseRefl [8..10] specRefl                  */
	MTSGPU_BSDF_MIRROR = 4,     /* params: [0..2] specularReflectance            (src/bsdfs/mirror.cpp)      */
	MTSGPU_BSDF_PHONG = 5,      /* params: [0] exponent [1] kd [2] ks [3] specularSamplingWeight
	                                       [4] diffuseSamplingWeight [5..7] diffuseRefl [8..10] specRefl
	                                       (values after Phong::configure, src/bsdfs/phong.cpp:74-96)   */
	MTSGPU_BSDF_ROUGHGLASS = 6, /* params: [0] distribution (0 beckmann, 1 phong, 2 ggx) [1] alpha (phong: the exponent
	                                       2/alpha^2 - 2 the constructor derives, roughglass.cpp:130-136) [2] intIOR
	                                       [3] extIOR [4..6] specularReflectance [7..9] specularTransmittance
	                                       (src/bsdfs/roughglass.cpp)                                              */
	MTSGPU_BSDF_DIFFTRANS = 7,  /* params: [0..2] transmittance                          (src/bsdfs/difftrans.cpp)  */
	MTSGPU_BSDF_WARD = 8,       /* params: [0] model type (0 ward, 1 ward-duer, 2 balanced) [1] alphaX [2] alphaY [3] kd [4] ks
	                                       [5] specularSamplingWeight [6] diffuseSamplingWeight [7..9] diffuseRefl
	                                       [10..12] specRefl (values after Ward::configure, src/bsdfs/ward.cpp:118-136).
	                                       alphaX != alphaY needs a tangent frame: accepted on spheres (dpdu / dpdv,
	                                       sphere.cpp:136-178), refused on triangle meshes, which carry no texture
	                                       coordinates here (as trimesh.cpp:547-556 refuses them)                      */
	MTSGPU_BSDF_COMPOSITE = 9,  /* params: [0] child count n, 1..MTSGPU_COMPOSITE_MAX [1..n] weights (>= 0)
	                                       [1+n..2n] the children's indices into the scene's BSDF table, stored as floats
	                                       (exact below 2^24).  Children are non-delta entries of any other type, each
	                                       with or without MTSGPU_BSDF_TWOSIDED      (src/bsdfs/composite.cpp)         */
	MTSGPU_BSDF_NTYPES = 10,
	/* OR-ed into bsdf_type: the BSDF is wrapped in a `twosided` adapter (src/bsdfs/twosided.cpp) */
	MTSGPU_BSDF_TWOSIDED = 0x100
};
#define MTSGPU_BSDF_NPARAMS 16
#define MTSGPU_COMPOSITE_MAX 7   /* children of a composite: 1 + 2 * 7 of the 16 slots */

/* Luminaire plugins on the path (src/luminaires/{area,constant}.cpp) */
enum {
	MTSGPU_LUM_AREA = 0,     /* params: [0..2] intensity; shape = emitting TriMesh            */
	MTSGPU_LUM_CONSTANT = 1, /* params: [0..2] intensity [3..5] bsphere centre [6] radius      */
	/* delta luminaires (isIntersectable() == false, path.cpp:118-120) */
	MTSGPU_LUM_POINT = 2,    /* params: [0..2] intensity [3..5] position                (src/luminaires/point.cpp) */
	MTSGPU_LUM_DIRECTIONAL = 3, /* [0..2] intensity [3..5] direction (unit) [6] disk radius = scene bsphere radius
	                               (src/luminaires/directional.cpp:65-91)                                        */
	MTSGPU_LUM_SPOT = 4,     /* [0..2] intensity [3..5] position [6] cos(beamWidth) [7] cos(cutoffAngle)
	                            [8] cutoffAngle (rad) [9] 1/(cutoffAngle-beamWidth) [10..18] world->luminaire
	                            3x3 (row major) [19] beamWidth (rad)           (src/luminaires/spot.cpp:33-118) */
	MTSGPU_LUM_COLLIMATED = 6, /* [0..2] intensity [3] radius [4..15] world->luminaire 3x4 (row major, affine)
	                            [16..27] luminaire->world 3x4              (src/luminaires/collimated.cpp) */
	MTSGPU_LUM_SKY = 7,      /* [0] skyScale [1] turbidity [2] clipBelowHorizon (0/1) [3..5] bsphere centre [6] radius = the
	                            scene's bounding sphere x 1.01, no camera expansion (sky.cpp:221-227) [7..15] world->luminaire
	                            3x3 (row major) [16] thetaS [17] phiS [18..22] aConst..eConst: what the object holds after
	                            serialize() and preprocess(); what configure() derives is mtsgpu_sky_configure().  Always
	                            the background luminaire, at most one per scene          (src/luminaires/sky.cpp) */
	MTSGPU_LUM_ENVMAP = 5    /* [0] intensityScale [3..5] bsphere centre [6] radius (envmap.cpp:112-126)
	                            [7..15] world->luminaire 3x3 [16..24] luminaire->world 3x3 (row major); the image and
	                            its sampling density are the env_* arrays of the scene   (src/luminaires/envmap.cpp) */
};
#define MTSGPU_LUM_NPARAMS 32
#define MTSGPU_SKY_NDERIVED 24   /* floats mtsgpu_sky_configure() writes */

/* Sampler kinds.  *_KEYED are the per-(pixel,sample)-keyed forms of the two
 * reference samplers (src/samplers/{independent,ldsampler}.cpp): identical
 * integer code, with Random (MT19937-64) replaced by a keyed SplitMix64 stream
 * so that samples are independent of traversal order. */
enum {
	MTSGPU_SAMPLER_INDEPENDENT_KEYED = 0,
	MTSGPU_SAMPLER_LD_KEYED = 1,
	/* The two purely deterministic QMC samplers (src/samplers/{halton,hammersley}.cpp): no Random involved, so the
	 * sample values are the reference's own, not a keyed variant: sample j of EVERY pixel is
	 * radicalInverse(primeTable[depth], j) (generate() resets the index for each pixel, halton.cpp:58-61).  The
	 * evaluation order inside Point2(nextValue(), nextValue()) (halton.cpp:88) is left to the compiler by the
	 * reference; x first is used here. */
	MTSGPU_SAMPLER_HALTON = 2,
	MTSGPU_SAMPLER_HAMMERSLEY = 3,
	/* src/samplers/stratified.cpp, keyed like the LD sampler: generate() shuffles the per-depth stratum
	 * permutations with the (seed, pixel, 0) stream, the jitter comes from the per-sample stream; sampleCount is
	 * rounded up to a perfect square (stratified.cpp:36-44) */
	MTSGPU_SAMPLER_STRATIFIED_KEYED = 4
};

/* shape_flags bits */
#define MTSGPU_SHAPE_HAS_NORMALS 1u  /* TriMesh has per-vertex normals (faceNormals=false) */

/* Shape plugins.  A TriMesh is expanded into one kd-tree primitive per triangle; every other shape is
 * ONE primitive that the tree only knows by its AABB (ShapeKDTree::addShape, src/librender/skdtree.cpp:43-60);
 * its tri_idx row is {NONE, NONE, NONE} and its TriAccel row has k = MTSGPU_KNOTRIANGLE (skdtree.cpp:92-96). */
enum {
	MTSGPU_SHAPE_TRIMESH = 0,
	MTSGPU_SHAPE_SPHERE = 1   /* src/shapes/sphere.cpp; params: [0..2] m_center [3] m_radius [4] m_inverted (0/1)
	                             [5..13] m_objectToWorld 3x3 (row major, scale removed: sphere.cpp:49-53)
	                             [14..22] m_worldToObject 3x3 [23] m_invSurfaceArea                           */
};
#define MTSGPU_SHAPE_NPARAMS 24
#define MTSGPU_KNOTRIANGLE 0xFFFFFFFFu

/*
 * Flattened scene.  This is what ShapeKDTree + TriMesh + BSDF/Luminaire
 * parameter blocks look like once laid out for HBM (Appendix A of SURVEY.md).
 *
 * Primitive index space = concatenation of the shapes' triangles in
 * ShapeKDTree::m_shapes order (src/librender/skdtree.cpp:43-65).
 */
typedef struct mtsgpu_scene {
	uint32_t abi_version;        /* MTSGPU_ABI_VERSION                                        */

	/* --- geometry (TriMesh storage, include/mitsuba/render/trimesh.h) --- */
	uint32_t n_shapes, n_tris, n_verts;   /* n_tris = number of kd-tree primitives (triangles + other shapes) */
	const float    *vtx_pos;     /* [n_verts][3]                                              */
	const float    *vtx_nrm;     /* [n_verts][3]; rows of shapes without normals are ignored  */
	const uint32_t *tri_idx;     /* [n_tris][3] indices into the global vertex pool           */
	const uint32_t *shape_tri_offset; /* [n_shapes+1] prefix sums (m_shapeMap)               */
	const int32_t  *shape_bsdf;  /* [n_shapes] index into bsdf_* or -1 (not an occluder)      */
	const int32_t  *shape_lum;   /* [n_shapes] index into lum_* or -1                         */
	const uint32_t *shape_flags; /* [n_shapes] MTSGPU_SHAPE_*                                 */
	const uint32_t *shape_type;  /* [n_shapes] MTSGPU_SHAPE_TRIMESH / _SPHERE; NULL = all TriMesh */
	const float    *shape_params;/* [n_shapes][MTSGPU_SHAPE_NPARAMS]; NULL iff shape_type is NULL  */

	/* --- SAH kd-tree (KDNode, include/mitsuba/render/gkdtree.h:442-470) ---
	 * node = 2 x u32: inner {axis | relOffsetToLeft<<2, float split},
	 *                 leaf  {1<<31 | primStart, primEnd}; children adjacent; root = 0 */
	uint32_t n_nodes, n_indices;
	const uint32_t *kd_nodes;    /* [n_nodes][2]                                              */
	const uint32_t *kd_indices;  /* [n_indices] primitive ids                                 */
	/* TriAccel, 12 x 4 B per primitive (include/mitsuba/render/triaccel.h:34-48) */
	const uint32_t *triaccel;    /* [n_tris][12]                                              */
	float aabb_min[3], aabb_max[3]; /* enlarged kd-tree AABB (gkdtree.h:1170-1176)          */

	/* --- BSDF parameter blocks --- */
	uint32_t n_bsdfs;
	const uint32_t *bsdf_type;   /* [n_bsdfs]                                                 */
	const float    *bsdf_params; /* [n_bsdfs][MTSGPU_BSDF_NPARAMS]                            */

	/* --- luminaires (Scene::m_luminaires order) --- */
	uint32_t n_lums;
	const uint32_t *lum_type;    /* [n_lums]                                                  */
	const float    *lum_params;  /* [n_lums][MTSGPU_LUM_NPARAMS]                              */
	const int32_t  *lum_shape;   /* [n_lums] emitting shape or -1                             */
	const float    *lum_inv_area;/* [n_lums] TriMesh::m_invSurfaceArea (trimesh.cpp:283)      */
	const uint32_t *lum_cdf_offset; /* [n_lums+1] into lum_tri_cdf; area: nTris+1 entries    */
	const float    *lum_tri_cdf; /* per-emitter triangle area CDFs (trimesh.cpp:279-283)      */
	const float    *lum_sel_cdf; /* [n_lums+1] Scene::m_luminairePDF cdf (scene.cpp:320-330)  */
	const float    *lum_sel_pdf; /* [n_lums]                                                  */
	float lum_sel_sum;           /* DiscretePDF::getOriginalSum()                             */
	int32_t background_lum;      /* index of the background luminaire or -1                   */

	/* --- the environment map of the MTSGPU_LUM_ENVMAP luminaire (at most one per scene) ---
	 * level 0 of MIPMap::fromBitmap (src/librender/mipmap.cpp:30-92,161-181: powers of two, ERepeat) and the
	 * DiscretePDF over level min(3, levels-1) that EnvMapLuminaire::configure builds (envmap.cpp:95-110) */
	uint32_t env_width, env_height;
	const float *env_pixels;     /* [env_height][env_width][3] linear RGB                     */
	uint32_t env_pdf_width, env_pdf_height;
	const float *env_pdf;        /* [w*h]   DiscretePDF::m_pdf after build()                  */
	const float *env_cdf;        /* [w*h+1] DiscretePDF::m_cdf                                */
} mtsgpu_scene;

/* PerspectiveCameraImpl state (src/cameras/perspective.cpp:43-112) */
typedef struct mtsgpu_camera {
	float raster_to_camera[16]; /* row-major 4x4, m_rasterToCamera                            */
	float camera_to_world[16];  /* row-major 4x4, m_cameraToWorld                             */
	float near_clip, far_clip;  /* camera.cpp:121-123                                         */
	int32_t width, height;      /* size of the rendered film = the crop window's size (Film::getCropSize,
	                               film.cpp:38-41); raster_to_camera maps ITS pixel coordinates            */
	float aperture_radius;      /* thin lens (perspective.cpp:90-103); 0 = pinhole            */
	float focus_depth;          /* camera.cpp:164                                             */
	int32_t kind;               /* 0 = perspective (src/cameras/perspective.cpp), 1 = orthographic
	                               (src/cameras/orthographic.cpp:104-118: origin = rasterToCamera(sample), d = +z,
	                               mint = 0, maxt = far - near; no lens sample)               */
	/* Film crop window (film.cpp:33-41: cropOffsetX/Y, cropWidth/Height inside a film_width x film_height film).
	 * The camera's raster space is that of the FULL film (perspective.cpp:52-63 scales NDC by m_film->getSize());
	 * the work units cover the crop window only and carry its offset (renderproc.cpp:146-154, imageproc.cpp:28-52:
	 * rect.setOffset(pos + m_offset)), so camera samples are generated at raster positions crop_offset +
	 * [0, width) x [0, height), and the film stores pixel (x, y) of the crop window at [y][x] (mfilm.cpp:118-143).
	 * Sampler keys are derived from the full-film pixel position: a cropped render equals the corresponding rectangle
	 * of the full render bit for bit.  film_width / film_height == 0 means no crop (film size = width x height). */
	int32_t crop_offset_x, crop_offset_y;
	int32_t film_width, film_height;
} mtsgpu_camera;

/* Per-kernel-class counters/timings of the last render (measurement, section 8d) */
typedef struct mtsgpu_stats {
	uint64_t camera_samples;
	uint64_t rays_closest, rays_shadow;
	/* algorithmic work of the traversal kernels (only filled when counting is on) */
	uint64_t n_inner, n_leaf, n_idx, n_tri_tested;
	uint64_t trace_launches;
	double trace_ms;     /* sum of HIP-event durations of all traversal launches        */
	double shade_ms;     /* shade / generate / accumulate kernels                       */
	double total_ms;     /* first launch -> last kernel end (device events)             */
	/* the `avgPathLength` statistic of the path tracer (path.cpp:24, :212-213: avgPathLength.incrementBase() per
	 * Li() call, += rRec.depth at its end): sum of the final depths; the average is path_length_sum / camera_samples */
	uint64_t path_length_sum;
	/* closest-hit launches repeated with static ray dealing because a material-queue segment overflowed */
	uint64_t bin_overflow_retries;
	/* time during which at least one traversal launch was running (device-driven bounces trace the shadow rays of a bounce
	 * next to the closest-hit launch of the following one: trace_ms then counts that time twice) */
	double trace_union_ms;
	/* vector-memory requests the traversal kernels ISSUED (lane level; only filled when counting is on): 16-byte sibling
	 * pairs fetched from global memory / served by the LDS copy of the top of the tree, single 8-byte nodes (two per pop)
	 * from global memory / from the LDS copy, 16-byte tails of leaf records (two per primitive whose plane distance lies
	 * inside the ray's interval), stack words spilled to HBM, 16-byte record heads (n_idx plus the heads fetched again when
	 * an interrupted leaf is resumed).  Ray and hit: 3 per ray. */
	uint64_t req_pair_global, req_pair_lds, req_node_global, req_node_lds, req_tail, req_spill, req_head;
	/* parts of trace_ms: the closest-hit launch of the first bounce of every pass (camera rays), and all any-hit launches;
	 * the remaining closest-hit launches are trace_ms - trace_first_ms - trace_shadow_ms */
	double trace_first_ms, trace_shadow_ms;
} mtsgpu_stats;

typedef struct mtsgpu_ctx mtsgpu_ctx;

/* --- lifecycle ----------------------------------------------------------- */
int  mtsgpu_create(int device, mtsgpu_ctx **out);
void mtsgpu_destroy(mtsgpu_ctx *ctx);
const char *mtsgpu_last_error(const mtsgpu_ctx *ctx); /* ctx may be NULL: global */
int  mtsgpu_abi_version(void);
/* first 16 hex digits of the sha256 of the library's sources, stamped in at build time (csrc/stamp.cpp): lets a
 * build script tell a stale binary from a current one */
const char *mtsgpu_source_hash(void);
/* sizeof() of the ABI structs as compiled into the library: 0 scene, 1 camera, 2 stats, 3 mesh,
 * 4 scene_desc, 5 kd_params (bindings check their own layout against these) */
size_t mtsgpu_abi_sizeof(int which);

/* Use a caller-owned HIP stream (hipStream_t passed as void*); NULL = own stream */
int  mtsgpu_set_stream(mtsgpu_ctx *ctx, void *hip_stream);

/* --- scene / integrator state (replaces Scene::initialize + plugin configure) */
int  mtsgpu_upload_scene(mtsgpu_ctx *ctx, const mtsgpu_scene *scene);
/* mtsgpu_upload_scene plus the vertex tangents of the meshes whose BSDF is anisotropic (TriMesh::computeTangentSpaceBasis,
 * trimesh.cpp:547-669; mtsgpu_flatten_tangents computes them): vtx_dpdu [n_verts][3] follows the scene's global vertex pool
 * (rows of shapes without tangents are ignored), shape_has_tangents [n_shapes] is non-zero for the meshes that carry them;
 * both may be NULL.  A hit on such a mesh gets the shading frame of skdtree.h:392-399 instead of Frame(n):
 *   dpdu = (t0.dpdu * b.x + t1.dpdu * b.y) + t2.dpdu * b.z;  n = normalize(interpolated normal);
 *   s = normalize(dpdu - n * dot(n, dpdu));  t = cross(n, s)
 * in binary32.  Every other shape keeps its frame, and a scene without a tangent mesh launches the kernels it launches after
 * mtsgpu_upload_scene.  A mesh with an anisotropic BSDF is accepted with tangents; without them it is accepted when it has no
 * vertex normals (the reference warns and renders it with the frame it has, trimesh.cpp:562-565) and refused otherwise, with
 * the reference's message.  MTSGPU_EINVAL also for tangents on a shape that is no mesh or has no vertex normals, and for a
 * non-finite tangent.  Costs 48 bytes per primitive on the device.  mtsgpu_set_vertex_colors and
 * mtsgpu_set_uv_textures work after either upload. */
int  mtsgpu_upload_scene_tangents(mtsgpu_ctx *ctx, const mtsgpu_scene *scene, const float *vtx_dpdu, const uint32_t *shape_has_tangents);
int  mtsgpu_set_camera(mtsgpu_ctx *ctx, const mtsgpu_camera *cam);
/* MonteCarloIntegrator properties (src/librender/integrator.cpp:272-292) */
int  mtsgpu_set_integrator(mtsgpu_ctx *ctx, int max_depth, int rr_depth, int strict_normals);
/* Switches to the `direct` integrator plugin (MIDirectIntegrator, src/integrators/direct/direct.cpp:33-56):
 * luminaireSamples, bsdfSamples >= 0 with a positive sum.  Counts above one draw from Sampler::next2DArray
 * (direct.cpp:58-63,122-127,156-161), which the independent, ldsampler and stratified samplers provide; with halton /
 * hammersley the render call fails as the reference does (halton.cpp:102-104).  sampleCount x count <= 65536.
 * mtsgpu_set_integrator() switches back to `path`. */
int  mtsgpu_set_direct_integrator(mtsgpu_ctx *ctx, int luminaire_samples, int bsdf_samples);
/* Sampler (src/samplers/{independent,ldsampler}.cpp): kind, sampleCount (LD: rounded up to pow2), LD depth, seed */
int  mtsgpu_set_sampler(mtsgpu_ctx *ctx, int kind, uint32_t spp, int ld_depth, uint64_t seed);
/* ImageBlock sharding (src/librender/imageproc.cpp:43-78): this ctx renders the tiles (tx, ty) of the
 * block_size^2 grid with morton(tx, ty) % n_parts == part (bits of tx and ty interleaved, tx lowest): with 8 parts
 * every 4 x 2 group of tiles holds one tile of each part, so the parts sample the image on a 2-D lattice and their
 * loads stay balanced whatever the picture shows.  The reference's own order (a spiral from the
 * centre) only serves the preview. */
int  mtsgpu_set_tiles(mtsgpu_ctx *ctx, int block_size, int part, int n_parts);
/* Reconstruction filter of the film as a TabulatedFilter (src/librender/rfilter.cpp:40-69,
 * include/mitsuba/render/rfilter.h:65-102): half extents and the 16x16 table Film::getTabulatedFilter()
 * holds.  values == NULL selects the box filter (src/rfilters/box.cpp).  Filters wider than half a
 * pixel make every ImageBlock carry a border of ceil(size - 0.5) pixels (renderproc.cpp:143-144). */
int  mtsgpu_set_rfilter(mtsgpu_ctx *ctx, float size_x, float size_y, const float *values);
/* Film property `highQualityEdges` (src/librender/film.cpp:51): the rendered rectangle grows by the filter
 * border on every side (renderproc.cpp:146-153), so pixels at the film's edge receive their full filter
 * support; the extra samples only land in block borders and are clipped by Film::putImageBlock. */
int  mtsgpu_set_film_edges(mtsgpu_ctx *ctx, int high_quality_edges);
/* Optional: render into a caller-owned device buffer [H][W][5] f32 (spec rgb, alpha, weight) */
int  mtsgpu_set_film_buffer(mtsgpu_ctx *ctx, void *device_ptr);
/* Tuning knobs (0 = default): paths in flight per pass; enable traversal counters */
int  mtsgpu_set_options(mtsgpu_ctx *ctx, uint64_t max_paths, int count_traversal, int time_kernels);

/* Scheduling knobs of the traversal kernel, for experiments and tests (none of them changes a result):
 *   refill_min / desc_min / leaf_min (1..64)  lane thresholds of k_trace
 *   batch (1..64, 0 = rule)                   rays per wave and batch
 *   dyn_div (0 = 4)                           1/dyn_div of a large launch's rounds are claimed dynamically
 *   sync_free (-1 rule, 0 off, 1 on)          bounce loop without host round trips (device-side counts); the rule
 *                                             turns it on for passes of at most 8 Mi paths
 *   chunk (1..1024, default 8)                bounces enqueued between two looks at the queue size (sync_free)
 *   test_retry (0/1)                          treat every first closest-hit launch as overflowed (exercises the retry)
 *   stats_wave (-1 rule, 0 lane, 1 wave)      form of the variance kernel of the test-case mode (below)
 *   miss_shaded (0/1, default 0)              1: a ray that leaves a scene without a background luminaire goes through the
 *                                             terminal queue and the shading kernel; 0: its path ends in the traversal kernel
 *   lean_closest (0..7, default 3)            which closest-hit launches of host-driven frames run the kernel without the mailbox
 *                                             (8 waves per SIMD; rays on which two primitives tie in t are traced again with the
 *                                             mailbox): 1 the incoherent launches of at least plain_below rays, 2 the coherent
 *                                             first launch, 4 the launches below plain_below */
int  mtsgpu_set_tuning(mtsgpu_ctx *ctx, const char *key, long value);

/* --- per-vertex colours and the `vertexcolors` texture (src/textures/vertexcolors.cpp: getValue(its) = its.color) -----
 * A TriMesh may carry one Spectrum per vertex (trimesh.h:121-126); fillIntersectionRecord interpolates them with the hit's
 * barycentrics in binary32, in the reference's operation order (skdtree.h:364,417-421):
 *     b = ((1 - u) - v, u, v);   its.color = (c0 * b.x + c1 * b.y) + c2 * b.z   per channel.
 * A `vertexcolors` texture in a texture-typed spectrum slot of a BSDF makes that slot take its.color instead of the three
 * floats of the parameter block.  The slots of each type, in slot order (bit s of a mask = slot s):
 *     lambertian  0 reflectance                       dielectric  0 specularReflectance  1 specularTransmittance
 *     roughmetal  0 specularReflectance               microfacet  0 diffuseReflectance   1 specularReflectance
 *     mirror      0 specularReflectance               phong       0 diffuseReflectance   1 specularReflectance
 *     roughglass  0 specularReflectance  1 specularTransmittance
 *     difftrans   0 transmittance                     ward        0 diffuseReflectance   1 specularReflectance
 * Roughmetal's ior and k and roughglass's alpha are not slots (plain properties / a float texture); MTSGPU_BSDF_TWOSIDED
 * does not change the meaning of a slot; a composite has no slot of its own and its children must not use one.  The three
 * floats of a coloured slot in the block should hold 1, the texture's getAverage() / getMaximum() (vertexcolors.cpp:49-55),
 * which is what Phong::configure and Ward::configure derive their sampling weights from.
 *
 * vtx_col [n_verts][3] follows the scene's global vertex pool (rows of shapes without colours are ignored),
 * shape_has_colors [n_shapes] is non-zero for the meshes that carry colours, bsdf_color_slots [n_bsdfs] holds the masks
 * (NULL = all zero).  Call after mtsgpu_upload_scene; a new upload clears it; all three NULL switch it off.  Scenes
 * without a coloured slot launch the kernels they launch without this call.  MTSGPU_EINVAL, with the scene's colours
 * switched off, when a mask names a slot beyond those of its type, a composite child has a coloured slot, a shape whose
 * BSDF has a coloured slot is a sphere or a mesh without colours (the reference would read an its.color nobody wrote,
 * shape.h:162-163), or a colour of a mesh that has them is not finite. */
int  mtsgpu_set_vertex_colors(mtsgpu_ctx *ctx, const float *vtx_col, const uint32_t *shape_has_colors, const uint32_t *bsdf_color_slots);

/* --- texture coordinates and the procedural uv textures `checkerboard` and `gridtexture` ------------------------------------
 * Both answer usesRayDifferentials() == false and forward the filtered getValue to the plain one (checkerboard.cpp:48-64,
 * gridtexture.cpp:51-73), so they need its.uv and nothing else.  All of it in binary32, in the reference's operation order:
 *   its.uv, triangle mesh (skdtree.h:364,408-415):  b = ((1 - u) - v, u, v);  its.uv = (t0 * b.x + t1 * b.y) + t2 * b.z per
 *     component; a mesh without texcoords gives (0, 0)
 *   its.uv, sphere (sphere.cpp:136-145):  local = worldToObject(p - center);  theta = acos(clamp(local.z / radius));
 *     phi = atan2(local.y, local.x), + 2 pi if negative;  its.uv = (phi * (0.5f * INV_PI), theta * INV_PI)
 *   Texture2D::getValue(its) (texture.cpp:73-82):  uv' = (uv.x * uscale, uv.y * vscale) + (uoffset, voffset)
 *   checkerboard:  x = 2 * modulo((int) (uv'.x * 2), 2) - 1, y likewise;  bright iff x * y == 1.  The cast truncates towards
 *     zero (the cell around 0 is twice as wide); modulo is the non-negative remainder
 *   gridtexture:   x = uv'.x - (int) uv'.x;  if (x > .5) x -= 1;  y likewise;  dark iff |x| < lineWidth || |y| < lineWidth
 * A slot is one of the texture-typed spectrum slots listed above for the vertex colours.  The three floats of a textured slot
 * in the block should hold the texture's getAverage(), which is what Phong::configure and Ward::configure derive their sampling
 * weights from: dark * 0.5f for the checkerboard (sic, checkerboard.cpp:66-68), bright for the grid (gridtexture.cpp:79-81). */
enum { MTSGPU_TEX_CHECKERBOARD = 0, MTSGPU_TEX_GRID = 1, MTSGPU_TEX_NKINDS = 2 };
typedef struct mtsgpu_uv_texture {
	uint32_t kind;                           /* MTSGPU_TEX_*                                              */
	float uoffset, voffset, uscale, vscale;  /* Texture2D: defaults 0, 0, 1, 1                            */
	float bright[3], dark[3];                /* brightColor (default .4), darkColor (default .2)          */
	float line_width;                        /* gridtexture's lineWidth (default .01); ignored otherwise  */
} mtsgpu_uv_texture;
/* vtx_uv [n_verts][2] follows the scene's global vertex pool (rows of shapes without texcoords are ignored), shape_has_uv
 * [n_shapes] is non-zero for the meshes that carry texcoords (both may be NULL: no mesh has any), textures [n_textures],
 * bsdf_slot_texture [n_bsdfs][2] an index into textures per slot or -1.  Call after mtsgpu_upload_scene; a new upload clears
 * it; everything NULL switches it off.  Scenes without a textured slot launch the kernels they launch without this call; a
 * scene may colour one slot (mtsgpu_set_vertex_colors) and texture another, in either order of the two calls.
 * MTSGPU_EINVAL, with the scene's textures switched off, when a slot lies beyond those of its type, a slot also has its
 * colour bit set (mtsgpu_set_vertex_colors refuses the same from its side), a composite child has a textured slot, a kind is
 * unknown, a parameter or a texcoord of a mesh that has them is not finite, or, for a texture some slot uses and a shape
 * whose BSDF has that slot, 2 * uv' reaches 2^31 - 2^16 in magnitude at a vertex (on a sphere: at uv = 0 or 1) -- the
 * reference's (int) cast is undefined from 2^31 on, and the margin covers the rounding of the interpolation.
 * Spheres are accepted.  A mesh without texcoords whose BSDF has a textured slot is ACCEPTED and shaded with uv = (0, 0):
 * that is the value the reference's Intersection carries there (skdtree.h:413-415), unlike its.color it is always written. */
int  mtsgpu_set_uv_textures(mtsgpu_ctx *ctx, const float *vtx_uv, const uint32_t *shape_has_uv, uint32_t n_textures,
                            const mtsgpu_uv_texture *textures, const int32_t *bsdf_slot_texture);

/* --- unfiltered bitmap textures: `ldrtexture` with filterType = "none" --------------------------------------------------------
 * With that filter type the MIPMap has one level and nothing is resampled, so the bitmap may have any size, and
 * Texture2D::getValue(its) returns the same texel with or without uv partials (mipmap.cpp:228-231 and :296-299 are one
 * expression): its.uv is all the lookup needs.  In binary32, integer after the two floors:
 *   uv' as above;  xPos = (int) floorf(uv'.x * (float) width), yPos likewise with height            (mipmap.cpp:229-231)
 *   MIPMap::getTexel (mipmap.cpp:203-225) AS WRITTEN: if (xPos <= 0 || yPos < 0 || xPos >= width || yPos >= height) the wrap
 *     mode applies -- repeat: modulo(., size), the non-negative remainder (util.cpp:424-427); clamp: to [0, size - 1]; black:
 *     return 0; white: return 1.  Column 0 therefore counts as out of range (sic): harmless under repeat and clamp, but under
 *     black and white every lookup in column 0 returns the constant
 *   the texel is texels[yPos][xPos]
 * The filtered modes (trilinear, ewa: ray differentials, the pyramid) are not served.  The three floats of a slot with a bitmap
 * should hold getAverage() = triangle(levels - 1, 0, 0) = that lookup at uv' = (0, 0): texel (0, 0) under repeat and clamp, 0
 * under black, 1 under white; verifyEnergyConservation reads getMaximum(), the per-channel maximum over the texels, at least 1
 * under white (mipmap.cpp:137-154).
 * MTSGPU_TEX_BITMAP is a kind of mtsgpu_uv_texture that only the calls below take: kind and the four Texture2D floats count,
 * the other seven words are ignored (the library keeps width, height, wrap mode and the pool index there). */
enum { MTSGPU_TEX_BITMAP = 2 };
/* the four modes of MIPMap::EWrapMode in the order of getTexel's switch -- not the enum's own numbering (mipmap.h:32-37: repeat,
 * black, white, clamp), which integration/streamparse.h translates */
enum { MTSGPU_WRAP_REPEAT = 0, MTSGPU_WRAP_CLAMP = 1, MTSGPU_WRAP_BLACK = 2, MTSGPU_WRAP_WHITE = 3 };
typedef struct mtsgpu_bitmap {
	uint32_t width, height;
	uint32_t wrap_mode;                      /* MTSGPU_WRAP_*                                             */
	uint32_t reserved;                       /* 0                                                         */
	const float *texels;                     /* [height][width][3] linear RGB: what m_pyramid[0] holds    */
} mtsgpu_bitmap;
/* The texels of all bitmaps of one call together number at most MTSGPU_BITMAP_MAX_TEXELS: the device indexes the pool with
 * one uint32 and a dimension is an int in the reference.  The pool costs 16 bytes per texel in HBM. */
#define MTSGPU_BITMAP_MAX_TEXELS 2147483647u
/* mtsgpu_set_uv_textures with bitmaps: a superset of that call, as mtsgpu_upload_scene_tangents is of the upload.  bitmaps
 * [n_bitmaps]; texture_bitmap [n_textures] names the bitmap of each texture of kind MTSGPU_TEX_BITMAP (several may share one;
 * ignored for the other kinds; may be NULL when no texture is a bitmap).  Same ownership: either call replaces what the other
 * one set, everything NULL switches textures off.  With n_bitmaps = 0 it does what mtsgpu_set_uv_textures does.  The same
 * checks, and MTSGPU_EINVAL as well, naming the index, for a bitmap with a zero dimension, an unknown wrap mode, a non-zero
 * reserved word, no texels, or a texel that is negative or not finite (clampNegative has run in the reference,
 * mipmap.cpp:169); more than MTSGPU_BITMAP_MAX_TEXELS texels in all; a bitmap texture whose texture_bitmap entry is out of
 * range; and, for a bitmap texture some slot uses and a shape whose BSDF has that slot, uv' * width or uv' * height reaching
 * 2^31 - 2^16 in magnitude at a vertex (on a sphere: at uv = 0 or 1), the range of the (int) cast with the margin of
 * mtsgpu_set_uv_textures. */
int  mtsgpu_set_uv_bitmap_textures(mtsgpu_ctx *ctx, const float *vtx_uv, const uint32_t *shape_has_uv, uint32_t n_textures,
                                   const mtsgpu_uv_texture *textures, const int32_t *bsdf_slot_texture, uint32_t n_bitmaps,
                                   const mtsgpu_bitmap *bitmaps, const int32_t *texture_bitmap);
/* The mask BSDF (src/bsdfs/mask.cpp) -- its side table and the call that hands it over, a superset of the call above -- is an
 * extension of this ABI with a header of its own, mtsgpu_mask.h: the list of entry points declared here is part of ABI version 8.
 * Likewise the snow BRDFs (src/bsdfs/wiscombe.cpp, hanrahan-krueger.cpp), a side table on Lambertian entries: mtsgpu_snow.h;
 * and the woven-cloth BRDF (src/bsdfs/irawan.cpp), a weave pool and a side table on Lambertian entries: mtsgpu_cloth.h. */
/* LDRTexture::initializeFrom (ldrtexture.cpp:116-202) and MIPMap::fromBitmap (mipmap.cpp:156-177) on the host: the decoded
 * file's bytes -> the texels an mtsgpu_bitmap takes.  data: height rows of width pixels of bpp bits -- 32 (r g b a), 24 (r g b),
 * 16 (luminance a), 8 (luminance), 1 (bit pos % 8 of byte pos / 8, pos counting pixels without row padding; set = 255).  The
 * 256-entry table: gamma == -1 is sRGB (v <= 0.04045 ? v / 12.92 : powf((v + 0.055) / 1.055, 2.4) at v = i / 255), anything else
 * powf(i / 255, gamma), in binary32 as the reference computes it on its host.  Alpha is dropped, fromLinearRGB is the identity
 * of an RGB build, clampNegative is applied.  out [height][width][3].  No context: errors go to mtsgpu_last_error(NULL).
 * MTSGPU_EINVAL for a null argument, a zero dimension, and any other bit depth ("%i bpp images are currently not
 * supported!", the reference's message). */
int  mtsgpu_ldr_texels(int bpp, uint32_t width, uint32_t height, const uint8_t *data, float gamma, float *out);

/* --- the hot path (replaces SampleIntegrator::render, integrator.cpp:87-120) */
int  mtsgpu_render(mtsgpu_ctx *ctx, volatile const int *cancel);
int  mtsgpu_sync(mtsgpu_ctx *ctx);
/* Film::putImageBlock sums: host copy of [H][W][5] f32 */
int  mtsgpu_read_film(mtsgpu_ctx *ctx, float *rgbaw);
int  mtsgpu_clear_film(mtsgpu_ctx *ctx);
int  mtsgpu_get_stats(mtsgpu_ctx *ctx, mtsgpu_stats *out);

/* --- test-case mode (`mitsuba -t`): per-pixel variance next to the film ---------------------------------------
 * What an ImageBlock with statistics collects (renderproc.cpp:44-50): SampleIntegrator::renderBlock runs Knuth's online
 * recurrence over the Li values of a pixel's sampleCount camera samples, in sample order, in binary32 per channel
 * (integrator.cpp:171-202):
 *     delta = spec - mean;  mean += delta * (1 / (float) (j + 1));  msq += delta * (spec - mean)
 * over EVERY sample -- also one ImageBlock::putSample rejects as invalid -- and keeps the last setVariance of a pixel:
 *     variance = msq * (1 / (float) (sampleCount - 1)),  nSamples = sampleCount.
 * With sampleCount == 1 that reciprocal is +inf and the stored variance is 0 * inf = NaN, as in the reference.  Pixels
 * this context does not render (tiles of other parts) keep variance 0, nSamples 0.  The film sums do not change.
 * The reference collects statistics with the box filter only (renderjob.cpp:96-99, mfilm.cpp:145): mtsgpu_render with
 * the mode on and a wider filter fails with MTSGPU_EINVAL and leaves the context usable.  mtsgpu_clear_film clears the
 * statistics too.  MFilm::develop's .m file and TestSupervisor::analyze's t-test live in the Python package (testmode.py).
 * Tuning key `stats_wave` (-1 rule, 0 one lane per pixel, 1 one wave per pixel) picks the form of the variance kernel. */
int  mtsgpu_set_film_statistics(mtsgpu_ctx *ctx, int on);
/* host copies of the variance [H][W][3] f32 and the sample counts [H][W] u32 (crop-window coordinates, like the film);
 * MTSGPU_ESTATE while the mode is off */
int  mtsgpu_read_film_statistics(mtsgpu_ctx *ctx, float *var3, uint32_t *nsamp);
/* which form of the variance kernel the last pass of the last mtsgpu_render ran: 0 lane per pixel, 1 wave per pixel,
 * -1 none (mode off, nothing rendered) */
int  mtsgpu_film_statistics_form(const mtsgpu_ctx *ctx);

/* --- several GPUs in one process -------------------------------------------------------------------------
 * A group owns one ctx per entry of devs[] (entries may repeat: two ctx on one GPU is how the single-GPU test box
 * exercises this path).  Configuration goes to every member through mtsgpu_group_ctx(g, i) with the ordinary
 * calls, or to all of them at once with the mtsgpu_group_* helpers; mtsgpu_group_render() then
 *   1. gives member i the tiles of part i of n (mtsgpu_set_tiles) and clears its film,
 *   2. renders all members concurrently, one host thread per member (SampleIntegrator::render, integrator.cpp:87-120,
 *      with the GPUs in the role of the scheduler's workers),
 *   3. sums the films into member 0's film (BlockedRenderProcess::processResult -> Film::putImageBlock,
 *      src/librender/renderproc.cpp:123-130, src/films/mfilm.cpp:118-143): ONE ncclReduce(sum, f32, W*H*5, root 0)
 *      over RCCL/xGMI when the devices are distinct and librccl can be loaded, otherwise -- and always when
 *      `ordered_reduce` is set -- peer copies into a staging buffer on device 0 added in member order 1, 2, ...,
 *      which makes the film independent of the collective's internal order for filters wider than a pixel.
 * mtsgpu_read_film(mtsgpu_group_ctx(g, 0)) returns the merged film.  The group call is blocking and must not be
 * entered concurrently; cancel is polled by every member. */
typedef struct mtsgpu_group mtsgpu_group;
int  mtsgpu_create_multi(int ndev, const int *devs, mtsgpu_group **out);
void mtsgpu_group_destroy(mtsgpu_group *g);
int  mtsgpu_group_size(const mtsgpu_group *g);
mtsgpu_ctx *mtsgpu_group_ctx(mtsgpu_group *g, int i);
const char *mtsgpu_group_last_error(const mtsgpu_group *g);
/* the same call on every member (scene upload runs on all devices concurrently) */
int  mtsgpu_group_upload_scene(mtsgpu_group *g, const mtsgpu_scene *scene);
/* mtsgpu_upload_scene_tangents on every member */
int  mtsgpu_group_upload_scene_tangents(mtsgpu_group *g, const mtsgpu_scene *scene, const float *vtx_dpdu, const uint32_t *shape_has_tangents);
int  mtsgpu_group_set_camera(mtsgpu_group *g, const mtsgpu_camera *cam);
int  mtsgpu_group_set_integrator(mtsgpu_group *g, int max_depth, int rr_depth, int strict_normals);
int  mtsgpu_group_set_sampler(mtsgpu_group *g, int kind, uint32_t spp, int ld_depth, uint64_t seed);
int  mtsgpu_group_set_rfilter(mtsgpu_group *g, float size_x, float size_y, const float *values);
/* block_size as in mtsgpu_set_tiles; ordered_reduce: 0 = RCCL when possible, 1 = always the ordered peer-copy sum,
 * 2 = fail when RCCL cannot be initialised and run the collective also for a single member (self-test of the
 * collective path on a one-GPU machine) */
int  mtsgpu_group_render(mtsgpu_group *g, int block_size, int ordered_reduce, volatile const int *cancel);
/* 0 = ordered peer-copy sum, 1 = RCCL ncclReduce: what the last mtsgpu_group_render used */
int  mtsgpu_group_last_reduce_kind(const mtsgpu_group *g);
/* The number of ranks of the group's RCCL communicator, once it exists and has passed its self-check (created by the first
 * mtsgpu_group_render that wants the collective: ncclCommInitAll gave every member a communicator, each reports the group's
 * size, and a one-float sum of ones arrived at the root as that size); 0 before that, when RCCL is not usable, or after a
 * collective failed and the group went back to the ordered sum. */
int  mtsgpu_group_rccl_ranks(const mtsgpu_group *g);
/* Why the last mtsgpu_group_render summed the films in member order although RCCL was asked for ("" when it did not have
 * to): librccl could not be loaded (the environment variable MTSGPU_RCCL_LIB names the library to load), the
 * communicator could not be created, or ncclReduce / ncclGroupEnd failed.  A failed collective does not lose the frame:
 * its result is received in a staging buffer, the members' films stay as rendered, the group stops using RCCL and adds
 * the films up in member order. */
const char *mtsgpu_group_reduce_note(const mtsgpu_group *g);
/* mtsgpu_set_tuning on every member.  One key belongs to the group itself and exists for tests: "rccl_fail" != 0 makes
 * the next collectives report a failure, which exercises the fall-back to the ordered sum. */
int  mtsgpu_group_set_tuning(mtsgpu_group *g, const char *key, long value);
/* mtsgpu_set_film_statistics on every member.  With the box filter every pixel belongs to exactly one member: after
 * mtsgpu_group_render member 0 holds the statistics of all members, copied pixel by pixel in member order (peer copies
 * like the ordered film sum; the u32 counts never pass through the f32 collective, and the film reduce is unchanged);
 * mtsgpu_read_film_statistics(mtsgpu_group_ctx(g, 0)) returns them. */
int  mtsgpu_group_set_film_statistics(mtsgpu_group *g, int on);
/* mtsgpu_set_vertex_colors on every member */
int  mtsgpu_group_set_vertex_colors(mtsgpu_group *g, const float *vtx_col, const uint32_t *shape_has_colors, const uint32_t *bsdf_color_slots);
/* mtsgpu_set_uv_textures on every member */
int  mtsgpu_group_set_uv_textures(mtsgpu_group *g, const float *vtx_uv, const uint32_t *shape_has_uv, uint32_t n_textures,
                                  const mtsgpu_uv_texture *textures, const int32_t *bsdf_slot_texture);

/* mtsgpu_set_uv_bitmap_textures on every member */
int  mtsgpu_group_set_uv_bitmap_textures(mtsgpu_group *g, const float *vtx_uv, const uint32_t *shape_has_uv, uint32_t n_textures,
                                         const mtsgpu_uv_texture *textures, const int32_t *bsdf_slot_texture, uint32_t n_bitmaps,
                                         const mtsgpu_bitmap *bitmaps, const int32_t *texture_bitmap);

/* HBM triad a[i] = b[i] + s * c[i] over three arrays of `bytes` each on `device` (float4 lanes, best of `iters`
 * launches): the practical bandwidth roof next to the 8 TB/s specification.  GB/s in *gbs. */
int  mtsgpu_hbm_triad(int device, size_t bytes, int iters, double *gbs);

/* Vector-memory request roof: lane-level 16-byte loads per second when every lane of every wave gathers its own random
 * element from `footprint_bytes` (a power of two; 4 MiB sits in the L2 like the upper kd-tree), with k_trace's grid
 * shape.  The traversal kernel is bound by this rate, not by DRAM bytes. */
int  mtsgpu_gather_roof(int device, size_t footprint_bytes, double *lane_requests_per_s);
/* Measurement: a traversal kernel against a replay of its own request stream.  A sample of n rays of the frame rendered
 * last is traced once with the counting kernel, which records every vector-memory request of every ray (which sibling
 * pair, node, leaf-record chunk; not recorded: what the kernel streams in and out in queue order -- queue ids, rays,
 * the ids and hits appended to the material bins -- stack words spilled to HBM, and the two extra chunks of a sphere
 * primitive); then (a) the product kernel of
 * that class and (b) a kernel that re-issues exactly those requests are timed: per ray in the recorded order, one 16-byte
 * load per request from the line the traversal asked for, eight independent requests in flight per lane, the grid shape
 * and LDS footprint of the closest-hit kernel, NO arithmetic, no stack, no mailbox, no dependence between the requests.
 * (b) is ONE throughput test of the memory system on this set of lines, not a bound: other issue orders may be faster.
 * kind selects the sample and the product kernel:
 *   0  every stride-th of the first n * stride path records -- after mtsgpu_render() each holds the LAST ray of its
 *      path; the rays are copied into queue order first -- with the closest-hit kernel as the bounces launch it
 *      (material binning on);
 *   1  the camera rays of the pass rendered last, generated again (the path records are overwritten), every stride-th,
 *      with the closest-hit kernel in the plain 64-ray batches of a first bounce;
 *   2  every stride-th slot of the shadow queue as the frame left it (slot i holds the ray of the deepest bounce that
 *      queued more than i shadow rays; host-driven passes only), moved to the front of the queue, with the any-hit
 *      kernel as the bounces launch it (direct-light terms parked in the path records: it clears the parked term of
 *      every occluded ray of the sample, in the dead path records).
 * out[12]: rays, recorded requests, rays whose list was truncated (256 requests), product ms, replay ms (best of reps),
 * then the issued-request counters of the sample: pairs global / LDS, nodes global / LDS, record heads, tails, spills.
 * Overwrites the hits of the sampled path records; call after the film has been read. */
int  mtsgpu_replay_roof(mtsgpu_ctx *ctx, int kind, uint32_t n, uint32_t stride, int reps, double *out);

/* --- standalone kernels exposed for parity tests and the traversal benchmark */
/* ShapeKDTree::rayIntersect(ray, its) / (ray) on n host rays.
 * rays: [n][8] f32 = o.xyz, mint, d.xyz, maxt.   hits: [n][4] u32 = t(f32 bits), u, v, prim
 * (prim = 0xFFFFFFFF on miss); shadow != 0 -> hits[i][3] = 1/0 occluded (src/librender/skdtree.cpp:108-199) */
int  mtsgpu_trace_rays(mtsgpu_ctx *ctx, const float *rays, uint32_t n, int shadow, uint32_t *hits);
/* LowDiscrepancySampler::generate() for one pixel key (keyed stream), tables as f32:
 * out1d [depth][spp], out2d [depth][spp][2] */
int  mtsgpu_ld_tables(mtsgpu_ctx *ctx, uint32_t pixel_key, float *out1d, float *out2d);
/* What the configured Sampler hands out on the device: generate() for the pixel with key `pixel_key`, then, for camera
 * sample `sample_index`, n calls of next1D() (two_d == 0: out[n]) or next2D() (out[2n]) (src/librender/sampler.cpp,
 * the plugins under src/samplers).  With the halton / hammersley samplers these are the reference's own numbers: the tables of
 * src/tests/test_samplers.cpp:33-78 are checked against this call.  n <= 4096. */
int  mtsgpu_sampler_values(mtsgpu_ctx *ctx, uint32_t pixel_key, uint32_t sample_index, uint32_t n, int two_d, float *out);
/* The reference's `Random` (MT19937-64, src/libcore/random.cpp:99-227, random.h:82-148) run on the device, one generator:
 * seed == 0 is a default-constructed Random (seed 5489), otherwise Random::seed(seed); clone > 0 takes the clone-th
 * Random(Random *) copy of it (random.cpp:105-110), the way per-worker samplers are made.  op 0: n x nextULong();
 * 1: n x nextFloat() as bit patterns; 2: n x nextSize(arg); 3: Random::shuffle of 0 .. n-1.  A test hook: the library's
 * samplers draw from keyed streams; this pins the generator itself to the reference's known answers. */
int  mtsgpu_random_values(mtsgpu_ctx *ctx, int op, uint64_t seed, uint64_t arg, uint32_t clone, uint32_t n, uint64_t *out);
/* The BSDF plugins as the device runs them, for n query records of ONE parameter block (bsdf_type may carry
 * MTSGPU_BSDF_TWOSIDED; params[MTSGPU_BSDF_NPARAMS] as in the enum above).  queries [n][6], out [n][8]:
 *   op 0  BSDF::f(bRec)               queries = wi.xyz, wo.xyz      out = f.rgb
 *   op 1  BSDF::pdf(bRec)             queries = wi.xyz, wo.xyz      out = pdf
 *   op 2  BSDF::sample(bRec, pdf, s)  queries = wi.xyz, s.x, s.y, - out = wo.xyz, pdf, f.rgb, sampledType (bit pattern)
 *         (src/librender/bsdf.cpp:37-48 for the plugins that do not override it; f = 0 and pdf = 0 for a failed sample)
 * wi / wo are in the local shading frame (include/mitsuba/render/bsdf.h:34-132).  A test hook: the chi-square
 * procedure of the reference (src/tests/test_chisquare.cpp:299-420 with the BSDFs of data/tests/test_bsdf.xml) runs
 * against these values, i.e. against the code k_shade executes, with no CPU restatement in between. */
int  mtsgpu_bsdf_eval(mtsgpu_ctx *ctx, uint32_t bsdf_type, const float *params, int op, uint32_t n, const float *queries, float *out);
/* The same operations, query and output layout for entry `index` of a BSDF table types[n_bsdfs], params[n_bsdfs][16] (what
 * mtsgpu_scene carries; checked as mtsgpu_upload_scene checks it).  A composite reaches its children through the table, so
 * mtsgpu_bsdf_eval returns MTSGPU_EINVAL for MTSGPU_BSDF_COMPOSITE and this call evaluates it. */
int  mtsgpu_bsdf_eval_table(mtsgpu_ctx *ctx, uint32_t n_bsdfs, const uint32_t *types, const float *params, uint32_t index, int op,
                            uint32_t n, const float *queries, float *out);
/* SkyLuminaire::configure() (sky.cpp:139-179) for one MTSGPU_LUM_SKY block: derived[MTSGPU_SKY_NDERIVED] = [0] zenith x
 * [1] zenith y [2] zenith Y [3..7] Perez coefficients of x [8..12] of y [13..17] of Y [18..20] the Perez denominators of
 * x, y, Y (sky.cpp:458-461) [21] sin(thetaS) [22] cos(thetaS).  Host only: needs no device and no context.  The library
 * derives the same array when a scene with a sky is uploaded and keeps it in device memory next to the scene. */
int  mtsgpu_sky_configure(const float *block, float *derived);
/* The luminaire plugins as the device runs them, for n query records of ONE parameter block[MTSGPU_LUM_NPARAMS].
 * queries [n][6], out [n][12]:
 *   op 0  Le(direction)        queries = direction.xyz (world)      out = Le.rgb
 *   op 1  sample(p, lRec, s)   queries = p.xyz, s.x, s.y, -         out = lRec.d.xyz, pdf, value.rgb (not divided by the
 *                                                                         pdf), -, lRec.sRec.p.xyz (end of the shadow ray)
 *   op 2  pdf(p, lRec)         queries = p.xyz, lRec.d.xyz          out = pdf
 * Serves MTSGPU_LUM_SKY (checked as mtsgpu_upload_scene checks it); MTSGPU_EINVAL for every other type.  A test hook
 * like mtsgpu_bsdf_eval: ops 0 and 1 call the device functions k_shade calls (sky_le, sky_sample), op 2 returns the constant
 * pdf_luminaire uses. */
int  mtsgpu_lum_eval(mtsgpu_ctx *ctx, uint32_t lum_type, const float *block, int op, uint32_t n, const float *queries, float *out);
/* The luminaires of the uploaded scene (mtsgpu_upload_scene; MTSGPU_ESTATE without one) as the shading kernels run them,
 * for n query records.  queries [n][16], out [n][16], one stride for the three operations:
 *   op 0  Scene::sampleLuminaire without its occlusion test (scene.cpp:396-415)
 *           queries = p.xyz, s.x, s.y
 *           out = found (0 / 1), luminaire index (-1 when not found), lRec.sRec.p.xyz, lRec.sRec.n.xyz, lRec.d.xyz,
 *                 lRec.pdf (multiplied by the selection probability), lRec.value.rgb (divided by that pdf)
 *           as the device function leaves them; p, n, d and value of a sample that was not found are not meaningful
 *   op 1  Scene::pdfLuminaire (scene.cpp:381-394)
 *           queries = p.xyz, lRec.sRec.p.xyz, lRec.sRec.n.xyz, lRec.d.xyz, luminaire index      out = pdf
 *           MTSGPU_EINVAL for an index >= n_lums and for a delta luminaire (point, directional, spot, collimated), for
 *           which no integrator asks
 *   op 2  Scene::LeBackground: Le(normalize(direction)) of the constant, envmap or sky background
 *           queries = direction.xyz (any length but 0)      out = Le.rgb
 *           MTSGPU_EINVAL when the scene has no background luminaire
 * Indices and `found` are floats holding small integers.  A test hook like mtsgpu_bsdf_eval: the three operations call
 * sample_luminaire, pdf_luminaire and background_le, the device functions k_shade calls, in the instantiation (sky or
 * not) the scene's frames use. */
int  mtsgpu_scene_lum_eval(mtsgpu_ctx *ctx, int op, uint32_t n, const float *queries, float *out);
/* its.color as the device computes it for the uploaded scene and its colours (mtsgpu_set_vertex_colors; MTSGPU_ESTATE without
 * them): prim [n] primitive indices, uv [n][2] the hit's barycentrics, out [n][3].  Primitives of shapes without colours
 * give 0.  A test hook: it calls the device function the shading kernels call. */
int  mtsgpu_vertex_color_eval(mtsgpu_ctx *ctx, uint32_t n, const uint32_t *prim, const float *uv, float *out);
/* mtsgpu_bsdf_eval with vertex colours: the slots of mask `slots` take color[3] instead of the block's floats.  Same ops,
 * query and output layout; evaluated through the device function that builds the per-hit block for the shading kernels,
 * so with slots == 0 it returns what mtsgpu_bsdf_eval returns, and otherwise what mtsgpu_bsdf_eval returns for the block
 * with those slots overwritten. */
int  mtsgpu_bsdf_eval_colored(mtsgpu_ctx *ctx, uint32_t bsdf_type, const float *params, uint32_t slots, const float color[3], int op,
                              uint32_t n, const float *queries, float *out);
/* its.uv and the value of *tex there, as the device computes them for the uploaded scene and its texcoords
 * (mtsgpu_set_uv_textures; without it every mesh gives uv = (0, 0)): prim [n] primitive indices, rec [n][3] = the hit's
 * barycentrics (u, v, unused) on a triangle, the world-space hit point on a sphere; out [n][5] = uv.x, uv.y, r, g, b.  tex
 * is checked like the textures of mtsgpu_set_uv_textures, but for the int range of the cast, which is the caller's to keep.
 * A test hook: it calls the device functions the shading kernels call. */
int  mtsgpu_uv_texture_eval(mtsgpu_ctx *ctx, const mtsgpu_uv_texture *tex, uint32_t n, const uint32_t *prim, const float *rec, float *out);
/* mtsgpu_uv_texture_eval for a bitmap: tex of kind MTSGPU_TEX_BITMAP with its Texture2D floats, *bitmap checked like those of
 * mtsgpu_set_uv_bitmap_textures and uploaded for this call alone; same records, same out [n][5].  mtsgpu_uv_texture_eval itself
 * keeps refusing the kind.  A test hook: it calls the device functions the shading kernels call. */
int  mtsgpu_bitmap_texture_eval(mtsgpu_ctx *ctx, const mtsgpu_uv_texture *tex, const mtsgpu_bitmap *bitmap, uint32_t n, const uint32_t *prim,
                                const float *rec, float *out);
/* mtsgpu_bsdf_eval_colored for scenes with uv textures: slot s takes nothing (slot_source[s] = 0), color[3] (1) or
 * values[s][3] (2, the texture's value at the hit).  Same ops, query and output layout; evaluated through the device function
 * that builds the per-hit block for the texture kernels, so it returns what mtsgpu_bsdf_eval returns for the block with
 * those slots overwritten.  A source other than 0 for a slot the type does not have, and a composite, are MTSGPU_EINVAL. */
int  mtsgpu_bsdf_eval_slots(mtsgpu_ctx *ctx, uint32_t bsdf_type, const float *params, const int32_t slot_source[2], const float color[3],
                            const float *values, int op, uint32_t n, const float *queries, float *out);
/* The shading frame as the device computes it for the uploaded scene and its tangents (mtsgpu_upload_scene_tangents; without
 * them every mesh gets Frame(n)): prim [n] primitive indices, rec [n][3] as for mtsgpu_uv_texture_eval; out [n][9] = s, t, n.
 * A test hook: it calls the device function the tangent shading kernels call. */
int  mtsgpu_shading_frame_eval(mtsgpu_ctx *ctx, uint32_t n, const uint32_t *prim, const float *rec, float *out);
/* MIPathTracer::Li for explicit camera samples: in [n][3] u32 = pixel x, y, sample index;
 * out [n][8] f32 = Li rgb, alpha, raster x, raster y, depth, unused */
int  mtsgpu_li_samples(mtsgpu_ctx *ctx, const uint32_t *pix_samples, uint32_t n, float *out);
/* What the film kernels consumed: records first .. first + n of the pass mtsgpu_render rendered last, in record order
 * (record = slot * sampleCount + sample index; slots in the order of the pass's tiles, row-major inside a tile).
 * out [n][8] f32 as for mtsgpu_li_samples = Li rgb (the parked direct-light term settled), alpha, raster x, raster y, depth;
 * the eighth float holds the record's pixel key as a bit pattern: index of the raster pixel in the rendered grid, which with
 * highQualityEdges is the full film grown by the filter border on every side (key = (y + border) * (film width + 2 * border)
 * + x + border), so pixels of the border -- which mtsgpu_li_samples cannot address -- are there.  The film kernels only
 * read the records, so the read-out is valid after mtsgpu_render; a frame rendered in one pass (max_paths large enough)
 * has all its records in place.  MTSGPU_ESTATE when there is no valid last pass (nothing rendered; a setter,
 * mtsgpu_li_samples or mtsgpu_trace_rays since), MTSGPU_EINVAL past its end.  A test hook: tests/ref64_film.py restates
 * ImageBlock::putSample in binary64 over these records and the film must agree. */
int  mtsgpu_pass_samples(mtsgpu_ctx *ctx, uint32_t first, uint32_t n, float *out);
/* The camera records as the camera kernel leaves them, before any bounce overwrites their ray: one launch of that kernel and
 * nothing else.  out [n][14] f32 = ray origin xyz, mint, ray direction xyz, maxt, raster x, raster y, and as bit patterns
 * (u32) the sampler's 1D and 2D counters after generation, the record's pixel key (as for mtsgpu_pass_samples) and its
 * sample index.  Two modes:
 *   pix_samples != NULL: explicit samples, in [n][3] i32 = pixel x, y of the crop window, sample index; first must be 0.  The
 *     sampler tables and arrays are built as mtsgpu_li_samples builds them, the keys lie in the grid mtsgpu_render uses, so
 *     with highQualityEdges the pixels of the filter border are there: x in [-border, width + border), y likewise.
 *   pix_samples == NULL: the pass mtsgpu_render rendered last is generated once more from its saved configuration, pixel list
 *     and sampler tables (as mtsgpu_replay_roof kind 1 does) and records first .. first + n are returned, in the order of
 *     mtsgpu_pass_samples.  MTSGPU_ESTATE when there is no valid last pass.
 * Either mode takes the path records: the last pass is invalid afterwards.  MTSGPU_EINVAL for a pixel or sample index out of
 * range, records past the end of the pass, more than 2^24 records.  A test hook: tests/ref64_camera.py restates
 * PerspectiveCameraImpl::generateRay and OrthographicCamera::generateRay in binary64 and the rays must agree. */
int  mtsgpu_camera_rays(mtsgpu_ctx *ctx, const int32_t *pix_samples, uint32_t first, uint32_t n, float *out);
/* How many entries the closest-hit launches of the last mtsgpu_render / mtsgpu_li_samples appended to every material queue,
 * summed over the bounces: out [MTSGPU_BSDF_NTYPES + 1] u64, entry t = hits on shapes whose BSDF has type t, the last one the
 * terminal queue (hits on shapes without a BSDF and -- in frames that shade their misses: scenes with a background luminaire,
 * the rounds of the direct integrator, the "miss_shaded" knob at 1 -- rays that hit nothing).  Every other frame ends a path
 * whose ray leaves the scene inside the traversal kernel, and that ray is in no queue.  A test hook. */
int  mtsgpu_bin_entries(mtsgpu_ctx *ctx, uint64_t *out);

/* --- host-side flattening (what Scene::initialize does on the CPU) ---------
 * Builds everything a mtsgpu_scene needs from plain meshes: vertex normals
 * (trimesh.cpp:473-545), area CDFs, TriAccel table, SAH kd-tree (gkdtree.h). */
typedef struct mtsgpu_mesh {
	uint32_t n_verts, n_tris;
	const float    *positions;  /* [n_verts][3]                                   */
	const float    *normals;    /* [n_verts][3] or NULL                           */
	const uint32_t *triangles;  /* [n_tris][3]                                    */
	int32_t face_normals;       /* TriMesh 'faceNormals' property                 */
	int32_t bsdf;               /* index or -1                                    */
	int32_t lum;                /* index of the area luminaire attached, or -1    */
	int32_t shape_type;         /* MTSGPU_SHAPE_TRIMESH, or MTSGPU_SHAPE_SPHERE (then n_verts = n_tris = 0) */
	float   sphere_center[3];   /* `center` / `radius` properties (sphere.cpp:44-47)                       */
	float   sphere_radius;
	int32_t sphere_inverted;    /* `inverted` property (sphere.cpp:56)                                      */
} mtsgpu_mesh;

typedef struct mtsgpu_scene_desc {
	uint32_t n_meshes;
	const mtsgpu_mesh *meshes;
	uint32_t n_bsdfs;
	const uint32_t *bsdf_type;
	const float    *bsdf_params;
	uint32_t n_lums;
	const uint32_t *lum_type;    /* area luminaires must be referenced by exactly one mesh */
	const float    *lum_params;  /* constant/directional/envmap: bsphere-derived entries are computed; spot: [6],[7],[9] are computed */
	float camera_pos[3];         /* for ConstantLuminaire::preprocess (constant.cpp:49-63) */
	int32_t has_camera;
	/* bitmap of the envmap luminaire, any size: [env_height][env_width][3] linear RGB (what Bitmap::getFloatData
	 * holds after the EXR is read, mipmap.cpp:161-181); its lum_params carry [0] intensityScale and
	 * [16..24] luminaire->world rotation, everything else is derived */
	uint32_t env_width, env_height;
	const float *env_bitmap;
} mtsgpu_scene_desc;

/* kd-tree build parameters (gkdtree.h:711-724 defaults when 0 / negative) */
typedef struct mtsgpu_kd_params {
	float traversal_cost, query_cost, empty_space_bonus;
	int32_t stop_prims, max_bad_refines, exact_prim_threshold, max_depth, min_max_bins;
	int32_t clip, retract, n_threads;
	/* bit set -- 1: the min-max binning phase (> exact_prim_threshold primitives per node, gkdtree.h:1735-1867) runs on
	 * the current HIP device; 2: the exact O(n log n) sweep below that threshold (gkdtree.h:1898-2345) runs there too.
	 * The tree is the same bit for bit either way.  An error if there is no device; 0 = host */
	int32_t gpu_binning;
} mtsgpu_kd_params;

typedef struct mtsgpu_flat_scene mtsgpu_flat_scene; /* owns the arrays of a mtsgpu_scene */
int  mtsgpu_flatten(const mtsgpu_scene_desc *desc, const mtsgpu_kd_params *kd, mtsgpu_flat_scene **out);
const mtsgpu_scene *mtsgpu_flat_scene_get(const mtsgpu_flat_scene *fs);
void mtsgpu_flat_scene_free(mtsgpu_flat_scene *fs);
/* Per-vertex colours of mesh `mesh_index` of the description (trimesh.h:121-126): colors [that mesh's n_verts][3], copied into
 * a pool the flat scene owns, in the flat scene's vertex order (the flattener keeps every mesh's vertices in the mesh's own
 * order, so a colour stays with its vertex).  colors == NULL takes the mesh's colours away again. */
int  mtsgpu_flat_scene_set_mesh_colors(mtsgpu_flat_scene *fs, uint32_t mesh_index, const float *colors);
/* what mtsgpu_set_vertex_colors takes: the pool [n_verts][3] and the flags [n_shapes]; NULL while no mesh has colours */
const float *mtsgpu_flat_scene_vertex_colors(const mtsgpu_flat_scene *fs);
const uint32_t *mtsgpu_flat_scene_shape_has_colors(const mtsgpu_flat_scene *fs);
/* The same for texture coordinates (trimesh.h m_texcoords): texcoords [that mesh's n_verts][2]; the pool [n_verts][2] and the
 * flags [n_shapes] are what mtsgpu_set_uv_textures takes, NULL while no mesh has texcoords.  Costs 8 bytes per vertex here;
 * on the device 32 bytes per primitive while textures are set. */
int  mtsgpu_flat_scene_set_mesh_texcoords(mtsgpu_flat_scene *fs, uint32_t mesh_index, const float *texcoords);
const float *mtsgpu_flat_scene_vertex_texcoords(const mtsgpu_flat_scene *fs);
const uint32_t *mtsgpu_flat_scene_shape_has_texcoords(const mtsgpu_flat_scene *fs);
/* mtsgpu_flatten with the texture coordinates known at flatten time: mesh_texcoords [n_meshes], entry s = the texcoords [that
 * mesh's n_verts][2] or NULL (always NULL for a sphere).  A mesh whose BSDF is anisotropic (a Ward with alphaU != alphaV, alone,
 * inside a composite or a twosided) is accepted when it has texcoords, and receives vertex tangents as
 * TriMesh::computeTangentSpaceBasis computes them (trimesh.cpp:547-669, binary32, triangle order; a zero vertex normal of such
 * a mesh becomes (1, 0, 0) in vtx_nrm as well); without texcoords it is refused with the reference's message; with texcoords
 * but without vertex normals (face_normals) it is accepted and gets no tangents.  No other mesh is touched.  The texcoords are
 * recorded as mtsgpu_flat_scene_set_mesh_texcoords records them. */
int  mtsgpu_flatten_tangents(const mtsgpu_scene_desc *desc, const mtsgpu_kd_params *kd, const float *const *mesh_texcoords, mtsgpu_flat_scene **out);
/* the tangents [n_verts][6] = dpdu, dpdv (rows of shapes without tangents are zero) and the flags [n_shapes]; NULL while no
 * mesh has tangents.  mtsgpu_upload_scene_tangents takes the dpdu halves. */
const float *mtsgpu_flat_scene_vertex_tangents(const mtsgpu_flat_scene *fs);
const uint32_t *mtsgpu_flat_scene_shape_has_tangents(const mtsgpu_flat_scene *fs);
/* kd-tree statistics logged by the reference builder (gkdtree.h:1178-1213) */
int  mtsgpu_flat_scene_kdstats(const mtsgpu_flat_scene *fs, double *out6 /* inner, leaf, idx, expTrav, expLeaves, expPrims */);

/* One shape of a Mitsuba `.serialized` mesh file, as <shape type="serialized"> with `shapeIndex` loads it
 * (TriMesh::TriMesh(Stream *, int index), src/librender/trimesh.cpp:156-236): header 0x041C / version 3, zlib
 * stream, single or double precision.  *mesh points into *out and stays valid until mtsgpu_loaded_mesh_free;
 * `bsdf` and `lum` are -1, `normals` is NULL when the file has none, `face_normals` follows the file's flag. */
typedef struct mtsgpu_loaded_mesh mtsgpu_loaded_mesh;
int  mtsgpu_load_serialized(const char *path, int shape_index, mtsgpu_loaded_mesh **out, mtsgpu_mesh *mesh);
void mtsgpu_loaded_mesh_free(mtsgpu_loaded_mesh *m);
/* the per-vertex colours of the loaded shape, [n_verts][3] (single or double precision in the file, trimesh.cpp:113-118,
 * 223-229), or NULL when the file has no EHasColors block; valid until mtsgpu_loaded_mesh_free */
const float *mtsgpu_loaded_mesh_colors(const mtsgpu_loaded_mesh *m);
/* likewise the texture coordinates, [n_verts][2] (trimesh.cpp:105-111,214-221), NULL without an EHasTexcoords block */
const float *mtsgpu_loaded_mesh_texcoords(const mtsgpu_loaded_mesh *m);

/* TabulatedFilter (src/librender/rfilter.cpp:40-69) of the reconstruction filter plugins: kind 0 `box`,
 * 1 `gaussian` (p0 = stddev; src/rfilters/gaussian.cpp:30-42,62-65), 2 `mitchell` (p0 = B, p1 = C; mitchell.cpp),
 * 3 `catmullrom`, 4 `wsinc` (p0 = cycles; wsinc.cpp).  half_size / p0 / p1 <= 0 (mitchell: < 0) select the
 * plugin's defaults.  size_xy[2], values[256] */
int  mtsgpu_tabulate_filter(int kind, float half_size, float p0, float p1, float *size_xy, float *values);

/* PerspectiveCameraImpl::configure for a lookAt camera (perspective.cpp:43-71,
 * transform.cpp:100-124,174-190).  fov in degrees along the smaller image side. */
int  mtsgpu_make_camera(const float origin[3], const float target[3], const float up[3],
                        float fov_deg, int width, int height, mtsgpu_camera *out);
/* the same camera looking through a crop window of a film_width x film_height film (perspective.cpp:52-63,
 * film.cpp:33-41): out->width/height = crop size, out->crop_offset_* = crop offset; fov along the smaller side of
 * the FULL film */
int  mtsgpu_make_camera_crop(const float origin[3], const float target[3], const float up[3], float fov_deg,
                             int film_width, int film_height, int crop_x, int crop_y, int crop_width, int crop_height,
                             mtsgpu_camera *out);
/* OrthographicCamera::configure (orthographic.cpp:46-82, transform.cpp:155-158) with toWorld =
 * lookAt(origin, target, up) * scale(scale_x, scale_y, 1): the view volume is 2*scale wide along its smaller side. */
int  mtsgpu_make_camera_ortho(const float origin[3], const float target[3], const float up[3],
                              float scale_x, float scale_y, int width, int height, mtsgpu_camera *out);

#ifdef __cplusplus
}
#endif
#endif /* MTSGPU_H */
