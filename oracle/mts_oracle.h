/*
 * mts_oracle.h -- CPU oracle for the path-tracing hot path.
 *
 * TEST INFRASTRUCTURE ONLY.  This is a plain-C restatement of the reference
 * algorithm (Mitsuba 0.2.1, /root/reference) used as the checker by tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg.  Nothing under
 * mitsuba-renderer_amd/ links, imports or executes it.
 *
 * PARITY PIN STATUS
 *   pinned  : Triangle::getClippedAABB against the reference's own KATs
 *             (src/tests/test_kd.cpp:34-83); radicalInverse / Halton /
 *             Hammersley against src/tests/test_samplers.cpp:33-87;
 *             Random == MT19937-64 against the published known answers
 *             (10000th output of seed 5489 = 9981545732273789042) and the
 *             values the survey measured from the reference.
 *   binary64: f, pdf and sample(bRec, pdf, s) of every BSDF plugin and the
 *             twosided wrapper, fresnel / fresnelConductor, and the radiance of
 *             the point, spot, directional and collimated luminaires, against a
 *             second, independent restatement in binary64 (tests/ref64.py),
 *             within a stated multiple of 2^-23 times a conditioning factor,
 *             exact zeros included (tests/test_closed_forms.py; the device in
 *             tests/test_gpu_closed_forms.py).  Independent of this code, but
 *             still a reading of the reference, not its output.
 *   unpinned: everything else ("parity unpinned").  The reference cannot be
 *             built in this image: every translation unit includes
 *             include/mitsuba/core/util.h:22 -> <boost/static_assert.hpp>
 *             (Boost, xerces-c, OpenEXR, libpng are absent and may not be
 *             stubbed), so no oracle/_ref exists.  Those functions are
 *             line-by-line restatements with file:line citations; their
 *             self-consistency is checked the way the reference's own
 *             test_chisquare.cpp does it.
 *
 * Scene data uses the same flat layout as include/mtsgpu.h (mtsgpu_scene).
 */
#ifndef MTS_ORACLE_H
#define MTS_ORACLE_H

#include <stdint.h>
#include <stddef.h>
#include "../include/mtsgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------- Random (src/libcore/random.cpp:99-227) ------------------ */
#define ORC_MT_N 312
typedef struct orc_random {
	uint64_t mt[ORC_MT_N];
	int mti;
} orc_random;

void     orc_random_seed(orc_random *r, uint64_t seed);            /* Random::seed(uint64_t)     */
void     orc_random_seed_array(orc_random *r, const uint64_t *key, uint64_t len); /* seed(uint64_t*,len) */
void     orc_random_seed_from(orc_random *r, orc_random *parent);  /* Random::seed(Random*)      */
uint64_t orc_random_next_ulong(orc_random *r);
float    orc_random_next_float(orc_random *r);
uint64_t orc_random_next_size(orc_random *r, uint64_t n);
void     orc_random_shuffle_u32(orc_random *r, uint32_t *a, size_t n); /* Random::shuffle       */

/* ---------------- keyed stream ---------------------- */
uint64_t orc_keyed_init(uint64_t seed, uint64_t a, uint64_t b);
uint64_t orc_keyed_next(uint64_t *state);

/* ---------------- low-discrepancy code (src/samplers/ldsampler.cpp:104-141) */
uint32_t orc_vdc_bits(uint32_t n, uint32_t scramble);     /* vanDerCorput before the divide */
uint32_t orc_sobol2_bits(uint32_t n, uint32_t scramble);  /* sobol2 before the divide       */
float    orc_u32_to_unit(uint32_t n);                     /* (Float) n / (Float) 0x100000000LL */
/* generate(): depth x (generate1D + generate2D) with the sequential MT stream */
void orc_ld_generate_mt(orc_random *r, uint32_t spp, int depth, float *out1d, float *out2d);
/* the same with the keyed stream of one pixel; perm tables optional (may be NULL) */
void orc_ld_generate_keyed(uint64_t seed, uint32_t pixel_key, uint32_t spp, int depth,
                           float *out1d, float *out2d);
float orc_radical_inverse(int b, uint64_t i);                 /* util.cpp:738-750 */
float orc_radical_inverse_incremental(int b, float x);       /* util.cpp:752-768 */

/* ---------------- warps / Fresnel (src/libcore/util.cpp:543-738) ---------- */
void  orc_square_to_sphere(const float s[2], float out[3]);
void  orc_square_to_hemisphere_psa(const float s[2], float out[3]);
void  orc_square_to_triangle(const float s[2], float out[2]);
void  orc_coordinate_system(const float a[3], float b[3], float c[3]);
float orc_fresnel_dielectric(float cosTheta1, float cosTheta2, float etaI, float etaT);
float orc_fresnel(float cosThetaI, float etaExt, float etaInt);
void  orc_fresnel_conductor(float cosTheta, const float eta[3], const float k[3], float out[3]);
/* deterministic elementary functions shared (as a specification) with the kernels */
float orc_sinf(float x); float orc_cosf(float x); float orc_expf(float x);
float orc_logf(float x); float orc_atanf(float x); float orc_pow4f(float x);
float orc_powf(float x, float y); float orc_acosf(float x); float orc_atan2f(float y, float x);
void  orc_square_to_disk_concentric(const float s[2], float out[2]);

/* ---------------- triangle code ------------------------------------------- */
/* Triangle::getClippedAABB (src/libcore/triangle.cpp:59-158); returns 0 if invalid */
int   orc_clipped_aabb(const float p0[3], const float p1[3], const float p2[3],
                       const float bmin[3], const float bmax[3], float omin[3], float omax[3]);
/* TriAccel::load (include/mitsuba/render/triaccel.h:63-95) -> 12 dwords */
int   orc_triaccel_load(const float A[3], const float B[3], const float C[3], uint32_t out[12]);
/* TriAccel::rayIntersect (triaccel.h:98-159) */
int   orc_triaccel_intersect(const uint32_t ta[12], const float o[3], const float d[3],
                             float mint, float maxt, float *u, float *v, float *t);

/* ---------------- flattening (Scene::initialize on the CPU) ---------------- */
typedef struct orc_flat_scene orc_flat_scene;
int  orc_flatten(const mtsgpu_scene_desc *desc, const mtsgpu_kd_params *kd, orc_flat_scene **out);
const mtsgpu_scene *orc_flat_scene_get(const orc_flat_scene *fs);
void orc_flat_scene_free(orc_flat_scene *fs);
int  orc_flat_scene_kdstats(const orc_flat_scene *fs, double *out6);
int  orc_make_camera(const float origin[3], const float target[3], const float up[3],
                     float fov_deg, int width, int height, mtsgpu_camera *out);
int orc_make_camera_ortho(const float origin[3], const float target[3], const float up[3],
                          float scale_x, float scale_y, int width, int height, mtsgpu_camera *out);

/* ---------------- traversal (skdtree.cpp:108-199, sahkdtree3.h:170-300) ---- */
typedef struct orc_trace_counts { uint64_t n_inner, n_leaf, n_idx, n_tri_tested; } orc_trace_counts;
/* same contract as mtsgpu_trace_rays; counts may be NULL */
void orc_trace_rays(const mtsgpu_scene *sc, const float *rays, uint32_t n, int shadow,
                    uint32_t *hits, orc_trace_counts *counts);

/* ---------------- the path tracer ------------------------------------------ */
typedef struct orc_render_params {
	int max_depth, rr_depth, strict_normals;   /* integrator.cpp:272-292 */
	int sampler_kind;                          /* MTSGPU_SAMPLER_*        */
	uint32_t spp; int ld_depth; uint64_t seed;
	int n_threads;                             /* OpenMP threads (0 = all) */
	int integrator;                            /* 0 = path (MIPathTracer), 1 = direct (MIDirectIntegrator) */
	int luminaire_samples, bsdf_samples;       /* direct.cpp:36-41; > 1: Sampler::next2DArray           */
} orc_render_params;

/* SampleIntegrator::renderBlock over a pixel rectangle [x0,x1) x [y0,y1) with the
 * keyed samplers; film: full-frame [H][W][5] f32 (spec rgb, alpha, weight), summed into. */
void orc_render_rect(const mtsgpu_scene *sc, const mtsgpu_camera *cam, const orc_render_params *p,
                     int x0, int y0, int x1, int y1, float *film, mtsgpu_stats *stats);
/* Sampler::generate() for a pixel, then n x next1D() (or next2D(): out[2n]) of camera sample `sample_index`;
 * same contract as mtsgpu_sampler_values */
void orc_sampler_values(const orc_render_params *p, uint32_t pixel_key, uint32_t sample_index, uint32_t n, int two_d, float *out);
/* MIPathTracer::Li for explicit (pixel, sample) pairs; same contract as mtsgpu_li_samples */
void orc_li_samples(const mtsgpu_scene *sc, const mtsgpu_camera *cam, const orc_render_params *p,
                    const uint32_t *pix_samples, uint32_t n, float *out);
/* Camera::generateRay for n given samples: in [n][4] = raster x, y, lens sample x, y; out [n][14] laid out like
 * mtsgpu_camera_rays (o, mint, d, maxt, raster x, y; the four words of the sampler and the key are left 0) */
void orc_camera_rays(const mtsgpu_camera *cam, uint32_t n, const float *samples, float *out);
/* The reference's own sequential sampling (one MT19937-64 stream, scanline pixel
 * order inside the rectangle): kind 0 = independent.cpp, 1 = ldsampler.cpp. */
void orc_render_rect_mt(const mtsgpu_scene *sc, const mtsgpu_camera *cam, const orc_render_params *p,
                        int kind, int x0, int y0, int x1, int y1, float *film);

/* TabulatedFilter (src/librender/rfilter.cpp:40-69): kind 0 = box (src/rfilters/box.cpp),
 * 1 = gaussian (src/rfilters/gaussian.cpp, halfSize / stddev properties) */
typedef struct orc_tabfilter { float size_x, size_y, values[16][16]; } orc_tabfilter;
void orc_tabulate_filter(int kind, float half_size, float p0, float p1, orc_tabfilter *out);
/* BlockedRenderProcess: every ImageBlock tile (imageproc.cpp:43-78) with t % n_parts == part is
 * rendered into a block with a border of ceil(size - 0.5) pixels (renderproc.cpp:143-144) through
 * ImageBlock::putSample, then added to the film (Film::putImageBlock, mfilm.cpp:118-143).
 * Summation order is fixed: inside a block by (pixel row-major, sample index),
 * blocks by (tx%2 + 2*(ty%2)) colour. */
/* rays of the reference's traversal benchmark (src/tests/test_kd.cpp:96-116) */
void orc_chord_rays(const float center[3], float radius, uint32_t n, float *rays);

/* test hooks for the luminaires: Luminaire::sample without the visibility test (out = p, n, d, value, pdf) and
 * Scene::pdfLuminaire */
void orc_luminaire_sample(const mtsgpu_scene *sc, int l, const float p[3], const float sample[2], float out[13]);
float orc_luminaire_pdf(const mtsgpu_scene *sc, int l, const float p[3], const float lp[3], const float ln[3], const float ld[3]);
/* mtsgpu_scene_lum_eval (include/mtsgpu.h) on the oracle: same ops, same [n][16] records; Scene::sampleLuminaire is taken
 * without its occlusion test.  -1 for what that call refuses, and for a scene with a sky. */
int orc_scene_lum_eval(const mtsgpu_scene *sc, int op, uint32_t n, const float *queries, float *out);

void orc_render_tiles(const mtsgpu_scene *sc, const mtsgpu_camera *cam, const orc_render_params *p,
                      const orc_tabfilter *filter, int block_size, int part, int n_parts, int hq_edges,
                      float *film, mtsgpu_stats *stats);

/* BSDF entry points for the chi-square self-consistency test (test_chisquare.cpp:299-420).
 * wi, wo in the local shading frame. */
void  orc_bsdf_f(uint32_t type, const float *params, const float wi[3], const float wo[3], float out[3]);
float orc_bsdf_pdf(uint32_t type, const float *params, const float wi[3], const float wo[3]);
/* sample(bRec, pdf, sample): returns f (not divided), fills wo, pdf, sampledType */
void  orc_bsdf_eval(uint32_t type, const float *params, int op, uint32_t n, const float *queries, float *out);
void  orc_bsdf_sample(uint32_t type, const float *params, const float wi[3], const float s[2],
                      float wo[3], float *pdf, uint32_t *sampled_type, float out[3]);

#ifdef __cplusplus
}
#endif
#endif
