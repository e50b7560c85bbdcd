/* mtsgpu_snow.h -- the snow BRDFs `wiscombe` and `hanrahankrueger`: an extension of the C ABI of mtsgpu.h (same library, same
 * conventions, same error codes).  ABI version 8 fixes the structs and the list of entry points of mtsgpu.h; what the snow BRDFs
 * add -- one struct and five entry points, no change to anything there -- is declared here, and a caller without one needs none
 * of it. */
#ifndef MTSGPU_SNOW_H
#define MTSGPU_SNOW_H
#include "mtsgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Wiscombe (src/bsdfs/wiscombe.cpp) and HanrahanKrueger (src/bsdfs/hanrahan-krueger.cpp) sample like the Lambertian
 * (squareToHemispherePSA, pdf = cos / pi, EDiffuseReflection) and differ from it in their value.  They are neither BSDF types
 * nor a bit of bsdf_type but a side table, one entry per BSDF: an entry with a snow record has the type word
 * MTSGPU_BSDF_LAMBERTIAN (optionally | MTSGPU_BSDF_TWOSIDED), so its hits land in the Lambertian's queue, and its block of the
 * main table is not read.  `derived` holds what the reference's configure() leaves behind (mtsgpu_wiscombe_configure,
 * mtsgpu_hk_configure), unused words 0:
 *   MTSGPU_SNOW_WISCOMBE  [0..2] wStar  [3..5] bStar  [6..8] xi  [9..11] P
 *   MTSGPU_SNOW_HK        [0..2] single-scattering albedo sigmaS / sigmaT  [3..5] ssFactor  [6..8] diffuse reflectance (already
 *                         times drFactor)  [9] g  [10] eta = etaInt / etaExt  [11] useDiffuseReflectance as 0 / 1 */
enum { MTSGPU_SNOW_NONE = 0, MTSGPU_SNOW_WISCOMBE = 1, MTSGPU_SNOW_HK = 2 };
typedef struct mtsgpu_bsdf_snow {
	uint32_t kind;         /* MTSGPU_SNOW_*  */
	uint32_t reserved;     /* 0              */
	float    derived[14];  /* see above      */
} mtsgpu_bsdf_snow;

/* Wiscombe::configure (wiscombe.cpp:70-101) in binary32 in the reference's operation order; + - * / and sqrt only, so exact on
 * any IEEE host.  raw = g, depth, w0.rgb, sigmaT.rgb: the four fields of Wiscombe::serialize.  The operators are read as
 * compiled: `m_gStar / bTmp` is the friend operator/(Float, Spectrum &) = bTmp * (1.0f / gStar) (spectrum.h:258-260).
 * MTSGPU_EINVAL for a NULL argument and, with the reason, for a derived value that is not finite (g == 0: bStar). */
int  mtsgpu_wiscombe_configure(const float raw[8], mtsgpu_bsdf_snow *out);
/* HanrahanKrueger::configure (hanrahan-krueger.cpp:89-132) likewise, with both Fdr fits, the eta == 1 case and the binary64
 * sub-expressions its literals 2.0 and 4.0 / 3.0 cause; its two exp calls are the library's dexp.  raw = sigmaA.rgb, sigmaS.rgb
 * (after the size multiplier), g, etaInt, etaExt, ssFactor.rgb, drFactor.rgb, useDiffuseReflectance (0 = off).  MTSGPU_EINVAL
 * for a NULL argument and, with the reason, for a derived value that is not finite (sigmaT == 0). */
int  mtsgpu_hk_configure(const float raw[16], mtsgpu_bsdf_snow *out);

/* Hands the snow table over: table [n_bsdfs] of the uploaded scene, or NULL.  Called after the upload; ownership as for
 * mtsgpu_set_vertex_colors: NULL or a table of MTSGPU_SNOW_NONE alone switches it off (the context then launches the kernels it
 * launches without one), a new upload clears it.  With a table the Lambertian's queue is shaded by kernels of its own
 * (k_shade_snw); every other queue by the kernels it has without one.
 * MTSGPU_EINVAL, naming the BSDF index and leaving the table off, for: an unknown kind, a non-zero reserved word, a non-finite
 * derived word, a snow entry whose type is not Lambertian (twosided allowed), that is a composite's child (the composite's loop
 * would run it as a Lambertian), that has a coloured or a textured slot, or that has a mask.  The last three are refused by
 * whichever of the calls involved comes second: mtsgpu_set_vertex_colors, the three texture calls and this one. */
int  mtsgpu_set_snow_bsdfs(mtsgpu_ctx *ctx, const mtsgpu_bsdf_snow *table);
/* mtsgpu_set_snow_bsdfs on every member */
int  mtsgpu_group_set_snow_bsdfs(mtsgpu_group *g, const mtsgpu_bsdf_snow *table);

/* mtsgpu_bsdf_eval for a snow entry: same ops, query and output layout.  bsdf_type carries only MTSGPU_BSDF_LAMBERTIAN and the
 * twosided bit; the entry is checked like a row of the table; kind MTSGPU_SNOW_NONE evaluates the Lambertian whose reflectance
 * is derived[0..2].  A test hook: it calls the device function the snow kernels call. */
int  mtsgpu_bsdf_eval_snow(mtsgpu_ctx *ctx, uint32_t bsdf_type, const mtsgpu_bsdf_snow *entry, int op, uint32_t n,
                           const float *queries, float *out);

#ifdef __cplusplus
}
#endif
#endif
