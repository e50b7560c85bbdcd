/* mtsgpu_cloth.h -- the woven-cloth BRDF `irawan` (src/bsdfs/irawan.cpp, irawan.h): an extension of the C ABI of mtsgpu.h (same
 * library, same conventions, same error codes).  ABI version 8 fixes the structs and the list of entry points of mtsgpu.h; what
 * the cloth adds -- two structs and six entry points, no change to anything there -- is declared here, and a caller without
 * cloth needs none of it. */
#ifndef MTSGPU_CLOTH_H
#define MTSGPU_CLOTH_H
#include "mtsgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One yarn as `Yarn` (irawan.h:41-73) holds it after parsing: the angles psi and umax in radians. */
enum { MTSGPU_YARN_WARP = 0, MTSGPU_YARN_WEFT = 1 };
typedef struct mtsgpu_yarn {
	uint32_t type;                 /* MTSGPU_YARN_*                                    */
	float    psi, umax, kappa;     /* fibre twist, maximum inclination, spine curvature */
	float    width, length;        /* the segment rectangle                             */
	float    centerU, centerV;     /* the segment centre in tile space                  */
	float    kd[3], ks[3];         /* diffuse and specular colour                       */
} mtsgpu_yarn;

/* One weave: `WeavePattern` (irawan.h:130-165) and the four members IrawanClothBRDF keeps next to it (irawan.cpp:80-85).  The
 * four d*UmaxOverD* are in radians.  pattern[tileWidth * tileHeight] holds 1-based yarn ids, row by row from the top. */
typedef struct mtsgpu_weave {
	float    alpha, beta, ss, hWidth, warpArea, weftArea;
	uint32_t tileWidth, tileHeight;
	float    dWarpUmaxOverDWarp, dWarpUmaxOverDWeft, dWeftUmaxOverDWarp, dWeftUmaxOverDWeft;
	float    fineness, period;
	float    repeatU, repeatV, kdMultiplier, ksMultiplier;
	uint32_t n_pattern;            /* entries of `pattern`: must equal tileWidth * tileHeight */
	uint32_t n_yarns;
	const uint32_t    *pattern;
	const mtsgpu_yarn *yarns;
} mtsgpu_weave;

/* IrawanClothBRDF samples like the Lambertian (squareToHemispherePSA, pdf = cos / pi) and differs from it in its value, which
 * depends on its.uv and on the directions in the tangent frame.  Like the snow BRDFs it is a side table: an entry with a weave
 * has the type word MTSGPU_BSDF_LAMBERTIAN (optionally | MTSGPU_BSDF_TWOSIDED), its hits land in the Lambertian's queue, and
 * its block of the main table is not read.  The sampled type the read-out reports is EGlossyReflection (0x10).
 *
 * f is restated in binary32 as compiled, not as intended: tileWidth and tileHeight are unsigned, so the yarn centre of a
 * negative (int) xy is a large positive number; and where the reference converts a negative float to uint64_t for a seed --
 * undefined in C++ -- this library takes what the reference's x86-64 build computes, (uint64_t)(int64_t) x, with the seed
 * products wrapping modulo 2^64.
 *
 * mtsgpu_set_cloth_bsdfs hands the table over: weaves[n_weaves], and bsdf_weave[n_bsdfs] of the uploaded scene holding a weave
 * index or -1.  Called after the upload and after the texture call that supplies the texcoords.  Ownership as for
 * mtsgpu_set_snow_bsdfs: NULL or a table of -1 alone switches it off (the context then launches the kernels it launches
 * without one), a new upload clears it.  With a table the Lambertian's queue is shaded by kernels of its own (k_shade_clo).
 * While a table is in force every texture call (mtsgpu_set_uv_textures and its supersets) is refused with MTSGPU_EINVAL and
 * changes nothing: the table was checked against the texcoords that call would replace, and the cloth kernels read them.
 * Switch the table off first.
 *
 * MTSGPU_EINVAL, naming the index and leaving the table off, for
 *   a weave whose n_pattern is not tileWidth * tileHeight, with a zero tile dimension, or with a pattern id outside 1..n_yarns
 *     (the reference's SAsserts);
 *   an unknown yarn type, a non-finite parameter;
 *   width, length or umax <= 0 of a yarn, warpArea or weftArea <= 0, fineness or period < 0 -- narrower than the reference,
 *     which accepts these and produces NaN;
 *   a weave index outside -1..n_weaves-1;
 *   a cloth entry that is not Lambertian (twosided allowed), that is a composite's child, that has a coloured slot, a textured
 *     slot, a mask or a snow record -- whichever of the calls involved comes second refuses;
 *   a mesh with a cloth BSDF and no texcoords ("... needs texture coordinates", trimesh.cpp:551-555);
 *   a mesh with a cloth BSDF, vertex normals and no uploaded tangents (one without vertex normals keeps the frame it has,
 *     trimesh.cpp:562-565);
 *   a vertex uv (on a sphere: uv = 0 or 1) from which one of f's casts -- (int) xy, floorToInt of the two noise arguments, the
 *     (uint64_t) seed factors -- could leave its type's range: the bound is 2^31 - 2^16 as for the texture calls. */
int  mtsgpu_set_cloth_bsdfs(mtsgpu_ctx *ctx, uint32_t n_weaves, const mtsgpu_weave *weaves, const int32_t *bsdf_weave);
/* mtsgpu_set_cloth_bsdfs on every member */
int  mtsgpu_group_set_cloth_bsdfs(mtsgpu_group *g, uint32_t n_weaves, const mtsgpu_weave *weaves, const int32_t *bsdf_weave);

/* mtsgpu_flatten_tangents in a superset form: bsdf_anisotropic[n_bsdfs], or NULL, flags BSDF entries that are treated as
 * anisotropic whatever their block says, so that a mesh with texcoords and a cloth entry -- IrawanClothBRDF is EAnisotropic, its
 * Lambertian entry is not -- receives vertex tangents (TriMesh::configure, trimesh.cpp:288-290).  NULL: mtsgpu_flatten_tangents. */
int  mtsgpu_flatten_tangents_flagged(const mtsgpu_scene_desc *desc, const mtsgpu_kd_params *kd, const float *const *mesh_texcoords,
                                     const uint32_t *bsdf_anisotropic, mtsgpu_flat_scene **out);

/* mtsgpu_bsdf_eval for a cloth entry.  bsdf_type carries only MTSGPU_BSDF_LAMBERTIAN and the twosided bit; the weave is checked
 * like a row of the table.  queries [n][8] = wi, then wo (ops 0, 1, 3) or the sample (op 2), then its.uv; out [n][8].  Ops 0 / 1
 * / 2 are f / pdf / sample(bRec, pdf, s) with the output layout of mtsgpu_bsdf_eval.  Op 3 returns the internals of f before
 * the integrand: yarn id (0-based, as a float), centre x, centre y, random1, random2, intensityVariation, u, v -- zeros where f
 * returns before it looks the yarn up (wi.z <= 0 or wo.z <= 0).  A test hook: it calls the device function the cloth kernels
 * call. */
int  mtsgpu_bsdf_eval_cloth(mtsgpu_ctx *ctx, uint32_t bsdf_type, const mtsgpu_weave *weave, int op, uint32_t n,
                            const float *queries, float *out);

/* What the setter and the hook require of one weave, without a context: the checks of the list above that concern the weave
 * alone and, with uv_range = uMin, uMax, vMin, vMax (or NULL), the casts of f on texcoords inside that range.  0, or
 * MTSGPU_EINVAL with the reason where a call without a context leaves it. */
int  mtsgpu_cloth_check(const mtsgpu_weave *weave, const float *uv_range);
/* The elementary functions of csrc/devmath.h as the host build of the library evaluates them -- the kernels evaluate the same
 * binary64 operations -- for n arguments: fn 0 sin, 1 cos, 2 tan, 3 exp, 4 log, 5 atan, 6 acos, 7 atan2(x, y), 8 sinh, 9 cosh,
 * 10 pow(x, 1.5).  A test hook: a float32 mirror is held to these bit for bit. */
int  mtsgpu_devmath(int fn, uint32_t n, const float *x, const float *y, float *out);

#ifdef __cplusplus
}
#endif
#endif
