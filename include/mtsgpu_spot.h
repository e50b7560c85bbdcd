/* mtsgpu_spot.h -- projection textures of the spot luminaire: an extension of the C ABI of mtsgpu.h (same library, same conventions,
 * same error codes).  ABI version 8 fixes the structs and the list of entry points of mtsgpu.h; what the textured spot adds -- four
 * entry points, no struct, no change to anything there -- is declared here, and a caller without such a luminaire needs none of it. */
#ifndef MTSGPU_SPOT_H
#define MTSGPU_SPOT_H
#include "mtsgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SpotLuminaire with a projection texture (src/luminaires/spot.cpp:87-108).  Inside the cutoff cone falloffCurve looks the texture
 * up at uv = 0.5 + 0.5 * localDir.xy / (localDir.z * uvFactor), uvFactor = tan(cutoffAngle) (configure(), :59; derived by the
 * library in binary32 with the tangent of DESIGN.md section 5), without uv partials (:97).  Texture2D::getValue(its) is then
 * getValue(uv') with uv' = uv * scale + offset (texture.cpp:73-82): a checkerboard, a grid texture, or an ldrtexture, whose
 * lookup without partials is MIPMap::triangle(0, u, v) (ldrtexture.cpp:230-232): the nearest texel for filterType none, and for
 * trilinear and ewa the bilinear lookup on level 0 alone (mipmap.cpp:232-242) -- no pyramid, no EWA.  The value multiplies the
 * intensity before the falloff factor does.
 *
 * textures [n_textures]: mtsgpu_uv_texture of kind MTSGPU_TEX_CHECKERBOARD, _GRID or _BITMAP; bitmaps [n_bitmaps] and
 * texture_bitmap [n_textures] as in mtsgpu_set_uv_bitmap_textures.  texture_bilinear [n_textures] (NULL: all 0): 0 = the nearest
 * texel (filterType none), 1 = triangle(0, ., .) (trilinear, ewa); ignored for the other kinds.  lum_texture [n_lums]: the
 * texture of each luminaire, -1 = none.
 * Call it after an upload; a new upload clears it.  Everything NULL, or every lum_texture -1, switches it off, and a context in
 * which no luminaire has a texture launches exactly the kernels it launches without this call and renders the same bytes.
 * MTSGPU_ESTATE before an upload.  MTSGPU_EINVAL, with a message that says why, for:
 *   a texture on a luminaire that is not a spot; an index out of range; an unknown kind, wrap mode or filter flag; a non-finite
 *   parameter; a bitmap refused by mtsgpu_set_uv_bitmap_textures;
 *   a bilinear bitmap whose width or height is not a power of two (the reference resamples it with a Lanczos kernel first,
 *   mipmap.cpp:34-88: not done here);
 *   a textured spot with cutoffAngle >= 90 degrees or a uvFactor that is not finite and positive (below 90 degrees localDir.z >
 *   cosCutoff > 0 and uv lies in the unit square up to rounding; from there on the division and the (int) casts have no bound);
 *   casts that could leave the int range: (|scale| + |offset| + 1) * max(2, width, height) >= 2^31 - 2^16 in u or v (the margin of 1
 *   covers uv a rounding outside [0, 1], the half-texel shift and the second tap of the bilinear lookup);
 *   a context that has a mask (mtsgpu_set_uv_masked_textures), a snow table or a cloth table in force: the kernels of a textured
 *   spot do not carry those families.  Those three calls refuse likewise while a textured spot is in force: whichever call comes
 *   second refuses. */
int  mtsgpu_set_spot_textures(mtsgpu_ctx *ctx, uint32_t n_textures, const mtsgpu_uv_texture *textures, uint32_t n_bitmaps,
                              const mtsgpu_bitmap *bitmaps, const int32_t *texture_bitmap, const uint32_t *texture_bilinear,
                              const int32_t *lum_texture);
/* mtsgpu_set_spot_textures on every member */
int  mtsgpu_group_set_spot_textures(mtsgpu_group *g, uint32_t n_textures, const mtsgpu_uv_texture *textures, uint32_t n_bitmaps,
                                    const mtsgpu_bitmap *bitmaps, const int32_t *texture_bitmap, const uint32_t *texture_bilinear,
                                    const int32_t *lum_texture);

/* What mtsgpu_set_spot_textures checks, without a context or a device: lum_type [n_lums] and lum_params [n_lums][MTSGPU_LUM_NPARAMS]
 * as the upload takes them; in_force: bit 0 a mask, bit 1 a snow table, bit 2 a cloth table is in force.  Returns 0 or
 * MTSGPU_EINVAL with the refusal in mtsgpu_last_error(NULL).  uv_factor [n_lums] (may be NULL) receives tan(cutoffAngle) of every
 * luminaire that has a texture and 0 for the others: what the call lays out for the kernels. */
int  mtsgpu_spot_textures_check(uint32_t n_lums, const uint32_t *lum_type, const float *lum_params, uint32_t n_textures,
                                const mtsgpu_uv_texture *textures, uint32_t n_bitmaps, const mtsgpu_bitmap *bitmaps,
                                const int32_t *texture_bitmap, const uint32_t *texture_bilinear, const int32_t *lum_texture,
                                uint32_t in_force, float *uv_factor);

/* SpotLuminaire::sample for n points p [n][3] of one spot, block [MTSGPU_LUM_NPARAMS] (checked as above; [6], [7], [9] are derived
 * from [8] and [19] as the flattener derives them), with texture *tex, its *bitmap (NULL unless the kind is MTSGPU_TEX_BITMAP;
 * uploaded for this call alone) and the filter flag `bilinear`.  out [n][8] = lRec.d xyz, uv.x, uv.y (before the Texture2D
 * transform; 0 outside the cutoff cone), lRec.value rgb.  A test hook: it calls the device function the shading kernels call.
 * mtsgpu_scene_lum_eval op 0 on a scene with a textured spot runs the instantiation of sample_luminaire that scene's frames run. */
int  mtsgpu_spot_eval(mtsgpu_ctx *ctx, const float *block, const mtsgpu_uv_texture *tex, const mtsgpu_bitmap *bitmap, uint32_t bilinear,
                      uint32_t n, const float *p, float *out);

#ifdef __cplusplus
}
#endif
#endif
