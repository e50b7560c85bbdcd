/* mtsgpu_mask.h -- the mask BSDF: an extension of the C ABI of mtsgpu.h (same library, same conventions, same error codes).
 * ABI version 8 fixes the structs and the list of entry points of mtsgpu.h; what the mask adds -- one struct and three entry
 * points, no change to anything there -- is declared here, and a caller that has no masked BSDF needs none of it. */
#ifndef MTSGPU_MASK_H
#define MTSGPU_MASK_H
#include "mtsgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The mask BSDF (src/bsdfs/mask.cpp), an adapter around a nested BSDF: with probability p = opacity.getLuminance() =
 * (r * 0.212671f + g * 0.715160f) + b * 0.072169f at the hit it is the nested BSDF (f and pdf times p, the sample's x divided by
 * p), otherwise the ray passes straight through: wo = -wi, EDeltaTransmission, value 1 - p, pdf (1 - p) |cosTheta(wo)|.  Nothing
 * clamps p.  A pass-through sample gets MIS weight 1, is exempt from Russian roulette and counts as a bounce.  Shadow rays do
 * not see masks (Scene::isOccluded): a masked surface occludes completely.
 * The mask is neither a BSDF type nor a bit of bsdf_type but a side table, one entry per BSDF: the opacity of the Mask around
 * it, which is always the outermost adapter (around TwoSidedBRDF, never inside it: twosided.cpp:71-73). */
enum { MTSGPU_MASK_NONE = 0, MTSGPU_MASK_CONSTANT = 1, MTSGPU_MASK_TEXTURE = 2 };
typedef struct mtsgpu_bsdf_mask {
	uint32_t kind;        /* MTSGPU_MASK_*                                            */
	int32_t  texture;     /* MASK_TEXTURE: index into `textures` of the same call     */
	float    opacity[3];  /* MASK_CONSTANT: the spectrum; MASK_TEXTURE: getAverage()  */
	uint32_t reserved;    /* 0                                                        */
} mtsgpu_bsdf_mask;
/* mtsgpu_set_uv_bitmap_textures with masks: a superset of that call as that one is of mtsgpu_set_uv_textures.  bsdf_mask
 * [n_bsdfs] or NULL.  Same ownership: any of the three calls replaces what the others set, everything NULL switches masks and
 * textures off, a new upload clears them.  With bsdf_mask NULL or every entry MTSGPU_MASK_NONE it does what
 * mtsgpu_set_uv_bitmap_textures does and the context launches the kernels it launches then; otherwise the textures, bitmaps and
 * texcoords are kept even when only a mask uses them, and the shading runs kernels of its own (k_shade_msk).  Masks combine
 * with coloured slots, textured slots and tangents.  The same checks, and MTSGPU_EINVAL as well, naming the BSDF index and
 * leaving masks and textures off, for: an unknown kind, a non-zero reserved word, a non-finite opacity, a texture index out of
 * range, a mask on a composite or on a composite's child.  The (int) cast range check of the two texture calls covers a mask's
 * texture for every shape whose BSDF has that mask, and at uv = (0, 0) for a mask on a BSDF that no shape uses.  Vertex colours
 * as opacity are not served: there is no kind for them. */
int  mtsgpu_set_uv_masked_textures(mtsgpu_ctx *ctx, const float *vtx_uv, const uint32_t *shape_has_uv, uint32_t n_textures,
                                   const mtsgpu_uv_texture *textures, const int32_t *bsdf_slot_texture, uint32_t n_bitmaps,
                                   const mtsgpu_bitmap *bitmaps, const int32_t *texture_bitmap, const mtsgpu_bsdf_mask *bsdf_mask);

/* mtsgpu_set_uv_masked_textures on every member */
int  mtsgpu_group_set_uv_masked_textures(mtsgpu_group *g, const float *vtx_uv, const uint32_t *shape_has_uv, uint32_t n_textures,
                                         const mtsgpu_uv_texture *textures, const int32_t *bsdf_slot_texture, uint32_t n_bitmaps,
                                         const mtsgpu_bitmap *bitmaps, const int32_t *texture_bitmap, const mtsgpu_bsdf_mask *bsdf_mask);

/* mtsgpu_bsdf_eval through the Mask adapter of the mask kernels (mask.cpp:73-161): opacity[3] is the spectrum whose luminance,
 * formed on the device, is the probability p of the nested BSDF.  Same ops, query and output layout: op 0 and 1 return f and
 * pdf times p; op 2 with sample.x <= p returns the nested sample at (sample.x / p, sample.y) with f and pdf times p, otherwise
 * wo = -wi, pdf (1 - p) |wi.z|, f = 1 - p, sampledType EDeltaTransmission (0x8).  p == 0 with sample.x == 0 divides 0 by 0 as the
 * reference does.  A composite is MTSGPU_EINVAL.  A test hook: it calls the device function the mask kernels call. */
int  mtsgpu_bsdf_eval_masked(mtsgpu_ctx *ctx, uint32_t bsdf_type, const float *params, const float opacity[3], int op, uint32_t n,
                             const float *queries, float *out);

#ifdef __cplusplus
}
#endif
#endif
