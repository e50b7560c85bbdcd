/* mtsgpu_cylinder.h -- the cylinder shape: an extension of the C ABI of mtsgpu.h (same library, same conventions, same error codes).
 * ABI version 8 fixes the structs and the list of entry points of mtsgpu.h; what the cylinder adds -- one struct, one shape type and
 * seven entry points, no change to anything there -- is declared here, and a caller that has no cylinder needs none of it. */
#ifndef MTSGPU_CYLINDER_H
#define MTSGPU_CYLINDER_H
#include "mtsgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The cylinder (src/shapes/cylinder.cpp): the open tube x^2 + y^2 = radius^2, 0 <= z <= length of its object space, no caps.
 * Like the sphere it is ONE kd-tree primitive with k = MTSGPU_KNOTRIANGLE; unlike the sphere's its box is clipped to a cell the
 * way Cylinder::getClippedAABB does it (cylinder.cpp:216-375), so the trees are the reference's.  mtsgpu_mesh has no room for
 * it and MTSGPU_SHAPE_NPARAMS is three floats short of its derived block, so both travel beside the description and the scene:
 * mesh s of the description has shape_type MTSGPU_SHAPE_CYLINDER (its other geometry fields are ignored, bsdf is read, lum must
 * be -1) and takes cylinders[s] of mtsgpu_flatten_cylinders. */
#define MTSGPU_SHAPE_CYLINDER 2
enum { MTSGPU_CYLINDER_POINTS = 0, MTSGPU_CYLINDER_TOWORLD = 1 };
typedef struct mtsgpu_cylinder {
	uint32_t form;          /* MTSGPU_CYLINDER_POINTS: p1, p2, radius; MTSGPU_CYLINDER_TOWORLD: to_world              */
	float    p1[3], p2[3];  /* the axis runs from p1 (z = 0) to p2 (z = length)                                        */
	float    radius;
	float    to_world[16];  /* row-major 4x4 from the unit cylinder (radius 1, length 1); its last row must be 0 0 0 1 */
} mtsgpu_cylinder;
/* The derived block, what both constructors leave behind: objectToWorld rows [0..11] (3x4), worldToObject rows [12..23] (3x4),
 * radius [24], length [25], 1 / surface area [26], 0 [27]. */
#define MTSGPU_CYLINDER_NDERIVED 28

/* Both constructors of cylinder.cpp:34-64 in binary32: POINTS gives translate(p1) * fromFrame(Frame(rel / length)), the inverse
 * being the product of the two inverses; TOWORLD takes radius and length from the images of (1,0,0) and (0,0,1), inverts the
 * matrix (Matrix::invert) and removes the scale, objectToWorld * scale(1/r, 1/r, 1/l).  Needs no context.  MTSGPU_EINVAL for a
 * non-finite input, radius <= 0 or length <= 0 (the reference's Assert), a singular matrix, a last row other than 0 0 0 1, an
 * unknown form. */
int  mtsgpu_cylinder_configure(const mtsgpu_cylinder *in, float *derived);

/* mtsgpu_flatten_tangents_flagged for a description with cylinders: cylinders [n_meshes], read for the meshes of type
 * MTSGPU_SHAPE_CYLINDER; NULL gives that call (which, like mtsgpu_flatten and mtsgpu_flatten_tangents, refuses the type).
 * mesh_texcoords may be NULL here.  A cylinder counts one primitive, its tri row is {MTSGPU_KNOTRIANGLE x 3}.  Refused, as
 * the reference cannot render it either: a cylinder with an area luminaire (Cylinder has no pdfArea: Shape::pdfArea raises,
 * shape.cpp:174-178, on the first BSDF-sampled hit). */
int  mtsgpu_flatten_cylinders(const mtsgpu_scene_desc *desc, const mtsgpu_kd_params *kd, const float *const *mesh_texcoords,
                              const uint32_t *bsdf_anisotropic, const mtsgpu_cylinder *cylinders, mtsgpu_flat_scene **out);
/* [n_shapes][MTSGPU_CYLINDER_NDERIVED], zero rows for the other shapes; NULL for a scene without a cylinder */
const float *mtsgpu_flat_scene_cylinders(const mtsgpu_flat_scene *fs);

/* mtsgpu_upload_scene_tangents plus the derived blocks of the cylinders: cylinders [n_shapes][MTSGPU_CYLINDER_NDERIVED], read for
 * the shapes of type MTSGPU_SHAPE_CYLINDER, or NULL; vtx_dpdu / shape_has_tangents both NULL or both given.  The only upload
 * that accepts the type: mtsgpu_upload_scene and mtsgpu_upload_scene_tangents refuse it and name this call, and this call
 * refuses it with cylinders NULL.  A scene without a cylinder is uploaded as by those two, launches exactly the kernels it
 * launches then and renders the same bytes.  A new upload of any kind replaces everything.  MTSGPU_EINVAL as well for a
 * non-finite block, radius <= 0, length <= 0, a cylinder with a luminaire, and a cylinder whose BSDF is not a plain
 * MTSGPU_BSDF_LAMBERTIAN (no other type, no MTSGPU_BSDF_TWOSIDED: their shading kernels do not build a cylinder's record yet).  For the
 * same reason a context whose scene has a cylinder refuses mtsgpu_set_uv_masked_textures with a mask, mtsgpu_set_snow_bsdfs and
 * mtsgpu_set_cloth_bsdfs with a table, each naming the cylinder. */
int  mtsgpu_upload_scene_cylinders(mtsgpu_ctx *ctx, const mtsgpu_scene *scene, const float *vtx_dpdu, const uint32_t *shape_has_tangents,
                                   const float *cylinders);
/* mtsgpu_upload_scene_cylinders on every member */
int  mtsgpu_group_upload_scene_cylinders(mtsgpu_group *g, const mtsgpu_scene *scene, const float *vtx_dpdu, const uint32_t *shape_has_tangents,
                                         const float *cylinders);

/* Cylinder::getAABB (cylinder.cpp:187-208) of a derived block: out6 = min, max.  A test hook. */
int  mtsgpu_cylinder_aabb(const float *derived, float *out6);
/* Cylinder::getClippedAABB (cylinder.cpp:216-375) of a derived block against n cells: boxes [n][6] = min, max; out [n][6]; valid
 * [n] = the result's isValid().  on_device = 0 runs the host builder's function, 1 the same function in a kernel of the device
 * exact phase's unit (needs a GPU).  A test hook. */
int  mtsgpu_cylinder_clip(const float *derived, uint32_t n, const float *boxes, int on_device, float *out, uint32_t *valid);
/* The intersection record of a cylinder (Cylinder::fillIntersectionRecord, cylinder.cpp:154-176) is read out through the hooks
 * of mtsgpu.h: for a primitive of a cylinder mtsgpu_shading_frame_eval and mtsgpu_uv_texture_eval take rec = the world-space
 * hit point, as for a sphere, and return the frame (normalize(dpdu), normalize(dpdv), n) and its.uv. */

#ifdef __cplusplus
}
#endif
#endif
