// scene_upload.cpp -- HBM residency of the flattened scene (include/mtsgpu.h): the three upload entry points.  What they check
// and what they lay out is scene_layout.cpp (host.h: checkScene, layoutScene); here the old scene goes, the new arrays are
// uploaded and the context commits to them.  What comes and goes between two uploads is scene_attach.cpp.
#include "ctx.h"

using namespace mg;

extern "C" {

// mtsgpu_upload_scene (no extras), mtsgpu_upload_scene_tangents and mtsgpu_upload_scene_cylinders (host.h: UploadExtras)
static int uploadScene(mtsgpu_ctx *c, const mtsgpu_scene *sc, const UploadExtras &x) {
	if (!c || !sc) return fail(c, MTSGPU_EINVAL, "null argument");
	c->lastPass.valid = false;
	if (sc->abi_version != MTSGPU_ABI_VERSION) return fail(c, MTSGPU_EINVAL, "scene ABI version %u != %d", sc->abi_version, MTSGPU_ABI_VERSION);
	// nothing is freed before the scene is known to be good: a refused upload keeps the scene in force
	float skyDerived[MTSGPU_SKY_NDERIVED] = { 0 };      // SkyLuminaire::configure() of the background sky, filled by its check
	SceneLayout lay;
	std::string why = checkScene(*sc, x, (uint32_t) trace_stack_levels() - 2, skyDerived);
	if (why.empty()) why = layoutScene(*sc, x, trace_top_nodes(), lay);
	if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
	HIPCHK(c, hipSetDevice(c->device));
	freeAll(c->sceneAllocs);
	c->clearAttachments();
	c->haveScene = false;

	DScene d{};
	int rc = 0;
	rc |= upload(c, (const uint32_t **) &d.nodes, lay.nodes.data(), lay.nodes.size());
	rc |= upload(c, (const uint32_t **) &d.leaf_ta, lay.leafTa.data(), lay.leafTa.size());
	rc |= upload(c, (const float **) &d.tri_pos, lay.triRec.data(), lay.triRec.size());
	d.tri_nrm = d.tri_pos ? d.tri_pos + 3 : nullptr;
	rc |= upload(c, &d.shape_bsdf, sc->shape_bsdf, sc->n_shapes);
	rc |= upload(c, &d.shape_lum, sc->shape_lum, sc->n_shapes);
	rc |= upload(c, &d.shape_flags, sc->shape_flags, sc->n_shapes);
	rc |= upload(c, &d.shape_bin, lay.shapeBin.data(), lay.shapeBin.size());
	rc |= upload(c, &d.shape_type, lay.shapeType.data(), lay.shapeType.size());
	rc |= upload(c, &d.shape_params, lay.shapeParams.data(), lay.shapeParams.size());
	rc |= upload(c, &d.shape_tri_offset, sc->shape_tri_offset, (size_t) sc->n_shapes + 1);
	rc |= upload(c, &d.bsdf_type, sc->bsdf_type, sc->n_bsdfs);
	rc |= upload(c, &d.bsdf_params, sc->bsdf_params, (size_t) MTSGPU_BSDF_NPARAMS * sc->n_bsdfs);
	rc |= upload(c, &d.lum_type, sc->lum_type, sc->n_lums);
	rc |= upload(c, &d.lum_params, sc->lum_params, (size_t) MTSGPU_LUM_NPARAMS * sc->n_lums);
	rc |= upload(c, &d.lum_shape, sc->lum_shape, sc->n_lums);
	rc |= upload(c, &d.lum_inv_area, sc->lum_inv_area, sc->n_lums);
	rc |= upload(c, &d.lum_cdf_offset, sc->lum_cdf_offset, (size_t) sc->n_lums + 1);
	rc |= upload(c, &d.lum_tri_cdf, sc->lum_tri_cdf, sc->lum_cdf_offset[sc->n_lums]);
	rc |= upload(c, &d.lum_sel_cdf, sc->lum_sel_cdf, (size_t) sc->n_lums + 1);
	rc |= upload(c, &d.lum_sel_pdf, sc->lum_sel_pdf, sc->n_lums);
	if (sc->background_lum >= 0 && sc->lum_type[sc->background_lum] == MTSGPU_LUM_ENVMAP) {
		const size_t np = (size_t) sc->env_pdf_width * sc->env_pdf_height;
		rc |= upload(c, &d.env_pixels, sc->env_pixels, 3 * (size_t) sc->env_width * sc->env_height);
		rc |= upload(c, &d.env_pdf, sc->env_pdf, np);
		rc |= upload(c, &d.env_cdf, sc->env_cdf, np + 1);
		d.env_width = sc->env_width; d.env_height = sc->env_height;
		d.env_pdf_width = sc->env_pdf_width; d.env_pdf_height = sc->env_pdf_height;
	}
	if (sc->background_lum >= 0 && sc->lum_type[sc->background_lum] == MTSGPU_LUM_SKY)      // derived once per scene (sky.cpp:139-179)
		rc |= upload(c, (const float **) &d.sky, (const float *) skyDerived, (size_t) MTSGPU_SKY_NDERIVED);
	const float *dDpdu = nullptr; const uint32_t *dHasTan = nullptr;
	if (!lay.triDpdu.empty()) {
		rc |= upload(c, &dDpdu, lay.triDpdu.data(), lay.triDpdu.size());
		rc |= upload(c, &dHasTan, lay.hasTan.data(), lay.hasTan.size());
	}
	if (rc) { freeAll(c->sceneAllocs); return rc; }

	c->tan.d = DTangents{ reinterpret_cast<const float4 *>(dDpdu), dHasTan };
	d.lum_sel_sum = sc->lum_sel_sum; d.background_lum = sc->background_lum;
	d.has_shapes = lay.hasShapes;
	d.n_lums = sc->n_lums; d.n_nodes = sc->n_nodes; d.n_tris = sc->n_tris; d.n_shapes = sc->n_shapes;
	for (int a = 0; a < 3; ++a) { d.aabb_min[a] = sc->aabb_min[a]; d.aabb_max[a] = sc->aabb_max[a]; }
	c->dsc = d; c->nTris = sc->n_tris;
	c->binMask = lay.binMask;
	keepHostScene(*sc, x, lay, c->host);
	c->haveScene = true;
	return 0;
}

int mtsgpu_upload_scene(mtsgpu_ctx *c, const mtsgpu_scene *sc) { return uploadScene(c, sc, UploadExtras()); }

int mtsgpu_upload_scene_cylinders(mtsgpu_ctx *c, const mtsgpu_scene *sc, const float *vtx_dpdu, const uint32_t *shape_has_tangents, const float *cylinders) {
	if ((vtx_dpdu == nullptr) != (shape_has_tangents == nullptr))
		return fail(c, MTSGPU_EINVAL, "vtx_dpdu and shape_has_tangents must both be given or both be NULL");
	return uploadScene(c, sc, UploadExtras{ vtx_dpdu, shape_has_tangents, true, cylinders, true });
}

int mtsgpu_upload_scene_tangents(mtsgpu_ctx *c, const mtsgpu_scene *sc, const float *vtx_dpdu, const uint32_t *shape_has_tangents) {
	if ((vtx_dpdu == nullptr) != (shape_has_tangents == nullptr))
		return fail(c, MTSGPU_EINVAL, "vtx_dpdu and shape_has_tangents must both be given or both be NULL");
	return uploadScene(c, sc, UploadExtras{ vtx_dpdu, shape_has_tangents, true, nullptr, false });
}

} // extern "C"
