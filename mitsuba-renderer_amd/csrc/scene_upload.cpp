// scene_upload.cpp -- HBM residency of the flattened scene (include/mtsgpu.h): what mtsgpu_upload_scene validates, re-lays
// out and uploads, and the per-vertex attributes that come and go between two uploads (vertex colours, uv textures).
#include "ctx.h"
#include <algorithm>
#include <cmath>
#include <cstring>

using namespace mg;

// what mtsgpu_set_uv_textures and mtsgpu_uv_texture_eval require of one descriptor; the reason, or an empty string
// (bitmaps: a call that takes MTSGPU_TEX_BITMAP, of which only the four Texture2D floats count)
std::string mg::checkUvTexture(const mtsgpu_uv_texture &t, bool bitmaps) {
	const bool bitmap = bitmaps && t.kind == (uint32_t) MTSGPU_TEX_BITMAP;
	if (t.kind >= (uint32_t) MTSGPU_TEX_NKINDS && !bitmap) return "unknown kind " + std::to_string(t.kind);
	const float *f = &t.uoffset;      // the eleven floats behind the kind
	for (int i = 0; i < (bitmap ? 4 : 11); ++i) if (!std::isfinite(f[i])) return "non-finite parameter";
	return std::string();
}

// what mtsgpu_set_uv_bitmap_textures and mtsgpu_bitmap_texture_eval require of one bitmap; the reason, or an empty string.
// *total counts the texels so far and is checked before any texel is read
std::string mg::checkBitmap(const mtsgpu_bitmap &b, uint64_t *total) {
	if (b.width == 0 || b.height == 0) return "zero dimension (" + std::to_string(b.width) + " x " + std::to_string(b.height) + ")";
	if (b.wrap_mode > (uint32_t) MTSGPU_WRAP_WHITE) return "unknown wrap mode " + std::to_string(b.wrap_mode);
	if (b.reserved != 0) return "reserved word is not zero";
	*total += (uint64_t) b.width * b.height;
	if (*total > (uint64_t) MTSGPU_BITMAP_MAX_TEXELS)
		return "more than " + std::to_string(MTSGPU_BITMAP_MAX_TEXELS) + " texels in all (the pool is indexed with one uint32)";
	if (!b.texels) return "no texels";
	const size_t n = 3 * (size_t) b.width * b.height;
	for (size_t i = 0; i < n; ++i)
		if (!std::isfinite(b.texels[i]) || b.texels[i] < 0.0f)
			return "texel (" + std::to_string((i / 3) % b.width) + ", " + std::to_string((i / 3) / b.width) + ") is negative or not finite";
	return std::string();
}

// the texels of one bitmap as the pool holds them: one float4 (r, g, b, unused) each, row-major
void mg::packBitmapTexels(const mtsgpu_bitmap &b, float *dst) {
	const size_t n = (size_t) b.width * b.height;
	for (size_t i = 0; i < n; ++i) {
		dst[4 * i] = b.texels[3 * i]; dst[4 * i + 1] = b.texels[3 * i + 1]; dst[4 * i + 2] = b.texels[3 * i + 2]; dst[4 * i + 3] = 0.0f;
	}
}

namespace {

// The rows of one mesh in a per-primitive gather array: for each of its primitives [t0, t1) the attribute of the three
// vertices (`comps` floats per vertex: 4 floats apart for tangents and colours, 2 for texcoords), in rows of 4 * stride
// floats.  A non-finite component is refused: false, and *bad names the vertex.
bool gatherMeshRows(const uint32_t *triIdx, uint32_t t0, uint32_t t1, const float *vtx, int comps, size_t stride, float *rows, uint32_t *bad) {
	const size_t slot = comps == 3 ? 4 : (size_t) comps;
	for (uint32_t t = t0; t < t1; ++t)
		for (int k = 0; k < 3; ++k) {
			const uint32_t v = triIdx[3 * (size_t) t + k];      // < n_verts: mtsgpu_upload_scene checked it
			const float *a = vtx + (size_t) comps * v;
			for (int i = 0; i < comps; ++i) if (!std::isfinite(a[i])) { *bad = v; return false; }
			std::memcpy(&rows[4 * stride * (size_t) t + slot * (size_t) k], a, sizeof(float) * (size_t) comps);
		}
	return true;
}

} // namespace

extern "C" {

// mtsgpu_upload_scene (vtx_dpdu = shape_has_tangents = NULL, withTangents = false), mtsgpu_upload_scene_tangents and
// mtsgpu_upload_scene_cylinders (cylinders = the derived blocks [n_shapes][MTSGPU_CYLINDER_NDERIVED] or NULL, `me` = the call
// that accepts them; NULL, nullptr in the other two, which refuse the shape type)
static int uploadScene(mtsgpu_ctx *c, const mtsgpu_scene *sc, const float *vtx_dpdu, const uint32_t *shape_has_tangents, bool withTangents,
                       const float *cylinders = nullptr, bool acceptsCylinders = false) {
	if (!c || !sc) return fail(c, MTSGPU_EINVAL, "null argument");
	c->lastPass.valid = false;
	if (sc->abi_version != MTSGPU_ABI_VERSION) return fail(c, MTSGPU_EINVAL, "scene ABI version %u != %d", sc->abi_version, MTSGPU_ABI_VERSION);
	if (sc->n_nodes == 0 || !sc->kd_nodes) return fail(c, MTSGPU_EINVAL, "scene has no kd-tree");
	if (sc->n_lums == 0) return fail(c, MTSGPU_EINVAL, "scene has no luminaire (Scene::initialize would add a constant one, scene.cpp:310-318)");
	HIPCHK(c, hipSetDevice(c->device));
	// --- validate everything the kernels index with (an out-of-range index would fault the GPU) ---
	for (uint32_t i = 0; i < sc->n_nodes; ++i) {
		const uint32_t a = sc->kd_nodes[2 * (size_t) i], b = sc->kd_nodes[2 * (size_t) i + 1];
		if (a & 0x80000000u) {
			if ((a & 0x7FFFFFFFu) > b || b > sc->n_indices) return fail(c, MTSGPU_EINVAL, "kd leaf %u: index range out of bounds", i);
		} else {
			if (a & 0x40000000u) return fail(c, MTSGPU_EINVAL, "kd node %u: indirection nodes are not supported (gkdtree.h:1116-1126 removes them)", i);
			const uint64_t left = (uint64_t) i + ((a & 0x3FFFFFFCu) >> 2);
			if ((a & 3u) == 3u || left <= i || left + 1 >= sc->n_nodes) return fail(c, MTSGPU_EINVAL, "kd node %u: bad axis/child offset", i);
		}
	}
	{
		// every node is reached exactly once from the root (the device order below is built by walking the tree: an
		// unreached node would land on the root's slot, a shared one twice) and no branch is deeper than the traversal
		// stack of k_trace (LDS levels + spill levels; the reference's own limit is MTS_KD_MAXDEPTH = 48, gkdtree.h:35)
		const uint32_t depthLimit = (uint32_t) trace_stack_levels() - 2;
		std::vector<uint8_t> seen(sc->n_nodes, 0);
		std::vector<std::pair<uint32_t, uint32_t>> stack;       // node, depth
		stack.emplace_back(0u, 1u);
		uint32_t visited = 0;
		while (!stack.empty()) {
			const auto [i, depth] = stack.back(); stack.pop_back();
			if (seen[i]) return fail(c, MTSGPU_EINVAL, "kd node %u is the child of two nodes", i);
			seen[i] = 1; ++visited;
			const uint32_t a = sc->kd_nodes[2 * (size_t) i];
			if (a & 0x80000000u) continue;
			if (depth >= depthLimit) return fail(c, MTSGPU_EINVAL, "kd-tree deeper than %u levels", depthLimit);
			const uint32_t left = i + ((a & 0x3FFFFFFCu) >> 2);
			stack.emplace_back(left + 1, depth + 1); stack.emplace_back(left, depth + 1);
		}
		if (visited != sc->n_nodes) return fail(c, MTSGPU_EINVAL, "kd-tree: %u of %u nodes are unreachable from the root", sc->n_nodes - visited, sc->n_nodes);
	}
	for (uint32_t i = 0; i < sc->n_indices; ++i)
		if (sc->kd_indices[i] >= sc->n_tris) return fail(c, MTSGPU_EINVAL, "kd index %u out of range", i);
	if ((sc->shape_type == nullptr) != (sc->shape_params == nullptr)) return fail(c, MTSGPU_EINVAL, "shape_type and shape_params must both be given or both be NULL");
	auto shapeType = [&](uint32_t s) { return sc->shape_type ? sc->shape_type[s] : (uint32_t) MTSGPU_SHAPE_TRIMESH; };
	for (uint32_t s = 0; s < sc->n_shapes; ++s) {
		if (shapeType(s) == MTSGPU_SHAPE_CYLINDER) {
			if (!acceptsCylinders) return fail(c, MTSGPU_EINVAL, "shape %u is a cylinder: its derived block travels beside the scene, upload it with mtsgpu_upload_scene_cylinders", s);
			if (!cylinders) return fail(c, MTSGPU_EINVAL, "shape %u is a cylinder, but mtsgpu_upload_scene_cylinders was given no cylinder blocks", s);
		} else if (shapeType(s) > MTSGPU_SHAPE_SPHERE) return fail(c, MTSGPU_EINVAL, "shape %u: unknown shape type", s);
		if (sc->shape_tri_offset[s] > sc->shape_tri_offset[s + 1] || sc->shape_tri_offset[s + 1] > sc->n_tris) return fail(c, MTSGPU_EINVAL, "shape_tri_offset not monotone");
		const bool mesh = shapeType(s) == MTSGPU_SHAPE_TRIMESH;
		if (!mesh) {
			// any other shape is ONE kd-tree primitive (skdtree.cpp:54-57)
			if (sc->shape_tri_offset[s + 1] - sc->shape_tri_offset[s] != 1) return fail(c, MTSGPU_EINVAL, "shape %u: a non-mesh shape must own exactly one primitive", s);
			const float *SP = sc->shape_params + (size_t) MTSGPU_SHAPE_NPARAMS * s;
			for (int i = 0; i < MTSGPU_SHAPE_NPARAMS; ++i) if (!std::isfinite(SP[i])) return fail(c, MTSGPU_EINVAL, "shape %u: non-finite parameter", s);
			if (shapeType(s) == MTSGPU_SHAPE_CYLINDER) {
				const std::string why = checkCylinderBlock(cylinders + (size_t) MTSGPU_CYLINDER_NDERIVED * s);
				if (!why.empty()) return fail(c, MTSGPU_EINVAL, "shape %u: %s", s, why.c_str());
				// what a cylinder's hit has been rendered and checked with: a plain Lambertian (constant, checkerboard, grid or bitmap
				// reflectance).  Every other family is refused by name until it has its frames: the shading kernels of the other
				// bins and of the mask, snow and cloth families are compiled without the cylinder's record (shade_bsdf.h: CYL)
				// (without a BSDF its closest hits would go to the terminal bin, whose kernel does not build a cylinder's record either)
				if (sc->shape_bsdf[s] < 0)
					return fail(c, MTSGPU_EINVAL, "shape %u: a cylinder without a BSDF is not served yet: give it a plain lambertian", s);
				if (sc->shape_bsdf[s] < (int32_t) sc->n_bsdfs && sc->bsdf_type[sc->shape_bsdf[s]] != (uint32_t) MTSGPU_BSDF_LAMBERTIAN)
					return fail(c, MTSGPU_EINVAL, "shape %u: a cylinder takes a plain lambertian BSDF only; BSDF %d is of type %u%s, not served on a cylinder yet",
					            s, sc->shape_bsdf[s], sc->bsdf_type[sc->shape_bsdf[s]] & 0xFFu, (sc->bsdf_type[sc->shape_bsdf[s]] & MTSGPU_BSDF_TWOSIDED) ? " under twosided" : "");
				if (sc->shape_lum[s] >= 0)
					return fail(c, MTSGPU_EINVAL, "shape %u: a cylinder cannot carry an area luminaire: Cylinder has no pdfArea, and Shape::pdfArea raises an error "
					            "on the first BSDF-sampled hit (shape.cpp:174-178), so the reference cannot render it either", s);
			} else if (SP[3] == 0.0f) return fail(c, MTSGPU_EINVAL, "shape %u: zero radius", s);
		}
		for (uint32_t t = sc->shape_tri_offset[s]; t < sc->shape_tri_offset[s + 1]; ++t) {
			const uint32_t k = sc->triaccel[12 * (size_t) t];
			if (mesh) {
				if (k == MTSGPU_KNOTRIANGLE) return fail(c, MTSGPU_EINVAL, "TriAccel %u: a mesh triangle is marked as a shape", t);
				for (int j = 0; j < 3; ++j)
					if (sc->tri_idx[3 * (size_t) t + j] >= sc->n_verts) return fail(c, MTSGPU_EINVAL, "triangle vertex index out of range");
			} else if (k != MTSGPU_KNOTRIANGLE) {
				return fail(c, MTSGPU_EINVAL, "TriAccel %u: the primitive of a non-mesh shape must have k = KNoTriangleFlag", t);
			}
			if (sc->triaccel[12 * (size_t) t + 10] != s) return fail(c, MTSGPU_EINVAL, "TriAccel %u: shape index does not match shape_tri_offset", t);
		}
	}
	for (uint32_t s = 0; s < sc->n_shapes; ++s) {
		if (sc->shape_bsdf[s] >= (int32_t) sc->n_bsdfs || sc->shape_lum[s] >= (int32_t) sc->n_lums) return fail(c, MTSGPU_EINVAL, "shape %u: bad BSDF/luminaire index", s);
		if (sc->shape_tri_offset[s] > sc->shape_tri_offset[s + 1]) return fail(c, MTSGPU_EINVAL, "shape_tri_offset not monotone");
		if (sc->shape_lum[s] >= 0 && (sc->lum_type[sc->shape_lum[s]] != MTSGPU_LUM_AREA || sc->lum_shape[sc->shape_lum[s]] != (int32_t) s))
			return fail(c, MTSGPU_EINVAL, "shape %u: luminaire link is inconsistent", s);
	}
	if (sc->shape_tri_offset[sc->n_shapes] != sc->n_tris) return fail(c, MTSGPU_EINVAL, "shape_tri_offset does not cover all triangles");
	for (uint32_t t = 0; t < sc->n_tris; ++t)
		if (sc->triaccel[12 * (size_t) t + 10] >= sc->n_shapes) return fail(c, MTSGPU_EINVAL, "TriAccel %u: shape index out of range", t);
	{
		const std::string why = checkBsdfTable(sc->n_bsdfs, sc->bsdf_type, sc->bsdf_params);
		if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
		// an anisotropic BSDF needs a tangent frame: spheres have one (dpdu / dpdv), a triangle mesh when the caller hands its
		// vertex tangents over.  Without them the reference renders a mesh that has no vertex normals with the frame it has
		// (trimesh.cpp:562-565); mtsgpu_upload_scene keeps refusing every such mesh
		for (uint32_t s = 0; s < sc->n_shapes; ++s) {
			const bool has = shape_has_tangents && shape_has_tangents[s];
			if (has && shapeType(s) != MTSGPU_SHAPE_TRIMESH) return fail(c, MTSGPU_EINVAL, "shape %u: only a triangle mesh can carry tangents", s);
			if (has && !(sc->shape_flags[s] & MTSGPU_SHAPE_HAS_NORMALS)) return fail(c, MTSGPU_EINVAL, "shape %u: tangents need vertex normals (trimesh.cpp:562-565)", s);
			if (has || !(sc->shape_bsdf[s] >= 0 && !shapeHasTangentFrame(shapeType(s)) && bsdfIsAnisotropic(sc->bsdf_type, sc->bsdf_params, (uint32_t) sc->shape_bsdf[s])))
				continue;
			if (!withTangents || (sc->shape_flags[s] & MTSGPU_SHAPE_HAS_NORMALS))
				return fail(c, MTSGPU_EINVAL, "%s", anisotropicOnMeshMessage(s).c_str());
		}
	}
	// the gather array of the tangents: dpdu of the three vertices of every primitive of a mesh that has them, zero elsewhere
	std::vector<float> triDpdu;
	std::vector<uint32_t> hasTan;
	{
		bool any = false;
		for (uint32_t s = 0; s < sc->n_shapes; ++s) any |= shape_has_tangents && shape_has_tangents[s];
		if (any) {
			triDpdu.assign(4 * (size_t) kTriDpduStride * ((size_t) sc->n_tris + 1), 0.0f);
			hasTan.assign((size_t) sc->n_shapes + 1, 0u);
			for (uint32_t s = 0; s < sc->n_shapes; ++s) {
				if (!shape_has_tangents[s]) continue;
				hasTan[s] = 1u;
				uint32_t v;      // the indices were checked above
				if (!gatherMeshRows(sc->tri_idx, sc->shape_tri_offset[s], sc->shape_tri_offset[s + 1], vtx_dpdu, 3, kTriDpduStride, triDpdu.data(), &v))
					return fail(c, MTSGPU_EINVAL, "shape %u: non-finite tangent at vertex %u", s, v);
			}
		}
	}
	float skyDerived[MTSGPU_SKY_NDERIVED] = { 0 };      // SkyLuminaire::configure() of the background sky, filled by its check
	for (uint32_t l = 0; l < sc->n_lums; ++l) {
		if (sc->lum_type[l] == MTSGPU_LUM_AREA) {
			const int32_t s = sc->lum_shape[l];
			if (s < 0 || s >= (int32_t) sc->n_shapes) return fail(c, MTSGPU_EINVAL, "luminaire %u: bad shape", l);
			const uint32_t n = sc->shape_tri_offset[s + 1] - sc->shape_tri_offset[s];
			if (shapeType((uint32_t) s) != MTSGPU_SHAPE_TRIMESH) {
				if (sc->lum_cdf_offset[l + 1] != sc->lum_cdf_offset[l]) return fail(c, MTSGPU_EINVAL, "luminaire %u: a non-mesh emitter has no triangle CDF", l);
			} else if (sc->lum_cdf_offset[l + 1] - sc->lum_cdf_offset[l] != n + 1) return fail(c, MTSGPU_EINVAL, "luminaire %u: CDF size mismatch", l);
		} else if (sc->lum_type[l] == MTSGPU_LUM_ENVMAP) {
			// everything env_triangle / env_pdf index with (envmap.cpp:123-193)
			if ((int32_t) l != sc->background_lum) return fail(c, MTSGPU_EINVAL, "luminaire %u: the envmap must be the background luminaire", l);
			const uint64_t np = (uint64_t) sc->env_pdf_width * sc->env_pdf_height;
			if (!sc->env_pixels || !sc->env_pdf || !sc->env_cdf || sc->env_width == 0 || sc->env_height == 0 || np == 0
			    || sc->env_width > 16384 || sc->env_height > 16384 || np > (1u << 26))
				return fail(c, MTSGPU_EINVAL, "luminaire %u: missing or oversized environment map", l);
			for (uint64_t i = 0; i < np; ++i)
				if (!(sc->env_cdf[i] <= sc->env_cdf[i + 1]) || !(sc->env_pdf[i] >= 0.0f)) return fail(c, MTSGPU_EINVAL, "luminaire %u: the environment map's CDF is not monotone", l);
			const float *LP = sc->lum_params + (size_t) MTSGPU_LUM_NPARAMS * l;
			for (int i = 0; i < 25; ++i) if (!std::isfinite(LP[i])) return fail(c, MTSGPU_EINVAL, "luminaire %u: non-finite parameter", l);
		} else if (sc->lum_type[l] == MTSGPU_LUM_SKY) {
			const std::string why = checkSkyLuminaire(l, sc->lum_params + (size_t) MTSGPU_LUM_NPARAMS * l, sc->background_lum, skyDerived);
			if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
		} else if (sc->lum_type[l] > MTSGPU_LUM_COLLIMATED) {
			return fail(c, MTSGPU_EINVAL, "luminaire %u: unknown type", l);
		}
	}
	if (sc->background_lum >= (int32_t) sc->n_lums) return fail(c, MTSGPU_EINVAL, "background luminaire out of range");

	freeAll(c->sceneAllocs);
	freeAll(c->colorAllocs);      // a new scene starts without vertex colours (mtsgpu_set_vertex_colors)
	c->dcol = DColors{ nullptr, nullptr };
	c->hostColorSlots.clear();
	freeAll(c->texAllocs);        // ... and without uv textures (mtsgpu_set_uv_textures, mtsgpu_set_uv_bitmap_textures)
	c->dtex = DTextures{ nullptr, nullptr, nullptr, nullptr };
	c->dmsk = DMasks{ nullptr };
	c->hostSlotTex.clear();
	c->hostMaskKind.clear();
	freeAll(c->snowAllocs);       // ... and without snow BRDFs (mtsgpu_set_snow_bsdfs)
	c->dsnw = DSnows{ nullptr };
	c->hostSnowKind.clear();
	freeAll(c->clothAllocs);      // ... and without cloth BRDFs (mtsgpu_set_cloth_bsdfs)
	c->dclo = DCloths{ nullptr, nullptr, nullptr, nullptr };
	c->hostClothWeave.clear();
	c->hostUvRange.clear();
	c->hostShapeHasUv.clear();
	c->dtan = DTangents{ nullptr, nullptr };      // ... and its tangents go with the scene's arrays
	c->haveScene = false;
	DScene d{};
	int rc = 0;
	{
		// Device node order.  The first trace_top_nodes() slots hold the root and the sibling pairs below it in
		// breadth-first order: k_trace keeps the first half of that prefix in LDS (kernels.h: kTopNodes).  After it,
		// 128-byte lines (16 nodes) are filled with breadth-first pieces of subtrees ("treelets") so that one L1 miss
		// serves several consecutive traversal steps.
		// The KDNode encoding is unchanged (siblings adjacent, relative offset to the left child,
		// gkdtree.h:442-470); only where a node lives changes, which traversal results do not depend on.
		const uint32_t N = sc->n_nodes;
		const uint32_t topSlots = trace_top_nodes();
		std::vector<uint32_t> newIndex(N, 0u);
		std::vector<uint32_t> stack, cand;           // entries: old index of the left node of a sibling pair
		auto leftOf = [&](uint32_t i) { return i + ((sc->kd_nodes[2 * (size_t) i] & 0x3FFFFFFCu) >> 2); };
		auto isLeaf = [&](uint32_t i) { return (sc->kd_nodes[2 * (size_t) i] & 0x80000000u) != 0; };
		uint32_t pos = 2;                            // slot 0 = root, slot 1 = padding
		newIndex[0] = 0;
		if (!isLeaf(0)) cand.push_back(leftOf(0));
		size_t head = 0;
		while (head < cand.size() || !stack.empty()) {
			if (head == cand.size()) { cand.clear(); head = 0; cand.push_back(stack.back()); stack.pop_back(); }
			const uint32_t l = cand[head++];
			newIndex[l] = pos; newIndex[l + 1] = pos + 1;
			pos += 2;
			for (uint32_t k = 0; k < 2; ++k)
				if (!isLeaf(l + k)) cand.push_back(leftOf(l + k));
			const bool full = pos < topSlots ? false : (pos == topSlots || (pos & 15u) == 0u);
			if (full) {
				// region full: the remaining frontier becomes the roots of later treelets (depth-first order)
				for (size_t k = cand.size(); k > head; --k) stack.push_back(cand[k - 1]);
				cand.clear(); head = 0;
			}
		}
		const uint32_t total = std::max<uint32_t>(pos, std::max(2u, topSlots));      // the LDS prefix is always there to copy
		if (total >= (1u << 29)) return fail(c, MTSGPU_EINVAL, "kd-tree too large");      // absolute child indices; k_trace's stack words keep node index * 2 below bit 30
		std::vector<uint32_t> dev(2 * (size_t) total, 0u);
		dev[2] = 0x80000000u; dev[3] = 0u;           // padding slot: empty leaf, never referenced
		for (uint32_t i = 0; i < N; ++i) {
			const uint32_t a = sc->kd_nodes[2 * (size_t) i], b = sc->kd_nodes[2 * (size_t) i + 1];
			uint32_t *o = &dev[2 * (size_t) newIndex[i]];
			if (a & 0x80000000u) { o[0] = a; o[1] = b; }
			else { o[0] = (a & 3u) | (newIndex[leftOf(i)] << 2); o[1] = b; }     // absolute left-child index (< 2^29)
		}
		rc |= upload(c, (const uint32_t **) &d.nodes, dev.data(), dev.size());
	}
	{
		// TriAccel records re-laid out in leaf order (one contiguous run per leaf, no index
		// indirection on the device); non-occluders are shapes without a BSDF
		// (Shape::isOccluder, shape.h:324)
		const size_t LS = 4 * (size_t) kLeafStride;                 // dwords per record slot
		// behind the records: four 16-byte rows per cylinder, worldToObject 3x4 and (radius, length, -, -) (kdevice.h); a
		// cylinder's record points at them with dword 4 = the index of the first row in units of 16 bytes
		std::vector<uint32_t> cylRow(sc->n_shapes, 0u);
		const size_t firstCylRow = (size_t) kLeafStride * ((size_t) sc->n_indices + 1);
		size_t nCyl = 0;
		for (uint32_t s = 0; s < sc->n_shapes; ++s)
			if (shapeType(s) == MTSGPU_SHAPE_CYLINDER) cylRow[s] = (uint32_t) (firstCylRow + 4 * nCyl++);
		if (firstCylRow + 4 * nCyl >= (1ull << 32)) return fail(c, MTSGPU_EINVAL, "too many leaf records");
		std::vector<uint32_t> ta(LS * ((size_t) sc->n_indices + 1) + 16 * nCyl, 0u);
		for (uint32_t s = 0; s < sc->n_shapes; ++s)
			if (shapeType(s) == MTSGPU_SHAPE_CYLINDER) {
				const float *D = cylinders + (size_t) MTSGPU_CYLINDER_NDERIVED * s;
				uint32_t *rows = &ta[4 * (size_t) cylRow[s]];
				std::memcpy(rows, D + 12, 48);
				std::memcpy(rows + 12, D + 24, 8);
			}
		for (uint32_t e = 0; e < sc->n_indices; ++e) {
			const uint32_t prim = sc->kd_indices[e];
			uint32_t *dst = &ta[LS * (size_t) e];
			std::memcpy(dst, sc->triaccel + 12 * (size_t) prim, 48);
			// dword 0 = k<<30 | non-occluder<<29 | primitive id (the head of the record decides everything
			// up to the plane distance); dword 10 stays the shape index
			if (prim >= (1u << 28)) return fail(c, MTSGPU_EINVAL, "more than 2^28 primitives");
			const bool isShape = dst[0] == MTSGPU_KNOTRIANGLE;
			dst[0] = (std::min(dst[0], 3u) << 30) | (sc->shape_bsdf[dst[10]] < 0 ? 0x20000000u : 0u) | prim;
			dst[11] = 0;
			if ((dst[0] >> 30) == 3u) {
				// k == 3: a degenerate triangle (dword 1 = 0) or a non-triangle shape (dword 1 = shape type,
				// dwords 4..7 = centre and radius of the sphere)
				dst[1] = 0;
				if (isShape) {
					const float *SP = sc->shape_params + (size_t) MTSGPU_SHAPE_NPARAMS * dst[10];
					dst[1] = shapeType(dst[10]);
					std::memcpy(dst + 4, SP, 16);
					if (dst[1] == MTSGPU_SHAPE_CYLINDER) dst[4] = cylRow[dst[10]];
				}
			}
		}
		rc |= upload(c, (const uint32_t **) &d.leaf_ta, ta.data(), ta.size());
		// per-primitive position / normal records for the shading kernels
		const size_t TS = 4 * (size_t) kTriStride;                    // floats per record (one 128-byte line)
		std::vector<float> triRec(TS * ((size_t) sc->n_tris + 1), 0.0f);
		for (uint32_t s = 0; s < sc->n_shapes; ++s)
			for (uint32_t t = sc->shape_tri_offset[s]; t < sc->shape_tri_offset[s + 1]; ++t) {
				float *P = &triRec[TS * (size_t) t], *Nn = P + 12;
				if (shapeType(s) != MTSGPU_SHAPE_TRIMESH) {
					// non-mesh shape: centre + radius, flag bit 31 (the rest comes from shape_params)
					// (bit 30: the shape is a cylinder, whose record fill_its builds from its own layout of shape_params)
					const uint32_t flags = sc->shape_flags[s] | 0x80000000u | (shapeType(s) == MTSGPU_SHAPE_CYLINDER ? 0x40000000u : 0u);
					std::memcpy(P, sc->shape_params + (size_t) MTSGPU_SHAPE_NPARAMS * s, 16);
					std::memcpy(P + 10, &s, 4); std::memcpy(P + 11, &flags, 4);
					continue;
				}
				for (int k = 0; k < 3; ++k) {
					const uint32_t v = sc->tri_idx[3 * (size_t) t + k];
					std::memcpy(P + 3 * k, sc->vtx_pos + 3 * (size_t) v, 12);
					std::memcpy(Nn + 3 * k, sc->vtx_nrm + 3 * (size_t) v, 12);
				}
				const uint32_t flags = sc->shape_flags[s];
				std::memcpy(P + 10, &s, 4); std::memcpy(P + 11, &flags, 4);
			}
		rc |= upload(c, (const float **) &d.tri_pos, triRec.data(), triRec.size());
		d.tri_nrm = d.tri_pos ? d.tri_pos + 3 : nullptr;
	}
	rc |= upload(c, &d.shape_bsdf, sc->shape_bsdf, sc->n_shapes);
	rc |= upload(c, &d.shape_lum, sc->shape_lum, sc->n_shapes);
	rc |= upload(c, &d.shape_flags, sc->shape_flags, sc->n_shapes);
	{
		std::vector<uint32_t> bin(sc->n_shapes + 1, (uint32_t) kNumBsdfTypes);
		for (uint32_t sIdx = 0; sIdx < sc->n_shapes; ++sIdx)
			if (sc->shape_bsdf[sIdx] >= 0) bin[sIdx] = sc->bsdf_type[sc->shape_bsdf[sIdx]] & 0xFFu;
		rc |= upload(c, &d.shape_bin, bin.data(), bin.size());
	}
	{
		std::vector<uint32_t> st(sc->n_shapes + 1, (uint32_t) MTSGPU_SHAPE_TRIMESH);
		std::vector<float> sp((size_t) MTSGPU_SHAPE_NPARAMS * (sc->n_shapes + 1), 0.0f);
		if (sc->shape_type) {
			std::copy(sc->shape_type, sc->shape_type + sc->n_shapes, st.begin());
			std::copy(sc->shape_params, sc->shape_params + (size_t) MTSGPU_SHAPE_NPARAMS * sc->n_shapes, sp.begin());
		}
		// a cylinder's device row, what the shading reads (shade_bsdf.h): [0..11] worldToObject 3x4, [12..20] the 3x3 of
		// objectToWorld, [21] length, [22] radius, [23] 1 / area
		for (uint32_t s = 0; s < sc->n_shapes; ++s)
			if (shapeType(s) == MTSGPU_SHAPE_CYLINDER) {
				const float *D = cylinders + (size_t) MTSGPU_CYLINDER_NDERIVED * s;
				float *P = &sp[(size_t) MTSGPU_SHAPE_NPARAMS * s];
				std::memcpy(P, D + 12, 48);
				for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) P[12 + 3 * i + j] = D[4 * i + j];
				P[21] = D[25]; P[22] = D[24]; P[23] = D[26];
			}
		rc |= upload(c, &d.shape_type, st.data(), st.size());
		rc |= upload(c, &d.shape_params, sp.data(), sp.size());
	}
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
	if (sc->background_lum >= 0 && sc->lum_type[sc->background_lum] == MTSGPU_LUM_SKY) {
		// what SkyLuminaire::configure() derives (sky.cpp:139-179), once per scene
		rc |= upload(c, (const float **) &d.sky, (const float *) skyDerived, (size_t) MTSGPU_SKY_NDERIVED);
	}
	const float *dDpdu = nullptr; const uint32_t *dHasTan = nullptr;
	if (!triDpdu.empty()) {
		rc |= upload(c, &dDpdu, triDpdu.data(), triDpdu.size());
		rc |= upload(c, &dHasTan, hasTan.data(), hasTan.size());
	}
	if (rc) { freeAll(c->sceneAllocs); return rc; }
	c->dtan = DTangents{ reinterpret_cast<const float4 *>(dDpdu), dHasTan };
	d.lum_sel_sum = sc->lum_sel_sum; d.background_lum = sc->background_lum;
	d.has_shapes = 0;
	for (uint32_t s = 0; s < sc->n_shapes; ++s) if (shapeType(s) != MTSGPU_SHAPE_TRIMESH) d.has_shapes = kHasShapes;
	for (uint32_t s = 0; s < sc->n_shapes; ++s) if (shapeType(s) == MTSGPU_SHAPE_CYLINDER) d.has_shapes = kHasCylinders;      // the CYL kernels of trace.hip
	d.n_lums = sc->n_lums; d.n_nodes = sc->n_nodes; d.n_tris = sc->n_tris; d.n_shapes = sc->n_shapes;
	for (int a = 0; a < 3; ++a) { d.aabb_min[a] = sc->aabb_min[a]; d.aabb_max[a] = sc->aabb_max[a]; }
	c->dsc = d; c->nTris = sc->n_tris;
	{
		mtsgpu_ctx::HostScene &h = c->host;
		h.nVerts = sc->n_verts;
		h.triIdx.assign(sc->tri_idx, sc->tri_idx + 3 * (size_t) sc->n_tris);
		h.shapeTriOffset.assign(sc->shape_tri_offset, sc->shape_tri_offset + sc->n_shapes + 1);
		h.shapeType.assign(sc->n_shapes, (uint32_t) MTSGPU_SHAPE_TRIMESH);
		if (sc->shape_type) h.shapeType.assign(sc->shape_type, sc->shape_type + sc->n_shapes);
		h.bsdfType.assign(sc->bsdf_type, sc->bsdf_type + sc->n_bsdfs);
		h.bsdfParams.assign(sc->bsdf_params, sc->bsdf_params + (size_t) MTSGPU_BSDF_NPARAMS * sc->n_bsdfs);
		h.shapeBsdf.assign(sc->shape_bsdf, sc->shape_bsdf + sc->n_shapes);
		h.lumType.assign(sc->lum_type, sc->lum_type + sc->n_lums);
		h.shapeNormals.assign(sc->n_shapes, 0u);
		h.shapeTangents.assign(sc->n_shapes, 0u);
		for (uint32_t s = 0; s < sc->n_shapes; ++s) {
			h.shapeNormals[s] = (sc->shape_flags[s] & MTSGPU_SHAPE_HAS_NORMALS) ? 1u : 0u;
			h.shapeTangents[s] = (shape_has_tangents && shape_has_tangents[s]) ? 1u : 0u;
		}
	}
	// material queues that can ever be non-empty: the BSDF types of shapes that have one, and the "terminal" bin
	c->binMask = 1u << kNumBsdfTypes;
	for (uint32_t sIdx = 0; sIdx < sc->n_shapes; ++sIdx)
		if (sc->shape_bsdf[sIdx] >= 0) c->binMask |= 1u << (sc->bsdf_type[sc->shape_bsdf[sIdx]] & 0xFFu);
	c->haveScene = true;
	return 0;
}

int mtsgpu_upload_scene(mtsgpu_ctx *c, const mtsgpu_scene *sc) { return uploadScene(c, sc, nullptr, nullptr, false); }

int mtsgpu_upload_scene_cylinders(mtsgpu_ctx *c, const mtsgpu_scene *sc, const float *vtx_dpdu, const uint32_t *shape_has_tangents, const float *cylinders) {
	if ((vtx_dpdu == nullptr) != (shape_has_tangents == nullptr))
		return fail(c, MTSGPU_EINVAL, "vtx_dpdu and shape_has_tangents must both be given or both be NULL");
	return uploadScene(c, sc, vtx_dpdu, shape_has_tangents, true, cylinders, true);
}

int mtsgpu_upload_scene_tangents(mtsgpu_ctx *c, const mtsgpu_scene *sc, const float *vtx_dpdu, const uint32_t *shape_has_tangents) {
	if ((vtx_dpdu == nullptr) != (shape_has_tangents == nullptr))
		return fail(c, MTSGPU_EINVAL, "vtx_dpdu and shape_has_tangents must both be given or both be NULL");
	return uploadScene(c, sc, vtx_dpdu, shape_has_tangents, true);
}

// the slot tables of the host (host.h) and of the kernels (kernels.h) are one table
constexpr bool colorSlotTablesAgree() {
	for (int t = 0; t < MTSGPU_BSDF_NTYPES; ++t)
		for (int k = 0; k < 2; ++k)
			if (kBsdfColorSlotOffset[t][k] != bsdf_color_slot_offset(t, k)) return false;
	return true;
}
static_assert(colorSlotTablesAgree(), "BSDF colour slot tables differ");

int mtsgpu_set_vertex_colors(mtsgpu_ctx *c, const float *vtx_col, const uint32_t *shape_has_colors, const uint32_t *bsdf_color_slots) {
	if (!c) return fail(c, MTSGPU_EINVAL, "null argument");
	if (!c->haveScene) return fail(c, MTSGPU_ESTATE, "mtsgpu_set_vertex_colors before mtsgpu_upload_scene");
	c->lastPass.valid = false;
	HIPCHK(c, hipSetDevice(c->device));
	// nothing may still read the arrays that go (the shading launches of a render that was not synchronised)
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
	freeAll(c->colorAllocs);
	c->dcol = DColors{ nullptr, nullptr };
	c->hostColorSlots.clear();
	if (!vtx_col && !shape_has_colors && !bsdf_color_slots) return 0;
	if ((vtx_col == nullptr) != (shape_has_colors == nullptr))
		return fail(c, MTSGPU_EINVAL, "vtx_col and shape_has_colors must both be given or both be NULL");
	const mtsgpu_ctx::HostScene &h = c->host;
	const uint32_t nShapes = (uint32_t) h.shapeBsdf.size(), nBsdfs = (uint32_t) h.bsdfType.size();
	bool anySlot = false;
	if (bsdf_color_slots) {
		const std::string why = checkBsdfColorSlots(nBsdfs, h.bsdfType.data(), h.bsdfParams.data(), bsdf_color_slots);
		if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
		if (!c->hostSlotTex.empty())      // a slot mtsgpu_set_uv_textures has given a texture
			for (uint32_t b = 0; b < nBsdfs; ++b)
				for (int s = 0; s < 2; ++s)
					if (((bsdf_color_slots[b] >> s) & 1u) && c->hostSlotTex[2 * (size_t) b + s] >= 0)
						return fail(c, MTSGPU_EINVAL, "BSDF %u: slot %d takes vertex colours and has a uv texture as well", b, s);
		for (uint32_t b = 0; b < nBsdfs && !c->hostSnowKind.empty(); ++b)      // an entry mtsgpu_set_snow_bsdfs has given a snow record
			if (bsdf_color_slots[b] && c->hostSnowKind[b] != (uint32_t) MTSGPU_SNOW_NONE)
				return fail(c, MTSGPU_EINVAL, "BSDF %u: the entry takes vertex colours and has a snow record, whose BRDF has no texture slot", b);
		for (uint32_t b = 0; b < nBsdfs && !c->hostClothWeave.empty(); ++b)      // an entry mtsgpu_set_cloth_bsdfs has given a weave
			if (bsdf_color_slots[b] && c->hostClothWeave[b] >= 0)
				return fail(c, MTSGPU_EINVAL, "BSDF %u: the entry takes vertex colours and has a weave, whose BRDF has no texture slot", b);
		for (uint32_t s = 0; s < nShapes; ++s) {
			const int32_t b = h.shapeBsdf[s];
			if (b < 0 || !bsdf_color_slots[b]) continue;
			if (h.shapeType[s] != MTSGPU_SHAPE_TRIMESH)
				return fail(c, MTSGPU_EINVAL, "shape %u: BSDF %d takes vertex colours, but a sphere has none (its.color would be read unwritten, shape.h:162-163)", s, b);
			if (!shape_has_colors || !shape_has_colors[s])
				return fail(c, MTSGPU_EINVAL, "shape %u: BSDF %d takes vertex colours, but the mesh has none (its.color would be read unwritten, shape.h:162-163)", s, b);
		}
		for (uint32_t b = 0; b < nBsdfs; ++b) anySlot |= bsdf_color_slots[b] != 0;
	}
	if (!vtx_col) return 0;       // masks that are all zero and no colours: nothing to keep
	// the gather array: the colours of the three vertices of every primitive of a coloured mesh, zero elsewhere
	std::vector<float> triCol(4 * (size_t) kTriColStride * ((size_t) c->nTris + 1), 0.0f);
	bool anyColors = false;
	for (uint32_t s = 0; s < nShapes; ++s) {
		if (!shape_has_colors[s]) continue;
		if (h.shapeType[s] != MTSGPU_SHAPE_TRIMESH) return fail(c, MTSGPU_EINVAL, "shape %u: only a triangle mesh can carry vertex colours", s);
		anyColors = true;
		uint32_t v;
		if (!gatherMeshRows(h.triIdx.data(), h.shapeTriOffset[s], h.shapeTriOffset[s + 1], vtx_col, 3, kTriColStride, triCol.data(), &v))
			return fail(c, MTSGPU_EINVAL, "shape %u: non-finite colour at vertex %u", s, v);
	}
	if (!anyColors) return 0;
	const float *dCol = nullptr; const uint32_t *dSlots = nullptr;
	int rc = upload(c, &dCol, triCol.data(), triCol.size(), &c->colorAllocs);
	if (!rc && anySlot) rc = upload(c, &dSlots, bsdf_color_slots, nBsdfs, &c->colorAllocs);
	if (rc) { freeAll(c->colorAllocs); return rc; }
	c->dcol = DColors{ reinterpret_cast<const float4 *>(dCol), dSlots };
	if (anySlot) c->hostColorSlots.assign(bsdf_color_slots, bsdf_color_slots + nBsdfs);
	return 0;
}

static_assert(sizeof(mtsgpu_uv_texture) == sizeof(DTexture) && offsetof(mtsgpu_uv_texture, line_width) == offsetof(DTexture, line_width)
              && offsetof(mtsgpu_uv_texture, bright) == offsetof(DTexture, bright), "mtsgpu_uv_texture and DTexture are one layout");
static_assert(MTSGPU_TEX_CHECKERBOARD == (int) kTexCheckerboard && MTSGPU_TEX_GRID == (int) kTexGrid, "texture kinds differ");
static_assert(MTSGPU_TEX_BITMAP == (int) kTexBitmap && offsetof(DTexture, width) == offsetof(mtsgpu_uv_texture, bright)
              && offsetof(DTexture, reserved) + sizeof(DTexture::reserved) == sizeof(DTexture), "the bitmap words are the seven behind vscale");
static_assert(sizeof(mtsgpu_bsdf_mask) == sizeof(DMask) && offsetof(mtsgpu_bsdf_mask, opacity) == offsetof(DMask, opacity)
              && offsetof(mtsgpu_bsdf_mask, texture) == offsetof(DMask, texture), "mtsgpu_bsdf_mask and DMask are one layout");
static_assert(MTSGPU_MASK_NONE == (int) kMaskNone && MTSGPU_MASK_CONSTANT == (int) kMaskConstant && MTSGPU_MASK_TEXTURE == (int) kMaskTexture,
              "mask kinds differ");
static_assert(MTSGPU_WRAP_REPEAT == (int) kWrapRepeat && MTSGPU_WRAP_CLAMP == (int) kWrapClamp && MTSGPU_WRAP_BLACK == (int) kWrapBlack
              && MTSGPU_WRAP_WHITE == (int) kWrapWhite, "wrap modes differ");

// 2 * uv' of texture t at texcoord (u, v) stays inside the range of the reference's (int) cast, with the margin the header states
// (a bitmap of sx x sy texels: uv' * (sx, sy), mipmap.cpp:229-230)
static bool uvCastInRange(const mtsgpu_uv_texture &t, float u, float v, double sx = 2.0, double sy = 2.0) {
	const double lim = 2147483648.0 - 65536.0;
	const double x = sx * ((double) u * t.uscale + t.uoffset), y = sy * ((double) v * t.vscale + t.voffset);
	return std::fabs(x) < lim && std::fabs(y) < lim;
}

// mtsgpu_set_uv_textures (withBitmaps = false: no bitmaps, and kind MTSGPU_TEX_BITMAP is unknown), mtsgpu_set_uv_bitmap_textures
// and mtsgpu_set_uv_masked_textures (me: the caller's name; bsdf_mask: only the last one has a table)
static int setUvTextures(mtsgpu_ctx *c, const float *vtx_uv, const uint32_t *shape_has_uv, uint32_t n_textures,
                         const mtsgpu_uv_texture *textures, const int32_t *bsdf_slot_texture, uint32_t n_bitmaps,
                         const mtsgpu_bitmap *bitmaps, const int32_t *texture_bitmap, bool withBitmaps, const char *me,
                         const mtsgpu_bsdf_mask *bsdf_mask = nullptr) {
	if (!c) return fail(c, MTSGPU_EINVAL, "null argument");
	if (!c->haveScene) return fail(c, MTSGPU_ESTATE, "%s before mtsgpu_upload_scene", me);
	// an entry mtsgpu_set_cloth_bsdfs has given a weave takes neither a textured slot nor a mask; and the cloth table was
	// checked against the texcoords that go with this call, so a texture call while one is in force is refused before anything
	// is freed (the cloth kernels read the uv array): the order is the texture call first (mtsgpu_cloth.h)
	for (uint32_t b = 0; b < (uint32_t) c->host.bsdfType.size() && !c->hostClothWeave.empty(); ++b) {
		if (c->hostClothWeave[b] < 0) continue;
		if (bsdf_slot_texture && (bsdf_slot_texture[2 * (size_t) b] >= 0 || bsdf_slot_texture[2 * (size_t) b + 1] >= 0))
			return fail(c, MTSGPU_EINVAL, "BSDF %u: the entry has a uv texture and a weave, whose BRDF has no texture slot", b);
		if (bsdf_mask && bsdf_mask[b].kind != (uint32_t) MTSGPU_MASK_NONE)
			return fail(c, MTSGPU_EINVAL, "BSDF %u: the entry has a mask and a weave: a mask around a cloth BRDF is not supported", b);
	}
	if (!c->hostClothWeave.empty())
		return fail(c, MTSGPU_EINVAL, "%s while a cloth table is in force: the texture call comes first (switch the table off with mtsgpu_set_cloth_bsdfs(ctx, 0, NULL, NULL))", me);
	c->lastPass.valid = false;
	HIPCHK(c, hipSetDevice(c->device));
	// nothing may still read the arrays that go (the shading launches of a render that was not synchronised)
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
	freeAll(c->texAllocs);
	c->dtex = DTextures{ nullptr, nullptr, nullptr, nullptr };
	c->dmsk = DMasks{ nullptr };
	c->hostSlotTex.clear();
	c->hostMaskKind.clear();
	c->hostUvRange.clear();
	c->hostShapeHasUv.clear();
	if (!vtx_uv && !shape_has_uv && !textures && !bsdf_slot_texture && !bitmaps && !texture_bitmap && !bsdf_mask) return 0;
	if ((vtx_uv == nullptr) != (shape_has_uv == nullptr))
		return fail(c, MTSGPU_EINVAL, "vtx_uv and shape_has_uv must both be given or both be NULL");
	if (n_textures && !textures) return fail(c, MTSGPU_EINVAL, "n_textures without textures");
	if (n_textures > (1u << 20)) return fail(c, MTSGPU_EINVAL, "at most 2^20 textures");
	if (n_bitmaps && !bitmaps) return fail(c, MTSGPU_EINVAL, "n_bitmaps without bitmaps");
	if (n_bitmaps > (1u << 20)) return fail(c, MTSGPU_EINVAL, "at most 2^20 bitmaps");
	const mtsgpu_ctx::HostScene &h = c->host;
	const uint32_t nShapes = (uint32_t) h.shapeBsdf.size(), nBsdfs = (uint32_t) h.bsdfType.size();
	for (uint32_t k = 0; k < n_textures; ++k) {
		const std::string why = checkUvTexture(textures[k], withBitmaps);
		if (!why.empty()) return fail(c, MTSGPU_EINVAL, "texture %u: %s", k, why.c_str());
	}
	// the bitmaps, the place of each in the pool, and the descriptors of the textures that show one
	std::vector<uint32_t> first(n_bitmaps, 0u);
	uint64_t nTexels = 0;
	for (uint32_t b = 0; b < n_bitmaps; ++b) {
		first[b] = (uint32_t) nTexels;
		const std::string why = checkBitmap(bitmaps[b], &nTexels);
		if (!why.empty()) return fail(c, MTSGPU_EINVAL, "bitmap %u: %s", b, why.c_str());
	}
	std::vector<DTexture> desc(n_textures);
	bool anyBitmap = false;
	for (uint32_t k = 0; k < n_textures; ++k) {
		std::memcpy(&desc[k], &textures[k], sizeof(DTexture));
		if (textures[k].kind != (uint32_t) MTSGPU_TEX_BITMAP) continue;
		const int32_t b = texture_bitmap ? texture_bitmap[k] : -1;
		if (b < 0 || (uint32_t) b >= n_bitmaps) return fail(c, MTSGPU_EINVAL, "texture %u: bitmap index %d out of range (%u bitmaps)", k, b, n_bitmaps);
		desc[k].width = bitmaps[b].width; desc[k].height = bitmaps[b].height; desc[k].wrap = bitmaps[b].wrap_mode; desc[k].first = first[b];
		desc[k].reserved[0] = desc[k].reserved[1] = desc[k].reserved[2] = 0u;
		anyBitmap = true;
	}
	bool anySlot = false;
	if (bsdf_slot_texture) {
		const std::string why = checkBsdfSlotTextures(nBsdfs, h.bsdfType.data(), h.bsdfParams.data(), bsdf_slot_texture, n_textures,
		                                              c->hostColorSlots.empty() ? nullptr : c->hostColorSlots.data());
		if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
		for (size_t i = 0; i < 2 * (size_t) nBsdfs; ++i) anySlot |= bsdf_slot_texture[i] >= 0;
	}
	bool anyMask = false, anyMaskTex = false;
	if (bsdf_mask && c->dsc.has_shapes == kHasCylinders)
		for (uint32_t b = 0; b < nBsdfs; ++b)
			if (bsdf_mask[b].kind != (uint32_t) MTSGPU_MASK_NONE)
				return fail(c, MTSGPU_EINVAL, "BSDF %u: the mask BSDF is not served in a scene with a cylinder yet (the mask kernels do not build a cylinder's record)", b);
	if (bsdf_mask) {
		const std::string why = checkBsdfMasks(nBsdfs, h.bsdfType.data(), h.bsdfParams.data(), bsdf_mask, n_textures);
		if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
		for (uint32_t b = 0; b < nBsdfs; ++b) {
			anyMask |= bsdf_mask[b].kind != (uint32_t) MTSGPU_MASK_NONE;
			anyMaskTex |= bsdf_mask[b].kind == (uint32_t) MTSGPU_MASK_TEXTURE;
		}
	}
	// an entry mtsgpu_set_snow_bsdfs has given a snow record takes neither a textured slot nor a mask
	for (uint32_t b = 0; b < nBsdfs && !c->hostSnowKind.empty(); ++b) {
		if (c->hostSnowKind[b] == (uint32_t) MTSGPU_SNOW_NONE) continue;
		if (bsdf_slot_texture && (bsdf_slot_texture[2 * (size_t) b] >= 0 || bsdf_slot_texture[2 * (size_t) b + 1] >= 0))
			return fail(c, MTSGPU_EINVAL, "BSDF %u: the entry has a uv texture and a snow record, whose BRDF has no texture slot", b);
		if (bsdf_mask && bsdf_mask[b].kind != (uint32_t) MTSGPU_MASK_NONE)
			return fail(c, MTSGPU_EINVAL, "BSDF %u: the entry has a mask and a snow record: a mask around a snow BRDF is not supported", b);
	}
	// the casts of texture k on shape s (s == nShapes: on no shape, at uv = 0); the reason, or an empty string
	auto castRange = [&](uint32_t s, int32_t k, const std::vector<float> &triUv) -> std::string {
		const size_t US = 4 * (size_t) kTriUvStride;
		bool ok = true;
		const bool bitmap = textures[k].kind == (uint32_t) MTSGPU_TEX_BITMAP;
		const double sx = bitmap ? (double) desc[k].width : 2.0, sy = bitmap ? (double) desc[k].height : 2.0;
		const bool mesh = s < nShapes && h.shapeType[s] == MTSGPU_SHAPE_TRIMESH, hasUv = s < nShapes && shape_has_uv && shape_has_uv[s];
		if (s < nShapes && !mesh) ok = uvCastInRange(textures[k], 0.0f, 0.0f, sx, sy) && uvCastInRange(textures[k], 1.0f, 1.0f, sx, sy);
		else if (!hasUv) ok = uvCastInRange(textures[k], 0.0f, 0.0f, sx, sy);
		else
			for (uint32_t t = h.shapeTriOffset[s]; ok && t < h.shapeTriOffset[s + 1]; ++t)
				for (int v = 0; v < 3; ++v)
					ok = ok && uvCastInRange(textures[k], triUv[US * (size_t) t + 2 * v], triUv[US * (size_t) t + 2 * v + 1], sx, sy);
		if (ok) return std::string();
		return "texture " + std::to_string(k) + " maps a texcoord outside the range of the (int) cast ("
		       + (bitmap ? "|uv' * size|" : "|2 uv'|") + " >= 2^31 - 2^16)";
	};
	// the gather array: the texcoords of the three vertices of every primitive of a mesh that has them, zero elsewhere
	const size_t US = 4 * (size_t) kTriUvStride;
	std::vector<float> triUv(US * ((size_t) c->nTris + 1), 0.0f);
	for (uint32_t s = 0; s < nShapes; ++s) {
		const bool hasUv = shape_has_uv && shape_has_uv[s];
		const bool mesh = h.shapeType[s] == MTSGPU_SHAPE_TRIMESH;
		if (hasUv && !mesh) return fail(c, MTSGPU_EINVAL, "shape %u: only a triangle mesh can carry texture coordinates", s);
		uint32_t bad;
		if (hasUv && !gatherMeshRows(h.triIdx.data(), h.shapeTriOffset[s], h.shapeTriOffset[s + 1], vtx_uv, 2, kTriUvStride, triUv.data(), &bad))
			return fail(c, MTSGPU_EINVAL, "shape %u: non-finite texcoord at vertex %u", s, bad);
		// the casts of the textures this shape is shaded with
		const int32_t b = h.shapeBsdf[s];
		if (b < 0) continue;
		for (int slot = 0; bsdf_slot_texture && slot < 2; ++slot) {
			const int32_t k = bsdf_slot_texture[2 * (size_t) b + slot];
			if (k < 0) continue;
			const std::string why = castRange(s, k, triUv);
			if (!why.empty()) return fail(c, MTSGPU_EINVAL, "shape %u: %s", s, why.c_str());
		}
		// ... and of the texture its mask reads
		if (bsdf_mask && bsdf_mask[b].kind == (uint32_t) MTSGPU_MASK_TEXTURE) {
			const std::string why = castRange(s, bsdf_mask[b].texture, triUv);
			if (!why.empty()) return fail(c, MTSGPU_EINVAL, "shape %u: BSDF %d: the opacity of its mask: %s", s, b, why.c_str());
		}
	}
	// a textured mask on a BSDF that no shape uses: the texture's offsets alone
	if (anyMaskTex) {
		std::vector<bool> used(nBsdfs, false);
		for (uint32_t s = 0; s < nShapes; ++s)
			if (h.shapeBsdf[s] >= 0) used[h.shapeBsdf[s]] = true;
		for (uint32_t b = 0; b < nBsdfs; ++b) {
			if (used[b] || bsdf_mask[b].kind != (uint32_t) MTSGPU_MASK_TEXTURE) continue;
			const std::string why = castRange(nShapes, bsdf_mask[b].texture, triUv);
			if (!why.empty()) return fail(c, MTSGPU_EINVAL, "BSDF %u: the opacity of its mask: %s", b, why.c_str());
		}
	}
	if (!anySlot && !vtx_uv && !anyMask) return 0;       // nothing to keep
	const float *dUv = nullptr, *dTexels = nullptr; const DTexture *dTex = nullptr; const int32_t *dSlots = nullptr;
	int rc = upload(c, &dUv, triUv.data(), triUv.size(), &c->texAllocs);
	// (a mask keeps the textures and the bitmaps when no slot uses them)
	if (!rc && (anySlot || anyMaskTex)) rc = upload(c, &dTex, desc.data(), n_textures, &c->texAllocs);
	if (!rc && anySlot) rc = upload(c, &dSlots, bsdf_slot_texture, 2 * (size_t) nBsdfs, &c->texAllocs);
	const DMask *dMask = nullptr;
	if (!rc && anyMask) rc = upload(c, &dMask, reinterpret_cast<const DMask *>(bsdf_mask), nBsdfs, &c->texAllocs);
	if (!rc && (anySlot || anyMaskTex) && anyBitmap) {
		// the pool: the bitmaps one behind the other, 16 bytes per texel
		std::vector<float> pool(4 * (size_t) nTexels);
		for (uint32_t b = 0; b < n_bitmaps; ++b) packBitmapTexels(bitmaps[b], &pool[4 * (size_t) first[b]]);
		rc = upload(c, &dTexels, pool.data(), pool.size(), &c->texAllocs);
	}
	if (rc) { freeAll(c->texAllocs); return rc; }
	c->dtex = DTextures{ reinterpret_cast<const float4 *>(dUv), dTex, dSlots, reinterpret_cast<const float4 *>(dTexels) };
	c->dmsk = DMasks{ dMask };
	if (anySlot) c->hostSlotTex.assign(bsdf_slot_texture, bsdf_slot_texture + 2 * (size_t) nBsdfs);
	if (vtx_uv) {
		// what mtsgpu_set_cloth_bsdfs checks its casts on: the extremes of every shape's texcoords
		c->hostShapeHasUv.assign(shape_has_uv, shape_has_uv + nShapes);
		c->hostUvRange.assign(4 * (size_t) nShapes, 0.0);
		for (uint32_t s = 0; s < nShapes; ++s) {
			if (!shape_has_uv[s]) continue;
			double *r = &c->hostUvRange[4 * (size_t) s];
			bool first = true;
			for (uint32_t t = h.shapeTriOffset[s]; t < h.shapeTriOffset[s + 1]; ++t)
				for (int v = 0; v < 3; ++v) {
					const double u = triUv[US * (size_t) t + 2 * v], w = triUv[US * (size_t) t + 2 * v + 1];
					if (first) { r[0] = r[1] = u; r[2] = r[3] = w; first = false; }
					r[0] = std::min(r[0], u); r[1] = std::max(r[1], u); r[2] = std::min(r[2], w); r[3] = std::max(r[3], w);
				}
		}
	}
	if (anyMask)
		for (uint32_t b = 0; b < nBsdfs; ++b) c->hostMaskKind.push_back(bsdf_mask[b].kind);
	return 0;
}

static_assert(sizeof(mtsgpu_bsdf_snow) == 64 && sizeof(mtsgpu_bsdf_snow) == sizeof(DSnow) && offsetof(mtsgpu_bsdf_snow, derived) == offsetof(DSnow, derived)
              && offsetof(mtsgpu_bsdf_snow, derived) == 8, "mtsgpu_bsdf_snow and DSnow are one layout");
static_assert(MTSGPU_SNOW_NONE == (int) kSnowNone && MTSGPU_SNOW_WISCOMBE == (int) kSnowWiscombe && MTSGPU_SNOW_HK == (int) kSnowHK, "snow kinds differ");

int mtsgpu_set_snow_bsdfs(mtsgpu_ctx *c, const mtsgpu_bsdf_snow *table) {
	if (!c) return fail(c, MTSGPU_EINVAL, "null argument");
	if (!c->haveScene) return fail(c, MTSGPU_ESTATE, "mtsgpu_set_snow_bsdfs before mtsgpu_upload_scene");
	c->lastPass.valid = false;
	HIPCHK(c, hipSetDevice(c->device));
	// nothing may still read the table that goes (the shading launches of a render that was not synchronised)
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
	freeAll(c->snowAllocs);
	c->dsnw = DSnows{ nullptr };
	c->hostSnowKind.clear();
	if (!table) return 0;
	if (c->dsc.has_shapes == kHasCylinders)
		return fail(c, MTSGPU_EINVAL, "the snow BRDFs are not served in a scene with a cylinder yet (the snow kernels do not build a cylinder's record)");
	const mtsgpu_ctx::HostScene &h = c->host;
	const uint32_t nBsdfs = (uint32_t) h.bsdfType.size();
	const std::string why = checkBsdfSnow(nBsdfs, h.bsdfType.data(), h.bsdfParams.data(), table,
	                                      c->hostColorSlots.empty() ? nullptr : c->hostColorSlots.data(),
	                                      c->hostSlotTex.empty() ? nullptr : c->hostSlotTex.data(),
	                                      c->hostMaskKind.empty() ? nullptr : c->hostMaskKind.data());
	if (!why.empty()) return fail(c, MTSGPU_EINVAL, "%s", why.c_str());
	for (uint32_t b = 0; b < nBsdfs && !c->hostClothWeave.empty(); ++b)      // an entry mtsgpu_set_cloth_bsdfs has given a weave
		if (table[b].kind != (uint32_t) MTSGPU_SNOW_NONE && c->hostClothWeave[b] >= 0)
			return fail(c, MTSGPU_EINVAL, "BSDF %u: the entry has a weave and a snow record", b);
	bool any = false;
	for (uint32_t b = 0; b < nBsdfs; ++b) any |= table[b].kind != (uint32_t) MTSGPU_SNOW_NONE;
	if (!any) return 0;           // nothing to keep: the context launches what it launches without a table
	const DSnow *dSnow = nullptr;
	if (int rc = upload(c, &dSnow, reinterpret_cast<const DSnow *>(table), nBsdfs, &c->snowAllocs)) { freeAll(c->snowAllocs); return rc; }
	c->dsnw = DSnows{ dSnow };
	for (uint32_t b = 0; b < nBsdfs; ++b) c->hostSnowKind.push_back(table[b].kind);
	return 0;
}

static_assert(sizeof(mtsgpu_yarn) == 56 && sizeof(mtsgpu_yarn) == sizeof(DYarn) && offsetof(mtsgpu_yarn, kd) == offsetof(DYarn, kd), "mtsgpu_yarn and DYarn are one layout");
static_assert(sizeof(DWeave) == 96 && offsetof(mtsgpu_weave, n_yarns) + 4 == offsetof(DWeave, first_pattern) && offsetof(mtsgpu_weave, pattern) == 80,
              "DWeave is the scalars of mtsgpu_weave, then the place of its arrays");

int mtsgpu_set_cloth_bsdfs(mtsgpu_ctx *c, uint32_t n_weaves, const mtsgpu_weave *weaves, const int32_t *bsdf_weave) {
	if (!c) return fail(c, MTSGPU_EINVAL, "null argument");
	if (!c->haveScene) return fail(c, MTSGPU_ESTATE, "mtsgpu_set_cloth_bsdfs before mtsgpu_upload_scene");
	c->lastPass.valid = false;
	HIPCHK(c, hipSetDevice(c->device));
	// nothing may still read the pool that goes (the shading launches of a render that was not synchronised)
	HIPCHK(c, hipStreamSynchronize(c->stream));
	if (c->stream2) HIPCHK(c, hipStreamSynchronize(c->stream2));
	freeAll(c->clothAllocs);
	c->dclo = DCloths{ nullptr, nullptr, nullptr, nullptr };
	c->hostClothWeave.clear();
	if (!bsdf_weave) return 0;
	if (c->dsc.has_shapes == kHasCylinders)
		return fail(c, MTSGPU_EINVAL, "the cloth BRDF is not served in a scene with a cylinder yet (the cloth kernels do not build a cylinder's record)");
	if (n_weaves && !weaves) return fail(c, MTSGPU_EINVAL, "n_weaves without weaves");
	if (n_weaves > (1u << 20)) return fail(c, MTSGPU_EINVAL, "at most 2^20 weaves");
	const mtsgpu_ctx::HostScene &h = c->host;
	const uint32_t nBsdfs = (uint32_t) h.bsdfType.size(), nShapes = (uint32_t) h.shapeBsdf.size();
	for (uint32_t k = 0; k < n_weaves; ++k) {
		const std::string why = checkWeave(weaves[k]);
		if (!why.empty()) return fail(c, MTSGPU_EINVAL, "weave %u: %s", k, why.c_str());
	}
	bool any = false;
	for (uint32_t b = 0; b < nBsdfs; ++b) {
		const int32_t k = bsdf_weave[b];
		if (k < -1 || k >= (int32_t) n_weaves) return fail(c, MTSGPU_EINVAL, "BSDF %u: weave index %d out of range (%u weaves)", b, k, n_weaves);
		if (k < 0) continue;
		any = true;
		if ((h.bsdfType[b] & ~(uint32_t) MTSGPU_BSDF_TWOSIDED) != (uint32_t) MTSGPU_BSDF_LAMBERTIAN)
			return fail(c, MTSGPU_EINVAL, "BSDF %u: a weave sits on a Lambertian entry (twosided allowed), not on type word %u", b, h.bsdfType[b]);
		if (!c->hostColorSlots.empty() && c->hostColorSlots[b])
			return fail(c, MTSGPU_EINVAL, "BSDF %u: a cloth BRDF has no texture slot, and the entry takes vertex colours", b);
		if (!c->hostSlotTex.empty() && (c->hostSlotTex[2 * (size_t) b] >= 0 || c->hostSlotTex[2 * (size_t) b + 1] >= 0))
			return fail(c, MTSGPU_EINVAL, "BSDF %u: a cloth BRDF has no texture slot, and the entry has a uv texture", b);
		if (!c->hostMaskKind.empty() && c->hostMaskKind[b] != (uint32_t) MTSGPU_MASK_NONE)
			return fail(c, MTSGPU_EINVAL, "BSDF %u: a mask around a cloth BRDF is not supported", b);
		if (!c->hostSnowKind.empty() && c->hostSnowKind[b] != (uint32_t) MTSGPU_SNOW_NONE)
			return fail(c, MTSGPU_EINVAL, "BSDF %u: the entry has a snow record and a weave", b);
	}
	for (uint32_t b = 0; b < nBsdfs; ++b) {
		if ((h.bsdfType[b] & 0xFFu) != MTSGPU_BSDF_COMPOSITE) continue;
		const float *P = h.bsdfParams.data() + (size_t) MTSGPU_BSDF_NPARAMS * b;
		const int n = (int) P[0];
		for (int i = 0; i < n; ++i)
			if (bsdf_weave[(uint32_t) P[1 + n + i]] >= 0)
				return fail(c, MTSGPU_EINVAL, "BSDF %u: composite child %d has a weave: the composite's loop would run it as a Lambertian, not supported", b, i);
	}
	if (!any) return 0;           // nothing to keep: the context launches what it launches without a table
	// the shapes a weave is shaded on: texcoords, a tangent frame, and the casts of f at the extremes of their texcoords
	for (uint32_t s = 0; s < nShapes; ++s) {
		const int32_t b = h.shapeBsdf[s];
		if (b < 0 || bsdf_weave[b] < 0) continue;
		double uMin = 0, uMax = 1, vMin = 0, vMax = 1;      // a sphere: uv in [0, 1]^2
		if (h.shapeType[s] == MTSGPU_SHAPE_TRIMESH) {
			if (c->hostShapeHasUv.empty() || !c->hostShapeHasUv[s])
				return fail(c, MTSGPU_EINVAL, "shape %u: the cloth BSDF (BSDF %d) needs texture coordinates: a mesh without them must be given some (trimesh.cpp:551-555)", s, b);
			if (h.shapeNormals[s] && !h.shapeTangents[s])
				return fail(c, MTSGPU_EINVAL, "shape %u: the cloth BSDF (BSDF %d) is anisotropic: a mesh with vertex normals needs its tangents (mtsgpu_upload_scene_tangents)", s, b);
			const double *r = &c->hostUvRange[4 * (size_t) s];
			uMin = r[0]; uMax = r[1]; vMin = r[2]; vMax = r[3];
		}       // (a sphere's its.uv comes from the hit point: it needs no texture call)
		const std::string why = clothCastRange(weaves[bsdf_weave[b]], uMin, uMax, vMin, vMax);
		if (!why.empty()) return fail(c, MTSGPU_EINVAL, "shape %u: weave %d: %s", s, bsdf_weave[b], why.c_str());
	}
	// one pool: the records, the pattern words and the yarns
	std::vector<DWeave> rec(n_weaves);
	std::vector<uint32_t> pat;
	std::vector<DYarn> yarns;
	for (uint32_t k = 0; k < n_weaves; ++k) {
		std::memset(&rec[k], 0, sizeof(DWeave));
		std::memcpy(&rec[k], &weaves[k], offsetof(mtsgpu_weave, pattern));
		rec[k].first_pattern = (uint32_t) pat.size(); rec[k].first_yarn = (uint32_t) yarns.size();
		pat.insert(pat.end(), weaves[k].pattern, weaves[k].pattern + weaves[k].n_pattern);
		const DYarn *y = reinterpret_cast<const DYarn *>(weaves[k].yarns);
		yarns.insert(yarns.end(), y, y + weaves[k].n_yarns);
	}
	const DWeave *dW = nullptr; const uint32_t *dP = nullptr; const DYarn *dY = nullptr; const int32_t *dB = nullptr;
	int rc = upload(c, &dW, rec.data(), rec.size(), &c->clothAllocs);
	if (!rc) rc = upload(c, &dP, pat.data(), pat.size(), &c->clothAllocs);
	if (!rc) rc = upload(c, &dY, yarns.data(), yarns.size(), &c->clothAllocs);
	if (!rc) rc = upload(c, &dB, bsdf_weave, nBsdfs, &c->clothAllocs);
	if (rc) { freeAll(c->clothAllocs); return rc; }
	c->dclo = DCloths{ dW, dP, dY, dB };
	c->hostClothWeave.assign(bsdf_weave, bsdf_weave + nBsdfs);
	return 0;
}

int mtsgpu_set_uv_textures(mtsgpu_ctx *c, const float *vtx_uv, const uint32_t *shape_has_uv, uint32_t n_textures,
                           const mtsgpu_uv_texture *textures, const int32_t *bsdf_slot_texture) {
	return setUvTextures(c, vtx_uv, shape_has_uv, n_textures, textures, bsdf_slot_texture, 0, nullptr, nullptr, false, "mtsgpu_set_uv_textures");
}

int mtsgpu_set_uv_bitmap_textures(mtsgpu_ctx *c, const float *vtx_uv, const uint32_t *shape_has_uv, uint32_t n_textures,
                                  const mtsgpu_uv_texture *textures, const int32_t *bsdf_slot_texture, uint32_t n_bitmaps,
                                  const mtsgpu_bitmap *bitmaps, const int32_t *texture_bitmap) {
	return setUvTextures(c, vtx_uv, shape_has_uv, n_textures, textures, bsdf_slot_texture, n_bitmaps, bitmaps, texture_bitmap, true,
	                     "mtsgpu_set_uv_bitmap_textures");
}

int mtsgpu_set_uv_masked_textures(mtsgpu_ctx *c, const float *vtx_uv, const uint32_t *shape_has_uv, uint32_t n_textures,
                                  const mtsgpu_uv_texture *textures, const int32_t *bsdf_slot_texture, uint32_t n_bitmaps,
                                  const mtsgpu_bitmap *bitmaps, const int32_t *texture_bitmap, const mtsgpu_bsdf_mask *bsdf_mask) {
	return setUvTextures(c, vtx_uv, shape_has_uv, n_textures, textures, bsdf_slot_texture, n_bitmaps, bitmaps, texture_bitmap, true,
	                     "mtsgpu_set_uv_masked_textures", bsdf_mask);
}

// LDRTexture::initializeFrom (ldrtexture.cpp:116-202) and MIPMap::fromBitmap (mipmap.cpp:156-177)
int mtsgpu_ldr_texels(int bpp, uint32_t width, uint32_t height, const uint8_t *data, float gamma, float *out) {
	if (!data || !out) return fail(nullptr, MTSGPU_EINVAL, "null argument");
	if (width == 0 || height == 0) return fail(nullptr, MTSGPU_EINVAL, "zero dimension (%u x %u)", width, height);
	if (bpp != 1 && bpp != 8 && bpp != 16 && bpp != 24 && bpp != 32)
		return fail(nullptr, MTSGPU_EINVAL, "%i bpp images are currently not supported!", bpp);
	float tbl[256];
	if (gamma == -1.0f) {
		for (int i = 0; i < 256; ++i) {      // fromSRGBComponent (:116-121)
			const float value = (float) i / 255.0f;
			tbl[i] = value <= 0.04045f ? value / 12.92f : std::pow((value + 0.055f) / (float) (1.0 + 0.055), 2.4f);
		}
	} else {
		for (int i = 0; i < 256; ++i) tbl[i] = std::pow((float) i / 255.0f, gamma);
	}
	for (int i = 0; i < 256; ++i) tbl[i] = std::max(tbl[i], 0.0f);      // clampNegative (a NaN of pow stays one: the upload refuses it)
	const size_t n = (size_t) width * height;
	for (size_t pos = 0; pos < n; ++pos) {
		float *o = out + 3 * pos;
		if (bpp == 32 || bpp == 24) {
			const uint8_t *p = data + (size_t) (bpp / 8) * pos;
			o[0] = tbl[p[0]]; o[1] = tbl[p[1]]; o[2] = tbl[p[2]];
		} else {
			const int value = bpp == 16 ? data[2 * pos] : bpp == 8 ? data[pos] : (data[pos / 8] & (1 << (pos % 8))) ? 255 : 0;
			o[0] = o[1] = o[2] = tbl[value];
		}
	}
	return 0;
}

} // extern "C"
