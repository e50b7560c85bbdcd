// host.h -- host-side pieces of libmtsgpu shared between translation units.
#pragma once
#include "../../include/mtsgpu.h"
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

namespace mg {

struct KdTree {
	std::vector<uint32_t> nodes;      // 2 dwords per node
	std::vector<uint32_t> indices;
	float aabbMin[3] = { 0, 0, 0 }, aabbMax[3] = { 0, 0, 0 };
	double stats[6] = { 0, 0, 0, 0, 0, 0 };
};

// genBox: [nTris][6] boxes, read for the primitives whose tri row is {MTSGPU_KNOTRIANGLE x 3}; may be NULL without such
void buildKdTree(const float *vtx, const uint32_t *tri, uint32_t nTris, const float *genBox, const mtsgpu_kd_params *kp, KdTree &out);
bool clippedTriangleBox(const float *p0, const float *p1, const float *p2, const float *bmin, const float *bmax,
                        float *omin, float *omax);

// Owns every array a mtsgpu_scene points to
struct FlatScene {
	mtsgpu_scene sc;
	KdTree kd;
	std::vector<float> envPixels, envPdf, envCdf;
	std::vector<float> vtxPos, vtxNrm, shapeParams, bsdfParams, lumParams, lumInvArea, lumTriCdf, lumSelCdf, lumSelPdf;
	std::vector<uint32_t> triIdx, shapeTriOffset, shapeFlags, shapeType, triaccel, bsdfType, lumType, lumCdfOffset;
	std::vector<int32_t> shapeBsdf, shapeLum, lumShape;
};

// What the kernels require of a BSDF table (mtsgpu_upload_scene, mtsgpu_bsdf_eval_table and the flattener all ask here):
// known types, and for a composite (block: [0] n, [1..n] weights, [1+n..2n] child indices as floats) 1 <= n <=
// MTSGPU_COMPOSITE_MAX, no negative weight (composite.cpp:45-46), children that exist and are neither composites nor delta
// BSDFs.  Returns the reason, or an empty string.
inline std::string checkBsdfTable(uint32_t n_bsdfs, const uint32_t *type, const float *params) {
	auto msg = [](uint32_t b, const std::string &what) { return "BSDF " + std::to_string(b) + ": " + what; };
	for (uint32_t b = 0; b < n_bsdfs; ++b) {
		if ((type[b] & ~(uint32_t) MTSGPU_BSDF_TWOSIDED) >= MTSGPU_BSDF_NTYPES) return msg(b, "unknown type");
		if ((type[b] & 0xFFu) != MTSGPU_BSDF_COMPOSITE) continue;
		const float *P = params + (size_t) MTSGPU_BSDF_NPARAMS * b;
		if (!(P[0] >= 1.0f && P[0] <= (float) MTSGPU_COMPOSITE_MAX) || P[0] != (float) (int) P[0])
			return msg(b, "a composite needs between 1 and " + std::to_string(MTSGPU_COMPOSITE_MAX) + " children");
		const int n = (int) P[0];
		for (int i = 0; i < n; ++i) {
			const float w = P[1 + i], ci = P[1 + n + i];
			const std::string child = "composite child " + std::to_string(i);
			if (!(w >= 0.0f) || !(w <= 3.4028235e38f)) return msg(b, child + ": invalid BRDF weight (negative or not finite, composite.cpp:45-46)");
			if (!(ci >= 0.0f && ci < (float) n_bsdfs) || ci != (float) (uint32_t) ci) return msg(b, child + ": index out of range");
			const uint32_t ct = type[(uint32_t) ci] & 0xFFu;
			if (ct >= MTSGPU_BSDF_NTYPES) return msg(b, child + ": unknown type");
			if (ct == MTSGPU_BSDF_COMPOSITE) return msg(b, child + " is a composite: nested composites are not supported");
			if (ct == MTSGPU_BSDF_DIELECTRIC || ct == MTSGPU_BSDF_MIRROR)
				return msg(b, child + " is a delta BSDF (dielectric, mirror): a composite would need fDelta / pdfDelta, not supported");
		}
		// DiscretePDF::build divides by the sum of the weights (pdf.h:87-91): all zero makes every pdf and knot NaN
		float sum = 0.0f;
		for (int i = 0; i < n; ++i) sum = sum + P[1 + i];
		if (!(sum > 0.0f) || !(sum <= 3.4028235e38f)) return msg(b, "the weights of a composite must have a positive, finite sum");
	}
	return std::string();
}
// BSDF::EAnisotropic of entry b of a checked table: a Ward with alphaX != alphaY (ward.cpp:84-85), alone or inside a composite
inline bool bsdfIsAnisotropic(const uint32_t *type, const float *params, uint32_t b) {
	const float *P = params + (size_t) MTSGPU_BSDF_NPARAMS * b;
	const uint32_t t = type[b] & 0xFFu;
	if (t == MTSGPU_BSDF_WARD) return P[1] != P[2];
	if (t != MTSGPU_BSDF_COMPOSITE) return false;
	const int n = (int) P[0];
	for (int i = 0; i < n; ++i) {
		const uint32_t c = (uint32_t) P[1 + n + i];
		if ((type[c] & 0xFFu) == MTSGPU_BSDF_WARD && bsdfIsAnisotropic(type, params, c)) return true;
	}
	return false;
}
// Shapes that give the shading frame a tangent an anisotropic BSDF can use: spheres (dpdu / dpdv).  Triangle meshes carry no
// texture coordinates here, and any shape type added later has none until it says so here.
inline bool shapeHasTangentFrame(uint32_t shape_type) { return shape_type == MTSGPU_SHAPE_SPHERE; }
// the reference's refusal of an anisotropic BSDF on a mesh without texture coordinates (trimesh.cpp:288-290, :547-556)
inline std::string anisotropicOnMeshMessage(uint32_t shape) {
	return "shape " + std::to_string(shape) + ": computeTangentSpace(): texture coordinates are required to generate tangent vectors. "
	       "If you want to render with an anisotropic material, please make sure that all associated shapes have valid texture "
	       "coordinates (triangle meshes have none here: an anisotropic Ward BSDF needs a sphere)";
}

void flattenScene(const mtsgpu_scene_desc &d, const mtsgpu_kd_params *kp, FlatScene &fs);

// One shape of a `.serialized` file (TriMesh::TriMesh(Stream *, int), src/librender/trimesh.cpp:156-236)
struct LoadedMesh {
	std::vector<float> positions, normals;     // normals empty when the file has none
	std::vector<uint32_t> triangles;
	bool faceNormals = false;
};
void loadSerializedMesh(const char *path, int index, LoadedMesh &out);   // throws std::runtime_error
// TabulatedFilter of the box / gaussian / mitchell / catmullrom / wsinc plugins (kinds 0..4): sizeXY[2], values[16*16]
void tabulateFilter(int kind, float halfSize, float p0, float p1, float *sizeXY, float *values);
void makeCamera(const float origin[3], const float target[3], const float up[3], float fovDeg, int width, int height,
                mtsgpu_camera &out);
void makeCameraOrtho(const float origin[3], const float target[3], const float up[3], float scaleX, float scaleY,
                     int width, int height, mtsgpu_camera &out);

} // namespace mg
