// scene_layout.cpp -- the pure half of the upload calls (host.h): what mtsgpu_upload_scene and the attachment setters check of
// the caller's arrays and what they lay out for the device.  No context and no HIP call: scene_upload.cpp and scene_attach.cpp
// free, upload and commit around these functions, and a stand-alone program can run them without a GPU (tests/upload_harness).
#include "host.h"
#include <algorithm>
#include <cmath>
#include <cstring>

namespace mg {

std::string checkCylinderBlock(const float *D) {
	for (int i = 0; i < MTSGPU_CYLINDER_NDERIVED; ++i)
		if (!std::isfinite(D[i])) return "non-finite cylinder parameter";
	if (!(D[24] > 0.0f) || !(D[25] > 0.0f)) return "a cylinder needs radius > 0 and length > 0 (Assert, cylinder.cpp:63)";
	return std::string();
}

// rows = NULL: the check alone
bool gatherMeshRows(const uint32_t *triIdx, uint32_t t0, uint32_t t1, const float *vtx, int comps, size_t stride, float *rows, uint32_t *bad) {
	const size_t slot = comps == 3 ? 4 : (size_t) comps;
	for (uint32_t t = t0; t < t1; ++t)
		for (int k = 0; k < 3; ++k) {
			const uint32_t v = triIdx[3 * (size_t) t + k];      // < n_verts: checkScene checked it
			const float *a = vtx + (size_t) comps * v;
			for (int i = 0; i < comps; ++i) if (!std::isfinite(a[i])) { *bad = v; return false; }
			if (rows) std::memcpy(&rows[4 * stride * (size_t) t + slot * (size_t) k], a, sizeof(float) * (size_t) comps);
		}
	return true;
}

namespace {
std::string shapeMsg(uint32_t s, const std::string &what) { return "shape " + std::to_string(s) + ": " + what; }
std::string lumMsg(uint32_t l, const std::string &what) { return "luminaire " + std::to_string(l) + ": " + what; }
uint32_t shapeTypeOf(const mtsgpu_scene &sc, uint32_t s) { return sc.shape_type ? sc.shape_type[s] : (uint32_t) MTSGPU_SHAPE_TRIMESH; }
}

std::string checkScene(const mtsgpu_scene &sc, const UploadExtras &x, uint32_t depthLimit, float *skyDerived) {
	if (sc.n_nodes == 0 || !sc.kd_nodes) return "scene has no kd-tree";
	if (sc.n_lums == 0) return "scene has no luminaire (Scene::initialize would add a constant one, scene.cpp:310-318)";
	for (uint32_t i = 0; i < sc.n_nodes; ++i) {
		const uint32_t a = sc.kd_nodes[2 * (size_t) i], b = sc.kd_nodes[2 * (size_t) i + 1];
		if (a & 0x80000000u) {
			if ((a & 0x7FFFFFFFu) > b || b > sc.n_indices) return "kd leaf " + std::to_string(i) + ": index range out of bounds";
		} else {
			if (a & 0x40000000u) return "kd node " + std::to_string(i) + ": indirection nodes are not supported (gkdtree.h:1116-1126 removes them)";
			const uint64_t left = (uint64_t) i + ((a & 0x3FFFFFFCu) >> 2);
			if ((a & 3u) == 3u || left <= i || left + 1 >= sc.n_nodes) return "kd node " + std::to_string(i) + ": bad axis/child offset";
		}
	}
	{
		// every node is reached exactly once from the root (the device order is built by walking the tree: an unreached node
		// would land on the root's slot, a shared one twice) and no branch is deeper than the traversal stack of k_trace (LDS
		// levels + spill levels; the reference's own limit is MTS_KD_MAXDEPTH = 48, gkdtree.h:35)
		std::vector<uint8_t> seen(sc.n_nodes, 0);
		std::vector<std::pair<uint32_t, uint32_t>> stack;       // node, depth
		stack.emplace_back(0u, 1u);
		uint32_t visited = 0;
		while (!stack.empty()) {
			const auto [i, depth] = stack.back(); stack.pop_back();
			if (seen[i]) return "kd node " + std::to_string(i) + " is the child of two nodes";
			seen[i] = 1; ++visited;
			const uint32_t a = sc.kd_nodes[2 * (size_t) i];
			if (a & 0x80000000u) continue;
			if (depth >= depthLimit) return "kd-tree deeper than " + std::to_string(depthLimit) + " levels";
			const uint32_t left = i + ((a & 0x3FFFFFFCu) >> 2);
			stack.emplace_back(left + 1, depth + 1); stack.emplace_back(left, depth + 1);
		}
		if (visited != sc.n_nodes)
			return "kd-tree: " + std::to_string(sc.n_nodes - visited) + " of " + std::to_string(sc.n_nodes) + " nodes are unreachable from the root";
	}
	for (uint32_t i = 0; i < sc.n_indices; ++i)
		if (sc.kd_indices[i] >= sc.n_tris) return "kd index " + std::to_string(i) + " out of range";
	if ((sc.shape_type == nullptr) != (sc.shape_params == nullptr)) return "shape_type and shape_params must both be given or both be NULL";
	for (uint32_t s = 0; s < sc.n_shapes; ++s) {
		const uint32_t type = shapeTypeOf(sc, s);
		if (type == MTSGPU_SHAPE_CYLINDER) {
			if (!x.acceptsCylinders)
				return "shape " + std::to_string(s) + " is a cylinder: its derived block travels beside the scene, upload it with mtsgpu_upload_scene_cylinders";
			if (!x.cylinders) return "shape " + std::to_string(s) + " is a cylinder, but mtsgpu_upload_scene_cylinders was given no cylinder blocks";
		} else if (type > MTSGPU_SHAPE_SPHERE) return shapeMsg(s, "unknown shape type");
		// the primitives of shape s are [offset[s], offset[s + 1]), inside the primitive arrays: every read below goes through it
		if (sc.shape_tri_offset[s] > sc.shape_tri_offset[s + 1] || sc.shape_tri_offset[s + 1] > sc.n_tris) return "shape_tri_offset not monotone";
		const bool mesh = type == MTSGPU_SHAPE_TRIMESH;
		if (!mesh) {
			// any other shape is ONE kd-tree primitive (skdtree.cpp:54-57)
			if (sc.shape_tri_offset[s + 1] - sc.shape_tri_offset[s] != 1) return shapeMsg(s, "a non-mesh shape must own exactly one primitive");
			const float *SP = sc.shape_params + (size_t) MTSGPU_SHAPE_NPARAMS * s;
			for (int i = 0; i < MTSGPU_SHAPE_NPARAMS; ++i) if (!std::isfinite(SP[i])) return shapeMsg(s, "non-finite parameter");
			if (type == MTSGPU_SHAPE_CYLINDER) {
				const std::string why = checkCylinderBlock(x.cylinders + (size_t) MTSGPU_CYLINDER_NDERIVED * s);
				if (!why.empty()) return shapeMsg(s, why);
				// what a cylinder's hit has been rendered and checked with: a plain Lambertian (constant, checkerboard, grid or bitmap
				// reflectance).  Every other family is refused by name until it has its frames: the shading kernels of the other
				// bins and of the mask, snow and cloth families are compiled without the cylinder's record (shade_bsdf.h: CYL)
				// (without a BSDF its closest hits would go to the terminal bin, whose kernel does not build a cylinder's record either)
				const int32_t b = sc.shape_bsdf[s];
				if (b < 0) return shapeMsg(s, "a cylinder without a BSDF is not served yet: give it a plain lambertian");
				if (b < (int32_t) sc.n_bsdfs && sc.bsdf_type[b] != (uint32_t) MTSGPU_BSDF_LAMBERTIAN)
					return shapeMsg(s, "a cylinder takes a plain lambertian BSDF only; BSDF " + std::to_string(b) + " is of type " + std::to_string(sc.bsdf_type[b] & 0xFFu)
					                   + ((sc.bsdf_type[b] & MTSGPU_BSDF_TWOSIDED) ? " under twosided" : "") + ", not served on a cylinder yet");
				if (sc.shape_lum[s] >= 0)
					return shapeMsg(s, "a cylinder cannot carry an area luminaire: Cylinder has no pdfArea, and Shape::pdfArea raises an error "
					                   "on the first BSDF-sampled hit (shape.cpp:174-178), so the reference cannot render it either");
			} else if (SP[3] == 0.0f) return shapeMsg(s, "zero radius");
		}
		for (uint32_t t = sc.shape_tri_offset[s]; t < sc.shape_tri_offset[s + 1]; ++t) {
			const uint32_t k = sc.triaccel[12 * (size_t) t];
			auto refuse = [t](const char *what) { return "TriAccel " + std::to_string(t) + ": " + what; };      // (built on refusal only: the loop runs per primitive)
			if (mesh) {
				if (k == MTSGPU_KNOTRIANGLE) return refuse("a mesh triangle is marked as a shape");
				for (int j = 0; j < 3; ++j)
					if (sc.tri_idx[3 * (size_t) t + j] >= sc.n_verts) return "triangle vertex index out of range";
			} else if (k != MTSGPU_KNOTRIANGLE) {
				return refuse("the primitive of a non-mesh shape must have k = KNoTriangleFlag");
			}
			if (sc.triaccel[12 * (size_t) t + 10] != s) return refuse("shape index does not match shape_tri_offset");
		}
	}
	for (uint32_t s = 0; s < sc.n_shapes; ++s) {
		if (sc.shape_bsdf[s] >= (int32_t) sc.n_bsdfs || sc.shape_lum[s] >= (int32_t) sc.n_lums) return shapeMsg(s, "bad BSDF/luminaire index");
		if (sc.shape_lum[s] >= 0 && (sc.lum_type[sc.shape_lum[s]] != MTSGPU_LUM_AREA || sc.lum_shape[sc.shape_lum[s]] != (int32_t) s))
			return shapeMsg(s, "luminaire link is inconsistent");
	}
	if (sc.shape_tri_offset[sc.n_shapes] != sc.n_tris) return "shape_tri_offset does not cover all triangles";
	for (uint32_t t = 0; t < sc.n_tris; ++t)
		if (sc.triaccel[12 * (size_t) t + 10] >= sc.n_shapes) return "TriAccel " + std::to_string(t) + ": shape index out of range";
	{
		const std::string why = checkBsdfTable(sc.n_bsdfs, sc.bsdf_type, sc.bsdf_params);
		if (!why.empty()) return why;
	}
	// an anisotropic BSDF needs a tangent frame: spheres have one (dpdu / dpdv), a triangle mesh when the caller hands its
	// vertex tangents over.  Without them the reference renders a mesh that has no vertex normals with the frame it has
	// (trimesh.cpp:562-565); mtsgpu_upload_scene keeps refusing every such mesh
	for (uint32_t s = 0; s < sc.n_shapes; ++s) {
		const bool has = x.shapeHasTangents && x.shapeHasTangents[s];
		if (has && shapeTypeOf(sc, s) != MTSGPU_SHAPE_TRIMESH) return shapeMsg(s, "only a triangle mesh can carry tangents");
		if (has && !(sc.shape_flags[s] & MTSGPU_SHAPE_HAS_NORMALS)) return shapeMsg(s, "tangents need vertex normals (trimesh.cpp:562-565)");
		if (has || !(sc.shape_bsdf[s] >= 0 && !shapeHasTangentFrame(shapeTypeOf(sc, s)) && bsdfIsAnisotropic(sc.bsdf_type, sc.bsdf_params, (uint32_t) sc.shape_bsdf[s])))
			continue;
		if (!x.withTangents || (sc.shape_flags[s] & MTSGPU_SHAPE_HAS_NORMALS)) return anisotropicOnMeshMessage(s);
	}
	// the tangents layoutScene gathers
	for (uint32_t s = 0; s < sc.n_shapes && x.shapeHasTangents; ++s) {
		uint32_t v;
		if (x.shapeHasTangents[s] && !gatherMeshRows(sc.tri_idx, sc.shape_tri_offset[s], sc.shape_tri_offset[s + 1], x.vtxDpdu, 3, kTriDpduStride, nullptr, &v))
			return shapeMsg(s, "non-finite tangent at vertex " + std::to_string(v));
	}
	for (uint32_t l = 0; l < sc.n_lums; ++l) {
		if (sc.lum_type[l] == MTSGPU_LUM_AREA) {
			const int32_t s = sc.lum_shape[l];
			if (s < 0 || s >= (int32_t) sc.n_shapes) return lumMsg(l, "bad shape");
			const uint32_t n = sc.shape_tri_offset[s + 1] - sc.shape_tri_offset[s];
			if (shapeTypeOf(sc, (uint32_t) s) != MTSGPU_SHAPE_TRIMESH) {
				if (sc.lum_cdf_offset[l + 1] != sc.lum_cdf_offset[l]) return lumMsg(l, "a non-mesh emitter has no triangle CDF");
			} else if (sc.lum_cdf_offset[l + 1] - sc.lum_cdf_offset[l] != n + 1) return lumMsg(l, "CDF size mismatch");
		} else if (sc.lum_type[l] == MTSGPU_LUM_ENVMAP) {
			// everything env_triangle / env_pdf index with (envmap.cpp:123-193)
			if ((int32_t) l != sc.background_lum) return lumMsg(l, "the envmap must be the background luminaire");
			const uint64_t np = (uint64_t) sc.env_pdf_width * sc.env_pdf_height;
			if (!sc.env_pixels || !sc.env_pdf || !sc.env_cdf || sc.env_width == 0 || sc.env_height == 0 || np == 0
			    || sc.env_width > 16384 || sc.env_height > 16384 || np > (1u << 26))
				return lumMsg(l, "missing or oversized environment map");
			for (uint64_t i = 0; i < np; ++i)
				if (!(sc.env_cdf[i] <= sc.env_cdf[i + 1]) || !(sc.env_pdf[i] >= 0.0f)) return lumMsg(l, "the environment map's CDF is not monotone");
			const float *LP = sc.lum_params + (size_t) MTSGPU_LUM_NPARAMS * l;
			for (int i = 0; i < 25; ++i) if (!std::isfinite(LP[i])) return lumMsg(l, "non-finite parameter");
		} else if (sc.lum_type[l] == MTSGPU_LUM_SKY) {
			const std::string why = checkSkyLuminaire(l, sc.lum_params + (size_t) MTSGPU_LUM_NPARAMS * l, sc.background_lum, skyDerived);
			if (!why.empty()) return why;
		} else if (sc.lum_type[l] > MTSGPU_LUM_COLLIMATED) {
			return lumMsg(l, "unknown type");
		}
	}
	if (sc.background_lum >= (int32_t) sc.n_lums) return "background luminaire out of range";
	return std::string();
}

std::string layoutScene(const mtsgpu_scene &sc, const UploadExtras &x, uint32_t topSlots, SceneLayout &out) {
	auto shapeType = [&](uint32_t s) { return shapeTypeOf(sc, s); };
	{
		// Device node order.  The first topSlots slots hold the root and the sibling pairs below it in breadth-first order:
		// k_trace keeps the first half of that prefix in LDS (kernels.h: kTopNodes).  After it, 128-byte lines (16 nodes) are
		// filled with breadth-first pieces of subtrees ("treelets") so that one L1 miss serves several consecutive traversal
		// steps.  The KDNode encoding is unchanged (siblings adjacent, relative offset to the left child, gkdtree.h:442-470);
		// only where a node lives changes, which traversal results do not depend on.
		const uint32_t N = sc.n_nodes;
		std::vector<uint32_t> newIndex(N, 0u);
		std::vector<uint32_t> stack, cand;           // entries: old index of the left node of a sibling pair
		auto leftOf = [&](uint32_t i) { return i + ((sc.kd_nodes[2 * (size_t) i] & 0x3FFFFFFCu) >> 2); };
		auto isLeaf = [&](uint32_t i) { return (sc.kd_nodes[2 * (size_t) i] & 0x80000000u) != 0; };
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
		if (total >= (1u << 29)) return "kd-tree too large";      // absolute child indices; k_trace's stack words keep node index * 2 below bit 30
		std::vector<uint32_t> &dev = out.nodes;
		dev.assign(2 * (size_t) total, 0u);
		dev[2] = 0x80000000u; dev[3] = 0u;           // padding slot: empty leaf, never referenced
		for (uint32_t i = 0; i < N; ++i) {
			const uint32_t a = sc.kd_nodes[2 * (size_t) i], b = sc.kd_nodes[2 * (size_t) i + 1];
			uint32_t *o = &dev[2 * (size_t) newIndex[i]];
			if (a & 0x80000000u) { o[0] = a; o[1] = b; }
			else { o[0] = (a & 3u) | (newIndex[leftOf(i)] << 2); o[1] = b; }     // absolute left-child index (< 2^29)
		}
	}
	{
		// TriAccel records re-laid out in leaf order (one contiguous run per leaf, no index indirection on the device);
		// non-occluders are shapes without a BSDF (Shape::isOccluder, shape.h:324)
		const size_t LS = 4 * (size_t) kLeafStride;                 // dwords per record slot
		// behind the records: four 16-byte rows per cylinder, worldToObject 3x4 and (radius, length, -, -) (kdevice.h); a
		// cylinder's record points at them with dword 4 = the index of the first row in units of 16 bytes
		std::vector<uint32_t> cylRow(sc.n_shapes, 0u);
		const size_t firstCylRow = (size_t) kLeafStride * ((size_t) sc.n_indices + 1);
		size_t nCyl = 0;
		for (uint32_t s = 0; s < sc.n_shapes; ++s)
			if (shapeType(s) == MTSGPU_SHAPE_CYLINDER) cylRow[s] = (uint32_t) (firstCylRow + 4 * nCyl++);
		if (firstCylRow + 4 * nCyl >= (1ull << 32)) return "too many leaf records";
		std::vector<uint32_t> &ta = out.leafTa;
		ta.assign(LS * ((size_t) sc.n_indices + 1) + 16 * nCyl, 0u);
		for (uint32_t s = 0; s < sc.n_shapes; ++s)
			if (shapeType(s) == MTSGPU_SHAPE_CYLINDER) {
				const float *D = x.cylinders + (size_t) MTSGPU_CYLINDER_NDERIVED * s;
				uint32_t *rows = &ta[4 * (size_t) cylRow[s]];
				std::memcpy(rows, D + 12, 48);
				std::memcpy(rows + 12, D + 24, 8);
			}
		for (uint32_t e = 0; e < sc.n_indices; ++e) {
			const uint32_t prim = sc.kd_indices[e];
			uint32_t *dst = &ta[LS * (size_t) e];
			std::memcpy(dst, sc.triaccel + 12 * (size_t) prim, 48);
			// dword 0 = k<<30 | non-occluder<<29 | primitive id (the head of the record decides everything
			// up to the plane distance); dword 10 stays the shape index
			if (prim >= (1u << 28)) return "more than 2^28 primitives";
			const bool isShape = dst[0] == MTSGPU_KNOTRIANGLE;
			dst[0] = (std::min(dst[0], 3u) << 30) | (sc.shape_bsdf[dst[10]] < 0 ? 0x20000000u : 0u) | prim;
			dst[11] = 0;
			if ((dst[0] >> 30) == 3u) {
				// k == 3: a degenerate triangle (dword 1 = 0) or a non-triangle shape (dword 1 = shape type,
				// dwords 4..7 = centre and radius of the sphere)
				dst[1] = 0;
				if (isShape) {
					const float *SP = sc.shape_params + (size_t) MTSGPU_SHAPE_NPARAMS * dst[10];
					dst[1] = shapeType(dst[10]);
					std::memcpy(dst + 4, SP, 16);
					if (dst[1] == MTSGPU_SHAPE_CYLINDER) dst[4] = cylRow[dst[10]];
				}
			}
		}
	}
	{
		// per-primitive position / normal records for the shading kernels
		const size_t TS = 4 * (size_t) kTriStride;                    // floats per record (one 128-byte line)
		std::vector<float> &triRec = out.triRec;
		triRec.assign(TS * ((size_t) sc.n_tris + 1), 0.0f);
		for (uint32_t s = 0; s < sc.n_shapes; ++s)
			for (uint32_t t = sc.shape_tri_offset[s]; t < sc.shape_tri_offset[s + 1]; ++t) {
				float *P = &triRec[TS * (size_t) t], *Nn = P + 12;
				if (shapeType(s) != MTSGPU_SHAPE_TRIMESH) {
					// non-mesh shape: centre + radius, flag bit 31 (the rest comes from shape_params)
					// (bit 30: the shape is a cylinder, whose record fill_its builds from its own layout of shape_params)
					const uint32_t flags = sc.shape_flags[s] | 0x80000000u | (shapeType(s) == MTSGPU_SHAPE_CYLINDER ? 0x40000000u : 0u);
					std::memcpy(P, sc.shape_params + (size_t) MTSGPU_SHAPE_NPARAMS * s, 16);
					std::memcpy(P + 10, &s, 4); std::memcpy(P + 11, &flags, 4);
					continue;
				}
				for (int k = 0; k < 3; ++k) {
					const uint32_t v = sc.tri_idx[3 * (size_t) t + k];
					std::memcpy(P + 3 * k, sc.vtx_pos + 3 * (size_t) v, 12);
					std::memcpy(Nn + 3 * k, sc.vtx_nrm + 3 * (size_t) v, 12);
				}
				const uint32_t flags = sc.shape_flags[s];
				std::memcpy(P + 10, &s, 4); std::memcpy(P + 11, &flags, 4);
			}
	}
	// the material queue of every shape's hits, and the queues that can ever be non-empty: the BSDF types of shapes that have
	// one, and the "terminal" bin
	out.shapeBin.assign((size_t) sc.n_shapes + 1, (uint32_t) kNumBsdfTypes);
	out.binMask = 1u << kNumBsdfTypes;
	for (uint32_t s = 0; s < sc.n_shapes; ++s)
		if (sc.shape_bsdf[s] >= 0) {
			out.shapeBin[s] = sc.bsdf_type[sc.shape_bsdf[s]] & 0xFFu;
			out.binMask |= 1u << out.shapeBin[s];
		}
	out.shapeType.assign((size_t) sc.n_shapes + 1, (uint32_t) MTSGPU_SHAPE_TRIMESH);
	out.shapeParams.assign((size_t) MTSGPU_SHAPE_NPARAMS * ((size_t) sc.n_shapes + 1), 0.0f);
	if (sc.shape_type) {
		std::copy(sc.shape_type, sc.shape_type + sc.n_shapes, out.shapeType.begin());
		std::copy(sc.shape_params, sc.shape_params + (size_t) MTSGPU_SHAPE_NPARAMS * sc.n_shapes, out.shapeParams.begin());
	}
	out.hasShapes = 0;
	for (uint32_t s = 0; s < sc.n_shapes; ++s) {
		if (shapeType(s) != MTSGPU_SHAPE_TRIMESH) out.hasShapes = std::max(out.hasShapes, kHasShapes);
		if (shapeType(s) != MTSGPU_SHAPE_CYLINDER) continue;
		out.hasShapes = kHasCylinders;      // the CYL kernels of trace.hip
		// a cylinder's device row, what the shading reads (shade_bsdf.h): [0..11] worldToObject 3x4, [12..20] the 3x3 of
		// objectToWorld, [21] length, [22] radius, [23] 1 / area
		const float *D = x.cylinders + (size_t) MTSGPU_CYLINDER_NDERIVED * s;
		float *P = &out.shapeParams[(size_t) MTSGPU_SHAPE_NPARAMS * s];
		std::memcpy(P, D + 12, 48);
		for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) P[12 + 3 * i + j] = D[4 * i + j];
		P[21] = D[25]; P[22] = D[24]; P[23] = D[26];
	}
	// the gather array of the tangents: dpdu of the three vertices of every primitive of a mesh that has them, zero elsewhere
	out.triDpdu.clear(); out.hasTan.clear();
	bool any = false;
	for (uint32_t s = 0; s < sc.n_shapes; ++s) any |= x.shapeHasTangents && x.shapeHasTangents[s];
	if (any) {
		out.triDpdu.assign(4 * (size_t) kTriDpduStride * ((size_t) sc.n_tris + 1), 0.0f);
		out.hasTan.assign((size_t) sc.n_shapes + 1, 0u);
		for (uint32_t s = 0; s < sc.n_shapes; ++s) {
			if (!x.shapeHasTangents[s]) continue;
			out.hasTan[s] = 1u;
			uint32_t v;      // finite: checkScene looked
			(void) gatherMeshRows(sc.tri_idx, sc.shape_tri_offset[s], sc.shape_tri_offset[s + 1], x.vtxDpdu, 3, kTriDpduStride, out.triDpdu.data(), &v);
		}
	}
	return std::string();
}

void keepHostScene(const mtsgpu_scene &sc, const UploadExtras &x, const SceneLayout &lay, HostScene &h) {
	h.nVerts = sc.n_verts; h.hasShapes = lay.hasShapes;
	h.triIdx.assign(sc.tri_idx, sc.tri_idx + 3 * (size_t) sc.n_tris);
	h.shapeTriOffset.assign(sc.shape_tri_offset, sc.shape_tri_offset + sc.n_shapes + 1);
	h.shapeType.assign(lay.shapeType.begin(), lay.shapeType.begin() + sc.n_shapes);
	h.bsdfType.assign(sc.bsdf_type, sc.bsdf_type + sc.n_bsdfs);
	h.bsdfParams.assign(sc.bsdf_params, sc.bsdf_params + (size_t) MTSGPU_BSDF_NPARAMS * sc.n_bsdfs);
	h.shapeBsdf.assign(sc.shape_bsdf, sc.shape_bsdf + sc.n_shapes);
	h.lumType.assign(sc.lum_type, sc.lum_type + sc.n_lums);
	h.lumParams.assign(sc.lum_params, sc.lum_params + (size_t) MTSGPU_LUM_NPARAMS * sc.n_lums);
	h.shapeNormals.assign(sc.n_shapes, 0u);
	h.shapeTangents.assign(sc.n_shapes, 0u);
	for (uint32_t s = 0; s < sc.n_shapes; ++s) {
		h.shapeNormals[s] = (sc.shape_flags[s] & MTSGPU_SHAPE_HAS_NORMALS) ? 1u : 0u;
		h.shapeTangents[s] = (x.shapeHasTangents && x.shapeHasTangents[s]) ? 1u : 0u;
	}
}

// what mtsgpu_set_uv_textures and mtsgpu_uv_texture_eval require of one descriptor; the reason, or an empty string
// (bitmaps: a call that takes MTSGPU_TEX_BITMAP, of which only the four Texture2D floats count)
std::string checkUvTexture(const mtsgpu_uv_texture &t, bool bitmaps) {
	const bool bitmap = bitmaps && t.kind == (uint32_t) MTSGPU_TEX_BITMAP;
	if (t.kind >= (uint32_t) MTSGPU_TEX_NKINDS && !bitmap) return "unknown kind " + std::to_string(t.kind);
	const float *f = &t.uoffset;      // the eleven floats behind the kind
	for (int i = 0; i < (bitmap ? 4 : 11); ++i) if (!std::isfinite(f[i])) return "non-finite parameter";
	return std::string();
}

// what mtsgpu_set_uv_bitmap_textures and mtsgpu_bitmap_texture_eval require of one bitmap; the reason, or an empty string.
// *total counts the texels so far and is checked before any texel is read
std::string checkBitmap(const mtsgpu_bitmap &b, uint64_t *total) {
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
void packBitmapTexels(const mtsgpu_bitmap &b, float *dst) {
	const size_t n = (size_t) b.width * b.height;
	for (size_t i = 0; i < n; ++i) {
		dst[4 * i] = b.texels[3 * i]; dst[4 * i + 1] = b.texels[3 * i + 1]; dst[4 * i + 2] = b.texels[3 * i + 2]; dst[4 * i + 3] = 0.0f;
	}
}

static_assert(sizeof(mtsgpu_uv_texture) == sizeof(DTexture) && offsetof(mtsgpu_uv_texture, line_width) == offsetof(DTexture, line_width)
              && offsetof(mtsgpu_uv_texture, bright) == offsetof(DTexture, bright), "mtsgpu_uv_texture and DTexture are one layout");
static_assert(MTSGPU_TEX_CHECKERBOARD == (int) kTexCheckerboard && MTSGPU_TEX_GRID == (int) kTexGrid, "texture kinds differ");
static_assert(MTSGPU_TEX_BITMAP == (int) kTexBitmap && offsetof(DTexture, width) == offsetof(mtsgpu_uv_texture, bright)
              && offsetof(DTexture, reserved) + sizeof(DTexture::reserved) == sizeof(DTexture), "the bitmap words are the seven behind vscale");
static_assert(MTSGPU_WRAP_REPEAT == (int) kWrapRepeat && MTSGPU_WRAP_CLAMP == (int) kWrapClamp && MTSGPU_WRAP_BLACK == (int) kWrapBlack
              && MTSGPU_WRAP_WHITE == (int) kWrapWhite, "wrap modes differ");

// 2 * uv' of texture t at texcoord (u, v) stays inside the range of the reference's (int) cast, with the margin the header states
// (a bitmap of sx x sy texels: uv' * (sx, sy), mipmap.cpp:229-230)
static bool uvCastInRange(const mtsgpu_uv_texture &t, float u, float v, double sx = 2.0, double sy = 2.0) {
	const double lim = 2147483648.0 - 65536.0;
	const double x = sx * ((double) u * t.uscale + t.uoffset), y = sy * ((double) v * t.vscale + t.voffset);
	return std::fabs(x) < lim && std::fabs(y) < lim;
}

std::string planTextures(const HostScene &h, const InForce &in, const TextureArgs &a, TexturePlan &out) {
	out = TexturePlan();
	if (!a.vtx_uv && !a.shape_has_uv && !a.textures && !a.bsdf_slot_texture && !a.bitmaps && !a.texture_bitmap && !a.bsdf_mask) return std::string();
	if ((a.vtx_uv == nullptr) != (a.shape_has_uv == nullptr)) return "vtx_uv and shape_has_uv must both be given or both be NULL";
	if (a.n_textures && !a.textures) return "n_textures without textures";
	if (a.n_textures > (1u << 20)) return "at most 2^20 textures";
	if (a.n_bitmaps && !a.bitmaps) return "n_bitmaps without bitmaps";
	if (a.n_bitmaps > (1u << 20)) return "at most 2^20 bitmaps";
	const uint32_t nShapes = (uint32_t) h.shapeBsdf.size(), nBsdfs = (uint32_t) h.bsdfType.size();
	const size_t nTris = h.triIdx.size() / 3;
	for (uint32_t k = 0; k < a.n_textures; ++k) {
		const std::string why = checkUvTexture(a.textures[k], a.withBitmaps);
		if (!why.empty()) return "texture " + std::to_string(k) + ": " + why;
	}
	// the bitmaps, the place of each in the pool, and the descriptors of the textures that show one
	std::vector<uint32_t> first(a.n_bitmaps, 0u);
	uint64_t nTexels = 0;
	for (uint32_t b = 0; b < a.n_bitmaps; ++b) {
		first[b] = (uint32_t) nTexels;
		const std::string why = checkBitmap(a.bitmaps[b], &nTexels);
		if (!why.empty()) return "bitmap " + std::to_string(b) + ": " + why;
	}
	std::vector<DTexture> &desc = out.desc;
	desc.resize(a.n_textures);
	for (uint32_t k = 0; k < a.n_textures; ++k) {
		std::memcpy(&desc[k], &a.textures[k], sizeof(DTexture));
		if (a.textures[k].kind != (uint32_t) MTSGPU_TEX_BITMAP) continue;
		const int32_t b = a.texture_bitmap ? a.texture_bitmap[k] : -1;
		if (b < 0 || (uint32_t) b >= a.n_bitmaps)
			return "texture " + std::to_string(k) + ": bitmap index " + std::to_string(b) + " out of range (" + std::to_string(a.n_bitmaps) + " bitmaps)";
		desc[k].width = a.bitmaps[b].width; desc[k].height = a.bitmaps[b].height; desc[k].wrap = a.bitmaps[b].wrap_mode; desc[k].first = first[b];
		desc[k].reserved[0] = desc[k].reserved[1] = desc[k].reserved[2] = 0u;
		out.anyBitmap = true;
	}
	if (a.bsdf_slot_texture) {
		const std::string why = checkBsdfSlotTextures(nBsdfs, h.bsdfType.data(), h.bsdfParams.data(), a.bsdf_slot_texture, a.n_textures, in);
		if (!why.empty()) return why;
		for (size_t i = 0; i < 2 * (size_t) nBsdfs; ++i) out.anySlot |= a.bsdf_slot_texture[i] >= 0;
	}
	if (a.bsdf_mask && h.hasShapes == kHasCylinders)
		for (uint32_t b = 0; b < nBsdfs; ++b)
			if (a.bsdf_mask[b].kind != (uint32_t) MTSGPU_MASK_NONE)
				return "BSDF " + std::to_string(b) + ": the mask BSDF is not served in a scene with a cylinder yet (the mask kernels do not build a cylinder's record)";
	if (a.bsdf_mask) {
		const std::string why = checkBsdfMasks(nBsdfs, h.bsdfType.data(), h.bsdfParams.data(), a.bsdf_mask, a.n_textures);
		if (!why.empty()) return why;
		for (uint32_t b = 0; b < nBsdfs; ++b) {
			out.anyMask |= a.bsdf_mask[b].kind != (uint32_t) MTSGPU_MASK_NONE;
			out.anyMaskTex |= a.bsdf_mask[b].kind == (uint32_t) MTSGPU_MASK_TEXTURE;
		}
	}
	// an entry mtsgpu_set_snow_bsdfs has given a snow record takes neither a textured slot nor a mask
	for (uint32_t b = 0; b < nBsdfs; ++b) {
		std::string held = claimRefusal(kFamTextures, b, textureSlotsClaimed(a.bsdf_slot_texture, b), in, kFamSnow);
		if (held.empty()) held = claimRefusal(kFamMasks, b, a.bsdf_mask && a.bsdf_mask[b].kind != (uint32_t) MTSGPU_MASK_NONE, in, kFamSnow);
		if (!held.empty()) return held;
	}
	// the casts of texture k on shape s (s == nShapes: on no shape, at uv = 0); the reason, or an empty string
	const size_t US = 4 * (size_t) kTriUvStride;
	std::vector<float> &triUv = out.triUv;
	auto castRange = [&](uint32_t s, int32_t k) -> std::string {
		bool ok = true;
		const mtsgpu_uv_texture &t = a.textures[k];
		const bool bitmap = t.kind == (uint32_t) MTSGPU_TEX_BITMAP;
		const double sx = bitmap ? (double) desc[k].width : 2.0, sy = bitmap ? (double) desc[k].height : 2.0;
		const bool mesh = s < nShapes && h.shapeType[s] == MTSGPU_SHAPE_TRIMESH, hasUv = s < nShapes && a.shape_has_uv && a.shape_has_uv[s];
		if (s < nShapes && !mesh) ok = uvCastInRange(t, 0.0f, 0.0f, sx, sy) && uvCastInRange(t, 1.0f, 1.0f, sx, sy);
		else if (!hasUv) ok = uvCastInRange(t, 0.0f, 0.0f, sx, sy);
		else
			for (uint32_t p = h.shapeTriOffset[s]; ok && p < h.shapeTriOffset[s + 1]; ++p)
				for (int v = 0; v < 3; ++v)
					ok = ok && uvCastInRange(t, triUv[US * (size_t) p + 2 * v], triUv[US * (size_t) p + 2 * v + 1], sx, sy);
		if (ok) return std::string();
		return "texture " + std::to_string(k) + " maps a texcoord outside the range of the (int) cast ("
		       + (bitmap ? "|uv' * size|" : "|2 uv'|") + " >= 2^31 - 2^16)";
	};
	// the gather array: the texcoords of the three vertices of every primitive of a mesh that has them, zero elsewhere
	triUv.assign(US * (nTris + 1), 0.0f);
	for (uint32_t s = 0; s < nShapes; ++s) {
		const bool hasUv = a.shape_has_uv && a.shape_has_uv[s];
		const bool mesh = h.shapeType[s] == MTSGPU_SHAPE_TRIMESH;
		if (hasUv && !mesh) return shapeMsg(s, "only a triangle mesh can carry texture coordinates");
		uint32_t bad;
		if (hasUv && !gatherMeshRows(h.triIdx.data(), h.shapeTriOffset[s], h.shapeTriOffset[s + 1], a.vtx_uv, 2, kTriUvStride, triUv.data(), &bad))
			return shapeMsg(s, "non-finite texcoord at vertex " + std::to_string(bad));
		// the casts of the textures this shape is shaded with
		const int32_t b = h.shapeBsdf[s];
		if (b < 0) continue;
		for (int slot = 0; a.bsdf_slot_texture && slot < 2; ++slot) {
			const int32_t k = a.bsdf_slot_texture[2 * (size_t) b + slot];
			if (k < 0) continue;
			const std::string why = castRange(s, k);
			if (!why.empty()) return shapeMsg(s, why);
		}
		// ... and of the texture its mask reads
		if (a.bsdf_mask && a.bsdf_mask[b].kind == (uint32_t) MTSGPU_MASK_TEXTURE) {
			const std::string why = castRange(s, a.bsdf_mask[b].texture);
			if (!why.empty()) return shapeMsg(s, "BSDF " + std::to_string(b) + ": the opacity of its mask: " + why);
		}
	}
	// a textured mask on a BSDF that no shape uses: the texture's offsets alone
	if (out.anyMaskTex) {
		std::vector<bool> used(nBsdfs, false);
		for (uint32_t s = 0; s < nShapes; ++s)
			if (h.shapeBsdf[s] >= 0) used[h.shapeBsdf[s]] = true;
		for (uint32_t b = 0; b < nBsdfs; ++b) {
			if (used[b] || a.bsdf_mask[b].kind != (uint32_t) MTSGPU_MASK_TEXTURE) continue;
			const std::string why = castRange(nShapes, a.bsdf_mask[b].texture);
			if (!why.empty()) return "BSDF " + std::to_string(b) + ": the opacity of its mask: " + why;
		}
	}
	if (!out.anySlot && !a.vtx_uv && !out.anyMask) return std::string();       // nothing to keep
	out.keep = true;
	if (!out.anySlot && !out.anyMaskTex) desc.clear();
	// (a mask keeps the textures and the bitmaps when no slot uses them)
	if ((out.anySlot || out.anyMaskTex) && out.anyBitmap) {
		out.pool.resize(4 * (size_t) nTexels);
		for (uint32_t b = 0; b < a.n_bitmaps; ++b) packBitmapTexels(a.bitmaps[b], &out.pool[4 * (size_t) first[b]]);
	}
	if (a.vtx_uv) {
		out.shapeHasUv.assign(a.shape_has_uv, a.shape_has_uv + nShapes);
		out.uvRange.assign(4 * (size_t) nShapes, 0.0);
		for (uint32_t s = 0; s < nShapes; ++s) {
			if (!a.shape_has_uv[s]) continue;
			double *r = &out.uvRange[4 * (size_t) s];
			bool none = true;
			for (uint32_t t = h.shapeTriOffset[s]; t < h.shapeTriOffset[s + 1]; ++t)
				for (int v = 0; v < 3; ++v) {
					const double u = triUv[US * (size_t) t + 2 * v], w = triUv[US * (size_t) t + 2 * v + 1];
					if (none) { r[0] = r[1] = u; r[2] = r[3] = w; none = false; }
					r[0] = std::min(r[0], u); r[1] = std::max(r[1], u); r[2] = std::min(r[2], w); r[3] = std::max(r[3], w);
				}
		}
	}
	return std::string();
}

std::string planSpots(uint32_t nLums, const uint32_t *lumType, const float *lumParams, const SpotArgs &a, bool haveMask, bool haveSnow,
                      bool haveCloth, SpotPlan &out) {
	out = SpotPlan();
	if (!a.textures && !a.bitmaps && !a.texture_bitmap && !a.texture_bilinear && !a.lum_texture) return std::string();
	if (!a.lum_texture) return "textures without lum_texture";
	if (a.n_textures && !a.textures) return "n_textures without textures";
	if (a.n_textures > (1u << 20)) return "at most 2^20 textures";
	if (a.n_bitmaps && !a.bitmaps) return "n_bitmaps without bitmaps";
	if (a.n_bitmaps > (1u << 20)) return "at most 2^20 bitmaps";
	for (uint32_t k = 0; k < a.n_textures; ++k) {
		const std::string why = checkUvTexture(a.textures[k], true);
		if (!why.empty()) return "texture " + std::to_string(k) + ": " + why;
		if (a.texture_bilinear && a.texture_bilinear[k] > 1u)
			return "texture " + std::to_string(k) + ": unknown filter flag " + std::to_string(a.texture_bilinear[k]) + " (0 = nearest, 1 = bilinear)";
	}
	std::vector<uint32_t> first(a.n_bitmaps, 0u);
	uint64_t nTexels = 0;
	for (uint32_t b = 0; b < a.n_bitmaps; ++b) {
		first[b] = (uint32_t) nTexels;
		const std::string why = checkBitmap(a.bitmaps[b], &nTexels);
		if (!why.empty()) return "bitmap " + std::to_string(b) + ": " + why;
	}
	std::vector<DTexture> &desc = out.desc;
	desc.resize(a.n_textures);
	bool anyBitmap = false;
	const double lim = 2147483648.0 - 65536.0;
	for (uint32_t k = 0; k < a.n_textures; ++k) {
		const mtsgpu_uv_texture &t = a.textures[k];
		std::memcpy(&desc[k], &t, sizeof(DTexture));
		double size = 2.0;
		if (t.kind == (uint32_t) MTSGPU_TEX_BITMAP) {
			const int32_t b = a.texture_bitmap ? a.texture_bitmap[k] : -1;
			if (b < 0 || (uint32_t) b >= a.n_bitmaps)
				return "texture " + std::to_string(k) + ": bitmap index " + std::to_string(b) + " out of range (" + std::to_string(a.n_bitmaps) + " bitmaps)";
			const mtsgpu_bitmap &bm = a.bitmaps[b];
			const bool bilinear = a.texture_bilinear && a.texture_bilinear[k] == 1u;
			if (bilinear && ((bm.width & (bm.width - 1u)) != 0u || (bm.height & (bm.height - 1u)) != 0u))
				return "texture " + std::to_string(k) + ": a filtered (trilinear / ewa) bitmap of " + std::to_string(bm.width) + " x " + std::to_string(bm.height)
				       + " texels: the reference resamples a size that is not a power of two with a Lanczos kernel first (mipmap.cpp:34-88), not done here";
			desc[k].width = bm.width; desc[k].height = bm.height; desc[k].wrap = bm.wrap_mode; desc[k].first = first[b];
			desc[k].reserved[0] = bilinear ? kSpotBilinear : 0u; desc[k].reserved[1] = desc[k].reserved[2] = 0u;
			size = std::max(2.0, (double) std::max(bm.width, bm.height));
			anyBitmap = true;
		}
		// uv lies in [0, 1] up to rounding: |uv'| <= |scale| + |offset|, and the margin of 1 covers the rounding, the half-texel
		// shift and the second tap of the bilinear lookup
		if (!((std::fabs((double) t.uscale) + std::fabs((double) t.uoffset) + 1.0) * size < lim)
		    || !((std::fabs((double) t.vscale) + std::fabs((double) t.voffset) + 1.0) * size < lim))
			return "texture " + std::to_string(k) + " can map uv outside the range of the (int) cast ((|scale| + |offset| + 1) * max(2, width, height) >= 2^31 - 2^16)";
	}
	bool any = false;
	out.uvFactor.assign(nLums, 0.0f);
	for (uint32_t l = 0; l < nLums; ++l) {
		const int32_t k = a.lum_texture[l];
		const std::string who = "luminaire " + std::to_string(l) + ": ";
		if (k < -1 || k >= (int64_t) a.n_textures) return who + "texture index " + std::to_string(k) + " out of range (" + std::to_string(a.n_textures) + " textures)";
		if (k < 0) continue;
		if (lumType[l] != (uint32_t) MTSGPU_LUM_SPOT) return who + "a projection texture on a luminaire that is not a spot (type " + std::to_string(lumType[l]) + ")";
		const float *P = lumParams + (size_t) MTSGPU_LUM_NPARAMS * l;
		// ([9], invTransitionWidth, is infinite where beamWidth = cutoffAngle, as in the reference, and then never read)
		for (int i = 0; i < 20; ++i) if (i != 9 && !std::isfinite(P[i])) return who + "non-finite spot parameter";
		// below 90 degrees localDir.z > cosCutoff > 0 where uv is formed
		if (!(P[8] < 0.5f * kPi) || !(std::cos((double) P[8]) > 0.0) || !(P[7] > 0.0f))
			return who + "a textured spot needs cutoffAngle < 90 degrees (from there on the division that forms uv and the casts of the lookup have no bound)";
		const float f = spotUvFactor(P[8]);
		if (!std::isfinite(f) || !(f > 0.0f)) return who + "uvFactor = tan(cutoffAngle) is not finite and positive";
		out.uvFactor[l] = f;
		any = true;
	}
	if (!any) { out = SpotPlan(); return std::string(); }      // nothing to keep: the context launches what it launches without the call
	if (haveMask) return spotBesideRefusal("the mask BSDF");
	if (haveSnow) return spotBesideRefusal("a snow BRDF");
	if (haveCloth) return spotBesideRefusal("the cloth BRDF");
	out.keep = true;
	if (anyBitmap) {
		out.pool.resize(4 * (size_t) nTexels);
		for (uint32_t b = 0; b < a.n_bitmaps; ++b) packBitmapTexels(a.bitmaps[b], &out.pool[4 * (size_t) first[b]]);
	}
	return std::string();
}

static_assert(sizeof(mtsgpu_yarn) == 56 && sizeof(mtsgpu_yarn) == sizeof(DYarn) && offsetof(mtsgpu_yarn, kd) == offsetof(DYarn, kd), "mtsgpu_yarn and DYarn are one layout");
static_assert(sizeof(DWeave) == 96 && offsetof(mtsgpu_weave, n_yarns) + 4 == offsetof(DWeave, first_pattern) && offsetof(mtsgpu_weave, pattern) == 80,
              "DWeave is the scalars of mtsgpu_weave, then the place of its arrays");

std::string planCloth(const HostScene &h, const InForce &in, uint32_t n_weaves, const mtsgpu_weave *weaves, const int32_t *bsdf_weave, ClothPlan &out) {
	out = ClothPlan();
	if (!bsdf_weave) return std::string();
	if (h.hasShapes == kHasCylinders)
		return "the cloth BRDF is not served in a scene with a cylinder yet (the cloth kernels do not build a cylinder's record)";
	if (n_weaves && !weaves) return "n_weaves without weaves";
	if (n_weaves > (1u << 20)) return "at most 2^20 weaves";
	const uint32_t nBsdfs = (uint32_t) h.bsdfType.size(), nShapes = (uint32_t) h.shapeBsdf.size();
	for (uint32_t k = 0; k < n_weaves; ++k) {
		const std::string why = checkWeave(weaves[k]);
		if (!why.empty()) return "weave " + std::to_string(k) + ": " + why;
	}
	bool any = false;
	for (uint32_t b = 0; b < nBsdfs; ++b) {
		const int32_t k = bsdf_weave[b];
		const std::string who = "BSDF " + std::to_string(b) + ": ";
		if (k < -1 || k >= (int32_t) n_weaves) return who + "weave index " + std::to_string(k) + " out of range (" + std::to_string(n_weaves) + " weaves)";
		if (k < 0) continue;
		any = true;
		if ((h.bsdfType[b] & ~(uint32_t) MTSGPU_BSDF_TWOSIDED) != (uint32_t) MTSGPU_BSDF_LAMBERTIAN)
			return who + "a weave sits on a Lambertian entry (twosided allowed), not on type word " + std::to_string(h.bsdfType[b]);
		const std::string held = claimRefusal(kFamCloth, b, 1u, in);
		if (!held.empty()) return held;
	}
	for (uint32_t b = 0; b < nBsdfs; ++b) {
		if ((h.bsdfType[b] & 0xFFu) != MTSGPU_BSDF_COMPOSITE) continue;
		const float *P = h.bsdfParams.data() + (size_t) MTSGPU_BSDF_NPARAMS * b;
		const int n = (int) P[0];
		for (int i = 0; i < n; ++i)
			if (bsdf_weave[(uint32_t) P[1 + n + i]] >= 0)
				return "BSDF " + std::to_string(b) + ": composite child " + std::to_string(i) + " has a weave: the composite's loop would run it as a Lambertian, not supported";
	}
	if (!any) return std::string();           // nothing to keep: the context launches what it launches without a table
	// the shapes a weave is shaded on: texcoords, a tangent frame, and the casts of f at the extremes of their texcoords
	for (uint32_t s = 0; s < nShapes; ++s) {
		const int32_t b = h.shapeBsdf[s];
		if (b < 0 || bsdf_weave[b] < 0) continue;
		double uMin = 0, uMax = 1, vMin = 0, vMax = 1;      // a sphere: uv in [0, 1]^2
		if (h.shapeType[s] == MTSGPU_SHAPE_TRIMESH) {
			const std::string bsdf = "the cloth BSDF (BSDF " + std::to_string(b) + ") ";
			if (!in.shapeHasUv || !in.shapeHasUv[s])
				return shapeMsg(s, bsdf + "needs texture coordinates: a mesh without them must be given some (trimesh.cpp:551-555)");
			if (h.shapeNormals[s] && !h.shapeTangents[s])
				return shapeMsg(s, bsdf + "is anisotropic: a mesh with vertex normals needs its tangents (mtsgpu_upload_scene_tangents)");
			const double *r = &in.uvRange[4 * (size_t) s];
			uMin = r[0]; uMax = r[1]; vMin = r[2]; vMax = r[3];
		}       // (a sphere's its.uv comes from the hit point: it needs no texture call)
		const std::string why = clothCastRange(weaves[bsdf_weave[b]], uMin, uMax, vMin, vMax);
		if (!why.empty()) return shapeMsg(s, "weave " + std::to_string(bsdf_weave[b]) + ": " + why);
	}
	// one pool: the records, the pattern words and the yarns
	out.keep = true;
	out.weaves.resize(n_weaves);
	for (uint32_t k = 0; k < n_weaves; ++k) {
		DWeave &rec = out.weaves[k];
		std::memset(&rec, 0, sizeof(DWeave));
		std::memcpy(&rec, &weaves[k], offsetof(mtsgpu_weave, pattern));
		rec.first_pattern = (uint32_t) out.pattern.size(); rec.first_yarn = (uint32_t) out.yarns.size();
		out.pattern.insert(out.pattern.end(), weaves[k].pattern, weaves[k].pattern + weaves[k].n_pattern);
		const DYarn *y = reinterpret_cast<const DYarn *>(weaves[k].yarns);
		out.yarns.insert(out.yarns.end(), y, y + weaves[k].n_yarns);
	}
	return std::string();
}

} // namespace mg
