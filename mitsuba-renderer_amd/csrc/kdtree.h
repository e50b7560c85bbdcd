// kdtree.h -- the kd-tree the builder hands to the flattener.  Plain C++: kdbuild.cpp includes this and not host.h.
#pragma once
#include "../../include/mtsgpu.h"
#include <cstdint>
#include <vector>

namespace mg {

struct KdTree {
	std::vector<uint32_t> nodes;      // 2 dwords per node
	std::vector<uint32_t> indices;
	float aabbMin[3] = { 0, 0, 0 }, aabbMax[3] = { 0, 0, 0 };
	double stats[6] = { 0, 0, 0, 0, 0, 0 };
};

// genBox: [nTris][6] boxes, read for the primitives whose tri row is {MTSGPU_KNOTRIANGLE x 3}; may be NULL without such
// cylTable: [nTris][8] = axis origin, axis direction, radius, 1 for the primitives that are cylinders (zero rows elsewhere), whose
// boxes are clipped as Cylinder::getClippedAABB clips them; NULL without a cylinder
void buildKdTree(const float *vtx, const uint32_t *tri, uint32_t nTris, const float *genBox, const mtsgpu_kd_params *kp, KdTree &out,
                 const float *cylTable = nullptr);
// Cylinder::getClippedAABB of the builder (kdbuild.h) on the host, or in a kernel of the device exact phase's unit: own6 =
// getAABB(), cyl8 = a row of cylTable, boxes [n][6], out [n][6], valid [n]
void cylinderClipHost(const float *cyl8, const float *own6, uint32_t n, const float *boxes, float *out, uint32_t *valid);
void cylinderClipDevice(const float *cyl8, const float *own6, uint32_t n, const float *boxes, float *out, uint32_t *valid);
bool clippedTriangleBox(const float *p0, const float *p1, const float *p2, const float *bmin, const float *bmax,
                        float *omin, float *omax);

} // namespace mg
