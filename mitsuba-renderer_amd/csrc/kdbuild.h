// kdbuild.h -- what the three units of the kd-tree builder share, private to them: kdbuild.cpp (the reference's builder
// on the host, buildKdTree), kdbuild_bin.hip (binning phase on the device), kdbuild_exact.hip (exact phase on the device).
// Plain C++: KD_HD is the only trace of HIP here, what the device units need of it is in kdbuild_dev.h.
#pragma once
#include "kdtree.h"
#include <cmath>
#include <functional>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>

#ifdef __HIPCC__
#define KD_HD __host__ __device__
#else
#define KD_HD
#endif

namespace mg {
namespace kd {

constexpr float kInf = std::numeric_limits<float>::infinity();
constexpr float kEps = 1e-4f;
// std::min(a, b) = (b < a) ? b : a and std::max(a, b) = (a < b) ? b : a, usable on the device
KD_HD inline float hdMin(float a, float b) { return (b < a) ? b : a; }
KD_HD inline float hdMax(float a, float b) { return (a < b) ? b : a; }

struct Box {
	float mn[3], mx[3];
	KD_HD void reset() { for (int i = 0; i < 3; ++i) { mn[i] = kInf; mx[i] = -kInf; } }
	KD_HD void expand(const float *p) { for (int i = 0; i < 3; ++i) { mn[i] = hdMin(mn[i], p[i]); mx[i] = hdMax(mx[i], p[i]); } }
	KD_HD void expand(const Box &b) { for (int i = 0; i < 3; ++i) { mn[i] = hdMin(mn[i], b.mn[i]); mx[i] = hdMax(mx[i], b.mx[i]); } }
	KD_HD void clip(const Box &b) { for (int i = 0; i < 3; ++i) { mn[i] = hdMax(mn[i], b.mn[i]); mx[i] = hdMin(mx[i], b.mx[i]); } }
	KD_HD bool valid() const { for (int i = 0; i < 3; ++i) if (mx[i] < mn[i]) return false; return true; }
	KD_HD float area() const {            // aabb.h:326-329
		const float dx = mx[0] - mn[0], dy = mx[1] - mn[1], dz = mx[2] - mn[2];
		return (float) 2.0 * (dx * dy + dx * dz + dy * dz);
	}
};

// Sutherland-Hodgman against one plane, double precision (triangle.cpp:61-106).  static, like primBox below: local to each unit
KD_HD static inline int clipPlane(const double (*in)[3], int inCount, double (*out)[3], int axis, double splitPos, bool isMinimum) {
	if (inCount < 3)
		return 0;
	double cur[3] = { in[0][0], in[0][1], in[0][2] };
	const double sign = isMinimum ? 1.0f : -1.0f;
	double distance = sign * (cur[axis] - splitPos);
	bool curIsInside = (distance >= 0);
	int outCount = 0;
	for (int i = 0; i < inCount; ++i) {
		const int nextIdx = (i + 1 == inCount) ? 0 : i + 1;
		const double next[3] = { in[nextIdx][0], in[nextIdx][1], in[nextIdx][2] };
		distance = sign * (next[axis] - splitPos);
		const bool nextIsInside = (distance >= 0);
		if (curIsInside && nextIsInside) {
			for (int c = 0; c < 3; ++c) out[outCount][c] = next[c];
			outCount++;
		} else if (curIsInside != nextIsInside) {
			const double t = (splitPos - cur[axis]) / (next[axis] - cur[axis]);
			for (int c = 0; c < 3; ++c) out[outCount][c] = cur[c] + (next[c] - cur[c]) * t;
			out[outCount][axis] = splitPos;
			outCount++;
			if (nextIsInside) {
				for (int c = 0; c < 3; ++c) out[outCount][c] = next[c];
				outCount++;
			}
		}
		for (int c = 0; c < 3; ++c) cur[c] = next[c];
		curIsInside = nextIsInside;
	}
	return outCount;
}

// Triangle::getClippedAABB (triangle.cpp:108-158): clip in double, round outward to float
KD_HD static inline bool clippedTriangleBoxHD(const float *p0, const float *p1, const float *p2, const float *bmin, const float *bmax,
                                       float *omin, float *omax) {
	const float inf = INFINITY;
	double a[10][3], b[10][3];
	for (int c = 0; c < 3; ++c) { a[0][c] = p0[c]; a[1][c] = p1[c]; a[2][c] = p2[c]; }
	int n = 3;
	for (int axis = 0; axis < 3; ++axis) {
		n = clipPlane(a, n, b, axis, (double) bmin[axis], true);
		n = clipPlane(b, n, a, axis, (double) bmax[axis], false);
	}
	for (int c = 0; c < 3; ++c) { omin[c] = inf; omax[c] = -inf; }
	for (int i = 0; i < n; ++i)
		for (int j = 0; j < 3; ++j) {
			const double pos_d = a[i][j];
			const float pos_f = (float) pos_d;
			float lo, hi;
			if (pos_f < pos_d) { lo = pos_f; hi = nextafterf(pos_f, inf); }
			else if (pos_f > pos_d) { hi = pos_f; lo = nextafterf(pos_f, -inf); }
			else lo = hi = pos_f;
			omin[j] = hdMin(omin[j], lo);
			omax[j] = hdMax(omax[j], hi);
		}
	for (int c = 0; c < 3; ++c) { omin[c] = hdMax(omin[c], bmin[c]); omax[c] = hdMin(omax[c], bmax[c]); }
	for (int c = 0; c < 3; ++c)
		if (omax[c] < omin[c])
			return false;
	return true;
}

// ---------------------------------------------------------------------------
// Cylinder::getClippedAABB (src/shapes/cylinder.cpp:216-375), operation for operation in binary32 (the units are compiled
// without FMA contraction).  One text for the host builder and the device exact phase.  cyl = one row of the builder's
// cylinder table (kCylRow floats): cylPt = objectToWorld(Point(0,0,0)), cylD = objectToWorld(Vector(0,0,1)), radius, 1.
// ---------------------------------------------------------------------------
constexpr int kCylRow = 8;
struct F3 { float x, y, z; };
KD_HD inline float f3at(const F3 &a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }
KD_HD inline void f3set(F3 &a, int i, float v) { if (i == 0) a.x = v; else if (i == 1) a.y = v; else a.z = v; }
KD_HD inline F3 f3add(F3 a, F3 b) { return F3{ a.x + b.x, a.y + b.y, a.z + b.z }; }
KD_HD inline F3 f3sub(F3 a, F3 b) { return F3{ a.x - b.x, a.y - b.y, a.z - b.z }; }
KD_HD inline F3 f3mul(F3 a, float s) { return F3{ a.x * s, a.y * s, a.z * s }; }
KD_HD inline float f3dot(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
KD_HD inline F3 f3cross(F3 a, F3 b) { return F3{ a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }
// solveQuadratic (src/libcore/util.cpp:450-488)
KD_HD inline bool kdSolveQuadratic(float a, float b, float c, float &x0, float &x1) {
	if (a == 0) {
		if (b != 0) { x0 = x1 = -c / b; return true; }
		return false;
	}
	const float discrim = b * b - 4.0f * a * c;
	if (discrim < 0)
		return false;
	const float sqrtDiscrim = sqrtf(discrim);
	float temp;
	if (b < 0) temp = -0.5f * (b - sqrtDiscrim);
	else       temp = -0.5f * (b + sqrtDiscrim);
	x0 = temp / a;
	x1 = c / temp;
	if (x0 > x1) { const float t = x0; x0 = x1; x1 = t; }
	return true;
}
// intersectCylPlane (cylinder.cpp:216-255): the ellipse an infinite cylinder cuts out of a plane
KD_HD inline bool cylPlane(F3 planePt, F3 planeNrml, F3 cylPt, F3 cylD, float radius, F3 &center, F3 *axes, float *lengths) {
	if (fabsf(f3dot(planeNrml, cylD)) < kEps)
		return false;
	F3 B, A = f3sub(cylD, f3mul(planeNrml, f3dot(cylD, planeNrml)));
	const float length = sqrtf(A.x * A.x + A.y * A.y + A.z * A.z);
	if (length != 0) {
		const float recip = 1.0f / length;
		A = F3{ A.x * recip, A.y * recip, A.z * recip };
		B = f3cross(planeNrml, A);
	} else {
		// coordinateSystem (util.cpp:602-611)
		if (fabsf(planeNrml.x) > fabsf(planeNrml.y)) {
			const float invLen = 1.0f / sqrtf(planeNrml.x * planeNrml.x + planeNrml.z * planeNrml.z);
			A = F3{ -planeNrml.z * invLen, 0.0f, planeNrml.x * invLen };
		} else {
			const float invLen = 1.0f / sqrtf(planeNrml.y * planeNrml.y + planeNrml.z * planeNrml.z);
			A = F3{ 0.0f, -planeNrml.z * invLen, planeNrml.y * invLen };
		}
		B = f3cross(planeNrml, A);
	}
	const F3 delta = f3sub(planePt, cylPt), deltaProj = f3sub(delta, f3mul(cylD, f3dot(delta, cylD)));
	const float aDotD = f3dot(A, cylD), bDotD = f3dot(B, cylD);
	const float c0 = 1 - aDotD * aDotD, c1 = 1 - bDotD * bDotD;
	const float c2 = 2 * f3dot(A, deltaProj), c3 = 2 * f3dot(B, deltaProj);
	const float c4 = f3dot(delta, deltaProj) - radius * radius;
	const float lambda = (c2 * c2 / (4 * c0) + c3 * c3 / (4 * c1) - c4) / (c0 * c1);
	const float alpha0 = -c2 / (2 * c0), beta0 = -c3 / (2 * c1);
	lengths[0] = sqrtf(c1 * lambda);
	lengths[1] = sqrtf(c0 * lambda);
	center = f3add(f3add(planePt, f3mul(A, alpha0)), f3mul(B, beta0));
	axes[0] = A; axes[1] = B;
	return true;
}
// intersectCylFace (cylinder.cpp:257-330); points whose coordinates are NaN (beta / alpha with alpha == 0, a negative lambda)
// fail contains() and the [0, 1] tests as they do there
KD_HD inline Box cylFace(int axis, F3 mn, F3 mx, F3 cylPt, F3 cylD, float radius) {
	const int axis1 = (axis + 1) % 3, axis2 = (axis + 2) % 3;
	F3 planeNrml{ 0.0f, 0.0f, 0.0f };
	f3set(planeNrml, axis, 1.0f);
	F3 ellipseCenter, ellipseAxes[2];
	float ellipseLengths[2];
	Box aabb; aabb.reset();
	if (!cylPlane(mn, planeNrml, cylPt, cylD, radius, ellipseCenter, ellipseAxes, ellipseLengths))
		return aabb;
	for (int i = 0; i < 4; ++i) {
		F3 p1, p2;
		f3set(p1, axis, f3at(mn, axis)); f3set(p2, axis, f3at(mn, axis));
		f3set(p1, axis1, ((i + 1) & 2) ? f3at(mn, axis1) : f3at(mx, axis1));
		f3set(p1, axis2, ((i + 0) & 2) ? f3at(mn, axis2) : f3at(mx, axis2));
		f3set(p2, axis1, ((i + 2) & 2) ? f3at(mn, axis1) : f3at(mx, axis1));
		f3set(p2, axis2, ((i + 1) & 2) ? f3at(mn, axis2) : f3at(mx, axis2));
		const float p1lx = f3dot(f3sub(p1, ellipseCenter), ellipseAxes[0]) / ellipseLengths[0];
		const float p1ly = f3dot(f3sub(p1, ellipseCenter), ellipseAxes[1]) / ellipseLengths[1];
		const float p2lx = f3dot(f3sub(p2, ellipseCenter), ellipseAxes[0]) / ellipseLengths[0];
		const float p2ly = f3dot(f3sub(p2, ellipseCenter), ellipseAxes[1]) / ellipseLengths[1];
		const float relx = p2lx - p1lx, rely = p2ly - p1ly;
		const float A = relx * relx + rely * rely;
		const float B = 2 * (p1lx * relx + p1ly * rely);
		const float C = (p1lx * p1lx + p1ly * p1ly) - 1;
		float x0, x1;
		if (kdSolveQuadratic(A, B, C, x0, x1)) {
			if (x0 >= 0 && x0 <= 1) { const F3 p = f3add(p1, f3mul(f3sub(p2, p1), x0)); const float q[3] = { p.x, p.y, p.z }; aabb.expand(q); }
			if (x1 >= 0 && x1 <= 1) { const F3 p = f3add(p1, f3mul(f3sub(p2, p1), x1)); const float q[3] = { p.x, p.y, p.z }; aabb.expand(q); }
		}
	}
	ellipseAxes[0] = f3mul(ellipseAxes[0], ellipseLengths[0]);
	ellipseAxes[1] = f3mul(ellipseAxes[1], ellipseLengths[1]);
	// the componentwise maxima of the ellipse
	for (int i = 0; i < 2; ++i) {
		const int j = (i == 0) ? axis1 : axis2;
		const float alpha = f3at(ellipseAxes[0], j), beta = f3at(ellipseAxes[1], j);
		const float ratio = beta / alpha, tmp = sqrtf(1 + ratio * ratio);
		const float cosTheta = 1 / tmp, sinTheta = ratio / tmp;
		const F3 p1 = f3add(f3add(ellipseCenter, f3mul(ellipseAxes[0], cosTheta)), f3mul(ellipseAxes[1], sinTheta));
		const F3 p2 = f3sub(f3sub(ellipseCenter, f3mul(ellipseAxes[0], cosTheta)), f3mul(ellipseAxes[1], sinTheta));
		const float q1[3] = { p1.x, p1.y, p1.z }, q2[3] = { p2.x, p2.y, p2.z }, lo[3] = { mn.x, mn.y, mn.z }, hi[3] = { mx.x, mx.y, mx.z };
		bool in1 = true, in2 = true;      // AABB::contains (aabb.h:133-138)
		for (int c = 0; c < 3; ++c) {
			if (q1[c] < lo[c] || q1[c] > hi[c]) in1 = false;
			if (q2[c] < lo[c] || q2[c] > hi[c]) in2 = false;
		}
		if (in1) aabb.expand(q1);
		if (in2) aabb.expand(q2);
	}
	return aabb;
}
// getClippedAABB (cylinder.cpp:332-375): own = getAABB(), to = the cell; false when the result is not valid
KD_HD inline bool cylinderClippedBox(const float *cyl, const Box &own, const Box &to, Box &out) {
	Box base = own;
	base.clip(to);
	const F3 cylPt{ cyl[0], cyl[1], cyl[2] }, cylD{ cyl[3], cyl[4], cyl[5] };
	const float radius = cyl[6];
	const float *n = base.mn, *x = base.mx;
	out.reset();
	out.expand(cylFace(0, F3{ n[0], n[1], n[2] }, F3{ n[0], x[1], x[2] }, cylPt, cylD, radius));
	out.expand(cylFace(0, F3{ x[0], n[1], n[2] }, F3{ x[0], x[1], x[2] }, cylPt, cylD, radius));
	out.expand(cylFace(1, F3{ n[0], n[1], n[2] }, F3{ x[0], n[1], x[2] }, cylPt, cylD, radius));
	out.expand(cylFace(1, F3{ n[0], x[1], n[2] }, F3{ x[0], x[1], x[2] }, cylPt, cylD, radius));
	out.expand(cylFace(2, F3{ n[0], n[1], n[2] }, F3{ x[0], x[1], n[2] }, cylPt, cylD, radius));
	out.expand(cylFace(2, F3{ n[0], n[1], x[2] }, F3{ x[0], x[1], x[2] }, cylPt, cylD, radius));
	out.clip(to);
	return out.valid();
}

// SurfaceAreaHeuristic (sahkdtree3.h:35-79)
struct SAH {
	float t0[3], t1[3];
	explicit SAH(const Box &b) {
		const float e[3] = { b.mx[0] - b.mn[0], b.mx[1] - b.mn[1], b.mx[2] - b.mn[2] };
		const float temp = 1.0f / (e[0] * e[1] + e[1] * e[2] + e[0] * e[2]);
		t0[0] = (e[1] * e[2]) * temp; t0[1] = (e[0] * e[2]) * temp; t0[2] = (e[0] * e[1]) * temp;
		t1[0] = (e[1] + e[2]) * temp; t1[1] = (e[0] + e[2]) * temp; t1[2] = (e[0] + e[1]) * temp;
	}
	void operator()(int axis, float leftWidth, float rightWidth, float &pl, float &pr) const {
		pl = t0[axis] + t1[axis] * leftWidth;
		pr = t0[axis] + t1[axis] * rightWidth;
	}
};

struct Split { float cost = kInf, pos = 0; int axis = 0; uint32_t numLeft = 0, numRight = 0; bool planarLeft = false; };
// a candidate split plane of the exact phase: how many primitives end on it, lie in it, start on it (indexed by event type)
enum : uint16_t { kEnd = 0, kPlanar = 1, kStart = 2 };
struct Candidate { float pos; int axis; uint32_t count[3]; };

struct Params {
	float traversalCost, queryCost, emptySpaceBonus;
	uint32_t stopPrims, maxBadRefines, exactPrimThreshold, maxDepth;
	int minMaxBins; bool clip, retract;
	// the caller's values, the reference's defaults where it gives none (gkdtree.h:711-724, :945-947)
	static Params from(const mtsgpu_kd_params *kp, uint32_t nPrims);
};

// The primitives by number.  `corners` says whether a primitive is a triangle and where its corners are; any other
// shape has its own box in genBox [n][6] (shape->getAABB(), skdtree.h:203-213).  The host reads the indexed mesh, the
// device exact phase nine floats per primitive (kdbuild_exact.hip); the boxes are the same expressions on both.
// cyl [n][kCylRow]: the cylinder table, NULL without a cylinder; row i is read when its last float is non-zero (a cylinder)
template <class Corners> struct GeometryOf { Corners corners; const float *genBox; const float *cyl; };
// static: a copy per unit, which the compiler sees through as it did the one-unit builder's local Geometry::box.  As inline
// members shared between units these were calls that may throw and write memory: the host binning loop ran 3-5 % slower
template <class G> KD_HD static void primBox(const G &g, uint32_t i, Box &b) {
	if (!g.corners.triangle(i)) {
		for (int a = 0; a < 3; ++a) { b.mn[a] = g.genBox[6 * (size_t) i + a]; b.mx[a] = g.genBox[6 * (size_t) i + 3 + a]; }
		return;
	}
	b.reset(); b.expand(g.corners.corner(i, 0)); b.expand(g.corners.corner(i, 1)); b.expand(g.corners.corner(i, 2));
}
template <class G> KD_HD static bool primClipped(const G &g, uint32_t i, const Box &to, Box &b) {
	if (!g.corners.triangle(i)) {
		if (g.cyl && g.cyl[kCylRow * (size_t) i + 7] != 0.0f) {      // Cylinder::getClippedAABB
			Box own; primBox(g, i, own);
			return cylinderClippedBox(g.cyl + kCylRow * (size_t) i, own, to, b);
		}
		primBox(g, i, b); b.clip(to);         // Shape::getClippedAABB (shape.cpp:59-63): getAABB().clip(box)
		return b.valid();
	}
	return clippedTriangleBoxHD(g.corners.corner(i, 0), g.corners.corner(i, 1), g.corners.corner(i, 2), to.mn, to.mx, b.mn, b.mx);
}
struct IndexedCorners {
	const float *vtx; const uint32_t *tri;      // a non-triangle primitive's tri row is {MTSGPU_KNOTRIANGLE x 3}
	KD_HD bool triangle(uint32_t i) const { return tri[3 * (size_t) i] != MTSGPU_KNOTRIANGLE; }
	KD_HD const float *corner(uint32_t i, int v) const { return vtx + 3 * (size_t) tri[3 * (size_t) i + v]; }
};
using Geometry = GeometryOf<IndexedCorners>;

// preliminary node: leaf {start, end} into the owning context's index list, inner {axis, children, split},
// or a reference to a subtree built by a job
struct PNode { uint8_t kind; uint32_t a, b; float split; };   // kind: 0 inner, 1 leaf, 2 job reference

// One build context = one independently growing piece of the tree (BuildContext, gkdtree.h)
struct Context {
	std::vector<PNode> nodes;
	std::vector<uint32_t> indices;
	uint32_t leafCount = 0, nonemptyLeafCount = 0, innerCount = 0, primIndexCount = 0, retracted = 0, pruned = 0;
	uint32_t allocNodes(uint32_t n) { const uint32_t r = (uint32_t) nodes.size(); nodes.resize(nodes.size() + n); return r; }
	std::vector<Candidate> planes;      // scratch of Builder::sweep: the candidate planes of the node being split

	// `node` becomes the leaf of the primitives appended to `indices` from `start` on
	void leaf(uint32_t node, uint32_t start, uint32_t primCount);
	void leafFromIndices(uint32_t node, const uint32_t *idx, uint32_t primCount);
	// `node` becomes an inner node with two new children (the left one, the right one follows); the mark keeps what
	// retract() needs to take its subtree back and leave one leaf of all its primitives (gkdtree.h:2327-2341, :1603-1637)
	struct Mark { uint32_t children, nodePos, indexPos, leafCount, nonemptyLeafCount, innerCount; };
	Mark openInner(uint32_t node, int axis, float split);
	void retract(uint32_t node, const Mark &mark);
};

struct Job { uint32_t depth; Box nodeBox; std::vector<uint32_t> prims; uint32_t badRefines; Context ctx; uint32_t root; double ms = 0; };

// (int64_t) of a bin coordinate as the x86 conversion the reference compiles to defines it: values outside the
// int64 range (a node that is flat along the axis divides by zero) give INT64_MIN; host and device agree on this
KD_HD inline int64_t binIndex(float v) {
	return (v >= -9223372036854775808.0f && v < 9223372036854775808.0f) ? (int64_t) v : (int64_t) 0x8000000000000000ull;
}

// Record of the min-max binning phase when it ran on the device: per node what minimizeCost chose, the unions of the
// boxes sent to either side and, for nodes the phase ends at, their primitive list
struct PlanNode {
	uint32_t count = 0;
	Split best;
	Box leftRaw, rightRaw;
	std::vector<uint32_t> prims;
	int child[2] = { -1, -1 };
};
struct Plan { std::vector<PlanNode> nodes; };

// The decisions of buildTreeMinMax that the host loop (Builder, kdbuild.cpp) and the device binning phase both take
struct Decisions {
	const Params &m_p;
	enum Early { kMakeLeaf, kDefer, kBin };
	Early early(uint32_t primCount, uint32_t depth) const {
		if (primCount <= m_p.stopPrims || depth >= m_p.maxDepth) return kMakeLeaf;
		if (primCount <= m_p.exactPrimThreshold) return kDefer;
		return kBin;
	}
	// what follows MinMaxBins::minimizeCost (gkdtree.h:1779-1800): 0 split, 1 leaf, 2 hand over to the exact method
	int afterMinimize(const Split &best, uint32_t primCount, uint32_t &badRefines) const {
		const float leafCost = primCount * m_p.queryCost;
		if (best.cost == kInf) return 2;
		if (best.cost >= leafCost) {
			if ((best.cost > 4 * leafCost && primCount < 16) || badRefines >= m_p.maxBadRefines) return 1;
			++badRefines;
		}
		return 0;
	}
	void binSetup(const Box &tight, float *binSize, float *invBinSize) const {
		const float recip = 1.0f / (float) m_p.minMaxBins;
		for (int a = 0; a < 3; ++a) { binSize[a] = (tight.mx[a] - tight.mn[a]) * recip; invBinSize[a] = 1 / binSize[a]; }
	}
	Split minimize(const Box &tight, const float *binSize, const float *invBinSize, const uint32_t *minBins, const uint32_t *maxBins, uint32_t primCount) const;
	void finishSplit(const Box &tight, Split &best, Box &leftBounds, Box &rightBounds, uint32_t numLeft, uint32_t numRight) const;
};

// Runs fn(item, worker) for the items 0 .. nItems - 1 on min(nThreads, nItems) threads, the calling one (worker 0) among
// them.  An exception that leaves a std::thread ends the process: the first one is kept, the other workers stop after
// their current item, and it is rethrown on the calling thread after the join, where mtsgpu_flatten makes it an error code
void runWorkers(int nThreads, size_t nItems, const std::function<void(size_t, int)> &fn);

// Runs the binning phase of the whole tree on the current HIP device and records it as a Plan (kdbuild_bin.hip)
void planOnDevice(const Decisions &b, const Params &p, const Geometry &g, uint32_t nPrims, const Box &scene, int nThreads, Plan &plan);
// Builds the subtrees of all jobs on the current HIP device; fills job.ctx, root = node 0 of the context (kdbuild_exact.hip)
void exactOnDevice(const Params &p, const Geometry &g, uint32_t nPrims, std::vector<std::unique_ptr<Job>> &jobs);

} // namespace kd
} // namespace mg
