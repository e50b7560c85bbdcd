// kdbuild_exact.hip -- the exact phase of the kd-tree builder on the device: exactOnDevice (kdbuild.h).  Only this unit includes rocPRIM.
#include "kdbuild_dev.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/transform_iterator.hpp>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

namespace mg {
using namespace kd;
namespace {      // the kernels keep the names profiles and ISA comparisons know them by: mg::<unnamed>::k_x_*

// ---------------------------------------------------------------------------------------------------------------
// Device exact phase: buildTree (gkdtree.h:1898-2345), the O(n log n) sweep for nodes of at most exactPrimThreshold
// primitives, for ALL such subtrees ("jobs") at once, one tree level per round.
//
// The reference keeps one event list per node, sorted by (axis, position, type), and re-uses it down the tree with
// stable partitions and merges.  Here a node is the contiguous run of its primitive instances (primitive id + the box
// the primitive has inside the node), always in ascending primitive order, and every level
//   1. emits the edge events of all instances (createEventList, :1490-1530) with a 58-bit key
//      node | axis | position | type and sorts them with ONE stable radix sort (rocPRIM): events of equal key keep
//      the instance order, i.e. the primitive order, which is the tie rule of EventLess above;
//   2. turns the sweep (:1936-2021) into prefix sums over the sorted events: the counts in front of and up to a group
//      of events at one position give numLeft / numRight / numPlanar of that candidate plane, its cost is evaluated by
//      the group's last event with the reference's expressions, and an atomic minimum over (cost, event index) per node
//      finds the candidate the sequential loop keeps (the first of the cheapest);
//   3. lets the HOST take the decisions of :2023-2051 (leaf, bad refines) from that record with the same code path;
//   4. classifies every instance against the plane (:2053-2103), re-clips the straddlers in binary64
//      (Triangle::getClippedAABB, :2140-2219) and scatters the instances to the children with prefix sums (stable).
// Leaves get their primitive order on the host from the boxes of their instances.  When the last level is done the
// host replays the nodes depth first with the bookkeeping of buildTree (cost of the subtree, retraction :2327-2341,
// counters) into the Context of every job, so everything downstream -- and the tree -- is what runExact produces.
// ---------------------------------------------------------------------------------------------------------------
struct XInst { uint32_t prim; Box box; uint32_t node; };        // 32 B; node = index inside its level
// A node of the exact phase, resident on the device.  The nodes of one level are contiguous, the children of a level's
// split nodes form the next level (left, right, in node order).
struct XNodeG {
	Box box;                         // the node's box
	uint32_t primCount;              // what the sweep counts numRight down from
	uint32_t instBegin, instCount;   // its instances in the level's instance array
	uint32_t depth, badRefines;
	uint32_t sweep, isSplit, isLeaf;
	int32_t axis; float split; uint32_t planarLeft;
	uint32_t numLeft, numRight;      // of the chosen plane (gkdtree.h:1950-2016)
	uint32_t child;                  // global index of the left child (the right one follows)
	uint32_t childBase[2];           // where the children's instances start in the next level's array
	uint32_t pruned[2];              // straddlers whose clipped box in the left / right child is empty
	uint32_t leafOffset;             // a leaf's primitives in the leaf item buffer
	float cost; uint32_t retract;    // filled bottom-up when all levels are done
};
// what the host needs of a node for the replay
struct XNodeH { uint32_t primCount; int32_t kind; int32_t axis; float split; uint32_t child, pruned, leafOffset, leafCount, retract; };
struct XTotals { uint32_t nSplit, nNextInst, nLeafItems, pad; };
struct XParams { float traversalCost, queryCost, emptySpaceBonus; int clip; uint32_t stopPrims, maxDepth, maxBadRefines; int retract; };

constexpr uint64_t kXInvalid = ~0ull;
constexpr uint32_t kXMaxNodes = 1u << 22;       // nodes per level (22 bits of the event key)

#define KXHIP(x) hipCheck((x), "device exact phase")

__device__ inline uint32_t xOrderable(float v) {
	const uint32_t u = __float_as_uint(v);
	return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// where the device keeps the corners: nine floats per primitive, NaN in the first slot of a non-triangle primitive
struct SoupCorners {
	const float *triPos;
	__device__ bool triangle(uint32_t i) const { return triPos[9 * (size_t) i] == triPos[9 * (size_t) i]; }
	__device__ const float *corner(uint32_t i, int v) const { return triPos + 9 * (size_t) i + 3 * v; }
};
using XGeometry = GeometryOf<SoupCorners>;

// transitionToNLogN (gkdtree.h:1668-1704): the instances of the jobs' primitives; keep[i] = 0 drops a primitive whose
// clipped box is empty or has no area
// CYL: the instantiation that knows the cylinder table, launched for scenes that have one; the other one reads no table and
// keeps the registers it had before there were cylinders
template <bool CYL>
__global__ void k_x_init(const float *triPos, const float *genBox, const float *cyl, const uint32_t *prims, const uint32_t *primNode, uint32_t n,
                         const XNodeG *nodes, int clip, XInst *out, uint32_t *keep) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	XInst x; x.prim = prims[i]; x.node = primNode[i];
	const XNodeG &nd = nodes[x.node];
	bool ok = true;
	const XGeometry geo{ { triPos }, genBox, CYL ? cyl : nullptr };
	if (clip) ok = primClipped(geo, x.prim, nd.box, x.box) && x.box.area() != 0;
	else primBox(geo, x.prim, x.box);
	out[i] = x; keep[i] = ok ? 1u : 0u;
}
__global__ void k_x_compact(const XInst *in, const uint32_t *keep, const uint32_t *scan, uint32_t n, XInst *out) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n && keep[i]) out[scan[i] - 1u] = in[i];
}
// the roots after the compaction: their instance ranges from the inclusive scan of the keep flags
__global__ void k_x_roots(XNodeG *nodes, uint32_t n, const uint32_t *scan, XTotals *totals) {
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= n) return;
	XNodeG &nd = nodes[k];
	const uint32_t b = nd.instBegin, c = nd.instCount;
	const uint32_t before = b ? scan[b - 1] : 0u, kept = c ? scan[b + c - 1] - before : 0u;
	nd.instBegin = before; nd.instCount = kept; nd.primCount = kept;
	if (k == n - 1) { totals->nNextInst = before + kept; totals->nSplit = 0; totals->nLeafItems = 0; }
}

// the leaves that need no sweep (gkdtree.h:1903-1906)
__global__ void k_x_prep(XNodeG *nodes, uint32_t n, XParams prm) {
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= n) return;
	XNodeG &nd = nodes[k];
	const bool preLeaf = nd.primCount <= prm.stopPrims || nd.depth >= prm.maxDepth;
	nd.sweep = preLeaf ? 0u : 1u; nd.isLeaf = preLeaf ? 1u : 0u; nd.isSplit = 0u;
	nd.pruned[0] = nd.pruned[1] = 0u;
}

// createEventList: two key slots per instance and axis (a planar primitive uses one)
__global__ void k_x_emit(const XInst *inst, uint32_t n, const XNodeG *nodes, unsigned long long *keys, uint32_t *vals) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const XInst x = inst[i];
	const bool sweep = nodes[x.node].sweep != 0u;
	for (int a = 0; a < 3; ++a) {
		unsigned long long k0 = kXInvalid, k1 = kXInvalid;
		if (sweep) {
			const unsigned long long hi = (unsigned long long) (x.node * 4u + (uint32_t) a) << 34;
			if (x.box.mn[a] == x.box.mx[a]) k0 = hi | ((unsigned long long) monoKey(x.box.mn[a]) << 2) | (unsigned long long) kPlanar;
			else {
				k0 = hi | ((unsigned long long) monoKey(x.box.mn[a]) << 2) | (unsigned long long) kStart;
				k1 = hi | ((unsigned long long) monoKey(x.box.mx[a]) << 2) | (unsigned long long) kEnd;
			}
		}
		keys[6 * (size_t) i + 2 * a] = k0; keys[6 * (size_t) i + 2 * a + 1] = k1;
		vals[6 * (size_t) i + 2 * a] = i; vals[6 * (size_t) i + 2 * a + 1] = i;
	}
}
// per sorted event: the (index + 1) of the event that opens its group, and where the segments (node, axis) start; the
// three per-type counters of the sweep are read off the keys by the scans themselves (XIsType)
__global__ void k_x_flags(const unsigned long long *keys, uint32_t n, uint32_t *head, uint32_t *segStart) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const unsigned long long k = keys[i];
	const bool valid = k != kXInvalid;
	const unsigned long long prev = i ? keys[i - 1] : kXInvalid;
	head[i] = (valid && (i == 0 || (prev >> 2) != (k >> 2))) ? i + 1u : 0u;
	if (valid && (i == 0 || (prev >> 34) != (k >> 34))) segStart[(uint32_t) (k >> 34)] = i;
}

struct XIsType {
	uint32_t type;
	__host__ __device__ uint32_t operator()(unsigned long long k) const { return (k != kXInvalid && (uint32_t) (k & 3ull) == type) ? 1u : 0u; }
};

// the candidate plane of the group of events that ends at sorted position i (gkdtree.h:1950-2016)
struct XCand { bool valid; float cost, pos; uint32_t numLeft, numRight, planarLeft; int axis; uint32_t node; };
__device__ inline XCand xCandidate(uint32_t i, const unsigned long long *keys, const uint32_t *vals, const uint32_t *E, const uint32_t *P,
                                   const uint32_t *S, const uint32_t *H, const uint32_t *segStart, const XInst *inst, const XNodeG *nodes,
                                   const XParams prm) {
	XCand c; c.valid = false;
	const unsigned long long k = keys[i];
	const uint32_t seg = (uint32_t) (k >> 34);
	c.node = seg >> 2; c.axis = (int) (seg & 3u);
	const XNodeG &nd = nodes[c.node];
	const uint32_t h = H[i] - 1u, s0 = segStart[seg];
	const uint32_t Ph = h ? P[h - 1] : 0u, Sh = h ? S[h - 1] : 0u;
	const uint32_t Es = s0 ? E[s0 - 1] : 0u, Ps = s0 ? P[s0 - 1] : 0u, Ss = s0 ? S[s0 - 1] : 0u;
	const uint32_t numPlanar = P[i] - Ph;
	const uint32_t nL = (Sh - Ss) + (Ph - Ps);                     // starts and planars of the groups in front
	const uint32_t nR = nd.primCount - ((P[i] - Ps) + (E[i] - Es)); // minus planars and ends up to and including this group
	// the position is that of the group's first event (ev->pos), taken from the box: the key has lost the sign of zero
	const XInst &hx = inst[vals[h]];
	const uint32_t htype = (uint32_t) (keys[h] & 3ull);
	const float pos = htype == kEnd ? hx.box.mx[c.axis] : hx.box.mn[c.axis];
	c.pos = pos;
	const float nmn = nd.box.mn[c.axis], nmx = nd.box.mx[c.axis];
	if (!(pos > nmn && pos < nmx)) return c;
	// SurfaceAreaHeuristic (sahkdtree3.h:35-79)
	const float e0 = nd.box.mx[0] - nd.box.mn[0], e1 = nd.box.mx[1] - nd.box.mn[1], e2 = nd.box.mx[2] - nd.box.mn[2];
	const float temp = 1.0f / (e0 * e1 + e1 * e2 + e0 * e2);
	const float t0 = (c.axis == 0 ? (e1 * e2) : c.axis == 1 ? (e0 * e2) : (e0 * e1)) * temp;
	const float t1 = (c.axis == 0 ? (e1 + e2) : c.axis == 1 ? (e0 + e2) : (e0 + e1)) * temp;
	const float pl = t0 + t1 * (pos - nmn), pr = t0 + t1 * (nmx - pos);
	const float nLF = (float) nL, nRF = (float) nR;
	if (numPlanar == 0) {
		float cost = prm.traversalCost + prm.queryCost * (pl * nLF + pr * nRF);
		if (nL == 0 || nR == 0) cost *= prm.emptySpaceBonus;
		c.cost = cost; c.numLeft = nL; c.numRight = nR; c.planarLeft = 0;
	} else {
		float costPlanarLeft = prm.traversalCost + prm.queryCost * (pl * (float) (nL + numPlanar) + pr * nRF);
		float costPlanarRight = prm.traversalCost + prm.queryCost * (pl * nLF + pr * (float) (nR + numPlanar));
		if (nL + numPlanar == 0 || nR == 0) costPlanarLeft *= prm.emptySpaceBonus;
		if (nL == 0 || nR + numPlanar == 0) costPlanarRight *= prm.emptySpaceBonus;
		if (costPlanarLeft < costPlanarRight) { c.cost = costPlanarLeft; c.numLeft = nL + numPlanar; c.numRight = nR; c.planarLeft = 1; }
		else { c.cost = costPlanarRight; c.numLeft = nL; c.numRight = nR + numPlanar; c.planarLeft = 0; }
	}
	c.valid = c.cost == c.cost;       // a NaN cost never wins "cost < best.cost"
	return c;
}
__global__ void k_x_cost(const unsigned long long *keys, const uint32_t *vals, uint32_t n, const uint32_t *E, const uint32_t *P, const uint32_t *S,
                         const uint32_t *H, const uint32_t *segStart, const XInst *inst, const XNodeG *nodes, XParams prm,
                         unsigned long long *nodeBest) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const unsigned long long k = keys[i];
	if (k == kXInvalid) return;
	const unsigned long long next = (i + 1 < n) ? keys[i + 1] : kXInvalid;
	if (next != kXInvalid && (next >> 2) == (k >> 2)) return;          // not the last event of its group
	const XCand c = xCandidate(i, keys, vals, E, P, S, H, segStart, inst, nodes, prm);
	if (!c.valid) return;
	atomicMin(&nodeBest[c.node], ((unsigned long long) xOrderable(c.cost) << 32) | (unsigned long long) i);
}
// what follows the sweep (gkdtree.h:2023-2051): a leaf after all, a "bad refine", or the split
__global__ void k_x_decide(XNodeG *nodes, uint32_t nNodes, const unsigned long long *nodeBest, const unsigned long long *keys, const uint32_t *vals,
                           const uint32_t *E, const uint32_t *P, const uint32_t *S, const uint32_t *H, const uint32_t *segStart, const XInst *inst,
                           XParams prm) {
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= nNodes) return;
	XNodeG &nd = nodes[k];
	if (!nd.sweep) return;
	float cost = INFINITY, pos = 0; int axis = 0; uint32_t numLeft = 0, numRight = 0, planarLeft = 0;
	const unsigned long long v = nodeBest[k];
	if (v != ~0ull) {
		const XCand c = xCandidate((uint32_t) v, keys, vals, E, P, S, H, segStart, inst, nodes, prm);
		cost = c.cost; pos = c.pos; axis = c.axis; numLeft = c.numLeft; numRight = c.numRight; planarLeft = c.planarLeft;
	}
	const float leafCost = nd.primCount * prm.queryCost;
	bool leaf = false;
	if (cost >= leafCost) {
		if ((cost > 4 * leafCost && nd.primCount < 16) || nd.badRefines >= prm.maxBadRefines || cost == INFINITY) leaf = true;
		else nd.badRefines++;
	}
	if (leaf) { nd.isLeaf = 1u; return; }
	nd.isSplit = 1u; nd.axis = axis; nd.split = pos; nd.planarLeft = planarLeft; nd.numLeft = numLeft; nd.numRight = numRight;
}

// classification wrt. the chosen plane (gkdtree.h:2053-2103) and the boxes of the straddlers inside the children
// (perfect splits, :2140-2219)
template <bool CYL>
__global__ void k_x_classify(const XInst *inst, uint32_t n, XNodeG *nodes, const float *triPos, const float *genBox, const float *cyl, int clip,
                             uint32_t *goesL, uint32_t *goesR, uint32_t *isLeafInst, float *boxL, float *boxR) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const XInst x = inst[i];
	XNodeG &nd = nodes[x.node];
	uint32_t L = 0, R = 0;
	isLeafInst[i] = nd.isLeaf;
	if (nd.isSplit) {
		const int a = nd.axis;
		const float split = nd.split, mn = x.box.mn[a], mx = x.box.mx[a];
		bool both = false;
		if (mn == mx) {
			if (mn < split || (mn == split && nd.planarLeft)) L = 1;
			else if (mn > split || (mn == split && !nd.planarLeft)) R = 1;
			else both = true;
		} else if (mx <= split) L = 1;
		else if (mn >= split) R = 1;
		else both = true;
		for (int c = 0; c < 3; ++c) { boxL[6 * (size_t) i + c] = x.box.mn[c]; boxL[6 * (size_t) i + 3 + c] = x.box.mx[c]; boxR[6 * (size_t) i + c] = x.box.mn[c]; boxR[6 * (size_t) i + 3 + c] = x.box.mx[c]; }
		if (both) {
			L = R = 1;
			if (clip) {
				const XGeometry geo{ { triPos }, genBox, CYL ? cyl : nullptr };
				Box l = nd.box, r = nd.box, in;
				l.mx[a] = split; r.mn[a] = split;
				if (primClipped(geo, x.prim, l, in) && in.area() > 0) { for (int c = 0; c < 3; ++c) { boxL[6 * (size_t) i + c] = in.mn[c]; boxL[6 * (size_t) i + 3 + c] = in.mx[c]; } }
				else { L = 0; atomicAdd(&nd.pruned[0], 1u); }
				if (primClipped(geo, x.prim, r, in) && in.area() > 0) { for (int c = 0; c < 3; ++c) { boxR[6 * (size_t) i + c] = in.mn[c]; boxR[6 * (size_t) i + 3 + c] = in.mx[c]; } }
				else { R = 0; atomicAdd(&nd.pruned[1], 1u); }
			}
		}
	}
	goesL[i] = L; goesR[i] = R;
}
// per node: how many instances go to either child (from the inclusive scans of the flags)
__global__ void k_x_counts(const XNodeG *nodes, uint32_t n, const uint32_t *sL, const uint32_t *sR, uint32_t *splitFlag, uint32_t *c2) {
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= n) return;
	const XNodeG &nd = nodes[k];
	const uint32_t b = nd.instBegin, c = nd.instCount;
	uint32_t nL = 0, nR = 0;
	if (nd.isSplit && c) { nL = sL[b + c - 1] - (b ? sL[b - 1] : 0u); nR = sR[b + c - 1] - (b ? sR[b - 1] : 0u); }
	splitFlag[k] = nd.isSplit; c2[2 * k] = nL; c2[2 * k + 1] = nR;
}
// the children of the split nodes = the next level (left, right, in node order); leaves learn where their items go
__global__ void k_x_children(XNodeG *nodes, uint32_t n, XNodeG *next, uint32_t nextGlobal, const uint32_t *sSplit, const uint32_t *c2, const uint32_t *sC2,
                             const uint32_t *sLeafInst, uint32_t nInst, uint32_t leafBase, XTotals *totals) {
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= n) return;
	XNodeG &nd = nodes[k];
	if (nd.isSplit) {
		const uint32_t r = sSplit[k] - 1u;
		nd.child = nextGlobal + 2u * r;
		for (int side = 0; side < 2; ++side) {
			XNodeG c;
			for (int a = 0; a < 3; ++a) { c.box.mn[a] = nd.box.mn[a]; c.box.mx[a] = nd.box.mx[a]; }
			if (side == 0) c.box.mx[nd.axis] = nd.split; else c.box.mn[nd.axis] = nd.split;
			c.primCount = (side == 0 ? nd.numLeft : nd.numRight) - nd.pruned[side];
			c.instCount = c2[2 * k + side];
			c.instBegin = sC2[2 * k + side] - c.instCount;
			c.depth = nd.depth + 1u; c.badRefines = nd.badRefines;
			c.sweep = c.isSplit = c.isLeaf = 0u; c.axis = 0; c.split = 0; c.planarLeft = 0; c.numLeft = c.numRight = 0;
			c.child = 0; c.childBase[0] = c.childBase[1] = 0; c.pruned[0] = c.pruned[1] = 0; c.leafOffset = 0; c.cost = 0; c.retract = 0;
			nd.childBase[side] = c.instBegin;
			next[2u * r + side] = c;
		}
	} else {
		// a leaf: its instances are contiguous in the level's compaction of leaf instances
		nd.leafOffset = leafBase + (nd.instBegin ? sLeafInst[nd.instBegin - 1] : 0u);
	}
	if (k == n - 1) {
		totals->nSplit = sSplit[n - 1]; totals->nNextInst = sC2[2 * n - 1];
		totals->nLeafItems = nInst ? sLeafInst[nInst - 1] : 0u;
	}
}
// instances to the children (stable: ascending primitive order is kept), leaf instances to the item buffer as
// (leaf, axis-0 position, type) keys in the order leafFromEvents needs after ONE stable sort at the end
__global__ void k_x_scatter(const XInst *inst, uint32_t n, const XNodeG *nodes, uint32_t levelGlobal, const uint32_t *goesL, const uint32_t *goesR,
                            const uint32_t *scanL, const uint32_t *scanR, const uint32_t *isLeafInst, const uint32_t *scanLeaf, const float *boxL,
                            const float *boxR, XInst *next, uint32_t leafBase, unsigned long long *leafKeys, uint32_t *leafPrims) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const XInst x = inst[i];
	const XNodeG &nd = nodes[x.node];
	const uint32_t b = nd.instBegin;
	if (goesL[i]) {
		XInst o; o.prim = x.prim;
		for (int c = 0; c < 3; ++c) { o.box.mn[c] = boxL[6 * (size_t) i + c]; o.box.mx[c] = boxL[6 * (size_t) i + 3 + c]; }
		o.node = nd.child - levelGlobal;          // index inside the next level (levelGlobal = global index of its first node)
		next[nd.childBase[0] + (scanL[i] - 1u - (b ? scanL[b - 1] : 0u))] = o;
	}
	if (goesR[i]) {
		XInst o; o.prim = x.prim;
		for (int c = 0; c < 3; ++c) { o.box.mn[c] = boxR[6 * (size_t) i + c]; o.box.mx[c] = boxR[6 * (size_t) i + 3 + c]; }
		o.node = nd.child + 1u - levelGlobal;
		next[nd.childBase[1] + (scanR[i] - 1u - (b ? scanR[b - 1] : 0u))] = o;
	}
	if (isLeafInst[i]) {
		const uint32_t pos = leafBase + scanLeaf[i] - 1u;
		const uint32_t type = x.box.mn[0] == x.box.mx[0] ? (uint32_t) kPlanar : (uint32_t) kStart;
		// (global node id of the leaf) | position | type: node ids grow with the buffer position
		leafKeys[pos] = ((unsigned long long) (nd.leafOffset) << 34) | ((unsigned long long) monoKey(x.box.mn[0]) << 2) | (unsigned long long) type;
		leafPrims[pos] = x.prim;
	}
}
// cost of the subtrees and retraction (gkdtree.h:2321-2341), one level at a time from the deepest one up
__global__ void k_x_cost_up(XNodeG *all, uint32_t levelBase, uint32_t n, XParams prm) {
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= n) return;
	XNodeG &nd = all[levelBase + k];
	const float leafCost = nd.primCount * prm.queryCost;
	nd.retract = 0u;
	if (!nd.isSplit) { nd.cost = leafCost; return; }
	const float leftCost = all[nd.child].cost, rightCost = all[nd.child + 1u].cost;
	const float e0 = nd.box.mx[0] - nd.box.mn[0], e1 = nd.box.mx[1] - nd.box.mn[1], e2 = nd.box.mx[2] - nd.box.mn[2];
	const float temp = 1.0f / (e0 * e1 + e1 * e2 + e0 * e2);
	const int a = nd.axis;
	const float t0 = (a == 0 ? (e1 * e2) : a == 1 ? (e0 * e2) : (e0 * e1)) * temp;
	const float t1 = (a == 0 ? (e1 + e2) : a == 1 ? (e0 + e2) : (e0 + e1)) * temp;
	const float pl = t0 + t1 * (nd.split - nd.box.mn[a]), pr = t0 + t1 * (nd.box.mx[a] - nd.split);
	const float finalCost = prm.traversalCost + (pl * leftCost + pr * rightCost);
	if (!prm.retract || finalCost < leafCost) { nd.cost = finalCost; return; }
	nd.cost = leafCost; nd.retract = 1u;
}
__global__ void k_x_host_view(const XNodeG *all, uint32_t n, XNodeH *out) {
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k >= n) return;
	const XNodeG &nd = all[k];
	XNodeH h;
	h.primCount = nd.primCount; h.kind = nd.isSplit ? 0 : 1; h.axis = nd.axis; h.split = nd.split; h.child = nd.child;
	h.pruned = nd.pruned[0] + nd.pruned[1]; h.leafOffset = nd.leafOffset; h.leafCount = nd.isSplit ? 0u : nd.instCount; h.retract = nd.retract;
	out[k] = h;
}

// rocPRIM's two calls: the first, without storage, says how many bytes the second needs
template <class Call> void withStorage(ThrowingBuf<unsigned char> &tmp, Call call) {
	size_t bytes = 0;
	KXHIP(call(nullptr, bytes));
	tmp.reserve(bytes + 16);
	KXHIP(call((void *) tmp.p, bytes));
}
struct XScan {
	ThrowingBuf<unsigned char> tmp;
	template <class In, class Op> void scan(In in, uint32_t *out, size_t n, Op op, hipStream_t st) {
		withStorage(tmp, [&](void *t, size_t &bytes) { return rocprim::inclusive_scan(t, bytes, in, out, n, op, st); });
	}
	void sum(const uint32_t *in, uint32_t *out, size_t n, hipStream_t st) { scan(in, out, n, rocprim::plus<uint32_t>(), st); }
	// inclusive count of the events of one type, straight from the sorted keys
	void countType(const unsigned long long *keys, uint32_t type, uint32_t *out, size_t n, hipStream_t st) {
		scan(rocprim::make_transform_iterator(keys, XIsType{ type }), out, n, rocprim::plus<uint32_t>(), st);
	}
	void max(const uint32_t *in, uint32_t *out, size_t n, hipStream_t st) { scan(in, out, n, rocprim::maximum<uint32_t>(), st); }
};
// a device buffer that keeps its contents when it grows
template <typename T> void growKeep(ThrowingBuf<T> &b, size_t used, size_t need, hipStream_t st) {
	if (need <= b.cap) return;
	ThrowingBuf<T> n;
	n.reserve(std::max(need, 2 * b.cap));
	if (used) KXHIP(hipMemcpyAsync(n.p, b.p, used * sizeof(T), hipMemcpyDeviceToDevice, st));
	KXHIP(hipStreamSynchronize(st));
	b.swap(n);
}

} // namespace

// mtsgpu_cylinder_clip on the device: cylinderClippedBox (kdbuild.h) as k_x_init and k_x_classify call it, one cell per thread
namespace {
__global__ void k_x_cyl_clip(const float *cyl8, const float *own6, uint32_t n, const float *boxes, float *out, uint32_t *valid) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	Box own, to, b;
	for (int a = 0; a < 3; ++a) { own.mn[a] = own6[a]; own.mx[a] = own6[3 + a]; to.mn[a] = boxes[6 * (size_t) i + a]; to.mx[a] = boxes[6 * (size_t) i + 3 + a]; }
	valid[i] = cylinderClippedBox(cyl8, own, to, b) ? 1u : 0u;
	for (int a = 0; a < 3; ++a) { out[6 * (size_t) i + a] = b.mn[a]; out[6 * (size_t) i + 3 + a] = b.mx[a]; }
}
}
void cylinderClipDevice(const float *cyl8, const float *own6, uint32_t n, const float *boxes, float *out, uint32_t *valid) {
	requireDevice("the cylinder clip hook");
	if (!n) return;
	const Stream st("cylinder clip hook");
	ThrowingBuf<float> dIn, dBoxes, dOut;
	ThrowingBuf<uint32_t> dValid;
	dIn.reserve(kCylRow + 6); dBoxes.reserve(6 * (size_t) n); dOut.reserve(6 * (size_t) n); dValid.reserve(n);
	KXHIP(hipMemcpyAsync(dIn.p, cyl8, kCylRow * sizeof(float), hipMemcpyHostToDevice, st));
	KXHIP(hipMemcpyAsync(dIn.p + kCylRow, own6, 6 * sizeof(float), hipMemcpyHostToDevice, st));
	KXHIP(hipMemcpyAsync(dBoxes.p, boxes, 6 * (size_t) n * sizeof(float), hipMemcpyHostToDevice, st));
	hipLaunchKernelGGL(k_x_cyl_clip, dim3((n + 255u) / 256u), dim3(256), 0, st, dIn.p, dIn.p + kCylRow, n, dBoxes.p, dOut.p, dValid.p);
	KXHIP(hipGetLastError());
	KXHIP(hipMemcpyAsync(out, dOut.p, 6 * (size_t) n * sizeof(float), hipMemcpyDeviceToHost, st));
	KXHIP(hipMemcpyAsync(valid, dValid.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
	KXHIP(hipStreamSynchronize(st));
}

void kd::exactOnDevice(const Params &p, const Geometry &g, uint32_t nPrims, std::vector<std::unique_ptr<Job>> &jobs) {
	requireDevice("the device exact phase");
	if (jobs.empty()) return;
	const Stream st("device exact phase");
	const int B = 256;
	auto grid = [&](size_t n) { return dim3((unsigned) ((n + B - 1) / B)); };
	const XParams prm{ p.traversalCost, p.queryCost, p.emptySpaceBonus, p.clip ? 1 : 0, p.stopPrims, p.maxDepth, p.maxBadRefines, p.retract ? 1 : 0 };
	const bool timing = std::getenv("MTSGPU_KDTIMING") != nullptr;
	double tm[4] = { 0, 0, 0, 0 };      // setup, levels, download, replay
	auto now = []() { return std::chrono::steady_clock::now(); };
	auto since = [](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count(); };
	auto tPhase = now();
	const int nThreads = std::max(1, std::min<int>(16, (int) std::thread::hardware_concurrency()));

	// geometry: nine floats per triangle (NaN marks a non-triangle primitive, whose box is in genBox)
	ThrowingBuf<float> dTri, dGen, dCyl;      // dCyl.p stays NULL without a cylinder
	{
		std::unique_ptr<float[]> tpBuf(new float[9 * (size_t) nPrims]);
		float *tp = tpBuf.get();
		std::atomic<bool> anyGenA(false);
		runWorkers(nThreads, (size_t) nThreads, [&](size_t t, int) {      // one slice per thread
			for (uint32_t i = (uint32_t) ((uint64_t) nPrims * t / nThreads); i < (uint32_t) ((uint64_t) nPrims * (t + 1) / nThreads); ++i) {
				const uint32_t *tr = g.corners.tri + 3 * (size_t) i;
				if (tr[0] == MTSGPU_KNOTRIANGLE) { for (int q = 0; q < 9; ++q) tp[9 * (size_t) i + q] = std::numeric_limits<float>::quiet_NaN(); anyGenA = true; continue; }
				for (int v = 0; v < 3; ++v) std::memcpy(&tp[9 * (size_t) i + 3 * v], g.corners.vtx + 3 * (size_t) tr[v], 12);
			}
		});
		const bool anyGen = anyGenA;
		dTri.reserve(9 * (size_t) nPrims);
		KXHIP(hipMemcpyAsync(dTri.p, tp, 9 * (size_t) nPrims * sizeof(float), hipMemcpyHostToDevice, st));
		dGen.reserve(anyGen ? 6 * (size_t) nPrims : 6);
		if (anyGen) KXHIP(hipMemcpyAsync(dGen.p, g.genBox, 6 * (size_t) nPrims * sizeof(float), hipMemcpyHostToDevice, st));
		if (g.cyl) {
			dCyl.reserve(kCylRow * (size_t) nPrims);
			KXHIP(hipMemcpyAsync(dCyl.p, g.cyl, kCylRow * (size_t) nPrims * sizeof(float), hipMemcpyHostToDevice, st));
		}
		KXHIP(hipStreamSynchronize(st));
	}

	// ---- the roots: one per job ----
	size_t nInit = 0;
	std::vector<XNodeG> roots(jobs.size());
	for (size_t j = 0; j < jobs.size(); ++j) {
		XNodeG n; std::memset(&n, 0, sizeof(n));
		n.box = jobs[j]->nodeBox;
		n.depth = jobs[j]->depth; n.badRefines = jobs[j]->badRefines;
		n.instBegin = (uint32_t) nInit; n.instCount = (uint32_t) jobs[j]->prims.size();
		nInit += jobs[j]->prims.size();
		roots[j] = n;
	}
	if (jobs.size() > kXMaxNodes) throw std::runtime_error("kd-tree build (device exact phase): too many subtrees");
	if (nInit >= (1ull << 31)) throw std::runtime_error("kd-tree build (device exact phase): too many primitives");

	ThrowingBuf<XNodeG> dAll;                            // every node, level after level
	size_t nAll = jobs.size();
	dAll.reserve(jobs.size() + nInit + nInit / 4 + 1024);      // about 0.55 nodes per primitive in practice; grows if needed
	KXHIP(hipMemcpyAsync(dAll.p, roots.data(), roots.size() * sizeof(XNodeG), hipMemcpyHostToDevice, st));
	ThrowingBuf<XInst> dInstA, dInstB;
	ThrowingBuf<uint32_t> dU[12], dV[8];
	ThrowingBuf<unsigned long long> dKeysA, dKeysB, dNodeBest, dLeafKeys, dLeafKeys2;
	ThrowingBuf<uint32_t> dValsA, dValsB, dSegStart, dLeafPrims, dLeafPrims2;
	ThrowingBuf<float> dBoxL, dBoxR;
	ThrowingBuf<XTotals> dTotals;
	ThrowingBuf<unsigned char> dSortTmp;
	XScan scan;
	dTotals.reserve(1);
	XTotals totals{};
	auto fetchTotals = [&]() {
		KXHIP(hipGetLastError());        // a failed launch is not sticky: catch it before its outputs are trusted
		KXHIP(hipMemcpyAsync(&totals, dTotals.p, sizeof(XTotals), hipMemcpyDeviceToHost, st));
		KXHIP(hipStreamSynchronize(st));
	};

	// ---- level 0: the instances of the jobs' primitive lists, clipped to the jobs' boxes ----
	size_t nInst = 0;
	{
		std::vector<uint32_t> hp(nInit), hn(nInit);
		size_t o = 0;
		for (size_t j = 0; j < jobs.size(); ++j)
			for (uint32_t prim : jobs[j]->prims) { hp[o] = prim; hn[o] = (uint32_t) j; ++o; }
		// every buffer gets its size once, with room for the straddlers that are duplicated on the way down (a
		// reallocation inside the level loop costs a device synchronisation; it still happens if a level outgrows this)
		const size_t instCap = nInit + nInit / 4 + 1024;
		for (int k = 0; k < 6; ++k) dU[k].reserve(instCap);
		for (int k = 7; k < 12; ++k) dU[k].reserve(6 * instCap);
		dInstA.reserve(instCap); dInstB.reserve(instCap);
		dKeysA.reserve(6 * instCap); dKeysB.reserve(6 * instCap); dValsA.reserve(6 * instCap); dValsB.reserve(6 * instCap);
		dBoxL.reserve(6 * instCap); dBoxR.reserve(6 * instCap);
		for (int k = 0; k < 4; ++k) dV[k].reserve(2 * std::min<size_t>(instCap, kXMaxNodes) + 1);
		dSegStart.reserve(4 * std::min<size_t>(instCap, kXMaxNodes)); dNodeBest.reserve(std::min<size_t>(instCap, kXMaxNodes));
		KXHIP(hipMemcpyAsync(dU[0].p, hp.data(), nInit * 4, hipMemcpyHostToDevice, st));
		KXHIP(hipMemcpyAsync(dU[1].p, hn.data(), nInit * 4, hipMemcpyHostToDevice, st));
		if (nInit) {
			hipLaunchKernelGGL((dCyl.p ? k_x_init<true> : k_x_init<false>), grid(nInit), dim3(B), 0, st, dTri.p, dGen.p, dCyl.p, dU[0].p, dU[1].p, (uint32_t) nInit, dAll.p, prm.clip, dInstB.p, dU[2].p);
			scan.sum(dU[2].p, dU[3].p, nInit, st);
			hipLaunchKernelGGL(k_x_compact, grid(nInit), dim3(B), 0, st, dInstB.p, dU[2].p, dU[3].p, (uint32_t) nInit, dInstA.p);
			hipLaunchKernelGGL(k_x_roots, grid(jobs.size()), dim3(B), 0, st, dAll.p, (uint32_t) jobs.size(), dU[3].p, dTotals.p);
			fetchTotals();
			nInst = totals.nNextInst;
		} else {
			KXHIP(hipStreamSynchronize(st));
		}
	}
	tm[0] = since(tPhase); tPhase = now();

	// ---- the levels ----
	std::vector<std::pair<size_t, size_t>> levels;       // (global index of the first node, nodes)
	size_t levelBase = 0, nA = jobs.size(), leafTotal = 0;
	dLeafKeys.reserve(nInit + nInit / 4 + 1024); dLeafPrims.reserve(nInit + nInit / 4 + 1024);
	while (nA > 0) {
		if (nA > kXMaxNodes) throw std::runtime_error("kd-tree build (device exact phase): more than 2^22 nodes in one level");
		levels.emplace_back(levelBase, nA);
		XNodeG *nodes = dAll.p + levelBase;
		hipLaunchKernelGGL(k_x_prep, grid(nA), dim3(B), 0, st, nodes, (uint32_t) nA, prm);
		const size_t nEv = 6 * nInst;
		if (nEv >= (1ull << 32)) throw std::runtime_error("kd-tree build (device exact phase): more than 2^32 edge events in one level");
		if (nInst) {
			dKeysA.reserve(nEv); dKeysB.reserve(nEv); dValsA.reserve(nEv); dValsB.reserve(nEv);
			for (int k = 7; k < 12; ++k) dU[k].reserve(nEv + 1);
			dSegStart.reserve(4 * nA); dNodeBest.reserve(nA);
			hipLaunchKernelGGL(k_x_emit, grid(nInst), dim3(B), 0, st, dInstA.p, (uint32_t) nInst, nodes, dKeysA.p, dValsA.p);
			{
				// node | axis | position | type: 34 + 2 + the bits the node ids of this level need (unused slots are all ones,
				// which no event is because axis 3 does not exist: they sort last)
				unsigned endBit = 36;
				while (endBit < 58 && ((nA - 1) >> (endBit - 36))) ++endBit;
				withStorage(dSortTmp, [&](void *t, size_t &bytes) { return rocprim::radix_sort_pairs(t, bytes, dKeysA.p, dKeysB.p, dValsA.p, dValsB.p, nEv, 0u, endBit, st); });
			}
			uint32_t *hd = dU[7].p, *sE = dU[8].p, *sP = dU[9].p, *sS = dU[10].p, *sH = dU[11].p;
			KXHIP(hipMemsetAsync(dSegStart.p, 0, 4 * nA * sizeof(uint32_t), st));
			KXHIP(hipMemsetAsync(dNodeBest.p, 0xFF, nA * sizeof(unsigned long long), st));
			hipLaunchKernelGGL(k_x_flags, grid(nEv), dim3(B), 0, st, dKeysB.p, (uint32_t) nEv, hd, dSegStart.p);
			scan.countType(dKeysB.p, kEnd, sE, nEv, st); scan.countType(dKeysB.p, kPlanar, sP, nEv, st); scan.countType(dKeysB.p, kStart, sS, nEv, st);
			scan.max(hd, sH, nEv, st);
			hipLaunchKernelGGL(k_x_cost, grid(nEv), dim3(B), 0, st, dKeysB.p, dValsB.p, (uint32_t) nEv, sE, sP, sS, sH, dSegStart.p, dInstA.p, nodes, prm, dNodeBest.p);
			hipLaunchKernelGGL(k_x_decide, grid(nA), dim3(B), 0, st, nodes, (uint32_t) nA, dNodeBest.p, dKeysB.p, dValsB.p, sE, sP, sS, sH, dSegStart.p, dInstA.p, prm);
		}
		// classification, clipping, children
		for (int k = 0; k < 6; ++k) dU[k].reserve(nInst + 1);
		for (int k = 0; k < 4; ++k) dV[k].reserve(2 * nA + 1);
		dBoxL.reserve(6 * nInst + 6); dBoxR.reserve(6 * nInst + 6);
		uint32_t *gL = dU[0].p, *gR = dU[1].p, *lf = dU[2].p, *sL = dU[3].p, *sR = dU[4].p, *sLf = dU[5].p;
		uint32_t *splitFlag = dV[0].p, *sSplit = dV[1].p, *c2 = dV[2].p, *sC2 = dV[3].p;
		if (nInst) {
			hipLaunchKernelGGL((dCyl.p ? k_x_classify<true> : k_x_classify<false>), grid(nInst), dim3(B), 0, st, dInstA.p, (uint32_t) nInst, nodes, dTri.p, dGen.p, dCyl.p, prm.clip, gL, gR, lf, dBoxL.p, dBoxR.p);
			scan.sum(gL, sL, nInst, st); scan.sum(gR, sR, nInst, st); scan.sum(lf, sLf, nInst, st);
		}
		hipLaunchKernelGGL(k_x_counts, grid(nA), dim3(B), 0, st, nodes, (uint32_t) nA, sL, sR, splitFlag, c2);
		scan.sum(splitFlag, sSplit, nA, st); scan.sum(c2, sC2, 2 * nA, st);
		// room for the next level's nodes (at most two per node)
		if (nAll + 2 * nA > dAll.cap) { growKeep(dAll, nAll, nAll + 2 * nA, st); nodes = dAll.p + levelBase; }
		hipLaunchKernelGGL(k_x_children, grid(nA), dim3(B), 0, st, nodes, (uint32_t) nA, dAll.p + nAll, (uint32_t) nAll, sSplit, c2, sC2, sLf, (uint32_t) nInst,
		                   (uint32_t) leafTotal, dTotals.p);
		fetchTotals();
		const size_t nNext = totals.nNextInst, nLeafItems = totals.nLeafItems;
		if (leafTotal + nLeafItems >= (1ull << 30)) throw std::runtime_error("kd-tree build (device exact phase): too many leaf entries");
		if (nInst) {
			dInstB.reserve(nNext + 1);
			growKeep(dLeafKeys, leafTotal, leafTotal + nLeafItems + 1, st); growKeep(dLeafPrims, leafTotal, leafTotal + nLeafItems + 1, st);
			hipLaunchKernelGGL(k_x_scatter, grid(nInst), dim3(B), 0, st, dInstA.p, (uint32_t) nInst, nodes, (uint32_t) nAll, gL, gR, sL, sR, lf, sLf,
			                   dBoxL.p, dBoxR.p, dInstB.p, (uint32_t) leafTotal, dLeafKeys.p, dLeafPrims.p);
		}
		dInstA.swap(dInstB);
		leafTotal += nLeafItems;
		nInst = nNext;
		levelBase = nAll;
		nA = 2 * (size_t) totals.nSplit;
		nAll += nA;
	}
	tm[1] = since(tPhase); tPhase = now();

	// ---- leaf order, subtree costs, download ----
	// leafFromEvents lists the axis-0 start / planar events in EventLess order: one stable sort of all leaf items by
	// (leaf, position, type); equal keys keep the ascending primitive order of the instances
	std::vector<uint32_t> leafStore(leafTotal);
	if (leafTotal) {
		dLeafKeys2.reserve(leafTotal); dLeafPrims2.reserve(leafTotal);
		withStorage(dSortTmp, [&](void *t, size_t &bytes) { return rocprim::radix_sort_pairs(t, bytes, dLeafKeys.p, dLeafKeys2.p, dLeafPrims.p, dLeafPrims2.p, leafTotal, 0u, 64u, st); });
		KXHIP(hipMemcpyAsync(leafStore.data(), dLeafPrims2.p, leafTotal * 4, hipMemcpyDeviceToHost, st));
	}
	for (size_t l = levels.size(); l-- > 0;)
		hipLaunchKernelGGL(k_x_cost_up, grid(levels[l].second), dim3(B), 0, st, dAll.p, (uint32_t) levels[l].first, (uint32_t) levels[l].second, prm);
	ThrowingBuf<XNodeH> dView;
	dView.reserve(nAll);
	hipLaunchKernelGGL(k_x_host_view, grid(nAll), dim3(B), 0, st, dAll.p, (uint32_t) nAll, dView.p);
	std::vector<XNodeH> all(nAll);
	KXHIP(hipGetLastError());
	KXHIP(hipMemcpyAsync(all.data(), dView.p, nAll * sizeof(XNodeH), hipMemcpyDeviceToHost, st));
	KXHIP(hipStreamSynchronize(st));
	// what the replay indexes with: child ids inside the node table, leaf ranges inside the leaf store
	for (size_t i = 0; i < nAll; ++i) {
		const XNodeH &n = all[i];
		if (n.kind == 1 ? (n.primCount > 0 && (n.leafCount != n.primCount || (size_t) n.leafOffset + n.leafCount > leafTotal))
		                : ((size_t) n.child + 1 >= nAll || (size_t) n.child <= i))
			throw std::runtime_error("kd-tree build (device exact phase): inconsistent node table read back from the device");
	}
	tm[2] = since(tPhase); tPhase = now();

	// ---- replay: the bookkeeping of buildTree per job, depth first (nodes, indices, counters, retraction) ----
	auto emit = [&](auto &self, Context &c, uint32_t id, uint32_t node) -> void {      // self: the lambda, for the recursion
		const XNodeH &n = all[id];
		if (n.kind == 1) return c.leafFromIndices(node, leafStore.data() + n.leafOffset, n.primCount);
		c.pruned += n.pruned;
		const Context::Mark mark = c.openInner(node, n.axis, n.split);
		self(self, c, n.child, mark.children);
		self(self, c, n.child + 1u, mark.children + 1);
		if (n.retract) c.retract(node, mark);
	};
	runWorkers(nThreads, jobs.size(), [&](size_t j, int) {
		Job &job = *jobs[j];
		job.root = job.ctx.allocNodes(1);
		emit(emit, job.ctx, (uint32_t) j, job.root);
		std::vector<uint32_t>().swap(job.prims);
	});
	tm[3] = since(tPhase);
	if (timing)
		std::fprintf(stderr, "[kdbuild] device exact phase: %zu levels, %zu nodes, %zu leaf entries; setup %.1f, levels %.1f, leaf sort + costs + download %.1f, replay %.1f ms\n",
		             levels.size(), nAll, leafTotal, tm[0], tm[1], tm[2], tm[3]);
}

} // namespace mg
