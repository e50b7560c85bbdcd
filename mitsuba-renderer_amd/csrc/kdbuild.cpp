// kdbuild.cpp -- host-side SAH kd-tree construction for libmtsgpu.
//
// Needed because the standalone driver / bench run where no Mitsuba exists
// (inside Mitsuba the plugin flattens the tree Scene::initialize already built).
// Same cost model and rules as the reference builder
// (include/mitsuba/render/gkdtree.h:913-1214, :1735-1867, :1898-2345, :2350-2608;
// SAH include/mitsuba/render/sahkdtree3.h:35-79; clipping src/libcore/triangle.cpp:59-158):
//   > exactPrimThreshold primitives : 128-bin min-max binning, tight child boxes
//   <= exactPrimThreshold           : exact O(n log n) sweep over sorted edge events with
//                                     perfect splits (re-clipping), empty-space bonus,
//                                     "bad refines" and retraction of subtrees that did not pay off
// Subtrees below the binning phase are independent jobs and are built by a pool
// of host threads (the reference hands them to its TreeBuilder threads, :1668-1704;
// like there, such a subtree reports cost -inf so it is never retracted from above).
// Edge events that compare equal are additionally ordered by primitive index so that
// the result does not depend on the sort implementation.
// Plain C++, no HIP construct and no host.h: g++ or clang++ -std=c++17 compile it, which is how
// tools/kdbuild_host_check.cpp puts it under the host sanitizers.  The device phases: kdbuild_bin.hip, kdbuild_exact.hip.
#include "kdbuild.h"
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <mutex>
#include <thread>

namespace mg {

bool clippedTriangleBox(const float *p0, const float *p1, const float *p2, const float *bmin, const float *bmax, float *omin, float *omax) {
	return kd::clippedTriangleBoxHD(p0, p1, p2, bmin, bmax, omin, omax);
}

namespace kd {

namespace {
struct Event { float pos; uint32_t index; uint16_t type, axis; };
struct EventLess {
	bool operator()(const Event &a, const Event &b) const {
		if (a.axis != b.axis) return a.axis < b.axis;
		if (a.pos != b.pos) return a.pos < b.pos;
		if (a.type != b.type) return a.type < b.type;
		return a.index < b.index;
	}
};
} // namespace

void runWorkers(int nThreads, size_t nItems, const std::function<void(size_t, int)> &fn) {
	std::atomic<size_t> next(0);
	std::exception_ptr firstError;
	std::mutex errorLock;
	auto worker = [&](int w) {
		try {
			for (size_t k; (k = next.fetch_add(1)) < nItems;)
				fn(k, w);
		} catch (...) {
			std::lock_guard<std::mutex> guard(errorLock);
			if (!firstError) firstError = std::current_exception();
			next.store(nItems);
		}
	};
	std::vector<std::thread> pool;
	for (int t = 1; t < nThreads && (size_t) t < nItems; ++t) pool.emplace_back(worker, t);
	worker(0);
	for (auto &t : pool) t.join();
	if (firstError) std::rethrow_exception(firstError);
}

void Context::leaf(uint32_t node, uint32_t start, uint32_t primCount) {
	PNode &n = nodes[node];
	n.kind = 1; n.a = start; n.b = start + primCount;
	if (primCount > 0) { nonemptyLeafCount++; primIndexCount += primCount; }
	leafCount++;
}
void Context::leafFromIndices(uint32_t node, const uint32_t *idx, uint32_t primCount) {
	const uint32_t start = (uint32_t) indices.size();
	if (primCount > 0) indices.insert(indices.end(), idx, idx + primCount);
	leaf(node, start, primCount);
}
Context::Mark Context::openInner(uint32_t node, int axis, float split) {
	const uint32_t children = allocNodes(2);
	const Mark mark{ children, (uint32_t) nodes.size(), (uint32_t) indices.size(), leafCount, nonemptyLeafCount, innerCount };
	PNode &n = nodes[node];
	n.kind = 0; n.a = (uint32_t) axis; n.b = children; n.split = split;
	innerCount++;
	return mark;
}
void Context::retract(uint32_t node, const Mark &mark) {
	nodes.resize(mark.nodePos);
	retracted++;
	leafCount = mark.leafCount; nonemptyLeafCount = mark.nonemptyLeafCount; innerCount = mark.innerCount;
	// createLeafAfterRetraction (gkdtree.h:1603-1637)
	const uint32_t start = mark.indexPos, indexCount = (uint32_t) indices.size() - start;
	std::sort(indices.begin() + start, indices.end());
	auto last = std::unique(indices.begin() + start, indices.end());
	const uint32_t nSeen = (uint32_t) (last - (indices.begin() + start));
	indices.erase(last, indices.end());
	primIndexCount = primIndexCount - indexCount + nSeen;
	PNode &n = nodes[node];
	n.kind = 1; n.a = start; n.b = start + nSeen;
	nonemptyLeafCount++;
	leafCount++;
}

// MinMaxBins::minimizeCost (gkdtree.h:2405-2510)
Split Decisions::minimize(const Box &tight, const float *binSize, const float *invBinSize, const uint32_t *minBins, const uint32_t *maxBins, uint32_t primCount) const {
	Split cand;
	int binIdx = 0, leftBin = 0;
	const int nb = m_p.minMaxBins;
	const SAH tch(tight);
	for (int axis = 0; axis < 3; ++axis) {
		uint32_t numLeft = 0, numRight = primCount;
		float leftWidth = 0, rightWidth = tight.mx[axis] - tight.mn[axis];
		const float bs = binSize[axis];
		for (int i = 0; i < nb - 1; ++i) {
			numLeft += minBins[binIdx];
			numRight -= maxBins[binIdx];
			leftWidth += bs;
			rightWidth -= bs;
			float pl, pr;
			tch(axis, leftWidth, rightWidth, pl, pr);
			const float cost = m_p.traversalCost + m_p.queryCost * (pl * (float) numLeft + pr * (float) numRight);
			if (cost < cand.cost) { cand.cost = cost; cand.axis = axis; cand.numLeft = numLeft; cand.numRight = numRight; leftBin = i; }
			binIdx++;
		}
		binIdx++;
	}
	const int axis = cand.axis;
	const float mn = tight.mn[axis], invBS = invBinSize[axis];
	const float fmax = std::numeric_limits<float>::max();
	float split = mn + (leftBin + 1) * binSize[axis];
	float splitNext = nextafterf(split, fmax);
	int idx = (int) ((split - mn) * invBS), idxNext = (int) ((splitNext - mn) * invBS);
	if (!(idx == leftBin && idxNext == leftBin + 1)) {
		float left = tight.mn[axis], right = tight.mx[axis];
		int it = 0;
		while (true) {
			split = left + (right - left) / 2;
			splitNext = nextafterf(split, fmax);
			idx = (int) ((split - mn) * invBS);
			idxNext = (int) ((splitNext - mn) * invBS);
			if (idx == leftBin && idxNext == leftBin + 1)
				break;
			if (std::abs(idx - idxNext) > 1 || ++it > 50) { cand.cost = kInf; break; }
			if (idx <= leftBin) left = split; else right = split;
		}
	}
	if (split <= tight.mn[axis] || split >= tight.mx[axis])
		cand.cost = kInf;
	cand.pos = split;
	return cand;
}

// tail of MinMaxBins::partition (gkdtree.h:2560-2596): tight child boxes, split moved onto the nearer of them
void Decisions::finishSplit(const Box &tight, Split &best, Box &leftBounds, Box &rightBounds, uint32_t numLeft, uint32_t numRight) const {
	const int axis = best.axis;
	const float splitPos = best.pos;
	leftBounds.clip(tight); rightBounds.clip(tight);
	leftBounds.mx[axis] = std::min(leftBounds.mx[axis], splitPos);
	rightBounds.mn[axis] = std::max(rightBounds.mn[axis], splitPos);
	if (leftBounds.mx[axis] != rightBounds.mn[axis]) {
		const SAH tch(tight);
		const float nL = (float) numLeft, nR = (float) numRight;
		float p1l, p1r, p2l, p2r;
		tch(axis, leftBounds.mx[axis] - tight.mn[axis], tight.mx[axis] - leftBounds.mx[axis], p1l, p1r);
		tch(axis, rightBounds.mn[axis] - tight.mn[axis], tight.mx[axis] - rightBounds.mn[axis], p2l, p2r);
		const float cost1 = m_p.traversalCost + m_p.queryCost * (p1l * nL + p1r * nR);
		const float cost2 = m_p.traversalCost + m_p.queryCost * (p2l * nL + p2r * nR);
		if (cost1 <= cost2) { best.cost = cost1; best.pos = leftBounds.mx[axis]; }
		else { best.cost = cost2; best.pos = rightBounds.mn[axis]; }
		leftBounds.mx[axis] = std::min(leftBounds.mx[axis], best.pos);
		rightBounds.mn[axis] = std::max(rightBounds.mn[axis], best.pos);
	}
}

namespace {
class Builder : public Decisions {
public:
	Builder(const Geometry &g, const Params &p, uint32_t nPrims) : Decisions{ p }, m_g(g), m_nPrims(nPrims) {}

	// SAH cost of splitting at a plane with nBelow / nAbove primitives on its sides (gkdtree.h:1974-1980: the empty-space
	// bonus applies when one side is empty)
	float planeCost(float probBelow, float probAbove, uint32_t nBelow, uint32_t nAbove) const {
		float cost = m_p.traversalCost + m_p.queryCost * (probBelow * (float) nBelow + probAbove * (float) nAbove);
		if (nBelow == 0 || nAbove == 0)
			cost *= m_p.emptySpaceBonus;
		return cost;
	}

	// The cheapest of the candidate planes strictly inside the node.  Primitives lying IN a plane go to the side that is
	// cheaper, to the right one when both cost the same (gkdtree.h:1996-2014)
	Split cheapestPlane(const std::vector<Candidate> &planes, const Box &nodeBox, uint32_t primCount) const {
		Split best;
		const SAH area(nodeBox);
		uint32_t below[3] = { 0, 0, 0 }, above[3] = { primCount, primCount, primCount };
		for (const Candidate &pl : planes) {
			const int k = pl.axis;
			const uint32_t inPlane = pl.count[kPlanar];
			above[k] -= inPlane + pl.count[kEnd];
			if (pl.pos > nodeBox.mn[k] && pl.pos < nodeBox.mx[k]) {
				float probBelow, probAbove;
				area(k, pl.pos - nodeBox.mn[k], nodeBox.mx[k] - pl.pos, probBelow, probAbove);
				Split s;
				s.pos = pl.pos; s.axis = k; s.numLeft = below[k]; s.numRight = above[k];
				s.cost = planeCost(probBelow, probAbove, below[k], above[k]);
				if (inPlane != 0) {
					const float withLeft = planeCost(probBelow, probAbove, below[k] + inPlane, above[k]);
					const float withRight = planeCost(probBelow, probAbove, below[k], above[k] + inPlane);
					s.planarLeft = withLeft < withRight;
					s.cost = s.planarLeft ? withLeft : withRight;
					(s.planarLeft ? s.numLeft : s.numRight) += inPlane;
				}
				if (s.cost < best.cost)
					best = s;
			}
			below[k] += pl.count[kStart] + inPlane;
		}
		return best;
	}

	static void pushEvents(std::vector<Event> &out, const Box &b, uint32_t index) {
		for (int axis = 0; axis < 3; ++axis) {
			const float mn = b.mn[axis], mx = b.mx[axis];
			if (mn == mx) {
				out.push_back(Event{ mn, index, kPlanar, (uint16_t) axis });
			} else {
				out.push_back(Event{ mn, index, kStart, (uint16_t) axis });
				out.push_back(Event{ mx, index, kEnd, (uint16_t) axis });
			}
		}
	}

	void leafFromEvents(Context &c, uint32_t node, const Event *es, const Event *ee, uint32_t primCount) const {
		const uint32_t start = (uint32_t) c.indices.size();
		for (const Event *e = es; primCount > 0 && e != ee && e->axis == 0; ++e)
			if (e->type == kStart || e->type == kPlanar)
				c.indices.push_back(e->index);
		c.leaf(node, start, primCount);
	}

	// The cost of an inner node from its children's; a subtree that did not pay off is retracted (gkdtree.h:2321-2341).
	// Below binned() that is only reachable when no job hangs there (their cost is -inf)
	float closeInner(Context &c, uint32_t node, const Context::Mark &mark, const Box &nodeBox, const Split &best, uint32_t primCount, float leftCost, float rightCost) const {
		float pl, pr;
		const SAH area(nodeBox);
		area(best.axis, best.pos - nodeBox.mn[best.axis], nodeBox.mx[best.axis] - best.pos, pl, pr);
		const float finalCost = m_p.traversalCost + (pl * leftCost + pr * rightCost);
		if (!m_p.retract || finalCost < primCount * m_p.queryCost)
			return finalCost;
		c.retract(node, mark);
		return primCount * m_p.queryCost;
	}

	// buildTree: exact greedy sweep (gkdtree.h:1898-2345)
	float sweep(Context &c, uint8_t *cls, uint32_t depth, uint32_t node, const Box &nodeBox,
	            std::vector<Event> &events, uint32_t primCount, uint32_t badRefines) const {
		const Event *eventStart = events.data(), *eventEnd = events.data() + events.size();
		const float leafCost = primCount * m_p.queryCost;
		if (primCount <= m_p.stopPrims || depth >= m_p.maxDepth) {
			leafFromEvents(c, node, eventStart, eventEnd, primCount);
			return leafCost;
		}
		// The greedy SAH step (gkdtree.h:1936-2021) in two passes over the sorted events, the way the device phase does it with
		// prefix sums (exactOnDevice): first every distinct (axis, position) becomes one candidate plane with the numbers of
		// primitives that end on it, lie in it and start on it; then a running count per axis turns those into the populations
		// left and right of each plane and the cheapest plane is kept -- the first one among equals, in (axis, position) order.
		const Event *axisStart[3] = { eventEnd, eventEnd, eventEnd };
		std::vector<Candidate> &planes = c.planes;
		planes.clear();
		for (const Event *ev = eventStart; ev < eventEnd; ++ev) {
			if (planes.empty() || planes.back().axis != ev->axis || planes.back().pos != ev->pos) {
				if (planes.empty() || planes.back().axis != ev->axis) axisStart[ev->axis] = ev;
				planes.push_back(Candidate{ ev->pos, (int) ev->axis, { 0, 0, 0 } });
			}
			planes.back().count[ev->type]++;
		}
		const Split best = cheapestPlane(planes, nodeBox, primCount);

		if (best.cost >= leafCost) {
			if ((best.cost > 4 * leafCost && primCount < 16) || badRefines >= m_p.maxBadRefines || best.cost == kInf) {
				leafFromEvents(c, node, eventStart, eventEnd, primCount);
				return leafCost;
			}
			++badRefines;
		}

		// classification wrt. the chosen plane (gkdtree.h:2053-2103)
		enum : uint8_t { kBoth = 0, kLeft = 1, kRight = 2, kBothDone = 3 };
		for (const Event *e = axisStart[best.axis]; e < eventEnd && e->axis == best.axis; ++e)
			cls[e->index] = kBoth;
		uint32_t primsLeft = 0, primsRight = 0, primsBoth = primCount;
		for (const Event *e = axisStart[best.axis]; e < eventEnd && e->axis == best.axis; ++e) {
			if (e->type == kEnd && e->pos <= best.pos) {
				cls[e->index] = kLeft; primsBoth--; primsLeft++;
			} else if (e->type == kStart && e->pos >= best.pos) {
				cls[e->index] = kRight; primsBoth--; primsRight++;
			} else if (e->type == kPlanar) {
				if (e->pos < best.pos || (e->pos == best.pos && best.planarLeft)) {
					cls[e->index] = kLeft; primsBoth--; primsLeft++;
				} else if (e->pos > best.pos || (e->pos == best.pos && !best.planarLeft)) {
					cls[e->index] = kRight; primsBoth--; primsRight++;
				}
			}
		}

		Box leftBox = nodeBox, rightBox = nodeBox;
		leftBox.mx[best.axis] = best.pos;
		rightBox.mn[best.axis] = best.pos;
		uint32_t prunedLeft = 0, prunedRight = 0;
		std::vector<Event> leftEvents, rightEvents;
		if (m_p.clip) {
			std::vector<Event> lt, rt, nl, nr;
			lt.reserve(6 * (size_t) primsLeft); rt.reserve(6 * (size_t) primsRight);
			nl.reserve(6 * (size_t) primsBoth); nr.reserve(6 * (size_t) primsBoth);
			for (const Event *e = eventStart; e < eventEnd; ++e) {
				const uint8_t k = cls[e->index];
				if (k == kLeft) lt.push_back(*e);
				else if (k == kRight) rt.push_back(*e);
				else if (k == kBoth) {
					Box cl, cr;
					const bool vl = primClipped(m_g, e->index, leftBox, cl), vr = primClipped(m_g, e->index, rightBox, cr);
					if (vl && cl.area() > 0) pushEvents(nl, cl, e->index); else prunedLeft++;
					if (vr && cr.area() > 0) pushEvents(nr, cr, e->index); else prunedRight++;
					cls[e->index] = kBothDone;
				}
			}
			c.pruned += prunedLeft + prunedRight;
			std::sort(nl.begin(), nl.end(), EventLess());
			std::sort(nr.begin(), nr.end(), EventLess());
			leftEvents.resize(lt.size() + nl.size());
			rightEvents.resize(rt.size() + nr.size());
			std::merge(lt.begin(), lt.end(), nl.begin(), nl.end(), leftEvents.begin(), EventLess());
			std::merge(rt.begin(), rt.end(), nr.begin(), nr.end(), rightEvents.begin(), EventLess());
		} else {
			for (const Event *e = eventStart; e < eventEnd; ++e) {
				const uint8_t k = cls[e->index];
				if (k == kLeft) leftEvents.push_back(*e);
				else if (k == kRight) rightEvents.push_back(*e);
				else if (k == kBoth) { leftEvents.push_back(*e); rightEvents.push_back(*e); }
			}
		}
		std::vector<Event>().swap(events);      // the parent's list is no longer needed

		const Context::Mark mark = c.openInner(node, best.axis, best.pos);
		const uint32_t children = mark.children;

		const float leftCost = sweep(c, cls, depth + 1, children, leftBox, leftEvents, best.numLeft - prunedLeft, badRefines);
		const float rightCost = sweep(c, cls, depth + 1, children + 1, rightBox, rightEvents, best.numRight - prunedRight, badRefines);
		return closeInner(c, node, mark, nodeBox, best, primCount, leftCost, rightCost);
	}

	// transitionToNLogN + createEventList (gkdtree.h:1668-1704, :1490-1530)
	float runExact(Context &c, uint8_t *cls, uint32_t depth, uint32_t node, const Box &nodeBox,
	               const std::vector<uint32_t> &prims, uint32_t badRefines) const {
		std::vector<Event> events;
		events.reserve(6 * prims.size());
		uint32_t actual = 0;
		for (uint32_t index : prims) {
			Box b;
			if (m_p.clip) {
				if (!primClipped(m_g, index, nodeBox, b) || b.area() == 0)
					continue;
			} else {
				primBox(m_g, index, b);
			}
			pushEvents(events, b, index);
			++actual;
		}
		std::sort(events.begin(), events.end(), EventLess());
		return sweep(c, cls, depth, node, nodeBox, events, actual, badRefines);
	}

	// buildTreeMinMax (gkdtree.h:1735-1867).  Nodes that drop to the exact method become jobs.
	// With a plan (device binning phase, planOnDevice in kdbuild_bin.hip) the histogram / partition loops are replaced by its records.
	float binned(Context &c, uint32_t depth, uint32_t node, const Box &nodeBox, const Box &tight,
	             std::vector<uint32_t> &prims, uint32_t badRefines, Plan *plan = nullptr, int planNode = -1) {
		PlanNode *pn = plan ? &plan->nodes[planNode] : nullptr;
		if (pn && pn->child[0] < 0)
			prims.swap(pn->prims);                         // terminal record: its primitive list was read back
		const uint32_t primCount = (pn && pn->child[0] >= 0) ? pn->count : (uint32_t) prims.size();
		const float leafCost = primCount * m_p.queryCost;
		switch (early(primCount, depth)) {
			case kMakeLeaf: c.leafFromIndices(node, prims.data(), primCount); return leafCost;
			case kDefer: return defer(c, depth, node, nodeBox, prims, badRefines);
			default: break;
		}

		Split best;
		Box leftBounds, rightBounds; leftBounds.reset(); rightBounds.reset();
		std::vector<uint32_t> leftPrims, rightPrims;
		if (!pn) {
			const int nb = m_p.minMaxBins;
			float binSize[3], invBinSize[3];
			binSetup(tight, binSize, invBinSize);
			std::vector<uint32_t> minBins(3 * (size_t) nb, 0u), maxBins(3 * (size_t) nb, 0u);
			const int64_t maxBin = nb - 1;
			for (uint32_t i = 0; i < primCount; ++i) {
				Box b; primBox(m_g, prims[i], b);
				for (int a = 0; a < 3; ++a) {
					const int64_t minIdx = binIndex((b.mn[a] - tight.mn[a]) * invBinSize[a]);
					const int64_t maxIdx = binIndex((b.mx[a] - tight.mn[a]) * invBinSize[a]);
					maxBins[a * nb + std::max((int64_t) 0, std::min(maxIdx, maxBin))]++;
					minBins[a * nb + std::max((int64_t) 0, std::min(minIdx, maxBin))]++;
				}
			}
			best = minimize(tight, binSize, invBinSize, minBins.data(), maxBins.data(), primCount);
		} else {
			best = pn->best;
		}
		switch (afterMinimize(best, primCount, badRefines)) {
			case 2: return defer(c, depth, node, nodeBox, prims, badRefines);
			case 1: c.leafFromIndices(node, prims.data(), primCount); return leafCost;
			default: break;
		}

		// MinMaxBins::partition (gkdtree.h:2517-2596)
		if (!pn) {
			const float splitPos = best.pos;
			const int axis = best.axis;
			leftPrims.reserve(best.numLeft); rightPrims.reserve(best.numRight);
			for (uint32_t i = 0; i < primCount; ++i) {
				const uint32_t p = prims[i];
				Box b; primBox(m_g, p, b);
				if (b.mx[axis] <= splitPos) { leftBounds.expand(b); leftPrims.push_back(p); }
				else if (b.mn[axis] > splitPos) { rightBounds.expand(b); rightPrims.push_back(p); }
				else { leftBounds.expand(b); rightBounds.expand(b); leftPrims.push_back(p); rightPrims.push_back(p); }
			}
			if (leftPrims.size() != best.numLeft || rightPrims.size() != best.numRight)
				throw std::runtime_error("kd-tree build: min-max binning and partition disagree");
			std::vector<uint32_t>().swap(prims);
		} else {
			leftBounds = pn->leftRaw; rightBounds = pn->rightRaw;
		}
		finishSplit(tight, best, leftBounds, rightBounds, best.numLeft, best.numRight);

		const Context::Mark mark = c.openInner(node, best.axis, best.pos);
		const uint32_t children = mark.children;

		Box childBox = nodeBox;
		childBox.mx[best.axis] = best.pos;
		const float leftCost = binned(c, depth + 1, children, childBox, leftBounds, leftPrims, badRefines, plan, pn ? pn->child[0] : -1);
		childBox.mn[best.axis] = best.pos;
		childBox.mx[best.axis] = nodeBox.mx[best.axis];
		const float rightCost = binned(c, depth + 1, children + 1, childBox, rightBounds, rightPrims, badRefines, plan, pn ? pn->child[1] : -1);
		return closeInner(c, node, mark, nodeBox, best, primCount, leftCost, rightCost);
	}

	// Hand a subtree to the job pool (parallel build) or build it right here (<= threshold scenes)
	float defer(Context &c, uint32_t depth, uint32_t node, const Box &nodeBox, std::vector<uint32_t> &prims, uint32_t badRefines) {
		if (!m_parallel) {
			// scratch classification per primitive id: every entry is written (kBoth) before the sweep reads it, so it
			// is left uninitialised -- zero-filling nPrims bytes per worker page-faults 2 GB at 10 M primitives
			std::unique_ptr<uint8_t[]> cls(new uint8_t[m_nPrims]);
			return runExact(c, cls.get(), depth, node, nodeBox, prims, badRefines);
		}
		m_jobs.emplace_back(new Job());
		Job &j = *m_jobs.back();
		j.depth = depth; j.nodeBox = nodeBox; j.prims.swap(prims); j.badRefines = badRefines;
		PNode &n = c.nodes[node];
		n.kind = 2; n.a = (uint32_t) m_jobs.size() - 1; n.b = 0;
		return -kInf;       // "Never tear down this subtree" (gkdtree.h:1691-1692)
	}

	void runJobs(int nThreads) {
		std::vector<std::unique_ptr<uint8_t[]>> cls((size_t) std::max(1, nThreads));      // one per worker, see defer()
		runWorkers(nThreads, m_jobs.size(), [&](size_t k, int w) {
			if (!cls[w]) cls[w].reset(new uint8_t[m_nPrims]);
			Job &j = *m_jobs[k];
			j.root = j.ctx.allocNodes(1);
			const auto tj0 = std::chrono::steady_clock::now();
			runExact(j.ctx, cls[w].get(), j.depth, j.root, j.nodeBox, j.prims, j.badRefines);
			j.ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tj0).count();
			std::vector<uint32_t>().swap(j.prims);
		});
	}

	const Geometry &m_g;
	uint32_t m_nPrims;
	bool m_parallel = false;
	std::vector<std::unique_ptr<Job>> m_jobs;
};
} // namespace

Params Params::from(const mtsgpu_kd_params *kp, uint32_t nPrims) {
	Params p;
	p.traversalCost = (kp && kp->traversal_cost > 0) ? kp->traversal_cost : 15;      // gkdtree.h:711-724
	p.queryCost = (kp && kp->query_cost > 0) ? kp->query_cost : 20;
	p.emptySpaceBonus = (kp && kp->empty_space_bonus > 0) ? kp->empty_space_bonus : 0.9f;
	p.stopPrims = (kp && kp->stop_prims > 0) ? (uint32_t) kp->stop_prims : 6;
	p.maxBadRefines = (kp && kp->max_bad_refines > 0) ? (uint32_t) kp->max_bad_refines : 3;
	p.exactPrimThreshold = (kp && kp->exact_prim_threshold > 0) ? (uint32_t) kp->exact_prim_threshold : 65536;
	p.minMaxBins = (kp && kp->min_max_bins > 1) ? kp->min_max_bins : 128;
	p.clip = !(kp && kp->clip < 0);
	p.retract = !(kp && kp->retract < 0);
	p.maxDepth = (kp && kp->max_depth > 0) ? (uint32_t) kp->max_depth : 0;
	int log2n = 0;
	for (uint32_t v = nPrims; v >>= 1;) log2n++;
	if (p.maxDepth == 0) p.maxDepth = (uint32_t) (int) (8 + 1.3f * log2n);                       // gkdtree.h:945-947
	p.maxDepth = std::min(p.maxDepth, 48u);
	return p;
}

// final layout (gkdtree.h:1042-1138): depth first, left child first, siblings adjacent
static void layOut(const Context &root, uint32_t prelimRoot, const std::vector<std::unique_ptr<Job>> &jobs, const Box &scene, KdTree &out) {
	uint32_t inner = root.innerCount, leaves = root.leafCount, nIdx = root.primIndexCount;
	for (auto &j : jobs) { inner += j->ctx.innerCount; leaves += j->ctx.leafCount; nIdx += j->ctx.primIndexCount; }
	const uint32_t nodeCount = inner + leaves;
	out.nodes.assign(2 * (size_t) nodeCount, 0u);
	out.indices.assign(nIdx, 0u);
	struct Item { const Context *ctx; uint32_t node, target; Box box; };
	std::vector<Item> stack;
	uint32_t nodePtr = 0, indexPtr = 0;
	float expTraversalSteps = 0, expLeavesVisited = 0, expPrimitivesIntersected = 0;
	stack.push_back(Item{ &root, prelimRoot, nodePtr++, scene });
	while (!stack.empty()) {
		Item it = stack.back(); stack.pop_back();
		const PNode *n = &it.ctx->nodes[it.node];
		if (n->kind == 2) {
			const Job &j = *jobs[n->a];
			it.ctx = &j.ctx; it.node = j.root;
			n = &it.ctx->nodes[it.node];
		}
		uint32_t *target = &out.nodes[2 * (size_t) it.target];
		if (n->kind == 1) {
			const uint32_t primsInLeaf = n->b - n->a;
			target[0] = 0x80000000u | indexPtr;
			target[1] = indexPtr + primsInLeaf;
			const float quantity = it.box.area();
			expLeavesVisited += quantity;
			expPrimitivesIntersected += quantity * primsInLeaf;
			for (uint32_t k = n->a; k < n->b; ++k)
				out.indices[indexPtr++] = it.ctx->indices[k];
		} else {
			expTraversalSteps += it.box.area();
			const uint32_t children = nodePtr;
			nodePtr += 2;
			const int axis = (int) n->a;
			target[0] = (uint32_t) axis | ((children - it.target) << 2);
			std::memcpy(&target[1], &n->split, 4);
			Box box = it.box;
			const float tmp = box.mn[axis];
			box.mn[axis] = n->split;
			stack.push_back(Item{ it.ctx, n->b + 1, children + 1, box });
			box.mn[axis] = tmp;
			box.mx[axis] = n->split;
			stack.push_back(Item{ it.ctx, n->b, children, box });
		}
	}
	if (nodePtr != nodeCount || indexPtr != nIdx)
		throw std::runtime_error("kd-tree build: layout pass is inconsistent");
	const float rootQuantity = scene.area();
	out.stats[0] = inner; out.stats[1] = leaves; out.stats[2] = nIdx;
	out.stats[3] = expTraversalSteps / rootQuantity;
	out.stats[4] = expLeavesVisited / rootQuantity;
	out.stats[5] = expPrimitivesIntersected / rootQuantity;

	// slightly enlarge the box (gkdtree.h:1170-1176); max uses the already-moved min
	for (int a = 0; a < 3; ++a) out.aabbMin[a] = scene.mn[a] - ((scene.mx[a] - scene.mn[a]) * kEps + kEps);
	for (int a = 0; a < 3; ++a) out.aabbMax[a] = scene.mx[a] + ((scene.mx[a] - out.aabbMin[a]) * kEps + kEps);
}

} // namespace kd

void cylinderClipHost(const float *cyl8, const float *own6, uint32_t n, const float *boxes, float *out, uint32_t *valid) {
	using namespace kd;
	Box own;
	for (int a = 0; a < 3; ++a) { own.mn[a] = own6[a]; own.mx[a] = own6[3 + a]; }
	for (uint32_t i = 0; i < n; ++i) {
		Box to, b;
		for (int a = 0; a < 3; ++a) { to.mn[a] = boxes[6 * (size_t) i + a]; to.mx[a] = boxes[6 * (size_t) i + 3 + a]; }
		valid[i] = cylinderClippedBox(cyl8, own, to, b) ? 1u : 0u;
		for (int a = 0; a < 3; ++a) { out[6 * (size_t) i + a] = b.mn[a]; out[6 * (size_t) i + 3 + a] = b.mx[a]; }
	}
}

void buildKdTree(const float *vtx, const uint32_t *tri, uint32_t nTris, const float *genBox, const mtsgpu_kd_params *kp, KdTree &out,
                 const float *cylTable) {
	using namespace kd;
	const Params p = Params::from(kp, nTris);
	const int nThreads = (kp && kp->n_threads > 0) ? kp->n_threads : (int) std::thread::hardware_concurrency();
	out = KdTree();
	if (nTris == 0) { out.nodes = { 0x80000000u, 0u }; return; }
	const Geometry g{ { vtx, tri }, genBox, cylTable };
	Builder b(g, p, nTris);
	// gpu_binning is a bit set: 1 = min-max binning phase on the device, 2 = exact phase on the device
	const bool exactOnDev = kp && (kp->gpu_binning & 2) != 0;
	b.m_parallel = nTris > p.exactPrimThreshold || exactOnDev;      // the device builds the exact subtrees as jobs
	Box scene; scene.reset();
	std::vector<uint32_t> prims(nTris);
	for (uint32_t i = 0; i < nTris; ++i) { Box t; primBox(g, i, t); scene.expand(t); prims[i] = i; }

	Context root;
	const uint32_t prelimRoot = root.allocNodes(1);
	const bool timing = std::getenv("MTSGPU_KDTIMING") != nullptr;
	const auto t0 = std::chrono::steady_clock::now();
	const bool onDevice = kp && (kp->gpu_binning & 1) != 0 && nTris > p.exactPrimThreshold;
	if (onDevice) {
		Plan plan;
		std::vector<uint32_t>().swap(prims);
		planOnDevice(b, p, g, nTris, scene, nThreads, plan);
		b.binned(root, 1, prelimRoot, scene, scene, prims, 0, &plan, 0);
	} else {
		b.binned(root, 1, prelimRoot, scene, scene, prims, 0);
	}
	const auto t1 = std::chrono::steady_clock::now();
	if (exactOnDev) exactOnDevice(p, g, nTris, b.m_jobs);
	else b.runJobs(nThreads);
	const auto t2 = std::chrono::steady_clock::now();
	if (timing) {
		double mx = 0, sum = 0;
		for (auto &j : b.m_jobs) { mx = std::max(mx, j->ms); sum += j->ms; }
		std::fprintf(stderr, "[kdbuild] jobs: longest %.1f ms, mean %.1f ms\n", mx, b.m_jobs.empty() ? 0.0 : sum / b.m_jobs.size());
		std::fprintf(stderr, "[kdbuild] %u prims: binning phase (%s) %.1f ms (%zu jobs), exact phase %.1f ms on %d threads\n", nTris, onDevice ? "device" : "host",
		             std::chrono::duration<double, std::milli>(t1 - t0).count(), b.m_jobs.size(),
		             std::chrono::duration<double, std::milli>(t2 - t1).count(), nThreads);
	}
	layOut(root, prelimRoot, b.m_jobs, scene, out);
}

} // namespace mg
