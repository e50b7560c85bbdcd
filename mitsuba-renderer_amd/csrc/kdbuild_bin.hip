// kdbuild_bin.hip -- the min-max binning phase of the kd-tree builder on the device: planOnDevice (kdbuild.h).
#include "kdbuild_dev.h"
#include <cstring>

namespace mg {
using namespace kd;
namespace {      // the kernels keep the names profiles and ISA comparisons know them by: mg::<unnamed>::k_kd_*

// ---------------------------------------------------------------------------------------------------------------
// Device binning phase.  buildTreeMinMax walks every primitive of a node twice (histogram, partition) on ONE host
// thread, and at >= 10 M triangles that serial walk is most of the build on a many-core host.  Both walks are integer /
// compare work over 24-byte boxes, so they run here level by level: all nodes of one level share three launches
// (histogram, count + child bounds, stable scatter); the 768 counters of each node come back to the host, which runs
// the reference's minimizeCost / split bookkeeping unchanged.  The result is a Plan that binned() replays, so the tree
// is the one the host loop builds, bit for bit (tests/test_gpu_parity.py::test_gpu_binning_builds_the_same_tree).
// ---------------------------------------------------------------------------------------------------------------
constexpr int kKdBlock = 256;
constexpr uint32_t kKdChunk = 2048;          // entries of one node handled by one workgroup
struct DevNode { float tmn[3], inv[3]; int32_t axis; float split; };
struct DevChunk { uint32_t start, count, node, pad; };
struct DevChunkOut { uint32_t nLeft, nRight; float lmn[3], lmx[3], rmn[3], rmx[3]; uint32_t pad[2]; };

#define KDHIP(x) hipCheck((x), "device binning")

__global__ void k_kd_iota(uint32_t *p, uint32_t n) {
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) p[i] = i;
}

// MinMaxBins::bin (gkdtree.h:2379-2403): hist[node][0..3nb) = minBins, [3nb..6nb) = maxBins
__global__ __launch_bounds__(kKdBlock) void k_kd_bin(const float *__restrict__ boxes, const uint32_t *__restrict__ cur,
		const DevChunk *__restrict__ chunks, const DevNode *__restrict__ nodes, uint32_t *__restrict__ hist, int nb) {
	extern __shared__ uint32_t s_h[];
	const DevChunk ch = chunks[blockIdx.x];
	const DevNode nd = nodes[ch.node];
	for (int i = threadIdx.x; i < 6 * nb; i += kKdBlock) s_h[i] = 0u;
	__syncthreads();
	const int64_t maxBin = nb - 1;
	for (uint32_t e = threadIdx.x; e < ch.count; e += kKdBlock) {
		const float *b = boxes + 6 * (size_t) cur[ch.start + e];
		for (int a = 0; a < 3; ++a) {
			const int64_t minIdx = binIndex((b[a] - nd.tmn[a]) * nd.inv[a]);
			const int64_t maxIdx = binIndex((b[3 + a] - nd.tmn[a]) * nd.inv[a]);
			atomicAdd(&s_h[3 * nb + a * nb + (int) max((int64_t) 0, min(maxIdx, maxBin))], 1u);
			atomicAdd(&s_h[a * nb + (int) max((int64_t) 0, min(minIdx, maxBin))], 1u);
		}
	}
	__syncthreads();
	uint32_t *out = hist + (size_t) ch.node * 6 * nb;
	for (int i = threadIdx.x; i < 6 * nb; i += kKdBlock)
		if (s_h[i]) atomicAdd(&out[i], s_h[i]);
}

// MinMaxBins::partition, first half: how many entries of the chunk go left / right, and the boxes they span
__global__ __launch_bounds__(kKdBlock) void k_kd_count(const float *__restrict__ boxes, const uint32_t *__restrict__ cur,
		const DevChunk *__restrict__ chunks, const DevNode *__restrict__ nodes, DevChunkOut *__restrict__ out) {
	__shared__ unsigned long long s_key[12];
	__shared__ uint32_t s_cnt[2];
	const DevChunk ch = chunks[blockIdx.x];
	const DevNode nd = nodes[ch.node];
	if (threadIdx.x < 12) s_key[threadIdx.x] = (threadIdx.x % 6 < 3) ? ~0ull : 0ull;     // mins start high, maxes low
	if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0u;
	__syncthreads();
	unsigned long long key[12];
	for (int k = 0; k < 12; ++k) key[k] = (k % 6 < 3) ? ~0ull : 0ull;
	uint32_t nL = 0, nR = 0;
	for (uint32_t e = threadIdx.x; e < ch.count; e += kKdBlock) {
		const float *b = boxes + 6 * (size_t) cur[ch.start + e];
		const bool leftOnly = b[3 + nd.axis] <= nd.split;
		const bool goesLeft = leftOnly || !(b[nd.axis] > nd.split), goesRight = !leftOnly;
		nL += goesLeft; nR += goesRight;
		for (int k = 0; k < 6; ++k) {
			const unsigned long long hi = (unsigned long long) monoKey(b[k]) << 32;
			const unsigned long long kmin = hi | e, kmax = hi | (0xFFFFFFFFu - e);
			if (k < 3) {
				if (goesLeft && kmin < key[k]) key[k] = kmin;
				if (goesRight && kmin < key[6 + k]) key[6 + k] = kmin;
			} else {
				if (goesLeft && kmax > key[k]) key[k] = kmax;
				if (goesRight && kmax > key[6 + k]) key[6 + k] = kmax;
			}
		}
	}
	for (int k = 0; k < 12; ++k) {
		if (k % 6 < 3) atomicMin(&s_key[k], key[k]); else atomicMax(&s_key[k], key[k]);
	}
	atomicAdd(&s_cnt[0], nL); atomicAdd(&s_cnt[1], nR);
	__syncthreads();
	DevChunkOut &o = out[blockIdx.x];
	if (threadIdx.x < 12) {
		const int k = threadIdx.x, comp = k % 6;
		const unsigned long long kk = s_key[k];
		const bool empty = (comp < 3) ? (kk == ~0ull) : (kk == 0ull);
		float v = (comp < 3) ? INFINITY : -INFINITY;             // Box::reset()
		if (!empty) {
			const uint32_t e = (comp < 3) ? (uint32_t) kk : 0xFFFFFFFFu - (uint32_t) kk;
			v = boxes[6 * (size_t) cur[ch.start + e] + comp];
		}
		float *dst = (k < 6) ? (comp < 3 ? o.lmn : o.lmx) : (comp < 3 ? o.rmn : o.rmx);
		dst[comp % 3] = v;
	}
	if (threadIdx.x == 0) { o.nLeft = s_cnt[0]; o.nRight = s_cnt[1]; }
}

// MinMaxBins::partition, second half: stable scatter (the lists keep the parent's order, as push_back gives it)
__global__ __launch_bounds__(kKdBlock) void k_kd_scatter(const float *__restrict__ boxes, const uint32_t *__restrict__ cur,
		const DevChunk *__restrict__ chunks, const DevNode *__restrict__ nodes, const uint2 *__restrict__ dst, uint32_t *__restrict__ next) {
	__shared__ uint32_t s_w[2][kKdBlock / 64];
	const DevChunk ch = chunks[blockIdx.x];
	const DevNode nd = nodes[ch.node];
	uint32_t baseL = dst[blockIdx.x].x, baseR = dst[blockIdx.x].y;
	const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
	for (uint32_t r = 0; r < ch.count; r += kKdBlock) {
		const uint32_t e = r + threadIdx.x;
		bool goesLeft = false, goesRight = false;
		uint32_t p = 0;
		if (e < ch.count) {
			p = cur[ch.start + e];
			const float *b = boxes + 6 * (size_t) p;
			const bool leftOnly = b[3 + nd.axis] <= nd.split;
			goesLeft = leftOnly || !(b[nd.axis] > nd.split); goesRight = !leftOnly;
		}
		const unsigned long long mL = __ballot(goesLeft), mR = __ballot(goesRight);
		const unsigned long long below = (1ull << lane) - 1ull;
		if (lane == 0) { s_w[0][wave] = (uint32_t) __popcll(mL); s_w[1][wave] = (uint32_t) __popcll(mR); }
		__syncthreads();
		uint32_t offL = 0, offR = 0, totL = 0, totR = 0;
		for (uint32_t w = 0; w < kKdBlock / 64; ++w) {
			if (w < wave) { offL += s_w[0][w]; offR += s_w[1][w]; }
			totL += s_w[0][w]; totR += s_w[1][w];
		}
		if (goesLeft) next[baseL + offL + (uint32_t) __popcll(mL & below)] = p;
		if (goesRight) next[baseR + offR + (uint32_t) __popcll(mR & below)] = p;
		baseL += totL; baseR += totR;
		__syncthreads();
	}
}

} // namespace

void kd::planOnDevice(const Decisions &b, const Params &p, const Geometry &g, uint32_t nPrims, const Box &scene, int nThreads, Plan &plan) {
	requireDevice("gpu_binning");
	const int nb = p.minMaxBins;
	if ((size_t) 6 * nb * sizeof(uint32_t) > 60 * 1024)
		throw std::runtime_error("kd-tree build: gpu_binning supports at most 2560 bins");
	const Stream st("device binning");

	// the boxes of all primitives, once (host threads), then resident
	std::vector<float> boxes(6 * (size_t) nPrims);
	const int nt = std::max(1, std::min(nThreads, 16));
	runWorkers(nt, (size_t) nt, [&](size_t slice, int) {      // one slice per thread
		for (uint32_t i = (uint32_t) ((uint64_t) nPrims * slice / nt); i < (uint32_t) ((uint64_t) nPrims * (slice + 1) / nt); ++i) {
			Box t; primBox(g, i, t);
			std::memcpy(&boxes[6 * (size_t) i], &t, sizeof(Box));
		}
	});
	ThrowingBuf<float> dBoxes; dBoxes.reserve(boxes.size());
	KDHIP(hipMemcpyAsync(dBoxes.p, boxes.data(), boxes.size() * sizeof(float), hipMemcpyHostToDevice, st));
	ThrowingBuf<uint32_t> dCur, dNext, dHist;
	dCur.reserve((size_t) nPrims + nPrims / 4 + 1024);
	k_kd_iota<<<(nPrims + 255) / 256, 256, 0, st>>>(dCur.p, nPrims);
	ThrowingBuf<DevNode> dNodes; ThrowingBuf<DevChunk> dChunks; ThrowingBuf<DevChunkOut> dOut; ThrowingBuf<uint2> dDst;

	struct Active { int plan; uint32_t off, count, depth, badRefines; Box tight; };
	std::vector<Active> level, nextLevel;
	plan.nodes.clear();
	plan.nodes.emplace_back();
	plan.nodes[0].count = nPrims;
	auto readBack = [&](int pn, const uint32_t *src, uint32_t off, uint32_t count) {
		plan.nodes[pn].prims.resize(count);
		if (count) KDHIP(hipMemcpyAsync(plan.nodes[pn].prims.data(), src + off, (size_t) count * 4, hipMemcpyDeviceToHost, st));
	};
	if (b.early(nPrims, 1) == Decisions::kBin) level.push_back(Active{ 0, 0, nPrims, 1, 0, scene });
	else readBack(0, dCur.p, 0, nPrims);

	std::vector<DevNode> hNodes; std::vector<DevChunk> hChunks; std::vector<uint32_t> hHist;
	std::vector<DevChunkOut> hOut; std::vector<uint2> hDst;
	auto upload = [&](auto &dev, const auto &host) { dev.reserve(host.size()); KDHIP(hipMemcpyAsync(dev.p, host.data(), host.size() * sizeof(host[0]), hipMemcpyHostToDevice, st)); };
	auto makeChunks = [&](const std::vector<uint32_t> &which) {
		hChunks.clear();
		for (uint32_t k : which)
			for (uint32_t o = 0; o < level[k].count; o += kKdChunk)
				hChunks.push_back(DevChunk{ level[k].off + o, std::min(kKdChunk, level[k].count - o), k, 0 });
		upload(dChunks, hChunks);
	};

	while (!level.empty()) {
		const uint32_t nAct = (uint32_t) level.size();
		// 1. histograms of every node of the level
		hNodes.assign(nAct, DevNode());
		std::vector<float> binSize(3 * (size_t) nAct), invBinSize(3 * (size_t) nAct);
		std::vector<uint32_t> all(nAct);
		for (uint32_t k = 0; k < nAct; ++k) {
			all[k] = k;
			b.binSetup(level[k].tight, &binSize[3 * k], &invBinSize[3 * k]);
			for (int a = 0; a < 3; ++a) { hNodes[k].tmn[a] = level[k].tight.mn[a]; hNodes[k].inv[a] = invBinSize[3 * k + a]; }
		}
		makeChunks(all);
		upload(dNodes, hNodes);
		dHist.reserve((size_t) nAct * 6 * nb);
		KDHIP(hipMemsetAsync(dHist.p, 0, (size_t) nAct * 6 * nb * 4, st));
		k_kd_bin<<<(uint32_t) hChunks.size(), kKdBlock, 6 * nb * sizeof(uint32_t), st>>>(dBoxes.p, dCur.p, dChunks.p, dNodes.p, dHist.p, nb);
		KDHIP(hipGetLastError());
		hHist.resize((size_t) nAct * 6 * nb);
		KDHIP(hipMemcpyAsync(hHist.data(), dHist.p, hHist.size() * 4, hipMemcpyDeviceToHost, st));
		KDHIP(hipStreamSynchronize(st));

		// 2. minimizeCost per node (host, 3 x 127 candidates each); nodes that stop here hand their list back
		std::vector<uint32_t> splitting;
		size_t nextSize = 0;
		std::vector<uint32_t> childOff(2 * (size_t) nAct, 0u);
		for (uint32_t k = 0; k < nAct; ++k) {
			Active &a = level[k];
			const uint32_t *h = &hHist[(size_t) k * 6 * nb];
			PlanNode &pn = plan.nodes[a.plan];
			pn.best = b.minimize(a.tight, &binSize[3 * k], &invBinSize[3 * k], h, h + 3 * nb, a.count);
			if (b.afterMinimize(pn.best, a.count, a.badRefines) != 0) {
				readBack(a.plan, dCur.p, a.off, a.count);
				continue;
			}
			hNodes[k].axis = pn.best.axis; hNodes[k].split = pn.best.pos;
			childOff[2 * k] = (uint32_t) nextSize; childOff[2 * k + 1] = (uint32_t) nextSize + pn.best.numLeft;
			nextSize += (size_t) pn.best.numLeft + pn.best.numRight;
			if (nextSize > 0xFFFFFFFFull) throw std::runtime_error("kd-tree build: a level of the binning phase exceeds 2^32 entries");
			splitting.push_back(k);
		}
		if (splitting.empty()) { KDHIP(hipStreamSynchronize(st)); break; }

		// 3. count + child bounds per chunk, offsets by a host scan over the chunks, stable scatter
		makeChunks(splitting);
		upload(dNodes, hNodes);
		dOut.reserve(hChunks.size());
		k_kd_count<<<(uint32_t) hChunks.size(), kKdBlock, 0, st>>>(dBoxes.p, dCur.p, dChunks.p, dNodes.p, dOut.p);
		KDHIP(hipGetLastError());
		hOut.resize(hChunks.size());
		KDHIP(hipMemcpyAsync(hOut.data(), dOut.p, hOut.size() * sizeof(DevChunkOut), hipMemcpyDeviceToHost, st));
		KDHIP(hipStreamSynchronize(st));
		hDst.resize(hChunks.size());
		std::vector<uint32_t> gotL(nAct, 0u), gotR(nAct, 0u);
		for (uint32_t k : splitting) { PlanNode &pn = plan.nodes[level[k].plan]; pn.leftRaw.reset(); pn.rightRaw.reset(); }
		for (size_t cidx = 0; cidx < hChunks.size(); ++cidx) {
			const uint32_t k = hChunks[cidx].node;
			PlanNode &pn = plan.nodes[level[k].plan];
			const DevChunkOut &o = hOut[cidx];
			hDst[cidx] = make_uint2(childOff[2 * k] + gotL[k], childOff[2 * k + 1] + gotR[k]);
			gotL[k] += o.nLeft; gotR[k] += o.nRight;
			// the chunks of a node arrive in list order, so this is the sequential expand() chain of the host loop
			Box l, r;
			std::memcpy(l.mn, o.lmn, 12); std::memcpy(l.mx, o.lmx, 12); std::memcpy(r.mn, o.rmn, 12); std::memcpy(r.mx, o.rmx, 12);
			pn.leftRaw.expand(l); pn.rightRaw.expand(r);
		}
		for (uint32_t k : splitting) {
			const PlanNode &pn = plan.nodes[level[k].plan];
			if (gotL[k] != pn.best.numLeft || gotR[k] != pn.best.numRight)
				throw std::runtime_error("kd-tree build: min-max binning and partition disagree");
		}
		upload(dDst, hDst);
		dNext.reserve(nextSize + 1024);
		k_kd_scatter<<<(uint32_t) hChunks.size(), kKdBlock, 0, st>>>(dBoxes.p, dCur.p, dChunks.p, dNodes.p, dDst.p, dNext.p);
		KDHIP(hipGetLastError());

		// 4. children: tight boxes as the host loop computes them; those that leave the phase read their list back
		nextLevel.clear();
		for (uint32_t k : splitting) {
			const Active a = level[k];
			Split best = plan.nodes[a.plan].best;
			Box lb = plan.nodes[a.plan].leftRaw, rb = plan.nodes[a.plan].rightRaw;
			b.finishSplit(a.tight, best, lb, rb, best.numLeft, best.numRight);
			const uint32_t counts[2] = { best.numLeft, best.numRight };
			const Box *boxes2[2] = { &lb, &rb };
			for (int side = 0; side < 2; ++side) {
				const int child = (int) plan.nodes.size();
				plan.nodes.emplace_back();
				plan.nodes[child].count = counts[side];
				plan.nodes[a.plan].child[side] = child;
				if (b.early(counts[side], a.depth + 1) == Decisions::kBin)
					nextLevel.push_back(Active{ child, childOff[2 * k + side], counts[side], a.depth + 1, a.badRefines, *boxes2[side] });
				else
					readBack(child, dNext.p, childOff[2 * k + side], counts[side]);
			}
		}
		KDHIP(hipStreamSynchronize(st));              // read-backs done before the buffers swap roles
		dCur.swap(dNext);
		level.swap(nextLevel);
	}
	KDHIP(hipStreamSynchronize(st));
}

} // namespace mg
