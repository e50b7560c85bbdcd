// kdbuild_host_check.cpp -- the host kd-tree builder on its own, under the host sanitizers.  csrc/kdbuild.cpp is plain
// C++, so this program links it with two throwing stubs for the device phases and needs neither hipcc nor a GPU:
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fno-fast-math -fsanitize=address,undefined -pthread \
//       -I mitsuba-renderer_amd/csrc tools/kdbuild_host_check.cpp mitsuba-renderer_amd/csrc/kdbuild.cpp -o kdbuild_host_check
//   ./kdbuild_host_check
//
// Deterministic triangle soups of 14, 2 000 and 40 000 triangles, each built with four parameter variants on 1 and on 5
// threads.  Prints node count, index count and an FNV-1a hash of nodes and indices per build: the lines are the record to
// compare a changed builder against (LABNOTES.md), a sanitizer report or a hash that depends on the thread count is a bug.
// Not a test of the suite and never loaded into Python; it runs on the CPU only.
#include "kdbuild.h"
#include <cstdio>

namespace mg {
namespace kd {
void planOnDevice(const Decisions &, const Params &, const Geometry &, uint32_t, const Box &, int, Plan &) {
	throw std::runtime_error("kdbuild_host_check: the device binning phase is not linked");
}
void exactOnDevice(const Params &, const Geometry &, uint32_t, std::vector<std::unique_ptr<Job>> &) {
	throw std::runtime_error("kdbuild_host_check: the device exact phase is not linked");
}
} // namespace kd
} // namespace mg

namespace {

uint32_t g_lcg = 1;
float uniform() {
	g_lcg = g_lcg * 1664525u + 1013904223u;
	return (float) (g_lcg >> 8) * (1.0f / 16777216.0f);
}

// n triangles in the unit cube; every seventh lies flat in a plane x = const, corners shared with nobody
void soup(uint32_t n, std::vector<float> &vtx, std::vector<uint32_t> &tri) {
	g_lcg = 12345u + n;
	const float size = 1.5f / std::cbrt((float) n);
	vtx.resize(9 * (size_t) n); tri.resize(3 * (size_t) n);
	for (uint32_t t = 0; t < n; ++t) {
		const float c[3] = { uniform(), uniform(), uniform() };
		for (int v = 0; v < 3; ++v)
			for (int a = 0; a < 3; ++a)
				vtx[9 * (size_t) t + 3 * v + a] = (a == 0 && t % 7 == 3) ? c[0] : c[a] + size * (uniform() - 0.5f);
		for (int v = 0; v < 3; ++v) tri[3 * (size_t) t + v] = 3 * t + v;
	}
}

uint64_t fnv(uint64_t h, const std::vector<uint32_t> &words) {
	for (uint32_t w : words)
		for (int b = 0; b < 4; ++b) { h ^= (w >> (8 * b)) & 0xFFu; h *= 0x100000001B3ull; }
	return h;
}

} // namespace

int main() {
	struct Variant { const char *name; int threshold, stopPrims, clip, retract; };
	const Variant variants[4] = { { "threshold 4, stop 1", 4, 1, 0, 0 }, { "threshold 300", 300, 0, 0, 0 },
	                              { "threshold 300, no clip", 300, 0, -1, 0 }, { "threshold 300, no retract", 300, 0, 0, -1 } };
	int failed = 0;
	for (uint32_t n : { 14u, 2000u, 40000u }) {
		std::vector<float> vtx; std::vector<uint32_t> tri;
		soup(n, vtx, tri);
		for (const Variant &v : variants) {
			uint64_t first = 0;
			for (int threads : { 1, 5 }) {
				mtsgpu_kd_params kp = {};
				kp.exact_prim_threshold = v.threshold; kp.stop_prims = v.stopPrims; kp.clip = v.clip; kp.retract = v.retract;
				kp.n_threads = threads;
				mg::KdTree kd;
				mg::buildKdTree(vtx.data(), tri.data(), n, nullptr, &kp, kd);
				const uint64_t h = fnv(fnv(0xCBF29CE484222325ull, kd.nodes), kd.indices);
				std::printf("%5u triangles, %-25s %d thread%s: %7zu nodes, %8zu indices, fnv %016llx\n", n, v.name, threads,
				            threads == 1 ? " " : "s", kd.nodes.size() / 2, kd.indices.size(), (unsigned long long) h);
				if (threads == 1) first = h;
				else if (h != first) { std::printf("  the tree depends on the thread count\n"); failed = 1; }
			}
		}
	}
	return failed;
}
