// kdbuild_dev.h -- the HIP plumbing the two device phases of the kd-tree builder share.  All of it throws
// std::runtime_error (mtsgpu_flatten makes that an error code); ctx.h's DevBuf returns a context error code instead.
#pragma once
#include "kdbuild.h"
#include <hip/hip_runtime.h>

namespace mg {
namespace kd {

inline void hipCheck(hipError_t e, const char *phase) {
	if (e != hipSuccess) throw std::runtime_error(std::string("kd-tree build (") + phase + "): " + hipGetErrorString(e));
}
inline void requireDevice(const char *what) {
	int ndev = 0;
	if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
		throw std::runtime_error(std::string("kd-tree build: ") + what + " was requested but there is no HIP device");
}
struct Stream {
	hipStream_t s;
	explicit Stream(const char *phase) { hipCheck(hipStreamCreate(&s), phase); }
	~Stream() { (void) hipStreamDestroy(s); }
	operator hipStream_t() const { return s; }
	Stream(const Stream &) = delete;
};
// Device memory; reserve() keeps no contents.  A failed allocation names the binning phase whichever phase asked, as ever.
template <typename T> struct ThrowingBuf {
	T *p = nullptr; size_t cap = 0;
	ThrowingBuf() = default; ThrowingBuf(const ThrowingBuf &) = delete;
	~ThrowingBuf() { if (p) (void) hipFree(p); }
	void reserve(size_t n) {
		if (n <= cap) return;
		if (p) { (void) hipFree(p); p = nullptr; cap = 0; }
		hipCheck(hipMalloc((void **) &p, n * sizeof(T)), "device binning");
		cap = n;
	}
	void swap(ThrowingBuf &o) { std::swap(p, o.p); std::swap(cap, o.cap); }
};
// An integer key in the order of the floats, -0 and +0 being one (they compare equal in EventLess).  Reducing bounds with it
// in any order returns what the sequential std::min / std::max chain does: ties go to the earliest entry, whose bits are read back
__device__ inline uint32_t monoKey(float v) {
	const uint32_t u = __float_as_uint(v + 0.0f);
	return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

} // namespace kd
} // namespace mg
