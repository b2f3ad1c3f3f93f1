/*
 * ntsm_hip_scope.h -- what the host side of every cohort library (ntsm_eval*.hip, ntsm_vcf.hip, ntsm_pca.hip,
 * ntsm_sitegen.hip, ntsm_sitegen_gap.hip) needs around its HIP calls: owners that release device buffers, events, a stream
 * and pinned host memory when their scope ends, on every return path, and one check.  Internal: not part of include/.
 *
 * A translation unit names itself before it includes this file:
 *   #define NTSM_HIP_TAG "ntsm_eval"       the prefix of the message
 *   #define NTSM_HIP_FAIL ...              the library's HIP error code, if it is not -2
 * HIPCHK(call): on a HIP error print "<tag>: <call> failed: <hipGetErrorString>" to stderr and return NTSM_HIP_FAIL from
 * the enclosing function.  Owners declared before it unwind, so a failing path needs no list of what to free.  The runtime
 * keeps a failed call's error until hipGetLastError reads it; the check reads it, or the launch check of the caller's next,
 * healthy call would report it.
 */
#ifndef NTSM_HIP_SCOPE_H
#define NTSM_HIP_SCOPE_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#ifndef NTSM_HIP_TAG
#error "define NTSM_HIP_TAG before including ntsm_hip_scope.h"
#endif
#ifndef NTSM_HIP_FAIL
#define NTSM_HIP_FAIL (-2)
#endif

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
	fprintf(stderr, NTSM_HIP_TAG ": %s failed: %s\n", #x, hipGetErrorString(e_)); (void) hipGetLastError(); return NTSM_HIP_FAIL; } } while (0)

namespace ntsm_hip {

/* device buffers, freed when the scope ends */
class Buffers {
	std::vector<void *> ptr;
public:
	Buffers() = default;
	Buffers(const Buffers &) = delete;
	Buffers &operator=(const Buffers &) = delete;
	~Buffers() { for (void *p : ptr) (void) hipFree(p); }
	/* count elements of T; a count of zero allocates one element, so no caller special-cases an empty input */
	template <typename T> hipError_t alloc(T **p, uint64_t count)
	{
		*p = nullptr;
		const hipError_t e = hipMalloc((void **) p, (count ? count : 1) * sizeof(T));
		if (e == hipSuccess) ptr.push_back(*p);
		return e;
	}
	/* free one buffer before the scope ends (to replace it with a larger one without holding both) */
	template <typename T> hipError_t release(T **p)
	{
		ptr.erase(std::remove(ptr.begin(), ptr.end(), (void *) *p), ptr.end());
		const hipError_t e = hipFree(*p);
		*p = nullptr;
		return e;
	}
};

/* N events, destroyed when the scope ends */
template <int N> class Events {
	hipEvent_t ev[N] = {};
public:
	Events() = default;
	Events(const Events &) = delete;
	Events &operator=(const Events &) = delete;
	~Events() { for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e); }
	hipError_t create()
	{
		for (hipEvent_t &e : ev) {
			const hipError_t rc = hipEventCreate(&e);
			if (rc != hipSuccess) return rc;
		}
		return hipSuccess;
	}
	hipEvent_t operator[](int i) const { return ev[i]; }
};

/* a stream, destroyed when the scope ends */
class Stream {
	hipStream_t s = nullptr;
public:
	Stream() = default;
	Stream(const Stream &) = delete;
	Stream &operator=(const Stream &) = delete;
	~Stream() { if (s) (void) hipStreamDestroy(s); }
	hipError_t create() { return hipStreamCreate(&s); }
	operator hipStream_t() const { return s; }
};

/* pinned host bytes, freed when the scope ends */
class Pinned {
	void *p = nullptr;
public:
	Pinned() = default;
	Pinned(const Pinned &) = delete;
	Pinned &operator=(const Pinned &) = delete;
	~Pinned() { if (p) (void) hipHostFree(p); }
	hipError_t alloc(uint64_t bytes) { return hipHostMalloc(&p, bytes, hipHostMallocDefault); }
	uint8_t *bytes() const { return (uint8_t *) p; }
};

}  // namespace ntsm_hip

#endif
