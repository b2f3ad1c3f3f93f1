/*
 * ntsm_eval_chunk.h -- one chunk of a cohort store on the device, stated once for ntsm_eval_cross.hip (the dense rectangle),
 * ntsm_eval_near.hip (the projection of a store), ntsm_eval_within.hip (the triangle, resident or streamed) and
 * ntsm_eval_profile.hip (the QC tallies; the chunk rule and the copy only): the chunk
 * rule; the kernels -- the genotype tallies of the chunk's samples over the dense [chunk sample][site][2] buffer and that
 * buffer's transpose to at / cg / term [site][chunk sample] --; and the step that stages a chunk: the 2-D copy from the
 * host pitch, those kernels, the wall clock and the events that time them.  Also what every store path repeats around its HIP
 * calls, whether it holds a band (ntsm_eval_band.h, which builds on this file) or not (ntsm_eval_trio.hip, ntsm_eval_ld.hip): the check of a store
 * argument, the launch rule of the kernels with a wave-uniform row group, the timed launch and the timed copy.  Internal: not
 * part of include/.  The kernels have internal linkage; each translation unit that includes this file carries its own copy, and names itself first
 * (NTSM_HIP_TAG, ntsm_hip_scope.h).
 */
#ifndef NTSM_EVAL_CHUNK_H
#define NTSM_EVAL_CHUNK_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>

#include "../../include/ntsm_eval_hip.h"
#include "ntsm_eval_score.h"
#include "ntsm_hip_scope.h"

namespace ntsm_eval_chunk {

constexpr int kThreads = 256;
constexpr int kTile = 64;                    /* the transpose moves 64 samples x 64 sites per workgroup */
constexpr uint32_t kMaxGridY = 65535;        /* a grid's second dimension ends here (hipDeviceAttributeMaxGridDimY) */

/* counts [sample][site][2] (dense) -> at / cg / term [site][sample]; grid (tiles of sites, tiles of samples from sample s_first on) */
static __global__ __launch_bounds__(kThreads) void prepare_kernel(const uint2 *__restrict__ counts, uint32_t n_samples, uint32_t n_sites,
		uint32_t min_cov, uint32_t s_first, uint32_t *__restrict__ at, uint32_t *__restrict__ cg, double *__restrict__ term)
{
	__shared__ uint2 tile[kTile][kTile + 1];
	const uint32_t m0 = blockIdx.x * kTile, s0 = s_first + blockIdx.y * kTile;
	const uint32_t lo = threadIdx.x % kTile, hi = threadIdx.x / kTile;              /* hi: 0 ... 3 */
	for (uint32_t r = hi; r < (uint32_t) kTile; r += kThreads / kTile) {             /* lanes along the sites of one sample */
		const uint32_t s = s0 + r, site = m0 + lo;
		if (s < n_samples && site < n_sites) tile[r][lo] = counts[(uint64_t) s * n_sites + site];
	}
	__syncthreads();
	for (uint32_t r = hi; r < (uint32_t) kTile; r += kThreads / kTile) {             /* lanes along the samples of one site */
		const uint32_t s = s0 + lo, site = m0 + r;
		if (s >= n_samples || site >= n_sites) continue;
		const uint2 c = tile[lo][r];
		const uint64_t cell = (uint64_t) site * n_samples + s;
		at[cell] = c.x;
		cg[cell] = c.y;
		term[cell] = ntsm_eval_term(c.x, c.y, min_cov);
	}
}

/* hets, homs, miss of every sample of the chunk (calcHomHetMiss, :742-767): one workgroup per sample; integer sums */
static __global__ __launch_bounds__(kThreads) void tally_kernel(const uint2 *__restrict__ counts, uint32_t n_sites, uint32_t min_cov,
		uint32_t *__restrict__ geno)
{
	__shared__ uint32_t sum[3];
	if (threadIdx.x < 3) sum[threadIdx.x] = 0;
	__syncthreads();
	const uint2 *row = counts + (uint64_t) blockIdx.x * n_sites;
	uint32_t hets = 0, homs = 0, miss = 0;
	for (uint32_t site = threadIdx.x; site < n_sites; site += kThreads) {
		const uint2 c = row[site];
		const bool a = c.x > min_cov, b = c.y > min_cov;
		hets += a && b;
		homs += a != b;
		miss += !a && !b;
	}
	atomicAdd(&sum[0], hets);
	atomicAdd(&sum[1], homs);
	atomicAdd(&sum[2], miss);
	__syncthreads();
	if (threadIdx.x < 3) geno[(uint64_t) blockIdx.x * 3 + threadIdx.x] = sum[threadIdx.x];
}

/* A launch whose grid.y grows with a caller's count goes out in slices of at most kMaxGridY: each(first, count)
 * starts the launch of groups first ... first + count - 1 of n_groups. */
template <typename Each> inline void for_grid_y_slices(uint64_t n_groups, Each &&each)
{
	for (uint64_t g = 0; g < n_groups; g += kMaxGridY) each(g, (uint32_t) std::min<uint64_t>(kMaxGridY, n_groups - g));
}

/* the launches; the caller checks hipGetLastError */
inline void launch_prepare(const uint32_t *counts, uint32_t n_samples, uint32_t n_sites, uint32_t min_cov, uint32_t *at, uint32_t *cg, double *term)
{
	for_grid_y_slices(((uint64_t) n_samples + kTile - 1) / kTile, [&](uint64_t tile, uint32_t tiles) {
		hipLaunchKernelGGL(prepare_kernel, dim3((n_sites + kTile - 1) / kTile, tiles), dim3(kThreads), 0, 0, (const uint2 *) counts, n_samples, n_sites, min_cov,
				(uint32_t) (tile * kTile), at, cg, term);
	});
}

inline void launch_tally(const uint32_t *counts, uint32_t n_samples, uint32_t n_sites, uint32_t min_cov, uint32_t *geno)
{
	hipLaunchKernelGGL(tally_kernel, dim3(n_samples), dim3(kThreads), 0, 0, (const uint2 *) counts, n_sites, min_cov, geno);
}

/* The chunk rule: the caller's db_chunk, or, for 0, as many samples as fit in half of what is free
 * on the device after `fixed` bytes, at `per_sample` bytes each -- fewer passes, fuller launches -- and at least 64. */
inline uint32_t samples_per_pass(uint32_t db_chunk, uint32_t n_db, size_t free_bytes, uint64_t per_sample, uint64_t fixed)
{
	uint32_t chunk = db_chunk;
	if (chunk == 0) {
		const uint64_t budget = free_bytes / 2 > fixed ? free_bytes / 2 - fixed : 0;
		chunk = (uint32_t) std::min<uint64_t>(n_db, std::max<uint64_t>(64, budget / per_sample));
	}
	return std::min(chunk, n_db);
}

/* what every entry point asks of a store argument: n samples of n_sites sites each, [site][2] uint32 at a pitch of `stride` bytes */
inline bool valid_store(const void *counts, uint64_t stride, uint32_t n, uint32_t n_sites)
{
	return !(!counts && n && n_sites) && stride >= 8ull * n_sites && stride % 4 == 0;
}

/* Workgroup width and row group of one launch of a kernel that puts the columns across the lanes and a group of 1, 2 or 4 rows on
 * the wave-uniform side (ntsm_eval_cross.hip, ntsm_eval_contam.hip, the duo kernel of ntsm_eval_trio.hip).  A lane's walk over the
 * sites is sequential, so the only parallelism is across pairs: the widest group whose launch still puts a wave on every SIMD wins
 * (each column value loaded is used `group` times); a rectangle too small for that takes single rows, which at least spreads what
 * there is.  One-wave workgroups at every size: measured 4 to 5 % faster than 256 threads on 1 and 8 queries against 4,096 samples
 * with the cross kernel and not measured again for the other two (sections 9.7, 9.8).  forced_width and
 * forced_group are the caller's _tune values, 0 = this rule. */
constexpr uint64_t kFillWaves = 1024;        /* one wave on every SIMD of the 256 CUs */
inline void launch_shape(uint32_t n_rows, uint32_t n_cols, uint32_t forced_width, uint32_t forced_group, uint32_t &width, uint32_t &group)
{
	width = forced_width ? forced_width : 64;
	const uint64_t waves = (n_cols + 63) / 64;
	group = 1;
	for (uint32_t t = 4; t > 1; t /= 2)
		if (t / 2 < n_rows && waves * ((n_rows + t - 1) / t) >= kFillWaves) { group = t; break; }
	if (forced_group) group = forced_group;
}

typedef std::chrono::steady_clock wall;
static inline double ms_since(wall::time_point t) { return std::chrono::duration<double, std::milli>(wall::now() - t).count(); }

/* one hipMemcpy, its wall time added to *ms */
static inline int timed_copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, double *ms)
{
	const auto t = wall::now();
	HIPCHK(hipMemcpy(dst, src, bytes, kind));
	*ms += ms_since(t);
	return 0;
}

/* the interval between two events that have completed, added to *ms */
static inline int add_interval(hipEvent_t e0, hipEvent_t e1, double *ms)
{
	float f = 0;
	HIPCHK(hipEventElapsedTime(&f, e0, e1));
	*ms += f;
	return 0;
}

/* The timed launch: e0, what `launches` starts on the null stream, e1, the wait for e1, and the interval added to *ms.  `launches`
 * returns 0 or the failure of its own check of hipGetLastError. */
template <typename Launches> static inline int timed(hipEvent_t e0, hipEvent_t e1, double *ms, Launches &&launches)
{
	HIPCHK(hipEventRecord(e0, 0));
	const int rc = launches();
	if (rc) return rc;
	HIPCHK(hipEventRecord(e1, 0));
	HIPCHK(hipEventSynchronize(e1));
	return add_interval(e0, e1, ms);
}

/* Samples first ... first + count - 1 of the store: one 2-D copy from the host pitch to d_raw [count][site][2], timed into
 * tm.upload_ms (added).  The whole of staging for a caller that reads the dense buffer itself (ntsm_eval_profile.hip). */
static inline int upload(const void *db, uint64_t stride, uint32_t first, uint32_t count, uint32_t n_sites, uint32_t *d_raw, ntsm_eval_cross_times &tm)
{
	const uint64_t row_bytes = 8ull * n_sites;
	const auto t = wall::now();
	HIPCHK(hipMemcpy2D(d_raw, row_bytes, (const char *) db + (uint64_t) first * stride, stride, row_bytes, count, hipMemcpyHostToDevice));
	tm.upload_ms += ms_since(t);
	return 0;
}

/* That copy; then, between e0 and e1, with d_at the transpose to at / cg / term [site][count] and with d_geno the tallies.
 * It waits for nothing: a caller adds the interval (e0, e1) to tm.prepare_kernel_ms once it has waited for e1 or for a later
 * event of its own, so a walk over chunks keeps the one wait per chunk it has. */
static inline int stage(const void *db, uint64_t stride, uint32_t first, uint32_t count, uint32_t n_sites, uint32_t min_cov, uint32_t *d_raw, uint32_t *d_at,
		uint32_t *d_cg, double *d_term, uint32_t *d_geno, hipEvent_t e0, hipEvent_t e1, ntsm_eval_cross_times &tm)
{
	const int rc = upload(db, stride, first, count, n_sites, d_raw, tm);
	if (rc) return rc;
	HIPCHK(hipEventRecord(e0, 0));
	if (d_at) {
		launch_prepare(d_raw, count, n_sites, min_cov, d_at, d_cg, d_term);
		HIPCHK(hipGetLastError());
	}
	if (d_geno) {
		launch_tally(d_raw, count, n_sites, min_cov, d_geno);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipEventRecord(e1, 0));
	return 0;
}

}  // namespace ntsm_eval_chunk

#endif
