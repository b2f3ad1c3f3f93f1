/*
 * ntsm_eval.hip -- all-pairs scoring of ntsmEval on one MI355X (include/ntsm_eval_hip.h; reference:
 * src/CompareCounts.hpp:591-624 computeScore and the functions it calls).
 *
 * Layout.  The reference keeps m_counts[sample][site]; a pair walks two rows.  Here the counts are transposed once to
 * [site][sample] and one thread owns one pair (i, j): a 256-thread workgroup takes 256 consecutive j against TI = 4
 * consecutive i, so at every site the j side is one coalesced 4-byte load per array and the i side is wave-uniform
 * (scalar loads), and each j value loaded is used for four pairs.  The single-sample term of a site,
 *   first * freqAT + second * freqCG   (computeSumLogPSingle, :971-987),
 * does not depend on the partner, so it is computed once per (sample, site) by the prepare kernel and the pair kernel only
 * adds it when the site is valid for the pair -- the same additions in the same order as the reference's loop over
 * validIndexes.  The term, the per-site update of a pair and its record are those of ntsm_eval_score.h, which
 * ntsm_eval_pca.hip's kernels call as well: the arithmetic (IEEE double without contraction, sequential sums) is stated there.
 * Bound: the vector ALUs (two correctly rounded double divisions per pair and site); the 12 bytes per j and site come
 * from L2 for all but the first of the workgroups that share a j range.
 */
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/ntsm_eval_hip.h"
#include "ntsm_eval_score.h"
#define NTSM_HIP_TAG "ntsm_eval"
#include "ntsm_hip_scope.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTI = 4;                       /* samples i per workgroup row */

/* [sample][site][2] -> at[site][sample], cg[site][sample], term[site][sample] */
__global__ __launch_bounds__(kThreads) void ntsm_eval_prepare(const uint32_t *counts, uint32_t n_samples, uint32_t n_sites, uint32_t min_cov,
		uint32_t *at, uint32_t *cg, double *term)
{
	const uint64_t cell = (uint64_t) blockIdx.x * kThreads + threadIdx.x;       /* site-major: neighbouring threads = neighbouring samples */
	if (cell >= (uint64_t) n_samples * n_sites) return;
	const uint32_t site = (uint32_t) (cell / n_samples), s = (uint32_t) (cell % n_samples);
	const uint32_t a0 = counts[((uint64_t) s * n_sites + site) * 2], a1 = counts[((uint64_t) s * n_sites + site) * 2 + 1];
	at[cell] = a0;
	cg[cell] = a1;
	term[cell] = ntsm_eval_term(a0, a1, min_cov);
}

__global__ __launch_bounds__(kThreads) void ntsm_eval_pair_kernel(const uint32_t *__restrict__ at, const uint32_t *__restrict__ cg, const double *__restrict__ term,
		uint32_t n_samples, uint32_t n_sites, uint32_t min_cov, ntsm_eval_record *__restrict__ out)
{
	const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t i0 = blockIdx.y * kTI;
	if (blockIdx.x * blockDim.x + (blockDim.x - 1) <= i0) return;               /* the whole tile lies on or below the diagonal */
	const uint32_t jc = j < n_samples ? j : n_samples - 1;                      /* lanes past the end compute a copy of the last sample, not stored */
	ntsm_eval_acc acc[kTI];
	for (uint32_t site = 0; site < n_sites; ++site) {
		const uint64_t row = (uint64_t) site * n_samples;
		const ntsm_eval_side sj = ntsm_eval_side_of(at[row + jc], cg[row + jc], term[row + jc], min_cov);
#pragma unroll
		for (int ii = 0; ii < kTI; ++ii) {
			const uint32_t i = i0 + ii < n_samples ? i0 + ii : n_samples - 1;   /* wave-uniform: scalar loads */
			acc[ii].add(ntsm_eval_side_of(at[row + i], cg[row + i], term[row + i], min_cov), sj, min_cov);
		}
	}
	if (j >= n_samples) return;
#pragma unroll
	for (int ii = 0; ii < kTI; ++ii) {
		const uint32_t i = i0 + ii;
		if (i >= n_samples || j <= i) continue;
		out[(uint64_t) i * n_samples - (uint64_t) i * (i + 1) / 2 + (j - i - 1)] = acc[ii].record();   /* ntsm_eval_pair_index */
	}
}

}  // namespace

extern "C" int ntsm_eval_pairs(int device, const uint32_t *counts, uint32_t n_samples, uint32_t n_sites, uint32_t min_cov,
		ntsm_eval_record *out, double *kernel_ms)
{
	if (!counts || (!out && n_samples > 1)) return -1;
	if (kernel_ms) *kernel_ms = 0;
	if (n_samples < 2 || n_sites == 0) {
		for (uint64_t p = 0; n_samples >= 2 && p < (uint64_t) n_samples * (n_samples - 1) / 2; ++p) out[p] = ntsm_eval_record {};
		return 0;
	}
	const uint64_t cells = (uint64_t) n_samples * n_sites, pairs = (uint64_t) n_samples * (n_samples - 1) / 2;
	ntsm_hip::Buffers b;
	ntsm_hip::Events<2> ev;
	uint32_t *d_counts, *d_at, *d_cg;
	double *d_term;
	ntsm_eval_record *d_out;
	HIPCHK(hipSetDevice(device));
	HIPCHK(b.alloc(&d_counts, cells * 2));
	HIPCHK(b.alloc(&d_at, cells));
	HIPCHK(b.alloc(&d_cg, cells));
	HIPCHK(b.alloc(&d_term, cells));
	HIPCHK(b.alloc(&d_out, pairs));
	HIPCHK(hipMemcpy(d_counts, counts, cells * 2 * sizeof(uint32_t), hipMemcpyHostToDevice));
	HIPCHK(ev.create());
	hipLaunchKernelGGL(ntsm_eval_prepare, dim3((unsigned) ((cells + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0,
			d_counts, n_samples, n_sites, min_cov, d_at, d_cg, d_term);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(ev[0], 0));
	{   /* the sums of a pair are sequential over the sites, so the only parallelism is across pairs: few samples get
	     * one-wave workgroups (S = 256: 256 workgroups instead of 64) */
		const unsigned bt = n_samples <= 1024 ? 64 : kThreads;
		hipLaunchKernelGGL(ntsm_eval_pair_kernel, dim3((n_samples + bt - 1) / bt, (n_samples + kTI - 1) / kTI), dim3(bt), 0, 0,
				d_at, d_cg, d_term, n_samples, n_sites, min_cov, d_out);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(ev[1], 0));
	HIPCHK(hipMemcpy(out, d_out, pairs * sizeof(ntsm_eval_record), hipMemcpyDeviceToHost));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
	if (kernel_ms) *kernel_ms = ms;
	return 0;
}
