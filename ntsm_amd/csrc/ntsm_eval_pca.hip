/*
 * ntsm_eval_pca.hip -- the PCA-guided pair search of ntsmEval on one MI355X (include/ntsm_eval_hip.h: ntsm_eval_open,
 * ntsm_eval_project, ntsm_eval_candidates, ntsm_eval_score_pairs; reference: src/CompareCounts.hpp:116-211 projectPCs,
 * :285-398 computeScorePCA).
 *
 * Session.  The counts stay on the device in the files' layout, [sample][site][2], next to the single-sample term of
 * every (sample, site) (computeSumLogPSingle's  first * freqAT + second * freqCG, :971-987: ntsm_eval_score.h's
 * ntsm_eval_term, which ntsm_eval.hip's prepare kernel calls too).  Both kernels that read them give one lane one sample
 * and walk its sites in order, so a lane streams its own row and a 64-byte line serves it for 8 (counts) or 8 (terms)
 * consecutive sites.
 *
 * Projection.  One lane per (sample, component): the chain over the sites is sequential (the reference's inner_product),
 * so the parallelism is N * D chains.  A lane forms the genotype code of each site from its counts and adds the product
 * RN64(v_c * rot[d][j]) of a [site][dim][4] table built on the host with real long double (four 16-byte entries per site
 * and component: one cache line, read by every lane of the wave) with the integer x87 add of xprec.h.
 *
 * Search.  Brute force over all pairs: one workgroup per row i, the row's point read wave-uniformly, lanes over k.  A
 * counting pass, a prefix sum over the rows on the host, then a filling pass that compacts each row in k order (wave
 * ballots + an LDS scan across the four waves).  The host half -- offsets, capacity, the order of a radius row by (evalMetric,
 * k) -- is ntsm_eval_pca.h's finish_candidates, shared with the search against a store.
 * IEEE double with __dadd_rn / __dsub_rn / __dmul_rn: the reference is built without contraction.
 *
 * Scoring.  One lane per listed pair, both rows gathered; the per-site update and the record are ntsm_eval_score.h's, the
 * ones ntsm_eval_pair_kernel calls, so a record is bit-identical to the all-pairs one (sample pi as sample 1).
 *
 * What the search against a cohort store (ntsm_eval_near.hip) needs as well -- the projection kernel and its product table,
 * evalMetric, calcDistance, the selection rule, the term and scoring kernels -- is ntsm_eval_pca.h's.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "../../include/ntsm_eval_hip.h"
#define NTSM_HIP_TAG "ntsm_eval"
#include "ntsm_eval_pca.h"
#include "ntsm_eval_score.h"
#include "ntsm_hip_scope.h"
#include "xprec.h"

struct ntsm_eval_session {
	int device;
	uint32_t n, m, min_cov;
	uint32_t *counts;                        /* [n][m][2] */
	double *term;                            /* [n][m] */
};

namespace {

using ntsm_eval_pca::kThreads;

/* computeScorePCA's selection of pair (i, k) of one cloud (ntsm_eval_pca.h) */
__device__ inline bool pca_take(const double *cloud, const double *radius, uint32_t dim, uint32_t i, uint32_t k, double ri, double *metric)
{
	return ntsm_eval_pca::take(cloud + (uint64_t) i * dim, cloud + (uint64_t) k * dim, dim, i, k, ri, radius[k], metric);
}

/* pass 1: count[i] = number of pairs of row i */
__global__ __launch_bounds__(kThreads) void pca_count_kernel(const double *__restrict__ cloud, const double *__restrict__ radius, uint32_t n, uint32_t dim,
		uint32_t *__restrict__ count)
{
	const uint32_t i = blockIdx.x;
	const double ri = radius[i];
	uint32_t c = 0;
	for (uint32_t k0 = 0; k0 < n; k0 += kThreads) {
		const uint32_t k = k0 + threadIdx.x;
		double dm;
		c += (k < n && pca_take(cloud, radius, dim, i, k, ri, &dm)) ? 1u : 0u;
	}
	__shared__ uint32_t s_sum[kThreads / 64];
	for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
	if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = c;
	__syncthreads();
	if (threadIdx.x == 0) {
		uint32_t t = 0;
		for (int w = 0; w < kThreads / 64; ++w) t += s_sum[w];
		count[i] = t;
	}
}

/* pass 2: the pairs of row i at offset[i], in k order */
__global__ __launch_bounds__(kThreads) void pca_fill_kernel(const double *__restrict__ cloud, const double *__restrict__ radius, uint32_t n, uint32_t dim,
		const uint64_t *__restrict__ offset, uint32_t *__restrict__ pk, double *__restrict__ metric, double *__restrict__ dist)
{
	const uint32_t i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const double ri = radius[i];
	__shared__ uint32_t s_cnt[kThreads / 64];
	uint64_t base = offset[i];
	for (uint32_t k0 = 0; k0 < n; k0 += kThreads) {
		const uint32_t k = k0 + threadIdx.x;
		double dm = 0.0;
		const bool take = k < n && pca_take(cloud, radius, dim, i, k, ri, &dm);
		const uint64_t ballot = __ballot(take);
		if (lane == 0) s_cnt[wave] = (uint32_t) __popcll(ballot);
		__syncthreads();
		uint32_t before = 0, total = 0;
		for (uint32_t w = 0; w < kThreads / 64; ++w) { before += w < wave ? s_cnt[w] : 0u; total += s_cnt[w]; }
		if (take) {
			const uint64_t p = base + before + (uint32_t) __popcll(ballot & ((1ull << lane) - 1));
			pk[p] = k;
			metric[p] = dm;
			dist[p] = ntsm_eval_pca::calc_distance(cloud + (uint64_t) i * dim, cloud + (uint64_t) k * dim, dim);
		}
		base += total;
		__syncthreads();
	}
}

/* the session's device state: the upload and the term of every cell */
int session_upload(ntsm_eval_session *s, const uint32_t *counts, uint64_t cells)
{
	HIPCHK(hipMalloc(&s->counts, (cells ? cells : 1) * 2 * sizeof(uint32_t)));
	HIPCHK(hipMalloc(&s->term, (cells ? cells : 1) * sizeof(double)));
	if (cells == 0) return 0;
	HIPCHK(hipMemcpy(s->counts, counts, cells * 2 * sizeof(uint32_t), hipMemcpyHostToDevice));
	ntsm_eval_pca::launch_term(s->counts, cells, s->min_cov, s->term);
	HIPCHK(hipGetLastError());
	HIPCHK(hipDeviceSynchronize());
	return 0;
}

}  // namespace

extern "C" int ntsm_eval_open(int device, const uint32_t *counts, uint32_t n_samples, uint32_t n_sites, uint32_t min_cov, ntsm_eval_session **h)
{
	if (!h || (!counts && (uint64_t) n_samples * n_sites > 0)) return -1;
	*h = nullptr;
	HIPCHK(hipSetDevice(device));                                               /* before the session exists: ntsm_eval_close sets its device */
	ntsm_eval_session *s = new ntsm_eval_session { device, n_samples, n_sites, min_cov, nullptr, nullptr };
	const int rc = session_upload(s, counts, (uint64_t) n_samples * n_sites);
	if (rc) { ntsm_eval_close(s); return rc; }
	*h = s;
	return 0;
}

extern "C" void ntsm_eval_close(ntsm_eval_session *h)
{
	if (!h) return;
	(void) hipSetDevice(h->device);
	(void) hipFree(h->counts);
	(void) hipFree(h->term);
	delete h;
}

extern "C" int ntsm_eval_project(ntsm_eval_session *h, const long double *norm, const long double *rot, uint32_t dim, double *cloud, double *kernel_ms)
{
	if (kernel_ms) *kernel_ms = 0;
	if (!h || (h->m && (!norm || (dim && !rot))) || (h->n && dim && !cloud)) return -1;
	const uint32_t n = h->n, m = h->m;
	if ((uint64_t) n * dim == 0) return 0;
	const std::vector<ntsm_x64> tab = ntsm_eval_pca::product_table(norm, rot, m, dim);
	if (m == 0) {                                                               /* no site: inner_product of nothing */
		for (uint64_t t = 0; t < (uint64_t) n * dim; ++t) cloud[t] = 0.0;
		return 0;
	}
	HIPCHK(hipSetDevice(h->device));
	ntsm_hip::Buffers b;
	ntsm_x64 *d_tab;
	double *d_cloud;
	HIPCHK(b.alloc(&d_tab, tab.size()));
	HIPCHK(b.alloc(&d_cloud, (uint64_t) n * dim));
	HIPCHK(hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(ntsm_x64), hipMemcpyHostToDevice));
	ntsm_hip::Events<2> ev;
	HIPCHK(ev.create());
	HIPCHK(hipEventRecord(ev[0], 0));
	ntsm_eval_pca::launch_project(h->counts, n, m, h->min_cov, d_tab, dim, d_cloud);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(ev[1], 0));
	HIPCHK(hipMemcpy(cloud, d_cloud, (uint64_t) n * dim * sizeof(double), hipMemcpyDeviceToHost));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
	if (kernel_ms) *kernel_ms = ms;
	return 0;
}

extern "C" int ntsm_eval_candidates(ntsm_eval_session *h, const double *cloud, uint32_t dim, const double *radius, uint32_t *pi, uint32_t *pk,
		double *dist, uint64_t capacity, uint64_t *n_pairs, double *kernel_ms)
{
	if (kernel_ms) *kernel_ms = 0;
	if (!h || !n_pairs || (h->n && (!radius || (dim && !cloud))) || (capacity && (!pi || !pk || !dist))) return -1;
	*n_pairs = 0;
	const uint32_t n = h->n;
	if (n < 2) return 0;
	HIPCHK(hipSetDevice(h->device));
	ntsm_hip::Buffers b;
	double *d_cloud, *d_radius;
	uint32_t *d_count;
	HIPCHK(b.alloc(&d_cloud, (uint64_t) n * dim));
	HIPCHK(b.alloc(&d_radius, n));
	HIPCHK(b.alloc(&d_count, n));
	if (dim) HIPCHK(hipMemcpy(d_cloud, cloud, (uint64_t) n * dim * sizeof(double), hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(d_radius, radius, n * sizeof(double), hipMemcpyHostToDevice));
	ntsm_hip::Events<2> ev;
	HIPCHK(ev.create());
	HIPCHK(hipEventRecord(ev[0], 0));
	hipLaunchKernelGGL(pca_count_kernel, dim3(n), dim3(kThreads), 0, 0, d_cloud, d_radius, n, dim, d_count);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(ev[1], 0));
	std::vector<uint32_t> count(n);
	HIPCHK(hipMemcpy(count.data(), d_count, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return ntsm_eval_pca::finish_candidates(b, ev[0], ev[1], count,
			[&](const uint64_t *d_offset, uint32_t *d_k, double *d_metric, double *d_dist) {
				hipLaunchKernelGGL(pca_fill_kernel, dim3(n), dim3(kThreads), 0, 0, d_cloud, d_radius, n, dim, d_offset, d_k, d_metric, d_dist);
			},
			[&](uint32_t i) { return radius[i]; }, pi, pk, dist, capacity, n_pairs, kernel_ms);
}

extern "C" int ntsm_eval_score_pairs(ntsm_eval_session *h, const uint32_t *pi, const uint32_t *pk, uint64_t n_pairs, ntsm_eval_record *out,
		double *kernel_ms)
{
	if (kernel_ms) *kernel_ms = 0;
	if (!h || (n_pairs && (!pi || !pk || !out))) return -1;
	for (uint64_t p = 0; p < n_pairs; ++p)
		if (pi[p] >= h->n || pk[p] >= h->n || pi[p] == pk[p]) return -1;
	if (n_pairs == 0) return 0;
	if (h->m == 0) {
		for (uint64_t p = 0; p < n_pairs; ++p) out[p] = ntsm_eval_record {};
		return 0;
	}
	HIPCHK(hipSetDevice(h->device));
	ntsm_hip::Buffers b;
	uint32_t *d_pi, *d_pk;
	ntsm_eval_record *d_out;
	HIPCHK(b.alloc(&d_pi, n_pairs));
	HIPCHK(b.alloc(&d_pk, n_pairs));
	HIPCHK(b.alloc(&d_out, n_pairs));
	HIPCHK(hipMemcpy(d_pi, pi, n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(d_pk, pk, n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice));
	ntsm_hip::Events<2> ev;
	HIPCHK(ev.create());
	HIPCHK(hipEventRecord(ev[0], 0));
	ntsm_eval_pca::launch_score(h->counts, h->term, h->m, h->min_cov, d_pi, d_pk, n_pairs, d_out);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(ev[1], 0));
	HIPCHK(hipMemcpy(out, d_out, n_pairs * sizeof(ntsm_eval_record), hipMemcpyDeviceToHost));
	float ms = 0;
	HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
	if (kernel_ms) *kernel_ms = ms;
	return 0;
}
