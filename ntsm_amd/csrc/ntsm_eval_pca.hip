/*
 * ntsm_eval_pca.hip -- the PCA-guided pair search of ntsmEval on one MI355X (include/ntsm_eval_hip.h: ntsm_eval_open,
 * ntsm_eval_project, ntsm_eval_candidates, ntsm_eval_score_pairs; reference: src/CompareCounts.hpp:116-211 projectPCs,
 * :285-398 computeScorePCA).
 *
 * Session.  The counts stay on the device in the files' layout, [sample][site][2], next to the single-sample term of
 * every (sample, site) (computeSumLogPSingle's  first * freqAT + second * freqCG, :971-987, the expression of
 * ntsm_eval.hip's prepare kernel).  Both kernels that read them give one lane one sample and walk its sites in order, so a
 * lane streams its own row and a 64-byte line serves it for 8 (counts) or 8 (terms) consecutive sites.
 *
 * Projection.  One lane per (sample, component): the chain over the sites is sequential (the reference's inner_product),
 * so the parallelism is N * D chains.  A lane forms the genotype code of each site from its counts and adds the product
 * RN64(v_c * rot[d][j]) of a [site][dim][4] table built on the host with real long double (four 16-byte entries per site
 * and component: one cache line, read by every lane of the wave) with the integer x87 add of xprec.h.
 *
 * Search.  Brute force over all pairs: one workgroup per row i, the row's point read wave-uniformly, lanes over k.  A
 * counting pass, a prefix sum over the rows on the host, then a filling pass that compacts each row in k order (wave
 * ballots + an LDS scan across the four waves).  The host sorts each radius row by evalMetric (stable: ties keep k order).
 * IEEE double with __dadd_rn / __dsub_rn / __dmul_rn: the reference is built without contraction.
 *
 * Scoring.  One lane per listed pair, both rows gathered; the same operations in the same order as ntsm_eval_pair_kernel,
 * so a record is bit-identical to the all-pairs one (sample pi as sample 1).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <vector>

#include "../../include/ntsm_eval_hip.h"
#include "xprec.h"

struct ntsm_eval_session {
	int device;
	uint32_t n, m, min_cov;
	uint32_t *counts;                        /* [n][m][2] */
	double *term;                            /* [n][m] */
};

namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void pca_term_kernel(const uint32_t *counts, uint64_t cells, uint32_t min_cov, double *term)
{
	const uint64_t cell = (uint64_t) blockIdx.x * kThreads + threadIdx.x;
	if (cell >= cells) return;
	const uint32_t a0 = counts[cell * 2], a1 = counts[cell * 2 + 1];
	double fAT = 0, fCG = 0;                                                   /* :971-987, as ntsm_eval_prepare */
	if (a0 > min_cov) fAT = __ddiv_rn((double) a0, (double) (a0 + a1));
	if (a1 > min_cov) fCG = __ddiv_rn((double) a1, (double) (a0 + a1));
	term[cell] = __dadd_rn(__dmul_rn((double) a0, fAT), __dmul_rn((double) a1, fCG));
}

/* m_cloud[i][d] (:166-211); tab[(site * dim + d) * 4 + code], code 0 / 1 / 2 = genotype 0 / 0.5 / 1, 3 = missing */
__global__ __launch_bounds__(kThreads) void pca_project_kernel(const uint32_t *__restrict__ counts, uint32_t n, uint32_t m, uint32_t min_cov,
		const ntsm_x64 *__restrict__ tab, uint32_t dim, double *__restrict__ cloud)
{
	const uint32_t i = blockIdx.x * kThreads + threadIdx.x, d = blockIdx.y;
	if (i >= n) return;
	const uint32_t *row = counts + (uint64_t) i * m * 2;
	double acc = 0.0;
	for (uint32_t j = 0; j < m; ++j) {
		const uint32_t a0 = row[2 * j], a1 = row[2 * j + 1];
		const uint32_t cAT = a0 > min_cov ? a0 : 0u, cCG = a1 > min_cov ? a1 : 0u;
		const uint32_t den = cAT + cCG;                                         /* unsigned, as the reference's */
		uint32_t code = 3;
		if (den != 0) {
			const double g = __ddiv_rn((double) cAT, (double) den);
			code = g < 0.25 ? 0u : g < 0.75 ? 1u : 2u;                          /* (g - 0.25) < 0.0 has the sign of g - 0.25 */
		}
		acc = ntsm_x87_acc(acc, tab[((uint64_t) j * dim + d) * 4 + code]);
	}
	cloud[(uint64_t) i * dim + d] = acc;
}

/* nanoflann L2_Adaptor::evalMetric (vendor/nanoflann.hpp:452-486) */
__device__ inline double eval_metric(const double *a, const double *b, uint32_t dim)
{
	double result = 0.0;
	uint32_t t = 0;
	for (; t + 4 <= dim; t += 4) {
		const double d0 = __dsub_rn(a[t], b[t]), d1 = __dsub_rn(a[t + 1], b[t + 1]);
		const double d2 = __dsub_rn(a[t + 2], b[t + 2]), d3 = __dsub_rn(a[t + 3], b[t + 3]);
		result = __dadd_rn(result, __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(d0, d0), __dmul_rn(d1, d1)), __dmul_rn(d2, d2)), __dmul_rn(d3, d3)));
	}
	for (; t < dim; ++t) {
		const double d0 = __dsub_rn(a[t], b[t]);
		result = __dadd_rn(result, __dmul_rn(d0, d0));
	}
	return result;
}

/* calcDistance (:926-932): pow(x, 2) folds to x * x */
__device__ inline double calc_distance(const double *a, const double *b, uint32_t dim)
{
	double dist = 0.0;
	for (uint32_t t = 0; t < dim; ++t) {
		const double x = a[t] < b[t] ? __dsub_rn(b[t], a[t]) : __dsub_rn(a[t], b[t]);
		dist = __dadd_rn(dist, __dmul_rn(x, x));
	}
	return dist;
}

/* computeScorePCA's selection of pair (i, k) (:315-337 radius rows, :358-365 search-all rows) */
__device__ inline bool pca_take(const double *cloud, const double *radius, uint32_t dim, uint32_t i, uint32_t k, double ri, double *metric)
{
	const double rk = radius[k];
	if (!(ri < DBL_MAX)) {
		*metric = 0.0;
		return !(DBL_MAX == rk && k <= i);
	}
	const double dm = eval_metric(cloud + (uint64_t) i * dim, cloud + (uint64_t) k * dim, dim);
	*metric = dm;
	if (!(dm < ri)) return false;
	if (ri == rk) return k > i;
	return !(ri < rk);
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
			dist[p] = calc_distance(cloud + (uint64_t) i * dim, cloud + (uint64_t) k * dim, dim);
		}
		base += total;
		__syncthreads();
	}
}

/* one record per listed pair, sample pi as sample 1: ntsm_eval_pair_kernel's operations in its order */
__global__ __launch_bounds__(kThreads) void pca_score_kernel(const uint32_t *__restrict__ counts, const double *__restrict__ term, uint32_t m, uint32_t min_cov,
		const uint32_t *__restrict__ pi, const uint32_t *__restrict__ pk, uint64_t n_pairs, ntsm_eval_record *__restrict__ out)
{
	const uint64_t p = (uint64_t) blockIdx.x * kThreads + threadIdx.x;
	if (p >= n_pairs) return;
	const uint32_t *ra = counts + (uint64_t) pi[p] * m * 2, *rb = counts + (uint64_t) pk[p] * m * 2;
	const double *ta = term + (uint64_t) pi[p] * m, *tb = term + (uint64_t) pk[p] * m;
	double joint = 0, s1 = 0, s2 = 0;
	uint32_t nv = 0, hets1 = 0, homs1 = 0, hets2 = 0, homs2 = 0, sh_het = 0, sh_hom = 0, ibs0 = 0;
	for (uint32_t site = 0; site < m; ++site) {
		const uint32_t a0 = ra[2 * site], a1 = ra[2 * site + 1], b0 = rb[2 * site], b1 = rb[2 * site + 1];
		const bool vi = a0 > min_cov || a1 > min_cov, vj = b0 > min_cov || b1 > min_cov;
		if (!(vi && vj)) continue;                                              /* gatherValidEntries, :1057-1078 */
		nv++;
		const uint32_t cAT = a0 + b0, cCG = a1 + b1;                            /* computeSumLogPJoint, :1018-1031 */
		const double den = (double) (cAT + cCG);
		double fAT = 0, fCG = 0;
		if (cAT > min_cov) fAT = __ddiv_rn((double) cAT, den);
		if (cCG > min_cov) fCG = __ddiv_rn((double) cCG, den);
		joint = __dadd_rn(joint, __dadd_rn(__dmul_rn((double) cAT, fAT), __dmul_rn((double) cCG, fCG)));
		s1 = __dadd_rn(s1, ta[site]);
		s2 = __dadd_rn(s2, tb[site]);
		const bool heti = a0 > min_cov && a1 > min_cov, hetj = b0 > min_cov && b1 > min_cov;   /* calcRelatedness, :1151-1188 */
		const bool i_at = a0 > min_cov, j_at = b0 > min_cov;
		hets1 += heti; homs1 += !heti;
		hets2 += hetj; homs2 += !hetj;
		if (heti && hetj) sh_het++;
		else if (!heti && !hetj) { if (i_at == j_at) sh_hom++; else ibs0++; }
	}
	ntsm_eval_record r;
	r.sum_joint = joint; r.sum_single1 = s1; r.sum_single2 = s2;
	r.n_valid = nv;
	r.hets1 = hets1; r.homs1 = homs1; r.hets2 = hets2; r.homs2 = homs2;
	r.shared_hets = sh_het; r.shared_homs = sh_hom; r.ibs0 = ibs0; r.ibs2 = sh_het + sh_hom;
	out[p] = r;
}

/* device buffers freed on every return path */
struct DevBuf {
	std::vector<void *> ptr;
	~DevBuf() { for (void *p : ptr) (void) hipFree(p); }
	template <typename T> hipError_t alloc(T **p, uint64_t count)
	{
		*p = nullptr;
		if (count == 0) count = 1;
		const hipError_t e = hipMalloc((void **) p, count * sizeof(T));
		if (e == hipSuccess) ptr.push_back(*p);
		return e;
	}
};

struct Timer {
	hipEvent_t e0 = nullptr, e1 = nullptr;
	~Timer() { if (e0) (void) hipEventDestroy(e0); if (e1) (void) hipEventDestroy(e1); }
	hipError_t init() { hipError_t e = hipEventCreate(&e0); return e != hipSuccess ? e : hipEventCreate(&e1); }
};

}  // namespace

#define PCHK(x) do { if ((x) != hipSuccess) return -2; } while (0)

extern "C" int ntsm_eval_open(int device, const uint32_t *counts, uint32_t n_samples, uint32_t n_sites, uint32_t min_cov, ntsm_eval_session **h)
{
	if (!h || (!counts && (uint64_t) n_samples * n_sites > 0)) return -1;
	*h = nullptr;
	ntsm_eval_session *s = new ntsm_eval_session { device, n_samples, n_sites, min_cov, nullptr, nullptr };
	const uint64_t cells = (uint64_t) n_samples * n_sites;
	int rc = 0;
	if (hipSetDevice(device) != hipSuccess || hipMalloc(&s->counts, (cells ? cells : 1) * 2 * sizeof(uint32_t)) != hipSuccess ||
	    hipMalloc(&s->term, (cells ? cells : 1) * sizeof(double)) != hipSuccess) rc = -2;
	if (!rc && cells) {
		if (hipMemcpy(s->counts, counts, cells * 2 * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) rc = -2;
		if (!rc) {
			hipLaunchKernelGGL(pca_term_kernel, dim3((unsigned) ((cells + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0, s->counts, cells, min_cov, s->term);
			if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = -2;
		}
	}
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
	/* the x87 products RN64(v_c * rot[d][j]) (:190-210): v_c = double(c - norm[j]) for c = 0, 0.5, 1; +0.0 for a missing site */
	std::vector<ntsm_x64> tab((uint64_t) m * dim * 4);
	for (uint32_t j = 0; j < m; ++j) {
		double v[4];
		for (int c = 0; c < 3; ++c) {
			volatile long double diff = (long double) (c * 0.5) - norm[j];
			v[c] = (double) diff;
		}
		v[3] = 0.0;
		for (uint32_t d = 0; d < dim; ++d)
			for (int c = 0; c < 4; ++c) {
				volatile long double prod = (long double) v[c] * rot[(uint64_t) d * m + j];
				tab[((uint64_t) j * dim + d) * 4 + c] = ntsm_x64_from_ld(prod);
			}
	}
	if (m == 0) {                                                               /* no site: inner_product of nothing */
		for (uint64_t t = 0; t < (uint64_t) n * dim; ++t) cloud[t] = 0.0;
		return 0;
	}
	PCHK(hipSetDevice(h->device));
	DevBuf b;
	ntsm_x64 *d_tab;
	double *d_cloud;
	PCHK(b.alloc(&d_tab, tab.size()));
	PCHK(b.alloc(&d_cloud, (uint64_t) n * dim));
	PCHK(hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(ntsm_x64), hipMemcpyHostToDevice));
	Timer t;
	PCHK(t.init());
	PCHK(hipEventRecord(t.e0, 0));
	hipLaunchKernelGGL(pca_project_kernel, dim3((n + kThreads - 1) / kThreads, dim), dim3(kThreads), 0, 0, h->counts, n, m, h->min_cov, d_tab, dim, d_cloud);
	PCHK(hipGetLastError());
	PCHK(hipEventRecord(t.e1, 0));
	PCHK(hipMemcpy(cloud, d_cloud, (uint64_t) n * dim * sizeof(double), hipMemcpyDeviceToHost));
	float ms = 0;
	PCHK(hipEventElapsedTime(&ms, t.e0, t.e1));
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
	PCHK(hipSetDevice(h->device));
	DevBuf b;
	double *d_cloud, *d_radius;
	uint32_t *d_count;
	PCHK(b.alloc(&d_cloud, (uint64_t) n * dim));
	PCHK(b.alloc(&d_radius, n));
	PCHK(b.alloc(&d_count, n));
	if (dim) PCHK(hipMemcpy(d_cloud, cloud, (uint64_t) n * dim * sizeof(double), hipMemcpyHostToDevice));
	PCHK(hipMemcpy(d_radius, radius, n * sizeof(double), hipMemcpyHostToDevice));
	Timer t;
	PCHK(t.init());
	PCHK(hipEventRecord(t.e0, 0));
	hipLaunchKernelGGL(pca_count_kernel, dim3(n), dim3(kThreads), 0, 0, d_cloud, d_radius, n, dim, d_count);
	PCHK(hipGetLastError());
	PCHK(hipEventRecord(t.e1, 0));
	std::vector<uint32_t> count(n);
	PCHK(hipMemcpy(count.data(), d_count, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
	float ms0 = 0;
	PCHK(hipEventElapsedTime(&ms0, t.e0, t.e1));
	std::vector<uint64_t> offset(n + 1, 0);
	for (uint32_t i = 0; i < n; ++i) offset[i + 1] = offset[i] + count[i];
	const uint64_t total = offset[n];
	*n_pairs = total;
	if (kernel_ms) *kernel_ms = ms0;
	if (total > capacity) return NTSM_EVAL_E_CAPACITY;
	if (total == 0) return 0;
	uint64_t *d_offset;
	uint32_t *d_pk;
	double *d_metric, *d_dist;
	PCHK(b.alloc(&d_offset, n + 1));
	PCHK(b.alloc(&d_pk, total));
	PCHK(b.alloc(&d_metric, total));
	PCHK(b.alloc(&d_dist, total));
	PCHK(hipMemcpy(d_offset, offset.data(), (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
	PCHK(hipEventRecord(t.e0, 0));
	hipLaunchKernelGGL(pca_fill_kernel, dim3(n), dim3(kThreads), 0, 0, d_cloud, d_radius, n, dim, d_offset, d_pk, d_metric, d_dist);
	PCHK(hipGetLastError());
	PCHK(hipEventRecord(t.e1, 0));
	std::vector<uint32_t> k(total);
	std::vector<double> metric(total), dd(total);
	PCHK(hipMemcpy(k.data(), d_pk, total * sizeof(uint32_t), hipMemcpyDeviceToHost));
	PCHK(hipMemcpy(metric.data(), d_metric, total * sizeof(double), hipMemcpyDeviceToHost));
	PCHK(hipMemcpy(dd.data(), d_dist, total * sizeof(double), hipMemcpyDeviceToHost));
	float ms1 = 0;
	PCHK(hipEventElapsedTime(&ms1, t.e0, t.e1));
	if (kernel_ms) *kernel_ms = (double) ms0 + ms1;
	/* radius rows in ascending evalMetric (nanoflann sorts its matches); the fill wrote k ascending, so a stable sort
	 * orders exact ties by k */
	std::vector<uint64_t> ord;
	for (uint32_t i = 0; i < n; ++i) {
		const uint64_t lo = offset[i], hi = offset[i + 1];
		ord.resize(hi - lo);
		for (uint64_t p = lo; p < hi; ++p) ord[p - lo] = p;
		if (radius[i] < DBL_MAX)
			std::stable_sort(ord.begin(), ord.end(), [&](uint64_t x, uint64_t y) { return metric[x] < metric[y]; });
		for (uint64_t q = 0; q < ord.size(); ++q) {
			pi[lo + q] = i;
			pk[lo + q] = k[ord[q]];
			dist[lo + q] = dd[ord[q]];
		}
	}
	return 0;
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
	PCHK(hipSetDevice(h->device));
	DevBuf b;
	uint32_t *d_pi, *d_pk;
	ntsm_eval_record *d_out;
	PCHK(b.alloc(&d_pi, n_pairs));
	PCHK(b.alloc(&d_pk, n_pairs));
	PCHK(b.alloc(&d_out, n_pairs));
	PCHK(hipMemcpy(d_pi, pi, n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice));
	PCHK(hipMemcpy(d_pk, pk, n_pairs * sizeof(uint32_t), hipMemcpyHostToDevice));
	Timer t;
	PCHK(t.init());
	PCHK(hipEventRecord(t.e0, 0));
	hipLaunchKernelGGL(pca_score_kernel, dim3((unsigned) ((n_pairs + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0, h->counts, h->term, h->m, h->min_cov,
			d_pi, d_pk, n_pairs, d_out);
	PCHK(hipGetLastError());
	PCHK(hipEventRecord(t.e1, 0));
	PCHK(hipMemcpy(out, d_out, n_pairs * sizeof(ntsm_eval_record), hipMemcpyDeviceToHost));
	float ms = 0;
	PCHK(hipEventElapsedTime(&ms, t.e0, t.e1));
	if (kernel_ms) *kernel_ms = ms;
	return 0;
}
