/*
 * ntsm_eval_pca.h -- the steps of the PCA-guided search that its two forms share, each stated once: ntsm_eval_pca.hip (one
 * run's samples against each other) and ntsm_eval_near.hip (new samples against a cohort store).  The projection kernel,
 * the genotype code of a site and the host's product table (src/CompareCounts.hpp:166-211), nanoflann's evalMetric, calcDistance
 * and computeScorePCA's selection of a pair (:285-398), the host half of a candidate search (from the rows' counts to the
 * ordered list), and the scoring of listed pairs over [sample][site][2] rows.  Internal: not part of include/.  The kernels
 * have internal linkage; a translation unit names itself (NTSM_HIP_TAG, ntsm_hip_scope.h) before it includes this file.
 */
#ifndef NTSM_EVAL_PCA_H
#define NTSM_EVAL_PCA_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <vector>

#include "../../include/ntsm_eval_hip.h"
#include "ntsm_eval_score.h"
#include "ntsm_hip_scope.h"
#include "xprec.h"

namespace ntsm_eval_pca {

constexpr int kThreads = 256;

/* the column of the product table a site's counts select: 0 / 1 / 2 = genotype 0 / 0.5 / 1, 3 = missing (:179-198) */
__device__ inline uint32_t genotype_code(uint32_t a0, uint32_t a1, uint32_t min_cov)
{
	const uint32_t cAT = a0 > min_cov ? a0 : 0u, cCG = a1 > min_cov ? a1 : 0u;
	const uint32_t den = cAT + cCG;                                             /* unsigned, as the reference's */
	if (den == 0) return 3;
	const double g = __ddiv_rn((double) cAT, (double) den);
	return g < 0.25 ? 0u : g < 0.75 ? 1u : 2u;                                  /* (g - 0.25) < 0.0 has the sign of g - 0.25 */
}

/* the x87 products RN64(v_c * rot[d][j]) (:190-210): v_c = double(c - norm[j]) for c = 0, 0.5, 1; +0.0 for a missing site.
 * tab[(site * dim + d) * 4 + code] */
inline std::vector<ntsm_x64> product_table(const long double *norm, const long double *rot, uint32_t m, uint32_t dim)
{
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
	return tab;
}

/* m_cloud[i][d] (:166-211) over dense [sample][site][2] rows: one lane per (sample, component), grid (n / 256, dim) */
static __global__ __launch_bounds__(kThreads) void project_kernel(const uint32_t *__restrict__ counts, uint32_t n, uint32_t m, uint32_t min_cov,
		const ntsm_x64 *__restrict__ tab, uint32_t dim, double *__restrict__ cloud)
{
	const uint32_t i = blockIdx.x * kThreads + threadIdx.x, d = blockIdx.y;
	if (i >= n) return;
	const uint32_t *row = counts + (uint64_t) i * m * 2;
	double acc = 0.0;
	for (uint32_t j = 0; j < m; ++j)
		acc = ntsm_x87_acc(acc, tab[((uint64_t) j * dim + d) * 4 + genotype_code(row[2 * j], row[2 * j + 1], min_cov)]);
	cloud[(uint64_t) i * dim + d] = acc;
}

inline void launch_project(const uint32_t *counts, uint32_t n, uint32_t m, uint32_t min_cov, const ntsm_x64 *tab, uint32_t dim, double *cloud)
{
	hipLaunchKernelGGL(project_kernel, dim3((n + kThreads - 1) / kThreads, dim), dim3(kThreads), 0, 0, counts, n, m, min_cov, tab, dim, cloud);
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

/* computeScorePCA's selection of pair (i, k) in row i (:315-337 radius rows, :358-365 search-all rows), given evalMetric of
 * the two points: the pair is printed in the row of the larger radius, on equal radii in the row of the lower index */
__device__ inline bool take_with_metric(uint32_t i, uint32_t k, double ri, double rk, double dm)
{
	if (!(ri < DBL_MAX)) return !(DBL_MAX == rk && k <= i);
	if (!(dm < ri)) return false;
	if (ri == rk) return k > i;
	return !(ri < rk);
}

/* the same with the points: a search-all row evaluates no metric (*metric = 0) */
__device__ inline bool take(const double *pi, const double *pk, uint32_t dim, uint32_t i, uint32_t k, double ri, double rk, double *metric)
{
	*metric = ri < DBL_MAX ? eval_metric(pi, pk, dim) : 0.0;
	return take_with_metric(i, k, ri, rk, *metric);
}

/* the single-sample term of every cell of [sample][site][2] rows */
static __global__ __launch_bounds__(kThreads) void term_kernel(const uint32_t *counts, uint64_t cells, uint32_t min_cov, double *term)
{
	const uint64_t cell = (uint64_t) blockIdx.x * kThreads + threadIdx.x;
	if (cell >= cells) return;
	term[cell] = ntsm_eval_term(counts[cell * 2], counts[cell * 2 + 1], min_cov);
}

/* one record per listed pair of rows, row pi as sample 1 */
static __global__ __launch_bounds__(kThreads) void score_kernel(const uint32_t *__restrict__ counts, const double *__restrict__ term, uint32_t m, uint32_t min_cov,
		const uint32_t *__restrict__ pi, const uint32_t *__restrict__ pk, uint64_t n_pairs, ntsm_eval_record *__restrict__ out)
{
	const uint64_t p = (uint64_t) blockIdx.x * kThreads + threadIdx.x;
	if (p >= n_pairs) return;
	const uint32_t *ra = counts + (uint64_t) pi[p] * m * 2, *rb = counts + (uint64_t) pk[p] * m * 2;
	const double *ta = term + (uint64_t) pi[p] * m, *tb = term + (uint64_t) pk[p] * m;
	ntsm_eval_acc acc;
	for (uint32_t site = 0; site < m; ++site)
		acc.add(ntsm_eval_side_of(ra[2 * site], ra[2 * site + 1], ta[site], min_cov),
		        ntsm_eval_side_of(rb[2 * site], rb[2 * site + 1], tb[site], min_cov), min_cov);
	out[p] = acc.record();
}

inline void launch_term(const uint32_t *counts, uint64_t cells, uint32_t min_cov, double *term)
{
	hipLaunchKernelGGL(term_kernel, dim3((unsigned) ((cells + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0, counts, cells, min_cov, term);
}

inline void launch_score(const uint32_t *counts, const double *term, uint32_t m, uint32_t min_cov, const uint32_t *pi, const uint32_t *pk,
		uint64_t n_pairs, ntsm_eval_record *out)
{
	hipLaunchKernelGGL(score_kernel, dim3((unsigned) ((n_pairs + kThreads - 1) / kThreads)), dim3(kThreads), 0, 0, counts, term, m, min_cov, pi, pk, n_pairs, out);
}

/* The host half of a candidate search.  count[i] is the number of pairs of row i, from a counting pass that ran between e0
 * and e1 and is complete.  Prefix sum, *n_pairs, the capacity protocol (NTSM_EVAL_E_CAPACITY with the size reported; nothing
 * further for an empty list), then fill(d_offset, d_k, d_metric, d_dist) launches the caller's filling pass over device
 * arrays allocated here in b -- row i's pairs from d_offset[i] on -- and each row is ordered and written to pi / pk / dist.
 * radius_of(i) < DBL_MAX says that row i is a radius row.  *kernel_ms = count + fill.
 *
 * Order: a radius row by ascending evalMetric (nanoflann sorts its matches), exact ties by ascending k; a search-all row by
 * k.  The session search used to say this as a stable sort by metric alone; its fill writes k ascending within a row, and a
 * stable sort keeps that order among equal metrics, which is what the second key says.  A fill that writes a row in any
 * order (a query row of the search against a store) needs the key, so the total order is the one spelling. */
template <typename Fill, typename RadiusOf>
int finish_candidates(ntsm_hip::Buffers &b, hipEvent_t e0, hipEvent_t e1, const std::vector<uint32_t> &count, Fill fill, RadiusOf radius_of, uint32_t *pi,
		uint32_t *pk, double *dist, uint64_t capacity, uint64_t *n_pairs, double *kernel_ms)
{
	const uint32_t n = (uint32_t) count.size();
	float ms0 = 0, ms1 = 0;
	HIPCHK(hipEventElapsedTime(&ms0, e0, e1));
	std::vector<uint64_t> offset((uint64_t) n + 1, 0);
	for (uint32_t i = 0; i < n; ++i) offset[i + 1] = offset[i] + count[i];
	const uint64_t total = offset[n];
	*n_pairs = total;
	if (kernel_ms) *kernel_ms = ms0;
	if (total > capacity) return NTSM_EVAL_E_CAPACITY;
	if (total == 0) return 0;
	uint64_t *d_offset;
	uint32_t *d_k;
	double *d_metric, *d_dist;
	HIPCHK(b.alloc(&d_offset, (uint64_t) n + 1));
	HIPCHK(b.alloc(&d_k, total));
	HIPCHK(b.alloc(&d_metric, total));
	HIPCHK(b.alloc(&d_dist, total));
	HIPCHK(hipMemcpy(d_offset, offset.data(), ((uint64_t) n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
	HIPCHK(hipEventRecord(e0, 0));
	fill(d_offset, d_k, d_metric, d_dist);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(e1, 0));
	std::vector<uint32_t> k(total);
	std::vector<double> metric(total), dd(total);
	HIPCHK(hipMemcpy(k.data(), d_k, total * sizeof(uint32_t), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(metric.data(), d_metric, total * sizeof(double), hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(dd.data(), d_dist, total * sizeof(double), hipMemcpyDeviceToHost));
	HIPCHK(hipEventElapsedTime(&ms1, e0, e1));
	if (kernel_ms) *kernel_ms = (double) ms0 + ms1;
	std::vector<uint64_t> ord;
	for (uint32_t i = 0; i < n; ++i) {
		const uint64_t lo = offset[i], hi = offset[i + 1];
		ord.resize(hi - lo);
		for (uint64_t p = lo; p < hi; ++p) ord[p - lo] = p;
		const bool by_metric = radius_of(i) < DBL_MAX;
		const auto before = [&](uint64_t x, uint64_t y) {
			if (by_metric && metric[x] != metric[y]) return metric[x] < metric[y];
			return k[x] < k[y];
		};
		if (!std::is_sorted(ord.begin(), ord.end(), before)) std::sort(ord.begin(), ord.end(), before);   /* a search-all row that came in k order is left alone */
		for (uint64_t q = 0; q < ord.size(); ++q) {
			pi[lo + q] = i;
			pk[lo + q] = k[ord[q]];
			dist[lo + q] = dd[ord[q]];
		}
	}
	return 0;
}

}  // namespace ntsm_eval_pca

#endif
