/*
 * ntsm_eval_pca.h -- the steps of the PCA-guided search that its two forms share, each stated once: ntsm_eval_pca.hip (one
 * run's samples against each other) and ntsm_eval_near.hip (new samples against a cohort store).  The projection kernel,
 * the genotype code of a site and the host's product table (src/CompareCounts.hpp:166-211), nanoflann's evalMetric, calcDistance
 * and computeScorePCA's selection of a pair (:285-398), and the scoring of listed pairs over [sample][site][2] rows.
 * Internal: not part of include/.  The kernels have internal linkage.
 */
#ifndef NTSM_EVAL_PCA_H
#define NTSM_EVAL_PCA_H

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cstdint>
#include <vector>

#include "ntsm_eval_score.h"
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

}  // namespace ntsm_eval_pca

#endif
