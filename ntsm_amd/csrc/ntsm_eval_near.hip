/*
 * ntsm_eval_near.hip -- the PCA-guided search of new samples against a cohort store on one MI355X (include/ntsm_eval_hip.h:
 * ntsm_eval_project_store, ntsm_eval_cross_candidates, ntsm_eval_cross_score_pairs; ntsmEval --index / --near; reference:
 * src/CompareCounts.hpp:116-211 projectPCs, :285-398 computeScorePCA).  Indices follow the concatenation [queries; database]:
 * query q is sample q, database sample d is sample n_q + d.
 *
 * Projection of a store.  The store is walked in chunks as ntsm_eval_cross walks it (the chunk rule and the staging step of
 * ntsm_eval_chunk.h, here without the transpose) and each chunk is projected by the session's kernel (ntsm_eval_pca.h:
 * one lane per (sample, component) over the dense rows), so cloud bits are ntsm_eval_project's by construction.  A kernel
 * over the transposed [site][chunk sample] layout of the cross path -- samples across the lanes, coalesced loads, the table
 * entry wave-uniform -- was built and measured first: 134.8 and 141.4 ms against 135.9 and 136.3 ms on 4,096 x 96,287 sites x
 * 20 components.  The chain of integer x87 adds bounds both, not the loads, and the transposed form needs the transpose and
 * three times the device memory per sample on top: a negative result (NOTEBOOK.md), the row form stays.
 *
 * Search.  One pass over the (n_q + n_db) columns k of the concatenation with the columns across the lanes and the queries
 * wave-uniform: for each (query q, column k) evalMetric is formed once (it is symmetric bit for bit: (a - b)^2 = (b - a)^2)
 * and the selection rule of ntsm_eval_pca.h is asked twice, for row q and, where k is a database sample, for row k.  A
 * counting pass, the prefix sum over the rows on the host, a filling pass: a query row is filled through one wave-aggregated
 * atomic per wave and query (its order does not matter: the host sorts), a database row by its own lane, queries ascending.
 * The host half is ntsm_eval_pca.h's finish_candidates: a radius row by (evalMetric, k) and a search-all row by k, which is
 * the session search's order.  The grid is (columns / 256): never one workgroup per database row.  The search between two
 * stores (ntsm_eval_between_candidates; ntsmEval --between-near) is the same two kernels launched over
 * the database columns alone, store A in the queries' place: no pair of two samples of A is ever evaluated.
 *
 * Scoring of listed pairs.  Every pair has a query in it, so it names at most one database sample.  The distinct database
 * samples of the list are copied row by row from the mapped store, at most `chunk` per pass, to dense rows behind the
 * queries' rows; a pass scores its pairs with the listed-pair kernel of ntsm_eval_pca.h over those rows (slot numbers in
 * place of sample numbers) and its records are scattered back to list order.  ntsm_eval_store_score_pairs, at the end of
 * this file, is the same for pairs of two store samples (ntsmEval --within-near); one pass is stated once for both
 * (PairPass), the cut of a list into passes is each caller's own.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/ntsm_eval_hip.h"
#include "host/eval_within.hpp"
#define NTSM_HIP_TAG "ntsm_eval_near"
#include "ntsm_eval_chunk.h"
#include "ntsm_eval_pca.h"
#include "ntsm_eval_score.h"
#include "ntsm_hip_scope.h"
#include "xprec.h"

namespace {

constexpr int kThreads = 256;

using ntsm_eval_chunk::add_interval;
using ntsm_eval_chunk::ms_since;
using ntsm_eval_chunk::wall;

/* the point and radius of column k of the concatenation */
struct Columns {
	const double *q_cloud, *q_radius, *db_cloud, *db_radius;
	uint32_t n_q, n_db, dim;
	__device__ const double *point(uint32_t k) const { return k < n_q ? q_cloud + (uint64_t) k * dim : db_cloud + (uint64_t) (k - n_q) * dim; }
	__device__ double radius(uint32_t k) const { return k < n_q ? q_radius[k] : db_radius[k - n_q]; }
};

/* what rows q and k say about the pair (q, k), q a query, k any column: bit 0 = row q takes k, bit 1 = row k takes q (only
 * asked where k is a database sample: a query's row is asked when that query is the wave-uniform side) */
__device__ inline uint32_t near_decide(const Columns &c, uint32_t q, uint32_t k, double rk, const double *pk, double *metric)
{
	const double rq = c.q_radius[q];
	const double *pq = c.q_cloud + (uint64_t) q * c.dim;
	const bool need = rq < DBL_MAX || (k >= c.n_q && rk < DBL_MAX);            /* a search-all row evaluates no metric */
	const double dm = need ? ntsm_eval_pca::eval_metric(pq, pk, c.dim) : 0.0;
	*metric = dm;
	uint32_t bits = ntsm_eval_pca::take_with_metric(q, k, rq, rk, dm) ? 1u : 0u;
	if (k >= c.n_q && ntsm_eval_pca::take_with_metric(k, q, rk, rq, dm)) bits |= 2u;
	return bits;
}

/* Both passes walk the columns from k_first on: 0 for the whole concatenation, n_q for the database columns alone.
 * pass 1: q_count[q] += the pairs of row q among this workgroup's columns; db_count[d] = the pairs of row n_q + d */
__global__ __launch_bounds__(kThreads) void near_count_kernel(Columns c, uint32_t k_first, uint32_t *__restrict__ q_count, uint32_t *__restrict__ db_count)
{
	const uint32_t n = c.n_q + c.n_db, k = k_first + blockIdx.x * kThreads + threadIdx.x;
	const bool live = k < n;
	const uint32_t kc = live ? k : n - 1;
	const double rk = c.radius(kc);
	const double *pk = c.point(kc);
	uint32_t own = 0;
	for (uint32_t q = 0; q < c.n_q; ++q) {
		double dm;
		const uint32_t bits = live ? near_decide(c, q, kc, rk, pk, &dm) : 0u;
		const uint64_t ballot = __ballot(bits & 1u);
		if ((threadIdx.x & 63) == 0 && ballot) atomicAdd(&q_count[q], (uint32_t) __popcll(ballot));
		own += bits >> 1;
	}
	if (live && k >= c.n_q) db_count[k - c.n_q] = own;
}

/* pass 2: row q's pairs from q_offset[q] on through q_cursor[q] (any order), row n_q + d's at db_offset[d], queries ascending */
__global__ __launch_bounds__(kThreads) void near_fill_kernel(Columns c, uint32_t k_first, const uint64_t *__restrict__ q_offset, uint32_t *__restrict__ q_cursor,
		const uint64_t *__restrict__ db_offset, uint32_t *__restrict__ other, double *__restrict__ metric, double *__restrict__ dist)
{
	const uint32_t n = c.n_q + c.n_db, k = k_first + blockIdx.x * kThreads + threadIdx.x, lane = threadIdx.x & 63;
	const bool live = k < n;
	const uint32_t kc = live ? k : n - 1;
	const double rk = c.radius(kc);
	const double *pk = c.point(kc);
	uint64_t own = (live && k >= c.n_q) ? db_offset[k - c.n_q] : 0;
	for (uint32_t q = 0; q < c.n_q; ++q) {
		double dm = 0.0;
		const uint32_t bits = live ? near_decide(c, q, kc, rk, pk, &dm) : 0u;
		const uint64_t ballot = __ballot(bits & 1u);
		uint32_t base = 0;
		if (lane == 0 && ballot) base = atomicAdd(&q_cursor[q], (uint32_t) __popcll(ballot));
		base = __shfl(base, 0, 64);
		if (bits) {
			const double dd = ntsm_eval_pca::calc_distance(c.q_cloud + (uint64_t) q * c.dim, pk, c.dim);
			if (bits & 1u) {
				const uint64_t p = q_offset[q] + base + (uint32_t) __popcll(ballot & ((1ull << lane) - 1));
				other[p] = k; metric[p] = dm; dist[p] = dd;
			}
			if (bits & 2u) { other[own] = q; metric[own] = dm; dist[own] = dd; ++own; }
		}
	}
}

/* One pass of a list scorer: dense rows [slot][site][2] with their terms, the pass's pairs as slot numbers, its records. */
struct PairPass {
	ntsm_hip::Buffers b;
	ntsm_hip::Events<3> ev;
	uint32_t *d_rows, *d_pi, *d_pk;
	double *d_term;
	ntsm_eval_record *d_out;
	uint32_t n_sites, min_cov;

	/* room for `slots` rows and passes of at most `most` pairs */
	int alloc(uint64_t slots, uint64_t most, uint32_t sites, uint32_t cov)
	{
		n_sites = sites;
		min_cov = cov;
		HIPCHK(b.alloc(&d_rows, slots * n_sites * 2));
		HIPCHK(b.alloc(&d_term, slots * n_sites));
		HIPCHK(b.alloc(&d_pi, most));
		HIPCHK(b.alloc(&d_pk, most));
		HIPCHK(b.alloc(&d_out, most));
		HIPCHK(ev.create());
		return 0;
	}

	/* Store samples sample[0 ... rn - 1] go to slots slot0 ... (row by row from the mapped store) and get their terms; the pn
	 * pairs (slot_i[x], slot_k[x]) are scored into out[0 ... pn - 1]; one wait, after the scoring kernel; timed into tm (added) */
	int run(const void *db_counts, uint64_t db_stride_bytes, uint32_t slot0, const uint32_t *sample, uint32_t rn, const uint32_t *slot_i,
			const uint32_t *slot_k, uint64_t pn, ntsm_eval_record *out, ntsm_eval_cross_times &tm)
	{
		const uint64_t first = (uint64_t) slot0 * n_sites;
		auto t = wall::now();
		for (uint32_t r = 0; r < rn; ++r)
			HIPCHK(hipMemcpy(d_rows + (first + (uint64_t) r * n_sites) * 2, (const char *) db_counts + (uint64_t) sample[r] * db_stride_bytes, 8ull * n_sites,
					hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(d_pi, slot_i, pn * sizeof(uint32_t), hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(d_pk, slot_k, pn * sizeof(uint32_t), hipMemcpyHostToDevice));
		tm.upload_ms += ms_since(t);
		HIPCHK(hipEventRecord(ev[0], 0));
		if (rn) {
			ntsm_eval_pca::launch_term(d_rows + first * 2, (uint64_t) rn * n_sites, min_cov, d_term + first);
			HIPCHK(hipGetLastError());
		}
		HIPCHK(hipEventRecord(ev[1], 0));
		ntsm_eval_pca::launch_score(d_rows, d_term, n_sites, min_cov, d_pi, d_pk, pn, d_out);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(ev[2], 0));
		HIPCHK(hipEventSynchronize(ev[2]));
		int rc = add_interval(ev[0], ev[1], &tm.prepare_kernel_ms);
		if (!rc) rc = add_interval(ev[1], ev[2], &tm.cross_kernel_ms);
		if (rc) return rc;
		t = wall::now();
		HIPCHK(hipMemcpy(out, d_out, pn * sizeof(ntsm_eval_record), hipMemcpyDeviceToHost));
		tm.download_ms += ms_since(t);
		tm.chunks++;
		return 0;
	}
};

}  // namespace

extern "C" int ntsm_eval_project_store(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n_db, uint32_t n_sites, uint32_t min_cov,
		const long double *norm, const long double *rot, uint32_t dim, uint32_t db_chunk, double *cloud, uint32_t *db_geno,
		ntsm_eval_cross_times *times)
{
	if (times) *times = ntsm_eval_cross_times {};
	if (!ntsm_eval_chunk::valid_store(db_counts, db_stride_bytes, n_db, n_sites) || (n_sites && (!norm || (dim && !rot))) || (!cloud && n_db && dim)) return -1;
	if (n_db && dim) memset(cloud, 0, (size_t) n_db * dim * sizeof(double));     /* no site: inner_product of nothing */
	if (db_geno && n_db) memset(db_geno, 0, (size_t) n_db * 3 * sizeof(uint32_t));
	if (n_db == 0 || n_sites == 0) return 0;

	const std::vector<ntsm_x64> tab = ntsm_eval_pca::product_table(norm, rot, n_sites, dim);
	const uint64_t row_bytes = 8ull * n_sites;
	HIPCHK(hipSetDevice(device));
	size_t free_b = 0, total_b = 0;
	if (db_chunk == 0) HIPCHK(hipMemGetInfo(&free_b, &total_b));
	const uint32_t chunk = ntsm_eval_chunk::samples_per_pass(db_chunk, n_db, free_b, row_bytes + 8ull * dim + 12, tab.size() * sizeof(ntsm_x64));

	ntsm_hip::Buffers b;
	ntsm_hip::Events<3> ev;
	uint32_t *d_raw, *d_geno;
	double *d_cloud;
	ntsm_x64 *d_tab;
	HIPCHK(b.alloc(&d_raw, (uint64_t) chunk * n_sites * 2));
	HIPCHK(b.alloc(&d_geno, (uint64_t) chunk * 3));
	HIPCHK(b.alloc(&d_cloud, (uint64_t) chunk * dim));
	HIPCHK(b.alloc(&d_tab, tab.size()));
	HIPCHK(ev.create());
	ntsm_eval_cross_times tm {};
	auto t = wall::now();
	HIPCHK(hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(ntsm_x64), hipMemcpyHostToDevice));
	tm.upload_ms += ms_since(t);

	for (uint32_t c0 = 0; c0 < n_db; c0 += chunk) {
		const uint32_t cn = std::min(chunk, n_db - c0);
		int rc = ntsm_eval_chunk::stage(db_counts, db_stride_bytes, c0, cn, n_sites, min_cov, d_raw, nullptr, nullptr, nullptr, db_geno ? d_geno : nullptr,
				ev[0], ev[1], tm);
		if (rc) return rc;
		if (dim) {
			ntsm_eval_pca::launch_project(d_raw, cn, n_sites, min_cov, d_tab, dim, d_cloud);
			HIPCHK(hipGetLastError());
		}
		HIPCHK(hipEventRecord(ev[2], 0));
		HIPCHK(hipEventSynchronize(ev[2]));
		t = wall::now();
		if (dim) HIPCHK(hipMemcpy(cloud + (uint64_t) c0 * dim, d_cloud, (size_t) cn * dim * sizeof(double), hipMemcpyDeviceToHost));
		if (db_geno) HIPCHK(hipMemcpy(db_geno + (uint64_t) c0 * 3, d_geno, (size_t) cn * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
		tm.download_ms += ms_since(t);
		if ((rc = add_interval(ev[0], ev[1], &tm.prepare_kernel_ms)) != 0) return rc;
		if ((rc = add_interval(ev[1], ev[2], &tm.cross_kernel_ms)) != 0) return rc;
		tm.chunks++;
	}
	if (times) *times = tm;
	return 0;
}

namespace {

/* The search of both entry points below.  `rectangle`: only the database columns are walked, so a pair is listed exactly
 * when one of its samples is a query and the other a database sample; otherwise all columns, query-query pairs included. */
int search_columns(int device, const double *q_cloud, const double *q_radius, uint32_t n_q, const double *db_cloud, const double *db_radius, uint32_t n_db,
		uint32_t dim, bool rectangle, uint32_t *pi, uint32_t *pk, double *dist, uint64_t capacity, uint64_t *n_pairs, double *kernel_ms)
{
	if (kernel_ms) *kernel_ms = 0;
	if (!n_pairs || (n_q && (!q_radius || (dim && !q_cloud))) || (n_db && (!db_radius || (dim && !db_cloud))) || (capacity && (!pi || !pk || !dist)))
		return -1;
	*n_pairs = 0;
	const uint64_t n64 = (uint64_t) n_q + n_db;
	if (n64 > UINT32_MAX) return -1;
	const uint32_t n = (uint32_t) n64;
	if (n_q == 0 || n < 2 || (rectangle && n_db == 0)) return 0;                 /* no query: no pair has one; no database sample: nor has the rectangle */
	HIPCHK(hipSetDevice(device));
	ntsm_hip::Buffers b;
	double *d_qc, *d_qr, *d_dc, *d_dr;
	uint32_t *d_qcount, *d_dcount;                                               /* d_qcount: the queries' counts, then their rows' cursors */
	HIPCHK(b.alloc(&d_qc, (uint64_t) n_q * dim));
	HIPCHK(b.alloc(&d_qr, n_q));
	HIPCHK(b.alloc(&d_dc, (uint64_t) n_db * dim));
	HIPCHK(b.alloc(&d_dr, n_db));
	HIPCHK(b.alloc(&d_qcount, 2ull * n_q));
	HIPCHK(b.alloc(&d_dcount, n_db));
	if (dim) HIPCHK(hipMemcpy(d_qc, q_cloud, (uint64_t) n_q * dim * sizeof(double), hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(d_qr, q_radius, n_q * sizeof(double), hipMemcpyHostToDevice));
	if (dim && n_db) HIPCHK(hipMemcpy(d_dc, db_cloud, (uint64_t) n_db * dim * sizeof(double), hipMemcpyHostToDevice));
	if (n_db) HIPCHK(hipMemcpy(d_dr, db_radius, (uint64_t) n_db * sizeof(double), hipMemcpyHostToDevice));
	HIPCHK(hipMemset(d_qcount, 0, 2ull * n_q * sizeof(uint32_t)));
	const Columns cols { d_qc, d_qr, d_dc, d_dr, n_q, n_db, dim };
	const uint32_t k_first = rectangle ? n_q : 0;
	const dim3 grid((n - k_first + kThreads - 1) / kThreads);
	ntsm_hip::Events<2> ev;
	HIPCHK(ev.create());
	HIPCHK(hipEventRecord(ev[0], 0));
	hipLaunchKernelGGL(near_count_kernel, grid, dim3(kThreads), 0, 0, cols, k_first, d_qcount, d_dcount);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(ev[1], 0));
	std::vector<uint32_t> count(n, 0);
	HIPCHK(hipMemcpy(count.data(), d_qcount, n_q * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (n_db) HIPCHK(hipMemcpy(count.data() + n_q, d_dcount, (uint64_t) n_db * sizeof(uint32_t), hipMemcpyDeviceToHost));
	return ntsm_eval_pca::finish_candidates(b, ev[0], ev[1], count,
			[&](const uint64_t *d_offset, uint32_t *d_k, double *d_metric, double *d_dist) {
				hipLaunchKernelGGL(near_fill_kernel, grid, dim3(kThreads), 0, 0, cols, k_first, d_offset, d_qcount + n_q, d_offset + n_q, d_k, d_metric, d_dist);
			},
			[&](uint32_t i) { return i < n_q ? q_radius[i] : db_radius[i - n_q]; }, pi, pk, dist, capacity, n_pairs, kernel_ms);
}

}  // namespace

extern "C" int ntsm_eval_cross_candidates(int device, const double *q_cloud, const double *q_radius, uint32_t n_q, const double *db_cloud,
		const double *db_radius, uint32_t n_db, uint32_t dim, uint32_t *pi, uint32_t *pk, double *dist, uint64_t capacity, uint64_t *n_pairs,
		double *kernel_ms)
{
	return search_columns(device, q_cloud, q_radius, n_q, db_cloud, db_radius, n_db, dim, false, pi, pk, dist, capacity, n_pairs, kernel_ms);
}

/* The search between two stores (ntsmEval --between-near): store A's samples are the wave-uniform side, store B's run across
 * the lanes, and the columns of A are never walked -- their (n_a)^2 / 2 metric evaluations would all be thrown away. */
extern "C" int ntsm_eval_between_candidates(int device, const double *a_cloud, const double *a_radius, uint32_t n_a, const double *b_cloud,
		const double *b_radius, uint32_t n_b, uint32_t dim, uint32_t *pi, uint32_t *pk, double *dist, uint64_t capacity, uint64_t *n_pairs,
		double *kernel_ms)
{
	return search_columns(device, a_cloud, a_radius, n_a, b_cloud, b_radius, n_b, dim, true, pi, pk, dist, capacity, n_pairs, kernel_ms);
}

extern "C" int ntsm_eval_cross_score_pairs(int device, const uint32_t *q_counts, uint32_t n_q, const void *db_counts, uint64_t db_stride_bytes,
		uint32_t n_db, uint32_t n_sites, uint32_t min_cov, const uint32_t *pi, const uint32_t *pk, uint64_t n_pairs, uint32_t db_chunk,
		ntsm_eval_record *out, ntsm_eval_cross_times *times)
{
	if (times) *times = ntsm_eval_cross_times {};
	if ((!q_counts && n_q && n_sites) || !ntsm_eval_chunk::valid_store(db_counts, db_stride_bytes, n_db, n_sites) || (n_pairs && (!pi || !pk || !out))) return -1;
	const uint64_t n = (uint64_t) n_q + n_db;
	if (n > UINT32_MAX) return -1;
	for (uint64_t p = 0; p < n_pairs; ++p)
		if (pi[p] >= n || pk[p] >= n || pi[p] == pk[p] || (pi[p] >= n_q && pk[p] >= n_q)) return -1;
	if (n_pairs == 0) return 0;
	memset(out, 0, n_pairs * sizeof(ntsm_eval_record));
	if (n_sites == 0) return 0;

	/* the distinct database samples of the list, ascending (the store is read front to back), and each pair's */
	std::vector<uint32_t> named;
	for (uint64_t p = 0; p < n_pairs; ++p) {
		if (pi[p] >= n_q) named.push_back(pi[p] - n_q);
		if (pk[p] >= n_q) named.push_back(pk[p] - n_q);
	}
	std::sort(named.begin(), named.end());
	named.erase(std::unique(named.begin(), named.end()), named.end());
	const uint64_t row_bytes = 8ull * n_sites;
	HIPCHK(hipSetDevice(device));
	size_t free_b = 0, total_b = 0;
	if (db_chunk == 0) HIPCHK(hipMemGetInfo(&free_b, &total_b));
	const uint32_t n_named = (uint32_t) named.size();
	const uint32_t chunk = std::max(1u, ntsm_eval_chunk::samples_per_pass(db_chunk, n_named, free_b, 2 * row_bytes,
			2ull * n_q * row_bytes + n_pairs * (sizeof(ntsm_eval_record) + 8)));
	const uint32_t passes = std::max(1u, (n_named + chunk - 1) / chunk);         /* a list of query-query pairs still takes one */
	/* pairs grouped by pass: a pair without a database sample goes with the first */
	std::vector<std::vector<uint64_t>> of_pass(passes);
	const auto rank = [&](uint32_t s) { return (uint32_t) (std::lower_bound(named.begin(), named.end(), s - n_q) - named.begin()); };
	for (uint64_t p = 0; p < n_pairs; ++p) {
		const uint32_t s = pi[p] >= n_q ? pi[p] : pk[p];
		of_pass[s >= n_q ? rank(s) / chunk : 0].push_back(p);
	}
	uint64_t most = 0;
	for (const auto &v : of_pass) most = std::max<uint64_t>(most, v.size());

	PairPass d;
	const uint64_t qcells = (uint64_t) n_q * n_sites;
	int rc = d.alloc((uint64_t) n_q + chunk, most, n_sites, min_cov);
	if (rc) return rc;
	ntsm_eval_cross_times tm {};
	auto t = wall::now();
	if (qcells) HIPCHK(hipMemcpy(d.d_rows, q_counts, qcells * 2 * sizeof(uint32_t), hipMemcpyHostToDevice));
	tm.upload_ms += ms_since(t);
	if (qcells) {                                                                /* the queries' terms: once, in front of the passes */
		HIPCHK(hipEventRecord(d.ev[0], 0));
		ntsm_eval_pca::launch_term(d.d_rows, qcells, min_cov, d.d_term);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(d.ev[1], 0));
		HIPCHK(hipEventSynchronize(d.ev[1]));
		if ((rc = add_interval(d.ev[0], d.ev[1], &tm.prepare_kernel_ms)) != 0) return rc;
	}
	std::vector<uint32_t> a, c;
	std::vector<ntsm_eval_record> rec;
	for (uint32_t pass = 0; pass < passes; ++pass) {
		const std::vector<uint64_t> &list = of_pass[pass];
		if (list.empty()) continue;
		const uint32_t r0 = pass * chunk, rn = r0 < n_named ? std::min(chunk, n_named - r0) : 0;
		a.resize(list.size());
		c.resize(list.size());
		rec.resize(list.size());
		const auto slot = [&](uint32_t s) { return s < n_q ? s : n_q + rank(s) - r0; };
		for (uint64_t x = 0; x < list.size(); ++x) { a[x] = slot(pi[list[x]]); c[x] = slot(pk[list[x]]); }
		if ((rc = d.run(db_counts, db_stride_bytes, n_q, named.data() + r0, rn, a.data(), c.data(), list.size(), rec.data(), tm)) != 0) return rc;
		t = wall::now();
		for (uint64_t x = 0; x < list.size(); ++x) out[list[x]] = rec[x];        /* back to list order */
		tm.download_ms += ms_since(t);
	}
	if (times) *times = tm;
	return 0;
}

/* Listed pairs of two store samples (ntsmEval --within-near): the scheme above with the query block removed.  Both samples of
 * a pair have to be on the device at once, so the passes are eval_within.hpp's cut of the list -- contiguous pieces of it,
 * each over at most `chunk` distinct samples -- and a pass's records go back to the list as one copy. */
extern "C" int ntsm_eval_store_score_pairs(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n_db, uint32_t n_sites,
		uint32_t min_cov, const uint32_t *pi, const uint32_t *pk, uint64_t n_pairs, uint32_t db_chunk,
		ntsm_eval_record *out, ntsm_eval_cross_times *times)
{
	if (times) *times = ntsm_eval_cross_times {};
	if (!ntsm_eval_chunk::valid_store(db_counts, db_stride_bytes, n_db, n_sites) || (n_pairs && (!pi || !pk || !out)) || db_chunk == 1) return -1;
	for (uint64_t p = 0; p < n_pairs; ++p)
		if (pi[p] >= n_db || pk[p] >= n_db || pi[p] == pk[p]) return -1;
	if (n_pairs == 0) return 0;
	memset(out, 0, n_pairs * sizeof(ntsm_eval_record));
	if (n_sites == 0) return 0;

	const uint64_t row_bytes = 8ull * n_sites;
	HIPCHK(hipSetDevice(device));
	size_t free_b = 0, total_b = 0;
	if (db_chunk == 0) HIPCHK(hipMemGetInfo(&free_b, &total_b));
	const uint32_t chunk = std::max(2u, ntsm_eval_chunk::samples_per_pass(db_chunk, n_db, free_b, 2 * row_bytes, n_pairs * (sizeof(ntsm_eval_record) + 8)));
	const ntsm::eval_within::Passes cut = ntsm::eval_within::pack_passes(pi, pk, n_pairs, n_db, chunk);
	uint64_t most = 0;
	uint32_t slots = 0;
	for (size_t x = 0; x < cut.passes(); ++x) {
		most = std::max(most, cut.pair_begin[x + 1] - cut.pair_begin[x]);
		slots = std::max(slots, (uint32_t) (cut.sample_begin[x + 1] - cut.sample_begin[x]));
	}

	PairPass d;
	int rc = d.alloc(slots, most, n_sites, min_cov);
	ntsm_eval_cross_times tm {};
	for (size_t x = 0; x < cut.passes() && !rc; ++x) {
		const uint64_t p0 = cut.pair_begin[x], s0 = cut.sample_begin[x];
		rc = d.run(db_counts, db_stride_bytes, 0, cut.sample.data() + s0, (uint32_t) (cut.sample_begin[x + 1] - s0), cut.slot_i.data() + p0,
				cut.slot_k.data() + p0, cut.pair_begin[x + 1] - p0, out + p0, tm);
	}
	if (rc) return rc;
	if (times) *times = tm;
	return 0;
}
