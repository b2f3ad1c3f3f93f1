/*
 * include/ntsm_eval_hip.h -- C ABI of the MI355X (gfx950) all-pairs scoring of ntsmEval.
 *
 * The reference (src/CompareCounts.hpp) scores every pair of samples by walking all sites three times per pair:
 *   gatherValidEntries(i, j)                       :1057-1078   sites where both samples have an allele above min_cov
 *   computeLogLikelihood(i, j, valid)              :1093-1099   -2 * (joint - (single_i + single_j)),
 *     computeSumLogPJoint / computeSumLogPSingle   :1013-1033, :968-989   three sequential double sums over the valid sites
 *   calcRelatedness(i, j, valid)                   :1144-1196   genotype tallies (het / hom / shared / ibs0 / ibs2)
 * inside  for i: for j > i  (computeScore, :591-624, an OpenMP loop over i).  This library replaces exactly those calls:
 * one launch returns, for every pair, the three sums, the number of valid sites and the eight tallies; the caller forms
 * score = skew(-2 * (joint - (single1 + single2)), cov1, cov2) / n_valid  (:611-615, :1081-1083), relatedness and
 * homConcord (:1190-1194) and prints (resultsStr, :843-905) -- ntsm_amd/csrc/host/ntsm_eval_main.cpp does.
 * The sums are accumulated in site order with IEEE double operations and no contraction, i.e. bit for bit what one
 * thread of the reference computes.  Pinned to the reference itself: the CLI's stdout equals, byte for byte, that of
 * oracle/_ref/ref_ntsmEval -- the unmodified src/CompareCounts.hpp behind oracle/ref_eval_driver.cpp -- and its recordings
 * under tests/golden/eval/ (tests/test_eval_reference.py).
 */
#ifndef NTSM_EVAL_HIP_H
#define NTSM_EVAL_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ntsm_eval_record {        /* one pair (i < j); 64 bytes */
	double sum_joint, sum_single1, sum_single2;
	uint64_t n_valid;
	uint32_t hets1, homs1, hets2, homs2, shared_hets, shared_homs, ibs0, ibs2;
} ntsm_eval_record;

/* index of pair (i, j), i < j < n, in the output: rows i in order, j ascending inside a row (the reference's loop order) */
static inline uint64_t ntsm_eval_pair_index(uint32_t i, uint32_t j, uint32_t n)
{
	return (uint64_t) i * n - (uint64_t) i * (i + 1) / 2 + (j - i - 1);
}

/* counts: host array [n_samples][n_sites][2] = m_counts (countAT, countCG per site, src/CompareCounts.hpp:99-101).
 * out: host array of n_samples * (n_samples - 1) / 2 records.  kernel_ms (may be NULL): duration of the pair kernel
 * from HIP events.  Returns 0, -1 bad argument, -2 HIP error. */
int ntsm_eval_pairs(int device, const uint32_t *counts, uint32_t n_samples, uint32_t n_sites, uint32_t min_cov,
		ntsm_eval_record *out, double *kernel_ms);

/* ---- PCA-guided pair search (the reference's -p / -n mode: CompareCounts::projectPCs, :116-211, and computeScorePCA,
 * :285-398), in ntsm_amd/csrc/ntsm_eval_pca.hip.  A session holds one run's counts on the device; the caller loads the
 * files, forms the summaries and radii and prints (ntsm_amd/csrc/host/ntsm_eval_main.cpp).
 *
 * ntsm_eval_project: m_cloud[i][d] = inner_product(vals_i, rot[d], 0.0) (:166-211), bit for bit: per site
 *   cAT = countAT > min_cov ? countAT : 0 (cCG alike); a site with cAT + cCG == 0 gives v = +0.0 (not centred), else
 *   g = double(cAT) / double(cAT + cCG), c = g < 0.25 ? 0 : g < 0.75 ? 0.5 : 1, v = double(c - norm[j]) (x87 subtraction);
 *   each step acc = RN53(RN64(acc + RN64(v * rot[d][j]))), sites in order from +0.0 (x87 products and sums, a double
 *   accumulator).  The library's host code forms the products with real long double (a [site][dim][4] table: c = 0, 1/2,
 *   1 and the missing site's +0.0 * rot) and the device runs the sequential x87 add in integers (ntsm_amd/csrc/xprec.h),
 *   one lane per (sample, component).  An accumulator that has overflowed stays where it is, as on the x87: from acc = +-inf
 *   on, every finite product leaves it unchanged (inf +- finite = inf), so a component prints inf where the reference does.
 *   Outside the promise: a table entry that is itself infinite or NaN (RN64(v * rot) beyond the x87 range, or rot not
 *   finite), which the table has no encoding for, and a centre value with |norm[j]| beyond DBL_MAX.
 *
 * ntsm_eval_candidates: the pairs that computeScorePCA scores (:311-398), in its one-thread print order.  Rows i
 * ascending; a row with radius[i] < DBL_MAX takes every k with evalMetric(cloud[i], cloud[k]) < radius[i] (nanoflann's
 * L2_Adaptor, vendor/nanoflann.hpp:452-486: groups of four as result += ((d0^2 + d1^2) + d2^2) + d3^2, then the last 0-3
 * terms one by one; RadiusResultSet keeps dist < radius, :305-307), skips k when radius[k] == radius[i] and k <= i, or
 * when radius[i] < radius[k], and orders the row by ascending evalMetric (the reference sorts the matches); a row with
 * radius DBL_MAX ("search all") takes every k ascending except k <= i of radius DBL_MAX.  dist[p] is calcDistance (:926-932,
 * a sequential sum of squared differences: a different rounding order from evalMetric).  The search is brute force over
 * all N^2 pairs in IEEE double without contraction.  Two deviations from the kd-tree, both intended: (1) ties in evalMetric
 * are ordered by ascending k (the reference's order among exact ties is that of its kd-tree leaves); (2) nanoflann prunes
 * nodes with an incrementally rounded bound, which could in principle drop a point one ulp inside the radius; brute force
 * keeps it.
 *
 * ntsm_eval_score_pairs: for each (pi[p], pk[p]), any order (pi > pk included), the record ntsm_eval_pairs gives for that
 * pair with sample pi[p] as sample 1, i.e. bit-identical to ntsm_eval_pairs' record of (min, max) with the 1 / 2 fields
 * swapped when pi[p] > pk[p].  Device memory is O(samples * sites + pairs), never O(samples^2). */
typedef struct ntsm_eval_session ntsm_eval_session;

#define NTSM_EVAL_E_CAPACITY (-3)   /* ntsm_eval_candidates: the caller's buffers are too small; *n_pairs = the size needed */

/* counts: host [n_samples][n_sites][2] (as for ntsm_eval_pairs), uploaded once.  Returns 0, -1 bad argument, -2 HIP error. */
int ntsm_eval_open(int device, const uint32_t *counts, uint32_t n_samples, uint32_t n_sites, uint32_t min_cov, ntsm_eval_session **h);
void ntsm_eval_close(ntsm_eval_session *h);
/* norm: [n_sites], rot: [dim][n_sites] (the first dim components), cloud: out [n_samples][dim].  kernel_ms (may be NULL):
 * HIP-event time of the projection kernel.  Returns 0, -1, -2. */
int ntsm_eval_project(ntsm_eval_session *h, const long double *norm, const long double *rot, uint32_t dim, double *cloud,
		double *kernel_ms);
/* cloud: [n_samples][dim], radius: [n_samples] (squared radii, DBL_MAX = search all).  Writes up to capacity pairs to
 * pi / pk / dist (any may be NULL when capacity is 0) and their number to *n_pairs.  kernel_ms: the two search kernels.
 * Returns 0, -1, -2, or NTSM_EVAL_E_CAPACITY with *n_pairs = the number of pairs (nothing written). */
int ntsm_eval_candidates(ntsm_eval_session *h, const double *cloud, uint32_t dim, const double *radius, uint32_t *pi, uint32_t *pk,
		double *dist, uint64_t capacity, uint64_t *n_pairs, double *kernel_ms);
/* out: [n_pairs] records.  kernel_ms: the scoring kernel.  Returns 0, -1 (an index out of range, or pi[p] == pk[p]), -2. */
int ntsm_eval_score_pairs(ntsm_eval_session *h, const uint32_t *pi, const uint32_t *pk, uint64_t n_pairs, ntsm_eval_record *out,
		double *kernel_ms);

/* ---- Queries against a cohort (ntsmEval --against STORE; ntsm_amd/csrc/ntsm_eval_cross.hip): the n_q x n_db rectangle of
 * pairs (query, database sample), tiled like the all-pairs kernel -- database samples across the lanes, a group of queries
 * wave-uniform -- with the database walked in chunks, so a cohort store mapped from disk (ntsm_amd/csrc/host/eval_store.hpp)
 * is passed as it lies and never has to fit on the device at once.  The arithmetic is ntsm_eval_score.h's. */
typedef struct ntsm_eval_cross_times {   /* milliseconds */
	double upload_ms, prepare_kernel_ms, cross_kernel_ms, download_ms;   /* summed over the chunks; prepare includes the tallies */
	uint32_t chunks;
} ntsm_eval_cross_times;

/* q_counts: host [n_q][n_sites][2].
 * db_counts: host; sample d at (const char *) db_counts + d * db_stride_bytes, [n_sites][2] each.
 *   db_stride_bytes >= 8 * n_sites and a multiple of 4, so a mapped store is passed as it lies.
 * db_chunk: database samples per pass; 0 = the library's choice (as many as fit in half of the device's free memory).
 *   Device memory is O((n_q + chunk) * n_sites + n_q * chunk), never O(n_db * n_sites).
 * out: [n_q][n_db].  out[q * n_db + d] is, bit for bit, the record ntsm_eval_pairs gives for pair (q, n_q + d)
 *   of the concatenation [queries; database] -- the query is sample 1.
 * db_geno (may be NULL): [n_db][3] = hets, homs, miss of each database sample at min_cov (calcHomHetMiss, :742-767).
 * times (may be NULL).
 * Returns 0, -1 bad argument, -2 HIP error.  n_q == 0, n_db == 0 or n_sites == 0: zeroed outputs, no device work. */
int ntsm_eval_cross(int device, const uint32_t *q_counts, uint32_t n_q, const void *db_counts, uint64_t db_stride_bytes,
		uint32_t n_db, uint32_t n_sites, uint32_t min_cov, uint32_t db_chunk,
		ntsm_eval_record *out, uint32_t *db_geno, ntsm_eval_cross_times *times);

/* For measurements only (tools/eval_store_bench.py): force the cross kernel's workgroup width (64 or 256) and query group
 * size (1, 2 or 4) of later calls in this process; 0 = the library's rule.  Returns 0, -1 for another value. */
int ntsm_eval_cross_tune(uint32_t width, uint32_t query_group);

/* ---- The PCA-guided search of new samples against a cohort store (ntsmEval --index / --near; ntsm_amd/csrc/ntsm_eval_near.hip;
 * DESIGN.md section 9.2): projectPCs (src/CompareCounts.hpp:116-211) over a mapped store, computeScorePCA's pairs (:285-398)
 * that have a query in them, and their records.  Indices follow the concatenation [queries; database] throughout: query q is
 * sample q, database sample d is sample n_q + d.  ntsm_eval_cross_times is reused: cross_kernel_ms is the projection or
 * scoring kernel, prepare_kernel_ms the tallies or the terms, upload_ms includes the row copies.
 *
 * ntsm_eval_project_store: db_counts / db_stride_bytes / db_chunk as for ntsm_eval_cross (one 2-D copy per chunk, no
 *   host-side gather); norm [n_sites], rot [dim][n_sites] as for ntsm_eval_project.
 *   cloud: out [n_db][dim], bit for bit what ntsm_eval_project gives on a dense copy of the same samples (:166-211).
 *   db_geno (may be NULL): [n_db][3] as ntsm_eval_cross's (calcHomHetMiss, :742-767).
 *   Returns 0, -1 bad argument, -2 HIP error.  n_db == 0 or n_sites == 0: zeroed outputs, no device work. */
int ntsm_eval_project_store(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n_db, uint32_t n_sites, uint32_t min_cov,
		const long double *norm, const long double *rot, uint32_t dim, uint32_t db_chunk, double *cloud, uint32_t *db_geno,
		ntsm_eval_cross_times *times);

/* ntsm_eval_cross_candidates: exactly the sublist of ntsm_eval_candidates' output on the concatenated clouds and radii in
 *   which pi < n_q or pk < n_q -- order, indices and dist (calcDistance, :926-932) the same, query-query pairs included.  A
 *   pair (q, d) stands in the row of d when radius[d] > radius[q], else in the row of q (:318-334); rows ascending, queries
 *   first; a radius row by ascending evalMetric (vendor/nanoflann.hpp:452-486), ties by ascending k; a search-all row by k.
 *   q_cloud [n_q][dim], db_cloud [n_db][dim], radii squared, DBL_MAX = search all.  One pass over the rectangle, database
 *   samples across the lanes.  Capacity protocol and return codes as ntsm_eval_candidates. */
int ntsm_eval_cross_candidates(int device, const double *q_cloud, const double *q_radius, uint32_t n_q, const double *db_cloud,
		const double *db_radius, uint32_t n_db, uint32_t dim, uint32_t *pi, uint32_t *pk, double *dist, uint64_t capacity, uint64_t *n_pairs,
		double *kernel_ms);

/* ntsm_eval_cross_score_pairs: out[p] is, bit for bit, the record ntsm_eval_score_pairs gives for (pi[p], pk[p]) on the
 *   concatenation (sample pi[p] as sample 1; either orientation).  Only the distinct database samples the list names leave
 *   the host: copied row by row from db_counts in passes of at most db_chunk distinct samples (0 = the library's choice from
 *   free memory); device memory is O((n_q + chunk) * n_sites + n_pairs).
 *   Returns 0, -1 (a bad argument, an index out of range, pi[p] == pk[p], or a pair with no query in it), -2. */
int ntsm_eval_cross_score_pairs(int device, const uint32_t *q_counts, uint32_t n_q, const void *db_counts, uint64_t db_stride_bytes,
		uint32_t n_db, uint32_t n_sites, uint32_t min_cov, const uint32_t *pi, const uint32_t *pk, uint64_t n_pairs, uint32_t db_chunk,
		ntsm_eval_record *out, ntsm_eval_cross_times *times);

/* ---- The pairs inside a cohort store (ntsmEval --within / --within-near; ntsm_amd/csrc/ntsm_eval_within.hip and
 * ntsm_eval_near.hip): computeScore's triangle (src/CompareCounts.hpp:591-624) over a mapped store, in
 * bands of rows, and the records of listed pairs that name two store samples.  db_counts / db_stride_bytes / db_chunk as for
 * ntsm_eval_cross; the mapping must outlive the session.
 *
 * ntsm_eval_within_open: the store is resident when the chunk rule, asked at 24 bytes per sample and site (what
 *   ntsm_eval_pairs holds), answers n_db: it is uploaded, transposed and tallied once, here.  Otherwise, or when a non-zero
 *   db_chunk < n_db forces it, it is streamed: every _rows call uploads its band's rows and walks the columns from row_first on
 *   in chunks of db_chunk; device memory is then O((n_rows + chunk) * n_sites + the band's records).
 *   Returns 0, -1 bad argument, -2 HIP error.  n_db < 2 or n_sites == 0: a session without device work.
 * ntsm_eval_within_rows: the records of the pairs (i, j), row_first <= i < row_first + n_rows, i < j < n_db, in
 *   ntsm_eval_pair_index order: out[ntsm_eval_pair_index(i, j, n_db) - ntsm_eval_pair_index(row_first, row_first + 1, n_db)],
 *   each bit for bit ntsm_eval_pairs' record on a dense copy of the store's samples.
 *   db_geno (may be NULL): [n_db][3]; entries row_first ... n_db - 1 are written as ntsm_eval_cross writes them.
 *   times (may be NULL): cross_kernel_ms is the pair kernel; chunks counts the column chunks this call uploaded, so it is 0
 *   exactly when the store is resident; the first call on a resident store also reports the upload and preparation of open.
 *   Returns 0, -1 (row_first + n_rows > n_db, n_rows == 0, a NULL it needs), -2.  n_db < 2 or n_sites == 0: zeroed outputs. */
typedef struct ntsm_eval_within_session ntsm_eval_within_session;
int ntsm_eval_within_open(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n_db, uint32_t n_sites,
		uint32_t min_cov, uint32_t db_chunk, ntsm_eval_within_session **h);
int ntsm_eval_within_rows(ntsm_eval_within_session *h, uint32_t row_first, uint32_t n_rows, ntsm_eval_record *out,
		uint32_t *db_geno, ntsm_eval_cross_times *times);
void ntsm_eval_within_close(ntsm_eval_within_session *h);
/* For measurements and tests only: force the workgroup width (64 or 256) of later _rows calls in this process; 0 = the
 * library's rule (64 at every size: DESIGN.md section 9.3 has the measurement that moved it off ntsm_eval_pairs' rule).
 * Returns 0, -1 for another value. */
int ntsm_eval_within_tune(uint32_t width);

/* ntsm_eval_store_score_pairs: out[p] is, bit for bit, the record ntsm_eval_score_pairs gives for (pi[p], pk[p]) on a dense
 *   copy of the store (sample pi[p] as sample 1; either orientation).  A pair needs both of its samples on the device at once:
 *   the list is cut in list order into passes of at most db_chunk distinct samples (ntsm_amd/csrc/host/eval_within.hpp;
 *   0 = the library's choice from free memory, at 16 bytes per sample and site), rows are copied one by one from db_counts and
 *   a sample may be copied in more than one pass; device memory is O(chunk * n_sites + n_pairs).
 *   Returns 0, -1 (a bad argument, an index out of range, pi[p] == pk[p], db_chunk == 1), -2. */
int ntsm_eval_store_score_pairs(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n_db, uint32_t n_sites,
		uint32_t min_cov, const uint32_t *pi, const uint32_t *pk, uint64_t n_pairs, uint32_t db_chunk,
		ntsm_eval_record *out, ntsm_eval_cross_times *times);

/* ---- One cohort store against another (ntsmEval --between; ntsm_amd/csrc/ntsm_eval_between.hip): the
 * n_a x n_b rectangle of pairs (a sample of store A, a sample of store B) over two mapped stores, in bands of rows of A.  A's
 * site table is the run's: B's sites are matched to it by site_map.  a_counts / a_stride_bytes and b_counts / b_stride_bytes
 * as db_counts / db_stride_bytes of ntsm_eval_cross, over n_sites_a and n_sites_b sites; both mappings must outlive the session.
 *
 * ntsm_eval_between_open:
 *   site_map: [n_sites_a]; site_map[s] is the index among B's sites of A's site s, UINT32_MAX where B lacks it (it then counts
 *     0 / 0 for every sample of B).  NULL = the two tables are identical (n_sites_b == n_sites_a).
 *   b_chunk: samples of B per pass, 0 = the library's choice.  B is resident when the chunk rule, asked at 24 bytes per sample
 *     and site of A, answers n_b: it is uploaded, remapped, transposed and tallied once, here.  Otherwise, or when a non-zero
 *     b_chunk < n_b forces it, it is streamed: every _rows call walks B in chunks of b_chunk.  Device memory is
 *     O((n_rows + chunk) * n_sites_a + chunk * n_sites_b + n_rows * n_b).
 *   Returns 0, -2 HIP error, -1 bad argument: a NULL pointer the call needs, a stride below 8 * its n_sites or not a multiple
 *     of 4, a map entry >= n_sites_b that is not UINT32_MAX, a map that names one site of B twice, no map although
 *     n_sites_b != n_sites_a.  n_a == 0, n_b == 0 or n_sites_a == 0: a session without device work.
 * ntsm_eval_between_rows: rows row_first ... row_first + n_rows - 1 of A against every sample of B.
 *   out: [n_rows][n_b].  out[(a - row_first) * n_b + b] is, bit for bit, the record ntsm_eval_pairs gives for pair (a, n_a + b)
 *     of the dense concatenation [A; B remapped to A's sites] -- the sample of A is sample 1.
 *   a_geno (may be NULL): [n_rows][3], b_geno (may be NULL): [n_b][3] = hets, homs, miss (calcHomHetMiss, :742-767) over A's
 *     n_sites_a sites, as ntsm_eval_cross writes db_geno: a site B lacks is a missing site of its samples.
 *   times (may be NULL): cross_kernel_ms is the rectangle kernel; chunks counts the chunks of B this call uploaded, so it is 0
 *     exactly when B is resident; the first call on a resident B also reports the upload and preparation of open.
 *   Returns 0, -2, -1 (row_first + n_rows > n_a, n_rows == 0, a NULL it needs).  n_a == 0, n_b == 0 or n_sites_a == 0: zeroed
 *     outputs, no device work and no HIP call; of an A without samples the one range there is, (0, 0), is taken. */
typedef struct ntsm_eval_between_session ntsm_eval_between_session;
int ntsm_eval_between_open(int device, const void *a_counts, uint64_t a_stride_bytes, uint32_t n_a, const void *b_counts,
		uint64_t b_stride_bytes, uint32_t n_b, uint32_t n_sites_a, uint32_t n_sites_b, const uint32_t *site_map,
		uint32_t min_cov, uint32_t b_chunk, ntsm_eval_between_session **h);
int ntsm_eval_between_rows(ntsm_eval_between_session *h, uint32_t row_first, uint32_t n_rows, ntsm_eval_record *out,
		uint32_t *a_geno, uint32_t *b_geno, ntsm_eval_cross_times *times);
void ntsm_eval_between_close(ntsm_eval_between_session *h);
/* For measurements and tests only: force the workgroup width (64 or 256) of later _rows calls in this process; 0 = the
 * library's rule (256 where a launch has more than 256 columns, else 64: DESIGN.md section 9.4 has the measurement).
 * Returns 0, -1 for another value. */
int ntsm_eval_between_tune(uint32_t width);

/* ---- The PCA-guided search between two cohort stores (ntsmEval --between-near; ntsm_amd/csrc/ntsm_eval_between_near.hip and
 * ntsm_eval_near.hip): projectPCs (src/CompareCounts.hpp:116-211) of store B over store A's site table,
 * computeScorePCA's pairs (:285-398) that name one sample of each store, and their records.  Indices follow the concatenation
 * [A; B] throughout: sample a of A is sample a, sample b of B is sample n_a + b.  Stores, strides and site_map as for
 * ntsm_eval_between_open, with its validity rules (-1 before any HIP call); times as for ntsm_eval_project_store.
 *
 * ntsm_eval_project_store_mapped: cloud [n_b][dim] is, bit for bit, what ntsm_eval_project gives on the dense copy of B
 *   remapped to A's sites (site s of A = B's site site_map[s], 0 / 0 where B lacks it), and b_geno (may be NULL) [n_b][3] what
 *   ntsm_eval_cross gives as db_geno on that copy.  norm [n_sites_a], rot [dim][n_sites_a].  A chunk of B arrives by one 2-D
 *   copy, a kernel remaps its rows to A's sites, and the projection and tally kernels of ntsm_eval_project_store run on the
 *   remapped rows.  b_chunk: 0 = the chunk rule at 8 * (n_sites_a + n_sites_b) bytes per sample.  site_map == NULL is exactly
 *   ntsm_eval_project_store.  Returns 0, -1, -2.  n_b == 0 or n_sites_a == 0: zeroed outputs, no device work. */
int ntsm_eval_project_store_mapped(int device, const void *b_counts, uint64_t b_stride_bytes, uint32_t n_b, uint32_t n_sites_a, uint32_t n_sites_b,
		const uint32_t *site_map, uint32_t min_cov, const long double *norm, const long double *rot, uint32_t dim, uint32_t b_chunk, double *cloud,
		uint32_t *b_geno, ntsm_eval_cross_times *times);

/* ntsm_eval_between_candidates: exactly the sublist of ntsm_eval_candidates' output on the concatenated clouds and radii in
 *   which one index is < n_a and the other >= n_a -- order, indices and dist the same; a pair stands in the row of the sample
 *   with the larger radius, so pi is often a sample of B.  Samples of B across the lanes, samples of A wave-uniform; the
 *   columns of A are never walked.  Capacity protocol and return codes as ntsm_eval_candidates.  n_a == 0 or n_b == 0: no
 *   pairs, no device work. */
int ntsm_eval_between_candidates(int device, const double *a_cloud, const double *a_radius, uint32_t n_a, const double *b_cloud,
		const double *b_radius, uint32_t n_b, uint32_t dim, uint32_t *pi, uint32_t *pk, double *dist, uint64_t capacity, uint64_t *n_pairs,
		double *kernel_ms);

/* ntsm_eval_between_score_pairs: out[p] is, bit for bit, the record ntsm_eval_score_pairs gives for (pi[p], pk[p]) on the dense
 *   concatenation [A; B remapped to A's sites] (sample pi[p] as sample 1; either orientation).  The list is cut in list order
 *   into passes of at most `chunk` distinct samples of both stores together (ntsm_amd/csrc/host/eval_within.hpp; 0 = the
 *   library's choice from free memory); rows of A are copied to their slots as they lie, rows of B through a staging area and
 *   the remap kernel (without a map, straight in); neighbouring samples are one 2-D copy.  times->chunks = the passes.
 *   Returns 0, -2, -1 (a bad argument, an index out of range, a pair of two samples of A or of two of B, chunk == 1). */
int ntsm_eval_between_score_pairs(int device, const void *a_counts, uint64_t a_stride_bytes, uint32_t n_a, const void *b_counts,
		uint64_t b_stride_bytes, uint32_t n_b, uint32_t n_sites_a, uint32_t n_sites_b, const uint32_t *site_map, uint32_t min_cov, const uint32_t *pi,
		const uint32_t *pk, uint64_t n_pairs, uint32_t chunk, ntsm_eval_record *out, ntsm_eval_cross_times *times);

/* ---- The QC tables of a cohort store (ntsmEval --qc; ntsm_amd/csrc/ntsm_eval_profile.hip): what
 * computeScoreSingle (src/CompareCounts.hpp:541-585) tallies per sample, and the same classes per site, in one pass over a
 * mapped store.  The rule is calcHomHetMiss (:742-767) with strict > min_cov: both alleles above is a het, exactly one a hom,
 * neither a miss.  db_counts / db_stride_bytes / db_chunk as for ntsm_eval_cross: one 2-D copy per chunk, the same chunk rule
 * (at 8 * n_sites + 12 bytes per sample); one kernel reads each chunk once.
 *   db_geno (may be NULL): [n_db][3] = hets, homs, miss per sample, value for value ntsm_eval_cross's and
 *     ntsm_eval_project_store's db_geno on the same store.
 *   site_tally (may be NULL): [n_sites][4] = homAT, homCG, het, miss per site: the number of samples of each class there, a
 *     hom counted under the allele that is above min_cov.  The four sum to n_db at every site.
 *   site_cov (may be NULL): [n_sites] = the sum over the samples of uint64(countAT) + uint64(countCG), raw: not masked by
 *     min_cov, and never wrapped.
 *   times (may be NULL): upload_ms the copies, cross_kernel_ms the kernel, download_ms the outputs' way back, chunks.
 * All sums are integer sums: two calls give the same bits.
 * Returns 0, -2 HIP error, -1 bad argument: a NULL db_counts the call needs, all three outputs NULL, a stride below
 * 8 * n_sites or not a multiple of 4.  n_db == 0 or n_sites == 0: zeroed outputs, no device work. */
int ntsm_eval_store_profile(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n_db, uint32_t n_sites,
		uint32_t min_cov, uint32_t db_chunk, uint32_t *db_geno, uint32_t *site_tally, uint64_t *site_cov, ntsm_eval_cross_times *times);

/* ---- The cross-sample contamination check over a cohort store (ntsmEval --contam; ntsm_amd/csrc/ntsm_eval_contam.hip; DESIGN.md
 * section 9.7): the n_db x n_db rectangle of ordered pairs (target q, source d) of the store's own samples, in bands of rows.
 * The reference has no such run; the contract is this text.  db_counts / db_stride_bytes / db_chunk as for ntsm_eval_cross; the
 * mapping must outlive the session.  c = min_cov (strict >, as in the scoring), D = min_depth.
 *
 * A site with target counts (a, g) = (countAT, countCG): t = uint64(a) + uint64(g), m = min(a, g).  It is informative for q iff
 *   t >= D and 4 * m < t, in 64 bits: the minor allele is below a quarter.  a == g is never informative, so the major allele
 *   is AT iff a > g.  With x the source's count of q's minor allele there and y its count of q's major allele,
 *   carries = x > c, has_major = y > c, and the site falls in
 *     class 0, lack: !carries && has_major      class 1, het: carries && has_major      class 2, opp: carries && !has_major
 *   or, with neither (a miss of d), is skipped for this pair.  In its class k: sites[k] += 1, minor[k] += m, depth[k] += t.
 *   The diagonal (q, q) is a pair like any other.  Per target alone, over its informative sites: tally = (sites, sum of m, sum
 *   of t).  All sums are integer sums: two calls give the same bits.
 *
 * ntsm_eval_contam_open: the store is resident when the chunk rule, asked at 16 bytes per sample and site (at, cg and the dense
 *   copy they are transposed from), answers n_db: it is uploaded, transposed and tallied once, here.  Otherwise, or when a
 *   non-zero db_chunk < n_db forces it, it is streamed: every _rows call uploads its band's rows and walks all n_db columns in
 *   chunks of db_chunk; device memory is then O((n_rows + chunk) * n_sites + n_rows * n_db).
 *   Returns 0, -2 HIP error, -1 bad argument, before any HIP call: a NULL it needs, a stride below 8 * n_sites or not a multiple
 *   of 4.  n_db == 0 or n_sites == 0: a session without device work.
 * ntsm_eval_contam_rows: targets row_first ... row_first + n_rows - 1 against every sample as a source.
 *   out: [n_rows][n_db].  out[(q - row_first) * n_db + d] is the record of (q, d); pad is 0.
 *   tally (may be NULL): [n_rows][3] = sites, minor reads, depth of each target of the band.
 *   times (may be NULL): cross_kernel_ms is the rectangle kernel, prepare_kernel_ms the transposes and tallies; chunks counts
 *     the column chunks this call uploaded, so it is 0 exactly when the store is resident; the first call on a resident store
 *     also reports the upload and preparation of open.
 *   Returns 0, -2, -1 (row_first + n_rows > n_db, n_rows == 0, a NULL it needs), the -1 before any HIP call.  n_sites == 0:
 *   zeroed outputs, no device work; of n_db == 0 there is no range to take. */
typedef struct ntsm_eval_contam_record { uint64_t minor[3], depth[3]; uint32_t sites[3], pad /* 0 */; } ntsm_eval_contam_record;  /* 64 bytes */
typedef struct ntsm_eval_contam_session ntsm_eval_contam_session;
int ntsm_eval_contam_open(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n_db, uint32_t n_sites,
		uint32_t min_cov, uint32_t min_depth, uint32_t db_chunk, ntsm_eval_contam_session **h);
int ntsm_eval_contam_rows(ntsm_eval_contam_session *h, uint32_t row_first, uint32_t n_rows, ntsm_eval_contam_record *out,
		uint64_t *tally, ntsm_eval_cross_times *times);
void ntsm_eval_contam_close(ntsm_eval_contam_session *h);
/* For measurements and tests only: force the rectangle kernel's workgroup width (64 or 256) and target group (1, 2 or 4) of later
 * _rows calls in this process; 0 = the library's rule (ntsm_eval_cross's, inherited).  Returns 0, -1 for another value. */
int ntsm_eval_contam_tune(uint32_t width, uint32_t target_group);

/* ---- Parent-parent-child trios in a cohort store (ntsmEval --trios; ntsm_amd/csrc/ntsm_eval_trio.hip):
 * which samples form a trio, and do the trios of a pedigree hold.  The reference has no such run; the contract is this text.
 * db_counts / db_stride_bytes / db_chunk as for ntsm_eval_cross.  All accumulated quantities are integers: two calls of any
 * entry give the same bytes.
 *
 * The genotype rule of this run.  c = min_cov (strict >, as everywhere in the scoring), D = min_depth.  For a sample's cell
 *   (a, g) = (countAT, countCG): A = a > c, G = g > c, t = uint64(a) + uint64(g), and the cell is
 *     het    A && G                  (not depth-gated: both alleles were seen above the cut)
 *     homAT  A && !G && t >= D
 *     homCG  !A && G && t >= D
 *     miss   everything else
 *   called = het | homAT | homCG.  With D = 0 this is the classing of calcHomHetMiss / calcRelatedness (src/CompareCounts.hpp:
 *   1144-1196).  D is there because at low depth a het site shows one allele only and looks like a Mendelian error.
 * A duo (x, y), symmetric: called = the sites where both are called, opp = the sites where one is homAT and the other homCG.
 *   The diagonal is a pair like any other: called = the sample's called sites, opp = 0.
 * A trio (child k; parents x, y), over the sites where all three are called: called += 1; err_hom += 1 when the child is homAT
 *   and x or y is homCG, or the child is homCG and x or y is homAT; err_het += 1 when the child is het and x, y are both homAT
 *   or both homCG.  In bit-planes, 0 / 1 / 2 = homAT / het / homCG:
 *     cl = called_K & called_X & called_Y
 *     eh = cl & ((K0 & (X2 | Y2)) | (K2 & (X0 | Y0)))
 *     et = cl & K1 & ((X0 & Y0) | (X2 & Y2))
 *   The two error classes are disjoint; the record is symmetric in x and y and not in the child; pad is 0.
 *
 * ntsm_eval_trio_open: streams the store once, in chunks of db_chunk samples (0 = the chunk rule, asked at what a staged chunk
 *   holds beside the planes: 8 * n_sites bytes per sample), and builds the three planes hom_at, het, hom_cg, one bit per sample
 *   and site, on the device.  The planes are always resident (3 * ceil(n_sites / 64) * 8 bytes per sample); the counts go back
 *   before open returns.  The mapping need not outlive the call.
 *   geno (may be NULL): [n_db][4] = homAT, het, homCG, miss of each sample under this rule; the four sum to n_sites.
 *   times (may be NULL): upload_ms the copies, prepare_kernel_ms the plane and geno kernels, download_ms geno's way back,
 *     chunks the chunks uploaded.
 *   Returns 0, -2 HIP error, -1 bad argument, before any HIP call: a NULL it needs, a stride below 8 * n_sites or not a
 *   multiple of 4.  n_db == 0 or n_sites == 0: a session without device work (geno zeroed).
 * ntsm_eval_trio_duos: rows row_first ... row_first + n_rows - 1 against every sample: out [n_rows][n_db],
 *   out[(x - row_first) * n_db + y] the duo (x, y).  kernel_ms (may be NULL): the rectangle kernel, from HIP events.
 *   Returns 0, -2, -1 (row_first + n_rows > n_db, n_rows == 0, a NULL it needs), the -1 before any HIP call.  n_sites == 0:
 *   zeroed records; of n_db == 0 there is no range to take.
 * ntsm_eval_trio_score: trio lists in CSR form.  Entry i, i < n_children, has the child child[i] and the candidate list
 *   cand[offset[i] ... offset[i + 1]) of length k_i; its k_i (k_i - 1) / 2 records are the pairs of list positions p < q, p
 *   ascending and q ascending inside p, the record of (p, q) being the trio (child[i]; cand[offset[i] + p], cand[offset[i] + q]);
 *   they start at out[sum over j < i of k_j (k_j - 1) / 2].  Lists need not be sorted and may repeat a sample; a child may
 *   appear in several entries; lists of length 0 or 1 give no records.  offset: [n_children + 1].  kernel_ms (may be NULL).
 *   Returns 0, -2, -1 before any HIP call: a NULL it needs, an index >= n_db, a candidate equal to its entry's child, a
 *   decreasing offset, offset[0] != 0.  n_children == 0: nothing to do, returns 0.  n_sites == 0: zeroed records. */
typedef struct ntsm_eval_trio_duo { uint32_t called, opp; } ntsm_eval_trio_duo;   /* 8 bytes */
typedef struct ntsm_eval_trio_record { uint32_t called, err_hom, err_het, pad /* 0 */; } ntsm_eval_trio_record;   /* 16 bytes */
typedef struct ntsm_eval_trio_session ntsm_eval_trio_session;
int ntsm_eval_trio_open(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n_db, uint32_t n_sites, uint32_t min_cov,
		uint32_t min_depth, uint32_t db_chunk, uint32_t *geno, ntsm_eval_cross_times *times, ntsm_eval_trio_session **h);
int ntsm_eval_trio_duos(ntsm_eval_trio_session *h, uint32_t row_first, uint32_t n_rows, ntsm_eval_trio_duo *out, double *kernel_ms);
int ntsm_eval_trio_score(ntsm_eval_trio_session *h, const uint32_t *child, const uint64_t *offset, const uint32_t *cand, uint32_t n_children,
		ntsm_eval_trio_record *out, double *kernel_ms);
void ntsm_eval_trio_close(ntsm_eval_trio_session *h);
/* For measurements and tests only: force the workgroup width (64 or 256) of later _duos and _score calls in this process: the
 * duo kernel's workgroup, and the trio kernel's tile for every list (64 threads: the 16 x 16 tile, 256 threads: the 64 x 64
 * tile); 0 = the library's rule (duo: ntsm_eval_cross's, inherited; trio: the small tile for lists of up to 16).  Returns 0, -1
 * for another value. */
int ntsm_eval_trio_tune(uint32_t width);

/* ---- Site-pair LD over a cohort store (ntsmEval --ld; ntsm_amd/csrc/ntsm_eval_ld.hip): the transpose of
 * the trio question -- bit-planes with the samples along the bits, and a popcount GEMM over sites x sites.  The reference has no
 * such run; the contract is this text.  db_counts / db_stride_bytes / db_chunk as for ntsm_eval_cross.  All accumulated quantities
 * are integers: two calls of any entry give the same bytes.
 *
 * Classes.  c = min_cov, D = min_depth; a cell's class is "the genotype rule of this run" of the trio section above, unchanged
 *   (one function for both libraries: ntsm_amd/csrc/ntsm_eval_geno.h).  Dosage x = 0 for homAT, 1 for het, 2 for homCG.
 * Per site s, as sets of samples: H_s = het, G_s = homCG, C_s = called.
 * The record of the ordered site pair (s, t), eight counts of samples:
 *     n  = |C_s & C_t|   hs = |H_s & C_t|   gs = |G_s & C_t|   ht = |C_s & H_t|   gt = |C_s & G_t|
 *     hh = |H_s & H_t|   hg = |(H_s & G_t) | (G_s & H_t)|      gg = |G_s & G_t|
 *   The two sets under hg are disjoint.  The record of (t, s) is that of (s, t) with hs <-> ht and gs <-> gt.  The diagonal is a
 *   pair like any other.
 * Moments, in int64, exact for n_db <= 2^24 (a larger store is refused):
 *     Sx = hs + 2 gs   Sy = ht + 2 gt   Sxx = hs + 4 gs   Syy = ht + 4 gt   Sxy = hh + 2 hg + 4 gg
 *     cov = n Sxy - Sx Sy    vx = n Sxx - Sx^2    vy = n Syy - Sy^2
 * r^2 is undefined when n < min_called, vx == 0 or vy == 0; else it is the double (double(cov) * double(cov)) / (double(vx) *
 *   double(vy)): two multiplications and one division, each rounded once (no contraction).  r^2 <= 1.0.  dir is + when cov > 0,
 *   else -.  The expressions are ntsm_amd/csrc/host/eval_ld.hpp's, which the device's test of a pair compiles too.
 * A pair is selected when s < t, r^2 is defined and r^2 >= r2_min.
 *
 * ntsm_eval_ld_open: streams the store once, in chunks of db_chunk samples (0 = the chunk rule, asked at 8 * n_sites bytes per
 *   sample), and builds three planes het, hom_cg, called as [plane][sample word][site] uint64 on the device: a word holds 64
 *   samples, the site index is fastest, bits past n_db in the last word are zero.  The planes are always resident
 *   (3 * ceil(n_db / 64) * 8 bytes per site); the counts go back before open returns.  The mapping need not outlive the call.
 *   site_geno (may be NULL): [n_sites][4] = het, homCG, called, homAT of each site: the number of samples of each class there.
 *   times (may be NULL): upload_ms the copies, prepare_kernel_ms the plane and site_geno kernels, download_ms site_geno's way
 *     back, chunks the chunks uploaded.
 *   Returns 0, -2 HIP error, -1 bad argument, before any HIP call: a NULL it needs, a stride below 8 * n_sites or not a multiple
 *   of 4, n_db > 2^24.  n_db == 0 or n_sites == 0: a session without device work (site_geno zeroed).
 * ntsm_eval_ld_rows: the dense records of sites row_first ... row_first + n_rows - 1 against every site: out [n_rows][n_sites],
 *   out[(s - row_first) * n_sites + t] the record of (s, t).  kernel_ms (may be NULL): the rectangle kernel, from HIP events.
 *   Returns 0, -2, -1 (row_first + n_rows > n_sites, n_rows == 0, a NULL it needs), the -1 before any HIP call.  n_db == 0: zeroed
 *   records; of n_sites == 0 there is no range to take.
 * ntsm_eval_ld_select: the selected pairs (a, b) with row_first <= a < row_first + n_rows and a < b < n_sites, sorted by (a, b).
 *   Only tiles on or above the diagonal are evaluated, the test runs on the device and no dense rectangle is written.
 *   cap: the pairs out_pairs holds (out_pairs may be NULL when cap is 0).  *n_found is always the true total.  Returns 0; 1 when
 *   *n_found > cap, out_pairs then unspecified; -2; -1 as _rows, and for a non-finite r2_min or a NULL n_found.  n_db == 0:
 *   nothing is selected. */
typedef struct ntsm_eval_ld_record { uint32_t n, hs, gs, ht, gt, hh, hg, gg; } ntsm_eval_ld_record;   /* 32 bytes */
typedef struct ntsm_eval_ld_pair { uint32_t a, b; ntsm_eval_ld_record rec; } ntsm_eval_ld_pair;   /* 40 bytes */
#define NTSM_EVAL_LD_MAX_SAMPLES (1u << 24)
typedef struct ntsm_eval_ld_session ntsm_eval_ld_session;
int ntsm_eval_ld_open(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n_db, uint32_t n_sites, uint32_t min_cov,
		uint32_t min_depth, uint32_t db_chunk, uint32_t *site_geno, ntsm_eval_cross_times *times, ntsm_eval_ld_session **h);
int ntsm_eval_ld_rows(ntsm_eval_ld_session *h, uint32_t row_first, uint32_t n_rows, ntsm_eval_ld_record *out, double *kernel_ms);
int ntsm_eval_ld_select(ntsm_eval_ld_session *h, uint32_t row_first, uint32_t n_rows, uint32_t min_called, double r2_min, uint64_t cap,
		ntsm_eval_ld_pair *out_pairs, uint64_t *n_found, double *kernel_ms);
void ntsm_eval_ld_close(ntsm_eval_ld_session *h);
/* For measurements and tests only: force the register block of the rectangle kernel -- rows x columns of pairs per lane, one of
 * 2 x 2, 4 x 2 and 2 x 4, which with 16 x 16 lanes is a tile of 32 x 32, 64 x 32 or 32 x 64 sites -- of later _rows and _select
 * calls in this process; (0, 0) = the library's rule (2 x 2).  Returns 0, -1 for another value. */
int ntsm_eval_ld_tune(uint32_t block_rows, uint32_t block_cols);

#ifdef __cplusplus
}
#endif
#endif
