/*
 * ntsm_eval_within.hip -- the pairs inside a cohort store on one MI355X (include/ntsm_eval_hip.h: ntsm_eval_within_open /
 * _rows / _close; ntsmEval --within): the triangle of pairs (i, j), i < j, of the store's own samples,
 * in bands of rows, each record bit for bit what ntsm_eval_pairs gives on a dense copy of the samples.
 *
 * Kernel.  The pair kernel's tile (ntsm_eval.hip) restated over two buffers: the columns j go across the lanes, one
 * coalesced 4 + 4 + 8-byte load per lane and site out of at / cg / term [site][column]; kTI = 4 consecutive rows i are
 * wave-uniform (scalar loads) out of arrays of their own pitch; one ntsm_eval_acc per pair walks the sites in order
 * (ntsm_eval_score.h), so the sums are the reference's sequential sums.  Both buffers are windows of the store: element 0 of
 * the rows is sample row_first, element 0 of the columns is sample col_first, and everything about the diagonal is decided
 * on those global numbers -- a workgroup whose last column is <= its first row returns, a pair is stored only when j > i.
 *
 * Two ways of holding the store.  Resident: the whole store fits the chunk rule at 24 bytes per sample and site (what
 * ntsm_eval_pairs holds); it is uploaded, transposed and tallied once at open, and a band's rows and columns are offsets
 * into the same arrays.  Streamed: each call uploads and transposes its band's rows into a buffer of their own (pitch =
 * n_rows) and walks the columns row_first ... n_db - 1 in chunks of db_chunk, as ntsm_eval_cross walks a store; the columns
 * before row_first never leave the host.  The chunk rule and the staging of a window (copy, transpose, tallies) are
 * ntsm_eval_chunk.h's.  One stream, no overlap.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/ntsm_eval_hip.h"
#include "host/eval_within.hpp"
#define NTSM_HIP_TAG "ntsm_eval_within"
#include "ntsm_eval_chunk.h"
#include "ntsm_eval_score.h"
#include "ntsm_hip_scope.h"

namespace {

using ntsm_eval_chunk::kThreads;
using ntsm_eval_chunk::ms_since;
using ntsm_eval_chunk::wall;
namespace band = ntsm::eval_within;
constexpr int kTI = 4;                       /* rows i per workgroup, as in ntsm_eval.hip */

uint32_t g_width = 0;                        /* ntsm_eval_within_tune */

/* grid (columns / blockDim.x, rows / kTI).  rat / rcg / rterm [site][row_pitch]: element r is sample row_first + r, n_rows of
 * them; cat / ccg / cterm [site][col_pitch]: element c is sample col_first + c, n_cols of them.  out: the band's records,
 * pair (i, j) at ntsm_eval_pair_index(i, j, n_db) - out_base. */
__global__ __launch_bounds__(kThreads) void ntsm_eval_within_kernel(const uint32_t *__restrict__ rat, const uint32_t *__restrict__ rcg,
		const double *__restrict__ rterm, uint32_t row_pitch, uint32_t row_first, uint32_t n_rows, const uint32_t *__restrict__ cat,
		const uint32_t *__restrict__ ccg, const double *__restrict__ cterm, uint32_t col_pitch, uint32_t col_first, uint32_t n_cols,
		uint32_t n_db, uint32_t n_sites, uint32_t min_cov, ntsm_eval_record *__restrict__ out, uint64_t out_base)
{
	const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t r0 = blockIdx.y * kTI;
	if ((uint64_t) col_first + blockIdx.x * blockDim.x + (blockDim.x - 1) <= (uint64_t) row_first + r0) return;   /* the whole tile lies on or below the diagonal */
	const uint32_t cc = c < n_cols ? c : n_cols - 1;                             /* lanes past the end compute a copy of the last column, not stored */
	ntsm_eval_acc acc[kTI];
	for (uint32_t site = 0; site < n_sites; ++site) {
		const uint64_t col = (uint64_t) site * col_pitch + cc, row = (uint64_t) site * row_pitch;
		const ntsm_eval_side sj = ntsm_eval_side_of(cat[col], ccg[col], cterm[col], min_cov);
#pragma unroll
		for (int ii = 0; ii < kTI; ++ii) {
			const uint32_t r = r0 + ii < n_rows ? r0 + ii : n_rows - 1;         /* wave-uniform: scalar loads; past the band's end a copy of its last row */
			acc[ii].add(ntsm_eval_side_of(rat[row + r], rcg[row + r], rterm[row + r], min_cov), sj, min_cov);
		}
	}
	if (c >= n_cols) return;
	const uint32_t j = col_first + c;
#pragma unroll
	for (int ii = 0; ii < kTI; ++ii) {
		const uint32_t i = row_first + r0 + ii;
		if (r0 + ii >= n_rows || j <= i) continue;
		out[(uint64_t) i * n_db - (uint64_t) i * (i + 1) / 2 + (j - i - 1) - out_base] = acc[ii].record();   /* ntsm_eval_pair_index */
	}
}

/* a window of transposed samples on the device */
struct Window { const uint32_t *at, *cg; const double *term; uint32_t pitch, first, count; };

/* the pairs of the rows' samples with the columns' samples, timed into *ms (added) */
int launch_within(const Window &rows, const Window &cols, uint32_t n_db, uint32_t n_sites, uint32_t min_cov, ntsm_eval_record *d_out, uint64_t out_base,
		hipEvent_t e0, hipEvent_t e1, double *ms)
{
	/* One-wave workgroups at every size.  The kernel is built for both widths and started out with ntsm_eval_pairs' rule (64
	 * up to 1,024 columns in the launch, else 256), at which it runs at that kernel's speed; measured on the whole triangle of
	 * 4,096 x 96,287 sites, 64 threads take 2,412 ms against 2,954 ms for 256 (three runs each, spreads 47 and 46 ms; DESIGN.md
	 * section 9.3), as ntsm_eval_cross found for the rectangle.  256 is reachable through ntsm_eval_within_tune only. */
	const unsigned bt = g_width ? g_width : 64;
	HIPCHK(hipEventRecord(e0, 0));
	hipLaunchKernelGGL(ntsm_eval_within_kernel, dim3((cols.count + bt - 1) / bt, (rows.count + kTI - 1) / kTI), dim3(bt), 0, 0, rows.at, rows.cg, rows.term,
			rows.pitch, rows.first, rows.count, cols.at, cols.cg, cols.term, cols.pitch, cols.first, cols.count, n_db, n_sites, min_cov, d_out, out_base);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(e1, 0));
	HIPCHK(hipEventSynchronize(e1));
	return ntsm_eval_chunk::add_interval(e0, e1, ms);
}

/* ntsm_eval_chunk::stage and the wait for it: the pair kernel's launch records the same two events next */
int stage(const char *db, uint64_t stride, uint32_t first, uint32_t count, uint32_t n_sites, uint32_t min_cov, uint32_t *d_raw, uint32_t *d_at, uint32_t *d_cg,
		double *d_term, uint32_t *d_geno, hipEvent_t e0, hipEvent_t e1, ntsm_eval_cross_times &tm)
{
	const int rc = ntsm_eval_chunk::stage(db, stride, first, count, n_sites, min_cov, d_raw, d_at, d_cg, d_term, d_geno, e0, e1, tm);
	if (rc) return rc;
	HIPCHK(hipEventSynchronize(e1));
	return ntsm_eval_chunk::add_interval(e0, e1, &tm.prepare_kernel_ms);
}

}  // namespace

struct ntsm_eval_within_session {
	int device = 0;
	const char *db = nullptr;
	uint64_t stride = 0;
	uint32_t n_db = 0, n_sites = 0, min_cov = 0;
	uint32_t chunk = 0;                      /* columns per pass of a streamed store */
	bool resident = false;
	ntsm_hip::Buffers b;
	ntsm_hip::Events<2> ev;
	/* resident: the whole store [site][n_db]; streamed: one chunk of columns [site][chunk] with its staging and tallies */
	uint32_t *d_at = nullptr, *d_cg = nullptr, *d_raw = nullptr, *d_geno = nullptr;
	double *d_term = nullptr;
	std::vector<uint32_t> geno;              /* resident: [n_db][3], taken at open */
	ntsm_eval_cross_times open_times {};     /* resident: the upload and preparation of open, reported by the first _rows call */
};

extern "C" int ntsm_eval_within_tune(uint32_t width)
{
	if (width != 0 && width != 64 && width != 256) return -1;
	g_width = width;
	return 0;
}

extern "C" int ntsm_eval_within_open(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n_db, uint32_t n_sites, uint32_t min_cov,
		uint32_t db_chunk, ntsm_eval_within_session **h)
{
	if (!h) return -1;
	*h = nullptr;
	if ((!db_counts && n_db && n_sites) || db_stride_bytes < 8ull * n_sites || db_stride_bytes % 4) return -1;
	std::unique_ptr<ntsm_eval_within_session> s(new ntsm_eval_within_session);
	s->device = device;
	s->db = (const char *) db_counts;
	s->stride = db_stride_bytes;
	s->n_db = n_db; s->n_sites = n_sites; s->min_cov = min_cov;
	if (n_db < 2 || n_sites == 0) { *h = s.release(); return 0; }                /* nothing to score: no device work, here or in _rows */

	const uint64_t row_bytes = 8ull * n_sites;
	HIPCHK(hipSetDevice(device));
	size_t free_b = 0, total_b = 0;
	if (db_chunk == 0) HIPCHK(hipMemGetInfo(&free_b, &total_b));
	s->chunk = ntsm_eval_chunk::samples_per_pass(db_chunk, n_db, free_b, 3 * row_bytes + 12, 0);
	s->resident = s->chunk == n_db;
	const uint64_t cells = (uint64_t) s->chunk * n_sites;
	HIPCHK(s->ev.create());
	HIPCHK(s->b.alloc(&s->d_at, cells));
	HIPCHK(s->b.alloc(&s->d_cg, cells));
	HIPCHK(s->b.alloc(&s->d_term, cells));
	HIPCHK(s->b.alloc(&s->d_geno, (uint64_t) s->chunk * 3));
	HIPCHK(s->b.alloc(&s->d_raw, cells * 2));
	if (s->resident) {
		const int rc = stage(s->db, s->stride, 0, n_db, n_sites, min_cov, s->d_raw, s->d_at, s->d_cg, s->d_term, s->d_geno, s->ev[0], s->ev[1], s->open_times);
		if (rc) return rc;
		s->geno.resize((size_t) n_db * 3);
		const auto t = wall::now();
		HIPCHK(hipMemcpy(s->geno.data(), s->d_geno, s->geno.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
		s->open_times.download_ms += ms_since(t);
		HIPCHK(s->b.release(&s->d_raw));                                         /* the staging third goes back before the records need room */
	}
	*h = s.release();
	return 0;
}

extern "C" void ntsm_eval_within_close(ntsm_eval_within_session *h)
{
	if (!h) return;
	if (h->d_at) (void) hipSetDevice(h->device);                                 /* a session without device work touches no device here either */
	delete h;
}

extern "C" int ntsm_eval_within_rows(ntsm_eval_within_session *h, uint32_t row_first, uint32_t n_rows, ntsm_eval_record *out, uint32_t *db_geno,
		ntsm_eval_cross_times *times)
{
	if (times) *times = ntsm_eval_cross_times {};
	if (!h || n_rows == 0 || (uint64_t) row_first + n_rows > h->n_db) return -1;
	const uint32_t n_db = h->n_db, n_sites = h->n_sites, min_cov = h->min_cov;
	const uint64_t records = band::band_records(row_first, n_rows, n_db), base = band::band_base(row_first, n_db);
	if (!out && records) return -1;
	if (n_db < 2 || n_sites == 0) {
		if (records) memset(out, 0, records * sizeof(ntsm_eval_record));
		if (db_geno) memset(db_geno + (size_t) row_first * 3, 0, (size_t) (n_db - row_first) * 3 * sizeof(uint32_t));
		return 0;
	}
	HIPCHK(hipSetDevice(h->device));
	ntsm_hip::Buffers b;                                                          /* this call's: the records and, streamed, the band's rows */
	ntsm_eval_record *d_out;
	HIPCHK(b.alloc(&d_out, records));
	ntsm_eval_cross_times tm = h->open_times;
	h->open_times = ntsm_eval_cross_times {};
	const uint32_t n_cols = n_db - row_first;
	if (h->resident) {
		const Window rows { h->d_at + row_first, h->d_cg + row_first, h->d_term + row_first, n_db, row_first, n_rows };
		const Window cols { rows.at, rows.cg, rows.term, n_db, row_first, n_cols };
		const int rc = launch_within(rows, cols, n_db, n_sites, min_cov, d_out, base, h->ev[0], h->ev[1], &tm.cross_kernel_ms);
		if (rc) return rc;
		if (db_geno) memcpy(db_geno + (size_t) row_first * 3, h->geno.data() + (size_t) row_first * 3, (size_t) n_cols * 3 * sizeof(uint32_t));
	} else {
		uint32_t *d_rraw, *d_rat, *d_rcg;
		double *d_rterm;
		const uint64_t rcells = (uint64_t) n_rows * n_sites;
		HIPCHK(b.alloc(&d_rat, rcells));
		HIPCHK(b.alloc(&d_rcg, rcells));
		HIPCHK(b.alloc(&d_rterm, rcells));
		HIPCHK(b.alloc(&d_rraw, rcells * 2));
		int rc = stage(h->db, h->stride, row_first, n_rows, n_sites, min_cov, d_rraw, d_rat, d_rcg, d_rterm, nullptr, h->ev[0], h->ev[1], tm);
		if (rc) return rc;
		HIPCHK(b.release(&d_rraw));
		const Window rows { d_rat, d_rcg, d_rterm, n_rows, row_first, n_rows };
		for (uint32_t c0 = row_first; c0 < n_db; c0 += h->chunk) {
			const uint32_t cn = std::min(h->chunk, n_db - c0);
			rc = stage(h->db, h->stride, c0, cn, n_sites, min_cov, h->d_raw, h->d_at, h->d_cg, h->d_term, db_geno ? h->d_geno : nullptr, h->ev[0], h->ev[1], tm);
			if (rc) return rc;
			const Window cols { h->d_at, h->d_cg, h->d_term, cn, c0, cn };
			rc = launch_within(rows, cols, n_db, n_sites, min_cov, d_out, base, h->ev[0], h->ev[1], &tm.cross_kernel_ms);
			if (rc) return rc;
			if (db_geno) {
				const auto t = wall::now();
				HIPCHK(hipMemcpy(db_geno + (size_t) c0 * 3, h->d_geno, (size_t) cn * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
				tm.download_ms += ms_since(t);
			}
			tm.chunks++;
		}
	}
	const auto t = wall::now();
	if (records) HIPCHK(hipMemcpy(out, d_out, records * sizeof(ntsm_eval_record), hipMemcpyDeviceToHost));
	tm.download_ms += ms_since(t);
	if (times) *times = tm;
	return 0;
}
