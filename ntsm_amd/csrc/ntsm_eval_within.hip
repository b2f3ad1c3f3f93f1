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
 * ntsm_eval_chunk.h's; the holding, the band's rows and the walk over the columns are ntsm_eval_band.h's.  What is here: the
 * kernel, its launch, and the 24 bytes per sample and site.  One stream, no overlap.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <memory>

#include "../../include/ntsm_eval_hip.h"
#include "host/eval_within.hpp"
#define NTSM_HIP_TAG "ntsm_eval_within"
#include "ntsm_eval_band.h"
#include "ntsm_eval_score.h"
#include "ntsm_hip_scope.h"

namespace {

using ntsm_eval_band::Staged;
using ntsm_eval_band::Window;
using ntsm_eval_chunk::kThreads;
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

/* the pairs of the rows' samples with the columns' samples, timed into *ms (added) */
int launch_within(const Window &rows, const Window &cols, uint32_t n_db, uint32_t n_sites, uint32_t min_cov, ntsm_eval_record *d_out, uint64_t out_base,
		hipEvent_t e0, hipEvent_t e1, double *ms)
{
	/* One-wave workgroups at every size.  The kernel is built for both widths and started out with ntsm_eval_pairs' rule (64
	 * up to 1,024 columns in the launch, else 256), at which it runs at that kernel's speed; measured on the whole triangle of
	 * 4,096 x 96,287 sites, 64 threads take 2,412 ms against 2,954 ms for 256 (three runs each, spreads 47 and 46 ms; DESIGN.md
	 * section 9.3), as ntsm_eval_cross found for the rectangle.  256 is reachable through ntsm_eval_within_tune only. */
	const unsigned bt = g_width ? g_width : 64;
	return ntsm_eval_chunk::timed(e0, e1, ms, [&] {
		hipLaunchKernelGGL(ntsm_eval_within_kernel, dim3((cols.count + bt - 1) / bt, (rows.count + kTI - 1) / kTI), dim3(bt), 0, 0, rows.at, rows.cg, rows.term,
				rows.pitch, rows.first, rows.count, cols.at, cols.cg, cols.term, cols.pitch, cols.first, cols.count, n_db, n_sites, min_cov, d_out, out_base);
		HIPCHK(hipGetLastError());
		return 0;
	});
}

}  // namespace

struct ntsm_eval_within_session {
	const char *db = nullptr;
	uint64_t stride = 0;
	uint32_t n_db = 0, n_sites = 0, min_cov = 0;
	ntsm_eval_band::Holding<uint32_t> hold;  /* the store's samples as columns, with their hets, homs, miss */

	/* ntsm_eval_chunk.h's staging of a window, for the columns and for a streamed band's rows */
	auto stager()
	{
		return [this](uint32_t first, uint32_t count, const Staged<uint32_t> &to, bool tallies, ntsm_eval_cross_times &tm) {
			return ntsm_eval_band::stage_scored(db, stride, first, count, n_sites, min_cov, to, tallies, hold.ev[0], hold.ev[1], tm);
		};
	}
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
	if (!ntsm_eval_chunk::valid_store(db_counts, db_stride_bytes, n_db, n_sites)) return -1;
	std::unique_ptr<ntsm_eval_within_session> s(new ntsm_eval_within_session);
	s->db = (const char *) db_counts;
	s->stride = db_stride_bytes;
	s->n_db = n_db; s->n_sites = n_sites; s->min_cov = min_cov;
	if (n_db < 2 || n_sites == 0) { *h = s.release(); return 0; }                /* nothing to score: no device work, here or in _rows */

	/* 24 bytes per sample and site (what ntsm_eval_pairs holds): the transposed 16 and the dense 8; and the tallies */
	int rc = s->hold.open(device, n_db, n_sites, n_sites, db_chunk, 3 * 8ull * n_sites + 12, true, true);
	if (rc || (rc = s->hold.fill(s->stager())) != 0) return rc;
	*h = s.release();
	return 0;
}

extern "C" void ntsm_eval_within_close(ntsm_eval_within_session *h)
{
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
	if (!h->hold.device_work) {
		if (records) memset(out, 0, records * sizeof(ntsm_eval_record));
		if (db_geno) memset(db_geno + (size_t) row_first * 3, 0, (size_t) (n_db - row_first) * 3 * sizeof(uint32_t));
		return 0;
	}
	HIPCHK(hipSetDevice(h->hold.device));
	ntsm_hip::Buffers b;                                                          /* this call's: streamed, the band's rows */
	ntsm_eval_cross_times tm = h->hold.take_open_times();
	Window rows;
	int rc = h->hold.band_rows(b, row_first, n_rows, nullptr, h->stager(), tm, rows);
	if (rc) return rc;
	/* the columns before row_first pair with no row of the band: a streamed store leaves them on the host */
	rc = h->hold.walk(row_first, records, out, db_geno, h->stager(), [&](const Window &cols, ntsm_eval_record *d_out) {
		return launch_within(rows, cols, n_db, n_sites, min_cov, d_out, base, h->hold.ev[0], h->hold.ev[1], &tm.cross_kernel_ms);
	}, tm);
	if (rc) return rc;
	if (times) *times = tm;
	return 0;
}

