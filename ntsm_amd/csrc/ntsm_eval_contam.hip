/*
 * ntsm_eval_contam.hip -- the cross-sample contamination check over a cohort store on one MI355X (include/ntsm_eval_hip.h:
 * ntsm_eval_contam_open / _rows / _close; ntsmEval --contam): the n_db x n_db rectangle of ordered pairs
 * (target q, source d) of the store's own samples, in bands of rows.  At the sites where the target looks homozygous (its
 * minor allele below a quarter of at least min_depth reads) the target's minor reads and depth are summed in three classes by
 * what the source carries there: it lacks the target's minor allele, it has both alleles, it has the minor allele only.  All
 * sums are integers: there is no rounding, no order, and two calls give the same bits.
 *
 * Kernel.  The cross kernel's tile (ntsm_eval_cross.hip) with another per-site update: the sources d go across the lanes, one
 * coalesced 4 + 4-byte load per lane and site out of at / cg [site][column]; a group of TQ targets is wave-uniform (scalar
 * loads out of arrays of their own pitch), so the depth t, the minor count m, whether the site is informative and which
 * allele is the major one are formed once per target and site, and a site that is not informative for a target costs its
 * lanes nothing (a wave-uniform branch).  A lane keeps nine integers per target -- minor[3] and depth[3] in 64 bits, sites[3]
 * in 32 -- and walks the sites in order.  The diagonal (q, q) is a pair like any other.
 *
 * Two ways of holding the store, as ntsm_eval_within.hip has them.  Resident: the store fits the chunk rule at 16 bytes per
 * sample and site (at and cg, and the dense copy the transpose reads); it is uploaded, transposed and tallied once at open and
 * a band's rows are an offset into the columns' arrays.  Streamed: each call uploads and transposes its band's rows (pitch =
 * n_rows) and walks all n_db columns in chunks.  The holding, the band's rows and the walk are ntsm_eval_band.h's; the chunk
 * rule, the 2-D copy and the launch rule are ntsm_eval_chunk.h's; the transpose is this file's, since that header's also
 * writes the 8-byte term plane of the scoring, which nothing reads here.  The per-target tallies come from one workgroup per
 * row over the dense copy.  One stream, no overlap.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <memory>

#include "../../include/ntsm_eval_hip.h"
#define NTSM_HIP_TAG "ntsm_eval_contam"
#include "ntsm_eval_band.h"
#include "ntsm_hip_scope.h"

namespace {

using ntsm_eval_band::Staged;
using ntsm_eval_band::Window;
using ntsm_eval_chunk::kThreads;
using ntsm_eval_chunk::kTile;

uint32_t g_width = 0, g_target_group = 0;    /* ntsm_eval_contam_tune */

/* counts [sample][site][2] (dense) -> at / cg [site][sample]: ntsm_eval_chunk::prepare_kernel without the term plane */
__global__ __launch_bounds__(kThreads) void ntsm_eval_contam_transpose_kernel(const uint2 *__restrict__ counts, uint32_t n_samples, uint32_t n_sites,
		uint32_t s_first, uint32_t *__restrict__ at, uint32_t *__restrict__ cg)
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
	}
}

/* what a site is for a target with counts (a, g): depth, minor count, informative or not, and the major allele */
struct Site { uint64_t t; uint32_t m; bool informative, major_at; };
__device__ __host__ inline Site site_of(uint32_t a, uint32_t g, uint32_t min_depth)
{
	Site s;
	s.t = (uint64_t) a + (uint64_t) g;
	s.m = a < g ? a : g;
	s.informative = s.t >= min_depth && 4 * (uint64_t) s.m < s.t;
	s.major_at = a > g;
	return s;
}

/* sites, minor reads and depth of every row's informative sites: one workgroup per row over the dense buffer, in
 * ntsm_eval_chunk::tally_kernel's style; tally [row][3] */
__global__ __launch_bounds__(kThreads) void ntsm_eval_contam_tally_kernel(const uint2 *__restrict__ counts, uint32_t n_sites, uint32_t min_depth,
		unsigned long long *__restrict__ tally)
{
	__shared__ unsigned long long sum[3];
	if (threadIdx.x < 3) sum[threadIdx.x] = 0;
	__syncthreads();
	const uint2 *row = counts + (uint64_t) blockIdx.x * n_sites;
	unsigned long long sites = 0, minor = 0, depth = 0;
	for (uint32_t site = threadIdx.x; site < n_sites; site += kThreads) {
		const uint2 c = row[site];
		const Site s = site_of(c.x, c.y, min_depth);
		if (!s.informative) continue;
		sites += 1;
		minor += s.m;
		depth += s.t;
	}
	atomicAdd(&sum[0], sites);
	atomicAdd(&sum[1], minor);
	atomicAdd(&sum[2], depth);
	__syncthreads();
	if (threadIdx.x < 3) tally[(uint64_t) blockIdx.x * 3 + threadIdx.x] = sum[threadIdx.x];
}

/* grid (columns / blockDim.x, rows / TQ).  rat / rcg [site][row_pitch]: element r is the band's row r, n_rows of them;
 * cat / ccg [site][col_pitch]: element c is the launch's column c, n_cols of them.  out [n_rows][out_pitch], column c at c. */
template <int TQ> __global__ __launch_bounds__(kThreads) void ntsm_eval_contam_kernel(const uint32_t *__restrict__ rat, const uint32_t *__restrict__ rcg,
		uint32_t row_pitch, uint32_t n_rows, const uint32_t *__restrict__ cat, const uint32_t *__restrict__ ccg, uint32_t col_pitch, uint32_t n_cols,
		uint32_t n_sites, uint32_t min_cov, uint32_t min_depth, ntsm_eval_contam_record *__restrict__ out, uint64_t out_pitch)
{
	const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t q0 = blockIdx.y * TQ;
	const uint32_t dc = d < n_cols ? d : n_cols - 1;                              /* lanes past the end compute a copy of the last column, not stored */
	uint32_t q[TQ];
#pragma unroll
	for (int k = 0; k < TQ; ++k) q[k] = q0 + k < n_rows ? q0 + k : n_rows - 1;     /* wave-uniform: scalar loads */
	uint64_t minor[TQ][3], depth[TQ][3];
	uint32_t sites[TQ][3];
#pragma unroll
	for (int k = 0; k < TQ; ++k)
#pragma unroll
		for (int c = 0; c < 3; ++c) { minor[k][c] = 0; depth[k][c] = 0; sites[k][c] = 0; }
	for (uint32_t site = 0; site < n_sites; ++site) {
		const uint64_t col = (uint64_t) site * col_pitch + dc, row = (uint64_t) site * row_pitch;
		const uint32_t sa = cat[col], sg = ccg[col];
#pragma unroll
		for (int k = 0; k < TQ; ++k) {
			const Site s = site_of(rat[row + q[k]], rcg[row + q[k]], min_depth);    /* the same for every lane */
			if (!s.informative) continue;
			const bool carries = (s.major_at ? sg : sa) > min_cov, has_major = (s.major_at ? sa : sg) > min_cov;
			const bool in[3] = { !carries && has_major, carries && has_major, carries && !has_major };   /* lack, het, opp; neither: a miss of the source */
#pragma unroll
			for (int c = 0; c < 3; ++c) {
				minor[k][c] += in[c] ? s.m : 0;
				depth[k][c] += in[c] ? s.t : 0;
				sites[k][c] += in[c];
			}
		}
	}
	if (d >= n_cols) return;
#pragma unroll
	for (int k = 0; k < TQ; ++k) {
		if (q0 + k >= n_rows) continue;
		ntsm_eval_contam_record r;
#pragma unroll
		for (int c = 0; c < 3; ++c) { r.minor[c] = minor[k][c]; r.depth[c] = depth[k][c]; r.sites[c] = sites[k][c]; }
		r.pad = 0;
		out[(uint64_t) (q0 + k) * out_pitch + d] = r;
	}
}

/* The band's rows against the window's columns, into columns cols.first ... of d_out [rows.count][n_db]; timed into *ms (added).
 * Width and target group: ntsm_eval_chunk.h's launch rule, inherited and not measured again for this kernel. */
int launch_contam(const Window &rows, const Window &cols, uint32_t n_db, uint32_t n_sites, uint32_t min_cov, uint32_t min_depth, ntsm_eval_contam_record *d_out,
		hipEvent_t e0, hipEvent_t e1, double *ms)
{
	uint32_t width, tq;
	ntsm_eval_chunk::launch_shape(rows.count, cols.count, g_width, g_target_group, width, tq);
	const dim3 grid((cols.count + width - 1) / width, (rows.count + tq - 1) / tq);
	auto kernel = tq == 4 ? ntsm_eval_contam_kernel<4> : tq == 2 ? ntsm_eval_contam_kernel<2> : ntsm_eval_contam_kernel<1>;
	return ntsm_eval_chunk::timed(e0, e1, ms, [&] {
		hipLaunchKernelGGL(kernel, grid, dim3(width), 0, 0, rows.at, rows.cg, rows.pitch, rows.count, cols.at, cols.cg, cols.pitch, cols.count, n_sites, min_cov,
				min_depth, d_out + cols.first, (uint64_t) n_db);
		HIPCHK(hipGetLastError());
		return 0;
	});
}

}  // namespace

struct ntsm_eval_contam_session {
	const char *db = nullptr;
	uint64_t stride = 0;
	uint32_t n_db = 0, n_sites = 0, min_cov = 0, min_depth = 0;
	ntsm_eval_band::Holding<uint64_t> hold;  /* the store's samples as columns; their tallies are read as targets, by row */

	/* ntsm_eval_chunk::upload, then this file's transpose (no term plane) and, with `tallies`, its tallies */
	auto stager()
	{
		return [this](uint32_t first, uint32_t count, const Staged<uint64_t> &to, bool tallies, ntsm_eval_cross_times &tm) {
			const int rc = ntsm_eval_chunk::upload(db, stride, first, count, n_sites, to.raw, tm);
			if (rc) return rc;
			return ntsm_eval_chunk::timed(hold.ev[0], hold.ev[1], &tm.prepare_kernel_ms, [&] {
				ntsm_eval_chunk::for_grid_y_slices(((uint64_t) count + kTile - 1) / kTile, [&](uint64_t tile, uint32_t tiles) {
					hipLaunchKernelGGL(ntsm_eval_contam_transpose_kernel, dim3((n_sites + kTile - 1) / kTile, tiles), dim3(kThreads), 0, 0, (const uint2 *) to.raw, count,
							n_sites, (uint32_t) (tile * kTile), to.at, to.cg);
				});
				HIPCHK(hipGetLastError());
				if (tallies) {
					hipLaunchKernelGGL(ntsm_eval_contam_tally_kernel, dim3(count), dim3(kThreads), 0, 0, (const uint2 *) to.raw, n_sites, min_depth,
							(unsigned long long *) to.tally);
					HIPCHK(hipGetLastError());
				}
				return 0;
			});
		};
	}
};

extern "C" int ntsm_eval_contam_tune(uint32_t width, uint32_t target_group)
{
	if ((width != 0 && width != 64 && width != 256) || (target_group != 0 && target_group != 1 && target_group != 2 && target_group != 4)) return -1;
	g_width = width;
	g_target_group = target_group;
	return 0;
}

extern "C" int ntsm_eval_contam_open(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n_db, uint32_t n_sites, uint32_t min_cov,
		uint32_t min_depth, uint32_t db_chunk, ntsm_eval_contam_session **h)
{
	if (!h) return -1;
	*h = nullptr;
	if (!ntsm_eval_chunk::valid_store(db_counts, db_stride_bytes, n_db, n_sites)) return -1;
	std::unique_ptr<ntsm_eval_contam_session> s(new ntsm_eval_contam_session);
	s->db = (const char *) db_counts;
	s->stride = db_stride_bytes;
	s->n_db = n_db; s->n_sites = n_sites; s->min_cov = min_cov; s->min_depth = min_depth;
	if (n_db == 0 || n_sites == 0) { *h = s.release(); return 0; }                /* nothing to sum: no device work, here or in _rows */

	/* 16 bytes per sample and site: at and cg, and the dense copy the transpose reads; and the tallies.  A streamed walk takes
	 * none per chunk: the tallies are the targets', staged with a band's rows. */
	int rc = s->hold.open(device, n_db, n_sites, n_sites, db_chunk, 2 * 8ull * n_sites + 3 * sizeof(uint64_t), false, false);
	if (rc || (rc = s->hold.fill(s->stager())) != 0) return rc;
	*h = s.release();
	return 0;
}

extern "C" void ntsm_eval_contam_close(ntsm_eval_contam_session *h)
{
	delete h;
}

extern "C" int ntsm_eval_contam_rows(ntsm_eval_contam_session *h, uint32_t row_first, uint32_t n_rows, ntsm_eval_contam_record *out, uint64_t *tally,
		ntsm_eval_cross_times *times)
{
	if (times) *times = ntsm_eval_cross_times {};
	if (!h || !out || n_rows == 0 || (uint64_t) row_first + n_rows > h->n_db) return -1;
	const uint32_t n_db = h->n_db, n_sites = h->n_sites;
	const uint64_t records = (uint64_t) n_rows * n_db;
	if (!h->hold.device_work) {                                                  /* no site; n_db == 0 has no range to take */
		memset(out, 0, records * sizeof(ntsm_eval_contam_record));
		if (tally) memset(tally, 0, (size_t) n_rows * 3 * sizeof(uint64_t));
		return 0;
	}
	HIPCHK(hipSetDevice(h->hold.device));
	ntsm_hip::Buffers b;                                                          /* this call's: streamed, the band's rows */
	ntsm_eval_cross_times tm = h->hold.take_open_times();
	Window rows;
	int rc = h->hold.band_rows(b, row_first, n_rows, tally, h->stager(), tm, rows);
	if (rc) return rc;
	rc = h->hold.walk(0, records, out, nullptr, h->stager(), [&](const Window &cols, ntsm_eval_contam_record *d_out) {
		return launch_contam(rows, cols, n_db, n_sites, h->min_cov, h->min_depth, d_out, h->hold.ev[0], h->hold.ev[1], &tm.cross_kernel_ms);
	}, tm);
	if (rc) return rc;
	if (times) *times = tm;
	return 0;
}
