/*
 * ntsm_eval_between.hip -- one cohort store scored against another on one MI355X (include/ntsm_eval_hip.h:
 * ntsm_eval_between_open / _rows / _close / _tune; ntsmEval --between): the rectangle of pairs
 * (a, b), a a sample of store A and b a sample of store B, in bands of rows of A, each record bit for bit what
 * ntsm_eval_pairs gives for pair (a, n_a + b) of the dense concatenation [A; B remapped to A's sites].
 *
 * Rectangle tile.  The pair kernel's tile (ntsm_eval.hip) over two buffers, as ntsm_eval_within.hip restates it, without a
 * diagonal: B's samples go across the lanes, one coalesced 4 + 4 + 8-byte load per lane and site out of at / cg / term
 * [site][column]; kTI = 4 consecutive rows of A are wave-uniform (scalar loads) out of arrays of their own pitch; one
 * ntsm_eval_acc per pair walks the sites in order (ntsm_eval_score.h), so the sums are the reference's sequential sums.
 * Every pair of the rectangle is stored at [row][column]; lanes past the last column and rows past the band's end compute
 * a clamped copy and store nothing.
 *
 * Mapped staging.  A store takes its locus table from whatever built it, so B may list A's loci in another order and lack
 * some.  A window of B arrives dense as [sample][n_sites_b][2] by one 2-D copy from the store's stride; the transposing
 * kernel then writes at / cg / term [n_sites_a][window], reading B's site site_map[s] for A's site s and writing 0 / 0 with
 * the term of a 0 / 0 site where B lacks it, and the tallies are taken over the same remapped sites.  With identical tables
 * (site_map == NULL) the staging is ntsm_eval_chunk.h's as it is.
 *
 * Holdings.  B is resident when the chunk rule, asked at 24 bytes per sample and site of A, answers n_b: staged once at
 * open, the dense third released again.  Otherwise every _rows call walks B in chunks of b_chunk.  A's band is always
 * uploaded and transposed by the _rows call into a buffer of its own pitch.  The holding, the staging of a band's rows and
 * the walk are ntsm_eval_band.h's; what is here: the kernels, the launch, B's stager and the bytes per sample.  One stream,
 * no overlap.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>

#include "../../include/ntsm_eval_hip.h"
#include "host/eval_between.hpp"
#define NTSM_HIP_TAG "ntsm_eval_between"
#include "ntsm_eval_band.h"
#include "ntsm_eval_score.h"
#include "ntsm_hip_scope.h"

namespace {

using ntsm_eval_band::Staged;
using ntsm_eval_band::Window;
using ntsm_eval_chunk::kThreads;
using ntsm_eval_chunk::kTile;
using ntsm_eval_chunk::ms_since;
using ntsm_eval_chunk::timed_copy;
using ntsm_eval_chunk::valid_store;
using ntsm_eval_chunk::wall;
constexpr int kTI = 4;                       /* rows of A per workgroup, as in ntsm_eval.hip */
constexpr uint32_t kLacks = ntsm::eval_between::kLacks;
using ntsm_eval_chunk::kMaxGridY;

uint32_t g_width = 0;                        /* ntsm_eval_between_tune */

/* grid (columns / blockDim.x, rows / kTI).  rat / rcg / rterm [site][row_pitch]: n_rows rows of A; cat / ccg / cterm
 * [site][col_pitch]: n_cols samples of B.  out: the record of (row r, column c) at out[r * out_pitch + c]. */
__global__ __launch_bounds__(kThreads) void ntsm_eval_between_kernel(const uint32_t *__restrict__ rat, const uint32_t *__restrict__ rcg,
		const double *__restrict__ rterm, uint32_t row_pitch, uint32_t n_rows, const uint32_t *__restrict__ cat, const uint32_t *__restrict__ ccg,
		const double *__restrict__ cterm, uint32_t col_pitch, uint32_t n_cols, uint32_t n_sites, uint32_t min_cov, ntsm_eval_record *__restrict__ out,
		uint64_t out_pitch)
{
	const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t r0 = blockIdx.y * kTI;
	const uint32_t cc = c < n_cols ? c : n_cols - 1;                             /* lanes past the end compute a copy of the last column, not stored */
	uint32_t r[kTI];
#pragma unroll
	for (int ii = 0; ii < kTI; ++ii) r[ii] = r0 + ii < n_rows ? r0 + ii : n_rows - 1;   /* wave-uniform: scalar loads; past the band's end a copy of its last row */
	ntsm_eval_acc acc[kTI];
	for (uint32_t site = 0; site < n_sites; ++site) {
		const uint64_t col = (uint64_t) site * col_pitch + cc, row = (uint64_t) site * row_pitch;
		const ntsm_eval_side sb = ntsm_eval_side_of(cat[col], ccg[col], cterm[col], min_cov);
#pragma unroll
		for (int ii = 0; ii < kTI; ++ii) acc[ii].add(ntsm_eval_side_of(rat[row + r[ii]], rcg[row + r[ii]], rterm[row + r[ii]], min_cov), sb, min_cov);
	}
	if (c >= n_cols) return;
#pragma unroll
	for (int ii = 0; ii < kTI; ++ii)
		if (r0 + ii < n_rows) out[(uint64_t) (r0 + ii) * out_pitch + c] = acc[ii].record();
}

/* counts [sample][n_sites_b][2] (dense) -> at / cg / term [n_sites_a][sample] through the map: ntsm_eval_chunk.h's
 * prepare_kernel with the read side gathered.  Lanes run along A's sites of one sample, so the reads are coalesced wherever
 * the map is locally monotone; the writes run along the samples of one site and are always coalesced. */
__global__ __launch_bounds__(kThreads) void ntsm_eval_between_prepare_kernel(const uint2 *__restrict__ counts, const uint32_t *__restrict__ site_map,
		uint32_t n_samples, uint32_t n_sites_a, uint32_t n_sites_b, uint32_t min_cov, uint32_t s_first, uint32_t *__restrict__ at, uint32_t *__restrict__ cg,
		double *__restrict__ term)
{
	__shared__ uint2 tile[kTile][kTile + 1];
	const uint32_t m0 = blockIdx.x * kTile, s0 = s_first + blockIdx.y * kTile;
	const uint32_t lo = threadIdx.x % kTile, hi = threadIdx.x / kTile;
	const uint32_t from = m0 + lo < n_sites_a ? site_map[m0 + lo] : kLacks;      /* this lane's site of B in the first phase */
	for (uint32_t r = hi; r < (uint32_t) kTile; r += kThreads / kTile) {
		const uint32_t s = s0 + r;
		if (s < n_samples) tile[r][lo] = from != kLacks ? counts[(uint64_t) s * n_sites_b + from] : make_uint2(0u, 0u);
	}
	__syncthreads();
	for (uint32_t r = hi; r < (uint32_t) kTile; r += kThreads / kTile) {
		const uint32_t s = s0 + lo, site = m0 + r;
		if (s >= n_samples || site >= n_sites_a) continue;
		const uint2 c = tile[lo][r];
		const uint64_t cell = (uint64_t) site * n_samples + s;
		at[cell] = c.x;
		cg[cell] = c.y;
		term[cell] = ntsm_eval_term(c.x, c.y, min_cov);
	}
}

/* ntsm_eval_chunk.h's tally_kernel over A's sites: a site B lacks is a missing site */
__global__ __launch_bounds__(kThreads) void ntsm_eval_between_tally_kernel(const uint2 *__restrict__ counts, const uint32_t *__restrict__ site_map,
		uint32_t n_sites_a, uint32_t n_sites_b, uint32_t min_cov, uint32_t *__restrict__ geno)
{
	__shared__ uint32_t sum[3];
	if (threadIdx.x < 3) sum[threadIdx.x] = 0;
	__syncthreads();
	const uint2 *row = counts + (uint64_t) blockIdx.x * n_sites_b;
	uint32_t hets = 0, homs = 0, miss = 0;
	for (uint32_t site = threadIdx.x; site < n_sites_a; site += kThreads) {
		const uint32_t from = site_map[site];
		const uint2 c = from != kLacks ? row[from] : make_uint2(0u, 0u);
		const bool a = c.x > min_cov, b = c.y > min_cov;
		hets += a && b;
		homs += a != b;
		miss += !a && !b;
	}
	atomicAdd(&sum[0], hets);
	atomicAdd(&sum[1], homs);
	atomicAdd(&sum[2], miss);
	__syncthreads();
	if (threadIdx.x < 3) geno[(uint64_t) blockIdx.x * 3 + threadIdx.x] = sum[threadIdx.x];
}

/* the pairs of the rows with the columns into d_out [rows.count][out_pitch] from column cols.first on, timed into *ms (added) */
int launch_between(const Window &rows, const Window &cols, uint32_t n_sites, uint32_t min_cov, ntsm_eval_record *d_out, uint64_t out_pitch, hipEvent_t e0,
		hipEvent_t e1, double *ms)
{
	/* 256 threads, unlike ntsm_eval_cross and ntsm_eval_within: on 1,024 rows x 4,096 columns x 96,287 sites they take 777 ms
	 * against 817 ms for 64 (three alternating runs each, spreads 11 and 14 ms).  A launch of at most
	 * 256 columns keeps one-wave workgroups: a wider one would only add waves that compute clamped copies.  Nothing between
	 * 256 and 4,096 columns has been measured.  ntsm_eval_between_tune forces either width. */
	const unsigned bt = g_width ? g_width : cols.count > 256 ? 256 : 64;
	return ntsm_eval_chunk::timed(e0, e1, ms, [&] {
		for (uint32_t y0 = 0; y0 < rows.count; y0 += kMaxGridY * kTI) {             /* a grid's second dimension ends at 65,535 */
			const uint32_t yn = std::min<uint32_t>(rows.count - y0, kMaxGridY * kTI);
			hipLaunchKernelGGL(ntsm_eval_between_kernel, dim3((cols.count + bt - 1) / bt, (yn + kTI - 1) / kTI), dim3(bt), 0, 0, rows.at + y0, rows.cg + y0,
					rows.term + y0, rows.pitch, yn, cols.at, cols.cg, cols.term, cols.pitch, cols.count, n_sites, min_cov,
					d_out + (uint64_t) y0 * out_pitch + cols.first, out_pitch);
			HIPCHK(hipGetLastError());
		}
		return 0;
	});
}

}  // namespace

struct ntsm_eval_between_session {
	const char *a = nullptr, *b = nullptr;
	uint64_t a_stride = 0, b_stride = 0;
	uint32_t n_a = 0, n_b = 0, n_sites_a = 0, n_sites_b = 0, min_cov = 0;
	ntsm_eval_band::Holding<uint32_t> hold;  /* B over A's sites as columns, with its hets, homs, miss; its buffers hold the map too */
	uint32_t *d_map = nullptr;

	/* A's rows: ntsm_eval_chunk.h's staging of a window as it is */
	auto stager_a()
	{
		return [this](uint32_t first, uint32_t count, const Staged<uint32_t> &to, bool tallies, ntsm_eval_cross_times &tm) {
			return ntsm_eval_band::stage_scored(a, a_stride, first, count, n_sites_a, min_cov, to, tallies, hold.ev[0], hold.ev[1], tm);
		};
	}

	/* B's samples over A's sites.  Identical tables: as A's.  Mapped: the 2-D copy of B's own n_sites_b-wide rows, then this
	 * file's gathering transpose and tallies. */
	auto stager_b()
	{
		return [this](uint32_t first, uint32_t count, const Staged<uint32_t> &to, bool tallies, ntsm_eval_cross_times &tm) {
			if (!d_map) return ntsm_eval_band::stage_scored(b, b_stride, first, count, n_sites_a, min_cov, to, tallies, hold.ev[0], hold.ev[1], tm);
			const uint64_t row_bytes = 8ull * n_sites_b;
			const auto t = wall::now();
			if (row_bytes) HIPCHK(hipMemcpy2D(to.raw, row_bytes, b + (uint64_t) first * b_stride, b_stride, row_bytes, count, hipMemcpyHostToDevice));
			tm.upload_ms += ms_since(t);
			return ntsm_eval_chunk::timed(hold.ev[0], hold.ev[1], &tm.prepare_kernel_ms, [&] {
				ntsm_eval_chunk::for_grid_y_slices(((uint64_t) count + kTile - 1) / kTile, [&](uint64_t tile, uint32_t tiles) {
					hipLaunchKernelGGL(ntsm_eval_between_prepare_kernel, dim3((n_sites_a + kTile - 1) / kTile, tiles), dim3(kThreads), 0, 0, (const uint2 *) to.raw, d_map,
							count, n_sites_a, n_sites_b, min_cov, (uint32_t) (tile * kTile), to.at, to.cg, to.term);
				});
				HIPCHK(hipGetLastError());
				if (tallies) {
					hipLaunchKernelGGL(ntsm_eval_between_tally_kernel, dim3(count), dim3(kThreads), 0, 0, (const uint2 *) to.raw, d_map, n_sites_a, n_sites_b, min_cov,
							to.tally);
					HIPCHK(hipGetLastError());
				}
				return 0;
			});
		};
	}
};

extern "C" int ntsm_eval_between_tune(uint32_t width)
{
	if (width != 0 && width != 64 && width != 256) return -1;
	g_width = width;
	return 0;
}

extern "C" int ntsm_eval_between_open(int device, const void *a_counts, uint64_t a_stride_bytes, uint32_t n_a, const void *b_counts, uint64_t b_stride_bytes,
		uint32_t n_b, uint32_t n_sites_a, uint32_t n_sites_b, const uint32_t *site_map, uint32_t min_cov, uint32_t b_chunk, ntsm_eval_between_session **h)
{
	if (!h) return -1;
	*h = nullptr;
	if (!valid_store(a_counts, a_stride_bytes, n_a, n_sites_a) || !valid_store(b_counts, b_stride_bytes, n_b, n_sites_b)) return -1;
	if (site_map ? !ntsm::eval_between::valid_map(site_map, n_sites_a, n_sites_b) : n_sites_a != n_sites_b) return -1;
	std::unique_ptr<ntsm_eval_between_session> s(new ntsm_eval_between_session);
	s->a = (const char *) a_counts; s->a_stride = a_stride_bytes; s->n_a = n_a; s->n_sites_a = n_sites_a;
	s->b = (const char *) b_counts; s->b_stride = b_stride_bytes; s->n_b = n_b; s->n_sites_b = n_sites_b;
	s->min_cov = min_cov;
	if (n_a == 0 || n_b == 0 || n_sites_a == 0) { *h = s.release(); return 0; }   /* nothing to score: no device work, here or in _rows */

	/* 24 bytes per sample and site of A: the transposed 16 and the dense 8 (a map that leaves sites of B unnamed may make the dense third the larger) */
	int rc = s->hold.open(device, n_b, n_sites_a, n_sites_b, b_chunk, 16ull * n_sites_a + 8ull * std::max(n_sites_a, n_sites_b) + 12, true, true);
	if (rc) return rc;
	if (site_map) {
		HIPCHK(s->hold.b.alloc(&s->d_map, n_sites_a));
		if ((rc = timed_copy(s->d_map, site_map, (size_t) n_sites_a * sizeof(uint32_t), hipMemcpyHostToDevice, &s->hold.open_times.upload_ms)) != 0) return rc;
	}
	if ((rc = s->hold.fill(s->stager_b())) != 0) return rc;
	*h = s.release();
	return 0;
}

extern "C" void ntsm_eval_between_close(ntsm_eval_between_session *h)
{
	delete h;
}

extern "C" int ntsm_eval_between_rows(ntsm_eval_between_session *h, uint32_t row_first, uint32_t n_rows, ntsm_eval_record *out, uint32_t *a_geno,
		uint32_t *b_geno, ntsm_eval_cross_times *times)
{
	if (times) *times = ntsm_eval_cross_times {};
	if (!h || (uint64_t) row_first + n_rows > h->n_a) return -1;
	if (n_rows == 0 && h->n_a != 0) return -1;                                   /* of a store A without samples, (0, 0) is the one range there is */
	const uint32_t n_b = h->n_b, n_sites = h->n_sites_a, min_cov = h->min_cov;
	const uint64_t records = (uint64_t) n_rows * n_b;
	if (!out && records) return -1;
	if (!h->hold.device_work) {
		if (records) memset(out, 0, records * sizeof(ntsm_eval_record));
		if (a_geno && n_rows) memset(a_geno, 0, (size_t) n_rows * 3 * sizeof(uint32_t));
		if (b_geno && n_b) memset(b_geno, 0, (size_t) n_b * 3 * sizeof(uint32_t));
		return 0;
	}
	HIPCHK(hipSetDevice(h->hold.device));
	ntsm_hip::Buffers b;                                                          /* this call's: the band's rows, always staged: they are A's */
	ntsm_eval_cross_times tm = h->hold.take_open_times();
	Window rows;
	int rc = ntsm_eval_band::stage_rows(b, row_first, n_rows, n_sites, true, a_geno, h->stager_a(), tm, rows);
	if (rc) return rc;
	rc = h->hold.walk(0, records, out, b_geno, h->stager_b(), [&](const Window &cols, ntsm_eval_record *d_out) {
		return launch_between(rows, cols, n_sites, min_cov, d_out, n_b, h->hold.ev[0], h->hold.ev[1], &tm.cross_kernel_ms);
	}, tm);
	if (rc) return rc;
	if (times) *times = tm;
	return 0;
}
