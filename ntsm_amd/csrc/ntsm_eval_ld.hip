/*
 * ntsm_eval_ld.hip -- site-pair LD over a cohort store on one MI355X (include/ntsm_eval_hip.h: ntsm_eval_ld_open / _rows /
 * _select / _close; ntsmEval --ld).  The transpose of ntsm_eval_trio.hip: the store is streamed once, at
 * open, into three bit-planes -- het, hom_cg, called, one bit per site and sample, 64 samples to a word -- and the counts go back.
 * The record of a site pair is then eight popcounts over sample words, and the rectangle sites x sites is a popcount "GEMM" with
 * K = sample words.  Every sum is an integer sum: no rounding, no order, and two calls give the same bytes.
 *
 * Layout.  planes [plane][sample word][site], uint64, the site index fastest: the rectangle kernel stages a tile's sites of one
 * word as one coalesced run, and the builder's lanes (sites across the lanes) write one.  Bits past n_db in the last word are
 * zero in all three planes, so no kernel masks a tail.
 *
 * Kernels.
 *   planes   a lane is a site, a workgroup 256 sites of one sample word: over the samples of that word that the chunk holds, a
 *            wave's load along the sites of one sample is one coalesced 512-byte read and every lane shifts its own class bits into
 *            its own three words -- no ballot (it would reduce along the sites) and no LDS.  A chunk may start and end anywhere: a
 *            word that two chunks share is completed by OR, the launches being in order on one stream.
 *   geno     popcounts of the planes per site, sites across the lanes.
 *   ld       one workgroup of 16 x 16 lanes takes a tile of (16 RR) row sites x (16 RC) column sites, stages both sides' plane
 *            words through LDS in slabs of kSlab sample words, and every lane keeps an RR x RC register block of pairs, eight 32-bit
 *            counts each: per pair and word 9 ANDs, 1 OR and 8 popcounts of 64 bits.  The row side's words are the same address for
 *            the 16 lanes of one ty (a broadcast), the column side is a run of RC words per lane, 16 lanes covering the 64 banks
 *            once: both free of bank conflicts.  Two instances of the one body: _rows stores the dense records; _select skips the
 *            tiles below the diagonal, tests every pair a < b in registers (eval_ld.hpp's expressions) and appends the selected
 *            ones through one atomic add per wave.
 * One stream, no overlap.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>

#include "../../include/ntsm_eval_hip.h"
#define NTSM_HIP_TAG "ntsm_eval_ld"
#include "host/eval_ld.hpp"
#include "ntsm_eval_chunk.h"
#include "ntsm_eval_geno.h"
#include "ntsm_hip_scope.h"

namespace {

using ntsm_eval_chunk::kThreads;
using ntsm_eval_chunk::timed;
constexpr int kSlab = 8;                     /* sample words per LDS slab: ntsm_eval_trio.hip's, inherited and not measured here */
constexpr int kTX = 16;                      /* the workgroup is kTX x kTX lanes */
constexpr uint32_t kMaxGridY = 65535;

uint32_t g_rr = 0, g_rc = 0;                 /* ntsm_eval_ld_tune */

/* counts [count][site][2] (dense) of samples first ... first + count - 1 -> their bits in planes [3][n_words][n_sites].
 * grid (sites / 256, sample words of the chunk from w_first on) */
__global__ __launch_bounds__(kThreads) void ntsm_eval_ld_planes_kernel(const uint2 *__restrict__ counts, uint32_t count, uint32_t n_sites, uint32_t min_cov,
		uint32_t min_depth, uint32_t first, uint32_t w_first, uint32_t n_words, uint64_t *__restrict__ planes)
{
	const uint32_t site = blockIdx.x * kThreads + threadIdx.x;
	const uint32_t w = w_first + blockIdx.y;
	if (site >= n_sites) return;
	const uint32_t lo = std::max(first, w * 64), hi = std::min(first + count, w * 64 + 64);   /* n_db <= 2^24: no wrap */
	uint64_t het = 0, cg = 0, called = 0;
#pragma unroll 8
	for (uint32_t s = lo; s < hi; ++s) {
		const uint2 c = counts[(uint64_t) (s - first) * n_sites + site];
		const int cls = ntsm_eval_class_of(c.x, c.y, min_cov, min_depth);
		const uint64_t bit = 1ull << (s & 63);
		het |= cls == 1 ? bit : 0;
		cg |= cls == 2 ? bit : 0;
		called |= cls != 3 ? bit : 0;
	}
	const uint64_t plane = (uint64_t) n_words * n_sites, at = (uint64_t) w * n_sites + site;
	planes[at] |= het;
	planes[plane + at] |= cg;
	planes[2 * plane + at] |= called;
}

/* geno [n_sites][4] = het, homCG, called, homAT: the popcounts of the planes of every site */
__global__ __launch_bounds__(kThreads) void ntsm_eval_ld_geno_kernel(const uint64_t *__restrict__ planes, uint32_t n_sites, uint32_t n_words, uint32_t *__restrict__ geno)
{
	const uint32_t site = blockIdx.x * kThreads + threadIdx.x;
	if (site >= n_sites) return;
	const uint64_t plane = (uint64_t) n_words * n_sites;
	uint32_t c[3] = { 0, 0, 0 };
	for (uint32_t w = 0; w < n_words; ++w) {
		const uint64_t *row = planes + (uint64_t) w * n_sites + site;
#pragma unroll
		for (int pl = 0; pl < 3; ++pl) c[pl] += __popcll(row[pl * plane]);
	}
	uint32_t *g = geno + 4ull * site;
	g[0] = c[0]; g[1] = c[1]; g[2] = c[2]; g[3] = c[2] - c[0] - c[1];
}

/* acc + popcount(v) in two instructions: v_bcnt_u32_b32 takes the running sum as its addend.  Written as the instruction itself:
 * from `acc += __popcll(v)` the compiler forms two counts from zero and a three-operand add, half as much again. */
__device__ inline uint32_t bcnt(uint32_t v, uint32_t acc)
{
	uint32_t r;
	asm("v_bcnt_u32_b32 %0, %1, %2" : "=v"(r) : "v"(v), "v"(acc));
	return r;
}
__device__ inline uint32_t count_into(uint32_t acc, uint64_t v) { return bcnt((uint32_t) (v >> 32), bcnt((uint32_t) v, acc)); }

/* what the _select instance needs beside the planes */
struct Select {
	uint32_t min_called;
	double r2_min;
	uint64_t cap;                            /* pairs `out` holds */
	ntsm_eval_ld_pair *out;
	unsigned long long *found;               /* counts every selected pair, also those beyond cap */
};

/* grid (column tiles from tile_col0 on, row tiles from tile_row0 on); rows are sites row_first + r, r < n_rows; columns every
 * site.  Lane (tx, ty) holds rows r0 + ty * RR + r and columns c0 + tx * RC + c. */
template <int RR, int RC, bool SELECT> __global__ __launch_bounds__(kTX * kTX) void ntsm_eval_ld_kernel(const uint64_t *__restrict__ planes, uint32_t n_sites,
		uint32_t n_words, uint32_t row_first, uint32_t n_rows, uint32_t tile_row0, uint32_t tile_col0, ntsm_eval_ld_record *__restrict__ out, Select sel)
{
	constexpr int TR = kTX * RR, TC = kTX * RC, kBlock = kTX * kTX;
	__shared__ uint64_t srow[kSlab][3][TR], scol[kSlab][3][TC];                      /* [word][het, hom_cg, called][site of the tile] */
	const uint32_t r0 = (tile_row0 + blockIdx.y) * TR;                               /* relative to row_first; < n_rows */
	const uint64_t c0 = (uint64_t) (tile_col0 + blockIdx.x) * TC;                    /* < n_sites */
	if (SELECT && c0 + TC - 1 <= (uint64_t) row_first + r0) return;                  /* the tile holds no pair a < b: the whole workgroup leaves */
	const uint32_t tx = threadIdx.x % kTX, ty = threadIdx.x / kTX;
	uint32_t acc[RR][RC][8];
#pragma unroll
	for (int r = 0; r < RR; ++r)
#pragma unroll
		for (int c = 0; c < RC; ++c)
#pragma unroll
			for (int k = 0; k < 8; ++k) acc[r][c][k] = 0;
	const uint64_t plane = (uint64_t) n_words * n_sites;
	for (uint32_t w0 = 0; w0 < n_words; w0 += kSlab) {
		__syncthreads();                                                           /* the slab before this one has been read */
		for (uint32_t idx = threadIdx.x; idx < (uint32_t) (kSlab * 3 * (TR + TC)); idx += kBlock) {
			const bool col = idx >= (uint32_t) (kSlab * 3 * TR);
			const uint32_t j = col ? idx - kSlab * 3 * TR : idx, T = col ? TC : TR;
			const uint32_t w = j / (3 * T), pl = j % (3 * T) / T, i = j % T;
			const uint64_t site = col ? c0 + i : (uint64_t) row_first + r0 + i;
			const bool in = col ? site < n_sites : r0 + i < n_rows;                  /* past the band, the sites or the last word: nothing is counted */
			uint64_t v = 0;
			if (in && w0 + w < n_words) v = planes[pl * plane + (uint64_t) (w0 + w) * n_sites + site];
			(col ? &scol[0][0][0] : &srow[0][0][0])[j] = v;
		}
		__syncthreads();
#pragma unroll 1
		for (int w = 0; w < kSlab; ++w) {
			uint64_t Hs[RR], Gs[RR], Cs[RR], Ht[RC], Gt[RC], Ct[RC];
#pragma unroll
			for (int r = 0; r < RR; ++r) { Hs[r] = srow[w][0][ty * RR + r]; Gs[r] = srow[w][1][ty * RR + r]; Cs[r] = srow[w][2][ty * RR + r]; }
#pragma unroll
			for (int c = 0; c < RC; ++c) { Ht[c] = scol[w][0][tx * RC + c]; Gt[c] = scol[w][1][tx * RC + c]; Ct[c] = scol[w][2][tx * RC + c]; }
#pragma unroll
			for (int r = 0; r < RR; ++r)
#pragma unroll
				for (int c = 0; c < RC; ++c) {
					uint32_t *a = acc[r][c];
					a[0] = count_into(a[0], Cs[r] & Ct[c]);
					a[1] = count_into(a[1], Hs[r] & Ct[c]);
					a[2] = count_into(a[2], Gs[r] & Ct[c]);
					a[3] = count_into(a[3], Cs[r] & Ht[c]);
					a[4] = count_into(a[4], Cs[r] & Gt[c]);
					a[5] = count_into(a[5], Hs[r] & Ht[c]);
					a[6] = count_into(a[6], (Hs[r] & Gt[c]) | (Gs[r] & Ht[c]));
					a[7] = count_into(a[7], Gs[r] & Gt[c]);
				}
		}
	}
	if (!SELECT) {
#pragma unroll
		for (int r = 0; r < RR; ++r)
#pragma unroll
			for (int c = 0; c < RC; ++c) {
				const uint32_t row = r0 + ty * RR + r;
				const uint64_t colm = c0 + tx * RC + c;
				if (row >= n_rows || colm >= n_sites) continue;
				const uint32_t *a = acc[r][c];
				out[(uint64_t) row * n_sites + colm] = ntsm_eval_ld_record { a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7] };
			}
		return;
	}
	/* the selected pairs of this lane, their places in the wave by a prefix sum, and one atomic add for the wave */
	uint32_t mask = 0;
#pragma unroll
	for (int r = 0; r < RR; ++r)
#pragma unroll
		for (int c = 0; c < RC; ++c) {
			const uint32_t row = r0 + ty * RR + r;
			const uint64_t b = c0 + tx * RC + c;
			const uint32_t *a = acc[r][c];
			const ntsm_eval_ld_record rec { a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7] };
			if (row < n_rows && b < n_sites && (uint64_t) row_first + row < b && ntsm::eval_ld::selected(rec, sel.min_called, sel.r2_min)) mask |= 1u << (r * RC + c);
		}
	const uint32_t lane = threadIdx.x % 64, mine = __popc(mask);
	uint32_t incl = mine;
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t t = __shfl_up(incl, d);
		if (lane >= (uint32_t) d) incl += t;
	}
	const uint32_t total = __shfl(incl, 63);
	if (total == 0) return;                                                        /* wave-uniform */
	uint32_t lo = 0, hi = 0;
	if (lane == 63) {
		const unsigned long long base = atomicAdd(sel.found, (unsigned long long) total);
		lo = (uint32_t) base; hi = (uint32_t) (base >> 32);
	}
	lo = __shfl(lo, 63); hi = __shfl(hi, 63);
	uint64_t pos = ((uint64_t) hi << 32 | lo) + incl - mine;
#pragma unroll
	for (int r = 0; r < RR; ++r)
#pragma unroll
		for (int c = 0; c < RC; ++c) {
			if (!(mask >> (r * RC + c) & 1)) continue;
			if (pos < sel.cap) {
				const uint32_t *a = acc[r][c];
				ntsm_eval_ld_pair p;
				p.a = row_first + r0 + ty * RR + r;
				p.b = (uint32_t) (c0 + tx * RC + c);
				p.rec = ntsm_eval_ld_record { a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7] };
				sel.out[pos] = p;
			}
			++pos;
		}
}

/* the register block of a call: the forced one, or 2 x 2 -- 32 accumulators and five to seven waves on a SIMD.  The loop waits for
 * its LDS reads every word and for two barriers every slab, so the waves that hide that count for more than the operand reuse of
 * a larger block: measured 4 % faster than 4 x 2 and 6 % faster than 2 x 4 on the triangle of 96,287 sites */
void block_of(uint32_t &rr, uint32_t &rc)
{
	rr = g_rr ? g_rr : 2;
	rc = g_rc ? g_rc : 2;
}

/* the launches of one call: every row tile of the band, in slices of what a grid's y takes */
template <int RR, int RC, bool SELECT> int launch(const uint64_t *planes, uint32_t n_sites, uint32_t n_words, uint32_t row_first, uint32_t n_rows,
		ntsm_eval_ld_record *out, const Select &sel)
{
	constexpr uint32_t TR = kTX * RR, TC = kTX * RC;
	const uint32_t row_tiles = (n_rows + TR - 1) / TR;
	const uint32_t col0 = SELECT ? (uint32_t) (((uint64_t) row_first + 1) / TC) : 0;   /* the first column tile that holds a b > row_first */
	const uint32_t col_tiles = (uint32_t) (((uint64_t) n_sites + TC - 1) / TC);
	if (col0 >= col_tiles) return 0;                                               /* the band is the last site alone: it has no pair */
	for (uint32_t t = 0; t < row_tiles; t += kMaxGridY) {
		hipLaunchKernelGGL((ntsm_eval_ld_kernel<RR, RC, SELECT>), dim3(col_tiles - col0, std::min(kMaxGridY, row_tiles - t)), dim3(kTX * kTX), 0, 0, planes, n_sites, n_words,
				row_first, n_rows, t, col0, out, sel);
		HIPCHK(hipGetLastError());
	}
	return 0;
}

template <bool SELECT> int launch_block(const uint64_t *planes, uint32_t n_sites, uint32_t n_words, uint32_t row_first, uint32_t n_rows, ntsm_eval_ld_record *out,
		const Select &sel)
{
	uint32_t rr, rc;
	block_of(rr, rc);
	if (rr == 2 && rc == 2) return launch<2, 2, SELECT>(planes, n_sites, n_words, row_first, n_rows, out, sel);
	if (rr == 2) return launch<2, 4, SELECT>(planes, n_sites, n_words, row_first, n_rows, out, sel);
	return launch<4, 2, SELECT>(planes, n_sites, n_words, row_first, n_rows, out, sel);
}

}  // namespace

struct ntsm_eval_ld_session {
	int device = 0;
	uint32_t n_db = 0, n_sites = 0, n_words = 0;
	ntsm_hip::Buffers b;
	ntsm_hip::Events<2> ev;
	uint64_t *d_planes = nullptr;            /* [3][n_words][n_sites]; NULL: a session without device work */
};

extern "C" int ntsm_eval_ld_tune(uint32_t block_rows, uint32_t block_cols)
{
	const bool ok = (block_rows == 0 && block_cols == 0) || (block_rows == 2 && block_cols == 2) || (block_rows == 4 && block_cols == 2) || (block_rows == 2 && block_cols == 4);
	if (!ok) return -1;
	g_rr = block_rows; g_rc = block_cols;
	return 0;
}

extern "C" int ntsm_eval_ld_open(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n_db, uint32_t n_sites, uint32_t min_cov,
		uint32_t min_depth, uint32_t db_chunk, uint32_t *site_geno, ntsm_eval_cross_times *times, ntsm_eval_ld_session **h)
{
	if (times) *times = ntsm_eval_cross_times {};
	if (!h) return -1;
	*h = nullptr;
	if (!ntsm_eval_chunk::valid_store(db_counts, db_stride_bytes, n_db, n_sites) || n_db > NTSM_EVAL_LD_MAX_SAMPLES) return -1;
	std::unique_ptr<ntsm_eval_ld_session> s(new ntsm_eval_ld_session);
	s->device = device;
	s->n_db = n_db; s->n_sites = n_sites;
	s->n_words = (n_db + 63) / 64;
	if (n_db == 0 || n_sites == 0) {                                               /* nothing to class: no device work, here or later */
		if (site_geno) memset(site_geno, 0, (size_t) n_sites * 4 * sizeof(uint32_t));
		*h = s.release();
		return 0;
	}
	const uint32_t n_words = s->n_words;
	const uint64_t plane_words = 3ull * n_words * n_sites;
	ntsm_eval_cross_times tm {};
	HIPCHK(hipSetDevice(device));
	HIPCHK(s->ev.create());
	HIPCHK(s->b.alloc(&s->d_planes, plane_words));
	HIPCHK(hipMemset(s->d_planes, 0, plane_words * sizeof(uint64_t)));               /* the builder ORs into them */
	/* what a staged chunk holds beside the planes, which are there already: its dense counts */
	size_t free_b = 0, total_b = 0;
	if (db_chunk == 0) HIPCHK(hipMemGetInfo(&free_b, &total_b));
	const uint32_t chunk = ntsm_eval_chunk::samples_per_pass(db_chunk, n_db, free_b, 8ull * n_sites, 0);
	ntsm_hip::Buffers b;                                                          /* open's own: the staging goes back when it returns */
	uint32_t *d_raw;
	HIPCHK(b.alloc(&d_raw, (uint64_t) chunk * n_sites * 2));
	const uint32_t site_blocks = (uint32_t) (((uint64_t) n_sites + kThreads - 1) / kThreads);
	for (uint32_t first = 0; first < n_db; first += chunk) {
		const uint32_t count = std::min(chunk, n_db - first);
		int rc = ntsm_eval_chunk::upload(db_counts, db_stride_bytes, first, count, n_sites, d_raw, tm);
		if (rc) return rc;
		const uint32_t w_lo = first / 64, w_hi = (first + count - 1) / 64;             /* the sample words this chunk has bits in */
		rc = timed(s->ev[0], s->ev[1], &tm.prepare_kernel_ms, [&] {                  /* it waits: the next chunk overwrites d_raw */
			for (uint32_t w = w_lo; w <= w_hi; w += kMaxGridY) {
				hipLaunchKernelGGL(ntsm_eval_ld_planes_kernel, dim3(site_blocks, std::min(kMaxGridY, w_hi - w + 1)), dim3(kThreads), 0, 0, (const uint2 *) d_raw, count,
						n_sites, min_cov, min_depth, first, w, n_words, s->d_planes);
				HIPCHK(hipGetLastError());
			}
			return 0;
		});
		if (rc) return rc;
		tm.chunks++;
	}
	if (site_geno) {
		uint32_t *d_geno;
		HIPCHK(b.alloc(&d_geno, (uint64_t) n_sites * 4));
		int rc = timed(s->ev[0], s->ev[1], &tm.prepare_kernel_ms, [&] {
			hipLaunchKernelGGL(ntsm_eval_ld_geno_kernel, dim3(site_blocks), dim3(kThreads), 0, 0, s->d_planes, n_sites, n_words, d_geno);
			HIPCHK(hipGetLastError());
			return 0;
		});
		if (rc || (rc = ntsm_eval_chunk::timed_copy(site_geno, d_geno, (size_t) n_sites * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, &tm.download_ms)) != 0) return rc;
	}
	if (times) *times = tm;
	*h = s.release();
	return 0;
}

extern "C" void ntsm_eval_ld_close(ntsm_eval_ld_session *h)
{
	if (!h) return;
	if (h->d_planes) (void) hipSetDevice(h->device);                              /* a session without device work touches no device here either */
	delete h;
}

extern "C" int ntsm_eval_ld_rows(ntsm_eval_ld_session *h, uint32_t row_first, uint32_t n_rows, ntsm_eval_ld_record *out, double *kernel_ms)
{
	if (kernel_ms) *kernel_ms = 0;
	if (!h || !out || n_rows == 0 || (uint64_t) row_first + n_rows > h->n_sites) return -1;
	const uint64_t records = (uint64_t) n_rows * h->n_sites;
	if (!h->d_planes) {                                                            /* no sample; n_sites == 0 has no range to take */
		memset(out, 0, records * sizeof(ntsm_eval_ld_record));
		return 0;
	}
	HIPCHK(hipSetDevice(h->device));
	ntsm_hip::Buffers b;
	ntsm_eval_ld_record *d_out;
	HIPCHK(b.alloc(&d_out, records));
	double ms = 0;
	const int rc = timed(h->ev[0], h->ev[1], &ms, [&] { return launch_block<false>(h->d_planes, h->n_sites, h->n_words, row_first, n_rows, d_out, Select {}); });
	if (rc) return rc;
	HIPCHK(hipMemcpy(out, d_out, records * sizeof(ntsm_eval_ld_record), hipMemcpyDeviceToHost));
	if (kernel_ms) *kernel_ms = ms;
	return 0;
}

extern "C" int ntsm_eval_ld_select(ntsm_eval_ld_session *h, uint32_t row_first, uint32_t n_rows, uint32_t min_called, double r2_min, uint64_t cap,
		ntsm_eval_ld_pair *out_pairs, uint64_t *n_found, double *kernel_ms)
{
	if (kernel_ms) *kernel_ms = 0;
	if (n_found) *n_found = 0;
	if (!h || !n_found || n_rows == 0 || (uint64_t) row_first + n_rows > h->n_sites || !std::isfinite(r2_min) || (cap && !out_pairs)) return -1;
	if (!h->d_planes) return 0;                                                    /* no sample: r^2 is defined nowhere */
	/* the pairs a < b the band holds: no call finds more, so the device's buffer is never larger */
	const uint64_t rows = n_rows, possible = rows * (h->n_sites - 1) - (rows * row_first + rows * (rows - 1) / 2);
	HIPCHK(hipSetDevice(h->device));
	ntsm_hip::Buffers b;
	Select sel { min_called, r2_min, std::min(cap, possible), nullptr, nullptr };
	HIPCHK(b.alloc(&sel.out, sel.cap));
	HIPCHK(b.alloc(&sel.found, 1));
	HIPCHK(hipMemset(sel.found, 0, sizeof(unsigned long long)));
	double ms = 0;
	const int rc = timed(h->ev[0], h->ev[1], &ms, [&] { return launch_block<true>(h->d_planes, h->n_sites, h->n_words, row_first, n_rows, nullptr, sel); });
	if (rc) return rc;
	unsigned long long found = 0;
	HIPCHK(hipMemcpy(&found, sel.found, sizeof(found), hipMemcpyDeviceToHost));
	*n_found = found;
	if (kernel_ms) *kernel_ms = ms;
	if (found > cap) return 1;
	if (found == 0) return 0;
	HIPCHK(hipMemcpy(out_pairs, sel.out, found * sizeof(ntsm_eval_ld_pair), hipMemcpyDeviceToHost));
	/* the waves append in the order they finish: the (a, b) order makes two calls the same bytes */
	std::sort(out_pairs, out_pairs + found, [](const ntsm_eval_ld_pair &x, const ntsm_eval_ld_pair &y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
	return 0;
}
