/*
 * ntsm_eval_trio.hip -- parent-parent-child trios in a cohort store on one MI355X (include/ntsm_eval_hip.h:
 * ntsm_eval_trio_open / _duos / _score / _close; ntsmEval --trios).  The store is streamed once, at open,
 * into three bit-planes -- hom_at, het, hom_cg, one bit per sample and site, 64 sites to a word -- and the counts go back.  Both
 * questions are then logic and popcounts over site words: the duo rectangle (sites both samples are called at, sites where they
 * are opposite homozygotes) and the Mendelian errors of listed triples (child; two parents).  Every sum is an integer sum: no
 * rounding, no order, and two calls give the same bytes.
 *
 * Layout.  planes [plane][word][sample], uint64: the duo kernel's lanes (samples across the lanes) load one coalesced row of
 * words per plane and site word, its rows are scalar loads, and the trio kernel's staging reads a list's samples out of the
 * same rows (coalesced where the list is a run of samples, a gather of 8-byte words where it is not).  Bits past n_sites in the
 * last word are zero in all three planes, so no kernel masks a tail.
 *
 * Kernels.
 *   planes   one workgroup per (site word, 64 samples of the chunk): lanes run along the 64 sites of one sample (one coalesced
 *            512-byte read), one ballot per class turns them into one word per plane, and the 3 x 64 words go through LDS so
 *            that the store along the samples is coalesced too.
 *   geno     popcounts of the planes per sample, samples across the lanes, the words cut over blockIdx.y, integer atomics.
 *   duo      the contam and cross kernel's shape: columns across the lanes, a group of 1 / 2 / 4 rows wave-uniform (scalar
 *            loads), the loop over site words, two 32-bit accumulators per row from 64-bit popcounts.
 *   trio     a popcount "GEMM": one workgroup takes one (entry, tile of list positions p x tile of list positions q) work item
 *            of a flat list formed on the host, stages the tile's plane words through LDS in slabs of kSlab site words -- already
 *            folded with the child's words, so that a pair costs four ANDs, two ORs and three popcounts per word, see fold()
 *            -- and every lane keeps an RB x RB register block of pairs, three 32-bit counts each.  Two instances: 256 threads
 *            on a 64 x 64 tile (RB 4) for lists longer than 16, and one wave on a 16 x 16 tile (RB 2) for the short lists that a
 *            real cohort's candidate lists are; a call launches each over its own items.
 * One stream, no overlap.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/ntsm_eval_hip.h"
#define NTSM_HIP_TAG "ntsm_eval_trio"
#include "ntsm_eval_chunk.h"
#include "ntsm_eval_geno.h"
#include "ntsm_hip_scope.h"

namespace {

using ntsm_eval_chunk::kThreads;
using ntsm_eval_chunk::timed;
constexpr int kSlab = 8;                     /* site words per LDS slab of the trio kernel */
constexpr uint32_t kShortList = 16;          /* lists up to this long take the one-wave tile */
constexpr uint32_t kMaxGridY = 65535;

uint32_t g_width = 0;                        /* ntsm_eval_trio_tune */

/* counts [count][site][2] (dense) -> words `word` of samples first ... first + count - 1 in planes [3][n_words][n_db].
 * grid (tiles of 64 samples * n_words), word fastest; wave v of the workgroup takes samples v * 16 ... v * 16 + 15 of its tile. */
__global__ __launch_bounds__(kThreads) void ntsm_eval_trio_planes_kernel(const uint2 *__restrict__ counts, uint32_t count, uint32_t n_sites, uint32_t min_cov,
		uint32_t min_depth, uint32_t first, uint32_t n_db, uint32_t n_words, uint64_t *__restrict__ planes)
{
	__shared__ uint64_t tile[3][64];
	const uint32_t word = blockIdx.x % n_words, s0 = blockIdx.x / n_words * 64;
	const uint32_t lane = threadIdx.x % 64, wave = threadIdx.x / 64;
	const uint64_t site = (uint64_t) word * 64 + lane;
	for (uint32_t i = 0; i < 16; ++i) {
		const uint32_t r = wave * 16 + i, s = s0 + r;                              /* wave-uniform */
		int cls = 3;
		if (s < count && site < n_sites) {
			const uint2 c = counts[(uint64_t) s * n_sites + site];
			cls = ntsm_eval_class_of(c.x, c.y, min_cov, min_depth);                 /* the genotype rule, shared with --ld: ntsm_eval_geno.h */
		}
		const uint64_t b0 = __ballot(cls == 0), b1 = __ballot(cls == 1), b2 = __ballot(cls == 2);
		if (lane == 0) { tile[0][r] = b0; tile[1][r] = b1; tile[2][r] = b2; }
	}
	__syncthreads();
	if (threadIdx.x < 192) {
		const uint32_t pl = threadIdx.x / 64, r = threadIdx.x % 64;
		if (s0 + r < count) planes[((uint64_t) pl * n_words + word) * n_db + first + s0 + r] = tile[pl][r];
	}
}

/* geno [n_db][4], zeroed: columns 0 ... 2 += the popcounts of the three planes.  grid (n_db / 64, n_words / per); 256 threads =
 * 64 samples x 4 word lanes */
__global__ __launch_bounds__(kThreads) void ntsm_eval_trio_geno_kernel(const uint64_t *__restrict__ planes, uint32_t n_db, uint32_t n_words, uint32_t per,
		uint32_t *__restrict__ geno)
{
	const uint32_t s = blockIdx.x * 64 + threadIdx.x % 64;
	const uint32_t w0 = blockIdx.y * per, w1 = w0 + per < n_words ? w0 + per : n_words;
	if (s >= n_db) return;
	const uint64_t plane = (uint64_t) n_words * n_db;
	uint32_t c[3] = { 0, 0, 0 };
	for (uint32_t w = w0 + threadIdx.x / 64; w < w1; w += kThreads / 64) {
		const uint64_t *row = planes + (uint64_t) w * n_db + s;
#pragma unroll
		for (int pl = 0; pl < 3; ++pl) c[pl] += __popcll(row[pl * plane]);
	}
#pragma unroll
	for (int pl = 0; pl < 3; ++pl) atomicAdd(&geno[(uint64_t) s * 4 + pl], c[pl]);
}

/* grid (columns / blockDim.x, rows / TQ): rows row_first + r, r < n_rows, against every sample; out [n_rows][n_db] */
template <int TQ> __global__ __launch_bounds__(kThreads) void ntsm_eval_trio_duo_kernel(const uint64_t *__restrict__ planes, uint32_t n_db, uint32_t n_words,
		uint32_t row_first, uint32_t n_rows, ntsm_eval_trio_duo *__restrict__ out)
{
	const uint32_t y = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t yc = y < n_db ? y : n_db - 1;                                   /* lanes past the end compute a copy of the last column, not stored */
	const uint32_t r0 = blockIdx.y * TQ;
	uint32_t x[TQ], called[TQ], opp[TQ];
#pragma unroll
	for (int k = 0; k < TQ; ++k) { x[k] = row_first + (r0 + k < n_rows ? r0 + k : n_rows - 1); called[k] = 0; opp[k] = 0; }   /* wave-uniform: scalar loads */
	const uint64_t plane = (uint64_t) n_words * n_db;
	for (uint32_t w = 0; w < n_words; ++w) {
		const uint64_t *row = planes + (uint64_t) w * n_db;
		const uint64_t y0 = row[yc], y1 = row[plane + yc], y2 = row[2 * plane + yc];
		const uint64_t cy = y0 | y1 | y2;
#pragma unroll
		for (int k = 0; k < TQ; ++k) {
			const uint64_t x0 = row[x[k]], x1 = row[plane + x[k]], x2 = row[2 * plane + x[k]];   /* the same for every lane */
			called[k] += __popcll((x0 | x1 | x2) & cy);
			opp[k] += __popcll((x0 & y2) | (x2 & y0));
		}
	}
	if (y >= n_db) return;
#pragma unroll
	for (int k = 0; k < TQ; ++k) {
		if (r0 + k >= n_rows) continue;
		ntsm_eval_trio_duo d;
		d.called = called[k];
		d.opp = opp[k];
		out[(uint64_t) (r0 + k) * n_db + y] = d;
	}
}

/* one entry of a _score call on the device, and one work item: the tile of list positions [p0, p0 + T) x [q0, q0 + T), p0 <= q0 */
struct Entry { uint64_t cand_off, out_off; uint32_t child, k; };
struct Item { uint32_t entry, p0, q0; };

/* the records of an entry: pairs of list positions p < q < k, p ascending, q ascending inside p */
__device__ __host__ inline uint64_t pair_offset(uint64_t p, uint64_t q, uint64_t k) { return p * (2 * k - p - 1) / 2 + (q - p - 1); }

/* What staging leaves in LDS for list sample S = (s0, s1, s2) under child K = (k0, k1, k2), so that a pair (X on the p side, Y
 * on the q side) is
 *   cl = P.c & Q.c                    called_K & called_X & called_Y
 *   eh = (P.a | Q.a) & cl             cl & ((K0 & (X2 | Y2)) | (K2 & (X0 | Y0)))
 *   et = (P.u & Q.u) | (P.v & Q.v)    K1 & ((X0 & Y0) | (X2 & Y2)); every class is a subset of called, so cl is implied
 * p side: c = called_K & called_S, a = (K0 & S2) | (K2 & S0), u = K1 & S0, v = K1 & S2
 * q side: c = called_S,            a = the same,              u = S0,      v = S2 */
__device__ inline void fold(bool q_side, uint64_t k0, uint64_t k1, uint64_t k2, uint64_t s0, uint64_t s1, uint64_t s2, uint64_t v[4])
{
	const uint64_t cs = s0 | s1 | s2;
	v[0] = q_side ? cs : cs & (k0 | k1 | k2);
	v[1] = (k0 & s2) | (k2 & s0);
	v[2] = q_side ? s0 : k1 & s0;
	v[3] = q_side ? s2 : k1 & s2;
}

/* grid (items); TX x TX threads, each an RB x RB block of the T x T tile, T = TX * RB.  Thread (tx, ty) holds list positions
 * p = p0 + ty * RB + r and q = q0 + tx * RB + c: the q side is read as one run of RB words per lane, the same for the lanes of
 * one ty, and the p side is the same word for TX neighbouring lanes -- both free of bank conflicts. */
template <int TX, int RB> __global__ __launch_bounds__(TX * TX) void ntsm_eval_trio_kernel(const uint64_t *__restrict__ planes, uint32_t n_db, uint32_t n_words,
		const Entry *__restrict__ entries, const Item *__restrict__ items, const uint32_t *__restrict__ cand, ntsm_eval_trio_record *__restrict__ out)
{
	constexpr int T = TX * RB, kBlock = TX * TX;
	__shared__ uint64_t stage[2][kSlab][4][T];                                     /* [p side, q side][word][c, a, u, v][list position] */
	const Item it = items[blockIdx.x];
	const Entry e = entries[it.entry];
	const uint32_t *list = cand + e.cand_off;
	const uint32_t tx = threadIdx.x % TX, ty = threadIdx.x / TX;
	const uint32_t p_base = it.p0 + ty * RB, q_base = it.q0 + tx * RB;
	const uint32_t q_last = q_base + RB - 1 < e.k - 1 ? q_base + RB - 1 : e.k - 1;   /* e.k >= 2 */
	const bool active = q_base < e.k && p_base < q_last;                           /* the block holds a pair p < q < k */
	uint32_t cl[RB][RB], eh[RB][RB], et[RB][RB];
#pragma unroll
	for (int r = 0; r < RB; ++r)
#pragma unroll
		for (int c = 0; c < RB; ++c) { cl[r][c] = 0; eh[r][c] = 0; et[r][c] = 0; }
	const uint64_t plane = (uint64_t) n_words * n_db;
	for (uint32_t w0 = 0; w0 < n_words; w0 += kSlab) {
		__syncthreads();                                                           /* the slab before this one has been read */
		for (uint32_t idx = threadIdx.x; idx < 2u * kSlab * T; idx += kBlock) {
			const uint32_t side = idx / (kSlab * T), w = idx % (kSlab * T) / T, i = idx % T;
			const uint32_t pos = (side ? it.q0 : it.p0) + i;
			uint64_t v[4] = { 0, 0, 0, 0 };                                        /* past the list or past the last word: nothing is counted */
			if (w0 + w < n_words && pos < e.k) {
				const uint64_t *row = planes + (uint64_t) (w0 + w) * n_db;
				const uint32_t s = list[pos];
				fold(side != 0, row[e.child], row[plane + e.child], row[2 * plane + e.child], row[s], row[plane + s], row[2 * plane + s], v);
			}
#pragma unroll
			for (int a = 0; a < 4; ++a) stage[side][w][a][i] = v[a];
		}
		__syncthreads();
		if (!active) continue;
#pragma unroll 1
		for (int w = 0; w < kSlab; ++w) {
			uint64_t P[4][RB], Q[4][RB];
#pragma unroll
			for (int a = 0; a < 4; ++a)
#pragma unroll
				for (int r = 0; r < RB; ++r) { P[a][r] = stage[0][w][a][ty * RB + r]; Q[a][r] = stage[1][w][a][tx * RB + r]; }
#pragma unroll
			for (int r = 0; r < RB; ++r)
#pragma unroll
				for (int c = 0; c < RB; ++c) {
					const uint64_t both = P[0][r] & Q[0][c];
					cl[r][c] += __popcll(both);
					eh[r][c] += __popcll((P[1][r] | Q[1][c]) & both);
					et[r][c] += __popcll((P[2][r] & Q[2][c]) | (P[3][r] & Q[3][c]));
				}
		}
	}
	if (!active) return;
#pragma unroll
	for (int r = 0; r < RB; ++r)
#pragma unroll
		for (int c = 0; c < RB; ++c) {
			const uint32_t p = p_base + r, q = q_base + c;
			if (p >= q || q >= e.k) continue;
			ntsm_eval_trio_record t;
			t.called = cl[r][c]; t.err_hom = eh[r][c]; t.err_het = et[r][c]; t.pad = 0;
			out[e.out_off + pair_offset(p, q, e.k)] = t;
		}
}

/* the tile edge an entry's list takes: the library's rule, or the forced width (64 threads: 16, 256 threads: 64) */
uint32_t tile_of(uint32_t k) { return g_width ? (g_width == 64 ? 16u : 64u) : k <= kShortList ? 16u : 64u; }

}  // namespace

struct ntsm_eval_trio_session {
	int device = 0;
	uint32_t n_db = 0, n_sites = 0, n_words = 0;
	ntsm_hip::Buffers b;
	ntsm_hip::Events<2> ev;
	uint64_t *d_planes = nullptr;            /* [3][n_words][n_db]; NULL: a session without device work */
};

extern "C" int ntsm_eval_trio_tune(uint32_t width)
{
	if (width != 0 && width != 64 && width != 256) return -1;
	g_width = width;
	return 0;
}

extern "C" int ntsm_eval_trio_open(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n_db, uint32_t n_sites, uint32_t min_cov,
		uint32_t min_depth, uint32_t db_chunk, uint32_t *geno, ntsm_eval_cross_times *times, ntsm_eval_trio_session **h)
{
	if (times) *times = ntsm_eval_cross_times {};
	if (!h) return -1;
	*h = nullptr;
	if (!ntsm_eval_chunk::valid_store(db_counts, db_stride_bytes, n_db, n_sites)) return -1;
	std::unique_ptr<ntsm_eval_trio_session> s(new ntsm_eval_trio_session);
	s->device = device;
	s->n_db = n_db; s->n_sites = n_sites;
	s->n_words = (uint32_t) (((uint64_t) n_sites + 63) / 64);
	if (n_db == 0 || n_sites == 0) {                                               /* nothing to class: no device work, here or later */
		if (geno) memset(geno, 0, (size_t) n_db * 4 * sizeof(uint32_t));
		*h = s.release();
		return 0;
	}
	const uint32_t n_words = s->n_words;
	ntsm_eval_cross_times tm {};
	HIPCHK(hipSetDevice(device));
	HIPCHK(s->ev.create());
	HIPCHK(s->b.alloc(&s->d_planes, 3ull * n_words * n_db));
	/* what a staged chunk holds beside the planes, which are there already: its dense counts */
	size_t free_b = 0, total_b = 0;
	if (db_chunk == 0) HIPCHK(hipMemGetInfo(&free_b, &total_b));
	const uint32_t chunk = ntsm_eval_chunk::samples_per_pass(db_chunk, n_db, free_b, 8ull * n_sites, 0);
	ntsm_hip::Buffers b;                                                          /* open's own: the staging goes back when it returns */
	uint32_t *d_raw;
	HIPCHK(b.alloc(&d_raw, (uint64_t) chunk * n_sites * 2));
	for (uint32_t first = 0; first < n_db; first += chunk) {
		const uint32_t count = std::min(chunk, n_db - first);
		int rc = ntsm_eval_chunk::upload(db_counts, db_stride_bytes, first, count, n_sites, d_raw, tm);
		if (rc) return rc;
		rc = timed(s->ev[0], s->ev[1], &tm.prepare_kernel_ms, [&] {                  /* it waits: the next chunk overwrites d_raw */
			hipLaunchKernelGGL(ntsm_eval_trio_planes_kernel, dim3((count + 63) / 64 * n_words), dim3(kThreads), 0, 0, (const uint2 *) d_raw, count, n_sites, min_cov,
					min_depth, first, n_db, n_words, s->d_planes);
			HIPCHK(hipGetLastError());
			return 0;
		});
		if (rc) return rc;
		tm.chunks++;
	}
	if (geno) {
		uint32_t *d_geno;
		HIPCHK(b.alloc(&d_geno, (uint64_t) n_db * 4));
		HIPCHK(hipMemset(d_geno, 0, (size_t) n_db * 4 * sizeof(uint32_t)));
		const uint32_t per = std::max(64u, (n_words + kMaxGridY - 1) / kMaxGridY);
		int rc = timed(s->ev[0], s->ev[1], &tm.prepare_kernel_ms, [&] {
			hipLaunchKernelGGL(ntsm_eval_trio_geno_kernel, dim3((n_db + 63) / 64, (n_words + per - 1) / per), dim3(kThreads), 0, 0, s->d_planes, n_db, n_words, per, d_geno);
			HIPCHK(hipGetLastError());
			return 0;
		});
		if (rc || (rc = ntsm_eval_chunk::timed_copy(geno, d_geno, (size_t) n_db * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, &tm.download_ms)) != 0) return rc;
		for (uint32_t d = 0; d < n_db; ++d) geno[4ull * d + 3] = n_sites - (geno[4ull * d] + geno[4ull * d + 1] + geno[4ull * d + 2]);
	}
	if (times) *times = tm;
	*h = s.release();
	return 0;
}

extern "C" void ntsm_eval_trio_close(ntsm_eval_trio_session *h)
{
	if (!h) return;
	if (h->d_planes) (void) hipSetDevice(h->device);                              /* a session without device work touches no device here either */
	delete h;
}

extern "C" int ntsm_eval_trio_duos(ntsm_eval_trio_session *h, uint32_t row_first, uint32_t n_rows, ntsm_eval_trio_duo *out, double *kernel_ms)
{
	if (kernel_ms) *kernel_ms = 0;
	if (!h || !out || n_rows == 0 || (uint64_t) row_first + n_rows > h->n_db) return -1;
	const uint32_t n_db = h->n_db;
	const uint64_t records = (uint64_t) n_rows * n_db;
	if (!h->d_planes) {                                                            /* no site; n_db == 0 has no range to take */
		memset(out, 0, records * sizeof(ntsm_eval_trio_duo));
		return 0;
	}
	HIPCHK(hipSetDevice(h->device));
	ntsm_hip::Buffers b;
	ntsm_eval_trio_duo *d_out;
	HIPCHK(b.alloc(&d_out, records));
	/* ntsm_eval_chunk.h's launch rule, inherited and not measured again for this kernel; no forced group */
	uint32_t width, tq;
	ntsm_eval_chunk::launch_shape(n_rows, n_db, g_width, 0, width, tq);
	auto kernel = tq == 4 ? ntsm_eval_trio_duo_kernel<4> : tq == 2 ? ntsm_eval_trio_duo_kernel<2> : ntsm_eval_trio_duo_kernel<1>;
	double ms = 0;
	const int rc = timed(h->ev[0], h->ev[1], &ms, [&] {
		for (uint32_t r = 0; r < n_rows; r += kMaxGridY * tq) {                    /* one launch, unless the band has more row groups than a grid's y takes */
			const uint32_t rows = std::min(kMaxGridY * tq, n_rows - r);
			hipLaunchKernelGGL(kernel, dim3((n_db + width - 1) / width, (rows + tq - 1) / tq), dim3(width), 0, 0, h->d_planes, n_db, h->n_words, row_first + r, rows,
					d_out + (uint64_t) r * n_db);
			HIPCHK(hipGetLastError());
		}
		return 0;
	});
	if (rc) return rc;
	HIPCHK(hipMemcpy(out, d_out, records * sizeof(ntsm_eval_trio_duo), hipMemcpyDeviceToHost));
	if (kernel_ms) *kernel_ms = ms;
	return 0;
}

extern "C" int ntsm_eval_trio_score(ntsm_eval_trio_session *h, const uint32_t *child, const uint64_t *offset, const uint32_t *cand, uint32_t n_children,
		ntsm_eval_trio_record *out, double *kernel_ms)
{
	if (kernel_ms) *kernel_ms = 0;
	if (!h) return -1;
	if (n_children == 0) return 0;
	if (!child || !offset || offset[0] != 0) return -1;
	for (uint32_t i = 0; i < n_children; ++i)
		if (offset[i + 1] < offset[i] || offset[i + 1] - offset[i] > UINT32_MAX || child[i] >= h->n_db) return -1;
	const uint64_t n_cand = offset[n_children];
	if (n_cand && !cand) return -1;
	/* the entries that have records, their place in out, and the work items of both tiles */
	std::vector<Entry> entries;
	std::vector<Item> items[2];                                                   /* the 16-wide tile's, the 64-wide tile's */
	uint64_t records = 0;
	for (uint32_t i = 0; i < n_children; ++i) {
		const uint32_t k = (uint32_t) (offset[i + 1] - offset[i]);
		for (uint64_t c = offset[i]; c < offset[i + 1]; ++c)
			if (cand[c] >= h->n_db || cand[c] == child[i]) return -1;
		if (k < 2) continue;
		const uint32_t tile = tile_of(k);
		for (uint32_t p0 = 0; p0 < k; p0 += tile)
			for (uint32_t q0 = p0; q0 < k; q0 += tile)
				if (q0 > p0 || k - p0 > 1) items[tile == 64].push_back(Item { (uint32_t) entries.size(), p0, q0 });   /* a diagonal tile of one position has no pair */
		entries.push_back(Entry { offset[i], records, child[i], k });
		records += (uint64_t) k * (k - 1) / 2;
	}
	if (records == 0) return 0;
	if (!out) return -1;
	if (entries.size() > UINT32_MAX) return -1;
	if (!h->d_planes) {                                                            /* no site: every count is 0 */
		memset(out, 0, records * sizeof(ntsm_eval_trio_record));
		return 0;
	}
	HIPCHK(hipSetDevice(h->device));
	ntsm_hip::Buffers b;
	Entry *d_entries;
	Item *d_items[2];
	uint32_t *d_cand;
	ntsm_eval_trio_record *d_out;
	HIPCHK(b.alloc(&d_entries, entries.size()));
	HIPCHK(b.alloc(&d_cand, n_cand));
	HIPCHK(b.alloc(&d_out, records));
	HIPCHK(hipMemcpy(d_entries, entries.data(), entries.size() * sizeof(Entry), hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(d_cand, cand, n_cand * sizeof(uint32_t), hipMemcpyHostToDevice));
	for (int t = 0; t < 2; ++t) {
		HIPCHK(b.alloc(&d_items[t], items[t].size()));
		if (!items[t].empty()) HIPCHK(hipMemcpy(d_items[t], items[t].data(), items[t].size() * sizeof(Item), hipMemcpyHostToDevice));
	}
	double ms = 0;
	const uint64_t kSlice = 1u << 30;                                              /* work items per launch: below a grid's x */
	const int rc = timed(h->ev[0], h->ev[1], &ms, [&] {
		for (int t = 0; t < 2; ++t)
			for (uint64_t i0 = 0; i0 < items[t].size(); i0 += kSlice) {
				const uint32_t n = (uint32_t) std::min<uint64_t>(kSlice, items[t].size() - i0);
				if (t == 0)
					hipLaunchKernelGGL((ntsm_eval_trio_kernel<8, 2>), dim3(n), dim3(64), 0, 0, h->d_planes, h->n_db, h->n_words, d_entries, d_items[t] + i0, d_cand, d_out);
				else
					hipLaunchKernelGGL((ntsm_eval_trio_kernel<16, 4>), dim3(n), dim3(256), 0, 0, h->d_planes, h->n_db, h->n_words, d_entries, d_items[t] + i0, d_cand, d_out);
				HIPCHK(hipGetLastError());
			}
		return 0;
	});
	if (rc) return rc;
	HIPCHK(hipMemcpy(out, d_out, records * sizeof(ntsm_eval_trio_record), hipMemcpyDeviceToHost));
	if (kernel_ms) *kernel_ms = ms;
	return 0;
}
