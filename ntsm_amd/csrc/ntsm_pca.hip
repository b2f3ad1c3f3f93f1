/*
 * ntsm_pca.hip -- device steps of ntsmPCA for the MI355X (gfx950); the contract is in include/ntsm_pca_hip.h,
 * the design in DESIGN.md section 11.
 *
 * The uploaded matrix lives in a zero-padded buffer [p_pad][ld] (ld = n rounded up to the 128-sample tile, p_pad = p
 * rounded up to the 16-site chunk), so no kernel has a ragged inner loop: the padding contributes exact zeros.
 *   ntsm_pca_expand        the cells of ntsm_vcf_run into that buffer, padding included: a wave per row, one 16-byte store per
 *                          lane (two samples), the lanes side by side along the sample dimension; a cell's value from a table
 *                          by its code
 *   ntsm_pca_store_genotype  the cells from a chunk of a cohort store instead: counts [sample][site][2]
 *                          read along the sites, the genotype code of each pair, a byte per cell transposed through LDS,
 *                          16-bit cells written along the samples, the per-site tallies of the called genotypes added
 *   ntsm_pca_centre        one workgroup per site: the row sum in a fixed order (per-thread strided partial sums, then a
 *                          binary tree in LDS), mean = sum / n, and the row rewritten as Ac (padding stays 0)
 *   ntsm_pca_gram_tiles    the hot path: one workgroup per (upper 128 x 128 tile, piece of the site dimension); 4 waves,
 *                          each a 64 x 64 sub-tile = 4 x 4 v_mfma_f64_16x16x4_f64 accumulators; both operand panels are
 *                          [16 sites][128 samples] slices of Ac staged in LDS, the next chunk prefetched into registers
 *   ntsm_pca_gram_reduce   sums the pieces of each tile in piece order and writes G and its mirror
 *   ntsm_pca_scores        U_D (descending, [n][d_pad]) out of dsyevd's ascending column-major eigenvectors, T = U_D s
 *   ntsm_pca_project       V = Ac U_D / s: one wave per 4 sites x 8 components, lanes strided over the samples, a fixed
 *                          butterfly over the lanes
 */
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rocsolver/rocsolver.h>             /* types only: the library is bound with dlopen on first use */

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../include/ntsm_pca_hip.h"
#define NTSM_HIP_TAG "ntsm_pca"
#define NTSM_HIP_FAIL NTSM_PCA_E_HIP
#include "ntsm_hip_scope.h"
#include "ntsm_eval_chunk.h"                 /* a chunk of a cohort store on the device: the chunk rule and the 2-D copy */
#include "ntsm_eval_pca.h"                   /* genotype_code */
#include "host/pca_text.hpp"                 /* store_centre_value: a site's centre as its text reads back */

namespace {

constexpr int kTile = 128;                   /* samples per tile edge */
constexpr int kChunk = 16;                   /* sites per LDS stage */
constexpr int kLds = kTile + 16;             /* LDS row stride in doubles: rows r and r + 1 of a ds_read_b64 half-wave fall
                                              * 32 banks apart (1152 B), so its 2 x 16 lanes cover the 64 banks once */
constexpr int kProjRows = 4, kProjComp = 8;  /* per wave of the projection kernel */

typedef double v4d __attribute__((ext_vector_type(4)));

/* The whole padded buffer [p_pad][ld] from the 16-bit cells: a wave owns a row at a time (grid-stride over the rows), lane l
 * the samples 2 l and 2 l + 1 of every 128-sample piece, so each store instruction writes 1 KiB of the row, 16 bytes per lane
 * (ld is a multiple of 128), and nothing but the row's base is computed in 64 bits.  A live cell is
 * value[lin > first_undef][code] with lin = row * n + sample, row_fill[row] for code 0; padding is zero.  Rows of cells are
 * cell_ld cells apart: n for cells that came from the host, so the two codes are loaded as two 16-bit values; the padded
 * leading dimension of the genotype step for cells that were made on the device (the linear index stays row * n + sample). */
__global__ __launch_bounds__(256) void ntsm_pca_expand(const uint16_t *__restrict__ cells, const double *__restrict__ value,
		const double *__restrict__ row_fill, uint64_t first_undef, uint64_t p, uint32_t n, uint32_t cell_ld, uint64_t p_pad, uint32_t ld,
		double *__restrict__ a)
{
	const uint32_t lane = threadIdx.x & 63;
	const uint64_t waves = (uint64_t) gridDim.x * 4;
	for (uint64_t row = (uint64_t) blockIdx.x * 4 + (threadIdx.x >> 6); row < p_pad; row += waves) {
		double *out_row = a + row * ld;
		if (row >= p) {                                          /* a padding row (the branch is uniform in the wave) */
			for (uint32_t col = lane * 2; col < ld; col += 128) *reinterpret_cast<double2 *>(out_row + col) = double2 { 0.0, 0.0 };
			continue;
		}
		const uint64_t base = row * n;
		const uint16_t *in_row = cells + row * cell_ld;
		const double fill = row_fill[row];
#pragma unroll 2
		for (uint32_t col = lane * 2; col < ld; col += 128) {
			double2 out = { 0.0, 0.0 };
			if (col < n) {
				const uint32_t c0 = in_row[col];
				out.x = c0 ? value[(base + col > first_undef ? 65536u : 0u) + c0] : fill;
				if (col + 1 < n) {
					const uint32_t c1 = in_row[col + 1];
					out.y = c1 ? value[(base + col + 1 > first_undef ? 65536u : 0u) + c1] : fill;
				}
			}
			*reinterpret_cast<double2 *>(out_row + col) = out;
		}
	}
}

/* The genotype step of a cohort store's chunk.  counts: the chunk, dense [count][n_sites] pairs;
 * sample i of it is column first + i of the cell matrix [n_sites][cell_ld].  A workgroup takes 64 sites x 256 columns, the
 * columns counted from col0 = first rounded down to a multiple of 64, so that a tile's row pieces start on 128-byte
 * boundaries whatever column the chunk starts at (cell_ld is a multiple of 64).
 *   read:   lane l of wave w is site l of the tile for the columns 64 w ... 64 w + 63, four at a time: four independent
 *           8-byte loads, side by side along the sites of one sample (512 B per wave-instruction), the code of each pair,
 *           and one ds_write_b32 of the four cells code + 1 (0: missing or outside the chunk) -- a byte per cell, so the
 *           tile is 16.25 KiB.  Rows are 65 dwords apart: the 32 lanes of a store's group fall on 32 banks.
 *           A lane is a site here, so the site's tallies over the wave's 64 columns add up in three registers, without a
 *           cross-lane step; the four waves add theirs in LDS and the workgroup adds 64 x 3 integers to the global tallies.
 *   write:  wave w takes the tile's sites w, w + 4, ...: a ds_read_b32 per lane (consecutive dwords), the four cells widened
 *           to 16 bits and stored as 8 bytes, 512 B of the cell row per wave-instruction.  A group of four columns that
 *           the chunk covers only in part (its first and last column need not be multiples of 4) is stored cell by cell,
 *           so nothing outside the chunk's columns is written and chunks may be processed in any order.
 * Integer atomics only: cells and tallies are the same for every chunk size. */
constexpr int kGenoSites = 64, kGenoCols = 256, kGenoPitch = kGenoCols + 4;

__global__ __launch_bounds__(256) void ntsm_pca_store_genotype(const uint2 *__restrict__ counts, uint32_t first, uint32_t count, uint32_t col0,
		uint32_t n_sites, uint32_t min_cov, uint16_t *__restrict__ cells, uint32_t cell_ld, uint32_t *__restrict__ tally)
{
	__shared__ __attribute__((aligned(16))) uint8_t tile[kGenoSites][kGenoPitch];
	__shared__ uint32_t sum[kGenoSites * 3];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t site0 = blockIdx.x * kGenoSites, tile_col = col0 + blockIdx.y * kGenoCols, end = first + count;
	if (threadIdx.x < kGenoSites * 3) sum[threadIdx.x] = 0;

	const bool site_ok = site0 + lane < n_sites;
	const uint2 *column = counts + (site_ok ? site0 + lane : 0u);
	uint32_t n_half = 0, n_one = 0, n_called = 0;
#pragma unroll 2
	for (uint32_t g = 0; g < 64; g += 4) {
		const uint32_t col = tile_col + wave * 64 + g;
		uint2 c[4];
		bool ok[4];
#pragma unroll
		for (int k = 0; k < 4; ++k) {                               /* unconditional loads of a row of the chunk: they stay in flight together */
			ok[k] = site_ok && col + k >= first && col + k < end;
			c[k] = column[(uint64_t) (ok[k] ? col + k - first : 0u) * n_sites];
		}
		uint32_t four = 0;
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			const uint32_t code = ntsm_eval_pca::genotype_code(c[k].x, c[k].y, min_cov);
			const bool called = ok[k] && code != 3;
			n_half += called && code == 1;
			n_one += called && code == 2;
			n_called += called;
			four |= (called ? code + 1 : 0u) << (8 * k);
		}
		*reinterpret_cast<uint32_t *>(&tile[lane][wave * 64 + g]) = four;
	}
	__syncthreads();                                               /* sum is zero, the tile is written */
	if (n_called) {
		atomicAdd(&sum[lane * 3], n_half);
		atomicAdd(&sum[lane * 3 + 1], n_one);
		atomicAdd(&sum[lane * 3 + 2], n_called);
	}

	for (uint32_t r = wave; r < (uint32_t) kGenoSites && site0 + r < n_sites; r += 4) {
		const uint32_t four = *reinterpret_cast<const uint32_t *>(&tile[r][lane * 4]);
		const uint32_t col = tile_col + lane * 4;
		uint16_t *out = cells + (uint64_t) (site0 + r) * cell_ld + col;
		if (col >= first && col + 4 <= end) {
			*reinterpret_cast<uint2 *>(out) = uint2 { (four & 0xFFu) | (four & 0xFF00u) << 8, (four >> 16 & 0xFFu) | (four >> 24) << 16 };
		} else {
#pragma unroll
			for (int k = 0; k < 4; ++k)
				if (col + k >= first && col + k < end) out[k] = (uint16_t) (four >> (8 * k) & 0xFFu);
		}
	}
	__syncthreads();
	if (threadIdx.x < kGenoSites * 3 && site0 + threadIdx.x / 3 < n_sites && sum[threadIdx.x])
		atomicAdd(&tally[(uint64_t) site0 * 3 + threadIdx.x], sum[threadIdx.x]);
}

__global__ __launch_bounds__(256) void ntsm_pca_centre(double *a, size_t ld, uint32_t n, double *means, int subtract)
{
	__shared__ double part[256];
	double *row = a + (size_t) blockIdx.x * ld;
	double s = 0.0;
	for (uint32_t j = threadIdx.x; j < n; j += 256) s += row[j];
	part[threadIdx.x] = s;
	__syncthreads();
	for (int w = 128; w > 0; w >>= 1) {
		if ((int) threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
		__syncthreads();
	}
	const double mean = part[0] / (double) n;
	if (threadIdx.x == 0) means[blockIdx.x] = mean;
	if (subtract)
		for (uint32_t j = threadIdx.x; j < n; j += 256) row[j] -= mean;
}

/* lane map of v_mfma_f64_16x16x4_f64: A operand lane l = A[row l & 15][k l >> 4], B operand lane l = B[k l >> 4][col l & 15],
 * result register r of lane l = D[row (l >> 4) + 4 r][col l & 15].  With A = (I panel)^T and B = the J panel both operands
 * are read from LDS as [site l >> 4][sample l & 15]. */
__global__ __launch_bounds__(256) void ntsm_pca_gram_tiles(const double *__restrict__ ac, size_t ld, uint32_t edge,
		uint32_t n_tiles, uint32_t chunks, uint32_t chunks_per_piece, double *__restrict__ partial)
{
	__shared__ __attribute__((aligned(16))) double sI[kChunk][kLds];
	__shared__ __attribute__((aligned(16))) double sJ[kChunk][kLds];
	uint32_t ti = 0, rem = blockIdx.x;
	while (rem >= edge - ti) { rem -= edge - ti; ++ti; }
	const uint32_t tj = ti + rem;
	const uint32_t c0 = blockIdx.y * chunks_per_piece, c1 = min(chunks, c0 + chunks_per_piece);
	const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
	const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
	const int lrow = tid >> 6, lcol = (tid & 63) * 2;             /* this thread's double2 of each 4-site slab of a panel */

	v4d acc[4][4];
#pragma unroll
	for (int m = 0; m < 4; ++m)
#pragma unroll
		for (int q = 0; q < 4; ++q) acc[m][q] = v4d { 0.0, 0.0, 0.0, 0.0 };

	/* named registers, not arrays: the prefetched chunk must stay in VGPRs across the loop's back edge */
	double2 i0, i1, i2, i3, j0, j1, j2, j3;
#define NTSM_PCA_FETCH1(c, r, I, J) { \
		const double *src = ac + ((size_t) (c) * kChunk + (r) * 4 + lrow) * ld + lcol; \
		I = *reinterpret_cast<const double2 *>(src + (size_t) ti * kTile); \
		J = *reinterpret_cast<const double2 *>(src + (size_t) tj * kTile); }
#define NTSM_PCA_FETCH(c) { NTSM_PCA_FETCH1(c, 0, i0, j0) NTSM_PCA_FETCH1(c, 1, i1, j1) NTSM_PCA_FETCH1(c, 2, i2, j2) NTSM_PCA_FETCH1(c, 3, i3, j3) }
#define NTSM_PCA_STAGE(r, I, J) { \
		*reinterpret_cast<double2 *>(&sI[(r) * 4 + lrow][lcol]) = I; \
		*reinterpret_cast<double2 *>(&sJ[(r) * 4 + lrow][lcol]) = J; }
	NTSM_PCA_FETCH(c0)                                           /* c0 < chunks: no piece is empty */
	for (uint32_t c = c0; c < c1; ++c) {
		__syncthreads();                                          /* the previous chunk's reads are done */
		NTSM_PCA_STAGE(0, i0, j0) NTSM_PCA_STAGE(1, i1, j1) NTSM_PCA_STAGE(2, i2, j2) NTSM_PCA_STAGE(3, i3, j3)
		__syncthreads();
		NTSM_PCA_FETCH(c + 1 < c1 ? c + 1 : c)                    /* unconditional: the loads stay in registers and in flight */
#pragma unroll
		for (int k0 = 0; k0 < kChunk; k0 += 4) {
			double a[4], b[4];
#pragma unroll
			for (int m = 0; m < 4; ++m) {
				a[m] = sI[k0 + (lane >> 4)][wm + m * 16 + (lane & 15)];
				b[m] = sJ[k0 + (lane >> 4)][wn + m * 16 + (lane & 15)];
			}
#pragma unroll
			for (int m = 0; m < 4; ++m)
#pragma unroll
				for (int q = 0; q < 4; ++q) acc[m][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[q], acc[m][q], 0, 0, 0);
		}
	}
#undef NTSM_PCA_FETCH
#undef NTSM_PCA_FETCH1
#undef NTSM_PCA_STAGE
	double *out = partial + ((size_t) blockIdx.y * n_tiles + blockIdx.x) * (kTile * kTile);
#pragma unroll
	for (int m = 0; m < 4; ++m)
#pragma unroll
		for (int q = 0; q < 4; ++q)
#pragma unroll
			for (int r = 0; r < 4; ++r)
				out[(size_t) (wm + m * 16 + (lane >> 4) + 4 * r) * kTile + wn + q * 16 + (lane & 15)] = acc[m][q][r];
}

/* grid (tiles, 16): block y sums rows [8y, 8y + 8) of its tile over the pieces, in piece order.  Of a diagonal tile only
 * the elements on or above the diagonal are used, so G is symmetric bit for bit by construction. */
__global__ __launch_bounds__(256) void ntsm_pca_gram_reduce(const double *__restrict__ partial, uint32_t edge, uint32_t n_tiles,
		uint32_t pieces, uint32_t n, double *__restrict__ g)
{
	uint32_t ti = 0, rem = blockIdx.x;
	while (rem >= edge - ti) { rem -= edge - ti; ++ti; }
	const uint32_t tj = ti + rem;
	for (int e = threadIdx.x; e < 8 * kTile; e += 256) {
		const uint32_t row = blockIdx.y * 8 + e / kTile, col = e % kTile;
		const size_t at = (size_t) blockIdx.x * (kTile * kTile) + (size_t) row * kTile + col;
		double s = 0.0;
		for (uint32_t q = 0; q < pieces; ++q) s += partial[(size_t) q * n_tiles * (kTile * kTile) + at];
		const uint32_t gi = ti * kTile + row, gj = tj * kTile + col;
		if (gi >= n || gj >= n || gi > gj) continue;
		g[(size_t) gi * n + gj] = s;
		g[(size_t) gj * n + gi] = s;
	}
}

/* evec: dsyevd's output, column-major, eigenvalues ascending: eigenvector of the i-th largest = column n - 1 - i */
__global__ __launch_bounds__(256) void ntsm_pca_scores(const double *__restrict__ evec, uint32_t n, uint32_t d, uint32_t d_pad,
		const double *__restrict__ s, double *__restrict__ ud, double *__restrict__ t)
{
	const size_t at = (size_t) blockIdx.x * 256 + threadIdx.x;
	if (at >= (size_t) n * d_pad) return;
	const uint32_t j = (uint32_t) (at / d_pad), i = (uint32_t) (at % d_pad);
	const double u = i < d ? evec[(size_t) (n - 1 - i) * n + j] : 0.0;
	ud[at] = u;
	if (i < d) t[(size_t) j * d + i] = u * s[i];
}

__global__ __launch_bounds__(256) void ntsm_pca_project(const double *__restrict__ ac, size_t ld, uint32_t n, uint64_t p,
		const double *__restrict__ ud, uint32_t d_pad, const double *__restrict__ s, uint32_t d, double *__restrict__ v)
{
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint64_t row0 = ((uint64_t) blockIdx.x * 4 + wave) * kProjRows;
	const uint32_t i0 = blockIdx.y * kProjComp;
	double acc[kProjRows][kProjComp];
#pragma unroll
	for (int r = 0; r < kProjRows; ++r)
#pragma unroll
		for (int i = 0; i < kProjComp; ++i) acc[r][i] = 0.0;
	for (uint32_t j = lane; j < n; j += 64) {
		double x[kProjRows];
#pragma unroll
		for (int r = 0; r < kProjRows; ++r) x[r] = ac[(row0 + r) * ld + j];
		const double2 *u = reinterpret_cast<const double2 *>(ud + (size_t) j * d_pad + i0);
#pragma unroll
		for (int i = 0; i < kProjComp; i += 2) {
			const double2 uu = u[i >> 1];
#pragma unroll
			for (int r = 0; r < kProjRows; ++r) {
				acc[r][i] = fma(x[r], uu.x, acc[r][i]);
				acc[r][i + 1] = fma(x[r], uu.y, acc[r][i + 1]);
			}
		}
	}
#pragma unroll
	for (int r = 0; r < kProjRows; ++r)
#pragma unroll
		for (int i = 0; i < kProjComp; ++i) {
			double x = acc[r][i];
#pragma unroll
			for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
			acc[r][i] = x;
		}
	if (lane == 0) {
#pragma unroll
		for (int r = 0; r < kProjRows; ++r)
#pragma unroll
			for (int i = 0; i < kProjComp; ++i)
				if (row0 + r < p && i0 + i < d) v[(row0 + r) * d + i0 + i] = acc[r][i] / s[i0 + i];
	}
}

/* rocSOLVER (and the rocBLAS it depends on) are bound on first use, as rccl_bind.cpp binds RCCL: the two libraries are
 * hundreds of megabytes of code objects that only this program's eigen step needs. */
struct Solver {
	decltype(&rocblas_create_handle) create_handle = nullptr;
	decltype(&rocblas_destroy_handle) destroy_handle = nullptr;
	decltype(&rocblas_set_atomics_mode) set_atomics_mode = nullptr;
	decltype(&rocsolver_dsyevd) dsyevd = nullptr;
	bool ok = false;
	Solver()
	{
		void *h = dlopen("librocsolver.so.0", RTLD_NOW | RTLD_GLOBAL);
		if (!h) h = dlopen("librocsolver.so", RTLD_NOW | RTLD_GLOBAL);
		if (!h) return;
		/* dlsym on the handle also searches its dependencies (librocblas) */
		create_handle = (decltype(create_handle)) dlsym(h, "rocblas_create_handle");
		destroy_handle = (decltype(destroy_handle)) dlsym(h, "rocblas_destroy_handle");
		set_atomics_mode = (decltype(set_atomics_mode)) dlsym(h, "rocblas_set_atomics_mode");
		dsyevd = (decltype(dsyevd)) dlsym(h, "rocsolver_dsyevd");
		ok = create_handle && destroy_handle && set_atomics_mode && dsyevd;
	}
};
const Solver &solver_bind()
{
	static Solver s;                                       /* thread-safe one-time binding */
	return s;
}

double ms_since(std::chrono::steady_clock::time_point t)
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

/* everything both entry points share: the padded matrix on the device, the row means, G; released with the scope */
struct Device {
	ntsm_hip::Buffers buf;
	ntsm_hip::Events<5> ev;
	uint16_t *cells = nullptr;
	uint32_t cell_ld = 0;                    /* cells per row of `cells`: n for host cells, padded for a store's */
	uint32_t *tally = nullptr;               /* a store's [p][3] */
	std::vector<uint32_t> tallies;           /* ... on the host */
	ntsm_pca_store_times st = {};
	double *value = nullptr, *row_fill = nullptr;
	double expand_ms = 0.0;
	double *a = nullptr, *means = nullptr, *partial = nullptr, *g = nullptr;
	double *w = nullptr, *e = nullptr, *s = nullptr, *ud = nullptr, *t = nullptr, *v = nullptr;
	rocblas_int *info = nullptr;
	size_t ld = 0;
	uint64_t p_pad = 0;
};

/* the rocBLAS handle of one run, destroyed on every return path */
struct Handle {
	const Solver &sv;
	rocblas_handle h = nullptr;
	explicit Handle(const Solver &s) : sv(s) {}
	Handle(const Handle &) = delete;
	~Handle() { if (h) (void) sv.destroy_handle(h); }
};

/* where the matrix comes from: host doubles [p][n], the cells of ntsm_vcf_run with the values of their codes, or the first
 * n records of a cohort store (the cells and the fills are then made here, section 11.1) */
struct Source {
	const double *a = nullptr;
	const uint16_t *cells = nullptr;
	const double *value = nullptr, *row_fill = nullptr;
	uint64_t first_undef_cell = ~0ull;
	const void *db = nullptr;
	uint64_t db_stride = 0;
	uint32_t min_cov = 0, db_chunk = 0;
};

bool shape_ok(uint64_t p, uint32_t n)
{
	return p >= 1 && n >= 1 && p < (1ull << 31) && n < (1u << 24);
}
bool args_ok(uint64_t p, uint32_t n, const double *a)
{
	return a && shape_ok(p, n);
}
bool args_ok(uint64_t p, uint32_t n, const Source &src)
{
	if (src.db) return shape_ok(p, n) && src.db_stride >= 8 * p && src.db_stride % 4 == 0;
	return src.cells && src.value && src.row_fill && shape_ok(p, n);
}

/* The cells and the tallies of a store's first n records, on the device (dev.cells [p][dev.cell_ld], dev.tally) and the
 * tallies on the host as well (dev.tallies): per chunk ntsm_eval_chunk::stage with neither transpose nor tally asked for --
 * the 2-D copy from the store's pitch into a dense [chunk][site][2] buffer -- and ntsm_pca_store_genotype.  One stream, one
 * wait per chunk.  The device is set and dev.ev exists. */
int store_cells_on_device(Device &dev, uint64_t p, uint32_t n, const Source &src)
{
	const uint32_t m = (uint32_t) p;
	uint32_t *d_raw = nullptr;
	size_t free_b = 0, total_b = 0;
	ntsm_eval_cross_times ctm {};
	dev.cell_ld = (n + 63u) / 64u * 64u;
	HIPCHK(dev.buf.alloc(&dev.cells, p * dev.cell_ld));
	HIPCHK(dev.buf.alloc(&dev.tally, p * 3));
	HIPCHK(hipMemset(dev.tally, 0, p * 3 * sizeof(uint32_t)));
	if (src.db_chunk == 0) HIPCHK(hipMemGetInfo(&free_b, &total_b));
	const uint32_t chunk = std::min(1u << 23, ntsm_eval_chunk::samples_per_pass(src.db_chunk, n, free_b, 8ull * p, 0));   /* grid.y <= 32,769 */
	HIPCHK(dev.buf.alloc(&d_raw, (uint64_t) chunk * p * 2));
	dev.st.chunk = chunk;
	for (uint32_t c0 = 0; c0 < n; c0 += chunk) {
		const uint32_t cn = std::min(chunk, n - c0), col0 = c0 & ~63u;
		if (const int rc = ntsm_eval_chunk::stage(src.db, src.db_stride, c0, cn, m, src.min_cov, d_raw, nullptr, nullptr, nullptr, nullptr, dev.ev[0],
		        dev.ev[1], ctm))
			return rc;
		ntsm_pca_store_genotype<<<dim3((m + kGenoSites - 1) / kGenoSites, (c0 + cn - col0 + kGenoCols - 1) / kGenoCols), dim3(256)>>>(
		    (const uint2 *) d_raw, c0, cn, col0, m, src.min_cov, dev.cells, dev.cell_ld, dev.tally);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(dev.ev[2], 0));
		HIPCHK(hipEventSynchronize(dev.ev[2]));                   /* the next chunk's copy overwrites d_raw */
		if (const int rc = ntsm_eval_chunk::add_interval(dev.ev[1], dev.ev[2], &dev.st.genotype_ms)) return rc;
		dev.st.chunks++;
	}
	dev.st.upload_ms = ctm.upload_ms;
	HIPCHK(dev.buf.release(&d_raw));
	const auto t0 = std::chrono::steady_clock::now();
	dev.tallies.resize(p * 3);
	HIPCHK(hipMemcpy(dev.tallies.data(), dev.tally, p * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
	dev.st.fill_ms = ms_since(t0);
	return 0;
}
bool run_args_ok(uint64_t p, uint32_t n, uint32_t d, const double *eigval, const double *rot, const double *comp)
{
	return n >= 2 && d >= 1 && d <= n && d <= p && eigval && rot && comp;
}

/* the matrix into the padded buffer dev.a: host doubles are copied into a zeroed buffer; cells are uploaded as they are, or
 * made from a store's records (store_cells_on_device), and expanded by ntsm_pca_expand, which writes the padding too
 * (dev.expand_ms, HIP events) */
int matrix_on_device(Device &dev, int device, uint64_t p, uint32_t n, const Source &src, ntsm_pca_times &tm)
{
	const uint32_t edge = (n + kTile - 1) / kTile;
	dev.ld = (size_t) edge * kTile;
	dev.p_pad = (p + kChunk - 1) / kChunk * kChunk;
	auto t0 = std::chrono::steady_clock::now();
	HIPCHK(hipSetDevice(device));
	HIPCHK(dev.ev.create());
	HIPCHK(dev.buf.alloc(&dev.a, dev.p_pad * dev.ld));
	if (src.a) {
		HIPCHK(hipMemset(dev.a, 0, dev.p_pad * dev.ld * sizeof(double)));
		HIPCHK(hipMemcpy2D(dev.a, dev.ld * sizeof(double), src.a, (size_t) n * sizeof(double), (size_t) n * sizeof(double), p, hipMemcpyHostToDevice));
		HIPCHK(hipDeviceSynchronize());
		tm.upload_ms = ms_since(t0);
		return 0;
	}
	float ms = 0;
	hipDeviceProp_t prop;
	HIPCHK(hipGetDeviceProperties(&prop, device));
	HIPCHK(dev.buf.alloc(&dev.value, 2 * 65536));
	HIPCHK(dev.buf.alloc(&dev.row_fill, p));
	if (src.db) {
		/* the cells never leave the device; the 12 bytes per site of the tallies come down, every site's fill is what its
		 * centre's text reads back as (the hand-over of `ntsmVCF --rotation`), and the codes 1, 2, 3 are 0, 0.5, 1 */
		if (const int rc = store_cells_on_device(dev, p, n, src)) return rc;
		const auto t1 = std::chrono::steady_clock::now();
		std::vector<double> value(2 * 65536, std::numeric_limits<double>::quiet_NaN()), fill(p);
		value[1] = 0.0; value[2] = 0.5; value[3] = 1.0;
		for (uint64_t s = 0; s < p; ++s) fill[s] = ntsm::store_centre_value(dev.tallies[3 * s], dev.tallies[3 * s + 1], dev.tallies[3 * s + 2]);
		HIPCHK(hipMemcpy(dev.value, value.data(), 2 * 65536 * sizeof(double), hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(dev.row_fill, fill.data(), p * sizeof(double), hipMemcpyHostToDevice));
		HIPCHK(hipDeviceSynchronize());
		dev.st.fill_ms += ms_since(t1);
		tm.upload_ms = dev.st.upload_ms;
	} else {
		dev.cell_ld = n;
		HIPCHK(dev.buf.alloc(&dev.cells, p * n));
		HIPCHK(hipMemcpy(dev.cells, src.cells, p * n * sizeof(uint16_t), hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(dev.value, src.value, 2 * 65536 * sizeof(double), hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(dev.row_fill, src.row_fill, p * sizeof(double), hipMemcpyHostToDevice));
		HIPCHK(hipDeviceSynchronize());
		tm.upload_ms = ms_since(t0);
	}
	/* a grid-stride walk over the rows, four per workgroup: 32 workgroups per compute unit keep every unit's store queue
	 * fed, and a short buffer gets no more workgroups than it has rows */
	const unsigned blocks = (unsigned) std::min<uint64_t>(dev.p_pad / 4, 32ull * (uint64_t) prop.multiProcessorCount);
	HIPCHK(hipEventRecord(dev.ev[3], 0));
	ntsm_pca_expand<<<dim3(blocks), dim3(256)>>>(dev.cells, dev.value, dev.row_fill, src.first_undef_cell, p, n, dev.cell_ld, dev.p_pad,
	    (uint32_t) dev.ld, dev.a);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(dev.ev[4], 0));
	HIPCHK(hipEventSynchronize(dev.ev[4]));
	HIPCHK(hipEventElapsedTime(&ms, dev.ev[3], dev.ev[4]));
	dev.expand_ms = dev.st.expand_ms = ms;
	return 0;
}

/* matrix, centre, Gram: leaves Ac (or A) in dev.a, the means in dev.means and G in dev.g */
int gram_on_device(Device &dev, int device, uint64_t p, uint32_t n, const Source &src, int centre, uint32_t split, ntsm_pca_times &tm)
{
	float ms = 0;
	const uint32_t edge = (n + kTile - 1) / kTile, n_tiles = edge * (edge + 1) / 2;
	const uint32_t chunks = (uint32_t) ((p + kChunk - 1) / kChunk);
	uint32_t pieces = split, cpp = 0;
	hipDeviceProp_t prop;
	if (const int rc = matrix_on_device(dev, device, p, n, src, tm)) return rc;
	HIPCHK(hipGetDeviceProperties(&prop, device));
	if (!pieces) {
		/* about 32 workgroups per compute unit: two are resident at a time (128 accumulator registers per lane), so the
		 * last, partly filled round of workgroups is a small share of the whole; at most 1 GiB of partial tiles */
		pieces = (32u * (uint32_t) prop.multiProcessorCount + n_tiles - 1) / n_tiles;
		pieces = std::min<uint32_t>(pieces, std::max<uint32_t>(1, (uint32_t) ((1ull << 30) / ((uint64_t) n_tiles * kTile * kTile * 8))));
	}
	pieces = std::max(1u, std::min(pieces, chunks));
	cpp = (chunks + pieces - 1) / pieces;
	pieces = (chunks + cpp - 1) / cpp;                          /* no empty piece; the last one may be short */
	HIPCHK(dev.buf.alloc(&dev.means, dev.p_pad));
	HIPCHK(dev.buf.alloc(&dev.partial, (size_t) pieces * n_tiles * kTile * kTile));
	HIPCHK(dev.buf.alloc(&dev.g, (size_t) n * n));

	HIPCHK(hipEventRecord(dev.ev[0], 0));
	ntsm_pca_centre<<<dim3((unsigned) p), dim3(256)>>>(dev.a, dev.ld, n, dev.means, centre ? 1 : 0);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(dev.ev[1], 0));
	ntsm_pca_gram_tiles<<<dim3(n_tiles, pieces), dim3(256)>>>(dev.a, dev.ld, edge, n_tiles, chunks, cpp, dev.partial);
	HIPCHK(hipGetLastError());
	ntsm_pca_gram_reduce<<<dim3(n_tiles, kTile / 8), dim3(256)>>>(dev.partial, edge, n_tiles, pieces, n, dev.g);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(dev.ev[2], 0));
	HIPCHK(hipEventSynchronize(dev.ev[2]));
	HIPCHK(hipEventElapsedTime(&ms, dev.ev[0], dev.ev[1]));
	tm.centre_ms = ms;
	HIPCHK(hipEventElapsedTime(&ms, dev.ev[1], dev.ev[2]));
	tm.gram_ms = ms;
	tm.gram_flops = (uint64_t) n * (n + 1ull) * p;
	tm.gram_bytes = (uint64_t) n_tiles * 2ull * kTile * dev.p_pad * 8ull            /* both panels of every tile */
	    + 2ull * pieces * n_tiles * kTile * kTile * 8ull + (uint64_t) n * n * 8ull;  /* partial tiles out and in, G */
	tm.gram_tiles = n_tiles;
	tm.gram_split = pieces;
	return 0;
}

/* the Gram step of either source */
int gram_of(int device, uint64_t p, uint32_t n, const Source &src, int centre, uint32_t split, double *gram, double *means,
		ntsm_pca_times *times, double *expand_ms)
{
	ntsm_pca_times tm = {};
	Device dev;
	if (const int rc = gram_on_device(dev, device, p, n, src, centre, split, tm)) return rc;
	auto t0 = std::chrono::steady_clock::now();
	HIPCHK(hipMemcpy(gram, dev.g, (size_t) n * n * sizeof(double), hipMemcpyDeviceToHost));
	if (means) HIPCHK(hipMemcpy(means, dev.means, p * sizeof(double), hipMemcpyDeviceToHost));
	tm.download_ms = ms_since(t0);
	if (times) *times = tm;
	if (expand_ms) *expand_ms = dev.expand_ms;
	return 0;
}

/* the whole PCA of any source; tallies and store_times are a store's (given once the matrix is on the device, so a rank
 * refusal has them too) */
int run_of(int device, uint64_t p, uint32_t n, const Source &src, uint32_t d, uint32_t split, double *eigval, double *rot,
		double *comp, uint32_t *bad_component, ntsm_pca_times *times, double *expand_ms, uint32_t *tallies = nullptr,
		ntsm_pca_store_times *store_times = nullptr)
{
	const Solver &sv = solver_bind();
	if (!sv.ok) return NTSM_PCA_E_SOLVER_MISSING;
	float ms = 0;
	ntsm_pca_times tm = {};
	Device dev;
	Handle handle(sv);
	rocblas_int info = 0;
	const uint32_t d_pad = (d + kProjComp - 1) / kProjComp * kProjComp;
	std::vector<double> w(n), s(d_pad, 1.0);
	if (const int rc = gram_on_device(dev, device, p, n, src, 1, split, tm)) return rc;
	if (tallies) std::copy(dev.tallies.begin(), dev.tallies.end(), tallies);
	if (store_times) *store_times = dev.st;

	/* eigenpairs of G: dsyevd overwrites G with the eigenvectors (column-major), eigenvalues ascending in w */
	HIPCHK(dev.buf.alloc(&dev.w, n));
	HIPCHK(dev.buf.alloc(&dev.e, n));
	HIPCHK(dev.buf.alloc(&dev.info, 1));
	{
		auto t0 = std::chrono::steady_clock::now();
		if (sv.create_handle(&handle.h) != rocblas_status_success) return NTSM_PCA_E_SOLVER;
		(void) sv.set_atomics_mode(handle.h, rocblas_atomics_not_allowed);    /* the same bits on every run */
		const rocblas_status st = sv.dsyevd(handle.h, rocblas_evect_original, rocblas_fill_upper, (rocblas_int) n, dev.g, (rocblas_int) n,
		    dev.w, dev.e, dev.info);
		if (st != rocblas_status_success) {
			fprintf(stderr, "ntsm_pca: rocsolver_dsyevd returned status %d\n", (int) st);
			return NTSM_PCA_E_SOLVER;
		}
		HIPCHK(hipDeviceSynchronize());
		HIPCHK(hipMemcpy(&info, dev.info, sizeof(info), hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(w.data(), dev.w, n * sizeof(double), hipMemcpyDeviceToHost));
		tm.eigen_ms = ms_since(t0);
		if (info != 0) {
			fprintf(stderr, "ntsm_pca: rocsolver_dsyevd did not converge (info = %d)\n", (int) info);
			return NTSM_PCA_E_SOLVER;
		}
	}
	for (uint32_t i = 0; i < d; ++i) {
		const double l = w[n - 1 - i], l1 = w[n - 1];
		if (!(l > (double) n * std::numeric_limits<double>::epsilon() * l1)) {
			if (bad_component) *bad_component = i;
			return NTSM_PCA_E_RANK;
		}
		eigval[i] = l;
		s[i] = std::sqrt(l);
	}

	HIPCHK(dev.buf.alloc(&dev.s, d_pad));
	HIPCHK(dev.buf.alloc(&dev.ud, (size_t) n * d_pad));
	HIPCHK(dev.buf.alloc(&dev.t, (size_t) n * d));
	HIPCHK(dev.buf.alloc(&dev.v, (size_t) p * d));
	HIPCHK(hipMemcpy(dev.s, s.data(), d_pad * sizeof(double), hipMemcpyHostToDevice));
	HIPCHK(hipEventRecord(dev.ev[0], 0));
	ntsm_pca_scores<<<dim3((unsigned) (((size_t) n * d_pad + 255) / 256)), dim3(256)>>>(dev.g, n, d, d_pad, dev.s, dev.ud, dev.t);
	HIPCHK(hipGetLastError());
	ntsm_pca_project<<<dim3((unsigned) (dev.p_pad / (4 * kProjRows)), d_pad / kProjComp), dim3(256)>>>(dev.a, dev.ld, n, p, dev.ud, d_pad,
	    dev.s, d, dev.v);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(dev.ev[1], 0));
	HIPCHK(hipEventSynchronize(dev.ev[1]));
	HIPCHK(hipEventElapsedTime(&ms, dev.ev[0], dev.ev[1]));
	tm.project_ms = ms;
	{
		auto t0 = std::chrono::steady_clock::now();
		HIPCHK(hipMemcpy(rot, dev.v, (size_t) p * d * sizeof(double), hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(comp, dev.t, (size_t) n * d * sizeof(double), hipMemcpyDeviceToHost));
		tm.download_ms = ms_since(t0);
	}
	/* sign (sklearn's svd_flip, v-based): the entry of v_i with the largest magnitude, the first on a tie, is positive */
	for (uint32_t i = 0; i < d; ++i) {
		double best = -1.0;
		bool neg = false;
		for (uint64_t k = 0; k < p; ++k) {
			const double x = rot[k * d + i];
			if (std::fabs(x) > best) { best = std::fabs(x); neg = std::signbit(x); }
		}
		if (!neg) continue;
		for (uint64_t k = 0; k < p; ++k) rot[k * d + i] = -rot[k * d + i];
		for (uint32_t j = 0; j < n; ++j) comp[(size_t) j * d + i] = -comp[(size_t) j * d + i];
	}
	if (times) *times = tm;
	if (expand_ms) *expand_ms = dev.expand_ms;
	return 0;
}

Source host_matrix(const double *a)
{
	Source src;
	src.a = a;
	return src;
}
Source cell_matrix(const uint16_t *cells, const double *value, const double *row_fill, uint64_t first_undef_cell)
{
	Source src;
	src.cells = cells;
	src.value = value;
	src.row_fill = row_fill;
	src.first_undef_cell = first_undef_cell;
	return src;
}
Source store_matrix(const void *db_counts, uint64_t db_stride_bytes, uint32_t min_cov, uint32_t db_chunk)
{
	Source src;
	src.db = db_counts;
	src.db_stride = db_stride_bytes;
	src.min_cov = min_cov;
	src.db_chunk = db_chunk;
	return src;
}

} // namespace

#define NTSM_PCA_EXPORT extern "C" __attribute__((visibility("default")))

NTSM_PCA_EXPORT int ntsm_pca_gram(int device, uint64_t p, uint32_t n, const double *a, int centre, uint32_t split, double *gram,
		double *means, ntsm_pca_times *times)
{
	if (!args_ok(p, n, a) || !gram) return NTSM_PCA_E_ARG;
	return gram_of(device, p, n, host_matrix(a), centre, split, gram, means, times, nullptr);
}

NTSM_PCA_EXPORT int ntsm_pca_run(int device, uint64_t p, uint32_t n, const double *a, uint32_t d, uint32_t split, double *eigval,
		double *rot, double *comp, uint32_t *bad_component, ntsm_pca_times *times)
{
	if (!args_ok(p, n, a) || !run_args_ok(p, n, d, eigval, rot, comp)) return NTSM_PCA_E_ARG;
	return run_of(device, p, n, host_matrix(a), d, split, eigval, rot, comp, bad_component, times, nullptr);
}

NTSM_PCA_EXPORT int ntsm_pca_expand_cells(int device, uint64_t p, uint32_t n, const uint16_t *cells, const double *value,
		const double *row_fill, uint64_t first_undef_cell, double *a, double *expand_ms)
{
	const Source src = cell_matrix(cells, value, row_fill, first_undef_cell);
	if (!args_ok(p, n, src) || !a) return NTSM_PCA_E_ARG;
	ntsm_pca_times tm = {};
	Device dev;
	if (const int rc = matrix_on_device(dev, device, p, n, src, tm)) return rc;
	HIPCHK(hipMemcpy2D(a, (size_t) n * sizeof(double), dev.a, dev.ld * sizeof(double), (size_t) n * sizeof(double), p, hipMemcpyDeviceToHost));
	if (expand_ms) *expand_ms = dev.expand_ms;
	return 0;
}

NTSM_PCA_EXPORT int ntsm_pca_gram_cells(int device, uint64_t p, uint32_t n, const uint16_t *cells, const double *value,
		const double *row_fill, uint64_t first_undef_cell, int centre, uint32_t split, double *gram, double *means,
		ntsm_pca_times *times, double *expand_ms)
{
	const Source src = cell_matrix(cells, value, row_fill, first_undef_cell);
	if (!args_ok(p, n, src) || !gram) return NTSM_PCA_E_ARG;
	return gram_of(device, p, n, src, centre, split, gram, means, times, expand_ms);
}

NTSM_PCA_EXPORT int ntsm_pca_run_cells(int device, uint64_t p, uint32_t n, const uint16_t *cells, const double *value,
		const double *row_fill, uint64_t first_undef_cell, uint32_t d, uint32_t split, double *eigval, double *rot, double *comp,
		uint32_t *bad_component, ntsm_pca_times *times, double *expand_ms)
{
	const Source src = cell_matrix(cells, value, row_fill, first_undef_cell);
	if (!args_ok(p, n, src) || !run_args_ok(p, n, d, eigval, rot, comp)) return NTSM_PCA_E_ARG;
	return run_of(device, p, n, src, d, split, eigval, rot, comp, bad_component, times, expand_ms);
}

NTSM_PCA_EXPORT int ntsm_pca_store_cells(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n, uint64_t n_sites,
		uint32_t min_cov, uint32_t db_chunk, uint16_t *cells, uint32_t *tallies, ntsm_pca_store_times *store_times)
{
	const Source src = store_matrix(db_counts, db_stride_bytes, min_cov, db_chunk);
	if (!args_ok(n_sites, n, src) || !cells || !tallies) return NTSM_PCA_E_ARG;
	Device dev;
	HIPCHK(hipSetDevice(device));
	HIPCHK(dev.ev.create());
	if (const int rc = store_cells_on_device(dev, n_sites, n, src)) return rc;
	HIPCHK(hipMemcpy2D(cells, (size_t) n * sizeof(uint16_t), dev.cells, (size_t) dev.cell_ld * sizeof(uint16_t), (size_t) n * sizeof(uint16_t), n_sites,
	    hipMemcpyDeviceToHost));
	std::copy(dev.tallies.begin(), dev.tallies.end(), tallies);
	if (store_times) *store_times = dev.st;
	return 0;
}

NTSM_PCA_EXPORT int ntsm_pca_run_store(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n, uint64_t n_sites,
		uint32_t min_cov, uint32_t db_chunk, uint32_t d, uint32_t split, double *eigval, double *rot, double *comp, uint32_t *tallies,
		uint32_t *bad_component, ntsm_pca_times *times, ntsm_pca_store_times *store_times)
{
	const Source src = store_matrix(db_counts, db_stride_bytes, min_cov, db_chunk);
	if (!args_ok(n_sites, n, src) || !run_args_ok(n_sites, n, d, eigval, rot, comp) || !tallies) return NTSM_PCA_E_ARG;
	return run_of(device, n_sites, n, src, d, split, eigval, rot, comp, bad_component, times, nullptr, tallies, store_times);
}
