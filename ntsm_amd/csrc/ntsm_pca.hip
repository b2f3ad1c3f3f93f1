/*
 * ntsm_pca.hip -- device steps of ntsmPCA for the MI355X (gfx950); the contract is in include/ntsm_pca_hip.h,
 * the design in DESIGN.md section 11.
 *
 * The uploaded matrix lives in a zero-padded buffer [p_pad][ld] (ld = n rounded up to the 128-sample tile, p_pad = p
 * rounded up to the 16-site chunk), so no kernel has a ragged inner loop: the padding contributes exact zeros.
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

namespace {

constexpr int kTile = 128;                   /* samples per tile edge */
constexpr int kChunk = 16;                   /* sites per LDS stage */
constexpr int kLds = kTile + 16;             /* LDS row stride in doubles: rows r and r + 1 of a ds_read_b64 half-wave fall
                                              * 32 banks apart (1152 B), so its 2 x 16 lanes cover the 64 banks once */
constexpr int kProjRows = 4, kProjComp = 8;  /* per wave of the projection kernel */

typedef double v4d __attribute__((ext_vector_type(4)));

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
	ntsm_hip::Events<3> ev;
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

bool args_ok(uint64_t p, uint32_t n, const double *a)
{
	return a && p >= 1 && n >= 1 && p < (1ull << 31) && n < (1u << 24);
}

/* upload, centre, Gram: leaves Ac (or A) in dev.a, the means in dev.means and G in dev.g */
int gram_on_device(Device &dev, int device, uint64_t p, uint32_t n, const double *a, int centre, uint32_t split, ntsm_pca_times &tm)
{
	float ms = 0;
	const uint32_t edge = (n + kTile - 1) / kTile, n_tiles = edge * (edge + 1) / 2;
	const uint32_t chunks = (uint32_t) ((p + kChunk - 1) / kChunk);
	dev.ld = (size_t) edge * kTile;
	dev.p_pad = (uint64_t) chunks * kChunk;
	uint32_t pieces = split, cpp = 0;
	hipDeviceProp_t prop;
	auto t0 = std::chrono::steady_clock::now();
	HIPCHK(hipSetDevice(device));
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
	HIPCHK(dev.ev.create());
	HIPCHK(dev.buf.alloc(&dev.a, dev.p_pad * dev.ld));
	HIPCHK(dev.buf.alloc(&dev.means, dev.p_pad));
	HIPCHK(dev.buf.alloc(&dev.partial, (size_t) pieces * n_tiles * kTile * kTile));
	HIPCHK(dev.buf.alloc(&dev.g, (size_t) n * n));
	HIPCHK(hipMemset(dev.a, 0, dev.p_pad * dev.ld * sizeof(double)));
	HIPCHK(hipMemcpy2D(dev.a, dev.ld * sizeof(double), a, (size_t) n * sizeof(double), (size_t) n * sizeof(double), p, hipMemcpyHostToDevice));
	HIPCHK(hipDeviceSynchronize());
	tm.upload_ms = ms_since(t0);

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

} // namespace

extern "C" __attribute__((visibility("default"))) int ntsm_pca_gram(int device, uint64_t p, uint32_t n, const double *a,
		int centre, uint32_t split, double *gram, double *means, ntsm_pca_times *times)
{
	if (!args_ok(p, n, a) || !gram) return NTSM_PCA_E_ARG;
	ntsm_pca_times tm = {};
	Device dev;
	if (const int rc = gram_on_device(dev, device, p, n, a, centre, split, tm)) return rc;
	auto t0 = std::chrono::steady_clock::now();
	HIPCHK(hipMemcpy(gram, dev.g, (size_t) n * n * sizeof(double), hipMemcpyDeviceToHost));
	if (means) HIPCHK(hipMemcpy(means, dev.means, p * sizeof(double), hipMemcpyDeviceToHost));
	tm.download_ms = ms_since(t0);
	if (times) *times = tm;
	return 0;
}

extern "C" __attribute__((visibility("default"))) int ntsm_pca_run(int device, uint64_t p, uint32_t n, const double *a,
		uint32_t d, uint32_t split, double *eigval, double *rot, double *comp, uint32_t *bad_component, ntsm_pca_times *times)
{
	if (!args_ok(p, n, a) || n < 2 || d < 1 || d > n || d > p || !eigval || !rot || !comp) return NTSM_PCA_E_ARG;
	const Solver &sv = solver_bind();
	if (!sv.ok) return NTSM_PCA_E_SOLVER_MISSING;
	float ms = 0;
	ntsm_pca_times tm = {};
	Device dev;
	Handle handle(sv);
	rocblas_int info = 0;
	const uint32_t d_pad = (d + kProjComp - 1) / kProjComp * kProjComp;
	std::vector<double> w(n), s(d_pad, 1.0);
	if (const int rc = gram_on_device(dev, device, p, n, a, 1, split, tm)) return rc;

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
	return 0;
}
