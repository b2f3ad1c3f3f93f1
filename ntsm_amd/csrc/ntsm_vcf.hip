/*
 * ntsm_vcf.hip -- the device step of ntsmVCF on one MI355X (include/ntsm_vcf_hip.h; reference: MultiCount::insertCount,
 * src/MultiCount.hpp:51-68, as VCFConvert::count calls it, src/VCFConvert.hpp:151-170, and the maxima and sums of
 * MultiCount::printNormMatrix, :156-187).
 *
 * State kernel: one workgroup per site, each lane 16 consecutive samples (one 128-bit load of a G row per event).  For
 * every key of the site's REF list, then of its VAR list, the lane walks the key's events in ordinal order with the 16
 * bytes of state in registers, applies insertCount's rule, and folds the final bytes into maxREF / maxVAR.  All lanes of
 * a workgroup walk the same events, so the loops are uniform; the G row of a line is shared by the ~2 x (W - k + 1)
 * keys of its site and comes from L2 after the first.  Warnings take a slot through one atomic counter; their content
 * does not depend on the slot, and the host sorts them into the one-thread order.
 * Sum kernel: one lane per site, the reference's sequential double sum over the samples (correctly rounded division,
 * built with -ffp-contract=off), plus the first sample with a zero denominator.
 * Records kernel (ntsm_vcf_records; MultiCount::printCountsMax, :93-138): the same walk over a window of samples, keeping
 * the sums of the final bytes beside their maxima, and leaving the device sample-major through a tile in LDS (below).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>

#include "../../include/ntsm_vcf_hip.h"
#define NTSM_HIP_TAG "ntsm_vcf"
#include "ntsm_hip_scope.h"

namespace {

constexpr int kLane = 16;                    /* samples per lane */
constexpr uint64_t kWarnInit = 1u << 16;     /* warning records the device buffer starts with; grown (and the kernels re-run) on overflow */

/* kWarn = false: the records kernel, which reports no warnings (warn, warn_cap and n_warn are not read) */
template <bool kWarn> __device__ __forceinline__ void apply(uint8_t (&st)[kLane], uint4 g, uint32_t side, uint32_t v1, uint32_t v2, uint32_t ord,
		uint32_t s0, uint32_t n_samples, ntsm_vcf_warning *warn, unsigned long long warn_cap, unsigned long long *n_warn)
{
	const uint32_t w[4] = { g.x, g.y, g.z, g.w };
	/* REF side: hom1 -> 2m, het -> m; VAR side: hom2 -> 2m, het -> m (VCFConvert.hpp:151-170) */
	const uint32_t full = side ? NTSM_VCF_HOM2 : NTSM_VCF_HOM1;
#pragma unroll
	for (int j = 0; j < kLane; ++j) {
		const uint32_t code = (w[j >> 2] >> ((j & 3) * 8)) & 0xFFu;
		if (code != full && code != NTSM_VCF_HET) continue;       /* no insert (also the padding) */
		const uint32_t value = code == full ? v2 : v1;
		const uint32_t old = st[j];
		if (old != 0) {                                            /* MultiCount.hpp:57-62 */
			if (kWarn && old != value && s0 + j < n_samples) {
				const unsigned long long slot = atomicAdd(n_warn, 1ull);
				if (slot < warn_cap) warn[slot] = ntsm_vcf_warning { ord, s0 + (uint32_t) j, old, value };
			}
		} else {
			st[j] = (uint8_t) value;                               /* the CAS stores the truncated value */
		}
	}
}

__global__ __launch_bounds__(256) void ntsm_vcf_state(uint32_t n_samples, uint32_t v1, uint32_t v2, const uint8_t *geno, uint32_t g_stride,
		const uint64_t *key_off, const uint32_t *ev_ord, const uint32_t *ev_ls, const uint64_t *site_off, const uint32_t *site_keys,
		uint16_t *cells, ntsm_vcf_warning *warn, unsigned long long warn_cap, unsigned long long *n_warn)
{
	const uint64_t site = blockIdx.x;
	const uint32_t n_chunks = (n_samples + kLane - 1) / kLane;
	for (uint32_t chunk = threadIdx.x; chunk < n_chunks; chunk += blockDim.x) {
		const uint32_t s0 = chunk * kLane;
		uint8_t mx[2][kLane];
#pragma unroll
		for (int j = 0; j < kLane; ++j) mx[0][j] = mx[1][j] = 0;
		for (uint32_t side = 0; side < 2; ++side) {
			for (uint64_t ki = site_off[2 * site + side]; ki < site_off[2 * site + side + 1]; ++ki) {
				const uint32_t key = site_keys[ki];
				uint8_t st[kLane];
#pragma unroll
				for (int j = 0; j < kLane; ++j) st[j] = 0;
				for (uint64_t e = key_off[key]; e < key_off[key + 1]; ++e) {
					const uint32_t ls = ev_ls[e];
					const uint4 g = *reinterpret_cast<const uint4 *>(geno + (uint64_t) (ls >> 1) * g_stride + s0);
					apply<true>(st, g, ls & 1u, v1, v2, ev_ord[e], s0, n_samples, warn, warn_cap, n_warn);
				}
#pragma unroll
				for (int j = 0; j < kLane; ++j) mx[side][j] = st[j] > mx[side][j] ? st[j] : mx[side][j];
			}
		}
		uint16_t *row = cells + site * n_samples;
#pragma unroll
		for (int j = 0; j < kLane; ++j)
			if (s0 + j < n_samples) row[s0 + j] = (uint16_t) (mx[0][j] | (mx[1][j] << 8));
	}
}

/* printNormMatrix's per-row loop (:162-187): sum += double(maxREF) / double(denom) in sample order */
__global__ __launch_bounds__(256) void ntsm_vcf_sums(uint64_t n_sites, uint32_t n_samples, const uint16_t *cells, double *sums, uint32_t *first_undef)
{
	const uint64_t site = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (site >= n_sites) return;
	const uint16_t *row = cells + site * n_samples;
	double sum = 0.0;
	uint32_t first = n_samples;
	for (uint32_t j = 0; j < n_samples; ++j) {
		const uint32_t c = row[j], r = c & 0xFFu, denom = r + (c >> 8);
		if (denom == 0) {
			if (first == n_samples) first = j;
		} else {
			sum = __dadd_rn(sum, __ddiv_rn((double) r, (double) denom));
		}
	}
	sums[site] = sum;
	first_undef[site] = first;
}

/*
 * Records kernel.  Tile: kTileSites = 32 sites x kTileSamples = 128 samples per workgroup of 256 lanes.  Walk: lane
 * (slot, l) = (tid / 8, tid % 8) walks site slot of the tile for the 16 samples of chunk l, as the state kernel does (one
 * 128-bit load of a G row per event; the 8 lanes of a site read 128 contiguous bytes), and keeps maxima and 32-bit sums of
 * the final bytes per side.  The 8 sites of a wave have lists of their own, so a wave runs as long as its longest site.
 * The tile is staged in LDS site-major and written sample-major: in the second phase lane (w, i) = (tid / 32, tid % 32)
 * writes site i of sample w, w + 8, ..., so the 32 lanes of a half wave store one sample's run of 32 consecutive sites,
 * 256 contiguous bytes per array, with 8-byte stores.  Row pitches of 130 uint16 (65 dwords) and 129 uint2 (258 dwords)
 * make both phase-2 reads conflict-free (32 lanes, 32 distinct banks / bank pairs).  Totals: every walking lane adds its
 * 16 x 2 values to 64-bit LDS counters of the tile's samples, and one 64-bit global atomicAdd per sample and total
 * leaves the tile; integer adds, so their order cannot change the result.
 * LDS: 8,320 B maxima + 33,024 B sums + 2,048 B totals = 43,392 B with sums (3 workgroups = 12 waves per CU of 160 KiB);
 * 10,368 B without (kSums = false; the 107 VGPRs of the walk then decide: 4 waves per SIMD, 4 workgroups per CU).
 */
constexpr int kTileSites = 32, kTileChunks = 8, kTileSamples = kTileChunks * kLane;
constexpr int kMaxPitch = kTileSamples + 2, kSumPitch = kTileSamples + 1;   /* elements of uint16 / uint2 */

template <bool kSums> __global__ __launch_bounds__(256) void ntsm_vcf_records_tile(uint32_t s_count, uint32_t w_stride, uint32_t n_sample_tiles,
		uint64_t n_sites, uint32_t v1, uint32_t v2, const uint8_t *geno, const uint64_t *key_off, const uint32_t *ev_ls,
		const uint64_t *site_off, const uint32_t *site_keys, uint2 *counts, uint2 *sums, unsigned long long *total, unsigned long long *sum_of_sums)
{
	__shared__ uint16_t l_max[kTileSites * kMaxPitch];
	__shared__ uint2 l_sum[kSums ? kTileSites * kSumPitch : 1];
	__shared__ unsigned long long l_tot[2][kTileSamples];
	const uint32_t tid = threadIdx.x;
	const uint32_t sample_tile = blockIdx.x % n_sample_tiles;
	const uint64_t site0 = (uint64_t) (blockIdx.x / n_sample_tiles) * kTileSites;
	if (tid < kTileSamples) l_tot[0][tid] = l_tot[1][tid] = 0;
	__syncthreads();
	{
		const uint32_t slot = tid / kTileChunks, c0 = (tid % kTileChunks) * kLane;   /* c0: first sample of the chunk, in the tile */
		const uint32_t s0 = sample_tile * kTileSamples + c0;                          /* ... in the window */
		const uint64_t site = site0 + slot;
		uint8_t mx[2][kLane];
		uint32_t sm[2][kLane];
#pragma unroll
		for (int j = 0; j < kLane; ++j) { mx[0][j] = mx[1][j] = 0; sm[0][j] = sm[1][j] = 0; }
		const bool walks = site < n_sites && s0 < w_stride;       /* a chunk past the window's columns has no G bytes */
		if (walks) {
			for (uint32_t side = 0; side < 2; ++side) {
				for (uint64_t ki = site_off[2 * site + side]; ki < site_off[2 * site + side + 1]; ++ki) {
					const uint32_t key = site_keys[ki];
					uint8_t st[kLane];
#pragma unroll
					for (int j = 0; j < kLane; ++j) st[j] = 0;
					for (uint64_t e = key_off[key]; e < key_off[key + 1]; ++e) {
						const uint32_t ls = ev_ls[e];
						const uint4 g = *reinterpret_cast<const uint4 *>(geno + (uint64_t) (ls >> 1) * w_stride + s0);
						apply<false>(st, g, ls & 1u, v1, v2, 0, s0, s_count, nullptr, 0, nullptr);
					}
#pragma unroll
					for (int j = 0; j < kLane; ++j) {
						mx[side][j] = st[j] > mx[side][j] ? st[j] : mx[side][j];
						sm[side][j] += st[j];
					}
				}
			}
		}
#pragma unroll
		for (int j = 0; j < kLane; ++j) {
			l_max[slot * kMaxPitch + c0 + j] = (uint16_t) (mx[0][j] | (mx[1][j] << 8));
			if (kSums) l_sum[slot * kSumPitch + c0 + j] = make_uint2(sm[0][j], sm[1][j]);
			if (walks && s0 + j < s_count) {                       /* columns past s_count may hold the next window's samples */
				atomicAdd(&l_tot[0][c0 + j], (unsigned long long) ((uint32_t) mx[0][j] + mx[1][j]));
				atomicAdd(&l_tot[1][c0 + j], (unsigned long long) (uint32_t) (sm[0][j] + sm[1][j]));
			}
		}
	}
	__syncthreads();
	const uint32_t i = tid % kTileSites;
	const uint64_t site = site0 + i;
	for (uint32_t w = tid / kTileSites; w < (uint32_t) kTileSamples; w += 256 / kTileSites) {
		const uint32_t sample = sample_tile * kTileSamples + w;
		if (sample >= s_count || site >= n_sites) continue;
		const uint32_t c = l_max[i * kMaxPitch + w];
		counts[(uint64_t) sample * n_sites + site] = make_uint2(c & 0xFFu, c >> 8);
		if (kSums) sums[(uint64_t) sample * n_sites + site] = l_sum[i * kSumPitch + w];
	}
	if (tid < (uint32_t) kTileSamples && sample_tile * kTileSamples + tid < s_count) {
		atomicAdd(&total[sample_tile * kTileSamples + tid], l_tot[0][tid]);
		atomicAdd(&sum_of_sums[sample_tile * kTileSamples + tid], l_tot[1][tid]);
	}
}

double now_ms()
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

/* what ntsm_vcf_run and ntsm_vcf_records refuse of the lists: every index the kernels follow is checked here, on the host,
 * so nothing on the device reads out of bounds */
bool lists_ok(uint32_t n_samples, uint64_t n_lines, const uint8_t *geno, uint32_t g_stride, uint64_t n_keys, const uint64_t *key_off,
		uint64_t n_events, const uint32_t *ev_ord, const uint32_t *ev_ls, uint64_t n_sites, const uint64_t *site_off, const uint32_t *site_keys)
{
	if (g_stride % kLane != 0 || g_stride < n_samples || (n_lines && !geno) || !key_off || (n_events && (!ev_ord || !ev_ls))) return false;
	if (n_lines > 0x7FFFFFFFull || n_keys >= 0xFFFFFFFFull || n_sites > 0x7FFFFFFFull) return false;
	if (key_off[0] != 0 || key_off[n_keys] != n_events) return false;
	for (uint64_t q = 0; q < n_keys; ++q)
		if (key_off[q + 1] < key_off[q]) return false;
	for (uint64_t e = 0; e < n_events; ++e)
		if ((ev_ls[e] >> 1) >= n_lines) return false;
	if (n_sites) {
		const uint64_t n_site_keys = site_off[2 * n_sites];
		if (site_off[0] != 0 || (n_site_keys && !site_keys)) return false;
		for (uint64_t i = 0; i < 2 * n_sites; ++i)
			if (site_off[i + 1] < site_off[i]) return false;
		for (uint64_t i = 0; i < n_site_keys; ++i)
			if (site_keys[i] >= n_keys) return false;
	}
	return true;
}

} // namespace

extern "C" int ntsm_vcf_run(int device, uint32_t n_samples, uint32_t multi,
		uint64_t n_lines, const uint8_t *geno, uint32_t g_stride,
		uint64_t n_keys, const uint64_t *key_off, uint64_t n_events, const uint32_t *ev_ord, const uint32_t *ev_ls,
		uint64_t n_sites, const uint64_t *site_off, const uint32_t *site_keys,
		uint16_t *cells, double *sums, uint32_t *first_undef,
		ntsm_vcf_warning *warn, uint64_t warn_cap, uint64_t *n_warn, ntsm_vcf_times *times)
{
	if (!n_warn || (n_sites && (!site_off || !sums || !first_undef)) || (n_sites && n_samples && !cells)) return -1;
	if (!lists_ok(n_samples, n_lines, geno, g_stride, n_keys, key_off, n_events, ev_ord, ev_ls, n_sites, site_off, site_keys)) return -1;
	const uint64_t n_site_keys = n_sites ? site_off[2 * n_sites] : 0;
	const uint32_t v1 = multi, v2 = multi * 2u;               /* opt::multi, opt::multi * 2 (unsigned) */
	const uint64_t n_cells = n_sites * (uint64_t) n_samples;
	double t_up = 0, t_down = 0;
	float ms_state = 0, ms_sum = 0;
	uint64_t launches = 0;
	*n_warn = 0;
	/* the device part: a HIP failure leaves it at once, its buffers and events released, and the times below are still filled */
	const auto on_device = [&]() -> int {
		ntsm_hip::Buffers b;
		ntsm_hip::Events<3> ev;
		uint8_t *d_geno;
		uint64_t *d_key_off, *d_site_off;
		uint32_t *d_ev_ord, *d_ev_ls, *d_site_keys, *d_first;
		uint16_t *d_cells;
		double *d_sums;
		ntsm_vcf_warning *d_warn;
		unsigned long long *d_n_warn, h_n_warn = 0, d_cap = std::min<uint64_t>(std::max<uint64_t>(warn_cap, 1), kWarnInit);
		int rc = 0;
		double t0 = now_ms();
		HIPCHK(hipSetDevice(device));
		HIPCHK(ev.create());
		/* +1 element everywhere: no zero-byte allocations */
		HIPCHK(b.alloc(&d_geno, n_lines * g_stride + kLane));
		HIPCHK(b.alloc(&d_key_off, n_keys + 1));
		HIPCHK(b.alloc(&d_ev_ord, n_events + 1));
		HIPCHK(b.alloc(&d_ev_ls, n_events + 1));
		HIPCHK(b.alloc(&d_site_off, 2 * n_sites + 1));
		HIPCHK(b.alloc(&d_site_keys, n_site_keys + 1));
		HIPCHK(b.alloc(&d_cells, n_cells + 1));
		HIPCHK(b.alloc(&d_sums, n_sites));
		HIPCHK(b.alloc(&d_first, n_sites));
		HIPCHK(b.alloc(&d_warn, d_cap));
		HIPCHK(b.alloc(&d_n_warn, 1));
		if (n_lines) HIPCHK(hipMemcpy(d_geno, geno, n_lines * g_stride, hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(d_key_off, key_off, (n_keys + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
		if (n_events) {
			HIPCHK(hipMemcpy(d_ev_ord, ev_ord, n_events * sizeof(uint32_t), hipMemcpyHostToDevice));
			HIPCHK(hipMemcpy(d_ev_ls, ev_ls, n_events * sizeof(uint32_t), hipMemcpyHostToDevice));
		}
		HIPCHK(hipMemcpy(d_site_off, site_off, (2 * n_sites + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
		if (n_site_keys) HIPCHK(hipMemcpy(d_site_keys, site_keys, n_site_keys * sizeof(uint32_t), hipMemcpyHostToDevice));
		t_up = now_ms() - t0;
		for (;;) {                                                 /* a second pass only if the warning buffer overflowed */
			HIPCHK(hipMemset(d_n_warn, 0, sizeof(unsigned long long)));
			HIPCHK(hipEventRecord(ev[0], 0));
			if (n_samples) {
				const uint32_t n_chunks = (n_samples + kLane - 1) / kLane;
				const uint32_t block = std::min<uint32_t>(256, (n_chunks + 63) / 64 * 64);
				hipLaunchKernelGGL(ntsm_vcf_state, dim3((uint32_t) n_sites), dim3(block), 0, 0, n_samples, v1, v2, d_geno, g_stride,
				    d_key_off, d_ev_ord, d_ev_ls, d_site_off, d_site_keys, d_cells, d_warn, d_cap, d_n_warn);
				HIPCHK(hipGetLastError());
				++launches;
			}
			HIPCHK(hipEventRecord(ev[1], 0));
			hipLaunchKernelGGL(ntsm_vcf_sums, dim3((uint32_t) ((n_sites + 255) / 256)), dim3(256), 0, 0, n_sites, n_samples, d_cells, d_sums, d_first);
			HIPCHK(hipGetLastError());
			HIPCHK(hipEventRecord(ev[2], 0));
			HIPCHK(hipEventSynchronize(ev[2]));
			HIPCHK(hipMemcpy(&h_n_warn, d_n_warn, sizeof(h_n_warn), hipMemcpyDeviceToHost));
			if (h_n_warn <= d_cap) break;
			HIPCHK(b.release(&d_warn));                            /* freed first: the two sizes are never held together */
			d_cap = h_n_warn;
			HIPCHK(b.alloc(&d_warn, d_cap));
		}
		HIPCHK(hipEventElapsedTime(&ms_state, ev[0], ev[1]));
		HIPCHK(hipEventElapsedTime(&ms_sum, ev[1], ev[2]));
		*n_warn = h_n_warn;
		t0 = now_ms();
		if (n_cells) HIPCHK(hipMemcpy(cells, d_cells, n_cells * sizeof(uint16_t), hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(sums, d_sums, n_sites * sizeof(double), hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(first_undef, d_first, n_sites * sizeof(uint32_t), hipMemcpyDeviceToHost));
		if (h_n_warn > warn_cap) rc = NTSM_VCF_E_CAPACITY;
		else if (h_n_warn) HIPCHK(hipMemcpy(warn, d_warn, h_n_warn * sizeof(ntsm_vcf_warning), hipMemcpyDeviceToHost));
		t_down = now_ms() - t0;
		return rc;
	};
	const int rc = n_sites ? on_device() : 0;
	if (times) {
		times->upload_ms = t_up;
		times->state_kernel_ms = ms_state;
		times->sum_kernel_ms = ms_sum;
		times->download_ms = t_down;
		/* G rows of the used lines, the event and key lists once, and the cells written */
		times->kernel_bytes = n_lines * (uint64_t) g_stride + n_events * 8 + (n_keys + 1) * 8 + n_site_keys * 4 + n_cells * 2;
		times->state_launches = launches;
	}
	return rc;
}

extern "C" int ntsm_vcf_records(int device, uint32_t n_samples, uint32_t multi,
		uint64_t n_lines, const uint8_t *geno, uint32_t g_stride,
		uint64_t n_keys, const uint64_t *key_off, uint64_t n_events, const uint32_t *ev_ord, const uint32_t *ev_ls,
		uint64_t n_sites, const uint64_t *site_off, const uint32_t *site_keys,
		uint32_t s_begin, uint32_t s_count,
		uint32_t *counts, uint64_t counts_pitch, uint32_t *sums, uint64_t sums_pitch,
		uint64_t *total, uint64_t *sum_of_sums, ntsm_vcf_records_times *times)
{
	if (!total || !sum_of_sums || (n_sites && (!site_off || !counts))) return -1;
	if (s_begin % kLane != 0 || s_count < 1 || s_begin > n_samples || s_count > n_samples - s_begin) return -1;
	const uint64_t row_bytes = 8 * n_sites;
	if (counts_pitch % 8 != 0 || counts_pitch < row_bytes || (sums && (sums_pitch % 8 != 0 || sums_pitch < row_bytes))) return -1;
	if (!lists_ok(n_samples, n_lines, geno, g_stride, n_keys, key_off, n_events, ev_ord, ev_ls, n_sites, site_off, site_keys)) return -1;
	const uint64_t n_site_keys = n_sites ? site_off[2 * n_sites] : 0;
	/* the window's columns: s_count rounded up to whole 16-sample chunks, inside the row because g_stride is a multiple of 16 */
	const uint32_t w_stride = (s_count + kLane - 1) / kLane * kLane;
	const uint32_t n_sample_tiles = (w_stride + kTileSamples - 1) / kTileSamples;
	const uint64_t n_site_tiles = (n_sites + kTileSites - 1) / kTileSites, n_pairs = n_sites * (uint64_t) s_count;
	if (n_site_tiles * n_sample_tiles > 0x7FFFFFFFull) return -1;
	const uint32_t v1 = multi, v2 = multi * 2u;
	double t_up = 0, t_down = 0;
	float ms_kernel = 0;
	uint64_t up_bytes = 0, down_bytes = 0;
	std::fill(total, total + s_count, 0);
	std::fill(sum_of_sums, sum_of_sums + s_count, 0);
	const auto on_device = [&]() -> int {
		ntsm_hip::Buffers b;
		ntsm_hip::Events<2> ev;
		uint8_t *d_geno;
		uint64_t *d_key_off, *d_site_off;
		uint32_t *d_ev_ls, *d_site_keys;
		uint2 *d_counts, *d_sums = nullptr;
		unsigned long long *d_tot;                                 /* [2][s_count]: total, sum_of_sums */
		double t0 = now_ms();
		HIPCHK(hipSetDevice(device));
		HIPCHK(ev.create());
		HIPCHK(b.alloc(&d_geno, n_lines * w_stride + kLane));
		HIPCHK(b.alloc(&d_key_off, n_keys + 1));
		HIPCHK(b.alloc(&d_ev_ls, n_events + 1));
		HIPCHK(b.alloc(&d_site_off, 2 * n_sites + 1));
		HIPCHK(b.alloc(&d_site_keys, n_site_keys + 1));
		HIPCHK(b.alloc(&d_counts, n_pairs));
		if (sums) HIPCHK(b.alloc(&d_sums, n_pairs));
		HIPCHK(b.alloc(&d_tot, 2 * (uint64_t) s_count));
		if (n_lines) HIPCHK(hipMemcpy2D(d_geno, w_stride, geno + s_begin, g_stride, w_stride, n_lines, hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(d_key_off, key_off, (n_keys + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
		if (n_events) HIPCHK(hipMemcpy(d_ev_ls, ev_ls, n_events * sizeof(uint32_t), hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(d_site_off, site_off, (2 * n_sites + 1) * sizeof(uint64_t), hipMemcpyHostToDevice));
		if (n_site_keys) HIPCHK(hipMemcpy(d_site_keys, site_keys, n_site_keys * sizeof(uint32_t), hipMemcpyHostToDevice));
		HIPCHK(hipMemset(d_tot, 0, 2 * (uint64_t) s_count * sizeof(unsigned long long)));
		up_bytes = n_lines * w_stride + (n_keys + 1) * 8 + n_events * 4 + (2 * n_sites + 1) * 8 + n_site_keys * 4;
		t_up = now_ms() - t0;
		HIPCHK(hipEventRecord(ev[0], 0));
		const dim3 grid((uint32_t) (n_site_tiles * n_sample_tiles)), block(256);
		if (sums)
			hipLaunchKernelGGL(ntsm_vcf_records_tile<true>, grid, block, 0, 0, s_count, w_stride, n_sample_tiles, n_sites, v1, v2, d_geno,
			    d_key_off, d_ev_ls, d_site_off, d_site_keys, d_counts, d_sums, d_tot, d_tot + s_count);
		else
			hipLaunchKernelGGL(ntsm_vcf_records_tile<false>, grid, block, 0, 0, s_count, w_stride, n_sample_tiles, n_sites, v1, v2, d_geno,
			    d_key_off, d_ev_ls, d_site_off, d_site_keys, d_counts, d_sums, d_tot, d_tot + s_count);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(ev[1], 0));
		HIPCHK(hipEventSynchronize(ev[1]));
		HIPCHK(hipEventElapsedTime(&ms_kernel, ev[0], ev[1]));
		t0 = now_ms();
		/* one 2-D copy per array: device rows of 8 * n_sites bytes to the caller's pitch */
		HIPCHK(hipMemcpy2D(counts, counts_pitch, d_counts, row_bytes, row_bytes, s_count, hipMemcpyDeviceToHost));
		if (sums) HIPCHK(hipMemcpy2D(sums, sums_pitch, d_sums, row_bytes, row_bytes, s_count, hipMemcpyDeviceToHost));
		static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "the totals are copied as they are");
		HIPCHK(hipMemcpy(total, d_tot, s_count * sizeof(uint64_t), hipMemcpyDeviceToHost));
		HIPCHK(hipMemcpy(sum_of_sums, d_tot + s_count, s_count * sizeof(uint64_t), hipMemcpyDeviceToHost));
		down_bytes = n_pairs * 8 * (sums ? 2 : 1) + 16ull * s_count;
		t_down = now_ms() - t0;
		return 0;
	};
	const int rc = n_sites ? on_device() : 0;
	if (times) {
		times->upload_ms = t_up;
		times->kernel_ms = ms_kernel;
		times->download_ms = t_down;
		/* the window's G columns of the used lines, the event and key lists once, and the records written */
		times->kernel_bytes = n_lines * (uint64_t) w_stride + n_events * 4 + (n_keys + 1) * 8 + n_site_keys * 4 + (2 * n_sites + 1) * 8 +
		    n_pairs * 8 * (sums ? 2 : 1) + 16ull * s_count;
		times->upload_bytes = up_bytes;
		times->download_bytes = down_bytes;
	}
	return rc;
}
