/*
 * ntsm_eval_profile.hip -- the per-sample and per-site genotype tallies of a cohort store on one MI355X
 * (include/ntsm_eval_hip.h: ntsm_eval_store_profile; ntsmEval --qc).  The rule is calcHomHetMiss
 * (src/CompareCounts.hpp:742-767) with strict > min_cov: both alleles above is a het, exactly one a hom, neither a miss.  Per
 * sample that gives the row of computeScoreSingle (:541-585), per site the same three classes with the hom kept apart by
 * allele, plus the site's raw coverage.
 *
 * Layout.  One kernel, one read of each chunk's dense [sample][site][2] buffer, no transpose and no terms (so not
 * ntsm_eval_chunk::stage, only its copy).  A workgroup of four waves owns a tile of 64 sites x kStrip samples: the lanes
 * run along the sites -- one coalesced 8-byte load per lane and row --, wave w takes rows w, w + 4, ... of the strip.  A lane
 * keeps its site's four tallies and 64-bit coverage sum in registers.  A row's three classes are three ballots and their
 * population counts, which lane 0 stores to the row's LDS entry: a row belongs to one wave, so nothing in the loop is an
 * atomic.  At the tile's end the waves' site partials meet in LDS and one integer atomic per site and value, then one per
 * sample and class, goes to global memory; the grid's second dimension runs over strips of samples, so several workgroups
 * add into one site, and its first over tiles of sites, so several add into one sample.  A lane past n_sites and a row past
 * the chunk's end take part in no ballot and no sum (a padded lane would read as a miss).  Everything is an integer sum:
 * the result does not depend on the order of the adds, and two calls give the same bits.
 *
 * Chunks.  The store is walked as ntsm_eval_cross walks it: the chunk rule and the 2-D copy of ntsm_eval_chunk.h, one
 * kernel and one wait per chunk.  The outputs live on the device for the whole call, zeroed once, and come back once.
 * Device memory is O(chunk * n_sites + n_sites + n_db).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../include/ntsm_eval_hip.h"
#define NTSM_HIP_TAG "ntsm_eval_profile"
#include "ntsm_eval_chunk.h"
#include "ntsm_hip_scope.h"

namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr uint32_t kStrip = 256;             /* samples of one workgroup's tile: 64 rows per wave */

/* counts: the chunk's rows [n_rows][n_sites]; geno: the entry of the chunk's first row; any output may be null.
 * grid (tiles of 64 sites, strips of kStrip rows) */
__global__ __launch_bounds__(kThreads) void ntsm_eval_profile_kernel(const uint2 *__restrict__ counts, uint32_t n_rows, uint32_t n_sites,
		uint32_t min_cov, uint32_t *__restrict__ geno, uint32_t *__restrict__ site_tally, unsigned long long *__restrict__ site_cov)
{
	__shared__ uint32_t s_geno[kStrip][3];                   /* hets, homs, miss of the strip's rows */
	__shared__ uint32_t s_tally[kWaves][4][64];              /* each wave's homAT, homCG, het, miss of the tile's sites */
	__shared__ unsigned long long s_cov[kWaves][64];
	const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint32_t site = blockIdx.x * 64 + lane, row0 = blockIdx.y * kStrip;
	const bool live = site < n_sites;
	const uint32_t rows = min(kStrip, n_rows - row0);        /* row0 < n_rows by the grid */
	uint32_t hom_at = 0, hom_cg = 0, het = 0, miss = 0;
	unsigned long long cov = 0;
	for (uint32_t r = wave; r < rows; r += kWaves) {         /* wave-uniform: every lane reaches the ballots */
		uint2 c = make_uint2(0, 0);
		if (live) c = counts[(uint64_t) (row0 + r) * n_sites + site];
		const bool a = c.x > min_cov, b = c.y > min_cov;
		const bool is_het = live && a && b, is_hom = live && a != b, is_miss = live && !a && !b;
		hom_at += is_hom && a;
		hom_cg += is_hom && b;
		het += is_het;
		miss += is_miss;
		cov += (unsigned long long) c.x + c.y;                /* a dead lane adds 0 and is never read */
		if (geno) {
			const uint64_t m_het = __ballot(is_het), m_hom = __ballot(is_hom), m_miss = __ballot(is_miss);
			if (lane == 0) {
				s_geno[r][0] = (uint32_t) __popcll(m_het);
				s_geno[r][1] = (uint32_t) __popcll(m_hom);
				s_geno[r][2] = (uint32_t) __popcll(m_miss);
			}
		}
	}
	s_tally[wave][0][lane] = hom_at;
	s_tally[wave][1][lane] = hom_cg;
	s_tally[wave][2][lane] = het;
	s_tally[wave][3][lane] = miss;
	s_cov[wave][lane] = cov;
	__syncthreads();
	if (live) {
		if (site_tally) {                                    /* wave w adds value w of the tile's sites */
			uint32_t v = 0;
			for (int w = 0; w < kWaves; ++w) v += s_tally[w][wave][lane];
			if (v) atomicAdd(&site_tally[(uint64_t) site * 4 + wave], v);
		}
		if (site_cov && wave == 0) {
			unsigned long long v = 0;
			for (int w = 0; w < kWaves; ++w) v += s_cov[w][lane];
			if (v) atomicAdd(&site_cov[site], v);
		}
	}
	if (geno && threadIdx.x < rows)                          /* one thread per row of the strip: only rows a wave wrote */
		for (int k = 0; k < 3; ++k)
			if (s_geno[threadIdx.x][k]) atomicAdd(&geno[(uint64_t) (row0 + threadIdx.x) * 3 + k], s_geno[threadIdx.x][k]);
}

}  // namespace

extern "C" int ntsm_eval_store_profile(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n_db, uint32_t n_sites,
		uint32_t min_cov, uint32_t db_chunk, uint32_t *db_geno, uint32_t *site_tally, uint64_t *site_cov, ntsm_eval_cross_times *times)
{
	if (times) *times = ntsm_eval_cross_times {};
	if (!ntsm_eval_chunk::valid_store(db_counts, db_stride_bytes, n_db, n_sites) || (!db_geno && !site_tally && !site_cov)) return -1;
	if (db_geno && n_db) memset(db_geno, 0, (size_t) n_db * 3 * sizeof(uint32_t));
	if (site_tally && n_sites) memset(site_tally, 0, (size_t) n_sites * 4 * sizeof(uint32_t));
	if (site_cov && n_sites) memset(site_cov, 0, (size_t) n_sites * sizeof(uint64_t));
	if (n_db == 0 || n_sites == 0) return 0;

	const uint64_t row_bytes = 8ull * n_sites;
	HIPCHK(hipSetDevice(device));
	size_t free_b = 0, total_b = 0;
	if (db_chunk == 0) HIPCHK(hipMemGetInfo(&free_b, &total_b));
	const uint32_t chunk = std::min(ntsm_eval_chunk::samples_per_pass(db_chunk, n_db, free_b, row_bytes + 12, 24ull * n_sites),
			65535u * kStrip);                                    /* the grid's second dimension holds 65,535 strips */

	ntsm_hip::Buffers b;
	ntsm_hip::Events<2> ev;
	uint32_t *d_raw, *d_geno = nullptr, *d_tally = nullptr;
	unsigned long long *d_cov = nullptr;
	HIPCHK(b.alloc(&d_raw, (uint64_t) chunk * n_sites * 2));
	if (db_geno) {
		HIPCHK(b.alloc(&d_geno, (uint64_t) n_db * 3));
		HIPCHK(hipMemset(d_geno, 0, (size_t) n_db * 3 * sizeof(uint32_t)));
	}
	if (site_tally) {
		HIPCHK(b.alloc(&d_tally, (uint64_t) n_sites * 4));
		HIPCHK(hipMemset(d_tally, 0, (size_t) n_sites * 4 * sizeof(uint32_t)));
	}
	if (site_cov) {
		HIPCHK(b.alloc(&d_cov, (uint64_t) n_sites));
		HIPCHK(hipMemset(d_cov, 0, (size_t) n_sites * sizeof(uint64_t)));
	}
	HIPCHK(ev.create());

	using ntsm_eval_chunk::ms_since;
	using ntsm_eval_chunk::wall;
	ntsm_eval_cross_times tm {};
	for (uint32_t c0 = 0; c0 < n_db; c0 += chunk) {
		const uint32_t cn = std::min(chunk, n_db - c0);
		int rc = ntsm_eval_chunk::upload(db_counts, db_stride_bytes, c0, cn, n_sites, d_raw, tm);
		if (rc) return rc;
		HIPCHK(hipEventRecord(ev[0], 0));
		hipLaunchKernelGGL(ntsm_eval_profile_kernel, dim3((n_sites + 63) / 64, (cn + kStrip - 1) / kStrip), dim3(kThreads), 0, 0, (const uint2 *) d_raw, cn,
				n_sites, min_cov, d_geno ? d_geno + (uint64_t) c0 * 3 : nullptr, d_tally, d_cov);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(ev[1], 0));
		HIPCHK(hipEventSynchronize(ev[1]));
		if ((rc = ntsm_eval_chunk::add_interval(ev[0], ev[1], &tm.cross_kernel_ms)) != 0) return rc;
		tm.chunks++;
	}
	const auto t = wall::now();
	if (db_geno) HIPCHK(hipMemcpy(db_geno, d_geno, (size_t) n_db * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (site_tally) HIPCHK(hipMemcpy(site_tally, d_tally, (size_t) n_sites * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
	if (site_cov) HIPCHK(hipMemcpy(site_cov, d_cov, (size_t) n_sites * sizeof(uint64_t), hipMemcpyDeviceToHost));
	tm.download_ms += ms_since(t);
	if (times) *times = tm;
	return 0;
}
