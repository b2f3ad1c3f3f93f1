/*
 * ntsm_eval_between_near.hip -- the PCA-guided search between two cohort stores on one MI355X (include/ntsm_eval_hip.h:
 * ntsm_eval_project_store_mapped, ntsm_eval_between_score_pairs; ntsmEval --between-near).  Store A's
 * site table is the run's; store B lists its loci in whatever order its builder did and may lack some, so what this file adds
 * to ntsm_eval_near.hip is one thing: a sample of B projected and scored over A's sites.  Indices follow the concatenation
 * [A; B]: sample a of A is a, sample b of B is n_a + b.  The third entry point of the run, ntsm_eval_between_candidates,
 * stands beside the search kernels it launches (ntsm_eval_near.hip).
 *
 * Row remap.  Rows of B arrive dense as [row][n_sites_b][2] by 2-D copies from the store's stride.  The kernel writes them as
 * [row][n_sites_a][2]: lanes run along A's sites, each loads its map entry once, and then per row reads 8 bytes of B's site
 * site_map[s] (gathered; coalesced wherever the map is locally monotone) and writes 8 bytes at A's site s (coalesced), 0 / 0
 * where the map says UINT32_MAX.  A destination list sends staging row r to any row of the output, so the listed-pair
 * scorer remaps straight into its slots.  After it the rows are what a dense copy of B over A's sites holds, and everything
 * downstream is the code that runs on such a copy: ntsm_eval_pca.h's project_kernel, term_kernel and score_kernel and
 * ntsm_eval_chunk.h's tally_kernel -- no arithmetic is stated here.
 *
 * Projection.  ntsm_eval_project_store's walk (ntsm_eval_near.hip) with the remap between the copy and the two kernels; the
 * chunk rule is asked at the bytes both buffers of a sample need.  Without a map it is that function.
 *
 * Listed pairs.  A pair names one sample of each store.  The list is cut into passes by eval_within.hpp's pack_passes over
 * the samples of both stores together (the concatenation's numbering); a pass's samples of A are copied to their slots as
 * they lie, its samples of B go to a staging area in ascending store order and through the remap into their slots (without
 * a map, straight in).  Neighbouring samples that go to neighbouring rows are one 2-D copy -- the row of a search-all sample
 * names the whole other store in order.  Then the terms of the pass's rows and the listed-pair kernel over slot numbers.
 * One stream, no overlap.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/ntsm_eval_hip.h"
#include "host/eval_between.hpp"
#include "host/eval_within.hpp"
#define NTSM_HIP_TAG "ntsm_eval_between_near"
#include "ntsm_eval_chunk.h"
#include "ntsm_eval_pca.h"
#include "ntsm_hip_scope.h"
#include "xprec.h"

namespace {

constexpr int kThreads = 256;
constexpr uint32_t kLacks = ntsm::eval_between::kLacks;
constexpr uint32_t kMaxGridY = 65535;

using ntsm_eval_chunk::add_interval;
using ntsm_eval_chunk::valid_store;
using ntsm_eval_chunk::ms_since;
using ntsm_eval_chunk::wall;

/* src [row][n_sites_b] -> dst [dst_row ? dst_row[row] : row][n_sites_a] through the map; grid (sites of A / 256, rows up to
 * 65,535: a workgroup strides over the rows).  Every entry of site_map is below n_sites_b or kLacks (valid_map, on the host). */
__global__ __launch_bounds__(kThreads) void remap_rows_kernel(const uint2 *__restrict__ src, const uint32_t *__restrict__ site_map,
		const uint32_t *__restrict__ dst_row, uint32_t n_rows, uint32_t n_sites_a, uint32_t n_sites_b, uint2 *__restrict__ dst)
{
	const uint32_t site = blockIdx.x * kThreads + threadIdx.x;
	if (site >= n_sites_a) return;
	const uint32_t from = site_map[site];
	for (uint32_t r = blockIdx.y; r < n_rows; r += gridDim.y) {
		const uint32_t to = dst_row ? dst_row[r] : r;                               /* wave-uniform */
		dst[(uint64_t) to * n_sites_a + site] = from != kLacks ? src[(uint64_t) r * n_sites_b + from] : make_uint2(0u, 0u);
	}
}

/* the caller checks hipGetLastError */
void launch_remap(const uint32_t *src, const uint32_t *site_map, const uint32_t *dst_row, uint32_t n_rows, uint32_t n_sites_a, uint32_t n_sites_b, uint32_t *dst)
{
	hipLaunchKernelGGL(remap_rows_kernel, dim3((n_sites_a + kThreads - 1) / kThreads, std::min(n_rows, kMaxGridY)), dim3(kThreads), 0, 0, (const uint2 *) src,
			site_map, dst_row, n_rows, n_sites_a, n_sites_b, (uint2 *) dst);
}

/* what both entry points ask of their map (ntsm_eval_between_open's rule) */
bool map_fits(const uint32_t *site_map, uint32_t n_sites_a, uint32_t n_sites_b)
{
	return site_map ? ntsm::eval_between::valid_map(site_map, n_sites_a, n_sites_b) : n_sites_a == n_sites_b;
}

/* (store sample, destination row) in destination order: each run of neighbouring samples that go to neighbouring rows of
 * `row_bytes` is one 2-D copy from the store's stride */
typedef std::vector<std::pair<uint32_t, uint32_t>> Placement;

int copy_runs(const Placement &rows, const char *store, uint64_t stride, uint64_t row_bytes, char *d_dst)
{
	for (size_t x = 0; x < rows.size();) {
		size_t y = x + 1;
		while (y < rows.size() && rows[y].first == rows[y - 1].first + 1 && rows[y].second == rows[y - 1].second + 1) ++y;
		HIPCHK(hipMemcpy2D(d_dst + rows[x].second * row_bytes, row_bytes, store + (uint64_t) rows[x].first * stride, stride, row_bytes, y - x, hipMemcpyHostToDevice));
		x = y;
	}
	return 0;
}

}  // namespace

extern "C" int ntsm_eval_project_store_mapped(int device, const void *b_counts, uint64_t b_stride_bytes, uint32_t n_b, uint32_t n_sites_a, uint32_t n_sites_b,
		const uint32_t *site_map, uint32_t min_cov, const long double *norm, const long double *rot, uint32_t dim, uint32_t b_chunk, double *cloud,
		uint32_t *b_geno, ntsm_eval_cross_times *times)
{
	if (!site_map) {                                                             /* identical tables: the unmapped walk as it is */
		if (times) *times = ntsm_eval_cross_times {};
		if (n_sites_a != n_sites_b) return -1;
		return ntsm_eval_project_store(device, b_counts, b_stride_bytes, n_b, n_sites_a, min_cov, norm, rot, dim, b_chunk, cloud, b_geno, times);
	}
	if (times) *times = ntsm_eval_cross_times {};
	if (!valid_store(b_counts, b_stride_bytes, n_b, n_sites_b) || (n_sites_a && (!norm || (dim && !rot))) || (!cloud && n_b && dim)) return -1;
	if (!map_fits(site_map, n_sites_a, n_sites_b)) return -1;
	if (n_b && dim) memset(cloud, 0, (size_t) n_b * dim * sizeof(double));
	if (b_geno && n_b) memset(b_geno, 0, (size_t) n_b * 3 * sizeof(uint32_t));
	if (n_b == 0 || n_sites_a == 0) return 0;

	const std::vector<ntsm_x64> tab = ntsm_eval_pca::product_table(norm, rot, n_sites_a, dim);
	const uint64_t from_bytes = 8ull * n_sites_b, to_bytes = 8ull * n_sites_a;
	HIPCHK(hipSetDevice(device));
	size_t free_b = 0, total_b = 0;
	if (b_chunk == 0) HIPCHK(hipMemGetInfo(&free_b, &total_b));
	/* a sample holds its row as B lists it and its row over A's sites */
	const uint32_t chunk = ntsm_eval_chunk::samples_per_pass(b_chunk, n_b, free_b, from_bytes + to_bytes + 8ull * dim + 12,
			tab.size() * sizeof(ntsm_x64) + 4ull * n_sites_a);

	ntsm_hip::Buffers b;
	ntsm_hip::Events<3> ev;
	uint32_t *d_stage, *d_raw, *d_geno, *d_map;
	double *d_cloud;
	ntsm_x64 *d_tab;
	HIPCHK(b.alloc(&d_stage, (uint64_t) chunk * n_sites_b * 2));
	HIPCHK(b.alloc(&d_raw, (uint64_t) chunk * n_sites_a * 2));
	HIPCHK(b.alloc(&d_geno, (uint64_t) chunk * 3));
	HIPCHK(b.alloc(&d_cloud, (uint64_t) chunk * dim));
	HIPCHK(b.alloc(&d_tab, tab.size()));
	HIPCHK(b.alloc(&d_map, n_sites_a));
	HIPCHK(ev.create());
	ntsm_eval_cross_times tm {};
	auto t = wall::now();
	HIPCHK(hipMemcpy(d_tab, tab.data(), tab.size() * sizeof(ntsm_x64), hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(d_map, site_map, (size_t) n_sites_a * sizeof(uint32_t), hipMemcpyHostToDevice));
	tm.upload_ms += ms_since(t);

	for (uint32_t c0 = 0; c0 < n_b; c0 += chunk) {
		const uint32_t cn = std::min(chunk, n_b - c0);
		t = wall::now();
		if (from_bytes)
			HIPCHK(hipMemcpy2D(d_stage, from_bytes, (const char *) b_counts + (uint64_t) c0 * b_stride_bytes, b_stride_bytes, from_bytes, cn, hipMemcpyHostToDevice));
		tm.upload_ms += ms_since(t);
		HIPCHK(hipEventRecord(ev[0], 0));
		launch_remap(d_stage, d_map, nullptr, cn, n_sites_a, n_sites_b, d_raw);
		HIPCHK(hipGetLastError());
		if (b_geno) {
			ntsm_eval_chunk::launch_tally(d_raw, cn, n_sites_a, min_cov, d_geno);
			HIPCHK(hipGetLastError());
		}
		HIPCHK(hipEventRecord(ev[1], 0));
		if (dim) {
			ntsm_eval_pca::launch_project(d_raw, cn, n_sites_a, min_cov, d_tab, dim, d_cloud);
			HIPCHK(hipGetLastError());
		}
		HIPCHK(hipEventRecord(ev[2], 0));
		HIPCHK(hipEventSynchronize(ev[2]));
		t = wall::now();
		if (dim) HIPCHK(hipMemcpy(cloud + (uint64_t) c0 * dim, d_cloud, (size_t) cn * dim * sizeof(double), hipMemcpyDeviceToHost));
		if (b_geno) HIPCHK(hipMemcpy(b_geno + (uint64_t) c0 * 3, d_geno, (size_t) cn * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
		tm.download_ms += ms_since(t);
		int rc = add_interval(ev[0], ev[1], &tm.prepare_kernel_ms);
		if (!rc) rc = add_interval(ev[1], ev[2], &tm.cross_kernel_ms);
		if (rc) return rc;
		tm.chunks++;
	}
	if (times) *times = tm;
	return 0;
}

extern "C" int ntsm_eval_between_score_pairs(int device, const void *a_counts, uint64_t a_stride_bytes, uint32_t n_a, const void *b_counts,
		uint64_t b_stride_bytes, uint32_t n_b, uint32_t n_sites_a, uint32_t n_sites_b, const uint32_t *site_map, uint32_t min_cov, const uint32_t *pi,
		const uint32_t *pk, uint64_t n_pairs, uint32_t chunk_arg, ntsm_eval_record *out, ntsm_eval_cross_times *times)
{
	if (times) *times = ntsm_eval_cross_times {};
	if (!valid_store(a_counts, a_stride_bytes, n_a, n_sites_a) || !valid_store(b_counts, b_stride_bytes, n_b, n_sites_b)) return -1;
	if ((n_pairs && (!pi || !pk || !out)) || chunk_arg == 1 || !map_fits(site_map, n_sites_a, n_sites_b)) return -1;
	const uint64_t n64 = (uint64_t) n_a + n_b;
	if (n64 > UINT32_MAX) return -1;
	const uint32_t n = (uint32_t) n64;
	for (uint64_t p = 0; p < n_pairs; ++p)
		if (pi[p] >= n || pk[p] >= n || (pi[p] < n_a) == (pk[p] < n_a)) return -1;  /* one sample of each store */
	if (n_pairs == 0) return 0;
	memset(out, 0, n_pairs * sizeof(ntsm_eval_record));
	if (n_sites_a == 0) return 0;

	const uint64_t a_bytes = 8ull * n_sites_a, b_bytes = 8ull * n_sites_b;
	HIPCHK(hipSetDevice(device));
	size_t free_b = 0, total_b = 0;
	if (chunk_arg == 0) HIPCHK(hipMemGetInfo(&free_b, &total_b));
	/* a slot is a row and its terms over A's sites; under a map every slot may be a sample of B with a staging row and its slot number */
	const uint32_t chunk = std::max(2u, ntsm_eval_chunk::samples_per_pass(chunk_arg, n, free_b, 2 * a_bytes + (site_map ? b_bytes + 4 : 0),
			n_pairs * (sizeof(ntsm_eval_record) + 8) + (site_map ? 4ull * n_sites_a : 0)));
	const ntsm::eval_within::Passes cut = ntsm::eval_within::pack_passes(pi, pk, n_pairs, n, chunk);
	uint64_t most = 0;
	uint32_t slots = 0;
	for (size_t x = 0; x < cut.passes(); ++x) {
		most = std::max(most, cut.pair_begin[x + 1] - cut.pair_begin[x]);
		slots = std::max(slots, (uint32_t) (cut.sample_begin[x + 1] - cut.sample_begin[x]));
	}

	ntsm_hip::Buffers b;
	ntsm_hip::Events<3> ev;
	uint32_t *d_rows, *d_pi, *d_pk, *d_stage = nullptr, *d_slot = nullptr, *d_map = nullptr;
	double *d_term;
	ntsm_eval_record *d_out;
	HIPCHK(b.alloc(&d_rows, (uint64_t) slots * n_sites_a * 2));
	HIPCHK(b.alloc(&d_term, (uint64_t) slots * n_sites_a));
	HIPCHK(b.alloc(&d_pi, most));
	HIPCHK(b.alloc(&d_pk, most));
	HIPCHK(b.alloc(&d_out, most));
	HIPCHK(ev.create());
	ntsm_eval_cross_times tm {};
	if (site_map) {
		HIPCHK(b.alloc(&d_stage, (uint64_t) slots * n_sites_b * 2));
		HIPCHK(b.alloc(&d_slot, slots));
		HIPCHK(b.alloc(&d_map, n_sites_a));
		const auto t = wall::now();
		HIPCHK(hipMemcpy(d_map, site_map, (size_t) n_sites_a * sizeof(uint32_t), hipMemcpyHostToDevice));
		tm.upload_ms += ms_since(t);
	}

	Placement of_a, of_b;
	std::vector<uint32_t> slot_of_stage;
	for (size_t x = 0; x < cut.passes(); ++x) {
		const uint64_t p0 = cut.pair_begin[x], pn = cut.pair_begin[x + 1] - p0, s0 = cut.sample_begin[x];
		const uint32_t rn = (uint32_t) (cut.sample_begin[x + 1] - s0);
		of_a.clear();
		of_b.clear();
		for (uint32_t slot = 0; slot < rn; ++slot) {
			const uint32_t s = cut.sample[s0 + slot];
			if (s < n_a) of_a.emplace_back(s, slot); else of_b.emplace_back(s - n_a, slot);
		}
		if (site_map) {                                                          /* staged in store order: row r of the staging area goes to slot_of_stage[r] */
			std::sort(of_b.begin(), of_b.end());
			slot_of_stage.resize(of_b.size());
			for (size_t r = 0; r < of_b.size(); ++r) { slot_of_stage[r] = of_b[r].second; of_b[r].second = (uint32_t) r; }
		}
		auto t = wall::now();
		int rc = copy_runs(of_a, (const char *) a_counts, a_stride_bytes, a_bytes, (char *) d_rows);
		if (rc) return rc;
		if (!site_map) rc = copy_runs(of_b, (const char *) b_counts, b_stride_bytes, a_bytes, (char *) d_rows);
		else if (b_bytes) rc = copy_runs(of_b, (const char *) b_counts, b_stride_bytes, b_bytes, (char *) d_stage);
		if (rc) return rc;
		if (site_map && !of_b.empty()) HIPCHK(hipMemcpy(d_slot, slot_of_stage.data(), of_b.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(d_pi, cut.slot_i.data() + p0, pn * sizeof(uint32_t), hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(d_pk, cut.slot_k.data() + p0, pn * sizeof(uint32_t), hipMemcpyHostToDevice));
		tm.upload_ms += ms_since(t);
		HIPCHK(hipEventRecord(ev[0], 0));
		if (site_map && !of_b.empty()) {
			launch_remap(d_stage, d_map, d_slot, (uint32_t) of_b.size(), n_sites_a, n_sites_b, d_rows);
			HIPCHK(hipGetLastError());
		}
		ntsm_eval_pca::launch_term(d_rows, (uint64_t) rn * n_sites_a, min_cov, d_term);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(ev[1], 0));
		ntsm_eval_pca::launch_score(d_rows, d_term, n_sites_a, min_cov, d_pi, d_pk, pn, d_out);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(ev[2], 0));
		HIPCHK(hipEventSynchronize(ev[2]));
		rc = add_interval(ev[0], ev[1], &tm.prepare_kernel_ms);
		if (!rc) rc = add_interval(ev[1], ev[2], &tm.cross_kernel_ms);
		if (rc) return rc;
		t = wall::now();
		HIPCHK(hipMemcpy(out + p0, d_out, pn * sizeof(ntsm_eval_record), hipMemcpyDeviceToHost));
		tm.download_ms += ms_since(t);
		tm.chunks++;
	}
	if (times) *times = tm;
	return 0;
}
