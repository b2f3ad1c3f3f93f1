/*
 * ntsm_eval_cross.hip -- queries against a cohort on one MI355X (include/ntsm_eval_hip.h: ntsm_eval_cross): the n_q x n_db
 * rectangle of pairs (query q, database sample d), each record bit for bit what ntsm_eval_pairs gives for pair (q, n_q + d)
 * of the concatenation [queries; database].
 *
 * Layout.  As in ntsm_eval.hip one thread owns one pair and walks the sites in order with one ntsm_eval_acc
 * (ntsm_eval_score.h), so the sums are the reference's sequential sums.  The database samples go across the lanes: the
 * counts of a chunk of them are transposed to at / cg / term [site][chunk sample], one coalesced 4 + 4 + 8-byte load per lane
 * and site.  A workgroup holds a group of TQ queries on the wave-uniform side (their arrays are [site][query]: scalar loads,
 * one ntsm_eval_side per query and site reused by every lane).  A rectangle has no diagonal: no tile is skipped and no
 * record is mirrored; the query is sample 1 of every record.
 *
 * Chunks.  The database is a host array with a fixed pitch between samples (a cohort store mapped from disk).  Per chunk:
 * the staging step of ntsm_eval_chunk.h -- one 2-D copy of the chunk's counts to a dense [chunk sample][site][2] buffer, the
 * transpose (through LDS, so that both its reads and its writes are coalesced) and the genotype tallies of the chunk's
 * samples (one workgroup per sample over the dense buffer), both reported as "prepare" --, the cross kernel, one wait, and
 * one 2-D copy of the chunk's columns of `out` back.  The chunk rule is that header's too.  One stream, no overlap.  Device
 * memory is O((n_q + chunk) * n_sites + n_q * chunk).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../include/ntsm_eval_hip.h"
#define NTSM_HIP_TAG "ntsm_eval_cross"
#include "ntsm_eval_chunk.h"
#include "ntsm_eval_score.h"
#include "ntsm_hip_scope.h"

namespace {

using ntsm_eval_chunk::kThreads;

uint32_t g_width = 0, g_query_group = 0;     /* ntsm_eval_cross_tune */

/* grid (chunk samples / blockDim.x, groups of TQ queries from query q_first on); out [n_q][out_pitch], the chunk's sample d at column d */
template <int TQ> __global__ __launch_bounds__(kThreads) void ntsm_eval_cross_kernel(const uint32_t *__restrict__ qat, const uint32_t *__restrict__ qcg,
		const double *__restrict__ qterm, uint32_t n_q, uint32_t q_first, const uint32_t *__restrict__ at, const uint32_t *__restrict__ cg,
		const double *__restrict__ term, uint32_t n_d, uint32_t n_sites, uint32_t min_cov, ntsm_eval_record *__restrict__ out, uint32_t out_pitch)
{
	const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
	const uint32_t q0 = q_first + blockIdx.y * TQ;
	const uint32_t dc = d < n_d ? d : n_d - 1;                                   /* lanes past the end compute a copy of the last sample, not stored */
	uint32_t q[TQ];
#pragma unroll
	for (int k = 0; k < TQ; ++k) q[k] = q0 + k < n_q ? q0 + k : n_q - 1;         /* wave-uniform: scalar loads */
	ntsm_eval_acc acc[TQ];
	for (uint32_t site = 0; site < n_sites; ++site) {
		const uint64_t rd = (uint64_t) site * n_d + dc, rq = (uint64_t) site * n_q;
		const ntsm_eval_side sd = ntsm_eval_side_of(at[rd], cg[rd], term[rd], min_cov);
#pragma unroll
		for (int k = 0; k < TQ; ++k) acc[k].add(ntsm_eval_side_of(qat[rq + q[k]], qcg[rq + q[k]], qterm[rq + q[k]], min_cov), sd, min_cov);
	}
	if (d >= n_d) return;
#pragma unroll
	for (int k = 0; k < TQ; ++k)
		if (q0 + k < n_q) out[(uint64_t) (q0 + k) * out_pitch + d] = acc[k].record();
}

}  // namespace

extern "C" int ntsm_eval_cross_tune(uint32_t width, uint32_t query_group)
{
	if ((width != 0 && width != 64 && width != 256) || (query_group != 0 && query_group != 1 && query_group != 2 && query_group != 4)) return -1;
	g_width = width;
	g_query_group = query_group;
	return 0;
}

extern "C" int ntsm_eval_cross(int device, const uint32_t *q_counts, uint32_t n_q, const void *db_counts, uint64_t db_stride_bytes,
		uint32_t n_db, uint32_t n_sites, uint32_t min_cov, uint32_t db_chunk,
		ntsm_eval_record *out, uint32_t *db_geno, ntsm_eval_cross_times *times)
{
	if (times) *times = ntsm_eval_cross_times {};
	if ((!q_counts && n_q && n_sites) || !ntsm_eval_chunk::valid_store(db_counts, db_stride_bytes, n_db, n_sites) || (!out && n_q && n_db)) return -1;
	if (n_q && n_db) memset(out, 0, (size_t) n_q * n_db * sizeof(ntsm_eval_record));
	if (db_geno && n_db) memset(db_geno, 0, (size_t) n_db * 3 * sizeof(uint32_t));
	if (n_q == 0 || n_db == 0 || n_sites == 0) return 0;

	const uint64_t row_bytes = 8ull * n_sites;
	HIPCHK(hipSetDevice(device));
	size_t free_b = 0, total_b = 0;
	if (db_chunk == 0) HIPCHK(hipMemGetInfo(&free_b, &total_b));
	const uint32_t chunk = ntsm_eval_chunk::samples_per_pass(db_chunk, n_db, free_b,
			3 * row_bytes + (uint64_t) n_q * sizeof(ntsm_eval_record) + 12, 3ull * n_q * row_bytes);

	ntsm_hip::Buffers b;
	ntsm_hip::Events<3> ev;
	uint32_t *d_q, *d_qat, *d_qcg, *d_raw, *d_at, *d_cg, *d_geno;
	double *d_qterm, *d_term;
	ntsm_eval_record *d_out;
	const uint64_t qcells = (uint64_t) n_q * n_sites, cells = (uint64_t) chunk * n_sites;
	HIPCHK(b.alloc(&d_q, qcells * 2));
	HIPCHK(b.alloc(&d_qat, qcells));
	HIPCHK(b.alloc(&d_qcg, qcells));
	HIPCHK(b.alloc(&d_qterm, qcells));
	HIPCHK(b.alloc(&d_raw, cells * 2));
	HIPCHK(b.alloc(&d_at, cells));
	HIPCHK(b.alloc(&d_cg, cells));
	HIPCHK(b.alloc(&d_term, cells));
	HIPCHK(b.alloc(&d_geno, (uint64_t) chunk * 3));
	HIPCHK(b.alloc(&d_out, (uint64_t) n_q * chunk));
	HIPCHK(ev.create());

	using ntsm_eval_chunk::ms_since;
	using ntsm_eval_chunk::wall;
	ntsm_eval_cross_times tm {};
	int rc = ntsm_eval_chunk::timed_copy(d_q, q_counts, qcells * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, &tm.upload_ms);
	if (rc) return rc;
	rc = ntsm_eval_chunk::timed(ev[0], ev[1], &tm.prepare_kernel_ms, [&] {
		ntsm_eval_chunk::launch_prepare(d_q, n_q, n_sites, min_cov, d_qat, d_qcg, d_qterm);
		HIPCHK(hipGetLastError());
		return 0;
	});
	if (rc) return rc;

	for (uint32_t c0 = 0; c0 < n_db; c0 += chunk) {
		const uint32_t cn = std::min(chunk, n_db - c0);
		rc = ntsm_eval_chunk::stage(db_counts, db_stride_bytes, c0, cn, n_sites, min_cov, d_raw, d_at, d_cg, d_term, db_geno ? d_geno : nullptr, ev[0], ev[1], tm);
		if (rc) return rc;
		/* ntsm_eval_chunk.h's launch rule, measured on this kernel: unlike ntsm_eval.hip no width switch;
		 * 256 threads are reachable through ntsm_eval_cross_tune only */
		uint32_t width, tq;
		ntsm_eval_chunk::launch_shape(n_q, cn, g_width, g_query_group, width, tq);
		auto kernel = tq == 4 ? ntsm_eval_cross_kernel<4> : tq == 2 ? ntsm_eval_cross_kernel<2> : ntsm_eval_cross_kernel<1>;
		ntsm_eval_chunk::for_grid_y_slices(((uint64_t) n_q + tq - 1) / tq, [&](uint64_t group, uint32_t groups) {   /* one launch up to 65,535 query groups */
			hipLaunchKernelGGL(kernel, dim3((cn + width - 1) / width, groups), dim3(width), 0, 0, d_qat, d_qcg, d_qterm, n_q, (uint32_t) (group * tq), d_at, d_cg, d_term,
					cn, n_sites, min_cov, d_out, chunk);
		});
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(ev[2], 0));
		HIPCHK(hipEventSynchronize(ev[2]));
		const auto t = wall::now();
		HIPCHK(hipMemcpy2D(out + c0, (size_t) n_db * sizeof(ntsm_eval_record), d_out, (size_t) chunk * sizeof(ntsm_eval_record),
				(size_t) cn * sizeof(ntsm_eval_record), n_q, hipMemcpyDeviceToHost));
		if (db_geno) HIPCHK(hipMemcpy(db_geno + (uint64_t) c0 * 3, d_geno, (size_t) cn * 3 * sizeof(uint32_t), hipMemcpyDeviceToHost));
		tm.download_ms += ms_since(t);
		if ((rc = ntsm_eval_chunk::add_interval(ev[0], ev[1], &tm.prepare_kernel_ms)) != 0) return rc;
		if ((rc = ntsm_eval_chunk::add_interval(ev[1], ev[2], &tm.cross_kernel_ms)) != 0) return rc;
		tm.chunks++;
	}
	if (times) *times = tm;
	return 0;
}
