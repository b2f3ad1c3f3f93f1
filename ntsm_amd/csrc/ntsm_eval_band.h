/*
 * ntsm_eval_band.h -- the band session of ntsm_eval_within.hip, ntsm_eval_between.hip and ntsm_eval_contam.hip, stated once: a
 * store's samples held on the device as the columns of a rectangle (or triangle) of pairs, and the walk of one band of rows over
 * them.  What a feature adds is its kernel, its per-sample byte count, its stager and its launch.
 *
 * Two ways of holding the columns.  Resident: the chunk rule (ntsm_eval_chunk.h), asked at the feature's bytes per sample, answers
 * the whole store; it is staged once at open, the tallies are taken to the host, the dense copy and the tally buffer go back, and
 * a band's columns are an offset into the same arrays.  Streamed: every band walks the columns in chunks through one chunk's worth
 * of buffers.  The open's upload and preparation are reported by the session's first _rows call.  A session that never reaches
 * open() has done no device work and touches no device when it ends.
 *
 * A stager is a callable (first, count, const Staged<Tally> &to, bool tallies, ntsm_eval_cross_times &tm): samples first ...
 * first + count - 1 of a store into to.raw (dense) and from there to.at / to.cg / to.term [site][count] and, with `tallies`,
 * to.tally [count][3]; it waits for its kernels and adds its times to tm.
 *
 * Internal: not part of include/.  Everything has internal linkage, since the checks carry the including file's NTSM_HIP_TAG
 * (ntsm_hip_scope.h).  One stream, no overlap.
 */
#ifndef NTSM_EVAL_BAND_H
#define NTSM_EVAL_BAND_H

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ntsm_eval_chunk.h"

namespace ntsm_eval_band {
namespace {

using ntsm_eval_chunk::timed_copy;

/* a window of transposed samples on the device: element c is sample first + c of its store, count of them; term: NULL where the
 * feature has no such plane */
struct Window { const uint32_t *at, *cg; const double *term; uint32_t pitch, first, count; };

/* what staging fills: the dense copy [sample][raw_sites][2], its transpose [site][count] and the samples' tallies [count][3] */
template <typename Tally> struct Staged {
	uint32_t *at = nullptr, *cg = nullptr, *raw = nullptr;
	double *term = nullptr;
	Tally *tally = nullptr;

	hipError_t alloc(ntsm_hip::Buffers &b, uint64_t count, uint64_t n_sites, uint64_t raw_sites, bool with_term, bool with_tally)
	{
		hipError_t e = b.alloc(&at, count * n_sites);
		if (e == hipSuccess) e = b.alloc(&cg, count * n_sites);
		if (e == hipSuccess && with_term) e = b.alloc(&term, count * n_sites);
		if (e == hipSuccess && with_tally) e = b.alloc(&tally, count * 3);
		if (e == hipSuccess) e = b.alloc(&raw, count * raw_sites * 2);
		return e;
	}
	/* the whole of it, holding samples first ... first + count - 1 */
	Window window(uint32_t first, uint32_t count) const { return Window { at, cg, term, count, first, count }; }
};

/* the scoring features' stager over a store with the columns' own sites: ntsm_eval_chunk::stage and the wait for it */
inline int stage_scored(const void *db, uint64_t stride, uint32_t first, uint32_t count, uint32_t n_sites, uint32_t min_cov, const Staged<uint32_t> &to, bool tallies,
		hipEvent_t e0, hipEvent_t e1, ntsm_eval_cross_times &tm)
{
	const int rc = ntsm_eval_chunk::stage(db, stride, first, count, n_sites, min_cov, to.raw, to.at, to.cg, to.term, tallies ? to.tally : nullptr, e0, e1, tm);
	if (rc) return rc;
	HIPCHK(hipEventSynchronize(e1));
	return ntsm_eval_chunk::add_interval(e0, e1, &tm.prepare_kernel_ms);
}

/* A band's rows staged into buffers of their own in `scope` (pitch = count): the dense copy goes back before the records need
 * room; with `tally` the rows' tallies are taken and downloaded to it. */
template <typename Tally, typename Stager> int stage_rows(ntsm_hip::Buffers &scope, uint32_t first, uint32_t count, uint32_t n_sites, bool with_term, Tally *tally,
		Stager &&stage, ntsm_eval_cross_times &tm, Window &rows)
{
	Staged<Tally> r;
	HIPCHK(r.alloc(scope, count, n_sites, n_sites, with_term, tally != nullptr));
	const int rc = stage(first, count, r, tally != nullptr, tm);
	if (rc) return rc;
	HIPCHK(scope.release(&r.raw));
	rows = r.window(first, count);
	return tally ? timed_copy(tally, r.tally, (size_t) count * 3 * sizeof(Tally), hipMemcpyDeviceToHost, &tm.download_ms) : 0;
}

/* the columns of a session: n samples over n_sites sites */
template <typename Tally> struct Holding {
	int device = 0;
	uint32_t n = 0, n_sites = 0;
	uint32_t chunk = 0;                      /* columns per pass of a streamed store */
	bool resident = false, device_work = false;
	ntsm_hip::Buffers b;
	ntsm_hip::Events<2> ev;
	Staged<Tally> col;                       /* resident: the whole store [site][n]; streamed: one chunk [site][chunk] */
	std::vector<Tally> tally;                /* resident: [n][3], taken at open */
	ntsm_eval_cross_times open_times {};     /* resident: the upload and preparation of open, reported by the first _rows call */

	~Holding() { if (device_work) (void) hipSetDevice(device); }   /* a session without device work touches no device here either */

	/* The chunk decision at per_sample bytes, and the buffers.  raw_sites: the sites of the store's dense rows (between: B's own).
	 * chunk_tallies: a streamed walk takes each chunk's tallies (within, between); resident, open takes them in any case. */
	int open(int device_, uint32_t n_, uint32_t n_sites_, uint32_t raw_sites, uint32_t db_chunk, uint64_t per_sample, bool with_term, bool chunk_tallies)
	{
		device = device_; n = n_; n_sites = n_sites_;
		HIPCHK(hipSetDevice(device));
		device_work = true;
		size_t free_b = 0, total_b = 0;
		if (db_chunk == 0) HIPCHK(hipMemGetInfo(&free_b, &total_b));
		chunk = ntsm_eval_chunk::samples_per_pass(db_chunk, n, free_b, per_sample, 0);
		resident = chunk == n;
		HIPCHK(ev.create());
		HIPCHK(col.alloc(b, chunk, n_sites, raw_sites, with_term, resident || chunk_tallies));
		return 0;
	}

	/* resident: the whole store staged, its tallies taken, the dense copy and the tally buffer released; streamed: nothing */
	template <typename Stager> int fill(Stager &&stage)
	{
		if (!resident) return 0;
		int rc = stage(0, n, col, true, open_times);
		if (rc) return rc;
		tally.resize((size_t) n * 3);
		if ((rc = timed_copy(tally.data(), col.tally, tally.size() * sizeof(Tally), hipMemcpyDeviceToHost, &open_times.download_ms)) != 0) return rc;
		HIPCHK(b.release(&col.raw));                                                  /* the staging goes back before the records need room */
		HIPCHK(b.release(&col.tally));
		return 0;
	}

	/* what a _rows call starts from: the open's times, once */
	ntsm_eval_cross_times take_open_times()
	{
		const ntsm_eval_cross_times t = open_times;
		open_times = ntsm_eval_cross_times {};
		return t;
	}

	/* the columns from sample `first` on, resident */
	Window from(uint32_t first, uint32_t count) const { return Window { col.at + first, col.cg + first, col.term ? col.term + first : nullptr, n, first, count }; }

	/* Rows first ... first + count - 1 of the held store as a band's rows, and with row_tally their tallies [count][3]: resident,
	 * an offset into the columns' arrays and what open took; streamed, stage_rows into `scope`. */
	template <typename Stager> int band_rows(ntsm_hip::Buffers &scope, uint32_t first, uint32_t count, Tally *row_tally, Stager &&stage, ntsm_eval_cross_times &tm,
			Window &rows)
	{
		if (!resident) return stage_rows(scope, first, count, n_sites, col.term != nullptr, row_tally, stage, tm, rows);
		rows = from(first, count);
		if (row_tally) memcpy(row_tally, tally.data() + (size_t) first * 3, (size_t) count * 3 * sizeof(Tally));
		return 0;
	}

	/* The band walk over the columns col_first ... n - 1: the records are allocated; resident, one window and one
	 * launch(window, d_out); streamed, for each chunk: stage, launch(window, d_out), the chunk's tallies, chunks++; then the records
	 * are downloaded.  col_tally: NULL, or [n][3] by store sample, written from col_first on. */
	template <typename Record, typename Stager, typename Launch> int walk(uint32_t col_first, uint64_t records, Record *out, Tally *col_tally, Stager &&stage,
			Launch &&launch, ntsm_eval_cross_times &tm)
	{
		ntsm_hip::Buffers scope;
		Record *d_out;
		HIPCHK(scope.alloc(&d_out, records));
		int rc;
		if (resident) {
			if ((rc = launch(from(col_first, n - col_first), d_out)) != 0) return rc;
			if (col_tally) memcpy(col_tally + (size_t) col_first * 3, tally.data() + (size_t) col_first * 3, (size_t) (n - col_first) * 3 * sizeof(Tally));
		} else {
			for (uint32_t c0 = col_first; c0 < n; c0 += chunk) {
				const uint32_t cn = std::min(chunk, n - c0);
				if ((rc = stage(c0, cn, col, col_tally != nullptr, tm)) != 0) return rc;
				if ((rc = launch(col.window(c0, cn), d_out)) != 0) return rc;
				if (col_tally && (rc = timed_copy(col_tally + (size_t) c0 * 3, col.tally, (size_t) cn * 3 * sizeof(Tally), hipMemcpyDeviceToHost, &tm.download_ms)) != 0)
					return rc;
				tm.chunks++;
			}
		}
		return records ? timed_copy(out, d_out, records * sizeof(Record), hipMemcpyDeviceToHost, &tm.download_ms) : 0;
	}
};

}  // namespace
}  // namespace ntsm_eval_band

#endif
