/*
 * eval_within.hpp -- the host arithmetic of the pairs inside a cohort store (ntsmEval --within / --within-near, DESIGN.md
 * section 9.3), stated once for the device library (ntsm_eval_within.hip, ntsm_eval_near.hip) and the CLI: where the records
 * of a band of rows lie, how many rows a band takes, and how a list of pairs of store samples is cut into passes that fit
 * the device.  Header only, host only, no HIP; tools/eval_within_check.cpp holds it against brute force under the host
 * sanitizers (`make within_check`).
 */
#ifndef NTSM_EVAL_WITHIN_HPP
#define NTSM_EVAL_WITHIN_HPP

#include <cstdint>
#include <vector>

namespace ntsm {
namespace eval_within {

/* The triangle of n samples in ntsm_eval_pair_index order: row i holds the pairs (i, j), i < j < n.  band_base(r, n) is the
 * number of pairs in the rows before r, i.e. ntsm_eval_pair_index(r, r + 1, n); r = n gives all n * (n - 1) / 2. */
inline uint64_t band_base(uint32_t r, uint32_t n) { return (uint64_t) r * n - (uint64_t) r * ((uint64_t) r + 1) / 2; }

/* the records of rows row_first ... row_first + n_rows - 1 (row_first + n_rows <= n) */
inline uint64_t band_records(uint32_t row_first, uint32_t n_rows, uint32_t n) { return band_base(row_first + n_rows, n) - band_base(row_first, n); }

/* where pair (i, j) lies in the output of a band that starts at row_first <= i */
inline uint64_t band_offset(uint32_t i, uint32_t j, uint32_t row_first, uint32_t n) { return band_base(i, n) + (j - i - 1) - band_base(row_first, n); }

/* The band rule: the most rows from row_first on whose records fit in `limit` records, and at least one (a row of more than
 * `limit` pairs is a band of its own).  A bound on host memory, not a tuned number. */
inline uint32_t band_rows(uint32_t row_first, uint32_t n, uint64_t limit)
{
	uint32_t lo = 1, hi = n - row_first;                                        /* the answer lies in [lo, hi]; records grow with the rows */
	if (band_records(row_first, hi, n) <= limit) return hi;
	while (lo + 1 < hi) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (band_records(row_first, mid, n) <= limit) lo = mid; else hi = mid;
	}
	return lo;
}

constexpr uint64_t kBandRecords = (1ull << 30) / 64;                            /* 1 GiB of 64-byte records */

/* Passes over a list of pairs of store samples.  A pair needs both of its samples on the device at once, so the list is cut
 * greedily in list order: a pair joins the current pass while the pass's distinct samples stay <= chunk (>= 2), otherwise
 * the pass closes and the pair opens the next one.  A pass is therefore a contiguous piece of the list, and a sample may be
 * copied in more than one pass. */
struct Passes {
	std::vector<uint64_t> pair_begin;        /* pass p scores pairs pair_begin[p] ... pair_begin[p + 1] - 1 */
	std::vector<uint64_t> sample_begin;      /* ... over the samples sample[sample_begin[p] ... sample_begin[p + 1] - 1], */
	std::vector<uint32_t> sample;            /*     distinct inside a pass, in order of first appearance: slot s holds the s-th */
	std::vector<uint32_t> slot_i, slot_k;    /* per pair: the slots of pi[p] and pk[p] inside its pass */
	size_t passes() const { return pair_begin.size() - 1; }
};

inline Passes pack_passes(const uint32_t *pi, const uint32_t *pk, uint64_t n_pairs, uint32_t n_db, uint32_t chunk)
{
	Passes out;
	out.pair_begin.push_back(0);
	out.sample_begin.push_back(0);
	out.slot_i.resize(n_pairs);
	out.slot_k.resize(n_pairs);
	std::vector<uint32_t> slot_of(n_db, UINT32_MAX);
	uint64_t first = 0;                                                          /* the open pass's first sample in out.sample */
	for (uint64_t p = 0; p < n_pairs; ++p) {
		const uint32_t held = (uint32_t) (out.sample.size() - first);
		const uint32_t fresh = (slot_of[pi[p]] == UINT32_MAX) + (slot_of[pk[p]] == UINT32_MAX);
		if (held + fresh > chunk) {                                             /* close the pass: forget its slots */
			for (uint64_t s = first; s < out.sample.size(); ++s) slot_of[out.sample[s]] = UINT32_MAX;
			first = out.sample.size();
			out.pair_begin.push_back(p);
			out.sample_begin.push_back(first);
		}
		for (const uint32_t s : { pi[p], pk[p] })
			if (slot_of[s] == UINT32_MAX) { slot_of[s] = (uint32_t) (out.sample.size() - first); out.sample.push_back(s); }
		out.slot_i[p] = slot_of[pi[p]];
		out.slot_k[p] = slot_of[pk[p]];
	}
	if (n_pairs) {
		out.pair_begin.push_back(n_pairs);
		out.sample_begin.push_back(out.sample.size());
	}
	return out;
}

}  // namespace eval_within
}  // namespace ntsm

#endif
