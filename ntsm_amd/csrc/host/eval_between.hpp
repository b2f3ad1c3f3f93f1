/*
 * eval_between.hpp -- the host arithmetic of one cohort store scored against another (ntsmEval --between, DESIGN.md section
 * 9.4), stated once for the device library (ntsm_eval_between.hip) and the CLI: how the loci of store B map onto the site
 * table of store A, what a map handed to the library must satisfy, and how many rows of A a band takes.  Header only, host
 * only, no HIP; tools/eval_between_check.cpp holds it against its cases under the host sanitizers (`make between_check`).
 */
#ifndef NTSM_EVAL_BETWEEN_HPP
#define NTSM_EVAL_BETWEEN_HPP

#include <algorithm>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "eval_store.hpp"

namespace ntsm {
namespace eval_between {

constexpr uint32_t kLacks = UINT32_MAX;      /* a map entry: B has no such locus */

/* A's sites seen from B.  A's locus table plays the first file's part and B's samples are later files of that run
 * (src/CompareCounts.hpp:71-114): a locus of A that B lacks counts 0 / 0, a locus of B that A lacks is refused. */
struct LocusMap {
	bool identical = false;                  /* the two tables list the same IDs in the same order: site_map is empty, pass NULL */
	std::vector<uint32_t> site_map;          /* [A's sites]: the index of the locus among B's sites, or kLacks */
	uint32_t lacking = 0;                    /* the loci of A that B lacks */
	const uint32_t *data() const { return identical ? nullptr : site_map.data(); }
};

/* Throws eval_store::Error naming the ID: a locus either table holds twice (a map needs one site per ID on both sides), or
 * a locus of B that A lacks.  `a_name` and `b_name` are the stores' names in those sentences. */
inline LocusMap map_loci(const std::vector<std::string> &a, const std::vector<std::string> &b, const std::string &a_name, const std::string &b_name)
{
	std::unordered_map<std::string, uint32_t> site_of;
	site_of.reserve(a.size());
	for (size_t s = 0; s < a.size(); ++s)
		if (!site_of.emplace(a[s], (uint32_t) s).second) throw eval_store::Error("locus " + a[s] + " stands twice in " + a_name);
	LocusMap m;
	if (a == b) { m.identical = true; return m; }
	m.site_map.assign(a.size(), kLacks);
	for (size_t s = 0; s < b.size(); ++s) {
		const auto at = site_of.find(b[s]);
		if (at == site_of.end()) throw eval_store::Error("locus " + b[s] + " of " + b_name + " is not in " + a_name);
		if (m.site_map[at->second] != kLacks) throw eval_store::Error("locus " + b[s] + " stands twice in " + b_name);
		m.site_map[at->second] = (uint32_t) s;
	}
	m.lacking = (uint32_t) (a.size() - b.size());
	return m;
}

inline LocusMap map_loci(const eval_store::View &a, const eval_store::View &b, const std::string &a_name, const std::string &b_name)
{
	return map_loci(a.locus, b.locus, a_name, b_name);
}

/* what the library asks of a map it is handed: every entry a site of B or kLacks, and no site of B named twice */
inline bool valid_map(const uint32_t *site_map, uint32_t n_sites_a, uint32_t n_sites_b)
{
	std::vector<bool> named(n_sites_b, false);
	for (uint32_t s = 0; s < n_sites_a; ++s) {
		const uint32_t b = site_map[s];
		if (b == kLacks) continue;
		if (b >= n_sites_b || named[b]) return false;
		named[b] = true;
	}
	return true;
}

/* The band rule of --within stated for a rectangle: the most rows of A from row_first on whose n_rows * n_b records fit in
 * `limit` records, and at least one.  A bound on host memory, not a tuned number.  n_b >= 1, row_first < n_a. */
inline uint32_t band_rows(uint32_t row_first, uint32_t n_a, uint32_t n_b, uint64_t limit)
{
	const uint64_t fit = limit / n_b;
	return (uint32_t) std::min<uint64_t>(n_a - row_first, fit ? fit : 1);
}

constexpr uint64_t kBandRecords = (1ull << 30) / 64;                            /* 1 GiB of 64-byte records */

}  // namespace eval_between
}  // namespace ntsm

#endif
