/*
 * eval_between.hpp -- the host arithmetic of one cohort store scored against another (ntsmEval --between, DESIGN.md section
 * 9.4), stated once for the device library (ntsm_eval_between.hip) and the CLI: how the loci of store B map onto the site
 * table of store A, what a map handed to the library must satisfy, and how many rows of A a band takes; for the PCA-guided
 * search between two stores (--between-near, section 9.5) also which rows of A are scored dense and whether B's index serves.
 * Header only, host only, no HIP; tools/eval_between_check.cpp and tools/eval_between_near_check.cpp hold it against its cases
 * under the host sanitizers (`make between_check`, `make between_near_check`).
 */
#ifndef NTSM_EVAL_BETWEEN_HPP
#define NTSM_EVAL_BETWEEN_HPP

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <unordered_map>
#include <utility>
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

/* The dense rows of --between-near: a sample of A whose squared radius is not below `all` (DBL_MAX,
 * "search all") owns its whole row of B.  The runs of consecutive such samples, (first, count) ascending: each goes through
 * ntsm_eval_between_rows as one range, cut by band_rows where it passes the band rule. */
inline std::vector<std::pair<uint32_t, uint32_t>> dense_runs(const double *radius, uint32_t n_a, double all)
{
	std::vector<std::pair<uint32_t, uint32_t>> runs;
	for (uint32_t a = 0; a < n_a; ++a) {
		if (radius[a] < all) continue;
		if (!runs.empty() && runs.back().first + runs.back().second == a) ++runs.back().second;
		else runs.emplace_back(a, 1u);
	}
	return runs;
}

/* Where the projections and tallies of B's samples come from in --between-near.  B.pcaidx holds them over B's own site table
 * and with the matrices of the run that wrote it; they are those of this run exactly when that table is A's and those
 * matrices are A's index's.  What the caller found out about B's index, and the two indexes' parameters: */
struct BIndexFacts {
	bool exists = false;                     /* there is a file B.pcaidx */
	bool valid = false;                      /* it opens as an index (eval_index.hpp: magic, version, offsets, size) */
	bool current = false;                    /* it was written for B's loci and holds every sample of B */
	bool identical_loci = false;             /* LocusMap::identical: B's locus table is A's */
	uint32_t dim_a = 0, min_cov_a = 0, dim_b = 0, min_cov_b = 0;
	const char *matrices_a = nullptr, *matrices_b = nullptr;   /* norm and rot as the files hold them */
	size_t matrix_size_a = 0, matrix_size_b = 0;
};

/* Does B.pcaidx serve?  Where it does not, B is projected and tallied in the run, through the map, and nothing is written.
 * Every condition alone says no. */
inline bool b_index_usable(const BIndexFacts &f)
{
	return f.exists && f.valid && f.current && f.identical_loci && f.dim_b == f.dim_a && f.min_cov_b == f.min_cov_a && f.matrices_a && f.matrices_b
	       && f.matrix_size_b == f.matrix_size_a && memcmp(f.matrices_a, f.matrices_b, f.matrix_size_a) == 0;
}

}  // namespace eval_between
}  // namespace ntsm

#endif
