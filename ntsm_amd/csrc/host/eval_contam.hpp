/*
 * eval_contam.hpp -- the host side of ntsmEval --contam: how many targets a band takes, and the text
 * of the pair table on stdout and of the per-sample table of --samples-out.  Header only, host only, no HIP: the integers are
 * the device's (include/ntsm_eval_hip.h: ntsm_eval_contam_rows), the doubles are formed here from them, each in one stated
 * expression and printed with std::to_string, so that a model can reproduce the bytes.  tools/eval_contam_check.cpp holds it
 * against its cases under the host sanitizers (`make contam_check`).
 *
 *   sample source sitesLack sitesHet sitesOpp rateLack rateHet rateOpp excess explained      (tabs between the fields)
 *   rateK     = double(minor[k]) / double(depth[k]), NA where depth[k] == 0      (k = lack, het, opp)
 *   rateAll   = double(tally minor) / double(tally depth) of the target, NA where that depth is 0
 *   excess    = rateOpp - rateLack
 *   explained = 1 - rateLack / rateAll
 * excess and explained read NA where an operand is NA or rateAll == 0.  A row is printed under `all`; otherwise when excess and
 * explained are numbers, excess >= min_excess and explained >= min_explained.
 *
 *   #sample sites minorReads depth rateAll
 */
#ifndef NTSM_EVAL_CONTAM_HPP
#define NTSM_EVAL_CONTAM_HPP

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../../include/ntsm_eval_hip.h"

namespace ntsm {
namespace eval_contam {

constexpr const char *kHeader = "sample\tsource\tsitesLack\tsitesHet\tsitesOpp\trateLack\trateHet\trateOpp\texcess\texplained\n";
constexpr const char *kSampleHeader = "#sample\tsites\tminorReads\tdepth\trateAll\n";
constexpr uint64_t kBandRecords = (1ull << 30) / sizeof(ntsm_eval_contam_record);   /* 1 GiB of records, as --within's bands */
/* the defaults of --contam-min and --contam-explained: conventions a user overrides, chosen from one simulation (a 10 % and
 * a 2 % mixture among 8 samples x 2,000 sites at 30x), not from real data */
constexpr double kMinExcess = 0.01, kMinExplained = 0.5;
constexpr uint32_t kMinDepth = 8;            /* the default of --contam-depth */

/* The band rule: the most targets from row_first on whose n_rows * n_db records fit in `limit` records, and at least one.  A
 * bound on host memory, not a tuned number.  n_db >= 1, row_first < n_db. */
inline uint32_t band_rows(uint32_t row_first, uint32_t n_db, uint64_t limit)
{
	const uint64_t fit = limit / n_db;
	return (uint32_t) std::min<uint64_t>(n_db - row_first, fit ? fit : 1);
}

/* The line of the pair (sample, source), appended to out if it is printed; returns whether it was.  tally = sites, minor reads,
 * depth of the target. */
inline bool row_line(std::string &out, const char *sample, const char *source, const ntsm_eval_contam_record &r, const uint64_t tally[3], bool all,
		double min_excess, double min_explained)
{
	bool has[3];
	double rate[3];
	for (int k = 0; k < 3; ++k) {
		has[k] = r.depth[k] != 0;
		rate[k] = has[k] ? double(r.minor[k]) / double(r.depth[k]) : 0.0;
	}
	const bool hasAll = tally[2] != 0;
	const double rateAll = hasAll ? double(tally[1]) / double(tally[2]) : 0.0;
	const bool hasExcess = has[2] && has[0], hasExplained = has[0] && hasAll && rateAll != 0.0;
	const double excess = hasExcess ? rate[2] - rate[0] : 0.0;
	const double explained = hasExplained ? 1 - rate[0] / rateAll : 0.0;
	if (!all && !(hasExcess && hasExplained && excess >= min_excess && explained >= min_explained)) return false;
	out += sample; out += "\t"; out += source;
	for (int k = 0; k < 3; ++k) { out += "\t"; out += std::to_string(r.sites[k]); }
	for (int k = 0; k < 3; ++k) { out += "\t"; out += has[k] ? std::to_string(rate[k]) : "NA"; }
	out += "\t"; out += hasExcess ? std::to_string(excess) : "NA";
	out += "\t"; out += hasExplained ? std::to_string(explained) : "NA";
	out += "\n";
	return true;
}

/* The lines of one band, targets in order and within a target the sources in order, the diagonal skipped: rec [n_rows][n_db],
 * tally [n_rows][3], names [n_db]. */
inline void band_text(std::string &out, const char *const *names, uint32_t n_db, uint32_t row_first, uint32_t n_rows, const ntsm_eval_contam_record *rec,
		const uint64_t *tally, bool all, double min_excess, double min_explained)
{
	for (uint32_t r = 0; r < n_rows; ++r)
		for (uint32_t d = 0; d < n_db; ++d)
			if (d != row_first + r)
				row_line(out, names[row_first + r], names[d], rec[(size_t) r * n_db + d], tally + 3 * (size_t) r, all, min_excess, min_explained);
}

/* one line of the --samples-out table, appended to out */
inline void sample_line(std::string &out, const char *name, const uint64_t tally[3])
{
	out += name; out += "\t"; out += std::to_string(tally[0]); out += "\t"; out += std::to_string(tally[1]); out += "\t"; out += std::to_string(tally[2]);
	out += "\t"; out += tally[2] ? std::to_string(double(tally[1]) / double(tally[2])) : "NA";
	out += "\n";
}

}  // namespace eval_contam
}  // namespace ntsm

#endif
