/*
 * eval_cli_rows.hpp -- the text ntsmEval prints on stdout (ntsm_eval_main.cpp): a sample's summaries, a scored pair's row
 * (resultsStr, src/CompareCounts.hpp:843-905), the QC row (computeScoreSingle, :541-585) and the printers of the three shapes
 * records come in: a candidate list, a block of a triangle or rectangle, the QC table.  Each is stated once for every run.
 */
#ifndef NTSM_EVAL_CLI_ROWS_HPP
#define NTSM_EVAL_CLI_ROWS_HPP

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <iostream>
#include <string>
#include <vector>

#include "../../../include/ntsm_eval_hip.h"
#include "eval_cli_args.hpp"
#include "eval_store.hpp"

namespace {

struct Counts {                              /* the members of CompareCounts the all-to-all path reads */
	std::vector<std::string> files, locus;
	std::vector<uint32_t> distinct;          /* [site][2] */
	std::vector<uint32_t> counts, sums;      /* [sample][site][2] */
	std::vector<uint64_t> rawTotal, total;
	std::vector<unsigned> kmerSize;
	size_t nSites() const { return locus.size(); }
};

struct Genotype { unsigned hets = 0, homs = 0, miss = 0; double errorRate = 0, cov = 0, radius = DBL_MAX; };

/* the library's tallies of one sample, geno [3] = hets, homs, miss */
inline void setTallies(Genotype &s, const uint32_t *geno) { s.hets = geno[0]; s.homs = geno[1]; s.miss = geno[2]; }

/* calcHomHetMiss (:742-767), computeErrorRate (:1198-1216), cov (:597-598) */
std::vector<Genotype> summaries(const Counts &c, const Opt &opt)
{
	const size_t m = c.nSites();
	std::vector<Genotype> g(c.files.size());
	const uint64_t distinctSum = ntsm::eval_store::sum_of_pairs(c.distinct.data(), m);
	for (size_t i = 0; i < g.size(); ++i) {
		const uint32_t *cnt = &c.counts[i * m * 2];
		for (size_t s = 0; s < m; ++s) {
			if (cnt[2 * s] > opt.minCov) { if (cnt[2 * s + 1] > opt.minCov) ++g[i].hets; else ++g[i].homs; }
			else if (cnt[2 * s + 1] > opt.minCov) ++g[i].homs;
			else ++g[i].miss;
		}
		g[i].errorRate = ntsm::eval_store::error_rate(c.rawTotal[i], c.kmerSize[i], ntsm::eval_store::sum_of_pairs(c.sums.data() + i * m * 2, m),
				distinctSum, opt.genomeSize);
		g[i].cov = double(c.total[i]) / double(m);
	}
	return g;
}

/* skew (:1081-1083) and computeLogLikelihood (:1093-1099) over a pair's record: sample i is sample 1 */
double pairScore(const ntsm_eval_record &r, const Genotype &gi, const Genotype &gj, const Opt &opt)
{
	double score = DBL_MAX;
	if (r.n_valid > 0) {
		score = -2.0 * (r.sum_joint - (r.sum_single1 + r.sum_single2));
		score = score / std::pow(gi.cov * gj.cov, opt.covSkew);
		score /= double(r.n_valid);
	}
	return score;
}

/* one scored pair (i, j), sample i as sample 1: kept under -a or below the threshold, then resultsStr (:843-905) + "\n"
 * on stdout; temp is the caller's line buffer */
void printRow(std::string &temp, const Counts &c, const std::vector<Genotype> &g, const Opt &opt, const ntsm_eval_record &r,
		uint32_t i, uint32_t j, const std::string &dist)
{
	const double score = pairScore(r, g[i], g[j], opt);
	if (!(opt.all || score < opt.scoreThresh)) return;
	const double homConcord = (double(r.shared_homs) - 2.0 * double(r.ibs0)) / double(r.homs1 < r.homs2 ? r.homs1 : r.homs2);
	const double relate = (double(r.shared_hets) - 2.0 * double(r.ibs0)) / double(r.hets1 < r.hets2 ? r.hets1 : r.hets2);
	temp.clear();
	temp += c.files[i]; temp += "\t"; temp += c.files[j]; temp += "\t"; temp += std::to_string(score);
	temp += opt.all ? (score < opt.scoreThresh ? "\t1\t" : "\t0\t") : "\t1\t";
	temp += dist; temp += "\t"; temp += std::to_string(relate);
	temp += "\t"; temp += std::to_string(r.ibs0); temp += "\t"; temp += std::to_string(r.ibs2);
	temp += "\t"; temp += std::to_string(homConcord);
	temp += "\t"; temp += std::to_string(r.hets1); temp += "\t"; temp += std::to_string(r.hets2); temp += "\t"; temp += std::to_string(r.shared_hets);
	temp += "\t"; temp += std::to_string(r.homs1); temp += "\t"; temp += std::to_string(r.homs2); temp += "\t"; temp += std::to_string(r.shared_homs);
	temp += "\t"; temp += std::to_string((uint64_t) r.n_valid);
	temp += "\t"; temp += std::to_string(g[i].cov); temp += "\t"; temp += std::to_string(g[j].cov);
	temp += "\t"; temp += std::to_string(g[i].errorRate); temp += "\t"; temp += std::to_string(g[j].errorRate);
	temp += "\t"; temp += std::to_string(g[i].miss); temp += "\t"; temp += std::to_string(g[j].miss);
	temp += "\t"; temp += std::to_string(g[i].homs); temp += "\t"; temp += std::to_string(g[j].homs);
	temp += "\t"; temp += std::to_string(g[i].hets); temp += "\t"; temp += std::to_string(g[j].hets);
	temp += "\n";
	std::cout << temp;
}

const char *kHeader = "sample1\tsample2\tscore\tsame\tdist\trelate\tibs0\tibs2\thomConcord\thet1\thet2\tsharedHet\thom1\thom2\tsharedHom\tn"
                      "\tcov1\tcov2\terrorRate1\terrorRate2\tmiss1\tmiss2\tallHom1\tallHom2\tallHet1\tallHet2";

/* the header and the rows of a candidate list with its records, in list order (computeScorePCA's output) */
void printCandidates(const Counts &c, const std::vector<Genotype> &g, const Opt &opt, const std::vector<uint32_t> &pi, const std::vector<uint32_t> &pk,
		const std::vector<double> &dist, const ntsm_eval_record *rec)
{
	std::cout << kHeader << "\n";
	std::string temp;
	for (size_t p = 0; p < pi.size(); ++p) printRow(temp, c, g, opt, rec[p], pi[p], pk[p], std::to_string(dist[p]));
}

/* the rows (i, j) of computeScore's output (:591-624) with i in [rowFirst, rowEnd), j in [colFirst, colEnd) and i < j, row by
 * row: a band of a triangle (colFirst = 0) or of a rectangle whose columns lie after its rows; after the header where this is
 * the first block.  recordOf(i, j) is the pair's record. */
template <typename RecordOf>
void printBlock(const Counts &c, const std::vector<Genotype> &g, const Opt &opt, bool header, uint32_t rowFirst, uint32_t rowEnd, uint32_t colFirst,
		uint32_t colEnd, RecordOf recordOf)
{
	if (header) std::cout << kHeader << "\n";
	std::string temp;
	for (uint32_t i = rowFirst; i < rowEnd; ++i)
		for (uint32_t j = std::max(colFirst, i + 1); j < colEnd; ++j) printRow(temp, c, g, opt, recordOf(i, j), i, j, "-1");
}

/* computeScoreSingle's header (:541-585), with the PC columns of -p where dim is not 0 */
std::string qcHeader(unsigned dim)
{
	std::string head = "sample\tcov\terrorRate\tmiss\thom\thet";
	for (unsigned d = 1; d <= dim; ++d) { head += "\tPC"; head += std::to_string(d); }
	return head;
}

/* and its row of one sample, cloud [dim] its projection: the single-file run prints it as it is, --qc with "\n" after it */
std::string qcRow(const std::string &name, const Genotype &s, const double *cloud, unsigned dim)
{
	std::string row = name;
	row += "\t"; row += std::to_string(s.cov); row += "\t"; row += std::to_string(s.errorRate);
	row += "\t"; row += std::to_string(s.miss); row += "\t"; row += std::to_string(s.homs); row += "\t"; row += std::to_string(s.hets);
	for (unsigned d = 0; d < dim; ++d) { row += "\t"; row += std::to_string(cloud[d]); }
	return row;
}

}  // namespace

#endif
