/*
 * ntsm_eval_main.cpp -- host mirror of the reference's ntsmEval (src/ntSeqMatchEval.cpp:86-349, src/CompareCounts.hpp):
 * same flags, same stdout bytes; the scoring is the HIP library's (include/ntsm_eval_hip.h).  The runs and their calls:
 *   FILES...                  all pairs, computeScore (:591-624): ntsm_eval_pairs
 *   FILE                      the QC table, computeScoreSingle (:541-585): no GPU unless -p asks for its PC columns
 *   -e FILE [-o]              the merged counts, mergeCounts (:626-674), after the analysis or (-o) in its place: no GPU
 *   -p ROT -n NORM FILES...   the PCA-guided search, projectPCs (:116-211) + computeScorePCA (:285-398), printed in the
 *                             one-thread order: ntsm_eval_open, _project, _candidates, _score_pairs
 * This build only:
 *   --pack STORE FILES...     writes or extends a cohort store (eval_store.hpp): no GPU
 *   --against STORE FILES...  computeScore's rows of FILES against the store's samples and each other: ntsm_eval_cross, ntsm_eval_pairs
 *   --index STORE -p -n       projects the store's samples into STORE.pcaidx (eval_index.hpp): ntsm_eval_project_store
 *   --near STORE FILES...     the rows of the -p run over [FILES..., the store's samples] that name one of FILES, through that
 *                             index: ntsm_eval_cross_candidates, then ntsm_eval_cross for the search-all queries' rows and
 *                             ntsm_eval_cross_score_pairs for the rest
 *   --within STORE            the all-to-all run over the store's own samples, in bands of rows: ntsm_eval_within_open / _rows
 *   --within-near STORE       the -p run over them through the index: ntsm_eval_cross_candidates without a database side, then
 *                             ntsm_eval_cross for the search-all samples' rows and ntsm_eval_store_score_pairs for the rest
 *   --between STORE_A STORE_B the rows of the all-to-all run over [A's samples, B's samples] that pair a sample of A with one of
 *                             B, B's loci matched to A's by ID, in bands of rows of A: ntsm_eval_between_open / _rows
 *   --between-near STORE_A STORE_B   the rows of the -p run over them that pair a sample of A with one of B, through A's index:
 *                             B's projections from its own index where that serves, else ntsm_eval_project_store_mapped; then
 *                             ntsm_eval_between_candidates, ntsm_eval_between_rows for the search-all rows of A and
 *                             ntsm_eval_between_score_pairs for the rest
 *   --qc STORE [-p ROT -n NORM] [--sites-out FILE]   computeScoreSingle's table (:541-585) with one row per sample of the store,
 *                             and per-site tallies under the same rule: ntsm_eval_store_profile; the PC columns of -p from
 *                             ntsm_eval_project_store
 *   --contam STORE [--samples-out FILE]   is a sample a mixture, and of whom: every ordered pair (target, source) of the store,
 *                             in bands of targets: ntsm_eval_contam_open / _rows; the table's text is eval_contam.hpp's
 *   --trios STORE [--ped FILE]   which samples form a parent-parent-child trio, or do a pedigree's trios hold: bit-planes of
 *                             genotype classes on the device: ntsm_eval_trio_open / _duos / _score; the runs and the text are
 *                             eval_trio.hpp's
 *   --ld STORE [--ld-prune FILE]   which pairs of sites are in linkage disequilibrium, and which sites does a prune keep:
 *                             bit-planes with the samples along the bits on the device: ntsm_eval_ld_open / _select; the
 *                             moments, the band walk, the text and the prune are eval_ld.hpp's
 * --within, --within-near, --between, --between-near, --qc, --contam, --trios and --ld read no counts file.  Not built, and refused: -b (the debug ground-truth mode) and -p without a
 * normalization file (the reference dies in an assert).  Pinned to the reference: stdout equals, byte for byte, that of the
 * unmodified scoring class (oracle/ref_eval_driver.cpp -> oracle/_ref/ref_ntsmEval -t 1) and its recordings,
 * tests/test_eval_reference.py.
 */
#include <getopt.h>

#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <iostream>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/ntsm_eval_hip.h"
#include "cli.hpp"
#include "eval_between.hpp"
#include "eval_contam.hpp"
#include "eval_index.hpp"
#include "eval_ld.hpp"
#include "eval_qc.hpp"
#include "eval_store.hpp"
#include "eval_trio.hpp"
#include "eval_within.hpp"

#define PROGRAM "ntsmEval"

namespace {

struct Opt {                                 /* src/Options.h:44-55 */
	double scoreThresh = 0.5, covSkew = 0.2;
	bool all = false;
	unsigned minCov = 1, threads = 1;
	uint64_t genomeSize = 6200000000ull;
	int verbose = 0, device = 0;
	std::string pca, merge, norm, debug;
	std::string pack, against;               /* --pack STORE, --against STORE (this build only) */
	std::string index, near;                 /* --index STORE, --near STORE: the PCA-guided search against a store */
	std::string within, withinNear;          /* --within STORE, --within-near STORE: the store's samples against each other */
	unsigned withinRows = 0;                 /* --within-rows N: rows per band of --within, 0 = the band rule */
	bool withinRowsGiven = false;
	std::string between;                     /* --between STORE_A; STORE_B is the one positional argument */
	unsigned betweenRows = 0;                /* --between-rows N: rows of A per band of --between, 0 = the band rule */
	bool betweenRowsGiven = false;
	std::string betweenNear;                 /* --between-near STORE_A; STORE_B is the one positional argument */
	std::string qc, sitesOut;                /* --qc STORE: the QC table of the store's samples; --sites-out FILE: its per-site table */
	bool sitesOutGiven = false;
	std::string contam, samplesOut;          /* --contam STORE: the contamination check over the store; --samples-out FILE: its per-sample table */
	unsigned contamDepth = ntsm::eval_contam::kMinDepth, contamRows = 0;   /* --contam-depth D; --contam-rows N: targets per band, 0 = the band rule */
	double contamMin = ntsm::eval_contam::kMinExcess, contamExplained = ntsm::eval_contam::kMinExplained;   /* --contam-min X, --contam-explained Y */
	bool samplesOutGiven = false, contamFlagGiven = false;
	std::string trios, ped;                  /* --trios STORE: parent-child trios in the store; --ped FILE: the trios to check instead of a search */
	unsigned trioDepth = ntsm::eval_trio::kMinDepth, trioCalled = ntsm::eval_trio::kMinCalled;   /* --trio-depth D, --trio-called M */
	double trioMax = ntsm::eval_trio::kMaxRate, trioDuo = ntsm::eval_trio::kMaxDuo;              /* --trio-max X, --trio-duo Y */
	bool trioExhaustive = false, trioFlagGiven = false, pedGiven = false;
	std::string ld, ldPrune;                 /* --ld STORE: site-pair LD over the store; --ld-prune FILE: the IDs of the sites a prune keeps */
	unsigned ldDepth = ntsm::eval_ld::kMinDepth, ldCalled = ntsm::eval_ld::kMinCalled;   /* --ld-depth D, --ld-called M */
	double ldMin = ntsm::eval_ld::kMinR2;    /* --ld-min T */
	bool ldFlagGiven = false, ldPruneGiven = false;
	bool minCovGiven = false, dimGiven = false;
	bool onlyMerge = false;
	unsigned dim = 20;                       /* src/Options.h:22, 35-39: the PCA search */
	double pcSearchRadius1 = 2, pcSearchRadius2 = 15, pcErrorThresh = 0.01, pcMissSite1 = 0.01, pcMissSite2 = 0.3;
};

struct Counts {                              /* the members of CompareCounts the all-to-all path reads */
	std::vector<std::string> files, locus;
	std::vector<uint32_t> distinct;          /* [site][2] */
	std::vector<uint32_t> counts, sums;      /* [sample][site][2] */
	std::vector<uint64_t> rawTotal, total;
	std::vector<unsigned> kmerSize;
	size_t nSites() const { return locus.size(); }
};

/* src/CompareCounts.hpp:30-114: the first file fixes loci and distinct counts, then every file fills its row.  Under
 * --against the store has fixed them (c.locus, c.distinct and `index` come filled) and a locus it lacks is a refusal.  The
 * reading of one file is eval_store.hpp's, shared with --pack. */
void load(Counts &c, ntsm::eval_store::LocusIndex index = {}, bool fromStore = false)
{
	if (!fromStore) ntsm::eval_store::read_locus_table(c.files.at(0), index, c.locus, c.distinct);
	const size_t n = c.files.size(), m = c.nSites();
	c.counts.assign(n * m * 2, 0u);
	c.sums.assign(n * m * 2, 0u);
	c.rawTotal.assign(n, 0);
	c.total.assign(n, 0);
	c.kmerSize.assign(n, 0);
	for (size_t i = 0; i < n; ++i) {
		ntsm::eval_store::Scalars sc;
		ntsm::eval_store::parse_counts_file(c.files[i], index, c.counts.data() + i * m * 2, c.sums.data() + i * m * 2, sc, fromStore);
		c.rawTotal[i] = sc.raw_total;
		c.total[i] = sc.total;
		c.kmerSize[i] = sc.kmer_size;
	}
}

struct Genotype { unsigned hets = 0, homs = 0, miss = 0; double errorRate = 0, cov = 0, radius = DBL_MAX; };

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

void printHelpDialog()
{
	const Opt d;
	std::cerr << "Usage: " PROGRAM " [FILES...]\n"
	    "Processes sets of counts files and compares their similarity.\n"
	    "If only a single file is provided general QC information returned.\n"
	    "  -t, --threads              Number of threads to run.[1]\n"
	    "  -s, --score_thresh = FLOAT Score threshold [" << std::to_string(d.scoreThresh) << "]\n"
	    "  -a, --all                  Output results of all tests tried, not just those that\n"
	    "                             pass the score threshold.\n"
	    "  -w, --skew = FLOAT         Divides the score by coverage. Formula: (cov1*cov2)^skew\n"
	    "                             Set to zero for no skew.[" << std::to_string(d.covSkew) << "]\n"
	    "  -c, --min_cov = INT        Keep only sites with this coverage and above.[" << std::to_string(d.minCov) << "]\n"
	    "  -g, --genome_size = INT    Diploid genome size for error rate estimation.\n"
	    "                             [" << std::to_string(d.genomeSize) << "]\n"
	    "  -e, --merge = STR          After analysis merge counts and output to file.\n"
	    "  -o, --only_merge           Do not perform an analysis. Only functions when\n"
	    "                             -e (--merge) option is specified.\n"
	    "  -p, --pca = STR            Use PCA information to speed up analysis. Input is a\n"
	    "                             set of rotational values from a PCA.\n"
	    "  -d, --dim = INT            Number of dimensions to consider in PCA. [" << std::to_string(d.dim) << "]\n"
	    "  -n, --norm = STR           Set of values use to center the data before rotation\n"
	    "                             during PCA. [Required if -p is enabled]\n"
	    "  -r, --error_rate = FLOAT   Error rate threshold for PCA based search [" << std::to_string(d.pcErrorThresh) << "]\n"
	    "  -1, --miss_small = FLOAT   Missing site threshold small for PCA based search [" << std::to_string(d.pcMissSite1) << "]\n"
	    "  -2, --miss_large = FLOAT   Missing site threshold large PCA based search [" << std::to_string(d.pcMissSite2) << "]\n"
	    "  -S, --small = FLOAT        Search radius for small PCA based search [" << std::to_string(d.pcSearchRadius1) << "]\n"
	    "  -l, --large = FLOAT        Search radius for large PCA based search [" << std::to_string(d.pcSearchRadius2) << "]\n"
	    "  -h, --help                 Display this dialog.\n"
	    "  -v, --verbose              Display verbose output.\n"
	    "This build only:\n"
	    "  -G, --gpu = INT            HIP device [0]\n"
	    "      --pack = STORE         Write the counts of FILES to the binary cohort store\n"
	    "                             STORE, or append them if it exists. Needs no GPU.\n"
	    "      --against = STORE      Score FILES against every sample of STORE and against\n"
	    "                             each other: the rows of the all-to-all run over FILES\n"
	    "                             followed by the store's samples whose sample1 is one of\n"
	    "                             FILES. Not with -p, -b, -e or -o.\n"
	    "      --index = STORE        Project every sample of STORE with -p ROT -n NORM [-d -c]\n"
	    "                             and write STORE.pcaidx, or extend it after an append.\n"
	    "                             Takes no FILES.\n"
	    "      --near = STORE         PCA-guided search of FILES against STORE through\n"
	    "                             STORE.pcaidx: the rows of the -p run over FILES followed\n"
	    "                             by the store's samples that name one of FILES. Rotation,\n"
	    "                             centre, -d and -c come from the index. Not with -p, -n,\n"
	    "                             -b, -e or -o.\n"
	    "      --within = STORE       The all-to-all run over the samples of STORE, read from\n"
	    "                             the store alone. Takes no FILES. Not with -p, -n, -b, -e\n"
	    "                             or -o.\n"
	    "      --within-near = STORE  The PCA-guided run (-p) over the samples of STORE through\n"
	    "                             STORE.pcaidx. Takes no FILES; rotation, centre, -d and -c\n"
	    "                             come from the index. Not with -p, -n, -b, -e or -o.\n"
	    "      --within-rows = INT    Rows per band of --within [0: as many as fit in 1 GiB of\n"
	    "                             records]. For tests and measurements.\n"
	    "      --between = STORE_A STORE_B\n"
	    "                             Score every sample of STORE_A against every sample of\n"
	    "                             STORE_B: the rows of the all-to-all run over A's samples\n"
	    "                             followed by B's that pair a sample of A (sample1) with\n"
	    "                             one of B (sample2). STORE_B is the one positional\n"
	    "                             argument; there are no FILES. B's loci are matched to A's\n"
	    "                             by ID: a locus B lacks counts 0 / 0, a locus A lacks is\n"
	    "                             refused. Not with -p, -n, -b, -e or -o.\n"
	    "      --between-rows = INT   Rows of STORE_A per band of --between [0 is refused;\n"
	    "                             absent: as many as fit in 1 GiB of records]. For tests\n"
	    "                             and measurements.\n"
	    "      --between-near = STORE_A STORE_B\n"
	    "                             The PCA-guided run (-p) over the samples of STORE_A\n"
	    "                             followed by those of STORE_B, through STORE_A.pcaidx: the\n"
	    "                             rows that pair a sample of one store with a sample of the\n"
	    "                             other. STORE_B is the one positional argument; loci as\n"
	    "                             for --between. Rotation, centre, -d and -c come from A's\n"
	    "                             index; B's projections from STORE_B.pcaidx where it was\n"
	    "                             written over the same loci with the same matrices, else\n"
	    "                             they are computed in the run. Not with -p, -n, -b, -e or\n"
	    "                             -o.\n"
	    "      --qc = STORE           The QC table of the single-file run with one row per sample\n"
	    "                             of STORE, in store order: sample cov errorRate miss hom\n"
	    "                             het, and with -p ROT -n NORM [-d] the PC columns. Every\n"
	    "                             row ends in a newline (the single-file run prints its one\n"
	    "                             row without one). Takes no FILES; reads and writes no\n"
	    "                             STORE.pcaidx. -a, -s, -w and the radius flags have no\n"
	    "                             effect. Not with -b, -e or -o.\n"
	    "      --sites-out = FILE     With --qc: write one line per locus of STORE to FILE:\n"
	    "                             #locusID called miss homAT homCG het freqAT hetObs hetExp\n"
	    "                             meanCov, the genotypes by the scoring's rule at -c.\n"
	    "      --contam = STORE       Is a sample of STORE a mixture, and of which other sample?\n"
	    "                             One row per ordered pair (sample, source) of the store:\n"
	    "                             at the sites where the sample looks homozygous (minor\n"
	    "                             allele below a quarter of at least --contam-depth reads)\n"
	    "                             the share of minor-allele reads where the source lacks\n"
	    "                             that allele (rateLack), has both (rateHet) or has only it\n"
	    "                             (rateOpp); excess = rateOpp - rateLack; explained =\n"
	    "                             1 - rateLack / the sample's rate over all such sites.\n"
	    "                             Without -a only rows with excess >= --contam-min and\n"
	    "                             explained >= --contam-explained. -c is the coverage above\n"
	    "                             which the source carries an allele. Takes no FILES. Not\n"
	    "                             with -p, -n, -b, -e or -o.\n"
	    "      --contam-depth = INT   Least depth of a site of the sample [" << std::to_string(d.contamDepth) << "]\n"
	    "      --contam-min = FLOAT   Least excess of a printed row [" << std::to_string(d.contamMin) << "]\n"
	    "      --contam-explained = FLOAT\n"
	    "                             Least explained share of a printed row [" << std::to_string(d.contamExplained) << "]\n"
	    "                             Both defaults are conventions to override: they come from\n"
	    "                             one simulation, not from real data.\n"
	    "      --contam-rows = INT    Samples per band of --contam [0: as many as fit in 1 GiB\n"
	    "                             of records]. For tests and measurements.\n"
	    "      --samples-out = FILE   With --contam: write one line per sample of STORE to\n"
	    "                             FILE: #sample sites minorReads depth rateAll.\n"
	    "      --trios = STORE        Which samples of STORE form a parent-parent-child trio?\n"
	    "                             A site of a sample is het when both alleles are above -c,\n"
	    "                             homozygous when one is and the site has at least\n"
	    "                             --trio-depth reads, else missing. A sample is a candidate\n"
	    "                             parent of a child when they share at least --trio-called\n"
	    "                             called sites and are opposite homozygotes at no more than\n"
	    "                             --trio-duo of them. One row per child and pair of its\n"
	    "                             candidates: child parentA parentB called errHom errHet\n"
	    "                             rate calledA oppA calledB oppB, the Mendelian errors over\n"
	    "                             the sites all three are called at. Without -a only rows\n"
	    "                             with called >= --trio-called and rate <= --trio-max.\n"
	    "                             Takes no FILES. Not with -p, -n, -b, -e or -o.\n"
	    "      --trio-depth = INT     Least depth of a homozygous site [" << std::to_string(d.trioDepth) << "]\n"
	    "      --trio-max = FLOAT     Largest error rate of a printed trio [" << std::to_string(d.trioMax) << "]\n"
	    "      --trio-duo = FLOAT     Largest opposite-homozygote rate of a candidate parent\n"
	    "                             [" << std::to_string(d.trioDuo) << "]\n"
	    "      --trio-called = INT    Least called sites of a candidate and of a printed trio\n"
	    "                             [" << std::to_string(d.trioCalled) << "]\n"
	    "                             All four defaults are conventions to override: they come\n"
	    "                             from one simulation, not from real data.\n"
	    "      --trio-exhaustive      With --trios: every pair of other samples is tried for\n"
	    "                             every child, without the candidate step.\n"
	    "      --ped = FILE           With --trios: no search. Check the trios of the six-column\n"
	    "                             pedigree FILE (columns 2-4: individual, father, mother;\n"
	    "                             lines with a 0 parent are skipped). An ID names the sample\n"
	    "                             whose stored name, basename, or basename without\n"
	    "                             _counts.txt, .counts.txt or .txt it equals. One row per\n"
	    "                             trio in file order, with a last column verdict: lowcov\n"
	    "                             (called < --trio-called), ok (rate <= --trio-max) or fail.\n"
	    "                             Not with -a or --trio-exhaustive.\n"
	    "      --ld = STORE           Which pairs of sites of STORE are in linkage disequilibrium?\n"
	    "                             Classes as for --trios, gated by --ld-depth; dosage 0 / 1 /\n"
	    "                             2 = homAT / het / homCG; r2 is the squared correlation of\n"
	    "                             the dosages over the samples called at both sites,\n"
	    "                             undefined below --ld-called such samples or where a site\n"
	    "                             does not vary among them. One row per pair of sites in\n"
	    "                             store order with r2 >= --ld-min: siteA siteB n r2 dir, dir\n"
	    "                             the sign of the covariance. With -a every pair with a\n"
	    "                             defined r2. Takes no FILES. Not with -p, -n, -b, -e or -o.\n"
	    "      --ld-depth = INT       Least depth of a homozygous site [" << std::to_string(d.ldDepth) << " reads]\n"
	    "      --ld-min = FLOAT       Least r2 of a printed pair [" << std::to_string(d.ldMin) << "]\n"
	    "      --ld-called = INT      Least samples called at both sites [" << std::to_string(d.ldCalled) << " samples]\n"
	    "                             All three defaults are conventions to override.\n"
	    "      --ld-prune = FILE      With --ld: write the IDs of the sites a greedy prune keeps\n"
	    "                             to FILE, one per line: in store order a site is dropped\n"
	    "                             when it pairs at r2 >= --ld-min with an earlier kept site\n"
	    "                             (also under -a).\n"
	    "Not in this build: -b (debug mode of the PCA search); the PCA-guided search (-p)\n"
	    "against a store (--index and --near are that search); merging (-e) from a store.\n" << std::endl;
	exit(EXIT_SUCCESS);
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

/* projectPCs' input files (:120-165): norm values (one long double per line, 0 where a line does not parse) and the first
 * opt.dim components of the rotation rows, matched to sites by position.  Stops the program where the reference asserts
 * (dim > components, rows != norm values) and where it would read past its arrays (fewer values than sites). */
void loadPCA(const Opt &opt, size_t nSites, std::vector<long double> &norm, std::vector<long double> &rot /*[dim][nSites]*/)
{
	if (opt.verbose > 0) std::cerr << "Projecting samples onto PCA" << std::endl;
	std::vector<long double> normVals;
	{
		std::ifstream fh(opt.norm);
		std::string line;
		while (fh.is_open() && std::getline(fh, line)) {
			std::stringstream ss(line);
			long double value = 0;
			ss >> value;
			normVals.push_back(value);
		}
	}
	unsigned compNum = 0;
	std::ifstream fh(opt.pca);
	std::string line;
	std::getline(fh, line);
	{
		std::stringstream ss(line);
		std::string val;
		ss >> val;
		while (ss >> val) ++compNum;
	}
	if (opt.verbose > 0) std::cerr << "Detected " << compNum << " components for " << normVals.size() << " sites" << std::endl;
	if (opt.dim > compNum) {                                 /* assert(opt::dim <= compNum), :153 */
		std::cerr << PROGRAM ": -d " << opt.dim << " exceeds the " << compNum << " components of " << opt.pca << std::endl;
		abort();
	}
	std::vector<std::vector<long double>> rows;             /* [row][dim] */
	while (std::getline(fh, line)) {
		std::stringstream ss(line);
		std::string rsID;
		ss >> rsID;
		std::vector<long double> v(opt.dim, 0.0L);
		for (unsigned d = 0; d < opt.dim; ++d) ss >> v[d];  /* after a failed read the rest stay 0, as in the reference */
		rows.push_back(std::move(v));
	}
	if (rows.size() != normVals.size()) {                   /* assert(index == normVals.size()), :165 */
		std::cerr << PROGRAM ": " << rows.size() << " rotation rows but " << normVals.size() << " normalization values" << std::endl;
		abort();
	}
	if (normVals.size() < nSites) {
		std::cerr << "Error: " << normVals.size() << " normalization values and rotation rows for " << nSites
		          << " sites; a PCA search with fewer values than sites is not part of this build" << std::endl;
		exit(EXIT_FAILURE);
	}
	norm.assign(normVals.begin(), normVals.begin() + nSites);
	rot.assign((size_t) opt.dim * nSites, 0.0L);
	for (size_t j = 0; j < nSites; ++j)
		for (unsigned d = 0; d < opt.dim; ++d) rot[(size_t) d * nSites + j] = rows[j][d];
}

int gpuFail(const char *what, int rc)
{
	std::cerr << PROGRAM ": " << what << " on the GPU failed (" << rc << "); there is no CPU path" << std::endl;
	return 3;
}

template <typename H, void (*Close)(H *)> struct Handle {   /* closes the library session it holds when its scope ends */
	H *h = nullptr;
	~Handle() { if (h) Close(h); }
};
typedef Handle<ntsm_eval_session, ntsm_eval_close> Session;
typedef Handle<ntsm_eval_within_session, ntsm_eval_within_close> WithinSession;
typedef Handle<ntsm_eval_between_session, ntsm_eval_between_close> BetweenSession;
typedef Handle<ntsm_eval_contam_session, ntsm_eval_contam_close> ContamSession;
typedef Handle<ntsm_eval_trio_session, ntsm_eval_trio_close> TrioSession;
typedef Handle<ntsm_eval_ld_session, ntsm_eval_ld_close> LdSession;

typedef std::chrono::steady_clock Clock;
double msSince(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }

void printTime(Clock::time_point t0)         /* the last line of every run's stderr */
{
	std::cerr << "Time: " << std::chrono::duration<double>(Clock::now() - t0).count() << " s" << std::endl;
}

/* projectPCs (:166-211) on the device: cloud [n][dim] */
int project(const Counts &c, const Opt &opt, ntsm_eval_session *h, const std::vector<long double> &norm, const std::vector<long double> &rot,
		std::vector<double> &cloud)
{
	cloud.assign(c.files.size() * (size_t) opt.dim, 0.0);
	double ms = 0;
	const int rc = ntsm_eval_project(h, norm.data(), rot.data(), opt.dim, cloud.data(), &ms);
	if (rc) return gpuFail("projection", rc);
	if (opt.verbose > 2)
		for (const std::string &f : c.files) std::cerr << "Normalizing " << f << std::endl;
	if (opt.verbose > 1) std::cerr << "projection kernel: " << ms << " ms" << std::endl << "Finished Normalization " << std::endl;
	return 0;
}

/* the squared search radius of every sample (:297-305; pow(x, 2) = x * x); DBL_MAX = search all */
std::vector<double> searchRadii(std::vector<Genotype> &g, size_t m, const Opt &opt)
{
	std::vector<double> radius(g.size());
	for (size_t i = 0; i < g.size(); ++i) {
		const double propMissing = double(g[i].miss) / double(m);
		g[i].radius = DBL_MAX;
		if (g[i].errorRate < opt.pcErrorThresh && propMissing < opt.pcMissSite1) g[i].radius = opt.pcSearchRadius1 * opt.pcSearchRadius1;
		else if (propMissing < opt.pcMissSite2) g[i].radius = opt.pcSearchRadius2 * opt.pcSearchRadius2;
		radius[i] = g[i].radius;
	}
	return radius;
}

/* A candidate list and the two calls that fetch it: ask the size with no room, allocate, ask again.  `call` is the library's
 * search with its inputs bound: (pi, pk, dist, capacity, &n_pairs, &kernel_ms). */
struct Candidates {
	std::vector<uint32_t> pi, pk;
	std::vector<double> dist;
	double kernelMs = 0;
	int search(const std::function<int(uint32_t *, uint32_t *, double *, uint64_t, uint64_t *, double *)> &call)
	{
		uint64_t np = 0;
		int rc = call(nullptr, nullptr, nullptr, 0, &np, &kernelMs);
		if (rc && rc != NTSM_EVAL_E_CAPACITY) return gpuFail("candidate search", rc);
		pi.resize(np); pk.resize(np); dist.resize(np);
		if (np && (rc = call(pi.data(), pk.data(), dist.data(), np, &np, &kernelMs)) != 0) return gpuFail("candidate search", rc);
		return 0;
	}
};

/* computeScorePCA (:285-398), the one-thread order of its rows */
int scorePCA(const Counts &c, std::vector<Genotype> &g, const Opt &opt, ntsm_eval_session *h, const std::vector<double> &cloud)
{
	if (opt.verbose > 1) std::cerr << "Generating kd-tree" << std::endl;
	const std::vector<double> radius = searchRadii(g, c.nSites(), opt);
	if (opt.verbose > 1) std::cerr << "Starting Score Computation with PCA" << std::endl;
	Candidates cand;
	int rc = cand.search([&](uint32_t *pi, uint32_t *pk, double *dist, uint64_t capacity, uint64_t *np, double *ms) {
		return ntsm_eval_candidates(h, cloud.data(), opt.dim, radius.data(), pi, pk, dist, capacity, np, ms);
	});
	if (rc) return rc;
	const uint64_t np = cand.pi.size();
	double msScore = 0;
	std::vector<ntsm_eval_record> rec(np);
	rc = ntsm_eval_score_pairs(h, cand.pi.data(), cand.pk.data(), np, rec.data(), &msScore);
	if (rc) return gpuFail("scoring", rc);
	if (opt.verbose > 1) std::cerr << "search kernels: " << cand.kernelMs << " ms, scoring kernel: " << msScore << " ms for " << np << " pairs" << std::endl;
	std::cout << kHeader << "\n";
	std::string temp;
	for (uint64_t p = 0; p < np; ++p) printRow(temp, c, g, opt, rec[p], cand.pi[p], cand.pk[p], std::to_string(cand.dist[p]));
	return 0;
}

constexpr int kOptPack = 1000, kOptAgainst = 1001, kOptIndex = 1002, kOptNear = 1003, kOptWithin = 1004, kOptWithinNear = 1005,
              kOptWithinRows = 1006, kOptBetween = 1007, kOptBetweenRows = 1008, kOptBetweenNear = 1009, kOptQc = 1010, kOptSitesOut = 1011,
              kOptContam = 1012, kOptContamDepth = 1013, kOptContamMin = 1014, kOptContamExplained = 1015, kOptContamRows = 1016, kOptSamplesOut = 1017,
              kOptTrios = 1018, kOptTrioDepth = 1019, kOptTrioMax = 1020, kOptTrioDuo = 1021, kOptTrioCalled = 1022, kOptTrioExhaustive = 1023, kOptPed = 1024,
              kOptLd = 1025, kOptLdDepth = 1026, kOptLdMin = 1027, kOptLdCalled = 1028, kOptLdPrune = 1029;   /* long-only: no letter of the reference's option string is taken */

/* --pack STORE FILES...: no GPU */
int packStore(const Counts &c, const Opt &opt)
{
	try {
		const uint64_t n = ntsm::eval_store::pack(opt.pack, c.files);
		if (opt.verbose > 0) std::cerr << "Packed " << c.files.size() << " files; " << opt.pack << " holds " << n << " samples" << std::endl;
	} catch (const std::exception &e) {                   /* a refusal, or a number that does not parse: the store is as it was */
		ntsm::refuse(e.what());
	}
	return 0;
}

/* What every store run opens: the mapped store, refused when it is empty or holds more samples than a run with nFiles
 * further ones numbers ("... one run scores" / "... one run projects").  With c, its locus table and distinct columns play
 * the part of the first file.  Throws the refusal. */
void openStore(const std::string &name, size_t nFiles, const char *does, ntsm::eval_store::View &store, Counts *c)
{
	namespace st = ntsm::eval_store;
	store.open(name);
	if (store.h.n_samples == 0) throw st::Error(name + " holds no samples");
	if (store.h.n_samples + nFiles > UINT32_MAX) throw st::Error(name + " holds more samples than one run " + does);
	if (!c) return;
	c->locus = store.locus;
	c->distinct.assign(store.distinct, store.distinct + 2 * (size_t) store.h.n_sites);
}

/* the store's samples as samples nq ... of a run: names, summaries from the record scalars and the given tallies.  The sites
 * are the run's (c.locus: the table of the store that openStore gave c, which under --between is not this store's). */
void appendStoreSamples(Counts &c, std::vector<Genotype> &g, const ntsm::eval_store::View &store, const Opt &opt,
		const std::function<void(uint32_t, Genotype &)> &tallies)
{
	namespace st = ntsm::eval_store;
	const uint32_t nq = (uint32_t) c.files.size(), nd = (uint32_t) store.h.n_samples, m = (uint32_t) c.nSites();
	const uint64_t distinctSum = st::sum_of_pairs(c.distinct.data(), m);
	g.resize((size_t) nq + nd);
	c.files.reserve((size_t) nq + nd);
	for (uint32_t d = 0; d < nd; ++d) {
		const st::RecordHead &h = store.head(d);
		Genotype &s = g[nq + d];
		tallies(d, s);
		s.errorRate = st::error_rate(h.raw_total, h.kmer_size, h.sum_of_sums, distinctSum, opt.genomeSize);
		s.cov = double(h.total) / double(m);
		c.files.push_back(store.name(d));
	}
}

/* --against STORE FILES...: the rows of computeScore (:591-624) over [FILES..., the store's samples] whose sample 1 is one
 * of FILES -- a prefix of that run's output.  The store's locus table and distinct columns play the part of the first file. */
int scoreAgainst(Counts &c, const Opt &opt, Clock::time_point t0)
{
	ntsm::eval_store::View store;
	const auto tMap = Clock::now();
	try {
		openStore(opt.against, c.files.size(), "scores", store, &c);
		if (opt.verbose > 0) std::cerr << "Reading count files" << std::endl;
		load(c, store.index(), true);
	} catch (const std::exception &e) {
		ntsm::refuse(e.what());
	}
	const double mapMs = msSince(tMap);                  /* mapping the store and reading the query files */
	std::vector<Genotype> g = summaries(c, opt);
	const uint32_t nq = (uint32_t) c.files.size(), nd = (uint32_t) store.h.n_samples, m = store.h.n_sites;
	if (opt.verbose > 1) std::cerr << "Finished loading files. Now comparing " << nq << " samples against the " << nd << " of " << opt.against << "." << std::endl;
	std::cerr << "Performing all-to-all score computation.\nSpecify -p (--pca) to enable faster comparisons." << std::endl;
	std::vector<ntsm_eval_record> qq((size_t) nq * (nq - 1) / 2), cross((size_t) nq * nd);
	std::vector<uint32_t> geno((size_t) nd * 3);
	double ms = 0;
	int rc = nq >= 2 ? ntsm_eval_pairs(opt.device, c.counts.data(), nq, m, opt.minCov, qq.data(), &ms) : 0;
	if (rc) return gpuFail("scoring", rc);
	ntsm_eval_cross_times times {};
	rc = ntsm_eval_cross(opt.device, c.counts.data(), nq, store.counts(0), store.h.stride, nd, m, opt.minCov, 0, cross.data(), geno.data(), &times);
	if (rc) return gpuFail("scoring against the store", rc);
	appendStoreSamples(c, g, store, opt, [&](uint32_t d, Genotype &s) { s.hets = geno[3 * d]; s.homs = geno[3 * d + 1]; s.miss = geno[3 * d + 2]; });
	const auto tPrint = Clock::now();
	std::cout << kHeader << "\n";
	std::string temp;
	for (uint32_t q = 0; q < nq; ++q) {
		for (uint32_t j = q + 1; j < nq; ++j) printRow(temp, c, g, opt, qq[ntsm_eval_pair_index(q, j, nq)], q, j, "-1");
		for (uint32_t d = 0; d < nd; ++d) printRow(temp, c, g, opt, cross[(size_t) q * nd + d], q, nq + d, "-1");
	}
	std::cout.flush();
	if (opt.verbose > 1)
		std::cerr << "store query: " << times.chunks << " chunks, map+load " << mapMs << " ms, query pairs " << ms << " ms, upload " << times.upload_ms
		          << " ms, prepare " << times.prepare_kernel_ms << " ms, cross kernel " << times.cross_kernel_ms << " ms, download " << times.download_ms
		          << " ms, print " << msSince(tPrint) << " ms" << std::endl;
	printTime(t0);
	return 0;
}

/* --index STORE -p ROT -n NORM [-d -c]: project the store's samples, or the tail an append added, into STORE.pcaidx */
int buildIndex(const Opt &opt, Clock::time_point t0)
{
	namespace st = ntsm::eval_store;
	namespace ix = ntsm::eval_index;
	const std::string path = ix::path_of(opt.index);
	st::View store;
	ix::View old;
	bool extend = false;
	std::vector<char> matrices;
	std::vector<long double> norm, rot;
	try {
		openStore(opt.index, 0, "projects", store, nullptr);
		loadPCA(opt, store.h.n_sites, norm, rot);
		matrices = ix::matrix_bytes(norm, rot);
		struct stat sb;
		if (stat(path.c_str(), &sb) == 0) {                   /* an index is there: extend it, or refuse */
			try {
				old.open(path);
				old.check_store(path, store, true);
			} catch (const st::Error &e) {
				throw st::Error(std::string(e.what()) + "; delete " + path + " to index the store anew");
			}
			if (old.h.dim != opt.dim || old.h.min_cov != opt.minCov || old.matrix_size() != matrices.size()
			    || memcmp(old.matrices(), matrices.data(), matrices.size()) != 0)
				throw st::Error(path + " was written with another -d, -c, rotation or centre; delete " + path + " to index the store anew");
			extend = true;
		}
	} catch (const std::exception &e) {
		ntsm::refuse(e.what());
	}
	const uint64_t kept = extend ? old.h.n_samples : 0, added = store.h.n_samples - kept;
	if (added == 0) {
		std::cerr << path << " is up to date: " << kept << " samples" << std::endl;
		return 0;
	}
	std::vector<double> cloud((size_t) added * opt.dim);
	std::vector<uint32_t> geno((size_t) added * 3);
	ntsm_eval_cross_times times {};
	const int rc = ntsm_eval_project_store(opt.device, store.counts(kept), store.h.stride, (uint32_t) added, store.h.n_sites, opt.minCov, norm.data(),
			rot.data(), opt.dim, 0, cloud.data(), geno.data(), &times);
	if (rc) return gpuFail("projecting the store", rc);
	try {
		ix::write(path, store, opt.dim, opt.minCov, matrices, extend ? old.records() : nullptr, kept, cloud.data(), geno.data(), added);
	} catch (const std::exception &e) {
		ntsm::refuse(e.what());
	}
	if (opt.verbose > 0) std::cerr << "Projected " << added << " samples; " << path << " holds " << kept + added << std::endl;
	if (opt.verbose > 1)
		std::cerr << "store index: " << times.chunks << " chunks, upload " << times.upload_ms << " ms, prepare " << times.prepare_kernel_ms
		          << " ms, projection kernel " << times.cross_kernel_ms << " ms, download " << times.download_ms << " ms" << std::endl;
	printTime(t0);
	return 0;
}

/* What --near, --within-near and --between-near open: the store (openStore) and its index, valid, current and written with the
 * run's -c and -d where those are given; -c and -d are then the index's.  Throws the refusal. */
void openIndexOf(const std::string &name, const ntsm::eval_store::View &store, ntsm::eval_index::View &index, Opt &opt)
{
	namespace st = ntsm::eval_store;
	const std::string path = ntsm::eval_index::path_of(name);
	struct stat sb;
	if (stat(path.c_str(), &sb) != 0) throw st::Error("there is no index " + path + ": run --index on the store first");
	index.open(path);
	index.check_store(path, store, false);
	if (opt.minCovGiven && opt.minCov != index.h.min_cov)
		throw st::Error("-c " + std::to_string(opt.minCov) + ", but " + path + " was written with -c " + std::to_string(index.h.min_cov));
	if (opt.dimGiven && opt.dim != index.h.dim)
		throw st::Error("-d " + std::to_string(opt.dim) + ", but " + path + " was written with -d " + std::to_string(index.h.dim));
	opt.minCov = index.h.min_cov;
	opt.dim = index.h.dim;
}

void openIndexedStore(const std::string &name, Counts &c, ntsm::eval_store::View &store, ntsm::eval_index::View &index, Opt &opt)
{
	openStore(name, c.files.size(), "scores", store, &c);
	openIndexOf(name, store, index, opt);
}

/* a store of one sample has no pair */
void refuseOneSample(const ntsm::eval_store::View &store, const std::string &name)
{
	if (store.h.n_samples == 1) throw ntsm::eval_store::Error(name + " holds one sample: nothing to compare");
}

/* the store's samples appended from the index: tallies into the summaries, projections into cloud [n_samples][dim] */
std::vector<double> appendIndexedSamples(Counts &c, std::vector<Genotype> &g, const ntsm::eval_store::View &store, const ntsm::eval_index::View &index,
		const Opt &opt)
{
	std::vector<double> cloud((size_t) store.h.n_samples * opt.dim);
	appendStoreSamples(c, g, store, opt, [&](uint32_t d, Genotype &s) {
		const ntsm::eval_index::Entry e = index.entry(d);
		s.hets = e.hets; s.homs = e.homs; s.miss = e.miss;
		memcpy(&cloud[(size_t) d * opt.dim], e.cloud, sizeof(double) * opt.dim);
	});
	return cloud;
}

/* What differs between the two store searches once the candidates are known. */
struct Route {
	uint32_t nOwners;                        /* samples 0 ... nOwners - 1 may own a dense row: the query files, or every store sample */
	uint32_t col0;                           /* the store's sample d is sample col0 + d of the run: after the queries, or at 0 */
	const void *owners; uint64_t ownerStride; /* owner i's counts [site][2] lie at owners + i * ownerStride bytes */
	std::function<int(const uint32_t *, const uint32_t *, uint64_t, ntsm_eval_record *, ntsm_eval_cross_times *)> scoreList;   /* the list scorer */
};

/* The second half of --near and --within-near.  A sample whose radius is DBL_MAX owns whole rows of the store: the owners'
 * counts go to a dense block that ntsm_eval_cross scores against the whole store (the owner is sample 1; identical records by
 * its contract), so the store is never gathered for them; every other pair goes through the list scorer and its records are
 * scattered back to list order.  Then the rows, the report line (mapMs, projectMs, searchMs: the caller's first half) and
 * the time. */
int routeAndScore(const Counts &c, const std::vector<Genotype> &g, const Opt &opt, const ntsm::eval_store::View &store, const std::vector<double> &radius,
		const Candidates &cand, const Route &route, double mapMs, double projectMs, double searchMs, Clock::time_point t0)
{
	const auto t = Clock::now();
	const uint32_t nd = (uint32_t) store.h.n_samples, m = store.h.n_sites;
	const uint64_t np = cand.pi.size();
	std::vector<uint32_t> dense, denseRow(route.nOwners, UINT32_MAX);
	for (uint32_t i = 0; i < route.nOwners; ++i)
		if (!(radius[i] < DBL_MAX)) { denseRow[i] = (uint32_t) dense.size(); dense.push_back(i); }
	std::vector<ntsm_eval_record> rect((size_t) dense.size() * nd), rec(np);
	ntsm_eval_cross_times crossTimes {}, listTimes {};
	if (!dense.empty()) {
		std::vector<uint32_t> sub(dense.size() * (size_t) m * 2);
		for (size_t r = 0; r < dense.size(); ++r) memcpy(&sub[r * m * 2], (const char *) route.owners + dense[r] * route.ownerStride, sizeof(uint32_t) * m * 2);
		const int rc = ntsm_eval_cross(opt.device, sub.data(), (uint32_t) dense.size(), store.counts(0), store.h.stride, nd, m, opt.minCov, 0, rect.data(), nullptr,
				&crossTimes);
		if (rc) return gpuFail("scoring against the store", rc);
	}
	std::vector<uint32_t> li, lk;
	std::vector<uint64_t> where;
	for (uint64_t p = 0; p < np; ++p) {
		const uint32_t i = cand.pi[p], k = cand.pk[p];
		if (i < route.nOwners && k >= route.col0 && denseRow[i] != UINT32_MAX) rec[p] = rect[(size_t) denseRow[i] * nd + (k - route.col0)];
		else { li.push_back(i); lk.push_back(k); where.push_back(p); }
	}
	std::vector<ntsm_eval_record> listed(li.size());
	const int rc = route.scoreList(li.data(), lk.data(), li.size(), listed.data(), &listTimes);
	if (rc) return gpuFail("scoring the candidate pairs", rc);
	for (size_t x = 0; x < where.size(); ++x) rec[where[x]] = listed[x];
	const double scoreMs = msSince(t);

	const auto tPrint = Clock::now();
	std::cout << kHeader << "\n";
	std::string temp;
	for (uint64_t p = 0; p < np; ++p) printRow(temp, c, g, opt, rec[p], cand.pi[p], cand.pk[p], std::to_string(cand.dist[p]));
	std::cout.flush();
	if (opt.verbose > 1)
		std::cerr << "store search: " << np << " pairs (" << li.size() << " listed, " << dense.size() << " dense rows), map+load " << mapMs << " ms, project "
		          << projectMs << " ms, search " << searchMs << " ms (kernels " << cand.kernelMs << " ms), score " << scoreMs << " ms (gather "
		          << listTimes.upload_ms << " ms, list kernel " << listTimes.cross_kernel_ms << " ms in " << listTimes.chunks << " passes, dense upload "
		          << crossTimes.upload_ms << " ms, dense kernel " << crossTimes.cross_kernel_ms << " ms), print " << msSince(tPrint) << " ms" << std::endl;
	printTime(t0);
	return 0;
}

/* --near STORE FILES...: the rows of computeScorePCA (:285-398) over [FILES..., the store's samples] in which sample 1 or
 * sample 2 is one of FILES, in that run's one-thread order.  The store's projections and tallies come from STORE.pcaidx, the
 * radii are formed here (scorePCA's), and only the counts of the candidates' samples leave the store -- except for a query
 * whose radius is DBL_MAX: it owns a whole row of the store (routeAndScore). */
int searchNear(Counts &c, Opt &opt, Clock::time_point t0)
{
	ntsm::eval_store::View store;
	ntsm::eval_index::View index;
	const auto tMap = Clock::now();
	try {
		openIndexedStore(opt.near, c, store, index, opt);
		if (opt.verbose > 0) std::cerr << "Reading count files" << std::endl;
		load(c, store.index(), true);
	} catch (const std::exception &e) {
		ntsm::refuse(e.what());
	}
	const double mapMs = msSince(tMap);
	std::vector<Genotype> g = summaries(c, opt);
	const uint32_t nq = (uint32_t) c.files.size(), nd = (uint32_t) store.h.n_samples, m = store.h.n_sites, dim = opt.dim;
	if (opt.verbose > 1) std::cerr << "Finished loading files. Now searching " << nq << " samples against the " << nd << " of " << opt.near << "." << std::endl;

	auto t = Clock::now();
	std::vector<double> qCloud;
	{
		std::vector<long double> norm, rot;
		index.matrices(norm, rot);
		Session session;
		int rc = ntsm_eval_open(opt.device, c.counts.data(), nq, m, opt.minCov, &session.h);
		if (rc) return gpuFail("session", rc);
		if ((rc = project(c, opt, session.h, norm, rot, qCloud)) != 0) return rc;
	}
	const double projectMs = msSince(t);

	t = Clock::now();
	const std::vector<double> dbCloud = appendIndexedSamples(c, g, store, index, opt);
	const std::vector<double> radius = searchRadii(g, m, opt);
	if (opt.verbose > 1) std::cerr << "Starting Score Computation with PCA" << std::endl;
	Candidates cand;
	const int rc = cand.search([&](uint32_t *pi, uint32_t *pk, double *dist, uint64_t capacity, uint64_t *np, double *ms) {
		return ntsm_eval_cross_candidates(opt.device, qCloud.data(), radius.data(), nq, dbCloud.data(), radius.data() + nq, nd, dim, pi, pk, dist, capacity, np, ms);
	});
	if (rc) return rc;
	const double searchMs = msSince(t);
	const Route route { nq, nq, c.counts.data(), 8ull * m,
		[&](const uint32_t *li, const uint32_t *lk, uint64_t n, ntsm_eval_record *out, ntsm_eval_cross_times *times) {
			return ntsm_eval_cross_score_pairs(opt.device, c.counts.data(), nq, store.counts(0), store.h.stride, nd, m, opt.minCov, li, lk, n, 0, out, times);
		} };
	return routeAndScore(c, g, opt, store, radius, cand, route, mapMs, projectMs, searchMs, t0);
}

/* one band's times added to a run's */
void addTimes(ntsm_eval_cross_times &sum, const ntsm_eval_cross_times &t)
{
	sum.upload_ms += t.upload_ms; sum.prepare_kernel_ms += t.prepare_kernel_ms; sum.cross_kernel_ms += t.cross_kernel_ms;
	sum.download_ms += t.download_ms; sum.chunks += t.chunks;
}

/* --within STORE: computeScore's rows (:591-624) over the store's samples in store order -- the stdout of the all-to-all run
 * over their files at one thread -- without reading a counts file.  The triangle comes in bands of rows (eval_within.hpp's
 * rule, or --within-rows), printed band by band, which is the reference's order; the first band's call brings every
 * sample's tallies. */
int scoreWithin(const Opt &opt, Clock::time_point t0)
{
	namespace band = ntsm::eval_within;
	ntsm::eval_store::View store;
	Counts c;
	const auto tMap = Clock::now();
	try {
		openStore(opt.within, 0, "scores", store, &c);
		refuseOneSample(store, opt.within);
	} catch (const std::exception &e) {
		ntsm::refuse(e.what());
	}
	const double mapMs = msSince(tMap);
	const uint32_t n = (uint32_t) store.h.n_samples, m = store.h.n_sites;
	if (opt.verbose > 1) std::cerr << "Mapped " << opt.within << ". Now comparing its " << n << " samples." << std::endl;
	std::cerr << "Performing all-to-all score computation.\nSpecify -p (--pca) to enable faster comparisons." << std::endl;
	WithinSession session;
	int rc = ntsm_eval_within_open(opt.device, store.counts(0), store.h.stride, n, m, opt.minCov, 0, &session.h);
	if (rc) return gpuFail("opening the store", rc);
	std::vector<uint32_t> geno((size_t) n * 3);
	std::vector<Genotype> g;
	std::vector<ntsm_eval_record> rec;
	ntsm_eval_cross_times sum {};
	uint32_t bands = 0;
	double printMs = 0;
	std::string temp;
	for (uint32_t first = 0; first < n; ++bands) {
		const uint32_t rows = opt.withinRows ? std::min(opt.withinRows, n - first) : band::band_rows(first, n, band::kBandRecords);
		rec.resize(band::band_records(first, rows, n));
		ntsm_eval_cross_times times {};
		rc = ntsm_eval_within_rows(session.h, first, rows, rec.data(), first == 0 ? geno.data() : nullptr, &times);
		if (rc) return gpuFail("scoring the store", rc);
		addTimes(sum, times);
		const auto tPrint = Clock::now();
		if (first == 0) {
			appendStoreSamples(c, g, store, opt, [&](uint32_t d, Genotype &s) { s.hets = geno[3 * d]; s.homs = geno[3 * d + 1]; s.miss = geno[3 * d + 2]; });
			std::cout << kHeader << "\n";
		}
		for (uint32_t i = first; i < first + rows; ++i)
			for (uint32_t j = i + 1; j < n; ++j) printRow(temp, c, g, opt, rec[band::band_offset(i, j, first, n)], i, j, "-1");
		printMs += msSince(tPrint);
		first += rows;
	}
	std::cout.flush();
	if (opt.verbose > 1)
		std::cerr << "store within: " << (sum.chunks ? "streamed" : "resident") << ", " << bands << " bands, " << sum.chunks << " chunks, map " << mapMs
		          << " ms, upload " << sum.upload_ms << " ms, prepare " << sum.prepare_kernel_ms << " ms, pair kernel " << sum.cross_kernel_ms
		          << " ms, download " << sum.download_ms << " ms, print " << printMs << " ms" << std::endl;
	printTime(t0);
	return 0;
}

/* --within-near STORE: computeScorePCA's rows (:285-398) over the store's samples -- the stdout of the -p run over their
 * files with the index's rotation, centre, -d and -c.  Projections and tallies come from STORE.pcaidx and the radii are formed
 * here, so the search is ntsm_eval_cross_candidates with every sample a query and no database side: by its contract
 * ntsm_eval_candidates' list.  Any sample may own whole rows (routeAndScore); the other pairs are pairs of two store samples. */
int searchWithin(Opt &opt, Clock::time_point t0)
{
	ntsm::eval_store::View store;
	ntsm::eval_index::View index;
	Counts c;
	const auto tMap = Clock::now();
	try {
		openIndexedStore(opt.withinNear, c, store, index, opt);
		refuseOneSample(store, opt.withinNear);
	} catch (const std::exception &e) {
		ntsm::refuse(e.what());
	}
	const double mapMs = msSince(tMap);
	const uint32_t n = (uint32_t) store.h.n_samples, m = store.h.n_sites, dim = opt.dim;
	if (opt.verbose > 1) std::cerr << "Mapped " << opt.withinNear << " and its index. Now searching its " << n << " samples." << std::endl;

	const auto t = Clock::now();
	std::vector<Genotype> g;
	const std::vector<double> cloud = appendIndexedSamples(c, g, store, index, opt);
	const std::vector<double> radius = searchRadii(g, m, opt);
	if (opt.verbose > 1) std::cerr << "Starting Score Computation with PCA" << std::endl;
	Candidates cand;
	const int rc = cand.search([&](uint32_t *pi, uint32_t *pk, double *dist, uint64_t capacity, uint64_t *np, double *ms) {
		return ntsm_eval_cross_candidates(opt.device, cloud.data(), radius.data(), n, nullptr, nullptr, 0, dim, pi, pk, dist, capacity, np, ms);
	});
	if (rc) return rc;
	const double searchMs = msSince(t);
	const Route route { n, 0, store.counts(0), store.h.stride,
		[&](const uint32_t *li, const uint32_t *lk, uint64_t np, ntsm_eval_record *out, ntsm_eval_cross_times *times) {
			return ntsm_eval_store_score_pairs(opt.device, store.counts(0), store.h.stride, n, m, opt.minCov, li, lk, np, 0, out, times);
		} };
	return routeAndScore(c, g, opt, store, radius, cand, route, mapMs, 0.0, searchMs, t0);
}

/* --between STORE_A STORE_B: computeScore's rows (:591-624) over [A's samples, B's samples] whose sample 1 is of A and whose
 * sample 2 is of B, in that run's order, without reading a counts file.  A's locus table and distinct columns play the first
 * file's part and B's samples are later files of that run: their loci are matched to A's by ID (eval_between.hpp), on the
 * device.  The rectangle comes in bands of rows of A (that header's rule, or --between-rows), printed band by band; a band's
 * call brings the tallies of its rows and the first one those of B's samples, taken over A's sites. */
int scoreBetween(const Opt &opt, const std::string &storeB, Clock::time_point t0)
{
	namespace band = ntsm::eval_between;
	ntsm::eval_store::View a, b;
	band::LocusMap map;
	Counts c;
	const auto tMap = Clock::now();
	try {
		openStore(opt.between, 0, "scores", a, &c);
		openStore(storeB, a.h.n_samples, "scores", b, nullptr);
		map = band::map_loci(a, b, opt.between, storeB);
	} catch (const std::exception &e) {
		ntsm::refuse(e.what());
	}
	const double mapMs = msSince(tMap);
	const uint32_t na = (uint32_t) a.h.n_samples, nb = (uint32_t) b.h.n_samples;
	if (opt.verbose > 1) std::cerr << "Mapped " << opt.between << " and " << storeB << ". Now comparing " << na << " samples against " << nb << "." << std::endl;
	std::cerr << "Performing all-to-all score computation.\nSpecify -p (--pca) to enable faster comparisons." << std::endl;
	BetweenSession session;
	int rc = ntsm_eval_between_open(opt.device, a.counts(0), a.h.stride, na, b.counts(0), b.h.stride, nb, a.h.n_sites, b.h.n_sites, map.data(), opt.minCov, 0,
			&session.h);
	if (rc) return gpuFail("opening the stores", rc);
	std::vector<Genotype> g;
	appendStoreSamples(c, g, a, opt, [](uint32_t, Genotype &) {});                /* A's tallies come with their bands */
	std::vector<uint32_t> genoA, genoB((size_t) nb * 3);
	std::vector<ntsm_eval_record> rec;
	ntsm_eval_cross_times sum {};
	uint32_t bands = 0;
	double printMs = 0;
	std::string temp;
	for (uint32_t first = 0; first < na; ++bands) {
		const uint32_t rows = opt.betweenRows ? std::min(opt.betweenRows, na - first) : band::band_rows(first, na, nb, band::kBandRecords);
		rec.resize((size_t) rows * nb);
		genoA.resize((size_t) rows * 3);
		ntsm_eval_cross_times times {};
		rc = ntsm_eval_between_rows(session.h, first, rows, rec.data(), genoA.data(), first == 0 ? genoB.data() : nullptr, &times);
		if (rc) return gpuFail("scoring the stores", rc);
		addTimes(sum, times);
		const auto tPrint = Clock::now();
		if (first == 0) {
			appendStoreSamples(c, g, b, opt, [&](uint32_t d, Genotype &s) { s.hets = genoB[3 * d]; s.homs = genoB[3 * d + 1]; s.miss = genoB[3 * d + 2]; });
			std::cout << kHeader << "\n";
		}
		for (uint32_t r = 0; r < rows; ++r) {
			Genotype &s = g[first + r];
			s.hets = genoA[3 * r]; s.homs = genoA[3 * r + 1]; s.miss = genoA[3 * r + 2];
			for (uint32_t d = 0; d < nb; ++d) printRow(temp, c, g, opt, rec[(size_t) r * nb + d], first + r, na + d, "-1");
		}
		printMs += msSince(tPrint);
		first += rows;
	}
	std::cout.flush();
	if (opt.verbose > 1)
		std::cerr << "store between: loci " << (map.identical ? "identical" : "mapped") << " (" << map.lacking << " of " << a.h.n_sites << " absent from " << storeB
		          << "), B " << (sum.chunks ? "streamed" : "resident") << ", " << bands << " bands, " << sum.chunks << " chunks, map " << mapMs << " ms, upload "
		          << sum.upload_ms << " ms, prepare " << sum.prepare_kernel_ms << " ms, pair kernel " << sum.cross_kernel_ms << " ms, download " << sum.download_ms
		          << " ms, print " << printMs << " ms" << std::endl;
	printTime(t0);
	return 0;
}

/* --between-near STORE_A STORE_B: computeScorePCA's rows (:285-398) over [A's samples, B's samples] that pair a sample of one
 * store with a sample of the other, in that run's one-thread order, with the rotation, centre, -d and -c of A's index.  A's
 * locus table and distinct columns play the first file's part, as in --between.  A's projections and tallies come from its
 * index; B's from B's index where eval_between.hpp's rule says it serves, else from ntsm_eval_project_store_mapped, and
 * nothing is written.  A sample of A whose radius is DBL_MAX owns its whole row of B: runs of such rows go through
 * --between's session (identical records by its contract; B is never gathered for them); every other pair -- those owned by
 * a search-all sample of B among them, as (b, a) -- goes through ntsm_eval_between_score_pairs. */
int searchBetween(Opt &opt, const std::string &storeB, Clock::time_point t0)
{
	namespace st = ntsm::eval_store;
	namespace ix = ntsm::eval_index;
	namespace band = ntsm::eval_between;
	st::View a, b;
	ix::View indexA, indexB;
	band::LocusMap map;
	band::BIndexFacts facts;
	Counts c;
	const auto tMap = Clock::now();
	try {
		openStore(opt.betweenNear, 0, "scores", a, &c);
		openStore(storeB, a.h.n_samples, "scores", b, nullptr);
		map = band::map_loci(a, b, opt.betweenNear, storeB);
		try {
			openIndexOf(opt.betweenNear, a, indexA, opt);
		} catch (const st::Error &e) {                       /* absent, invalid, stale, or another -c / -d */
			throw st::Error(std::string(e.what()) + " (--between-near searches through the index of store A: --index " + opt.betweenNear + " -p ROT -n NORM)");
		}
		const std::string pathB = ix::path_of(storeB);
		struct stat sb;
		facts.exists = stat(pathB.c_str(), &sb) == 0;
		if (facts.exists)
			try {
				indexB.open(pathB);
				facts.valid = true;
				indexB.check_store(pathB, b, false);
				facts.current = true;
			} catch (const st::Error &) {                    /* B is projected in the run instead */
			}
		facts.identical_loci = map.identical;
		facts.dim_a = indexA.h.dim; facts.min_cov_a = indexA.h.min_cov; facts.matrices_a = indexA.matrices(); facts.matrix_size_a = indexA.matrix_size();
		if (facts.valid) { facts.dim_b = indexB.h.dim; facts.min_cov_b = indexB.h.min_cov; facts.matrices_b = indexB.matrices(); facts.matrix_size_b = indexB.matrix_size(); }
	} catch (const std::exception &e) {
		ntsm::refuse(e.what());
	}
	const bool fromIndex = band::b_index_usable(facts);
	const double mapMs = msSince(tMap);
	const uint32_t na = (uint32_t) a.h.n_samples, nb = (uint32_t) b.h.n_samples, m = a.h.n_sites, dim = opt.dim;
	if (opt.verbose > 1)
		std::cerr << "Mapped " << opt.betweenNear << ", its index and " << storeB << ". Now searching " << na << " samples against " << nb << "." << std::endl;

	auto t = Clock::now();
	std::vector<Genotype> g;
	const std::vector<double> cloudA = appendIndexedSamples(c, g, a, indexA, opt);
	std::vector<double> cloudB;
	if (fromIndex) cloudB = appendIndexedSamples(c, g, b, indexB, opt);
	else {
		std::vector<long double> norm, rot;
		indexA.matrices(norm, rot);
		cloudB.assign((size_t) nb * dim, 0.0);
		std::vector<uint32_t> geno((size_t) nb * 3);
		const int rc = ntsm_eval_project_store_mapped(opt.device, b.counts(0), b.h.stride, nb, m, b.h.n_sites, map.data(), opt.minCov, norm.data(), rot.data(), dim, 0,
				cloudB.data(), geno.data(), nullptr);
		if (rc) return gpuFail("projecting the second store", rc);
		appendStoreSamples(c, g, b, opt, [&](uint32_t d, Genotype &s) { s.hets = geno[3 * d]; s.homs = geno[3 * d + 1]; s.miss = geno[3 * d + 2]; });
	}
	const double projectMs = msSince(t);

	t = Clock::now();
	const std::vector<double> radius = searchRadii(g, m, opt);
	if (opt.verbose > 1) std::cerr << "Starting Score Computation with PCA" << std::endl;
	Candidates cand;
	int rc = cand.search([&](uint32_t *pi, uint32_t *pk, double *dist, uint64_t capacity, uint64_t *np, double *ms) {
		return ntsm_eval_between_candidates(opt.device, cloudA.data(), radius.data(), na, cloudB.data(), radius.data() + na, nb, dim, pi, pk, dist, capacity, np, ms);
	});
	if (rc) return rc;
	const double searchMs = msSince(t);

	t = Clock::now();
	const uint64_t np = cand.pi.size();
	const std::vector<std::pair<uint32_t, uint32_t>> runs = band::dense_runs(radius.data(), na, DBL_MAX);
	std::vector<uint32_t> denseRow(na, UINT32_MAX);
	uint32_t nDense = 0;
	for (const auto &run : runs)
		for (uint32_t r = 0; r < run.second; ++r) denseRow[run.first + r] = nDense++;
	std::vector<ntsm_eval_record> rect((size_t) nDense * nb), rec(np);
	if (nDense) {
		BetweenSession session;
		rc = ntsm_eval_between_open(opt.device, a.counts(0), a.h.stride, na, b.counts(0), b.h.stride, nb, m, b.h.n_sites, map.data(), opt.minCov, 0, &session.h);
		if (rc) return gpuFail("opening the stores", rc);
		for (const auto &run : runs)
			for (uint32_t first = run.first, end = run.first + run.second; first < end;) {
				const uint32_t rows = band::band_rows(first, end, nb, band::kBandRecords);
				rc = ntsm_eval_between_rows(session.h, first, rows, rect.data() + (size_t) denseRow[first] * nb, nullptr, nullptr, nullptr);
				if (rc) return gpuFail("scoring the stores", rc);
				first += rows;
			}
	}
	std::vector<uint32_t> li, lk;
	std::vector<uint64_t> where;
	for (uint64_t p = 0; p < np; ++p) {
		const uint32_t i = cand.pi[p], k = cand.pk[p];
		if (i < na && denseRow[i] != UINT32_MAX) rec[p] = rect[(size_t) denseRow[i] * nb + (k - na)];
		else { li.push_back(i); lk.push_back(k); where.push_back(p); }
	}
	std::vector<ntsm_eval_record> listed(li.size());
	ntsm_eval_cross_times listTimes {};
	rc = ntsm_eval_between_score_pairs(opt.device, a.counts(0), a.h.stride, na, b.counts(0), b.h.stride, nb, m, b.h.n_sites, map.data(), opt.minCov, li.data(),
			lk.data(), li.size(), 0, listed.data(), &listTimes);
	if (rc) return gpuFail("scoring the candidate pairs", rc);
	for (size_t x = 0; x < where.size(); ++x) rec[where[x]] = listed[x];
	const double scoreMs = msSince(t);

	const auto tPrint = Clock::now();
	std::cout << kHeader << "\n";
	std::string temp;
	for (uint64_t p = 0; p < np; ++p) printRow(temp, c, g, opt, rec[p], cand.pi[p], cand.pk[p], std::to_string(cand.dist[p]));
	std::cout.flush();
	if (opt.verbose > 1)
		std::cerr << "store between-near: loci " << (map.identical ? "identical" : "mapped") << " (" << map.lacking << " of " << m << " absent from " << storeB
		          << "), B's projections " << (fromIndex ? "from index" : "projected") << ", " << np << " candidates (" << li.size() << " listed pairs in "
		          << listTimes.chunks << " passes, " << nDense << " dense rows of A in " << runs.size() << " runs), map " << mapMs << " ms, project " << projectMs
		          << " ms, search " << searchMs << " ms (kernels " << cand.kernelMs << " ms), score " << scoreMs << " ms (gather " << listTimes.upload_ms
		          << " ms, remap+terms " << listTimes.prepare_kernel_ms << " ms, list kernel " << listTimes.cross_kernel_ms << " ms), print " << msSince(tPrint)
		          << " ms" << std::endl;
	printTime(t0);
	return 0;
}

/* --sites-out FILE (and --samples-out FILE of --contam), opened before any GPU work and without touching what it holds: a file this run made is removed again
 * unless the table gets written */
struct SitesFile {
	std::string path;
	int fd = -1;
	bool created = false, written = false;
	~SitesFile()
	{
		if (fd >= 0) close(fd);
		if (created && !written) unlink(path.c_str());
	}
	bool open(const std::string &name)
	{
		path = name;
		struct stat sb;
		created = stat(name.c_str(), &sb) != 0;
		fd = ::open(name.c_str(), O_WRONLY | O_CREAT, 0644);
		return fd >= 0;
	}
	bool write(const std::string &text)
	{
		written = ftruncate(fd, 0) == 0 && ntsm::eval_store::write_all(fd, text.data(), text.size(), 0);
		return written;
	}
};

/* --qc STORE [-p ROT -n NORM] [--sites-out FILE]: computeScoreSingle (:541-585) with one row per sample of the store -- the row
 * the single-file run prints for a counts file whose loci and distinct columns are the store's --, each followed by "\n".  The
 * tallies of the samples and, for --sites-out, of the sites come from one pass over the store (ntsm_eval_store_profile); the
 * PC columns from ntsm_eval_project_store in the same run, STORE.pcaidx neither read nor written. */
int qcStore(const Opt &opt, Clock::time_point t0)
{
	ntsm::eval_store::View store;
	Counts c;
	std::vector<long double> norm, rot;
	SitesFile sites;
	const auto tMap = Clock::now();
	try {
		openStore(opt.qc, 0, "scores", store, &c);
		if (!opt.pca.empty()) loadPCA(opt, store.h.n_sites, norm, rot);
		if (opt.sitesOutGiven && !sites.open(opt.sitesOut)) throw ntsm::eval_store::Error("cannot write " + opt.sitesOut);
	} catch (const std::exception &e) {
		ntsm::refuse(e.what());
	}
	const double mapMs = msSince(tMap);
	const uint32_t n = (uint32_t) store.h.n_samples, m = store.h.n_sites;
	if (opt.verbose > 1) std::cerr << "Mapped " << opt.qc << ". Providing only QC information for its " << n << " samples." << std::endl;
	std::vector<uint32_t> geno((size_t) n * 3), tally(opt.sitesOutGiven ? (size_t) m * 4 : 0);
	std::vector<uint64_t> siteCov(opt.sitesOutGiven ? m : 0);
	ntsm_eval_cross_times times {}, projectTimes {};
	int rc = ntsm_eval_store_profile(opt.device, store.counts(0), store.h.stride, n, m, opt.minCov, 0, geno.data(), opt.sitesOutGiven ? tally.data() : nullptr,
			opt.sitesOutGiven ? siteCov.data() : nullptr, &times);
	if (rc) return gpuFail("profiling the store", rc);
	std::vector<double> cloud;
	if (!opt.pca.empty()) {
		cloud.assign((size_t) n * opt.dim, 0.0);
		rc = ntsm_eval_project_store(opt.device, store.counts(0), store.h.stride, n, m, opt.minCov, norm.data(), rot.data(), opt.dim, 0, cloud.data(), nullptr,
				&projectTimes);
		if (rc) return gpuFail("projecting the store", rc);
	}
	const auto tPrint = Clock::now();
	std::vector<Genotype> g;
	appendStoreSamples(c, g, store, opt, [&](uint32_t d, Genotype &s) { s.hets = geno[3 * d]; s.homs = geno[3 * d + 1]; s.miss = geno[3 * d + 2]; });
	std::string temp = "sample\tcov\terrorRate\tmiss\thom\thet";
	if (!opt.pca.empty())
		for (unsigned d = 1; d <= opt.dim; ++d) { temp += "\tPC"; temp += std::to_string(d); }
	std::cout << temp << std::endl;
	for (uint32_t i = 0; i < n; ++i) {
		temp.clear();
		temp += c.files[i]; temp += "\t"; temp += std::to_string(g[i].cov); temp += "\t"; temp += std::to_string(g[i].errorRate);
		temp += "\t"; temp += std::to_string(g[i].miss); temp += "\t"; temp += std::to_string(g[i].homs); temp += "\t"; temp += std::to_string(g[i].hets);
		for (unsigned d = 0; d < (opt.pca.empty() ? 0 : opt.dim); ++d) { temp += "\t"; temp += std::to_string(cloud[(size_t) i * opt.dim + d]); }
		temp += "\n";
		std::cout << temp;
	}
	std::cout.flush();
	if (opt.sitesOutGiven) {
		std::string text = ntsm::eval_qc::kSiteHeader;
		for (uint32_t s = 0; s < m; ++s) ntsm::eval_qc::site_line(text, c.locus[s].c_str(), &tally[(size_t) s * 4], siteCov[s], n);
		if (!sites.write(text)) { std::cerr << PROGRAM ": cannot write " << opt.sitesOut << std::endl; return 1; }
	}
	if (opt.verbose > 1)
		std::cerr << "store qc: " << times.chunks << " chunks, map+load " << mapMs << " ms, upload " << times.upload_ms << " ms, profile kernel " << times.cross_kernel_ms
		          << " ms, download " << times.download_ms << " ms, project " << projectTimes.upload_ms + projectTimes.prepare_kernel_ms + projectTimes.cross_kernel_ms
		             + projectTimes.download_ms << " ms (upload " << projectTimes.upload_ms << " ms, projection kernel " << projectTimes.cross_kernel_ms
		          << " ms), print " << msSince(tPrint) << " ms" << std::endl;
	printTime(t0);
	return 0;
}

/* --contam STORE [-c N] [--contam-depth D] [--contam-min X] [--contam-explained Y] [-a] [--contam-rows N] [--samples-out FILE]:
 * is a sample of the store a mixture, and of which other sample.  The rectangle of ordered pairs
 * (target, source) comes in bands of targets (eval_contam.hpp's rule, or --contam-rows), printed band by band, each band's call
 * bringing its targets' tallies; the rates, the filter and the text are that header's. */
int contamStore(const Opt &opt, Clock::time_point t0)
{
	namespace ct = ntsm::eval_contam;
	ntsm::eval_store::View store;
	SitesFile samples;
	const auto tMap = Clock::now();
	try {
		openStore(opt.contam, 0, "scores", store, nullptr);
		if (opt.samplesOutGiven && !samples.open(opt.samplesOut)) throw ntsm::eval_store::Error("cannot write " + opt.samplesOut);
	} catch (const std::exception &e) {
		ntsm::refuse(e.what());
	}
	const double mapMs = msSince(tMap);
	const uint32_t n = (uint32_t) store.h.n_samples, m = store.h.n_sites;
	if (opt.verbose > 1) std::cerr << "Mapped " << opt.contam << ". Now checking its " << n << " samples against each other." << std::endl;
	ContamSession session;
	int rc = ntsm_eval_contam_open(opt.device, store.counts(0), store.h.stride, n, m, opt.minCov, opt.contamDepth, 0, &session.h);
	if (rc) return gpuFail("opening the store", rc);
	std::vector<std::string> nameOf(n);
	std::vector<const char *> names(n);
	for (uint32_t d = 0; d < n; ++d) { nameOf[d] = store.name(d); names[d] = nameOf[d].c_str(); }
	std::vector<ntsm_eval_contam_record> rec;
	std::vector<uint64_t> tally((size_t) n * 3);
	ntsm_eval_cross_times sum {};
	uint32_t bands = 0;
	double printMs = 0;
	std::string temp;
	for (uint32_t first = 0; first < n; ++bands) {
		const uint32_t rows = opt.contamRows ? std::min(opt.contamRows, n - first) : ct::band_rows(first, n, ct::kBandRecords);
		rec.resize((size_t) rows * n);
		ntsm_eval_cross_times times {};
		rc = ntsm_eval_contam_rows(session.h, first, rows, rec.data(), tally.data() + (size_t) first * 3, &times);
		if (rc) return gpuFail("checking the store", rc);
		addTimes(sum, times);
		const auto tPrint = Clock::now();
		if (first == 0) std::cout << ct::kHeader;
		temp.clear();
		ct::band_text(temp, names.data(), n, first, rows, rec.data(), tally.data() + (size_t) first * 3, opt.all, opt.contamMin, opt.contamExplained);
		std::cout << temp;
		printMs += msSince(tPrint);
		first += rows;
	}
	std::cout.flush();
	if (opt.samplesOutGiven) {
		std::string text = ct::kSampleHeader;
		for (uint32_t i = 0; i < n; ++i) ct::sample_line(text, names[i], &tally[(size_t) i * 3]);
		if (!samples.write(text)) { std::cerr << PROGRAM ": cannot write " << opt.samplesOut << std::endl; return 1; }
	}
	if (opt.verbose > 1)
		std::cerr << "store contam: " << (sum.chunks ? "streamed" : "resident") << ", " << bands << " bands, " << sum.chunks << " chunks, map " << mapMs
		          << " ms, upload " << sum.upload_ms << " ms, prepare " << sum.prepare_kernel_ms << " ms, rectangle kernel " << sum.cross_kernel_ms
		          << " ms, download " << sum.download_ms << " ms, print " << printMs << " ms" << std::endl;
	printTime(t0);
	return 0;
}

/* --trios STORE [-c N] [--trio-depth D] [--trio-max X] [--trio-duo Y] [--trio-called M] [--trio-exhaustive] [-a] [--ped FILE]:
 * which samples of the store form a parent-parent-child trio, or whether a pedigree's trios hold.  The
 * runs, their rules and the text are eval_trio.hpp's; this opens the store and the session and hands it the library's two entry
 * points.  Every refusal -- the store, the pedigree, its IDs -- comes before the session is opened. */
int trioStore(const Opt &opt, Clock::time_point t0)
{
	namespace tr = ntsm::eval_trio;
	ntsm::eval_store::View store;
	std::vector<std::string> nameOf;
	std::vector<tr::PedTrio> pedTrios;
	tr::Ped ped;
	const auto tMap = Clock::now();
	try {
		openStore(opt.trios, 0, "scores", store, nullptr);
		if (store.h.n_samples < 3) throw tr::Error(opt.trios + " holds fewer than 3 samples: there is no trio to look for");
		nameOf.resize(store.h.n_samples);
		for (uint32_t d = 0; d < nameOf.size(); ++d) nameOf[d] = store.name(d);
		if (opt.pedGiven) {
			std::ifstream fh(opt.ped);
			struct stat sb;
			if (!fh.good() || stat(opt.ped.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) throw tr::Error("cannot read the pedigree file " + opt.ped);
			std::stringstream text;
			text << fh.rdbuf();
			ped = tr::parse_ped(text.str());
			pedTrios = tr::resolve(ped, nameOf);
		}
	} catch (const std::exception &e) {
		ntsm::refuse(e.what());
	}
	const double mapMs = msSince(tMap);
	const uint32_t n = (uint32_t) store.h.n_samples, m = store.h.n_sites;
	if (opt.verbose > 0 && opt.pedGiven)
		std::cerr << "Read " << pedTrios.size() << " trios from " << opt.ped << "; skipped " << ped.comments << " comment lines and " << ped.founders
		          << " lines without both parents" << std::endl;
	if (opt.verbose > 1) std::cerr << "Mapped " << opt.trios << ". Now looking for trios among its " << n << " samples." << std::endl;
	TrioSession session;
	ntsm_eval_cross_times open {};
	int rc = ntsm_eval_trio_open(opt.device, store.counts(0), store.h.stride, n, m, opt.minCov, opt.trioDepth, 0, nullptr, &open, &session.h);
	if (rc) return gpuFail("opening the store", rc);
	double duoMs = 0, scoreMs = 0, duoCallMs = 0, scoreCallMs = 0, printMs = 0;
	tr::Device dev;
	dev.duos = [&](uint32_t first, uint32_t rows, ntsm_eval_trio_duo *out) {
		const auto t = Clock::now();
		double ms = 0;
		const int r = ntsm_eval_trio_duos(session.h, first, rows, out, &ms);
		duoMs += ms; duoCallMs += msSince(t);
		return r;
	};
	dev.score = [&](const uint32_t *child, const uint64_t *offset, const uint32_t *cand, uint32_t count, ntsm_eval_trio_record *out) {
		const auto t = Clock::now();
		double ms = 0;
		const int r = ntsm_eval_trio_score(session.h, child, offset, cand, count, out, &ms);
		scoreMs += ms; scoreCallMs += msSince(t);
		return r;
	};
	const tr::Sink sink = [&](const std::string &text) { const auto t = Clock::now(); std::cout << text; printMs += msSince(t); };
	tr::Cuts cuts;
	cuts.min_called = opt.trioCalled; cuts.max_rate = opt.trioMax; cuts.max_duo = opt.trioDuo; cuts.all = opt.all; cuts.exhaustive = opt.trioExhaustive;
	tr::Stats st;
	try {
		rc = opt.pedGiven ? tr::pedigree(dev, nameOf, pedTrios, cuts, sink, st) : tr::search(dev, nameOf, cuts, sink, st);
	} catch (const tr::Error &e) {
		ntsm::refuse(e.what());
	}
	if (rc) return gpuFail("looking for trios", rc);
	std::cout.flush();
	if (opt.verbose > 1)
		std::cerr << "store trios: planes " << 3ull * ((m + 63ull) / 64) * 8 * n << " bytes, " << open.chunks << " chunks, " << st.bands << " duo bands, "
		          << st.children << " children with 2 or more candidates, " << st.triples << " triples, " << st.rows << " rows, map " << mapMs << " ms, upload "
		          << open.upload_ms << " ms, plane kernel " << open.prepare_kernel_ms << " ms, duo " << duoCallMs << " ms (kernel " << duoMs << " ms), score "
		          << scoreCallMs << " ms (kernel " << scoreMs << " ms), print " << printMs << " ms" << std::endl;
	printTime(t0);
	return 0;
}

/* --ld STORE [-c N] [--ld-depth D] [--ld-min T] [--ld-called M] [--ld-prune FILE] [-a]: which pairs of sites of the store are
 * in linkage disequilibrium, and which sites a prune keeps.  The band walk, the text and the prune are
 * eval_ld.hpp's; this opens the store and the session and hands the walk the library's selection.  Every refusal comes before the
 * session is opened.  NTSM_LD_PAIR_BUDGET (tests): the pairs of one call, in place of 1 GiB of them. */
int ldStore(const Opt &opt, Clock::time_point t0)
{
	namespace ld = ntsm::eval_ld;
	ntsm::eval_store::View store;
	SitesFile prunedFile;
	const auto tMap = Clock::now();
	try {
		openStore(opt.ld, 0, "scores", store, nullptr);
		if (store.h.n_samples < 2) throw ld::Error(opt.ld + " holds fewer than 2 samples: no site varies among them");
		if (store.h.n_samples > NTSM_EVAL_LD_MAX_SAMPLES) throw ld::Error(opt.ld + " holds more than 16777216 samples: the moments of --ld are exact up to there");
		if (store.h.n_sites < 2) throw ld::Error(opt.ld + " holds fewer than 2 sites: there is no pair of sites");
		if (opt.ldPruneGiven && !prunedFile.open(opt.ldPrune)) throw ld::Error("cannot write " + opt.ldPrune);
	} catch (const std::exception &e) {
		ntsm::refuse(e.what());
	}
	const double mapMs = msSince(tMap);
	const uint32_t n = (uint32_t) store.h.n_samples, m = store.h.n_sites;
	uint64_t budget = ld::kPairBudget;
	if (const char *b = getenv("NTSM_LD_PAIR_BUDGET")) budget = strtoull(b, nullptr, 10);
	if (opt.verbose > 1) std::cerr << "Mapped " << opt.ld << ". Now comparing its " << m << " sites over " << n << " samples." << std::endl;
	LdSession session;
	ntsm_eval_cross_times open {};
	int rc = ntsm_eval_ld_open(opt.device, store.counts(0), store.h.stride, n, m, opt.minCov, opt.ldDepth, 0, nullptr, &open, &session.h);
	if (rc) return gpuFail("opening the store", rc);
	std::vector<const char *> locus(m);
	for (uint32_t s = 0; s < m; ++s) locus[s] = store.locus[s].c_str();
	double kernelMs = 0, callMs = 0, printMs = 0;
	const double cut = opt.all ? 0.0 : opt.ldMin;                                  /* r2 >= 0 wherever it is defined */
	ld::Device dev;
	dev.select = [&](uint32_t first, uint32_t rows, uint64_t cap, ntsm_eval_ld_pair *out, uint64_t *found) {
		const auto t = Clock::now();
		double ms = 0;
		const int r = ntsm_eval_ld_select(session.h, first, rows, opt.ldCalled, cut, cap, out, found, &ms);
		kernelMs += ms; callMs += msSince(t);
		return r;
	};
	ld::Prune prune(m);
	bool headed = false;
	std::string text;
	ld::Stats st;
	rc = ld::walk(dev, m, budget, [&](const ntsm_eval_ld_pair *pairs, uint64_t count) {
		const auto t = Clock::now();
		text.clear();
		if (!headed) { text = ld::kHeader; headed = true; }
		ld::rows_text(text, locus.data(), pairs, count);
		std::cout << text;
		if (opt.ldPruneGiven) prune.add(pairs, count, opt.ldCalled, opt.ldMin);
		printMs += msSince(t);
	}, st);
	if (rc) return gpuFail("comparing the sites", rc);
	std::cout.flush();
	if (opt.ldPruneGiven && !prunedFile.write(prune.text(locus.data()))) { std::cerr << PROGRAM ": cannot write " << opt.ldPrune << std::endl; return 1; }
	if (opt.verbose > 1) {
		std::cerr << "store ld: planes " << 3ull * ((n + 63ull) / 64) * 8 * m << " bytes, " << open.chunks << " chunks, " << st.bands << " bands, " << st.reruns
		          << " re-runs, " << st.pairs << " pairs";
		if (opt.ldPruneGiven) std::cerr << ", " << prune.n_kept() << " kept sites";
		std::cerr << ", map " << mapMs << " ms, upload " << open.upload_ms << " ms, plane kernel " << open.prepare_kernel_ms << " ms, select " << callMs
		          << " ms (kernel " << kernelMs << " ms), print " << printMs << " ms" << std::endl;
	}
	printTime(t0);
	return 0;
}

/* what no store run goes with */
void refuseDebugAndMerge(const Opt &opt, const char *mode)
{
	if (!opt.debug.empty()) ntsm::refuse(std::string("-b with ") + mode + " is not part of this build");
	if (!opt.merge.empty() || opt.onlyMerge) ntsm::refuse(std::string("merging (-e, -o) with ") + mode + " is not part of this build: the store does not hold the per-site sums");
}

}  // namespace

int main(int argc, char **argv)
{
	Opt opt;
	bool die = false, storeMode = false, nearMode = false, withinMode = false, betweenMode = false, betweenNearMode = false, qcMode = false, contamMode = false, trioMode = false, ldMode = false;
	static struct option long_options[] = {
		{ "score_thresh", required_argument, nullptr, 's' }, { "all", no_argument, nullptr, 'a' },
		{ "min_cov", required_argument, nullptr, 'c' }, { "skew", required_argument, nullptr, 'w' },
		{ "genome_size", required_argument, nullptr, 'g' }, { "threads", required_argument, nullptr, 't' },
		{ "merge", required_argument, nullptr, 'e' }, { "only_merge", required_argument, nullptr, 'o' },
		{ "help", no_argument, nullptr, 'h' }, { "pca", required_argument, nullptr, 'p' }, { "norm", required_argument, nullptr, 'n' },
		{ "error_rate", required_argument, nullptr, 'r' }, { "miss_small", required_argument, nullptr, '1' },
		{ "miss_large", required_argument, nullptr, '2' }, { "small", required_argument, nullptr, 'k' },   /* 'k': as in the reference's table, no effect */
		{ "large", required_argument, nullptr, 'l' }, { "debug", required_argument, nullptr, 'b' },
		{ "gpu", required_argument, nullptr, 'G' }, { "verbose", no_argument, nullptr, 'v' },
		{ "pack", required_argument, nullptr, kOptPack }, { "against", required_argument, nullptr, kOptAgainst },
		{ "index", required_argument, nullptr, kOptIndex }, { "near", required_argument, nullptr, kOptNear },
		{ "within", required_argument, nullptr, kOptWithin }, { "within-near", required_argument, nullptr, kOptWithinNear },
		{ "within-rows", required_argument, nullptr, kOptWithinRows }, { "between", required_argument, nullptr, kOptBetween },
		{ "between-rows", required_argument, nullptr, kOptBetweenRows }, { "between-near", required_argument, nullptr, kOptBetweenNear },
		{ "qc", required_argument, nullptr, kOptQc }, { "sites-out", required_argument, nullptr, kOptSitesOut },
		{ "contam", required_argument, nullptr, kOptContam }, { "contam-depth", required_argument, nullptr, kOptContamDepth },
		{ "contam-min", required_argument, nullptr, kOptContamMin }, { "contam-explained", required_argument, nullptr, kOptContamExplained },
		{ "contam-rows", required_argument, nullptr, kOptContamRows }, { "samples-out", required_argument, nullptr, kOptSamplesOut },
		{ "trios", required_argument, nullptr, kOptTrios }, { "trio-depth", required_argument, nullptr, kOptTrioDepth },
		{ "trio-max", required_argument, nullptr, kOptTrioMax }, { "trio-duo", required_argument, nullptr, kOptTrioDuo },
		{ "trio-called", required_argument, nullptr, kOptTrioCalled }, { "trio-exhaustive", no_argument, nullptr, kOptTrioExhaustive },
		{ "ped", required_argument, nullptr, kOptPed },
		{ "ld", required_argument, nullptr, kOptLd }, { "ld-depth", required_argument, nullptr, kOptLdDepth }, { "ld-min", required_argument, nullptr, kOptLdMin },
		{ "ld-called", required_argument, nullptr, kOptLdCalled }, { "ld-prune", required_argument, nullptr, kOptLdPrune },
		{ nullptr, 0, nullptr, 0 } };
	int ch;
	while ((ch = getopt_long(argc, argv, "t:vhs:c:m:aw:g:p:n:d:r:e:o1:2:S:l:b:G:", long_options, nullptr)) != -1) {
		switch (ch) {
		case 'h': printHelpDialog(); break;
		case 'a': opt.all = true; break;
		case 's': ntsm::reference_flag('s', optarg, opt.scoreThresh); break;
		case 'w': ntsm::reference_flag('w', optarg, opt.covSkew); break;
		case 'c': ntsm::reference_flag('c', optarg, opt.minCov); opt.minCovGiven = true; break;
		case 'g': ntsm::reference_flag('g', optarg, opt.genomeSize); break;
		case 't': ntsm::reference_flag('t', optarg, opt.threads); break;
		case 'G': ntsm::reference_flag('G', optarg, opt.device); break;
		case 'e': opt.merge = optarg; break;
		case 'o': opt.onlyMerge = true; break;
		case 'p': ntsm::reference_flag('p', optarg, opt.pca); break;
		case 'n': ntsm::reference_flag('n', optarg, opt.norm); break;
		case 'd': ntsm::reference_flag('d', optarg, opt.dim); opt.dimGiven = true; break;
		case 'r': ntsm::reference_flag('r', optarg, opt.pcErrorThresh); break;
		case '1': ntsm::reference_flag('1', optarg, opt.pcMissSite1); break;
		case '2': ntsm::reference_flag('2', optarg, opt.pcMissSite2); break;
		case 'S': ntsm::reference_flag('S', optarg, opt.pcSearchRadius1); break;
		case 'l': ntsm::reference_flag('l', optarg, opt.pcSearchRadius2); break;
		case 'b': ntsm::reference_flag('b', optarg, opt.debug); break;
		case 'v': opt.verbose++; break;
		case kOptPack: opt.pack = optarg; storeMode = true; break;
		case kOptAgainst: opt.against = optarg; storeMode = true; break;
		case kOptIndex: opt.index = optarg; nearMode = true; break;
		case kOptNear: opt.near = optarg; nearMode = true; break;
		case kOptWithin: opt.within = optarg; withinMode = true; break;
		case kOptWithinNear: opt.withinNear = optarg; withinMode = true; break;
		case kOptWithinRows:
			if (!ntsm::read_whole(optarg, opt.withinRows)) ntsm::refuse(std::string("--within-rows takes a number of rows, not ") + optarg);
			opt.withinRowsGiven = true;
			break;
		case kOptBetween: opt.between = optarg; betweenMode = true; break;
		case kOptBetweenNear: opt.betweenNear = optarg; betweenNearMode = true; break;
		case kOptBetweenRows:
			if (!ntsm::read_whole(optarg, opt.betweenRows) || opt.betweenRows == 0)
				ntsm::refuse(std::string("--between-rows takes a number of rows of at least 1, not ") + optarg);
			opt.betweenRowsGiven = true;
			break;
		case kOptQc: opt.qc = optarg; qcMode = true; break;
		case kOptSitesOut: opt.sitesOut = optarg; opt.sitesOutGiven = true; break;
		case kOptContam: opt.contam = optarg; contamMode = true; break;
		case kOptContamDepth:
			if (optarg[0] == '-' || !ntsm::read_whole(optarg, opt.contamDepth)) ntsm::refuse(std::string("--contam-depth takes a number of reads, not ") + optarg);
			opt.contamFlagGiven = true;
			break;
		case kOptContamMin:
			if (!ntsm::read_whole(optarg, opt.contamMin)) ntsm::refuse(std::string("--contam-min takes a number, not ") + optarg);
			opt.contamFlagGiven = true;
			break;
		case kOptContamExplained:
			if (!ntsm::read_whole(optarg, opt.contamExplained)) ntsm::refuse(std::string("--contam-explained takes a number, not ") + optarg);
			opt.contamFlagGiven = true;
			break;
		case kOptContamRows:
			if (optarg[0] == '-' || !ntsm::read_whole(optarg, opt.contamRows)) ntsm::refuse(std::string("--contam-rows takes a number of samples, not ") + optarg);
			opt.contamFlagGiven = true;
			break;
		case kOptSamplesOut: opt.samplesOut = optarg; opt.samplesOutGiven = true; break;
		case kOptTrios: opt.trios = optarg; trioMode = true; break;
		case kOptTrioDepth:
			if (optarg[0] == '-' || !ntsm::read_whole(optarg, opt.trioDepth)) ntsm::refuse(std::string("--trio-depth takes a number of reads, not ") + optarg);
			opt.trioFlagGiven = true;
			break;
		case kOptTrioCalled:
			if (optarg[0] == '-' || !ntsm::read_whole(optarg, opt.trioCalled)) ntsm::refuse(std::string("--trio-called takes a number of sites, not ") + optarg);
			opt.trioFlagGiven = true;
			break;
		case kOptTrioMax:
			if (!ntsm::read_whole(optarg, opt.trioMax) || !std::isfinite(opt.trioMax)) ntsm::refuse(std::string("--trio-max takes a number, not ") + optarg);
			opt.trioFlagGiven = true;
			break;
		case kOptTrioDuo:
			if (!ntsm::read_whole(optarg, opt.trioDuo) || !std::isfinite(opt.trioDuo)) ntsm::refuse(std::string("--trio-duo takes a number, not ") + optarg);
			opt.trioFlagGiven = true;
			break;
		case kOptTrioExhaustive: opt.trioExhaustive = true; opt.trioFlagGiven = true; break;
		case kOptPed: opt.ped = optarg; opt.pedGiven = true; break;
		case kOptLd: opt.ld = optarg; ldMode = true; break;
		case kOptLdDepth:
			if (optarg[0] == '-' || !ntsm::read_whole(optarg, opt.ldDepth)) ntsm::refuse(std::string("--ld-depth takes a number of reads, not ") + optarg);
			opt.ldFlagGiven = true;
			break;
		case kOptLdCalled:
			if (optarg[0] == '-' || !ntsm::read_whole(optarg, opt.ldCalled)) ntsm::refuse(std::string("--ld-called takes a number of samples, not ") + optarg);
			opt.ldFlagGiven = true;
			break;
		case kOptLdMin:
			if (!ntsm::read_whole(optarg, opt.ldMin) || !std::isfinite(opt.ldMin)) ntsm::refuse(std::string("--ld-min takes a number, not ") + optarg);
			opt.ldFlagGiven = true;
			break;
		case kOptLdPrune: opt.ldPrune = optarg; opt.ldPruneGiven = true; opt.ldFlagGiven = true; break;
		case '?': die = true; break;
		default: break;                              /* m: read by the reference, without effect */
		}
	}
	Counts c;
	while (optind < argc) c.files.emplace_back(argv[optind++]);
	const char *sevenRuns = "--pack, --against, --index, --near, --within, --within-near and --between are seven runs: give one of them";
	if (ldMode && (storeMode || nearMode || withinMode || betweenMode || betweenNearMode || qcMode || contamMode || trioMode))
		ntsm::refuse("--ld compares the sites of one store and is a run of its own: it goes with none of --pack, --against, --index, --near, --within, "
		             "--within-near, --between, --between-near, --qc, --contam and --trios");
	if (opt.ldFlagGiven && !ldMode) ntsm::refuse("--ld-depth, --ld-min, --ld-called and --ld-prune belong to --ld: give them with --ld STORE");
	if (trioMode && (storeMode || nearMode || withinMode || betweenMode || betweenNearMode || qcMode || contamMode))
		ntsm::refuse("--trios looks for parent-child trios in one store and is a run of its own: it goes with none of --pack, --against, --index, --near, "
		             "--within, --within-near, --between, --between-near, --qc and --contam");
	if ((opt.trioFlagGiven || opt.pedGiven) && !trioMode)
		ntsm::refuse("--trio-depth, --trio-max, --trio-duo, --trio-called, --trio-exhaustive and --ped belong to --trios: give them with --trios STORE");
	if (contamMode && (storeMode || nearMode || withinMode || betweenMode || betweenNearMode || qcMode))
		ntsm::refuse("--contam checks one store for cross-sample contamination and is a run of its own: it goes with none of --pack, --against, --index, "
		             "--near, --within, --within-near, --between, --between-near and --qc");
	if (opt.contamFlagGiven && !contamMode)
		ntsm::refuse("--contam-depth, --contam-min, --contam-explained and --contam-rows belong to --contam: give them with --contam STORE");
	if (opt.samplesOutGiven && !contamMode) ntsm::refuse("--samples-out is the per-sample table of --contam: give it with --contam STORE");
	if (qcMode && (storeMode || nearMode || withinMode || betweenMode || betweenNearMode))
		ntsm::refuse("--qc prints the QC tables of one store and is a run of its own: it goes with none of --pack, --against, --index, --near, --within, "
		             "--within-near, --between and --between-near");
	if (opt.sitesOutGiven && !qcMode) ntsm::refuse("--sites-out is the per-site table of --qc: give it with --qc STORE");
	if (betweenNearMode) {                               /* --between-near: every refusal that needs no store, then the run */
		if (storeMode || nearMode || withinMode || betweenMode)
			ntsm::refuse("--pack, --against, --index, --near, --within, --within-near, --between and --between-near are eight runs: give one of them");
		if (opt.betweenRowsGiven) ntsm::refuse("--between-rows sets the bands of --between: it does not go with --between-near");
		if (opt.withinRowsGiven) ntsm::refuse("--within-rows sets the bands of --within: it does not go with --between-near");
		if (c.files.empty()) ntsm::refuse("--between-near needs the second store: --between-near STORE_A STORE_B");
		if (c.files.size() > 1) ntsm::refuse("--between-near takes STORE_B and no input files: it searches between the samples of two stores");
		if (!opt.pca.empty() || !opt.norm.empty()) ntsm::refuse("--between-near takes rotation and centre from the store's index: give no -p and no -n");
		refuseDebugAndMerge(opt, "--between-near");
		return searchBetween(opt, c.files[0], Clock::now());
	}
	if (opt.betweenRowsGiven && !betweenMode) ntsm::refuse("--between-rows sets the bands of --between: give it with --between STORE_A STORE_B");
	if (betweenMode) {                                   /* --between: every refusal that needs no store, then the run */
		if (storeMode || nearMode || withinMode) ntsm::refuse(sevenRuns);
		if (opt.withinRowsGiven) ntsm::refuse("--within-rows sets the bands of --within: the bands of --between are --between-rows");
		if (c.files.empty()) ntsm::refuse("--between needs the second store: --between STORE_A STORE_B");
		if (c.files.size() > 1) ntsm::refuse("--between takes STORE_B and no input files: it compares the samples of two stores");
		if (!opt.pca.empty() || !opt.norm.empty())
			ntsm::refuse("--between is the all-to-all run and takes no -p and no -n: a PCA-guided search between two stores is not part of this build "
			             "under this flag; it is --between-near STORE_A STORE_B");
		refuseDebugAndMerge(opt, "--between");
		return scoreBetween(opt, c.files[0], Clock::now());
	}
	if (withinMode) {                                    /* --within and --within-near: every refusal that needs no store, then the run */
		const bool near = opt.within.empty();
		const char *mode = near ? "--within-near" : "--within";
		if (storeMode || nearMode || (!opt.within.empty() && !opt.withinNear.empty())) ntsm::refuse(sevenRuns);
		if (!c.files.empty()) ntsm::refuse(std::string(mode) + " takes no input files: it compares the samples of the store with each other");
		if (!opt.pca.empty() || !opt.norm.empty())
			ntsm::refuse(near ? "--within-near takes rotation and centre from the store's index: give no -p and no -n"
			                  : "--within is the all-to-all run and takes no -p and no -n: the PCA-guided search inside a store is --within-near");
		refuseDebugAndMerge(opt, mode);
		if (opt.withinRowsGiven && near) ntsm::refuse("--within-rows sets the bands of --within: it does not go with --within-near");
		const auto t0 = Clock::now();
		return near ? searchWithin(opt, t0) : scoreWithin(opt, t0);
	}
	if (opt.withinRowsGiven) ntsm::refuse("--within-rows sets the bands of --within: give it with --within STORE");
	if (ldMode) {                                        /* --ld: every refusal that needs no store, then the run */
		if (!c.files.empty()) ntsm::refuse("--ld takes no input files: it compares the sites of the store");
		if (!opt.pca.empty() || !opt.norm.empty()) ntsm::refuse("--ld reads allele counts, not projections, and takes no -p and no -n");
		refuseDebugAndMerge(opt, "--ld");
		ntsm::try_help_if(die);
		return ldStore(opt, Clock::now());
	}
	if (trioMode) {                                      /* --trios: every refusal that needs no store, then the run */
		if (!c.files.empty()) ntsm::refuse("--trios takes no input files: it looks for trios among the samples of the store");
		if (!opt.pca.empty() || !opt.norm.empty()) ntsm::refuse("--trios reads allele counts, not projections, and takes no -p and no -n");
		refuseDebugAndMerge(opt, "--trios");
		if (opt.pedGiven && opt.trioExhaustive) ntsm::refuse("--ped checks the trios of a pedigree and searches nothing: it does not go with --trio-exhaustive");
		if (opt.pedGiven && opt.all) ntsm::refuse("--ped prints every trio of the pedigree with its verdict: it does not go with -a");
		ntsm::try_help_if(die);
		return trioStore(opt, Clock::now());
	}
	if (contamMode) {                                    /* --contam: every refusal that needs no store, then the run */
		if (!c.files.empty()) ntsm::refuse("--contam takes no input files: it checks the samples of the store against each other");
		if (!opt.pca.empty() || !opt.norm.empty()) ntsm::refuse("--contam reads allele counts, not projections, and takes no -p and no -n");
		refuseDebugAndMerge(opt, "--contam");
		ntsm::try_help_if(die);
		return contamStore(opt, Clock::now());
	}
	if (qcMode) {                                        /* --qc: every refusal that needs no store, then the run */
		if (!c.files.empty()) ntsm::refuse("--qc takes no input files: it prints the QC table of the samples of the store");
		refuseDebugAndMerge(opt, "--qc");
		if (!opt.pca.empty() || !opt.norm.empty()) {
			if (opt.pca.empty()) ntsm::refuse("--qc takes -n only with -p: the centre belongs to the rotation of the PC columns");
			if (!std::ifstream(opt.pca).good()) ntsm::refuse("--qc -p needs a readable rotation file");
			if (opt.norm.empty() || !std::ifstream(opt.norm).good()) ntsm::refuse("--qc -p needs a readable normalization file (-n)");
			if (opt.dim == 0) ntsm::refuse("a PCA search with -d 0 is not part of this build");
		}
		ntsm::try_help_if(die);
		return qcStore(opt, Clock::now());
	}
	if (nearMode) {                                      /* --index and --near: every refusal that needs no store comes before any file is read */
		const char *mode = opt.near.empty() ? "--index" : "--near";
		if (storeMode || (!opt.index.empty() && !opt.near.empty())) ntsm::refuse("--pack, --against, --index and --near are four runs: give one of them");
		refuseDebugAndMerge(opt, mode);
		if (!opt.near.empty()) {
			if (!opt.pca.empty() || !opt.norm.empty()) ntsm::refuse("--near takes rotation and centre from the store's index: give no -p and no -n");
			if (c.files.empty()) ntsm::refuse("--near needs input files");
		} else {
			if (!c.files.empty()) ntsm::refuse("--index takes no input files: it projects the samples of the store");
			if (opt.pca.empty() || !std::ifstream(opt.pca).good()) ntsm::refuse("--index needs a readable rotation file (-p)");
			if (opt.norm.empty() || !std::ifstream(opt.norm).good()) ntsm::refuse("--index needs a readable normalization file (-n)");
			if (opt.dim == 0) ntsm::refuse("a PCA search with -d 0 is not part of this build");
			return buildIndex(opt, Clock::now());
		}
	} else if (storeMode) {                              /* what --pack and --against do not go with: refused before any file is read */
		const char *mode = opt.pack.empty() ? "--against" : "--pack";
		if (!opt.pack.empty() && !opt.against.empty()) ntsm::refuse("--pack and --against are two runs: give one of them");
		if (!opt.pca.empty()) ntsm::refuse(std::string("the PCA-guided search (-p) ") + (opt.pack.empty() ? "against a store" : "with --pack") + " is not part of this build");
		refuseDebugAndMerge(opt, mode);
		if (c.files.empty()) ntsm::refuse(std::string(mode) + " needs input files");
	}
	for (const std::string &f : c.files)
		if (!std::ifstream(f).good()) {                  /* the reference asserts (src/ntSeqMatchEval.cpp:286) */
			std::cerr << PROGRAM ": input file " << f << " does not exist" << std::endl;
			abort();
		}
	if (c.files.empty()) { std::cerr << "Error: Need Input File" << std::endl; die = true; }
	/* the PCA path runs for one file (its PC columns) and for an analysis (not -o); refusals before any GPU work */
	const bool pcaRuns = !nearMode && !opt.pca.empty() && !c.files.empty() && (c.files.size() == 1 || !opt.onlyMerge);
	if (pcaRuns && !die) {
		if (!std::ifstream(opt.norm).good()) {           /* src/ntSeqMatchEval.cpp:335-338; the reference then dies in an assert */
			std::cerr << "Error: Need normalization file" << std::endl;
			std::cerr << "Error: a PCA search (-p) without a normalization file (-n) is not part of this build" << std::endl;
			die = true;
		} else if (!opt.debug.empty()) {
			std::cerr << "Error: the debug mode of the PCA search (-b) is not part of this build" << std::endl;
			die = true;
		} else if (opt.dim == 0) {
			std::cerr << "Error: a PCA search with -d 0 is not part of this build" << std::endl;
			die = true;
		}
	}
	ntsm::try_help_if(die);
	const auto t0 = Clock::now();
	if (!opt.pack.empty()) return packStore(c, opt);
	if (!opt.against.empty()) return scoreAgainst(c, opt, t0);
	if (!opt.near.empty()) return searchNear(c, opt, t0);
	if (opt.verbose > 0) std::cerr << "Reading count files" << std::endl;
	load(c);
	std::vector<Genotype> g = summaries(c, opt);
	std::vector<long double> norm, rot;
	if (pcaRuns) loadPCA(opt, c.nSites(), norm, rot);     /* every refusal and abort of the PCA inputs comes before the GPU */
	if (c.files.size() > 1 && opt.verbose > 1) std::cerr << "Finished loading files. Now comparing all samples." << std::endl;
	if (c.files.size() == 1) {                           /* computeScoreSingle, :541-585 */
		if (opt.verbose > 1) std::cerr << "Detected only 1 file, providing only QC information." << std::endl;
		std::string head = "sample\tcov\terrorRate\tmiss\thom\thet";
		std::vector<double> cloud;
		if (pcaRuns) {                                   /* projectPCs + the PC columns */
			Session session;
			int rc = ntsm_eval_open(opt.device, c.counts.data(), 1, (uint32_t) c.nSites(), opt.minCov, &session.h);
			if (rc) return gpuFail("session", rc);
			if ((rc = project(c, opt, session.h, norm, rot, cloud)) != 0) return rc;
			for (unsigned d = 1; d <= opt.dim; ++d) { head += "\tPC"; head += std::to_string(d); }
		}
		std::cout << head << std::endl;
		std::cout << c.files[0] << "\t" << std::to_string(g[0].cov) << "\t" << std::to_string(g[0].errorRate) << "\t" << std::to_string(g[0].miss)
		          << "\t" << std::to_string(g[0].homs) << "\t" << std::to_string(g[0].hets);
		for (double v : cloud) std::cout << "\t" << std::to_string(v);
	} else if (opt.onlyMerge) {                          /* src/ntSeqMatchEval.cpp:314-322 */
		if (opt.merge.empty()) { std::cerr << "(-l) cannot be used without --merge (-e) option." << std::endl; exit(EXIT_FAILURE); }
		std::cerr << " (-l) option detected. Not performing analysis, only merging." << std::endl;
	} else if (pcaRuns) {                                /* projectPCs + computeScorePCA, src/ntSeqMatchEval.cpp:333-341 */
		Session session;
		int rc = ntsm_eval_open(opt.device, c.counts.data(), (uint32_t) c.files.size(), (uint32_t) c.nSites(), opt.minCov, &session.h);
		if (rc) return gpuFail("session", rc);
		std::vector<double> cloud;
		rc = project(c, opt, session.h, norm, rot, cloud);
		if (!rc) rc = scorePCA(c, g, opt, session.h, cloud);
		if (rc) return rc;
	} else {                                             /* computeScore, :591-624 */
		std::cerr << "Performing all-to-all score computation.\nSpecify -p (--pca) to enable faster comparisons." << std::endl;
		const uint32_t n = (uint32_t) c.files.size();
		std::vector<ntsm_eval_record> rec((size_t) n * (n - 1) / 2);
		double ms = 0;
		const int rc = ntsm_eval_pairs(opt.device, c.counts.data(), n, (uint32_t) c.nSites(), opt.minCov, rec.data(), &ms);
		if (rc) return gpuFail("scoring", rc);
		if (opt.verbose > 1) std::cerr << "pair kernel: " << ms << " ms for " << rec.size() << " pairs" << std::endl;
		std::cout << kHeader;
		std::cout << "\n";
		std::string temp;
		for (uint32_t i = 0; i < n; ++i)
			for (uint32_t j = i + 1; j < n; ++j) printRow(temp, c, g, opt, rec[ntsm_eval_pair_index(i, j, n)], i, j, "-1");
	}
	std::cout.flush();
	if (c.files.size() > 1 && !opt.merge.empty()) {      /* mergeCounts, :626-674 */
		for (size_t i = 0; i < c.kmerSize.size(); ++i)
			for (size_t j = i + 1; j < c.kmerSize.size(); ++j)
				if (c.kmerSize[i] != c.kmerSize[j]) { std::cerr << PROGRAM ": counts files with different k cannot be merged" << std::endl; abort(); }   /* assert, :631-635 */
		std::ofstream out(opt.merge);
		uint64_t tk = 0;
		for (uint64_t v : c.rawTotal) tk += v;
		out << "#@TK\t" << std::to_string(tk) << "\n#@KS\t" << std::to_string(c.kmerSize[0])
		    << "\n#locusID\tcountAT\tcountCG\tsumAT\tsumCG\tdistinctAT\tdistinctCG\n";
		const size_t m = c.nSites();
		for (size_t s = 0; s < m; ++s) {
			unsigned cAT = 0, cCG = 0, sAT = 0, sCG = 0;
			for (size_t j = 0; j < c.files.size(); ++j) {
				cAT += c.counts[(j * m + s) * 2]; cCG += c.counts[(j * m + s) * 2 + 1];
				sAT += c.sums[(j * m + s) * 2]; sCG += c.sums[(j * m + s) * 2 + 1];
			}
			out << c.locus[s] << "\t" << cAT << "\t" << cCG << "\t" << sAT << "\t" << sCG << "\t" << c.distinct[2 * s] << "\t" << c.distinct[2 * s + 1] << "\n";
		}
	}
	printTime(t0);
	return 0;
}
