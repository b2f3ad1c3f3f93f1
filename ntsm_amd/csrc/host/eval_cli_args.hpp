/*
 * eval_cli_args.hpp -- ntsmEval's command line (ntsm_eval_main.cpp): the options, the table of runs, the table of this build's
 * own value flags, the help dialog, the parse and the walk that issues the first refusal that needs no store (DESIGN.md
 * section 9, "The run table").  A new run is one row of kRunTable, its rows of kValueFlags and kStray, and the function that
 * performs it.
 */
#ifndef NTSM_EVAL_CLI_ARGS_HPP
#define NTSM_EVAL_CLI_ARGS_HPP

#include <getopt.h>

#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

#include "cli.hpp"
#include "eval_contam.hpp"
#include "eval_ld.hpp"
#include "eval_trio.hpp"

#define PROGRAM "ntsmEval"

namespace {

/* the runs; Files is the reference's: all pairs, the one-file QC table, -p, -e */
enum Run { Files, Pack, Against, Index, Near, Within, WithinNear, Between, BetweenNear, Qc, Contam, Trios, Ld };
/* what marks one of this build's own flags as given: the flags of a group are refused together where their run is absent */
enum Group { gWithinRows, gBetweenRows, gSitesOut, gContam, gSamplesOut, gTrio, gPed, gLd, gLdPrune };
constexpr unsigned bit(unsigned x) { return 1u << x; }

struct Opt {                                 /* src/Options.h:44-55 */
	double scoreThresh = 0.5, covSkew = 0.2;
	bool all = false;
	unsigned minCov = 1, threads = 1;
	uint64_t genomeSize = 6200000000ull;
	int verbose = 0, device = 0;
	std::string pca, merge, norm, debug;
	Run run = Files;                         /* the run flag read last, */
	std::string store;                       /* its STORE (STORE_A of the two-store runs), */
	unsigned runsGiven = 0;                  /* and bit(r) for every run flag r read: two of them is a refusal */
	unsigned groups = 0;                     /* bit(g) for every group g of own flags read */
	bool unknownOption = false;              /* getopt has complained */
	bool pcaRuns = false;                    /* Files: -p applies (one file: its PC columns; several: the search, unless -o) */
	unsigned withinRows = 0, betweenRows = 0, contamRows = 0;   /* rows per band, 0 = the run's band rule */
	std::string sitesOut, samplesOut, ped, ldPrune;             /* --sites-out, --samples-out, --ped, --ld-prune FILE */
	unsigned contamDepth = ntsm::eval_contam::kMinDepth;
	double contamMin = ntsm::eval_contam::kMinExcess, contamExplained = ntsm::eval_contam::kMinExplained;
	unsigned trioDepth = ntsm::eval_trio::kMinDepth, trioCalled = ntsm::eval_trio::kMinCalled;
	double trioMax = ntsm::eval_trio::kMaxRate, trioDuo = ntsm::eval_trio::kMaxDuo;
	bool trioExhaustive = false;
	unsigned ldDepth = ntsm::eval_ld::kMinDepth, ldCalled = ntsm::eval_ld::kMinCalled;
	double ldMin = ntsm::eval_ld::kMinR2;
	bool minCovGiven = false, dimGiven = false;
	bool onlyMerge = false;
	unsigned dim = 20;                       /* src/Options.h:22, 35-39: the PCA search */
	double pcSearchRadius1 = 2, pcSearchRadius2 = 15, pcErrorThresh = 0.01, pcMissSite1 = 0.01, pcMissSite2 = 0.3;
	bool has(Group g) const { return groups & bit(g); }
};

typedef std::vector<std::string> Positionals;

/* the runs' functions, ntsm_eval_main.cpp */
int runFiles(Opt &, const Positionals &), packStore(Opt &, const Positionals &), scoreAgainst(Opt &, const Positionals &),
    buildIndex(Opt &, const Positionals &), searchNear(Opt &, const Positionals &), scoreWithin(Opt &, const Positionals &),
    searchWithin(Opt &, const Positionals &), scoreBetween(Opt &, const Positionals &), searchBetween(Opt &, const Positionals &),
    qcStore(Opt &, const Positionals &), contamStore(Opt &, const Positionals &), trioStore(Opt &, const Positionals &), ldStore(Opt &, const Positionals &);

/* ---- the run table.  The rows stand in the order in which the runs take precedence: a run refuses any other run with its
 * own sentence (`otherRun`), so of two run flags the earlier row speaks.  --within-near stands before --within only so that
 * --within's band flag is not yet stray when it is reached; the two share their sentence, as --near and --index do. */
enum Takes { kFilesNeeded, kNoFiles, kStoreB };              /* positionals: FILES (at least one), none, exactly STORE_B */
enum PcaRule { kPcaReference, kPcaOnlyPRefused, kPcaRefused, kPcaFromIndex, kPcaRequired, kPcaOptional };   /* -p / -n: as the reference
                                                                 takes them; -p refused; both refused; both refused, the index has them;
                                                                 both needed and readable (--index); -n only with -p, then readable (--qc) */
struct RunRow {
	Run run;                                 /* its option id is kOptRun + run */
	const char *flag;
	Takes takes;
	const char *tooFew, *tooMany;            /* the sentences of its positionals */
	PcaRule pca;
	const char *pcaSentence;
	const char *otherRun;                    /* the sentence it refuses another run with */
	const char *band[2];                     /* its own sentence for --between-rows, --within-rows given with it, where it has one */
	const char *steps;                       /* its checks, in its order: F positionals, P -p / -n, D -b / -e / -o, T --ped's rules,
	                                            W --within-rows after the others (--within-near), H an unknown option stops it here,
	                                            C the reference's checks of FILES and -p, an unknown option among them */
	int (*perform)(Opt &, const Positionals &);
};

#define SEVEN_RUNS "--pack, --against, --index, --near, --within, --within-near and --between are seven runs: give one of them"
#define FOUR_RUNS "--pack, --against, --index and --near are four runs: give one of them"
#define INDEX_HAS_THEM " takes rotation and centre from the store's index: give no -p and no -n"
#define COUNTS_ONLY " reads allele counts, not projections, and takes no -p and no -n"
constexpr RunRow kRunTable[] = {
	{ Ld, "--ld", kNoFiles, nullptr, "--ld takes no input files: it compares the sites of the store", kPcaRefused, "--ld" COUNTS_ONLY,
	  "--ld compares the sites of one store and is a run of its own: it goes with none of --pack, --against, --index, --near, --within, "
	  "--within-near, --between, --between-near, --qc, --contam and --trios", { nullptr, nullptr }, "FPDH", ldStore },
	{ Trios, "--trios", kNoFiles, nullptr, "--trios takes no input files: it looks for trios among the samples of the store", kPcaRefused, "--trios" COUNTS_ONLY,
	  "--trios looks for parent-child trios in one store and is a run of its own: it goes with none of --pack, --against, --index, --near, "
	  "--within, --within-near, --between, --between-near, --qc and --contam", { nullptr, nullptr }, "FPDTH", trioStore },
	{ Contam, "--contam", kNoFiles, nullptr, "--contam takes no input files: it checks the samples of the store against each other", kPcaRefused,
	  "--contam" COUNTS_ONLY,
	  "--contam checks one store for cross-sample contamination and is a run of its own: it goes with none of --pack, --against, --index, "
	  "--near, --within, --within-near, --between, --between-near and --qc", { nullptr, nullptr }, "FPDH", contamStore },
	{ Qc, "--qc", kNoFiles, nullptr, "--qc takes no input files: it prints the QC table of the samples of the store", kPcaOptional, nullptr,
	  "--qc prints the QC tables of one store and is a run of its own: it goes with none of --pack, --against, --index, --near, --within, "
	  "--within-near, --between and --between-near", { nullptr, nullptr }, "FDPH", qcStore },
	{ BetweenNear, "--between-near", kStoreB, "--between-near needs the second store: --between-near STORE_A STORE_B",
	  "--between-near takes STORE_B and no input files: it searches between the samples of two stores", kPcaFromIndex, "--between-near" INDEX_HAS_THEM,
	  "--pack, --against, --index, --near, --within, --within-near, --between and --between-near are eight runs: give one of them",
	  { "--between-rows sets the bands of --between: it does not go with --between-near", "--within-rows sets the bands of --within: it does not go with --between-near" },
	  "FPD", searchBetween },
	{ Between, "--between", kStoreB, "--between needs the second store: --between STORE_A STORE_B",
	  "--between takes STORE_B and no input files: it compares the samples of two stores", kPcaRefused,
	  "--between is the all-to-all run and takes no -p and no -n: a PCA-guided search between two stores is not part of this build "
	  "under this flag; it is --between-near STORE_A STORE_B", SEVEN_RUNS,
	  { nullptr, "--within-rows sets the bands of --within: the bands of --between are --between-rows" }, "FPD", scoreBetween },
	{ WithinNear, "--within-near", kNoFiles, nullptr, "--within-near takes no input files: it compares the samples of the store with each other", kPcaFromIndex,
	  "--within-near" INDEX_HAS_THEM, SEVEN_RUNS, { nullptr, "--within-rows sets the bands of --within: it does not go with --within-near" }, "FPDW", searchWithin },
	{ Within, "--within", kNoFiles, nullptr, "--within takes no input files: it compares the samples of the store with each other", kPcaRefused,
	  "--within is the all-to-all run and takes no -p and no -n: the PCA-guided search inside a store is --within-near", SEVEN_RUNS, { nullptr, nullptr }, "FPD",
	  scoreWithin },
	{ Near, "--near", kFilesNeeded, "--near needs input files", nullptr, kPcaFromIndex, "--near" INDEX_HAS_THEM, FOUR_RUNS, { nullptr, nullptr }, "DPFC", searchNear },
	{ Index, "--index", kNoFiles, nullptr, "--index takes no input files: it projects the samples of the store", kPcaRequired, nullptr, FOUR_RUNS,
	  { nullptr, nullptr }, "DFP", buildIndex },
	{ Pack, "--pack", kFilesNeeded, "--pack needs input files", nullptr, kPcaOnlyPRefused, "the PCA-guided search (-p) with --pack is not part of this build",
	  "--pack and --against are two runs: give one of them", { nullptr, nullptr }, "PDFC", packStore },
	{ Against, "--against", kFilesNeeded, "--against needs input files", nullptr, kPcaOnlyPRefused,
	  "the PCA-guided search (-p) against a store is not part of this build", nullptr, { nullptr, nullptr }, "PDFC", scoreAgainst },
	{ Files, nullptr, kFilesNeeded, nullptr, nullptr, kPcaReference, nullptr, nullptr, { nullptr, nullptr }, "C", runFiles },
};
#undef SEVEN_RUNS
#undef FOUR_RUNS
#undef INDEX_HAS_THEM
#undef COUNTS_ONLY

/* the sentences for a run's own flags given without it, each checked right after its owner's row */
struct Stray { Run owner; unsigned groups; int band; const char *sentence; };   /* band: its column of RunRow::band, or -1 */
constexpr Stray kStray[] = {
	{ Ld, bit(gLd) | bit(gLdPrune), -1, "--ld-depth, --ld-min, --ld-called and --ld-prune belong to --ld: give them with --ld STORE" },
	{ Trios, bit(gTrio) | bit(gPed), -1, "--trio-depth, --trio-max, --trio-duo, --trio-called, --trio-exhaustive and --ped belong to --trios: give them with --trios STORE" },
	{ Contam, bit(gContam), -1, "--contam-depth, --contam-min, --contam-explained and --contam-rows belong to --contam: give them with --contam STORE" },
	{ Contam, bit(gSamplesOut), -1, "--samples-out is the per-sample table of --contam: give it with --contam STORE" },
	{ Qc, bit(gSitesOut), -1, "--sites-out is the per-site table of --qc: give it with --qc STORE" },
	{ Between, bit(gBetweenRows), 0, "--between-rows sets the bands of --between: give it with --between STORE_A STORE_B" },
	{ Within, bit(gWithinRows), 1, "--within-rows sets the bands of --within: give it with --within STORE" },
};

/* ---- this build's own value flags: read whole or refused with "<flag> takes <noun>, not <value>"; the three bits are what
 * else is refused.  An unsigned value with a leading minus that is not refused wraps (--within-rows -1 is 4,294,967,295 rows);
 * the stream reads neither nan nor inf, so `nonFinite` changes nothing today. */
struct ValueFlag {
	const char *name;                        /* its option id is kOptValue + its row */
	unsigned Opt::*count;
	double Opt::*real;                       /* the member it fills: one of the two */
	const char *noun;
	bool minus, nonFinite, zero;             /* refused: a leading minus, a non-finite value, 0 */
	Group group;
};
constexpr ValueFlag kValueFlags[] = {
	{ "within-rows", &Opt::withinRows, nullptr, "a number of rows", false, false, false, gWithinRows },
	{ "between-rows", &Opt::betweenRows, nullptr, "a number of rows of at least 1", false, false, true, gBetweenRows },
	{ "contam-depth", &Opt::contamDepth, nullptr, "a number of reads", true, false, false, gContam },
	{ "contam-min", nullptr, &Opt::contamMin, "a number", false, false, false, gContam },
	{ "contam-explained", nullptr, &Opt::contamExplained, "a number", false, false, false, gContam },
	{ "contam-rows", &Opt::contamRows, nullptr, "a number of samples", true, false, false, gContam },
	{ "trio-depth", &Opt::trioDepth, nullptr, "a number of reads", true, false, false, gTrio },
	{ "trio-called", &Opt::trioCalled, nullptr, "a number of sites", true, false, false, gTrio },
	{ "trio-max", nullptr, &Opt::trioMax, "a number", false, true, false, gTrio },
	{ "trio-duo", nullptr, &Opt::trioDuo, "a number", false, true, false, gTrio },
	{ "ld-depth", &Opt::ldDepth, nullptr, "a number of reads", true, false, false, gLd },
	{ "ld-called", &Opt::ldCalled, nullptr, "a number of samples", true, false, false, gLd },
	{ "ld-min", nullptr, &Opt::ldMin, "a number", false, true, false, gLd },
};

void readValueFlag(const ValueFlag &f, const char *value, Opt &opt)
{
	bool ok = !(f.minus && value[0] == '-');
	if (ok && f.count) ok = ntsm::read_whole(value, opt.*f.count) && !(f.zero && opt.*f.count == 0);
	if (ok && f.real) ok = ntsm::read_whole(value, opt.*f.real) && !(f.nonFinite && !std::isfinite(opt.*f.real));
	if (!ok) ntsm::refuse(std::string("--") + f.name + " takes " + f.noun + ", not " + value);
	opt.groups |= bit(f.group);
}

/* long-only options: no letter of the reference's option string is taken */
constexpr int kOptRun = 1000, kOptValue = 1100, kOptSitesOut = 1200, kOptSamplesOut = 1201, kOptTrioExhaustive = 1202, kOptPed = 1203, kOptLdPrune = 1204;

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

/* This build's long options in the order getopt is given them, the help's: where an abbreviation is ambiguous getopt names
 * the possibilities in this order, and those bytes are kept.  A new flag is added here as well as to its table. */
constexpr const char *kLongOrder[] = {
	"pack", "against", "index", "near", "within", "within-near", "within-rows", "between", "between-rows", "between-near", "qc", "sites-out",
	"contam", "contam-depth", "contam-min", "contam-explained", "contam-rows", "samples-out", "trios", "trio-depth", "trio-max", "trio-duo",
	"trio-called", "trio-exhaustive", "ped", "ld", "ld-depth", "ld-min", "ld-called", "ld-prune" };

/* the getopt entry of one of them: a run's flag, a value flag, or one of the five path and no-value flags */
option ownOption(const char *name)
{
	for (const RunRow &r : kRunTable)
		if (r.flag && !strcmp(r.flag + 2, name)) return { name, required_argument, nullptr, kOptRun + r.run };
	for (const ValueFlag &f : kValueFlags)
		if (!strcmp(f.name, name)) return { name, required_argument, nullptr, kOptValue + int(&f - kValueFlags) };
	static const option others[] = { { "sites-out", required_argument, nullptr, kOptSitesOut }, { "samples-out", required_argument, nullptr, kOptSamplesOut },
		{ "trio-exhaustive", no_argument, nullptr, kOptTrioExhaustive }, { "ped", required_argument, nullptr, kOptPed }, { "ld-prune", required_argument, nullptr, kOptLdPrune } };
	for (const option &o : others)
		if (!strcmp(o.name, name)) return o;
	abort();                                     /* a name of kLongOrder that no table has */
}

/* step 1: the flags into opt; the run flags and the value flags come from their tables */
void readFlags(int argc, char **argv, Opt &opt)
{
	std::vector<option> longOptions = {
		{ "score_thresh", required_argument, nullptr, 's' }, { "all", no_argument, nullptr, 'a' },
		{ "min_cov", required_argument, nullptr, 'c' }, { "skew", required_argument, nullptr, 'w' },
		{ "genome_size", required_argument, nullptr, 'g' }, { "threads", required_argument, nullptr, 't' },
		{ "merge", required_argument, nullptr, 'e' }, { "only_merge", required_argument, nullptr, 'o' },
		{ "help", no_argument, nullptr, 'h' }, { "pca", required_argument, nullptr, 'p' }, { "norm", required_argument, nullptr, 'n' },
		{ "error_rate", required_argument, nullptr, 'r' }, { "miss_small", required_argument, nullptr, '1' },
		{ "miss_large", required_argument, nullptr, '2' }, { "small", required_argument, nullptr, 'k' },   /* 'k': as in the reference's table, no effect */
		{ "large", required_argument, nullptr, 'l' }, { "debug", required_argument, nullptr, 'b' },
		{ "gpu", required_argument, nullptr, 'G' }, { "verbose", no_argument, nullptr, 'v' } };
	for (const char *name : kLongOrder) longOptions.push_back(ownOption(name));
	longOptions.push_back({ nullptr, 0, nullptr, 0 });
	int ch;
	while ((ch = getopt_long(argc, argv, "t:vhs:c:m:aw:g:p:n:d:r:e:o1:2:S:l:b:G:", longOptions.data(), nullptr)) != -1) {
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
		case kOptSitesOut: opt.sitesOut = optarg; opt.groups |= bit(gSitesOut); break;
		case kOptSamplesOut: opt.samplesOut = optarg; opt.groups |= bit(gSamplesOut); break;
		case kOptTrioExhaustive: opt.trioExhaustive = true; opt.groups |= bit(gTrio); break;
		case kOptPed: opt.ped = optarg; opt.groups |= bit(gPed); break;
		case kOptLdPrune: opt.ldPrune = optarg; opt.groups |= bit(gLdPrune); break;
		case '?': opt.unknownOption = true; break;
		default:                                     /* m: read by the reference, without effect */
			if (ch >= kOptValue) readValueFlag(kValueFlags[ch - kOptValue], optarg, opt);
			else if (ch >= kOptRun) { opt.run = Run(ch - kOptRun); opt.store = optarg; opt.runsGiven |= bit(opt.run); }   /* given twice: the last STORE */
			break;
		}
	}
}

/* what no store run goes with */
void refuseDebugAndMerge(const Opt &opt, const char *mode)
{
	if (!opt.debug.empty()) ntsm::refuse(std::string("-b with ") + mode + " is not part of this build");
	if (!opt.merge.empty() || opt.onlyMerge) ntsm::refuse(std::string("merging (-e, -o) with ") + mode + " is not part of this build: the store does not hold the per-site sums");
}

bool readable(const std::string &path) { return std::ifstream(path).good(); }

/* 'P': the -p / -n rule of a run */
void checkPcaFlags(const RunRow &r, const Opt &opt)
{
	const bool any = !opt.pca.empty() || !opt.norm.empty();
	switch (r.pca) {
	case kPcaReference: break;                           /* 'C' has them */
	case kPcaOnlyPRefused: if (!opt.pca.empty()) ntsm::refuse(r.pcaSentence); break;
	case kPcaRefused: case kPcaFromIndex: if (any) ntsm::refuse(r.pcaSentence); break;
	case kPcaRequired: case kPcaOptional: {
		const bool qc = r.pca == kPcaOptional;
		if (qc && !any) break;
		if (qc && opt.pca.empty()) ntsm::refuse("--qc takes -n only with -p: the centre belongs to the rotation of the PC columns");
		if (!readable(opt.pca)) ntsm::refuse(qc ? "--qc -p needs a readable rotation file" : "--index needs a readable rotation file (-p)");
		if (!readable(opt.norm)) ntsm::refuse(std::string(qc ? "--qc -p" : "--index") + " needs a readable normalization file (-n)");
		if (opt.dim == 0) ntsm::refuse("a PCA search with -d 0 is not part of this build");
		break;
	}
	}
}

/* 'C': what the reference checks of FILES and -p, for the runs that read counts files; sets opt.pcaRuns */
void checkFilesAsTheReference(Opt &opt, const Positionals &files)
{
	bool die = opt.unknownOption;
	for (const std::string &f : files)
		if (!readable(f)) {                              /* the reference asserts (src/ntSeqMatchEval.cpp:286) */
			std::cerr << PROGRAM ": input file " << f << " does not exist" << std::endl;
			abort();
		}
	if (files.empty()) { std::cerr << "Error: Need Input File" << std::endl; die = true; }
	/* the PCA path runs for one file (its PC columns) and for an analysis (not -o); under --pack, --against and --near -p is refused by now */
	opt.pcaRuns = !opt.pca.empty() && !files.empty() && (files.size() == 1 || !opt.onlyMerge);
	if (opt.pcaRuns && !die) {
		if (!readable(opt.norm)) {                       /* src/ntSeqMatchEval.cpp:335-338; the reference then dies in an assert */
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
}

/* step 3: walk the table in its order and issue the first refusal that applies; returns the row of the run.  At a row: the
 * run is refused with another (any that is still given stands in a later row); then its own flags are refused without it.
 * Once that has passed the row of the one run given, that run's own checks follow in its `steps` order -- at once, except
 * that every stray flag comes first: with the run's own sentence where RunRow::band has one, and for --within-near only
 * after its other checks (its 'W'), which no table order gives. */
const RunRow &firstRefusal(Opt &opt, const Positionals &files)
{
	const RunRow *run = nullptr;
	for (const RunRow &r : kRunTable) {
		const bool given = r.run == Files ? opt.runsGiven == 0 : (opt.runsGiven & bit(r.run)) != 0;
		if (given && (opt.runsGiven & ~bit(r.run))) ntsm::refuse(r.otherRun);
		if (given) run = &r;
		for (const Stray &s : kStray) {
			if (s.owner != r.run || given || !(opt.groups & s.groups)) continue;
			const char *own = s.band >= 0 && run ? run->band[s.band] : nullptr;
			if (own && run->run == WithinNear) continue;
			ntsm::refuse(own ? own : s.sentence);
		}
	}
	for (const char *step = run->steps; *step; ++step)
		switch (*step) {
		case 'F':
			if (run->takes != kNoFiles && files.empty()) ntsm::refuse(run->tooFew);
			if (run->takes != kFilesNeeded && files.size() > (run->takes == kStoreB ? 1u : 0u)) ntsm::refuse(run->tooMany);
			break;
		case 'P': checkPcaFlags(*run, opt); break;
		case 'D': refuseDebugAndMerge(opt, run->flag); break;
		case 'T':
			if (opt.has(gPed) && opt.trioExhaustive) ntsm::refuse("--ped checks the trios of a pedigree and searches nothing: it does not go with --trio-exhaustive");
			if (opt.has(gPed) && opt.all) ntsm::refuse("--ped prints every trio of the pedigree with its verdict: it does not go with -a");
			break;
		case 'W': if (opt.has(gWithinRows)) ntsm::refuse(run->band[1]); break;
		case 'H': ntsm::try_help_if(opt.unknownOption); break;
		case 'C': checkFilesAsTheReference(opt, files); break;
		}
	return *run;
}

}  // namespace

#endif
