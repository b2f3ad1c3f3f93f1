/*
 * ntsm_pca_main.cpp -- ntsmPCA: the exact PCA rotation matrix of the matrix `ntsmVCF -p NAME` writes, on the MI355X.
 *
 *   ntsmPCA -m NAME_matrix.tsv [-n 20] [-p PREFIX] [-t THREADS] [-G DEVICE] [-v]
 *       ->  PREFIX_rotationalMatrix.tsv  (what `ntsmEval -p` reads)   and   PREFIX_components.tsv
 *   ntsmPCA --store STORE [-c 1] [--train N] [-n 20] -p PREFIX [-t THREADS] [-G DEVICE] [-v]
 *       ->  those two and PREFIX_center.txt (what `ntsmEval -n` reads), trained on the cohort store's own samples: the
 *           matrix is the genotypes that ntsmEval's projection derives from the store's counts, every site centred over
 *           the samples that call it.  It is made on the device from the mapped store
 *           (ntsm_pca_run_store) and never exists as text.  --train N takes the first N records.
 *
 * It takes the place of the upstream project's `ntsmSiteGen generate-pca-rot-mat` step (pandas + scikit-learn), with the
 * flags -m / -n / -p of that script, and computes what sklearn.decomposition.PCA(n_components=D, svd_solver="full")
 * computes on the transposed matrix -- deterministically: the output is a pure function of the input file, the same
 * bytes on every run and for every -t.  The arithmetic is in libntsm_pca_hip.so
 * (include/ntsm_pca_hip.h); there is no CPU fallback.
 *
 * The number text, the refusals' words and the writer of the two outputs are in pca_text.hpp, shared with
 * `ntsmVCF --rotation`, which does this program's work on the cells it has in memory (loader, cutter, flags: cli.hpp).
 *
 * The host reads the text (plain or gzip) and converts it on -t threads with std::from_chars, which is correctly
 * rounded; it formats the two outputs on -t threads with std::to_chars' shortest round-trip digits laid out the way
 * Python's repr lays them out, which is how pandas writes a float.
 *
 * Refused with "Error: ..." and exit status 1 before the device is touched and before anything is written: a missing,
 * unreadable or empty matrix, a header with fewer than 2 samples, a row whose field count differs from the header's, a
 * cell that is not a finite number, D < 1 or D > min(samples, sites); --store with -m or without -p, -c or --train
 * without --store, a store that is missing, invalid, empty or holds fewer than 2 samples, --train 0 or beyond the store.
 * After the eigen step: a requested component whose eigenvalue is not positive beyond rounding.
 */
#include <getopt.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "../../../include/ntsm_pca_hip.h"
#include "cli.hpp"
#include "eval_store.hpp"
#include "pca_text.hpp"

#define PROGRAM "ntsmPCA"

namespace {

struct Opt {
	int verbose = 0, device = 0;
	unsigned threads = 1;
	long long numComp = 20, minCov = 1, train = 0;
	bool minCovGiven = false, trainGiven = false;
	std::string matrix, prefix, store;
};

void printHelpDialog()
{
	std::cerr << "Usage: " PROGRAM " -m [MATRIX]\n"
	    "       " PROGRAM " --store [STORE] -p [PREFIX]\n"
	    "Computes the PCA rotation matrix (for ntsmEval -p) and the component\n"
	    "scores of the samples from the matrix ntsmVCF -p writes, or from the\n"
	    "samples of a cohort store; then also the centre file (for ntsmEval -n).\n"
	    "  -m, --matrix = STR     Matrix file (sites x samples, tab separated,\n"
	    "                         plain or gzip). [-m or --store required]\n"
	    "      --store = STR      Cohort store (ntsmCount --cohort --store,\n"
	    "                         ntsmEval --pack): train on its samples.\n"
	    "  -c, --minCov = INT     With --store: a count at or below it reads\n"
	    "                         as 0, as ntsmEval -c. [1]\n"
	    "      --train = INT      With --store: the first INT samples. [all]\n"
	    "  -n, --numComp = INT    Number of components. [20]\n"
	    "  -p, --prefix = STR     Prefix of PREFIX_rotationalMatrix.tsv and\n"
	    "                         PREFIX_components.tsv, with --store also of\n"
	    "                         PREFIX_center.txt (required there). []\n"
	    "  -t, --threads = INT    Number of threads to run.[1]\n"
	    "  -G, --gpu = INT        HIP device [0]\n"
	    "  -h, --help             Display this dialog.\n"
	    "  -v, --verbose          Display verbose output (stage times).\n"
	    "      --version          Print version information.\n" << std::endl;
	exit(EXIT_SUCCESS);
}

using ntsm::Name;
using ntsm::format_repr;                     /* tests/pca_text_check.cpp calls it from this file's scope */
using ntsm::line_end;
using ntsm::refuse;
using ntsm::on_threads;

/* one body line into one row of the matrix; an empty string when it is fine, else what is wrong with it */
std::string parse_row(const char *b, const char *e, uint32_t n, Name &name, double *row)
{
	const char *t = (const char *) memchr(b, '\t', (size_t) (e - b));
	name = Name { b, (size_t) ((t ? t : e) - b) };
	uint32_t j = 0;
	for (const char *q = t ? t + 1 : e; t; ++j) {
		t = (const char *) memchr(q, '\t', (size_t) (e - q));
		const char *f = t ? t : e;
		if (j < n) {
			double x = 0.0;
			if (!ntsm::parse_cell(q, f, x))
				return "the cell of sample " + std::to_string(j + 1) + " is not a finite number: '" + std::string(q, f) + "'";
			row[j] = x;
		}
		q = f + 1;
	}
	if (j != n) return ntsm::pca_row_fields_error(j + 1, n);
	return std::string();
}

struct Matrix {
	std::vector<Name> samples, sites;        /* views into the file's bytes */
	std::vector<double> a;                   /* [sites][samples] */
};

/* the text into the matrix: the header, then the body cut into T ranges at line ends, counted, and every range converted
 * into its rows.  Refused in this order: the header's shape, no sites, the first bad line of the file (whatever -t) */
Matrix read_matrix(const std::string &name, const ntsm::FileBytes &file, unsigned T)
{
	Matrix m;
	const char *const end = file.data + file.size;
	const char *nl = (const char *) memchr(file.data, '\n', file.size);   /* header: alleleID <TAB> sample ... */
	m.samples = ntsm::header_samples(file.data, nl ? nl : end);
	if (const std::string why = ntsm::pca_shape_error(name, m.samples.size(), 1); !why.empty()) refuse(why);   /* the sites are not counted yet */
	const uint32_t n = (uint32_t) m.samples.size();
	const ntsm::LineCuts cut = ntsm::cut_lines(nl ? nl + 1 : end, end, T);
	const uint64_t p = cut.lines_before[T];
	if (const std::string why = ntsm::pca_shape_error(name, n, p); !why.empty()) refuse(why);
	m.a.resize((size_t) p * n);
	m.sites.resize(p);
	std::vector<std::string> error(T);
	std::vector<uint64_t> error_row(T, ~0ull);
	on_threads(T, [&](unsigned t) {
		uint64_t k = cut.lines_before[t];
		for (const char *q = cut.at[t]; q < cut.at[t + 1]; ++k) {
			const char *x = (const char *) memchr(q, '\n', (size_t) (cut.at[t + 1] - q));
			const char *e = x ? x : cut.at[t + 1];
			error[t] = parse_row(q, line_end(q, e), n, m.sites[k], m.a.data() + (size_t) k * n);
			if (!error[t].empty()) { error_row[t] = k; return; }
			q = x ? x + 1 : cut.at[t + 1];
		}
	});
	for (unsigned t = 0; t < T; ++t)
		if (error_row[t] != ~0ull) refuse(ntsm::pca_row_error(name, error_row[t], m.sites[error_row[t]], error[t]));
	return m;
}

/* what is wrong with training on the first n of the store's samples, empty when nothing is (p: its sites) */
std::string store_shape_error(const std::string &store, uint64_t n, uint64_t p)
{
	if (n < 2) return "a PCA needs at least 2 samples: " + std::to_string(n) + " of " + store + " to train on";
	if (n >= (1u << 24)) return "too many samples: " + std::to_string(n) + " (--train takes a prefix)";
	if (p == 0) return store + " has no sites";
	return std::string();
}

/* --store: the PCA of the mapped store's first --train records on the device, then the three files */
int run_store(const Opt &opt, unsigned T)
{
	namespace st = ntsm::eval_store;
	ntsm::LapTimer timer { "[pca]", opt.verbose > 0 };
	st::View store;
	try {                                        /* validated as ntsmEval's store modes validate it */
		store.open(opt.store);
		if (store.h.n_samples == 0) throw st::Error(opt.store + " holds no samples");
	} catch (const st::Error &e) {
		refuse(e.what());
	}
	if (opt.trainGiven && (opt.train < 1 || (unsigned long long) opt.train > store.h.n_samples))
		refuse("--train " + std::to_string(opt.train) + ": " + opt.store + " holds " + std::to_string(store.h.n_samples) + " samples, the first 1 ... " +
		    std::to_string(store.h.n_samples) + " of them can be taken");
	const uint64_t n64 = opt.trainGiven ? (uint64_t) opt.train : store.h.n_samples, p = store.h.n_sites;
	if (const std::string why = store_shape_error(opt.store, n64, p); !why.empty()) refuse(why);
	const uint32_t n = (uint32_t) n64, d = (uint32_t) opt.numComp;
	if (const std::string why = ntsm::pca_dims_high_error(opt.numComp, n, p); !why.empty()) refuse(why);
	timer.lap("map");
	if (opt.verbose) std::cerr << "Matrix: " << p << " sites x " << n << " samples of " << opt.store << ", " << d << " components" << std::endl;
	uint32_t db_chunk = 0;                       /* samples per upload; a test forces several chunks with it */
	if (const char *c = getenv("NTSM_PCA_STORE_CHUNK")) db_chunk = (uint32_t) strtoul(c, nullptr, 10);
	std::vector<double> eigval(d), rot((size_t) p * d), comp((size_t) n * d);
	std::vector<uint32_t> tallies((size_t) p * 3);
	uint32_t bad = 0;
	ntsm_pca_times tm {};
	ntsm_pca_store_times stm {};
	const int rc = ntsm_pca_run_store(opt.device, store.counts(0), store.h.stride, n, p, (uint32_t) opt.minCov, db_chunk, d, 0, eigval.data(), rot.data(),
	    comp.data(), tallies.data(), &bad, &tm, &stm);
	if (rc != 0) refuse(ntsm::pca_run_error(rc, bad, d, opt.device));
	timer.lap("device");
	if (opt.verbose) {
		fprintf(stderr, "[pca] store: %u chunks of %u samples, upload %.3f ms, genotype %.3f ms, tallies and fills %.3f ms\n", stm.chunks, stm.chunk,
		    stm.upload_ms, stm.genotype_ms, stm.fill_ms);
		ntsm::pca_print_times(stderr, tm, &stm.expand_ms);
		if (opt.verbose > 1) for (uint32_t i = 0; i < d; ++i) fprintf(stderr, "[pca] eigenvalue %u: %.17g\n", i, eigval[i]);
	}
	std::string centre;
	for (uint64_t s = 0; s < p; ++s) { centre += ntsm::store_centre_text(tallies[3 * s], tallies[3 * s + 1], tallies[3 * s + 2]); centre += "\n"; }
	const std::string centre_path = opt.prefix + "_center.txt";
	FILE *cf = fopen(centre_path.c_str(), "wb");
	if (!cf) refuse("cannot write " + centre_path);
	const bool ok = fwrite(centre.data(), 1, centre.size(), cf) == centre.size();
	if (fclose(cf) != 0 || !ok) refuse("cannot write " + centre_path);
	std::vector<std::string> sample_names(n);
	std::vector<Name> sites(p), samples(n);
	for (uint64_t s = 0; s < p; ++s) sites[s] = Name { store.locus[s].data(), store.locus[s].size() };
	for (uint32_t j = 0; j < n; ++j) { sample_names[j] = store.name(j); samples[j] = Name { sample_names[j].data(), sample_names[j].size() }; }
	if (const std::string bad_path = ntsm::write_pca_tables(opt.prefix, sites, samples, rot.data(), comp.data(), d, T); !bad_path.empty())
		refuse("cannot write " + bad_path);
	timer.lap("write");
	if (opt.verbose) fprintf(stderr, "[pca] total: %.4f s\n", timer.total());
	return 0;
}

} // namespace

int main(int argc, char **argv)
{
	Opt opt;
	bool die = false;
	int OPT_VERSION = 0;
	enum { kOptStore = 1000, kOptTrain };            /* long options only */
	static struct option long_options[] = {
		{ "store", required_argument, nullptr, kOptStore }, { "train", required_argument, nullptr, kOptTrain },
		{ "minCov", required_argument, nullptr, 'c' },
		{ "matrix", required_argument, nullptr, 'm' }, { "numComp", required_argument, nullptr, 'n' },
		{ "prefix", required_argument, nullptr, 'p' }, { "threads", required_argument, nullptr, 't' },
		{ "gpu", required_argument, nullptr, 'G' }, { "help", no_argument, nullptr, 'h' },
		{ "version", no_argument, &OPT_VERSION, 1 }, { "verbose", no_argument, nullptr, 'v' }, { nullptr, 0, nullptr, 0 } };
	int ch;
	while ((ch = getopt_long(argc, argv, "m:n:p:t:G:c:vh", long_options, nullptr)) != -1) {
		switch (ch) {
		case 'h': printHelpDialog(); break;
		case 'm': opt.matrix = optarg; break;
		case kOptStore: opt.store = optarg; break;
		case 'c': opt.minCovGiven = true; ntsm::whole_flag('c', optarg, opt.minCov, die); break;
		case kOptTrain:
			opt.trainGiven = true;
			if (!ntsm::read_whole(optarg, opt.train)) { std::cerr << "Error - Invalid parameter train: " << optarg << std::endl; die = true; }
			break;
		case 'p': opt.prefix = optarg; break;
		case 'n': ntsm::whole_flag('n', optarg, opt.numComp, die); break;
		case 't': ntsm::whole_flag('t', optarg, opt.threads, die); break;
		case 'G': ntsm::whole_flag('G', optarg, opt.device, die); break;
		case 'v': opt.verbose++; break;
		case '?': die = true; break;
		default: break;
		}
	}
	if (OPT_VERSION) ntsm::print_version(PROGRAM, "Exact PCA rotation matrix of an ntsmVCF matrix on the MI355X");
	auto usage = [&](const std::string &msg) { std::cerr << msg << std::endl; die = true; };
	if (optind < argc) usage(std::string("Error: Unexpected argument ") + argv[optind] + " (the matrix is given with -m)");
	const bool fromStore = !opt.store.empty();
	if (fromStore && !opt.matrix.empty()) usage("Error: --store and -m each name the matrix: give one of them");
	else if (!fromStore && opt.matrix.empty()) usage("Error: Need Input File (-m) or a cohort store (--store)");
	if (!fromStore && opt.minCovGiven) usage("Error: -c belongs to --store (a matrix file holds genotypes, not counts)");
	if (!fromStore && opt.trainGiven) usage("Error: --train belongs to --store");
	if (fromStore && opt.prefix.empty()) usage("Error: --store needs -p PREFIX (PREFIX_center.txt is written beside the two tables)");
	if (fromStore && opt.minCovGiven && !die && (opt.minCov < 0 || opt.minCov > (long long) UINT32_MAX))
		usage("Error: -c " + std::to_string(opt.minCov) + " is not a count");
	ntsm::try_help_if(die);
	if (opt.numComp < 1) refuse(ntsm::pca_dims_low_error(opt.numComp));
	const unsigned T = ntsm::thread_count(opt.threads);
	if (fromStore) return run_store(opt, T);
	ntsm::LapTimer timer { "[pca]", opt.verbose > 0 };
	ntsm::FileBytes file;                        /* a directory is not a matrix file */
	if (!file.load(opt.matrix, T, ntsm::FileBytes::kDirectoryIsUnreadable)) refuse("cannot read the matrix file " + opt.matrix);
	if (file.size == 0) refuse("the matrix file " + opt.matrix + " is empty");
	timer.lap("read");
	const Matrix m = read_matrix(opt.matrix, file, T);
	timer.lap("parse");
	const uint64_t p = m.sites.size();
	const uint32_t n = (uint32_t) m.samples.size(), d = (uint32_t) opt.numComp;
	if (const std::string why = ntsm::pca_dims_high_error(opt.numComp, n, p); !why.empty()) refuse(why);
	if (opt.verbose) std::cerr << "Matrix: " << p << " sites x " << n << " samples, " << d << " components" << std::endl;
	std::vector<double> eigval(d), rot((size_t) p * d), comp((size_t) n * d);
	uint32_t bad = 0;
	ntsm_pca_times tm {};
	const int rc = ntsm_pca_run(opt.device, p, n, m.a.data(), d, 0, eigval.data(), rot.data(), comp.data(), &bad, &tm);
	if (rc != 0) refuse(ntsm::pca_run_error(rc, bad, d, opt.device));
	timer.lap("device");
	if (opt.verbose) {
		ntsm::pca_print_times(stderr, tm, nullptr);
		if (opt.verbose > 1) for (uint32_t i = 0; i < d; ++i) fprintf(stderr, "[pca] eigenvalue %u: %.17g\n", i, eigval[i]);
	}
	if (const std::string bad_path = ntsm::write_pca_tables(opt.prefix, m.sites, m.samples, rot.data(), comp.data(), d, T); !bad_path.empty())
		refuse("cannot write " + bad_path);
	timer.lap("write");
	if (opt.verbose) fprintf(stderr, "[pca] total: %.4f s\n", timer.total());
	return 0;
}
