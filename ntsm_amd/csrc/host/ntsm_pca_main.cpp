/*
 * ntsm_pca_main.cpp -- ntsmPCA: the exact PCA rotation matrix of the matrix `ntsmVCF -p NAME` writes, on the MI355X.
 *
 *   ntsmPCA -m NAME_matrix.tsv [-n 20] [-p PREFIX] [-t THREADS] [-G DEVICE] [-v]
 *       ->  PREFIX_rotationalMatrix.tsv  (what `ntsmEval -p` reads)   and   PREFIX_components.tsv
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
 * cell that is not a finite number, D < 1 or D > min(samples, sites).  After the eigen step: a requested component
 * whose eigenvalue is not positive beyond rounding.
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
#include "pca_text.hpp"

#define PROGRAM "ntsmPCA"

namespace {

struct Opt {
	int verbose = 0, device = 0;
	unsigned threads = 1;
	long long numComp = 20;
	std::string matrix, prefix;
};

void printHelpDialog()
{
	std::cerr << "Usage: " PROGRAM " -m [MATRIX]\n"
	    "Computes the PCA rotation matrix (for ntsmEval -p) and the component\n"
	    "scores of the samples from the matrix ntsmVCF -p writes.\n"
	    "  -m, --matrix = STR     Matrix file (sites x samples, tab separated,\n"
	    "                         plain or gzip). [required]\n"
	    "  -n, --numComp = INT    Number of components. [20]\n"
	    "  -p, --prefix = STR     Prefix of PREFIX_rotationalMatrix.tsv and\n"
	    "                         PREFIX_components.tsv. []\n"
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

} // namespace

int main(int argc, char **argv)
{
	Opt opt;
	bool die = false;
	int OPT_VERSION = 0;
	static struct option long_options[] = {
		{ "matrix", required_argument, nullptr, 'm' }, { "numComp", required_argument, nullptr, 'n' },
		{ "prefix", required_argument, nullptr, 'p' }, { "threads", required_argument, nullptr, 't' },
		{ "gpu", required_argument, nullptr, 'G' }, { "help", no_argument, nullptr, 'h' },
		{ "version", no_argument, &OPT_VERSION, 1 }, { "verbose", no_argument, nullptr, 'v' }, { nullptr, 0, nullptr, 0 } };
	int ch;
	while ((ch = getopt_long(argc, argv, "m:n:p:t:G:vh", long_options, nullptr)) != -1) {
		switch (ch) {
		case 'h': printHelpDialog(); break;
		case 'm': opt.matrix = optarg; break;
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
	if (opt.matrix.empty()) usage("Error: Need Input File (-m)");
	ntsm::try_help_if(die);
	if (opt.numComp < 1) refuse(ntsm::pca_dims_low_error(opt.numComp));
	const unsigned T = ntsm::thread_count(opt.threads);
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
