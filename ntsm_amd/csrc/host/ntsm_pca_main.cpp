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
 * `ntsmVCF --rotation`, which does this program's work on the cells it has in memory.
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
#include <fcntl.h>
#include <getopt.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <charconv>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/ntsm_pca_hip.h"
#include "gz_stream.hpp"
#include "pca_text.hpp"

#define PROGRAM "ntsmPCA"

namespace {

struct Opt {
	int verbose = 0, device = 0;
	unsigned threads = 1;
	long long numComp = 20;
	std::string matrix, prefix;
};

[[noreturn]] void refuse(const std::string &msg)
{
	std::cerr << "Error: " << msg << std::endl;
	exit(EXIT_FAILURE);
}

void printVersion()
{
	std::cerr << PROGRAM " (ntsm-mi355x)\n"
	          << "Exact PCA rotation matrix of an ntsmVCF matrix on the MI355X\n" << std::endl;
	exit(EXIT_SUCCESS);
}

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

template <typename T> bool parse(const char *s, T &out)
{
	std::stringstream c(s);
	return bool(c >> out) && c.eof();
}

/* The matrix file as bytes (plain: mapped; gzip: decoded) */
struct FileBytes {
	const char *data = nullptr;
	size_t size = 0;
	std::vector<char> owned;
	void *map = nullptr;
	~FileBytes() { if (map) munmap(map, size); }
	bool load(const std::string &path, unsigned threads)
	{
		if (ntsm::GzStream::is_gzip(path)) {
			ntsm::GzStream::set_decoder_threads(threads);
			ntsm::GzStream gz;
			if (!gz.open(path)) return false;
			std::vector<char> buf(1 << 22);
			for (;;) {
				const int n = gz.read(buf.data(), (unsigned) buf.size());
				if (n < 0) return false;
				if (n == 0) break;
				owned.insert(owned.end(), buf.data(), buf.data() + n);
			}
			data = owned.data();
			size = owned.size();
			return true;
		}
		const int fd = open(path.c_str(), O_RDONLY);
		if (fd < 0) return false;
		struct stat st;
		if (fstat(fd, &st) != 0 || S_ISDIR(st.st_mode)) { close(fd); return false; }
		if (S_ISREG(st.st_mode) && st.st_size > 0) {
			size = (size_t) st.st_size;
			map = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
			close(fd);
			if (map == MAP_FAILED) { map = nullptr; return false; }
			data = (const char *) map;
			return true;
		}
		std::vector<char> buf(1 << 20);                         /* empty, or not a regular file: read it through */
		for (ssize_t n; (n = read(fd, buf.data(), buf.size())) > 0;) owned.insert(owned.end(), buf.data(), buf.data() + n);
		close(fd);
		data = owned.data();
		size = owned.size();
		return true;
	}
};

using ntsm::Name;
using ntsm::format_repr;
using ntsm::line_end;
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
	auto invalid = [&](char flag) {
		std::cerr << "Error - Invalid parameter " << flag << ": " << optarg << std::endl;
		die = true;
	};
	int ch;
	while ((ch = getopt_long(argc, argv, "m:n:p:t:G:vh", long_options, nullptr)) != -1) {
		switch (ch) {
		case 'h': printHelpDialog(); break;
		case 'm': opt.matrix = optarg; break;
		case 'p': opt.prefix = optarg; break;
		case 'n': if (!parse(optarg, opt.numComp)) invalid('n'); break;
		case 't': if (!parse(optarg, opt.threads)) invalid('t'); break;
		case 'G': if (!parse(optarg, opt.device)) invalid('G'); break;
		case 'v': opt.verbose++; break;
		case '?': die = true; break;
		default: break;
		}
	}
	if (OPT_VERSION) printVersion();
	if (optind < argc) {
		std::cerr << "Error: Unexpected argument " << argv[optind] << " (the matrix is given with -m)" << std::endl;
		die = true;
	}
	if (opt.matrix.empty()) {
		std::cerr << "Error: Need Input File (-m)" << std::endl;
		die = true;
	}
	if (die) {
		std::cerr << "Try '--help' for more information.\n";
		exit(EXIT_FAILURE);
	}
	if (opt.numComp < 1) refuse(ntsm::pca_dims_low_error(opt.numComp));
	const unsigned T = opt.threads ? std::min(opt.threads, 256u) : std::max(1u, std::min(64u, std::thread::hardware_concurrency()));
	auto t_lap = std::chrono::steady_clock::now();
	const auto t_start = t_lap;
	auto lap = [&](const char *what) {
		const auto t = std::chrono::steady_clock::now();
		if (opt.verbose) fprintf(stderr, "[pca] %s: %.4f s\n", what, std::chrono::duration<double>(t - t_lap).count());
		t_lap = t;
	};

	FileBytes file;
	if (!file.load(opt.matrix, T)) refuse("cannot read the matrix file " + opt.matrix);
	if (file.size == 0) refuse("the matrix file " + opt.matrix + " is empty");
	lap("read");
	const char *const end = file.data + file.size;

	/* header: alleleID <TAB> sample ... */
	const char *nl = (const char *) memchr(file.data, '\n', file.size);
	const char *body = nl ? nl + 1 : end;
	const std::vector<Name> samples = ntsm::header_samples(file.data, nl ? nl : end);
	if (const std::string why = ntsm::pca_shape_error(opt.matrix, samples.size(), 1); !why.empty()) refuse(why);   /* the sites are not counted yet */
	const uint32_t n = (uint32_t) samples.size();

	/* body lines: cut the bytes into T ranges at line ends, count, then convert every range into its rows */
	std::vector<const char *> cut(T + 1, end);
	cut[0] = body;
	for (unsigned t = 1; t < T; ++t) {
		const char *q = body + (size_t) (end - body) * t / T;
		q = std::max(q, cut[t - 1]);
		const char *x = q < end ? (const char *) memchr(q, '\n', (size_t) (end - q)) : nullptr;
		cut[t] = x ? x + 1 : end;
	}
	std::vector<uint64_t> first(T + 1, 0);
	on_threads(T, [&](unsigned t) {
		uint64_t c = 0;
		for (const char *q = cut[t]; q < cut[t + 1];) {
			const char *x = (const char *) memchr(q, '\n', (size_t) (cut[t + 1] - q));
			++c;
			q = x ? x + 1 : cut[t + 1];
		}
		first[t + 1] = c;
	});
	for (unsigned t = 0; t < T; ++t) first[t + 1] += first[t];
	const uint64_t p = first[T];
	if (const std::string why = ntsm::pca_shape_error(opt.matrix, n, p); !why.empty()) refuse(why);
	std::vector<double> a((size_t) p * n);
	std::vector<Name> sites(p);
	std::vector<std::string> error(T);
	std::vector<uint64_t> error_row(T, ~0ull);
	on_threads(T, [&](unsigned t) {
		uint64_t k = first[t];
		for (const char *q = cut[t]; q < cut[t + 1]; ++k) {
			const char *x = (const char *) memchr(q, '\n', (size_t) (cut[t + 1] - q));
			const char *e = x ? x : cut[t + 1];
			error[t] = parse_row(q, line_end(q, e), n, sites[k], a.data() + (size_t) k * n);
			if (!error[t].empty()) { error_row[t] = k; return; }
			q = x ? x + 1 : cut[t + 1];
		}
	});
	for (unsigned t = 0; t < T; ++t)                               /* the first bad line of the file, whatever -t */
		if (error_row[t] != ~0ull) {
			refuse(ntsm::pca_row_error(opt.matrix, error_row[t], sites[error_row[t]], error[t]));
		}
	lap("parse");
	if (const std::string why = ntsm::pca_dims_high_error(opt.numComp, n, p); !why.empty()) refuse(why);
	const uint32_t d = (uint32_t) opt.numComp;
	if (opt.verbose) std::cerr << "Matrix: " << p << " sites x " << n << " samples, " << d << " components" << std::endl;

	std::vector<double> eigval(d), rot((size_t) p * d), comp((size_t) n * d);
	uint32_t bad = 0;
	ntsm_pca_times tm;
	memset(&tm, 0, sizeof tm);
	const int rc = ntsm_pca_run(opt.device, p, n, a.data(), d, 0, eigval.data(), rot.data(), comp.data(), &bad, &tm);
	if (rc != 0) refuse(ntsm::pca_run_error(rc, bad, d, opt.device));
	lap("device");
	if (opt.verbose) {
		ntsm::pca_print_times(stderr, tm, nullptr);
		if (opt.verbose > 1) for (uint32_t i = 0; i < d; ++i) fprintf(stderr, "[pca] eigenvalue %u: %.17g\n", i, eigval[i]);
	}

	if (const std::string bad_path = ntsm::write_pca_tables(opt.prefix, sites, samples, rot.data(), comp.data(), d, T); !bad_path.empty())
		refuse("cannot write " + bad_path);
	lap("write");
	if (opt.verbose) fprintf(stderr, "[pca] total: %.4f s\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count());
	return 0;
}
