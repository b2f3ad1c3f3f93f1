/*
 * ntsm_vcf_main.cpp -- host mirror of the reference's ntsmVCF (src/ntSeqMatchVCF.cpp:54-216, src/VCFConvert.hpp,
 * src/MultiCount.hpp): a multi-sample VCF and a reference genome to the PCA matrix NAME_matrix.tsv and the centre file
 * NAME_center.txt that ntsmEval -n reads.  Same flags (plus -G, the HIP device), same output and stderr bytes as ONE
 * thread of the reference with one correction: the sample x k-mer matrix is sized for the header's samples (the reference
 * sizes it before reading the header, VCFConvert.hpp:42 / MultiCount.hpp:278, and crashes at the first insert).
 *
 *   sites        ntsm::SiteSet (MultiCount::initCountsHash, :214-288: the same loader as FingerPrint's)
 *   genome       every record of -r through ntsm::SeqReader (VCFConvert.hpp:43-58; a later duplicate name wins)
 *   VCF          parsed here on -t threads (VCFConvert::count, :63-172): per line the REF / VAR windows
 *                (getSeqFromSite, :207-218), the genotype codes and the window k-mers that are keys (the EVENTS)
 *   inserts      + maxima + sums: one call into the HIP library (include/ntsm_vcf_hip.h), which replaces the
 *                insertCount calls (:151-170) and printNormMatrix's walk of the matrix (MultiCount.hpp:156-187)
 *   matrix       formatted here on -t threads (printNormMatrix, :148-201; iostream's %.*g / %.*Lg, the precision 19
 *                that sticks to the stream after the first undefined cell)
 *   rotation     -R: the PCA of that matrix in the same run (what ntsmPCA computes from NAME_matrix.tsv): the cells go
 *                to libntsm_pca_hip.so with the double every cell's text reads back as (include/ntsm_pca_hip.h,
 *                ntsm_pca_run_cells), and NAME_rotationalMatrix.tsv and NAME_components.tsv are written as ntsmPCA
 *                writes them (pca_text.hpp); -M leaves NAME_matrix.tsv out
 *   counts       --counts DIR / --store STORE (this build only): what the reference's VCFConvert::outputCounts would write
 *                (:176-187, MultiCount::printCountsMax, MultiCount.hpp:93-138; its main never calls it), per sample a
 *                counts file and / or a record of a cohort store (eval_store.hpp), from ntsm_vcf_records, in windows of
 *                samples so that memory does not grow with the cohort
 * Whatever -t is, the result is the one-thread result.  Inputs where the reference throws, asserts or has undefined
 * behaviour are refused with "Error: ..." and exit status 1.  A VCF that starts with the gzip
 * magic is decoded (ntsm::GzStream); the reference reads it as text and finds no samples.
 */
#include <getopt.h>
#include <sys/resource.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../../include/ntsm_pca_hip.h"
#include "../../../include/ntsm_vcf_hip.h"
#include "cli.hpp"
#include "eval_store.hpp"
#include "kmer.hpp"
#include "pca_text.hpp"
#include "seq_reader.hpp"
#include "site_set.hpp"

#define PROGRAM "ntsmVCF"

/* Referenced weakly: a program linked against a device library without the records step (the CPU stand-in of
 * tests/test_vcf.py) still links, and refuses --counts / --store */
extern "C" __attribute__((weak)) int ntsm_vcf_records(int device, uint32_t n_samples, uint32_t multi, uint64_t n_lines, const uint8_t *geno,
		uint32_t g_stride, uint64_t n_keys, const uint64_t *key_off, uint64_t n_events, const uint32_t *ev_ord, const uint32_t *ev_ls,
		uint64_t n_sites, const uint64_t *site_off, const uint32_t *site_keys, uint32_t s_begin, uint32_t s_count, uint32_t *counts,
		uint64_t counts_pitch, uint32_t *sums, uint64_t sums_pitch, uint64_t *total, uint64_t *sum_of_sums, ntsm_vcf_records_times *times);

namespace {

struct Opt {                                 /* src/Options.h: the members ntsmVCF reads */
	int verbose = 0, device = 0;
	unsigned threads = 1, k = 19, window = 31, multi = 20;
	bool dupes = false;
	bool rotation = false, no_matrix = false, dims_given = false;   /* -R, -M, -n (this build only) */
	long long numComp = 20;                                         /* ntsmPCA's -n and its default */
	std::string snp, ref, pca;
	std::string counts_dir, store;                                  /* --counts, --store (this build only) */
	bool want_counts = false, want_store = false;
	bool records() const { return want_counts || want_store; }
	std::vector<std::string> inputs;                                /* the arguments after the flags */
	unsigned T = 1;                                                 /* ntsm::thread_count(threads) */
};

constexpr unsigned kMaxWindow = 1u << 20;    /* getSeqFromSite keeps two window + 1 byte arrays on the stack */

void printHelpDialog()
{
	const Opt d;
	std::cerr << "Usage: " PROGRAM " -s [FASTA] -r [FASTA] [VCF]\n"
	    "Converts a multi vcf file to a set of counts files.\n"
	    "Alternatively, you may also create a matrix to be used for PCA.\n"
	    "  -t, --threads = INT    Number of threads to run.[1]\n"
	    "  -d, --dupes            Allow shared k-mers between sites to\n"
	    "                         be counted.\n"
	    "  -s, --snp = STR        Interleaved fasta of SNP sites to\n"
	    "                         k-merize. [required]\n"
	    "  -p, --pca = STR        With multivcf generate rotation and\n"
	    "                         centering files with this prefix.\n"
	    "  -k, --kmer = INT       k-mer size used. [19]\n"
	    "  -m, --multi = INT      Value to multiply base counts [" << std::to_string(d.multi) << "]\n"
	    "  -w, --window = INT     Window size used. [" << std::to_string(d.window) << "]\n"
	    "  -r, --ref = STR        Reference fasta. [required]\n"
	    "  -G, --gpu = INT        HIP device [0] (this build only)\n"
	    "  -R, --rotation         With -p: also run the PCA of the matrix (as\n"
	    "                         ntsmPCA does) and write the rotation for\n"
	    "                         ntsmEval -p and the components. (this build only)\n"
	    "  -n, --dims = INT       With -R: number of components. [" << std::to_string(d.numComp) << "]\n"
	    "  -M, --no-matrix        With -R: do not write the matrix file.\n"
	    "      --counts = DIR     Write DIR/SAMPLE.counts.txt for every sample.\n"
	    "                         (this build only)\n"
	    "      --store = STR      Create this cohort store for ntsmEval --against,\n"
	    "                         or append to it: one record per sample.\n"
	    "                         (this build only)\n"
	    "  -h, --help             Display this dialog.\n"
	    "  -v, --verbose          Display verbose output.\n"
	    "      --version          Print version information.\n" << std::endl;
	exit(EXIT_SUCCESS);
}

bool fexists(const std::string &f) { return std::ifstream(f).good(); }       /* src/Util.h:22-27 */

/* key lookup: canonical code -> key index (open addressing; the reference's m_kmerToHash) */
class KeyTable {
public:
	explicit KeyTable(const std::vector<uint64_t> &keys)
	{
		size_t cap = 16;
		while (cap < keys.size() * 2 + 16) cap <<= 1;
		mask_ = cap - 1;
		slot_.assign(cap, kEmpty);
		idx_.assign(cap, 0);
		for (size_t i = 0; i < keys.size(); ++i) {
			size_t h = hash(keys[i]);
			while (slot_[h] != kEmpty) h = (h + 1) & mask_;
			slot_[h] = keys[i];
			idx_[h] = (uint32_t) i;
		}
	}
	int64_t find(uint64_t code) const
	{
		for (size_t h = hash(code);; h = (h + 1) & mask_) {
			if (slot_[h] == code) return idx_[h];
			if (slot_[h] == kEmpty) return -1;
		}
	}
private:
	static constexpr uint64_t kEmpty = ~0ull;                    /* no canonical code of k <= 31 */
	size_t hash(uint64_t c) const { return (size_t) ((c * 0x9E3779B97F4A7C15ull) >> 20) & mask_; }
	size_t mask_ = 0;
	std::vector<uint64_t> slot_;
	std::vector<uint32_t> idx_;
};

struct Genome {                              /* VCFConvert::m_ref / m_chrIDs */
	std::vector<std::string> seq;
	std::unordered_map<std::string, uint32_t> id;
};

/* What one body line of the VCF contributes (VCFConvert::count, :102-171) */
struct Part {                                /* the lines [lo, hi) of one thread, in order */
	std::vector<uint32_t> ev_key;            /* events: key index */
	std::vector<uint8_t> ev_side;
	std::vector<uint32_t> ev_line;           /* used line, local numbering */
	std::vector<uint8_t> geno;               /* [used line][stride] */
	uint32_t used = 0;
	bool failed = false;
	std::string error;
	std::vector<std::string> rs_id;          /* -v -v -v: per line */
	std::vector<uint64_t> line_events;       /* -v -v -v: events per line */
};

struct Ctx {
	const Opt &opt;
	const Genome &genome;
	const KeyTable &table;
	uint32_t n_samples, stride;
};

/* std::getline(ss, item, '\t') repeated on one line: the i-th call gives field i, and once the fields are used up the
 * item keeps its last value (a failed getline does not touch it).  A call that reaches the end of the line without
 * extracting anything fails, so an empty last field -- the one after a trailing tab, or an empty line -- is not counted by
 * the reference's `while (getline(ss, item, '\t'))` loops (VCFConvert.hpp:86, :139), although it leaves item empty */
struct Fields {
	std::vector<std::pair<const char *, const char *>> f;
	void split(const char *b, const char *e)
	{
		f.clear();
		for (const char *p = b;;) {
			const char *t = (const char *) memchr(p, '\t', (size_t) (e - p));
			if (!t) { f.emplace_back(p, e); return; }
			f.emplace_back(p, t);
			p = t + 1;
		}
	}
	std::string get(size_t i) const { const auto &x = f[std::min(i, f.size() - 1)]; return std::string(x.first, x.second); }
	/* successful getline calls: every field but an empty last one */
	size_t n_read() const { return f.size() - (f.back().first == f.back().second ? 1 : 0); }
};

int genotype_code(const char *b, const char *e)              /* :140-146; anything else stays hom1 */
{
	if (e - b != 3 || b[1] != '|') return NTSM_VCF_HOM1;
	if (b[0] == '0' && b[2] == '0') return NTSM_VCF_HOM1;
	if ((b[0] == '0' && b[2] == '1') || (b[0] == '1' && b[2] == '0')) return NTSM_VCF_HET;
	if (b[0] == '1' && b[2] == '1') return NTSM_VCF_HOM2;
	return NTSM_VCF_HOM1;
}

void parse_lines(const Ctx &c, const char *lo, const char *hi, uint64_t first_line, Part &out)
{
	Fields fl;
	const unsigned W = c.opt.window, half = W / 2;
	std::vector<char> refStr(W + 1), varStr(W + 1);
	uint64_t line_no = first_line;
	for (const char *p = lo; p < hi; ++line_no) {
		const char *nl = (const char *) memchr(p, '\n', (size_t) (hi - p));
		const char *b = p, *e = nl;                              /* every line here ends in '\n' */
		p = nl + 1;
		auto fail = [&](const std::string &why) {
			out.failed = true;
			out.error = "line " + std::to_string(line_no) + " of the VCF: " + why;
		};
		if (b == e) { fail("empty line"); return; }             /* stoi("") throws */
		fl.split(b, e);
		const std::string chr = fl.get(0), pos_s = fl.get(1);
		long pos;
		try {
			pos = std::stoi(pos_s);                              /* :114 */
		} catch (const std::exception &) {
			fail("POS '" + pos_s + "' is not an int"); return;
		}
		const size_t n_before = out.ev_key.size();
		if (c.opt.verbose > 2) out.rs_id.push_back(fl.get(2));
		auto done_line = [&]() { if (c.opt.verbose > 2) out.line_events.push_back(out.ev_key.size() - n_before); };
		if (fl.get(3) == ".") { done_line(); continue; }         /* :121-124 */
		const std::string alt = fl.get(4);
		if (alt.size() != 1) { done_line(); continue; }          /* :125-128 */
		/* getSeqFromSite (:207-218) */
		const auto chr_it = c.genome.id.find(chr);
		if (chr_it == c.genome.id.end()) { fail("unknown chromosome '" + chr + "'"); return; }
		const std::string &g = c.genome.seq[chr_it->second];
		if (pos <= (long) half) { fail("POS " + std::to_string(pos) + " is not greater than half the window"); return; }
		const size_t offset = (size_t) pos - half - 1;
		if (g.empty() || offset > g.size()) { fail("the window at POS " + std::to_string(pos) + " starts past the end of " + chr); return; }
		strncpy(refStr.data(), g.c_str() + offset, W);
		strncpy(varStr.data(), g.c_str() + offset, W);
		varStr[half] = alt[0];
		varStr[W] = '\0';
		refStr[W] = '\0';
		/* genotypes (:137-149): fields 9 on; their number must be the header's */
		const size_t n_gt = fl.n_read() > 9 ? fl.n_read() - 9 : 0;
		if (n_gt != c.n_samples) {
			fail(std::to_string(n_gt) + " genotype fields, the header has " + std::to_string(c.n_samples) + " samples"); return;
		}
		const size_t n_ref_before = out.ev_key.size();
		for (int side = 0; side < 2 && c.n_samples; ++side) {     /* without samples no insert happens */
			const char *s = side ? varStr.data() : refStr.data();
			ntsm::for_each_kmer(s, strlen(s), c.opt.k, [&](uint64_t code, uint64_t) {
				const int64_t q = c.table.find(code);
				if (q < 0) return;                                   /* insertCount: not a key, nothing happens */
				out.ev_key.push_back((uint32_t) q);
				out.ev_side.push_back((uint8_t) side);
				out.ev_line.push_back(out.used);
			});
		}
		if (out.ev_key.size() > n_ref_before && c.n_samples) {
			const size_t at = out.geno.size();
			out.geno.resize(at + c.stride, (uint8_t) NTSM_VCF_PAD);
			for (uint32_t s = 0; s < c.n_samples; ++s) out.geno[at + s] = (uint8_t) genotype_code(fl.f[9 + s].first, fl.f[9 + s].second);
		}
		if (out.ev_key.size() > n_ref_before) ++out.used;
		done_line();
	}
}

long rss_kbytes()                            /* Util::getRSS: only in the Time line, which is not compared */
{
	struct rusage ru;
	getrusage(RUSAGE_SELF, &ru);
	return ru.ru_maxrss;
}

using ntsm::on_threads, ntsm::refuse;

/* The number text of NAME_matrix.tsv and NAME_center.txt (printNormMatrix, MultiCount.hpp:148-201), stated once: the
 * matrix writer prints these strings and -R hands the PCA what ntsmPCA would read back from them (text_value). */
std::string cell_text(unsigned r, unsigned v, int prec)     /* a defined cell: iostream's %.*g of maxREF / (maxREF + maxVAR) */
{
	char b[64];
	snprintf(b, sizeof b, "%.*g", prec, double(r) / double(r + v));
	return std::string(b);
}

using ntsm::centre_text;                                    /* a row's centre, also the text of its undefined cells: pca_text.hpp */

constexpr int kShortDigits = 6, kLongDigits = 19;           /* the stream's precision up to / after the first undefined cell */

double text_value(const std::string &text)                  /* the cell ntsmPCA reads from this text; NaN if it would refuse it */
{
	double x = 0.0;
	return ntsm::parse_cell(text.data(), text.data() + text.size(), x) ? x : std::numeric_limits<double>::quiet_NaN();
}

/* the flags and what is refused from them alone, in the reference's order (src/ntSeqMatchVCF.cpp:82-199), then this build's */
Opt read_options(int argc, char **argv)
{
	Opt opt;
	bool die = false;
	int OPT_VERSION = 0;
	enum { kOptCounts = 1000, kOptStore };                           /* long options only: none of the reference's letters */
	static struct option long_options[] = {
		{ "threads", required_argument, nullptr, 't' }, { "dupes", no_argument, nullptr, 'd' },
		{ "snp", required_argument, nullptr, 's' }, { "pca", required_argument, nullptr, 'p' },
		{ "kmer", required_argument, nullptr, 'k' }, { "multi", required_argument, nullptr, 'm' },
		{ "window", required_argument, nullptr, 'w' }, { "ref", required_argument, nullptr, 'r' },
		{ "help", no_argument, nullptr, 'h' }, { "version", no_argument, &OPT_VERSION, 1 },
		{ "verbose", no_argument, nullptr, 'v' }, { "gpu", required_argument, nullptr, 'G' },
		{ "rotation", no_argument, nullptr, 'R' }, { "dims", required_argument, nullptr, 'n' },
		{ "no-matrix", no_argument, nullptr, 'M' }, { "counts", required_argument, nullptr, kOptCounts },
		{ "store", required_argument, nullptr, kOptStore }, { nullptr, 0, nullptr, 0 } };
	int ch;
	while ((ch = getopt_long(argc, argv, "s:t:vhk:dr:w:m:p:G:Rn:M", long_options, nullptr)) != -1) {
		switch (ch) {                            /* src/ntSeqMatchVCF.cpp:82-156 */
		case 'h': printHelpDialog(); break;
		case 'd': opt.dupes = true; break;
		case 's': ntsm::reference_flag('s', optarg, opt.snp); break;
		case 'p': ntsm::reference_flag('p', optarg, opt.pca); break;
		case 'k': ntsm::reference_flag('k', optarg, opt.k); break;
		case 'w': ntsm::reference_flag('w', optarg, opt.window); break;
		case 'm': ntsm::reference_flag('m', optarg, opt.multi); break;
		case 't': ntsm::reference_flag('t', optarg, opt.threads); break;
		case 'r': ntsm::reference_flag('r', optarg, opt.ref); break;
		case 'G': ntsm::reference_flag('G', optarg, opt.device); break;
		case 'R': opt.rotation = true; break;
		case 'M': opt.no_matrix = true; break;
		case 'n': opt.dims_given = true; ntsm::whole_flag('n', optarg, opt.numComp, die); break;   /* as ntsmPCA reads its -n */
		case 'v': opt.verbose++; break;
		case kOptCounts: opt.want_counts = true; opt.counts_dir = optarg; break;
		case kOptStore: opt.want_store = true; opt.store = optarg; break;
		case '?': die = true; break;
		default: break;
		}
	}
	if (OPT_VERSION) ntsm::print_version(PROGRAM, "MI355X-native implementation of ntsmVCF (multi-sample VCF to PCA matrix)");
	auto usage = [&](const char *msg) { std::cerr << msg << std::endl; die = true; };
	if (opt.k > 32) usage("k cannot be greater than 32");            /* :168-171 */
	while (optind < argc) {
		opt.inputs.emplace_back(argv[optind++]);
		if (!fexists(opt.inputs.back())) refuse("input file " + opt.inputs.back() + " does not exist");   /* :176 asserts */
	}
	if (opt.inputs.empty()) usage("Error: Need Input File");
	if (!fexists(opt.ref)) usage("Error: Unable to load reference file");
	if (opt.rotation && opt.pca.empty()) usage("Error: -R needs -p");
	if (!opt.rotation && (opt.dims_given || opt.no_matrix)) usage(opt.dims_given ? "Error: -n needs -R" : "Error: -M needs -R");
	ntsm::try_help_if(die);
	if (opt.rotation && opt.numComp < 1) refuse(ntsm::pca_dims_low_error(opt.numComp));
	if (opt.inputs.size() > 1) refuse("ntsmVCF takes one VCF file, " + std::to_string(opt.inputs.size()) + " were given");   /* :199 asserts */
	if (opt.k == 0 || opt.k == 32) refuse("-k " + std::to_string(opt.k) + " is not supported (k must be 1 to 31)");
	if (opt.records() && !ntsm_vcf_records) refuse("--counts / --store: the device library of this build lacks the records step (ntsm_vcf_records)");
	if (opt.window >= kMaxWindow) refuse("-w " + std::to_string(opt.window) + " is too large (at most " + std::to_string(kMaxWindow - 1) + ")");
	opt.T = ntsm::thread_count(opt.threads);
	return opt;
}

ntsm::SiteSet load_sites(const Opt &opt)         /* VCFConvert's constructor, first half: the sites (MultiCount's) */
{
	ntsm::SiteSet sites;
	auto cannot_open = [&]() { std::cerr << "file " << opt.snp << " cannot be opened" << std::endl; exit(1); };
	if (!fexists(opt.snp)) cannot_open();                           /* MultiCount.hpp:218-221 */
	if (opt.verbose) std::cerr << "Opening " << opt.snp << std::endl;
	if (!sites.load(opt.snp, opt.k, opt.dupes, std::cerr)) cannot_open();
	const size_t n_sites = sites.ids.size();
	if (sites.ref.size() != sites.var.size())
		refuse("the sites file has an odd number of records (" + std::to_string(sites.ref.size() + sites.var.size()) + "): site " +
		    sites.ids.back() + " has no VAR record");
	if ((!opt.pca.empty() || opt.records()) && !opt.dupes && sites.n_erased) {
		/* without -d a shared k-mer is erased from the keys but stays in its first allele list: the reference's
		 * printNormMatrix throws at that site (m_kmerToHash.at), after rows that overlap the next sample's, and so does
		 * printCountsMax (--counts / --store) */
		size_t s = 0;
		auto has = [](const std::vector<int64_t> &l) { return std::find(l.begin(), l.end(), ntsm::SiteSet::kErased) != l.end(); };
		while (s < n_sites && !has(sites.ref[s]) && !has(sites.var[s])) ++s;
		refuse("the sites file has k-mers shared between sites (first at site " + sites.ids[std::min(s, n_sites - 1)] +
		    "); " + (opt.pca.empty() ? "--counts / --store need" : "-p needs") + " -d for such a file");
	}
	if (opt.want_store) {                                           /* a store finds a locus by its ID (eval_store::LocusIndex) */
		std::unordered_set<std::string> seen;
		for (const std::string &id : sites.ids)
			if (!seen.insert(id).second) refuse("the sites file has the locus ID " + id + " twice; --store needs distinct IDs");
	}
	return sites;
}

Genome load_genome(const Opt &opt)               /* the constructor's second half (VCFConvert.hpp:43-58) */
{
	if (opt.verbose > 1) std::cerr << "Loading Reference " << opt.ref << std::endl;
	Genome genome;
	ntsm::SeqReader rd;
	if (!rd.open(opt.ref)) refuse("cannot read the reference file " + opt.ref);
	for (int64_t l = rd.next(); l >= 0; l = rd.next()) {
		genome.id[rd.name()] = (uint32_t) genome.seq.size();
		genome.seq.emplace_back(rd.seq_data(), (size_t) l);
	}
	return genome;
}

struct Header {
	std::vector<std::string> samples;
	std::string matrix_head = "alleleID";              /* the header line of NAME_matrix.tsv: alleleID <TAB> sample ... */
	const char *body = nullptr, *body_end = nullptr;   /* the complete lines after the #CHROM line */
	uint64_t lines = 0;                                /* the lines before them */
};

Header read_header(const ntsm::FileBytes &vcf)   /* VCFConvert::count, :70-93 */
{
	Header h;
	const char *p = vcf.data, *const end = vcf.data + vcf.size;
	for (uint64_t line_no = 1; p < end; ++line_no) {
		const char *nl = (const char *) memchr(p, '\n', (size_t) (end - p));
		const char *b = p, *e = nl ? nl : end;
		p = nl ? nl + 1 : end;
		if (b == e) refuse("line " + std::to_string(line_no) + " of the VCF: empty line");   /* line.at(0) throws */
		if (*b != '#') continue;
		const char *t = (const char *) memchr(b, '\t', (size_t) (e - b));
		if (std::string(b, t ? t : e) != "#CHROM") continue;
		Fields fl;
		fl.split(b, e);
		for (size_t i = 9; i < fl.n_read(); ++i) h.samples.emplace_back(fl.f[i].first, fl.f[i].second);
		break;
	}
	for (const std::string &sm : h.samples) { h.matrix_head += "\t"; h.matrix_head += sm; }
	h.matrix_head += "\n";
	h.lines = (uint64_t) std::count(vcf.data, p, '\n');
	/* body: complete lines only (a last line without '\n' fails fh.good(), :108) */
	h.body = h.body_end = p;
	for (const char *q = end; q > p; --q)
		if (q[-1] == '\n') { h.body_end = q; break; }
	return h;
}

/* the body on T threads (:102-171); the first failure in file order is the refusal, whatever -t */
std::vector<Part> parse_body(const Ctx &ctx, const Header &h, unsigned T)
{
	std::vector<Part> parts(T);
	const ntsm::LineCuts cut = ntsm::cut_lines(h.body, h.body_end, T);
	on_threads(T, [&](unsigned t) { parse_lines(ctx, cut.at[t], cut.at[t + 1], h.lines + 1 + cut.lines_before[t], parts[t]); });
	for (const Part &pt : parts)
		if (pt.failed) refuse(pt.error);
	return parts;
}

struct Events {                              /* the inputs of ntsm_vcf_run (include/ntsm_vcf_hip.h), under its names */
	uint64_t n_lines = 0, n_keys = 0, n_events = 0, n_sites = 0;
	uint32_t g_stride = 0;
	std::vector<uint8_t> geno;
	std::vector<uint64_t> key_off, site_off;
	std::vector<uint32_t> ev_ord, ev_ls, site_keys;
};

/* events in one-thread order -> per-key lists (CSR), ascending ordinals; the parts' genotype rows move into one array */
Events build_events(std::vector<Part> &parts, const ntsm::SiteSet &sites, uint32_t stride)
{
	const unsigned T = (unsigned) parts.size();
	Events ev;
	ev.g_stride = stride;
	for (const Part &pt : parts) { ev.n_events += pt.ev_key.size(); ev.n_lines += pt.used; }
	if (ev.n_events > 0xFFFFFFFFull || ev.n_lines > 0x7FFFFFFFull) refuse("too many window k-mers in the VCF");
	ev.n_keys = sites.keys.size();
	ev.key_off.assign(ev.n_keys + 1, 0);
	for (const Part &pt : parts)
		for (uint32_t q : pt.ev_key) ev.key_off[q + 1]++;
	for (uint64_t q = 0; q < ev.n_keys; ++q) ev.key_off[q + 1] += ev.key_off[q];
	ev.ev_ord.resize(ev.n_events);
	ev.ev_ls.resize(ev.n_events);
	ev.geno.resize((size_t) ev.n_lines * stride);
	std::vector<uint64_t> fill(ev.key_off.begin(), ev.key_off.end() - 1);
	uint64_t ord = 0, line_base = 0;
	std::vector<uint64_t> geno_at(T + 1, 0);
	for (unsigned t = 0; t < T; ++t) {
		const Part &pt = parts[t];
		for (size_t i = 0; i < pt.ev_key.size(); ++i, ++ord) {
			const uint64_t at = fill[pt.ev_key[i]]++;
			ev.ev_ord[at] = (uint32_t) ord;
			ev.ev_ls[at] = (uint32_t) ((line_base + pt.ev_line[i]) * 2 + pt.ev_side[i]);
		}
		line_base += pt.used;
		geno_at[t + 1] = geno_at[t] + pt.geno.size();
	}
	on_threads(T, [&](unsigned t) {
		if (!parts[t].geno.empty()) memcpy(ev.geno.data() + geno_at[t], parts[t].geno.data(), parts[t].geno.size());
		std::vector<uint8_t>().swap(parts[t].geno);
	});
	/* per-site key lists (erased k-mers -- only without -d, and then without -p -- have no events: left out) */
	ev.n_sites = sites.ids.size();
	ev.site_off.assign(2 * ev.n_sites + 1, 0);
	for (size_t s = 0; s < ev.n_sites; ++s)
		for (int side = 0; side < 2; ++side) {
			for (int64_t q : side ? sites.var[s] : sites.ref[s])
				if (q >= 0) ev.site_keys.push_back((uint32_t) q);
			ev.site_off[2 * s + side + 1] = ev.site_keys.size();
		}
	return ev;
}

struct PcaNames { std::vector<ntsm::Name> samples, sites; };   /* views into the matrix header and the site ids */

/* -R: what ntsmPCA refuses from the shape of the matrix alone is refused here, in its words, after every refusal of
 * the VCF and before the device is touched.  The names are read back from the header line as ntsmPCA reads them (a
 * CRLF header's "\r" goes); site ids hold no white space (ntsm::SeqReader), so every row has the header's fields */
PcaNames rotation_shape_check(const Opt &opt, const std::string &head, const ntsm::SiteSet &sites, uint32_t n_samples)
{
	const std::string matrix_name = opt.pca + "_matrix.tsv";
	const size_t n_sites = sites.ids.size();
	PcaNames names { ntsm::header_samples(head.data(), head.data() + head.size() - 1), {} };
	std::string why = ntsm::pca_shape_error(matrix_name, names.samples.size(), n_sites);
	if (why.empty() && names.samples.size() != n_samples) why = "the header of " + matrix_name + " does not read back as its samples";
	if (why.empty()) why = ntsm::pca_dims_high_error(opt.numComp, n_samples, n_sites);
	if (!why.empty()) refuse(why);
	for (const std::string &id : sites.ids) names.sites.push_back(ntsm::Name { id.data(), id.size() });
	return names;
}

struct Step {                                /* the outputs of ntsm_vcf_run; warn in the library's order */
	std::vector<uint16_t> cells;
	std::vector<double> sums;
	std::vector<uint32_t> first_undef;
	std::vector<ntsm_vcf_warning> warn;
};

/* the device step: inserts, maxima, sums (include/ntsm_vcf_hip.h); called again when the warnings need more room */
Step device_step(const Opt &opt, const Events &ev, uint32_t n_samples, bool prof)
{
	Step st { std::vector<uint16_t>((size_t) ev.n_sites * n_samples), std::vector<double>(ev.n_sites), std::vector<uint32_t>(ev.n_sites),
	    std::vector<ntsm_vcf_warning>(1 << 20) };               /* 16 MB: more warnings cost a second call */
	uint64_t n_warn = 0;
	ntsm_vcf_times tm {};
	for (;;) {
		const int rc = ntsm_vcf_run(opt.device, n_samples, opt.multi, ev.n_lines, ev.geno.data(), ev.g_stride, ev.n_keys, ev.key_off.data(),
		    ev.n_events, ev.ev_ord.data(), ev.ev_ls.data(), ev.n_sites, ev.site_off.data(), ev.site_keys.data(), st.cells.data(),
		    st.sums.data(), st.first_undef.data(), st.warn.data(), st.warn.size(), &n_warn, &tm);
		if (rc == NTSM_VCF_E_CAPACITY) { st.warn.resize(n_warn); continue; }
		if (rc) refuse("the HIP device step failed (" + std::to_string(rc) + ")");
		break;
	}
	if (prof) fprintf(stderr, "[vcf] device: upload %.4f s, state kernel %.4f s, sum kernel %.4f s, download %.4f s, kernel bytes %llu, "
	    "state launches %llu\n", tm.upload_ms / 1e3, tm.state_kernel_ms / 1e3, tm.sum_kernel_ms / 1e3, tm.download_ms / 1e3,
	    (unsigned long long) tm.kernel_bytes, (unsigned long long) tm.state_launches);
	st.warn.resize(n_warn);
	return st;
}

/* the insert warnings in the one-thread order; under -v -v -v "Processing site" per line, its warnings after it */
void print_warnings(const Opt &opt, const std::vector<Part> &parts, std::vector<ntsm_vcf_warning> &warn)
{
	std::sort(warn.begin(), warn.end(), [](const ntsm_vcf_warning &a, const ntsm_vcf_warning &b) {
		return a.event != b.event ? a.event < b.event : a.sample < b.sample;
	});
	std::string text;
	auto put = [&](const ntsm_vcf_warning &w) {                 /* MultiCount.hpp:59-60 */
		text += "Warning: Inconsistent k-mer counts, check for overlapping sites: ";
		text += (char) (uint8_t) w.old;
		text += " vs " + std::to_string(w.value) + "\n";
	};
	if (opt.verbose > 2) {
		size_t wi = 0;
		uint64_t ev_end = 0;
		for (const Part &pt : parts)
			for (size_t i = 0; i < pt.rs_id.size(); ++i) {
				text += "Processing site: " + pt.rs_id[i] + "\n";
				ev_end += pt.line_events[i];
				for (; wi < warn.size() && warn[wi].event < ev_end; ++wi) put(warn[wi]);
			}
	} else {
		for (const ntsm_vcf_warning &w : warn) put(w);
	}
	std::cerr << text << std::flush;
}

/* printNormMatrix's text (MultiCount.hpp:148-201) from the device step's cells: the matrix writer and -R both read it here */
struct MatrixText {
	const uint32_t n_samples;
	const uint16_t *const cells;
	uint64_t first_undef_cell = ~0ull;               /* row-major; ~0: none */
	std::vector<std::string> centre, tab[2];         /* per site; per form (6 / 19 digits) the text of every code that can occur */
	MatrixText(const Opt &opt, const Step &st, uint32_t n) : n_samples(n), cells(st.cells.data()), centre(st.sums.size())
	{
		const size_t n_sites = st.sums.size();
		for (size_t s = 0; s < n_sites && first_undef_cell == ~0ull; ++s)
			if (st.first_undef[s] < n_samples) first_undef_cell = (uint64_t) s * n_samples + st.first_undef[s];
		for (size_t s = 0; s < n_sites; ++s) centre[s] = centre_text(st.sums[s], n_samples);
		tab[0].resize(65536);
		tab[1].resize(65536);
		const unsigned bv[3] = { 0u, opt.multi & 255u, (opt.multi * 2u) & 255u };   /* the bytes 0, (uint8_t) m, (uint8_t) 2m */
		for (unsigned r : bv)
			for (unsigned v : bv)
				if (r + v) { tab[0][r | v << 8] = cell_text(r, v, kShortDigits); tab[1][r | v << 8] = cell_text(r, v, kLongDigits); }
	}
	/* the text of cell (s, j): an undefined cell is its row's centre; the stream's precision is 19 after the first
	 * undefined cell, 6 up to and including it */
	void append_cell(std::string &o, size_t s, uint32_t j) const
	{
		const unsigned c = cells[s * n_samples + j];
		if ((c & 255u) + (c >> 8) == 0) { o += centre[s]; return; }
		const int long_form = (uint64_t) s * n_samples + j > first_undef_cell;
		const std::string &x = tab[long_form][c];
		if (!x.empty()) o += x;
		else o += cell_text(c & 255u, c >> 8, long_form ? kLongDigits : kShortDigits);
	}
};

struct Rotation { std::vector<double> rot, comp; uint32_t dims; };

/* -R: the PCA, before anything is written (a refusal writes nothing) */
Rotation run_rotation(const Opt &opt, const Step &st, const MatrixText &text, size_t n_sites, uint32_t n_samples, bool prof)
{
	const uint32_t dims = (uint32_t) opt.numComp;
	Rotation r { std::vector<double>((size_t) n_sites * dims), std::vector<double>((size_t) n_samples * dims), dims };
	/* the matrix the PCA sees is the text's: a code's value is what ntsmPCA reads back from the code's text, an undefined
	 * cell's from the row's centre text.  A code outside the table cannot occur (the device step writes only those bytes);
	 * its value is NaN, which the eigen step's rank test refuses */
	std::vector<double> value(2 * 65536, std::numeric_limits<double>::quiet_NaN()), row_fill(n_sites), eigval(dims);
	for (int form = 0; form < 2; ++form)
		for (unsigned c = 1; c < 65536; ++c)
			if (!text.tab[form][c].empty()) value[(size_t) form * 65536 + c] = text_value(text.tab[form][c]);
	for (size_t s = 0; s < n_sites; ++s) row_fill[s] = text_value(text.centre[s]);
	if (opt.verbose) std::cerr << "Matrix: " << n_sites << " sites x " << n_samples << " samples, " << dims << " components" << std::endl;
	uint32_t bad = 0;
	double expand_ms = 0.0;
	ntsm_pca_times ptm {};
	const int rc = ntsm_pca_run_cells(opt.device, n_sites, n_samples, st.cells.data(), value.data(), row_fill.data(), text.first_undef_cell,
	    dims, 0, eigval.data(), r.rot.data(), r.comp.data(), &bad, &ptm, &expand_ms);
	if (rc != 0) refuse(ntsm::pca_run_error(rc, bad, dims, opt.device));
	if (opt.verbose || prof) ntsm::pca_print_times(stderr, ptm, &expand_ms);
	return r;
}

/* printNormMatrix's two files (:148-201), both opened before either is written; the rows are formatted on T threads */
void write_outputs(const Opt &opt, const std::string &head, const std::vector<std::string> &ids, const MatrixText &text, uint32_t n_samples)
{
	FILE *out = opt.no_matrix ? nullptr : fopen((opt.pca + "_matrix.tsv").c_str(), "wb");
	FILE *cf = fopen((opt.pca + "_center.txt").c_str(), "wb");
	if ((!out && !opt.no_matrix) || !cf) refuse("cannot write " + opt.pca + "_matrix.tsv / _center.txt");
	if (out) fwrite(head.data(), 1, head.size(), out);
	const unsigned T = opt.T;
	const size_t n_sites = ids.size();
	const size_t batch = std::max<size_t>(1, (size_t) (64u << 20) / ((size_t) n_samples * 8 + 64));   /* ~64 MB of text per thread */
	std::vector<std::string> part(T);
	for (size_t s0 = 0; out && s0 < n_sites; s0 += batch * T) {
		on_threads(T, [&](unsigned t) {
			std::string &o = part[t];
			o.clear();
			const size_t lo = std::min(n_sites, s0 + batch * t), hi = std::min(n_sites, s0 + batch * (t + 1));
			for (size_t s = lo; s < hi; ++s) {
				o += ids[s];
				for (uint32_t j = 0; j < n_samples; ++j) { o += '\t'; text.append_cell(o, s, j); }
				o += '\n';
			}
		});
		for (unsigned t = 0; t < T; ++t) fwrite(part[t].data(), 1, part[t].size(), out);
	}
	std::string ctext;
	for (const std::string &c : text.centre) { ctext += c; ctext += "\n"; }
	fwrite(ctext.data(), 1, ctext.size(), cf);
	const bool ok = !out || fclose(out) == 0;
	if (fclose(cf) != 0 || !ok) refuse("writing " + opt.pca + "_matrix.tsv / _center.txt failed");
}

/* ---- --counts / --store: the records of ntsm_vcf_records as counts files and as a cohort store ------------------------------ */

namespace store = ntsm::eval_store;

struct RecordsPlan {                         /* what --counts / --store decide from the inputs alone, before the device */
	std::vector<std::string> paths;          /* --counts: DIR/SAMPLE.counts.txt per sample */
	std::vector<std::string> names;          /* --store: the record names (those paths, or the sample IDs) */
	std::vector<uint32_t> distinct;          /* [n_sites][2]: the sizes of the allele lists (printCountsMax's last columns) */
	store::Header head {};                   /* of the store as it is now (n_samples = 0 for one to create) */
	bool store_exists = false;
	uint32_t window = 16;                    /* samples per call of the device step */
};

constexpr uint64_t kWindowBytes = 256ull << 20;   /* records of one window: the host buffer does not grow with the cohort */

RecordsPlan plan_records(const Opt &opt, const ntsm::SiteSet &sites, const std::vector<std::string> &samples)
{
	RecordsPlan plan;
	if (samples.empty()) refuse("the VCF's header has no samples: --counts / --store have nothing to write");
	struct stat st;
	if (opt.want_counts) {
		for (const std::string &id : samples)
			if (id.empty() || id.find('/') != std::string::npos)
				refuse("the sample ID '" + id + "' cannot name a counts file (it is empty or contains '/')");
		if (stat(opt.counts_dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode)) refuse("--counts: " + opt.counts_dir + " is not a directory");
		for (const std::string &id : samples) plan.paths.push_back(opt.counts_dir + "/" + id + ".counts.txt");
	}
	const std::vector<std::string> &names = opt.want_counts ? plan.paths : samples;
	std::unordered_set<std::string> seen;
	try {
		for (const std::string &n : names) {
			store::check_name(n);
			if (!seen.insert(n).second) refuse("two samples are named " + n);
		}
		const size_t n_sites = sites.ids.size();
		for (size_t s = 0; s < n_sites; ++s) {
			plan.distinct.push_back((uint32_t) sites.ref[s].size());
			plan.distinct.push_back((uint32_t) sites.var[s].size());
		}
		plan.head = store::new_header(sites.ids);
		if (opt.want_store) {
			plan.names = names;
			plan.store_exists = stat(opt.store.c_str(), &st) == 0;
			if (plan.store_exists) {
				store::View v;
				v.open(opt.store);
				if (v.locus != sites.ids || (n_sites && memcmp(v.distinct, plan.distinct.data(), 8 * n_sites) != 0))
					refuse("the loci of the store " + opt.store + " (IDs and distinct columns) are not those of " + opt.snp);
				for (uint64_t r = 0; r < v.h.n_samples; ++r)
					if (seen.count(v.name(r))) refuse("the name " + v.name(r) + " is already in the store");
				plan.head = v.h;
			}
		}
	} catch (const store::Error &e) {
		refuse(e.what());
	}
	const bool dir_writable = !opt.want_counts || access(opt.counts_dir.c_str(), W_OK | X_OK) == 0;
	for (const std::string &p : plan.paths)                      /* a counts file that cannot be written, as far as a look tells */
		if (!dir_writable || (stat(p.c_str(), &st) == 0 && !S_ISREG(st.st_mode))) refuse("cannot write " + p);
	uint64_t window = std::max<uint64_t>(16, kWindowBytes / plan.head.stride / 16 * 16);
	if (const char *w = getenv("NTSM_VCF_STORE_WINDOW")) {       /* samples; a test forces several windows with it */
		unsigned long long v = 0;
		if (!ntsm::read_whole(w, v) || v < 1) refuse("NTSM_VCF_STORE_WINDOW=" + std::string(w) + " is not a number of samples");
		window = std::max<uint64_t>(16, std::min<uint64_t>(v, 1u << 30) / 16 * 16);
	}
	plan.window = (uint32_t) std::min<uint64_t>(window, (samples.size() + 15) / 16 * 16);
	return plan;
}

inline void append_number(std::string &o, uint32_t v)       /* std::to_string's digits, without its temporary */
{
	char b[10];
	int n = 0;
	do { b[n++] = (char) ('0' + v % 10); v /= 10; } while (v);
	while (n) o += b[--n];
}

/* printCountsMax's bytes for one sample (MultiCount.hpp:93-138); counts and sums are the sample's [n_sites][2] */
void counts_text(std::string &o, const std::vector<std::string> &ids, const uint32_t *counts, const uint32_t *sums, const uint32_t *distinct)
{
	o = "\n#locusID\tcountAT\tcountCG\tsumAT\tsumCG\tdistinctAT\tdistinctCG\n";
	for (size_t s = 0; s < ids.size(); ++s) {
		o += ids[s];
		for (const uint32_t *v : { counts, sums, distinct })
			for (int c = 0; c < 2; ++c) { o += '\t'; append_number(o, v[2 * s + c]); }
		o += '\n';
	}
}

/* The samples in windows: device step, then the window's counts files (formatted and written on T threads) and its store
 * records.  The store changes last: a new one is STORE.tmp until it is renamed, an old one gets its sample count when
 * every record is behind the last one; a failure on the way removes STORE.tmp or cuts the old store back to its size. */
void write_records(const Opt &opt, const RecordsPlan &plan, const Events &ev, const std::vector<std::string> &ids, uint32_t n_samples, bool prof)
{
	const size_t n_sites = ids.size();
	const uint64_t stride = plan.head.stride, old_size = plan.head.first + plan.head.n_samples * stride;
	const std::string tmp = opt.store + ".tmp", &target = plan.store_exists ? opt.store : tmp;
	bool store_open = false;
	const auto fail = [&](const std::string &why) {
		if (store_open && !plan.store_exists) unlink(tmp.c_str());
		if (store_open && plan.store_exists && truncate(opt.store.c_str(), (off_t) old_size) != 0) std::cerr << "cannot restore " << opt.store << std::endl;
		refuse(why);
	};
	store::Appender to;
	std::vector<char> recs((size_t) plan.window * stride);
	std::vector<uint32_t> sums(opt.want_counts ? (size_t) plan.window * 2 * n_sites : 0);
	std::vector<uint64_t> total(plan.window), sum_of_sums(plan.window);
	std::vector<std::string> text(opt.T), failed(opt.T);
	double dev_s[3] = { 0, 0, 0 }, text_s = 0, store_s = 0;
	uint64_t kernel_bytes = 0, n_windows = 0;
	const auto now = [] { return std::chrono::steady_clock::now(); };
	const auto since = [&](std::chrono::steady_clock::time_point t) { return std::chrono::duration<double>(now() - t).count(); };
	try {
		if (opt.want_store) {
			if (!plan.store_exists) {                                /* header (n_samples still 0) and locus section */
				const int fd = open(tmp.c_str(), O_CREAT | O_TRUNC | O_RDWR, 0644);
				if (fd < 0) refuse("cannot write " + tmp);
				store_open = true;
				const bool ok = store::write_head(fd, plan.head, ids, plan.distinct.data());
				close(fd);
				if (!ok) fail("cannot write " + tmp);
			}
			to.open(target, plan.head);
			store_open = true;
		}
		for (uint32_t s_begin = 0; s_begin < n_samples; s_begin += plan.window, ++n_windows) {
			const uint32_t cnt = std::min(plan.window, n_samples - s_begin);
			std::fill(recs.begin(), recs.begin() + (size_t) cnt * stride, 0);
			ntsm_vcf_records_times tm {};
			const int rc = ntsm_vcf_records(opt.device, n_samples, opt.multi, ev.n_lines, ev.geno.data(), ev.g_stride, ev.n_keys, ev.key_off.data(),
			    ev.n_events, ev.ev_ord.data(), ev.ev_ls.data(), ev.n_sites, ev.site_off.data(), ev.site_keys.data(), s_begin, cnt,
			    (uint32_t *) (recs.data() + store::kRecordHead), stride, opt.want_counts ? sums.data() : nullptr, 8 * n_sites, total.data(),
			    sum_of_sums.data(), &tm);
			if (rc) fail("the HIP records step failed (" + std::to_string(rc) + ")");
			dev_s[0] += tm.upload_ms / 1e3; dev_s[1] += tm.kernel_ms / 1e3; dev_s[2] += tm.download_ms / 1e3;
			kernel_bytes += tm.kernel_bytes;
			auto t0 = now();
			if (opt.want_counts) {
				on_threads(opt.T, [&](unsigned t) {
					for (uint32_t j = t; j < cnt && failed[t].empty(); j += opt.T) {
						counts_text(text[t], ids, (const uint32_t *) (recs.data() + (size_t) j * stride + store::kRecordHead),
						    sums.data() + (size_t) j * 2 * n_sites, plan.distinct.data());
						const std::string &path = plan.paths[s_begin + j];
						FILE *f = fopen(path.c_str(), "wb");
						const bool ok = f && fwrite(text[t].data(), 1, text[t].size(), f) == text[t].size();
						if ((f && fclose(f) != 0) || !ok) failed[t] = path;
					}
				});
				for (const std::string &path : failed)
					if (!path.empty()) fail("cannot write " + path);
				text_s += since(t0);
				t0 = now();
			}
			if (opt.want_store) {
				for (uint32_t j = 0; j < cnt; ++j)                       /* no #@TK / #@KS line in such a file: raw_total = kmer_size = 0 */
					store::fill_record_head(recs.data() + (size_t) j * stride, plan.names[s_begin + j], 0, 0, total[j], sum_of_sums[j]);
				to.write(recs.data(), (size_t) cnt * stride);
				store_s += since(t0);
			}
		}
		if (opt.want_store) {
			const auto t0 = now();
			to.commit(n_samples);
			if (!plan.store_exists && rename(tmp.c_str(), opt.store.c_str()) != 0) fail("cannot rename " + tmp + " to " + opt.store);
			store_s += since(t0);
		}
	} catch (const store::Error &e) {
		fail(e.what());
	}
	if (prof) {
		fprintf(stderr, "[vcf] records device: windows %llu of %u samples, upload %.4f s, kernel %.6f s, download %.4f s, kernel bytes %llu\n",
		    (unsigned long long) n_windows, plan.window, dev_s[0], dev_s[1], dev_s[2], (unsigned long long) kernel_bytes);
		if (opt.want_counts) fprintf(stderr, "[vcf] counts format + write: %.4f s\n", text_s);
		if (opt.want_store) fprintf(stderr, "[vcf] store write: %.4f s\n", store_s);
	}
}

} // namespace

/* The order is the contract: every refusal of the inputs before the device, nothing written before -R's PCA has succeeded */
int main(int argc, char **argv)
{
	const Opt opt = read_options(argc, argv);
	ntsm::LapTimer timer { "[vcf]", getenv("NTSM_VCF_PROF") != nullptr };   /* phase times on stderr (tools/vcf_bench.py) */
	const ntsm::SiteSet sites = load_sites(opt);
	timer.lap("sites");
	const Genome genome = load_genome(opt);
	timer.lap("genome");
	if (opt.verbose > 1) std::cerr << "Reading VCF file: " << opt.inputs[0] << std::endl;
	ntsm::FileBytes vcf;                         /* a directory reads as an empty VCF */
	if (!vcf.load(opt.inputs[0], opt.T, ntsm::FileBytes::kDirectoryIsEmpty)) refuse("cannot read the VCF file " + opt.inputs[0]);
	const Header header = read_header(vcf);
	const uint32_t n_samples = (uint32_t) header.samples.size(), stride = (n_samples + 15) / 16 * 16;
	if (opt.verbose > 1) std::cerr << "Starting multicount of each rsID for " << n_samples << " samples." << std::endl;
	const RecordsPlan plan = opt.records() ? plan_records(opt, sites, header.samples) : RecordsPlan();
	const KeyTable table(sites.keys);
	std::vector<Part> parts = parse_body(Ctx { opt, genome, table, n_samples, stride }, header, opt.T);
	timer.lap("parse");
	const Events events = build_events(parts, sites, stride);
	timer.lap("events");
	const PcaNames names = opt.rotation ? rotation_shape_check(opt, header.matrix_head, sites, n_samples) : PcaNames();
	Step step = device_step(opt, events, n_samples, timer.on);
	timer.lap("device step (total)");
	print_warnings(opt, parts, step.warn);
	if (opt.pca.empty()) {
		if (opt.verbose > 1) std::cerr << "Outputting counts" << std::endl;
	} else {
		for (int i = 0; i < 2 && opt.verbose > 1; ++i) std::cerr << "Outputting matrix and normalization values for PCA" << std::endl;
		const MatrixText text(opt, step, n_samples);
		Rotation rotation {};
		if (opt.rotation) {
			timer.lap("cell and centre text");
			rotation = run_rotation(opt, step, text, sites.ids.size(), n_samples, timer.on);
			timer.lap("pca (total)");
		}
		write_outputs(opt, header.matrix_head, sites.ids, text, n_samples);
		timer.lap("format + write");
		if (opt.rotation) {
			const std::string bad_path = ntsm::write_pca_tables(opt.pca, names.sites, names.samples, rotation.rot.data(), rotation.comp.data(),
			    rotation.dims, opt.T);
			if (!bad_path.empty()) refuse("cannot write " + bad_path);
			timer.lap("rotation + components write");
		}
	}
	if (opt.records()) {                         /* after -p's files: nothing of these is written before a -R PCA has succeeded */
		write_records(opt, plan, events, sites.ids, n_samples, timer.on);
		timer.lap("records (total)");
	}
	std::cerr << "Time: " << timer.total() << " s Memory: " << rss_kbytes() << " kbytes" << std::endl;
	return 0;
}
