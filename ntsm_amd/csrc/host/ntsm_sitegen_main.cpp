/*
 * ntsm_sitegen_main.cpp -- build/ntsmSiteGen: sites files (-s of ntsmCount, ntsmVCF, ntsmEval) from a genome and a VCF of
 * SNPs.  The port of upstream's `ntsmSiteGen generate-sites` (ntsm-scripts/makefile), DESIGN.md section 13:
 *
 *   step 1 (host)    candidate sub-k-mers of the SNP windows      contract: ntsm-scripts/extractSNPsfromVCF.py
 *   step 2 (device)  per candidate, the places of the genome within x substitutions (include/ntsm_sitegen_hip.h);
 *                    with -g, the places with a one-base gap as well (include/ntsm_sitegen_gap_hip.h), in one pass;
 *                    upstream: bwa index / aln -n 1 / samse.  -H reads the counts from a file and leaves the GPU alone
 *   step 3 (host)    keep the candidates with at most one place, write NAME_n{i}.fa    contract: filterRepetiveSNP.pl
 *
 * Nothing is written before the hit counts are there: every refusal (`Error: ...`, exit 1) comes earlier and leaves no
 * file behind.
 */
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/ntsm_sitegen_gap_hip.h"
#include "../../../include/ntsm_sitegen_hip.h"
#include "seq_reader.hpp"

namespace {

struct Options {
	std::string ref, vcf, prefix, hits;
	long k = 19, w = 31, threads = 4, x = 1, device = 0;
	long e = -1;                             /* -e / gapskip=: the end margin of -g; -1 = not given (5) */
	bool gaps = false;                       /* -g / gaps=1 */
	bool at_cg_only = true;                  /* the script's `ignore`, cleared by -i */
	int verbose = 0;
};

struct Record {
	std::string name, seq;
};

struct Entry {                              /* one value of the script's _vcfEntries dict */
	std::string id, chr, wt, var;
	long long pos = 0;
};

struct Candidate {
	uint32_t entry;
	uint16_t pos;
	uint8_t cg;                              /* 0: the AT line, 1: the CG line */
	uint64_t kmer;                           /* packed as include/ntsm_sitegen_hip.h says */
};

[[noreturn]] void fail(const std::string &msg)
{
	std::cerr << "Error: " << msg << std::endl;
	exit(1);
}

void usage()
{
	std::cerr << "Usage: ntsmSiteGen -r GENOME.fa[.gz] -v SNPS.vcf -p NAME [-k 19] [-w 31] [-t 4] [-i] [-x 1] [-g [-e 5]] [-H HITS.tsv] [-G 0] [-V]\n"
	             "       ntsmSiteGen generate-sites name=NAME ref=GENOME.fa vcf=SNPS.vcf [k=19] [w=31] [t=4] [gaps=1 [gapskip=5]] [hits=HITS.tsv]\n"
	             "  -r  reference genome, FASTA, plain or gzip\n"
	             "  -v  VCF of the SNPs (columns CHROM POS ID REF ALT are read)\n"
	             "  -p  prefix of the output files NAME_subKmers.fa, NAME_subKmerHits.tsv, NAME_n0.fa .. NAME_n{w-k}.fa\n"
	             "  -k  k-mer size (1 .. 31; the device step needs 11 .. 31)    -w  window size (>= k)\n"
	             "  -i  keep A/T <-> A/T and C/G <-> C/G SNPs\n"
	             "  -x  substitutions allowed when places of the genome are counted: 0 or 1\n"
	             "  -g  count the places that differ by a one-base gap too, as `bwa aln -n 1` does (gaps=1); needs -x 1\n"
	             "  -e  with -g: no gap within this many bases of either end of the k-mer, 1 .. (k - 1) / 2, default 5 (gapskip=N)\n"
	             "  -H  take the hit counts from this file (the form of NAME_subKmerHits.tsv); the GPU is not used\n"
	             "  -t  host threads (never changes the output)    -G  device    -V  timings on stderr\n";
}

bool parse_long(const char *s, long &out)
{
	char *end = nullptr;
	errno = 0;
	long v = strtol(s, &end, 10);
	if (errno || end == s || *end)
		return false;
	out = v;
	return true;
}

int code_of(char c)
{
	switch (c) {
	case 'A': return 0;
	case 'C': return 1;
	case 'G': return 2;
	case 'T': return 3;
	default: return -1;
	}
}

bool py_space(char c) { return c == ' ' || (c >= '\t' && c <= '\r') || (c >= 0x1c && c <= 0x1f); }

/* Python's int(str): optional blanks, optional sign, decimal digits (underscores are not taken) */
bool py_int(const std::string &s, long long &out)
{
	size_t a = 0, b = s.size();
	while (a < b && py_space(s[a])) a++;
	while (b > a && py_space(s[b - 1])) b--;
	bool neg = false;
	if (a < b && (s[a] == '+' || s[a] == '-')) neg = s[a++] == '-';
	if (a == b || b - a > 15)
		return false;
	long long v = 0;
	for (; a < b; a++) {
		if (s[a] < '0' || s[a] > '9')
			return false;
		v = v * 10 + (s[a] - '0');
	}
	out = neg ? -v : v;
	return true;
}

std::vector<Record> read_genome(const std::string &path)
{
	ntsm::SeqReader rd;
	if (!rd.open(path))
		fail("cannot open " + path);
	std::vector<Record> recs;
	int64_t len;
	while ((len = rd.next()) >= 0) {
		recs.emplace_back();
		recs.back().name = rd.name();
		recs.back().seq.assign(rd.seq_data(), (size_t)len);
	}
	if (len != -1)
		fail("cannot read " + path);
	return recs;
}

/* _parseVCF: the dict keeps the first line's place for an ID and the last line's values */
std::vector<Entry> parse_vcf(const std::string &path)
{
	std::ifstream in(path, std::ios::binary);
	if (!in)
		fail("cannot open " + path);
	std::vector<Entry> entries;
	std::unordered_map<std::string, size_t> at;
	std::string line;
	long long counter = 0, lineno = 0;
	while (std::getline(in, line)) {
		lineno++;
		const std::string where = " (" + path + " line " + std::to_string(lineno) + ")";
		if (!line.empty() && line[0] == '#')
			continue;
		while (!line.empty() && py_space(line.back()))
			line.pop_back();
		std::vector<std::string> f;
		size_t p = 0;
		for (;;) {
			size_t q = line.find('\t', p);
			f.push_back(line.substr(p, q == std::string::npos ? q : q - p));
			if (q == std::string::npos)
				break;
			p = q + 1;
		}
		if (f.size() < 5)
			fail("VCF line with fewer than five fields" + where);
		Entry e;
		e.id = f[2];
		if (e.id == ".")
			e.id = std::to_string(counter++);
		if (e.id.empty())
			fail("empty ID" + where);
		if (f[4].size() > 1)
			fail("Multiple alternate alleles found in VCF");
		if (f[4].empty())
			fail("empty ALT" + where);
		if (!py_int(f[1], e.pos))
			fail("POS is not an integer: " + f[1] + where);
		e.chr = f[0];
		e.wt = f[3];
		e.var = f[4];
		auto it = at.find(e.id);
		if (it == at.end()) {
			at.emplace(e.id, entries.size());
			entries.push_back(std::move(e));
		} else
			entries[it->second] = std::move(e);
	}
	return entries;
}

uint64_t pack(const char *s, long k)
{
	uint64_t v = 0;
	for (long i = 0; i < k; i++)
		v = (v << 2) | (uint64_t)code_of(s[i]);
	return v;
}

uint64_t canonical(uint64_t fw, long k)
{
	uint64_t rv = 0, q = fw;
	for (long i = 0; i < k; i++) {
		rv = (rv << 2) | (3 - (q & 3));
		q >>= 2;
	}
	return fw < rv ? fw : rv;
}

bool at_base(char c) { return c == 'A' || c == 'T'; }
bool cg_base(char c) { return c == 'C' || c == 'G'; }

struct Step1 {
	std::vector<Candidate> cands;
	std::vector<std::string> tmp, mod;       /* per entry: the window and the window with the variant, empty when skipped */
	std::string err;                         /* the script's stderr */
};

Step1 step1(const Options &opt, const std::vector<Record> &genome, const std::vector<Entry> &entries)
{
	const long w = opt.w, k = opt.k, half = w / 2, n_sub = w - k + 1;
	std::unordered_map<std::string, size_t> by_name;
	for (size_t i = 0; i < genome.size(); i++)
		if (!by_name.emplace(genome[i].name, i).second)
			fail("record name twice in the genome: " + genome[i].name);
	Step1 r;
	r.tmp.resize(entries.size());
	r.mod.resize(entries.size());
	std::unordered_map<uint64_t, uint32_t> count;
	std::ostringstream err;
	/* first pass: windows, the "does not match" lines, and the count of every sub-k-mer by canonical value */
	for (size_t i = 0; i < entries.size(); i++) {
		const Entry &e = entries[i];
		auto it = by_name.find(e.chr);
		if (it == by_name.end())
			fail("chromosome " + e.chr + " of SNP " + e.id + " is not in the genome");
		const std::string &seq = genome[it->second].seq;
		const long long offset = e.pos - 1, pos1 = offset - half;   /* ceil(offset - w / 2) */
		if (pos1 < 0 || pos1 + w > (long long)seq.size())
			fail("the window of SNP " + e.id + " (" + e.chr + ":" + std::to_string(e.pos) + ") does not lie inside its chromosome");
		std::string tmp = seq.substr((size_t)pos1, (size_t)w);
		for (char &c : tmp)
			if (c >= 'a' && c <= 'z')
				c = (char)(c - 32);
		if (e.wt.size() != 1 || e.wt[0] != tmp[half]) {
			err << "Wildtype allele does not match\nref:" << e.wt << "\nvar:" << e.var << "\nfasta:" << seq[(size_t)offset] << "\nkmer:" << tmp << "\n";
			continue;
		}
		const char wt = e.wt[0], var = e.var[0];
		if (opt.at_cg_only && ((at_base(wt) && at_base(var)) || (cg_base(wt) && cg_base(var))))
			continue;
		for (char c : tmp)
			if (code_of(c) < 0)
				fail("the window of SNP " + e.id + " holds a character outside ACGT: " + tmp);
		if (code_of(var) < 0)
			fail("the ALT of SNP " + e.id + " is not one of ACGT: " + e.var);
		std::string mod = tmp;
		mod[half] = var;
		for (long p = 0; p < n_sub; p++) {
			count[canonical(pack(tmp.data() + p, k), k)]++;
			count[canonical(pack(mod.data() + p, k), k)]++;
		}
		r.tmp[i] = std::move(tmp);
		r.mod[i] = std::move(mod);
	}
	/* second pass: the candidates and the script's counters */
	long long removed = 0, processed = 0, filtered = 0, kmers_removed = 0;
	for (size_t i = 0; i < entries.size(); i++) {
		const Entry &e = entries[i];
		if (r.tmp[i].empty()) {
			removed++;
			const std::string &seq = genome[by_name[e.chr]].seq;
			char centre = seq[(size_t)(e.pos - 1)];
			if (centre >= 'a' && centre <= 'z')
				centre = (char)(centre - 32);
			if (e.wt.size() == 1 && e.wt[0] == centre)
				filtered++;                       /* the wild type matched: the A/T <-> C/G rule skipped it */
			continue;
		}
		const long long before = kmers_removed;
		const bool wt_is_at = at_base(e.wt[0]);
		for (long p = 0; p < n_sub; p++) {
			const uint64_t kt = pack(r.tmp[i].data() + p, k), km = pack(r.mod[i].data() + p, k);
			const uint64_t first = wt_is_at ? kt : km, second = wt_is_at ? km : kt;
			if (count[canonical(first, k)] == 1)
				r.cands.push_back({(uint32_t)i, (uint16_t)p, 0, first});
			else
				kmers_removed++;
			if (count[canonical(second, k)] == 1)
				r.cands.push_back({(uint32_t)i, (uint16_t)p, 1, second});
			else
				kmers_removed++;
		}
		if (kmers_removed - before == n_sub)
			removed++;
		processed++;
	}
	err << "Processed " << processed << " SNPs. Removed " << removed << " SNPs. " << kmers_removed << " duplicate k-mers removed.\n";
	if (filtered > 0)
		err << "Filtered " << filtered << " SNPs that did not have A/T to C/G variants\n";
	r.err = err.str();
	return r;
}

std::string unpack(uint64_t v, long k)
{
	std::string s((size_t)k, 'A');
	for (long i = k - 1; i >= 0; i--) {
		s[(size_t)i] = "ACGT"[v & 3];
		v >>= 2;
	}
	return s;
}

std::string cand_name(const std::vector<Entry> &entries, const Candidate &c)
{
	return entries[c.entry].id + "|" + std::to_string(c.pos) + "|" + (c.cg ? "CG" : "AT");
}

/* the filter's /([^\|]+)\|(\d+)\|(AT|CG)/ on a candidate name, leftmost match: false when nothing matches */
bool filter_parse(const std::string &name, std::string &id, int &cg)
{
	size_t s = 0;
	const size_t n = name.size();
	while (s < n) {
		if (name[s] == '|') {
			s++;
			continue;
		}
		size_t p = name.find('|', s);
		if (p == std::string::npos)
			return false;
		size_t d = p + 1;
		while (d < n && name[d] >= '0' && name[d] <= '9')
			d++;
		if (d > p + 1 && d + 2 < n && name[d] == '|') {
			const bool is_at = name[d + 1] == 'A' && name[d + 2] == 'T', is_cg = name[d + 1] == 'C' && name[d + 2] == 'G';
			if (is_at || is_cg) {
				id = name.substr(s, p - s);
				cg = is_cg;
				return true;
			}
		}
		s = p + 1;
	}
	return false;
}

struct Side {
	bool seen = false;
	bool has_str = false;
	long missing = 0;
	std::string str;
};

/* buffered output file: by the time one is opened every refusal is behind us */
struct Out {
	FILE *f = nullptr;
	std::string path;
	explicit Out(const std::string &p) : path(p)
	{
		if (!(f = fopen(p.c_str(), "wb")))
			fail("cannot write " + p);
	}
	void put(const std::string &text)
	{
		if (fwrite(text.data(), 1, text.size(), f) != text.size())
			fail("cannot write " + path);
	}
	void close()
	{
		if (f && fclose(f))
			fail("cannot write " + path);
		f = nullptr;
	}
	~Out() { if (f) fclose(f); }
	Out(const Out &) = delete;
	Out &operator=(const Out &) = delete;
};

/* step 3: writes NAME_n0.fa .. NAME_n{w-k}.fa */
void step3(const Options &opt, const std::vector<Entry> &entries, const std::vector<Candidate> &cands, const std::vector<uint32_t> &hits)
{
	const long n_sub = opt.w - opt.k + 1;
	std::map<std::string, Side[2]> ids;      /* std::string orders byte-wise, as Perl's sort does */
	for (size_t c = 0; c < cands.size(); c++) {
		const std::string name = cand_name(entries, cands[c]);
		std::string id;
		int cg = 0;
		if (!filter_parse(name, id, cg)) {
			std::cerr << "unable to parse: " << name << "\n";
			continue;
		}
		Side &s = ids[id][cg];
		if (!s.seen) {
			s.seen = true;
			s.missing = n_sub;
		}
		if (hits[c] > 1)
			continue;
		if (s.has_str)
			s.str += 'N';
		s.str += unpack(cands[c].kmer, opt.k);
		s.has_str = true;
		s.missing--;
	}
	std::vector<std::unique_ptr<Out>> files;
	for (long i = 0; i < n_sub; i++)
		files.emplace_back(new Out(opt.prefix + "_n" + std::to_string(i) + ".fa"));
	for (const auto &kv : ids) {
		const Side &at = kv.second[0], &cg = kv.second[1];
		if (!at.seen || !cg.seen || !at.has_str || !cg.has_str)
			continue;
		const std::string text = ">" + kv.first + " ref\n" + at.str + "\n>" + kv.first + " var\n" + cg.str + "\n";
		for (long i = std::max(at.missing, cg.missing); i < n_sub; i++)
			files[(size_t)i]->put(text);
	}
	for (auto &f : files)
		f->close();
}

std::vector<uint32_t> read_hits(const Options &opt, const std::vector<Entry> &entries, const std::vector<Candidate> &cands)
{
	std::ifstream in(opt.hits, std::ios::binary);
	if (!in)
		fail("cannot open " + opt.hits);
	std::vector<uint32_t> hits;
	hits.reserve(cands.size());
	std::string line;
	while (std::getline(in, line)) {
		const size_t c = hits.size();
		if (c >= cands.size())
			fail(opt.hits + " has more lines than there are candidates (" + std::to_string(cands.size()) + ")");
		const size_t tab = line.find('\t');
		long v = 0;
		if (tab == std::string::npos || !parse_long(line.c_str() + tab + 1, v) || v < 0)
			fail(opt.hits + " line " + std::to_string(c + 1) + ": expected NAME <tab> HITS");
		const std::string name = cand_name(entries, cands[c]);
		if (line.compare(0, tab, name) != 0)
			fail(opt.hits + " line " + std::to_string(c + 1) + ": candidate " + line.substr(0, tab) + " where " + name + " was computed");
		hits.push_back((uint32_t)v);
	}
	if (hits.size() != cands.size())
		fail(opt.hits + " has " + std::to_string(hits.size()) + " lines, there are " + std::to_string(cands.size()) + " candidates");
	return hits;
}

double now_ms()
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

/* what either device run begins with: the refusal of a k the libraries do not take, and the candidates as they take them */
std::vector<uint64_t> device_candidates(const Options &opt, const std::vector<Candidate> &cands)
{
	if (opt.k < 11)
		fail("the device step needs k >= 11 (use -H for smaller k)");
	std::vector<uint64_t> packed(cands.size());
	for (size_t i = 0; i < cands.size(); i++)
		packed[i] = cands[i].kmer;
	return packed;
}

/* every record of the genome, one submit each, through the library whose submit function and its name are given */
template <typename Session>
void submit_genome(const std::vector<Record> &genome, Session *s, int (*submit)(Session *, const char *, uint64_t, const uint64_t *, uint64_t), const char *name)
{
	for (const Record &r : genome) {
		const uint64_t end = r.seq.size();
		if (const int rc = submit(s, r.seq.data(), end, &end, 1))
			fail(std::string(name) + " failed (" + std::to_string(rc) + ")");
	}
}

std::vector<uint32_t> device_hits(const Options &opt, const std::vector<Record> &genome, const std::vector<Candidate> &cands)
{
	const std::vector<uint64_t> packed = device_candidates(opt, cands);
	ntsm_sitegen *s = nullptr;
	int rc = ntsm_sitegen_open((int)opt.device, (uint32_t)opt.k, (uint32_t)opt.x, packed.size(), packed.data(), &s);
	if (rc)
		fail("ntsm_sitegen_open failed (" + std::to_string(rc) + "): device " + std::to_string(opt.device));
	submit_genome(genome, s, ntsm_sitegen_submit, "ntsm_sitegen_submit");
	std::vector<uint8_t> h8(cands.size() + 1);
	if ((rc = ntsm_sitegen_hits(s, h8.data())))
		fail("ntsm_sitegen_hits failed (" + std::to_string(rc) + ")");
	if (opt.verbose) {
		ntsm_sitegen_times t;
		if (!ntsm_sitegen_times_get(s, &t))
			fprintf(stderr, "Device: table build %.1f ms, table upload %.1f ms (%.1f MB), stage %.1f ms, upload %.1f ms, scan kernel %.1f ms in %llu launches "
			        "(%llu full: %.1f .. %.1f ms each); %llu windows, %llu bitmap tests, %llu probes\n", t.table_build_ms, t.table_upload_ms, t.table_bytes / 1e6,
			        t.stage_ms, t.upload_ms, t.kernel_ms, (unsigned long long)t.launches, (unsigned long long)t.full_launches, t.full_kernel_ms_min, t.full_kernel_ms_max, (unsigned long long)t.windows, (unsigned long long)t.bitmap_tests, (unsigned long long)t.probes);
	}
	ntsm_sitegen_close(s);
	return std::vector<uint32_t>(h8.begin(), h8.end() - 1);
}

/* -g: the second library, H and G in one pass; the program's count is min(H + G, 255) */
std::vector<uint32_t> device_gap_hits(const Options &opt, const std::vector<Record> &genome, const std::vector<Candidate> &cands)
{
	const std::vector<uint64_t> packed = device_candidates(opt, cands);
	ntsm_sitegap *s = nullptr;
	int rc = ntsm_sitegap_open((int)opt.device, (uint32_t)opt.k, (uint32_t)opt.e, packed.size(), packed.data(), &s);
	if (rc)
		fail("ntsm_sitegap_open failed (" + std::to_string(rc) + "): device " + std::to_string(opt.device));
	submit_genome(genome, s, ntsm_sitegap_submit, "ntsm_sitegap_submit");
	std::vector<uint8_t> sub(cands.size() + 1), gap(cands.size() + 1);
	if ((rc = ntsm_sitegap_hits(s, sub.data(), gap.data())))
		fail("ntsm_sitegap_hits failed (" + std::to_string(rc) + ")");
	if (opt.verbose) {
		struct ntsm_sitegap_stats t;
		if (!ntsm_sitegap_stats(s, &t))
			fprintf(stderr, "Device: table build %.1f ms, table upload %.1f ms (%.1f MB), stage %.1f ms, upload %.1f ms, scan kernel %.1f ms in %llu launches "
			        "(%llu full: %.1f .. %.1f ms each); %llu windows (%llu of k + 1 bases, %llu of k - 1), %llu bitmap tests, %llu probes\n", t.table_build_ms,
			        t.table_upload_ms, t.table_bytes / 1e6, t.stage_ms, t.upload_ms, t.kernel_ms, (unsigned long long)t.launches, (unsigned long long)t.full_launches,
			        t.full_kernel_ms_min, t.full_kernel_ms_max, (unsigned long long)t.windows, (unsigned long long)t.windows_long,
			        (unsigned long long)t.windows_short, (unsigned long long)t.bitmap_tests, (unsigned long long)t.probes);
	}
	ntsm_sitegap_close(s);
	std::vector<uint32_t> hits(cands.size());
	for (size_t i = 0; i < cands.size(); i++)
		hits[i] = std::min<uint32_t>((uint32_t)sub[i] + gap[i], 255);
	return hits;
}

} // namespace

int main(int argc, char **argv)
{
	Options opt;
	bool die = false;
	if (argc > 1 && argv[1][0] != '-') {     /* upstream's spelling: a target and name=value pairs */
		const std::string target = argv[1];
		if (target == "generate-pca-rot-mat")
			fail("generate-pca-rot-mat is not one command here: run ntsmVCF --rotation on the multi-sample VCF (or ntsmVCF, then ntsmPCA on its matrix)");
		if (target != "generate-sites")
			fail("unknown target " + target + " (generate-sites is the one this program has)");
		for (int i = 2; i < argc; i++) {
			const std::string a = argv[i];
			const size_t eq = a.find('=');
			const std::string key = a.substr(0, eq), val = eq == std::string::npos ? "" : a.substr(eq + 1);
			bool ok = eq != std::string::npos;
			if (key == "name") opt.prefix = val;
			else if (key == "ref") opt.ref = val;
			else if (key == "vcf") opt.vcf = val;
			else if (key == "k") ok = ok && parse_long(val.c_str(), opt.k);
			else if (key == "w") ok = ok && parse_long(val.c_str(), opt.w);
			else if (key == "t") ok = ok && parse_long(val.c_str(), opt.threads);
			else if (key == "hits") opt.hits = val;      /* -H; not one of upstream's */
			else if (key == "gaps") {                    /* -g / -e: this program's own as well */
				long v = -1;
				ok = ok && parse_long(val.c_str(), v) && (v == 0 || v == 1);
				opt.gaps = v == 1;
			}
			else if (key == "gapskip") ok = ok && parse_long(val.c_str(), opt.e) && opt.e >= 0;
			else ok = false;
			if (!ok)
				fail("cannot read parameter " + a);
		}
		if (opt.prefix.empty()) fail("missing required param 'name' (output file prefix)");
		if (opt.ref.empty()) fail("missing required param 'ref' (FASTA reference file)");
		if (opt.vcf.empty()) fail("missing required param 'vcf' (vcf file containing variants file)");
	} else {
		for (int i = 1; i < argc; i++) {
			const std::string a = argv[i];
			if (a == "-i") { opt.at_cg_only = false; continue; }
			if (a == "-V") { opt.verbose++; continue; }
			if (a == "-g") { opt.gaps = true; continue; }
			if (a == "-h" || a == "--help") { usage(); return 0; }
			if (a.size() != 2 || a[0] != '-' || !strchr("rvpkwtxeHG", a[1]) || i + 1 >= argc) {
				std::cerr << "Error - Invalid parameter: " << a << std::endl;
				die = true;
				break;
			}
			const char *val = argv[++i];
			bool ok = true;
			switch (a[1]) {
			case 'r': opt.ref = val; break;
			case 'v': opt.vcf = val; break;
			case 'p': opt.prefix = val; break;
			case 'H': opt.hits = val; break;
			case 'k': ok = parse_long(val, opt.k); break;
			case 'w': ok = parse_long(val, opt.w); break;
			case 't': ok = parse_long(val, opt.threads); break;
			case 'x': ok = parse_long(val, opt.x); break;
			case 'e': ok = parse_long(val, opt.e) && opt.e >= 0; break;
			case 'G': ok = parse_long(val, opt.device); break;
			}
			if (!ok) {
				std::cerr << "Error - Invalid parameter " << a[1] << ": " << val << std::endl;
				die = true;
			}
		}
		if (!die && (opt.ref.empty() || opt.vcf.empty() || opt.prefix.empty())) {
			std::cerr << "Error: -r, -v and -p are needed" << std::endl;
			die = true;
		}
		if (die) {
			usage();
			return 1;
		}
	}
	if (opt.k < 1 || opt.k > 31) fail("k must be 1 .. 31");
	if (opt.w < opt.k) fail("w must be at least k");
	if (opt.w > 65535) fail("w must be below 65536");
	if (opt.x < 0 || opt.x > 1) fail("x must be 0 or 1");
	if (opt.e >= 0 && !opt.gaps) fail("-e needs -g (gapskip= needs gaps=1): the end margin is that of the gapped places");
	if (opt.gaps && opt.x != 1) fail("-g needs -x 1: a one-base gap is counted beside one substitution, as bwa aln -n 1 has it");
	if (opt.gaps && opt.e < 0) opt.e = 5;
	if (opt.gaps && (opt.e < 1 || 2 * opt.e > opt.k - 1)) fail("e must be 1 .. (k - 1) / 2, here 1 .. " + std::to_string((opt.k - 1) / 2));
	if (opt.threads < 1) fail("t must be at least 1");
	if (opt.device < 0) fail("G must not be negative");

	double t0 = now_ms();
	const std::vector<Record> genome = read_genome(opt.ref);
	double t1 = now_ms();
	const std::vector<Entry> entries = parse_vcf(opt.vcf);
	Step1 s1 = step1(opt, genome, entries);
	double t2 = now_ms();
	const std::vector<uint32_t> hits = opt.hits.empty() ? (opt.gaps ? device_gap_hits(opt, genome, s1.cands) : device_hits(opt, genome, s1.cands)) : read_hits(opt, entries, s1.cands);
	double t3 = now_ms();
	std::cerr << s1.err;
	{
		Out fa(opt.prefix + "_subKmers.fa");
		for (const Candidate &c : s1.cands)
			fa.put(">" + cand_name(entries, c) + "\n" + unpack(c.kmer, opt.k) + "\n");
		fa.close();
		if (opt.hits.empty()) {
			Out tsv(opt.prefix + "_subKmerHits.tsv");
			for (size_t c = 0; c < s1.cands.size(); c++)
				tsv.put(cand_name(entries, s1.cands[c]) + "\t" + std::to_string(hits[c]) + "\n");
			tsv.close();
		}
	}
	double t4 = now_ms();
	step3(opt, entries, s1.cands, hits);
	if (opt.verbose)
		fprintf(stderr, "Time: genome %.1f ms, step 1 %.1f ms, step 2 %.1f ms, candidate files %.1f ms, step 3 %.1f ms; %zu SNPs, %zu candidates\n",
		        t1 - t0, t2 - t1, t3 - t2, t4 - t3, now_ms() - t4, entries.size(), s1.cands.size());
	return 0;
}
