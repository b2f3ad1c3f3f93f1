/*
 * tests/sitegen_restatement.cpp -- an independent restatement of ntsmSiteGen's three steps, written from the text of
 * upstream's ntsm-scripts/extractSNPsfromVCF.py and filterRepetiveSNP.pl and from the definition of H in
 * include/ntsm_sitegen_hip.h.  It shares no code with the product: strings and std::map where the product packs bits,
 * std::regex where the product matches by hand, and for H the definition itself (every candidate against every window,
 * both strands).  Two faster statements of H serve where that is too slow, and tests/test_sitegen.py checks both against
 * the definition: "neighbours" (many candidates) looks every k-mer within one substitution of a window up in a map of
 * the candidates; "halves" (a few candidates, a genome of any size, streamed) uses that one substitution leaves the left or
 * the right half of a k-mer intact, and compares a window with the candidates that share a half with it.
 *
 *   sitegen_restatement all GENOME.fa SNPS.vcf PREFIX k w x keep_all
 *       writes PREFIX_subKmers.fa, PREFIX_subKmerHits.tsv, PREFIX_sam.txt (one SAM-shaped line per candidate: name in
 *       column 1, the k-mer in column 10, X0:i:H when H > 0), PREFIX_n{i}.fa; the script's stderr on stderr.
 *       Exit 1 with "Error: ..." where the product refuses.
 *   sitegen_restatement hits GENOME.fa KMERS.txt k x naive|neighbours|halves
 *       KMERS.txt: one k-mer per line; prints min(H, 255) per line.
 */
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <map>
#include <regex>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

typedef std::vector<std::pair<std::string, std::string> > Genome;

static void die(const std::string &m)
{
	std::cerr << "Error: " << m << "\n";
	exit(1);
}

static Genome read_fasta(const std::string &path)
{
	std::ifstream in(path.c_str());
	if (!in) die("cannot open " + path);
	Genome g;
	std::string line;
	while (std::getline(in, line)) {
		if (!line.empty() && line[line.size() - 1] == '\r') line.erase(line.size() - 1);
		if (line.empty()) continue;
		if (line[0] == '>') {
			size_t e = 1;
			while (e < line.size() && !isspace((unsigned char)line[e])) e++;
			g.push_back(std::make_pair(line.substr(1, e - 1), std::string()));
		} else if (!g.empty())
			g.back().second += line;
	}
	return g;
}

static std::string upper(std::string s)
{
	for (size_t i = 0; i < s.size(); i++) s[i] = (char)toupper((unsigned char)s[i]);
	return s;
}

static bool acgt(const std::string &s)
{
	return s.find_first_not_of("ACGT") == std::string::npos;
}

static std::string revcomp(const std::string &s)
{
	std::string r(s.rbegin(), s.rend());
	for (size_t i = 0; i < r.size(); i++)
		r[i] = r[i] == 'A' ? 'T' : r[i] == 'T' ? 'A' : r[i] == 'C' ? 'G' : 'C';
	return r;
}

static std::string canon(const std::string &s)
{
	std::string r = revcomp(s);
	return s < r ? s : r;
}

/* ------------------------------------------------------------------------------------------------ H */
static uint64_t enc(const std::string &s)
{
	uint64_t v = 0;
	for (size_t i = 0; i < s.size(); i++)
		v = v * 4 + (s[i] == 'A' ? 0 : s[i] == 'C' ? 1 : s[i] == 'G' ? 2 : 3);
	return v;
}

/* every window of k bases of ACGT (after upper-casing) inside one record */
static std::vector<uint64_t> windows_of(const Genome &g, int k)
{
	std::vector<uint64_t> w;
	for (size_t r = 0; r < g.size(); r++) {
		const std::string s = upper(g[r].second);
		for (size_t p = 0; p + k <= s.size(); p++) {
			const std::string sub = s.substr(p, k);
			if (acgt(sub)) w.push_back(enc(sub));
		}
	}
	return w;
}

static inline bool within(uint64_t a, uint64_t b, int x)
{
	uint64_t d = a ^ b;
	d = (d | (d >> 1)) & 0x5555555555555555ull;      /* one bit per differing base */
	return x ? (d & (d - 1)) == 0 : d == 0;
}

static std::vector<int> hits_naive(const Genome &g, const std::vector<std::string> &cands, int k, int x)
{
	const std::vector<uint64_t> w = windows_of(g, k);
	std::vector<int> h(cands.size(), 0);
	for (size_t c = 0; c < cands.size(); c++) {
		const uint64_t f = enc(cands[c]), r = enc(revcomp(cands[c]));   /* ham(q, rc(g)) = ham(rc(q), g) */
		long n = 0;
		for (size_t i = 0; i < w.size(); i++)
			n += within(f, w[i], x) + within(r, w[i], x);
		h[c] = (int)std::min(n, 255l);
	}
	return h;
}

static std::vector<int> hits_neighbours(const Genome &g, const std::vector<std::string> &cands, int k, int x)
{
	std::unordered_map<uint64_t, std::vector<int> > at;   /* k-mer -> the candidates that are it (forward) or its reverse complement */
	for (size_t c = 0; c < cands.size(); c++) {
		at[enc(cands[c])].push_back((int)c);
		at[enc(revcomp(cands[c]))].push_back((int)c);
	}
	std::vector<long> h(cands.size(), 0);
	const std::vector<uint64_t> w = windows_of(g, k);
	for (size_t i = 0; i < w.size(); i++) {
		std::vector<uint64_t> near(1, w[i]);
		if (x)
			for (int p = 0; p < k; p++)
				for (uint64_t b = 1; b < 4; b++)
					near.push_back(w[i] ^ (b << (2 * p)));
		for (size_t j = 0; j < near.size(); j++) {
			std::unordered_map<uint64_t, std::vector<int> >::const_iterator it = at.find(near[j]);
			if (it != at.end())
				for (size_t e = 0; e < it->second.size(); e++) h[it->second[e]]++;
		}
	}
	std::vector<int> out(cands.size());
	for (size_t c = 0; c < cands.size(); c++) out[c] = (int)std::min(h[c], 255l);
	return out;
}

static std::vector<int> hits_halves(const Genome &g, const std::vector<std::string> &cands, int k, int x)
{
	const int lo_n = k / 2, hi_n = k - lo_n;                 /* the right half has lo_n bases, the left hi_n */
	const uint64_t lo_mask = (1ull << (2 * lo_n)) - 1;
	std::unordered_map<uint64_t, std::vector<std::pair<uint64_t, int> > > by_left, by_right;
	std::vector<bool> left_any(1ull << (2 * hi_n), false), right_any(1ull << (2 * lo_n), false);
	for (size_t c = 0; c < cands.size(); c++)
		for (int o = 0; o < 2; o++) {
			const uint64_t q = enc(o ? revcomp(cands[c]) : cands[c]);
			by_left[q >> (2 * lo_n)].push_back(std::make_pair(q, (int)c));
			by_right[q & lo_mask].push_back(std::make_pair(q, (int)c));
			left_any[q >> (2 * lo_n)] = true;
			right_any[q & lo_mask] = true;
		}
	std::vector<long> h(cands.size(), 0);
	const uint64_t kmask = (1ull << (2 * k)) - 1;
	for (size_t r = 0; r < g.size(); r++) {
		const std::string &s = g[r].second;
		uint64_t w = 0;
		int run = 0;
		for (size_t p = 0; p < s.size(); p++) {
			const char c = (char)toupper((unsigned char)s[p]);
			const int code = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
			if (code < 0) { run = 0; continue; }
			w = ((w << 2) | (uint64_t)code) & kmask;
			if (++run < k) continue;
			const uint64_t left = w >> (2 * lo_n), right = w & lo_mask;
			if (left_any[left]) {                                /* left half equal: the right half differs in <= x bases */
				const std::vector<std::pair<uint64_t, int> > &v = by_left[left];
				for (size_t e = 0; e < v.size(); e++) h[v[e].second] += within(v[e].first, w, x);
			}
			if (right_any[right]) {                              /* right half equal and the left differs: not counted above */
				const std::vector<std::pair<uint64_t, int> > &v = by_right[right];
				for (size_t e = 0; e < v.size(); e++) h[v[e].second] += (v[e].first >> (2 * lo_n)) != left && within(v[e].first, w, x);
			}
		}
	}
	std::vector<int> out(cands.size());
	for (size_t c = 0; c < cands.size(); c++) out[c] = (int)std::min(h[c], 255l);
	return out;
}

/* ------------------------------------------------------------------------------------------------ step 1 */
struct Snp {
	std::string chr, wt, var;
	long pos;
};

static bool to_int(std::string s, long &v)
{
	while (!s.empty() && isspace((unsigned char)s[0])) s.erase(0, 1);
	while (!s.empty() && isspace((unsigned char)s[s.size() - 1])) s.erase(s.size() - 1);
	if (s.empty()) return false;
	size_t i = (s[0] == '+' || s[0] == '-') ? 1 : 0;
	if (i == s.size() || s.size() > 15) return false;
	for (size_t j = i; j < s.size(); j++)
		if (!isdigit((unsigned char)s[j])) return false;
	v = atol(s.c_str());
	return true;
}

struct Cand {
	std::string name, seq;
};

static std::vector<Cand> extract(const Genome &g, const std::string &vcf, int k /* sub k-mer */, int w /* window */, bool keep_all, std::ostream &err)
{
	std::map<std::string, const std::string *> chrom;
	for (size_t i = 0; i < g.size(); i++) {
		if (chrom.count(g[i].first)) die("record name twice");
		chrom[g[i].first] = &g[i].second;
	}
	/* the dict: insertion order of keys, last value */
	std::vector<std::string> order;
	std::map<std::string, Snp> dict;
	std::ifstream in(vcf.c_str());
	if (!in) die("cannot open " + vcf);
	std::string line;
	long id_counter = 0;
	while (std::getline(in, line)) {
		if (!line.empty() && line[0] == '#') continue;
		while (!line.empty() && isspace((unsigned char)line[line.size() - 1])) line.erase(line.size() - 1);
		std::vector<std::string> f;
		std::stringstream ss(line);
		std::string tok;
		while (std::getline(ss, tok, '\t')) f.push_back(tok);
		if (!line.empty() && line[line.size() - 1] == '\t') f.push_back("");
		if (f.size() < 5) die("fewer than five fields");
		std::string id = f[2];
		if (id == ".") {
			std::ostringstream o;
			o << id_counter++;
			id = o.str();
		}
		if (id.empty()) die("empty ID");
		if (f[4].size() > 1) die("Multiple alternate alleles found in VCF");
		if (f[4].empty()) die("empty ALT");
		Snp s;
		if (!to_int(f[1], s.pos)) die("POS");
		s.chr = f[0]; s.wt = f[3]; s.var = f[4];
		if (!dict.count(id)) order.push_back(id);
		dict[id] = s;
	}
	const int half = w / 2;
	std::map<std::string, int> kmers;
	std::map<std::string, std::pair<std::string, std::string> > strs;   /* id -> (tmpStr, modStr) of the SNPs that pass */
	for (size_t o = 0; o < order.size(); o++) {
		const Snp &s = dict[order[o]];
		if (!chrom.count(s.chr)) die("unknown chromosome " + s.chr);
		const std::string &seq = *chrom[s.chr];
		const long offset = s.pos - 1;
		const long pos1 = (long)std::ceil((double)offset - w / 2.0);
		if (pos1 < 0 || pos1 + w > (long)seq.size()) die("window outside its chromosome");
		const std::string tmp = upper(seq.substr(pos1, w));
		if (s.wt != std::string(1, tmp[half])) {
			err << "Wildtype allele does not match\n" << "ref:" << s.wt << "\n" << "var:" << s.var << "\n" << "fasta:" << seq[offset] << "\n" << "kmer:" << tmp << "\n";
			continue;
		}
		const bool same_class = (std::string("AT").find(s.wt) != std::string::npos && std::string("AT").find(s.var) != std::string::npos)
		                        || (std::string("CG").find(s.wt) != std::string::npos && std::string("CG").find(s.var) != std::string::npos);
		if (same_class && !keep_all) continue;
		const std::string mod = tmp.substr(0, half) + s.var + tmp.substr(half + 1);
		if (!acgt(tmp) || !acgt(mod)) die("character outside ACGT");
		for (int p = 0; p + k <= w; p++) {
			kmers[canon(tmp.substr(p, k))]++;
			kmers[canon(mod.substr(p, k))]++;
		}
		strs[order[o]] = std::make_pair(tmp, mod);
	}
	long remove_count = 0, process_count = 0, filter_count = 0, kmers_removed = 0;
	std::vector<Cand> out;
	for (size_t o = 0; o < order.size(); o++) {
		const std::string &id = order[o];
		const Snp &s = dict[id];
		if (!strs.count(id)) {
			remove_count++;
			const std::string centre = upper(std::string(1, (*chrom[s.chr])[s.pos - 1]));
			if (s.wt == centre) filter_count++;
			continue;
		}
		const std::string &tmp = strs[id].first, &mod = strs[id].second;
		const long retained = kmers_removed;
		const bool wt_first = s.wt == "A" || s.wt == "T";
		for (int p = 0; p + k <= w; p++) {
			const std::string a = (wt_first ? tmp : mod).substr(p, k), c = (wt_first ? mod : tmp).substr(p, k);
			std::ostringstream n;
			n << id << "|" << p << "|";
			if (kmers[canon(a)] == 1) { Cand x = {n.str() + "AT", a}; out.push_back(x); } else kmers_removed++;
			if (kmers[canon(c)] == 1) { Cand x = {n.str() + "CG", c}; out.push_back(x); } else kmers_removed++;
		}
		if (kmers_removed - retained == w - k + 1) remove_count++;
		process_count++;
	}
	err << "Processed " << process_count << " SNPs. Removed " << remove_count << " SNPs. " << kmers_removed << " duplicate k-mers removed.\n";
	if (filter_count > 0) err << "Filtered " << filter_count << " SNPs that did not have A/T to C/G variants\n";
	return out;
}

/* ------------------------------------------------------------------------------------------------ step 3 */
static std::vector<std::string> filter(const std::vector<std::string> &sam, int w, int k)
{
	const int max_count = w - k + 1;
	std::map<std::string, std::map<std::string, int> > uniq;
	std::map<std::string, std::map<std::string, std::string> > str;
	const std::regex name_re("([^|]+)\\|([0-9]+)\\|(AT|CG)"), x0("X0:i:([0-9]+)"), x1(".*X1:i:([0-9]+)");
	for (size_t l = 0; l < sam.size(); l++) {
		std::vector<std::string> f;
		std::stringstream ss(sam[l]);
		std::string tok;
		while (std::getline(ss, tok, '\t')) f.push_back(tok);
		std::smatch m;
		if (f.empty() || !std::regex_search(f[0], m, name_re)) {
			std::cerr << "unable to parse: " << sam[l] << "\n";
			continue;
		}
		const std::string id = m[1], type = m[3], seq = f.size() > 9 ? f[9] : "";
		if (!uniq[id].count(type)) uniq[id][type] = max_count;
		bool keep = true;
		std::smatch c0, c1;
		if (std::regex_search(sam[l], c0, x0)) {
			long count = atol(c0[1].str().c_str());
			if (std::regex_search(sam[l], c1, x1)) count += atol(c1[1].str().c_str());
			keep = count == 1;
		}
		if (!keep) continue;
		if (str[id].count(type)) str[id][type] += "N" + seq;
		else str[id][type] = seq;
		uniq[id][type]--;
	}
	std::vector<std::string> files(max_count);
	for (std::map<std::string, std::map<std::string, int> >::iterator it = uniq.begin(); it != uniq.end(); ++it)
		for (int i = 0; i < max_count; i++) {
			std::map<std::string, int> &u = it->second;
			if (!u.count("AT") || !u.count("CG") || u["AT"] > i || u["CG"] > i) continue;
			if (!str[it->first].count("AT") || !str[it->first].count("CG")) continue;
			files[i] += ">" + it->first + " ref\n" + str[it->first]["AT"] + "\n>" + it->first + " var\n" + str[it->first]["CG"] + "\n";
		}
	return files;
}

static void write(const std::string &path, const std::string &text)
{
	std::ofstream o(path.c_str(), std::ios::binary);
	o << text;
	if (!o) die("cannot write " + path);
}

int main(int argc, char **argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	if (mode == "hits" && argc == 7) {
		const Genome g = read_fasta(argv[2]);
		std::ifstream in(argv[3]);
		std::vector<std::string> cands;
		std::string line;
		while (std::getline(in, line)) cands.push_back(line);
		const int k = atoi(argv[4]), x = atoi(argv[5]);
		const std::string how = argv[6];
		if (k < 1 || k > 31 || x < 0 || x > 1 || (how != "naive" && how != "neighbours" && how != "halves")) die("k, x, method");
		const std::vector<int> h = how == "naive" ? hits_naive(g, cands, k, x) : how == "halves" ? hits_halves(g, cands, k, x) : hits_neighbours(g, cands, k, x);
		std::string out;
		for (size_t i = 0; i < h.size(); i++) out += std::to_string(h[i]) + "\n";
		fwrite(out.data(), 1, out.size(), stdout);
		return 0;
	}
	if (mode == "all" && argc == 9) {
		const Genome g = read_fasta(argv[2]);
		const std::string prefix = argv[4];
		const int k = atoi(argv[5]), w = atoi(argv[6]), x = atoi(argv[7]);
		if (k < 1 || k > 31 || w < k) die("k, w");
		std::ostringstream err;
		const std::vector<Cand> cands = extract(g, argv[3], k, w, atoi(argv[8]) != 0, err);
		std::vector<std::string> seqs;
		for (size_t i = 0; i < cands.size(); i++) seqs.push_back(cands[i].seq);
		const std::vector<int> h = hits_naive(g, seqs, k, x);
		std::string fa, tsv;
		std::vector<std::string> sam;
		for (size_t i = 0; i < cands.size(); i++) {
			fa += ">" + cands[i].name + "\n" + cands[i].seq + "\n";
			tsv += cands[i].name + "\t" + std::to_string(h[i]) + "\n";
			std::string l = cands[i].name + "\t0\t*\t0\t0\t*\t*\t0\t0\t" + cands[i].seq + "\t*";
			if (h[i] > 0) l += "\tX0:i:" + std::to_string(h[i]);
			sam.push_back(l);
		}
		const std::vector<std::string> files = filter(sam, w, k);
		std::cerr << err.str();
		write(prefix + "_subKmers.fa", fa);
		write(prefix + "_subKmerHits.tsv", tsv);
		std::string samtext;
		for (size_t i = 0; i < sam.size(); i++) samtext += sam[i] + "\n";
		write(prefix + "_sam.txt", samtext);
		for (size_t i = 0; i < files.size(); i++) write(prefix + "_n" + std::to_string(i) + ".fa", files[i]);
		return 0;
	}
	std::cerr << "usage: sitegen_restatement all GENOME.fa SNPS.vcf PREFIX k w x keep_all | hits GENOME.fa KMERS.txt k x naive|neighbours|halves\n";
	return 2;
}
