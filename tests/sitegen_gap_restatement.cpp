/*
 * tests/sitegen_gap_restatement.cpp -- the definition of G in include/ntsm_sitegen_gap_hip.h (one-base gapped places of a
 * candidate k-mer) restated on strings, for tests/test_sitegen_gap.py.  It shares no code with the product.  Steps 1 and 3
 * of ntsmSiteGen and the substitution count H are those of tests/sitegen_restatement.cpp, whose text is compiled in
 * unchanged (its main under another name).
 *
 *   sitegen_gap_restatement hits GENOME.fa KMERS.txt k e naive|neighbours
 *       KMERS.txt: one k-mer per line; prints "min(H, 255) min(G, 255)" per line, H within one substitution.
 *       naive: the definition as it stands -- every candidate x every window of k + 1 and of k - 1 bases x both strands
 *       x every p (a pair whose first or last bases differ is passed over: with e >= 1 no p can qualify).
 *       neighbours: for dense sets.  From every long window each interior base is removed, into every short window each
 *       of the four bases is inserted at each interior position, and the k-mer that results is looked up in a map of the
 *       candidates and their reverse complements (keyed by the 2-bit code of the k-mer, as sitegen_restatement.cpp's own
 *       "neighbours" is); what is found is kept in a set per window, so a window counts once per candidate and strand
 *       however many positions lead to it.
 *   sitegen_gap_restatement all GENOME.fa SNPS.vcf PREFIX k w e keep_all
 *       as sitegen_restatement's `all` with x = 1, and X0:i: (and the hits file) set to min(H + G, 255).
 */
#define main sitegen_restatement_main
#include "sitegen_restatement.cpp"
#undef main

#include <set>

/* every window of n bases of ACGT (after upper-casing) inside one record, as a string */
static std::vector<std::string> text_windows(const Genome &g, int n)
{
	std::vector<std::string> w;
	for (size_t r = 0; r < g.size(); r++) {
		const std::string s = upper(g[r].second);
		for (size_t p = 0; p + n <= s.size(); p++) {
			const std::string sub = s.substr(p, n);
			if (acgt(sub)) w.push_back(sub);
		}
	}
	return w;
}

static bool long_place(const std::string &g, const std::string &q, int k, int e)
{
	for (int p = e; p <= k - e; p++)
		if (g.compare(0, p, q, 0, p) == 0 && g.compare(p + 1, k - p, q, p, k - p) == 0) return true;
	return false;
}

static bool short_place(const std::string &g, const std::string &q, int k, int e)
{
	for (int p = e; p <= k - 1 - e; p++)
		if (g.compare(0, p, q, 0, p) == 0 && g.compare(p, k - 1 - p, q, p + 1, k - 1 - p) == 0) return true;
	return false;
}

static std::vector<int> gaps_naive(const Genome &g, const std::vector<std::string> &cands, int k, int e)
{
	const std::vector<std::string> lw = text_windows(g, k + 1), sw = text_windows(g, k - 1);
	std::vector<int> out(cands.size(), 0);
	for (size_t c = 0; c < cands.size(); c++) {
		const std::string strand[2] = {cands[c], revcomp(cands[c])};
		long n = 0;
		for (int o = 0; o < 2; o++) {
			const std::string &q = strand[o];
			const char q0 = q[0], q1 = q[k - 1];
			for (size_t i = 0; i < lw.size(); i++)
				if (lw[i][0] == q0 && lw[i][k] == q1) n += long_place(lw[i], q, k, e);
			for (size_t i = 0; i < sw.size(); i++)
				if (sw[i][0] == q0 && sw[i][k - 2] == q1) n += short_place(sw[i], q, k, e);
		}
		out[c] = (int)std::min(n, 255l);
	}
	return out;
}

static std::vector<int> gaps_neighbours(const Genome &g, const std::vector<std::string> &cands, int k, int e)
{
	typedef std::unordered_map<uint64_t, std::vector<int> > Map;   /* k-mer (enc) -> 2 * candidate + strand */
	Map at;
	for (size_t c = 0; c < cands.size(); c++) {
		at[enc(cands[c])].push_back((int)(2 * c));
		at[enc(revcomp(cands[c]))].push_back((int)(2 * c + 1));
	}
	std::vector<long> h(cands.size(), 0);
	for (int kind = 0; kind < 2; kind++) {
		const int n = kind ? k - 1 : k + 1, last = kind ? k - 1 - e : k - e;
		const std::vector<uint64_t> w = windows_of(g, n);           /* base i of a window in bits 2 (n - 1 - i) and the next */
		for (size_t i = 0; i < w.size(); i++) {
			std::set<int> found;
			for (int p = e; p <= last; p++) {
				const uint64_t left = w[i] >> (2 * (n - p));           /* bases 0 .. p - 1 */
				for (uint64_t b = 0; b < (kind ? 4u : 1u); b++) {
					uint64_t q;
					if (kind)                                           /* left, b, bases p .. k - 2 */
						q = (((left << 2) | b) << (2 * (n - p))) | (w[i] & ((1ull << (2 * (n - p))) - 1));
					else                                                /* left, bases p + 1 .. k */
						q = (left << (2 * (n - p - 1))) | (w[i] & ((1ull << (2 * (n - p - 1))) - 1));
					Map::const_iterator it = at.find(q);
					if (it != at.end()) found.insert(it->second.begin(), it->second.end());
				}
			}
			for (std::set<int>::const_iterator f = found.begin(); f != found.end(); ++f) h[*f / 2]++;
		}
	}
	std::vector<int> out(cands.size());
	for (size_t c = 0; c < cands.size(); c++) out[c] = (int)std::min(h[c], 255l);
	return out;
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
		const int k = atoi(argv[4]), e = atoi(argv[5]);
		const std::string how = argv[6];
		if (k < 3 || k > 31 || e < 1 || 2 * e > k - 1 || (how != "naive" && how != "neighbours")) die("k, e, method");
		for (size_t c = 0; c < cands.size(); c++)
			if ((int)cands[c].size() != k || !acgt(cands[c])) die("candidate " + cands[c]);
		const std::vector<int> h = how == "naive" ? hits_naive(g, cands, k, 1) : hits_neighbours(g, cands, k, 1);
		const std::vector<int> gp = how == "naive" ? gaps_naive(g, cands, k, e) : gaps_neighbours(g, cands, k, e);
		std::string out;
		for (size_t i = 0; i < h.size(); i++) out += std::to_string(h[i]) + " " + std::to_string(gp[i]) + "\n";
		fwrite(out.data(), 1, out.size(), stdout);
		return 0;
	}
	if (mode == "all" && argc == 9) {
		const Genome g = read_fasta(argv[2]);
		const std::string prefix = argv[4];
		const int k = atoi(argv[5]), w = atoi(argv[6]), e = atoi(argv[7]);
		if (k < 3 || k > 31 || w < k || e < 1 || 2 * e > k - 1) die("k, w, e");
		std::ostringstream err;
		const std::vector<Cand> cands = extract(g, argv[3], k, w, atoi(argv[8]) != 0, err);
		std::vector<std::string> seqs;
		for (size_t i = 0; i < cands.size(); i++) seqs.push_back(cands[i].seq);
		const std::vector<int> h = hits_naive(g, seqs, k, 1), gp = gaps_naive(g, seqs, k, e);
		std::string fa, tsv, samtext;
		std::vector<std::string> sam;
		for (size_t i = 0; i < cands.size(); i++) {
			const int both = std::min(h[i] + gp[i], 255);
			fa += ">" + cands[i].name + "\n" + cands[i].seq + "\n";
			tsv += cands[i].name + "\t" + std::to_string(both) + "\n";
			std::string l = cands[i].name + "\t0\t*\t0\t0\t*\t*\t0\t0\t" + cands[i].seq + "\t*";
			if (both > 0) l += "\tX0:i:" + std::to_string(both);
			sam.push_back(l);
			samtext += l + "\n";
		}
		const std::vector<std::string> files = filter(sam, w, k);
		std::cerr << err.str();
		write(prefix + "_subKmers.fa", fa);
		write(prefix + "_subKmerHits.tsv", tsv);
		write(prefix + "_sam.txt", samtext);
		for (size_t i = 0; i < files.size(); i++) write(prefix + "_n" + std::to_string(i) + ".fa", files[i]);
		return 0;
	}
	std::cerr << "usage: sitegen_gap_restatement all GENOME.fa SNPS.vcf PREFIX k w e keep_all | hits GENOME.fa KMERS.txt k e naive|neighbours\n";
	return 2;
}
