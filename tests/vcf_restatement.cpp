/*
 * vcf_restatement.cpp -- an independent restatement of ntsmVCF (the reference's src/ntSeqMatchVCF.cpp,
 * src/VCFConvert.hpp, src/MultiCount.hpp) as ONE thread runs it, with the sample x k-mer matrix sized for the header's
 * samples.  Written from the reference text, deliberately plain: a std::map from k-mer hash to matrix column, the
 * matrix as bytes, one insert at a time, iostream for the output.  Shares no code with the port
 * (ntsm_amd/csrc/host/ntsm_vcf_main.cpp, ntsm_amd/csrc/ntsm_vcf.hip); tests/test_vcf.py compiles it with g++ and
 * compares the port's bytes with it.  Plain (uncompressed) FASTA and VCF only; it accepts only inputs the port accepts.
 *
 *   vcf_restatement -s SITES -r GENOME [-k K] [-w W] [-m M] [-d] -p PREFIX VCF
 * writes PREFIX_matrix.tsv, PREFIX_center.txt and, on stderr, the site collision and insert warnings.
 */
#include <unistd.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <iostream>
#include <map>
#include <set>
#include <sstream>
#include <string>
#include <vector>

static unsigned K = 19, WIN = 31, MULTI = 20;
static bool DUPES = false;

/* FASTA records: name = header up to the first white space, sequence = the lines up to the next '>' */
static std::vector<std::pair<std::string, std::string>> read_fasta(const std::string &path)
{
	std::vector<std::pair<std::string, std::string>> out;
	std::ifstream in(path);
	std::string line;
	while (std::getline(in, line)) {
		if (!line.empty() && line[0] == '>') {
			size_t e = 1;
			while (e < line.size() && !isspace((unsigned char) line[e])) ++e;
			out.emplace_back(line.substr(1, e - 1), "");
		} else if (!out.empty()) {
			out.back().second += line;
		}
	}
	return out;
}

/* the k-mers of a string (vendor/KseqHashIterator.hpp): ACGT in either case, anything else restarts; each k-mer is
 * hashed from min(forward, reverse complement); pos = one past its last base */
struct Kmer { uint64_t hash, pos; };
static std::vector<Kmer> kmers(const std::string &s)
{
	std::vector<Kmer> out;
	const uint64_t mask = (1ULL << (2 * K)) - 1, shift = 2 * (K - 1);
	uint64_t fw = 0, rv = 0;
	unsigned len = 0;
	for (size_t i = 0; i < s.size(); ++i) {
		int c;
		switch (s[i]) {
		case 'A': case 'a': c = 0; break;
		case 'C': case 'c': c = 1; break;
		case 'G': case 'g': c = 2; break;
		case 'T': case 't': case 'U': case 'u': c = 3; break;
		default: c = 4;
		}
		if (c == 4) { fw = rv = 0; len = 0; continue; }
		fw = ((fw << 2) | (uint64_t) c) & mask;
		rv = (rv >> 2) | ((uint64_t) (3 - c) << shift);
		if (++len >= K) {
			uint64_t key = fw < rv ? fw : rv;               /* the invertible hash of the reference */
			key = (~key + (key << 21)) & mask;
			key = key ^ key >> 24;
			key = ((key + (key << 3)) + (key << 8)) & mask;
			key = key ^ key >> 14;
			key = ((key + (key << 2)) + (key << 4)) & mask;
			key = key ^ key >> 28;
			key = (key + (key << 31)) & mask;
			out.push_back({ key, i + 1 });
		}
	}
	return out;
}

int main(int argc, char **argv)
{
	std::string snp, ref, prefix;
	int c;
	while ((c = getopt(argc, argv, "s:r:k:w:m:dp:")) != -1) {
		switch (c) {
		case 's': snp = optarg; break;
		case 'r': ref = optarg; break;
		case 'k': K = (unsigned) atoi(optarg); break;
		case 'w': WIN = (unsigned) atoi(optarg); break;
		case 'm': MULTI = (unsigned) strtoul(optarg, nullptr, 10); break;
		case 'd': DUPES = true; break;
		case 'p': prefix = optarg; break;
		default: return 2;
		}
	}
	const std::string vcf = argv[optind];

	/* sites: records alternate REF / VAR; a hash gets the next column when first seen, later sightings warn */
	std::map<uint64_t, uint64_t> column;
	std::set<uint64_t> shared;
	std::vector<std::string> ids;
	std::vector<std::vector<uint64_t>> refList, varList;
	uint64_t columns = 0;
	const auto recs = read_fasta(snp);
	for (size_t r = 0; r < recs.size(); ++r) {
		std::vector<uint64_t> &list = (r % 2 == 0) ? (refList.emplace_back(), refList.back()) : (varList.emplace_back(), varList.back());
		for (const Kmer &km : kmers(recs[r].second)) {
			if (column.count(km.hash)) {
				std::cerr << "Warning: " << recs[r].first << " of " << (r % 2 == 0 ? "REF" : "VAR") << " file has a k-mer collision at pos: "
				          << km.pos << std::endl;
				shared.insert(km.hash);
			} else {
				list.push_back(km.hash);
				column[km.hash] = columns++;
			}
		}
		if (r % 2 == 0) ids.push_back(recs[r].first);
	}
	if (!DUPES)
		for (uint64_t h : shared) column.erase(h);

	/* genome: the last record of a name wins */
	std::map<std::string, std::string> genome;
	for (auto &g : read_fasta(ref)) genome[g.first] = g.second;

	/* VCF header: samples after the ninth field of the #CHROM line */
	std::ifstream fh(vcf);
	std::string line;
	std::vector<std::string> samples;
	while (std::getline(fh, line)) {
		if (line[0] != '#') continue;
		std::vector<std::string> f;
		std::stringstream ss(line);
		std::string item;
		while (std::getline(ss, item, '\t')) f.push_back(item);
		if (f[0] == "#CHROM") { samples.assign(f.begin() + std::min<size_t>(9, f.size()), f.end()); break; }
	}
	const size_t N = samples.size();
	std::vector<uint8_t> mat(columns * N, 0);                      /* [sample][column] */

	auto insert = [&](size_t sample, uint64_t col, unsigned value) {
		uint8_t &cell = mat[col + columns * sample];
		if (cell > 0) {
			if (cell != value)
				std::cerr << "Warning: Inconsistent k-mer counts, check for overlapping sites: " << cell << " vs " << value << std::endl;
			return;
		}
		cell = (uint8_t) value;
	};

	/* body: complete lines only */
	while (std::getline(fh, line) && !fh.eof()) {
		std::vector<std::string> f;
		{
			size_t a = 0;
			for (size_t b; (b = line.find('\t', a)) != std::string::npos; a = b + 1) f.push_back(line.substr(a, b - a));
			f.push_back(line.substr(a));
		}
		auto field = [&](size_t i) { return f[std::min(i, f.size() - 1)]; };
		const long pos = std::stol(field(1));
		if (field(3) == ".") continue;
		if (field(4).size() != 1) continue;
		const std::string &chrom = genome.at(field(0));
		/* the window: W bases from pos - W/2 - 1, cut at the end of the chromosome (or at a NUL) */
		const size_t start = (size_t) pos - WIN / 2 - 1;
		std::string refWin = chrom.substr(start, WIN);
		refWin = refWin.substr(0, strlen(refWin.c_str()));
		std::string varWin = refWin;
		if (varWin.size() > WIN / 2) varWin[WIN / 2] = field(4)[0];
		else if (varWin.size() == WIN / 2 && WIN > 0) varWin += field(4)[0];      /* the ALT byte replaces the first NUL */
		if (varWin.find('\0') != std::string::npos) varWin.resize(varWin.find('\0'));
		std::vector<int> g(N, 0);                                   /* 0 hom1, 1 het, 2 hom2; anything else hom1 */
		for (size_t s = 0; s < N; ++s) {
			const std::string &x = f[9 + s];
			g[s] = x == "0|1" || x == "1|0" ? 1 : x == "1|1" ? 2 : 0;
		}
		/* a k-mer that is not a key changes nothing */
		for (const Kmer &km : kmers(refWin)) {
			auto it = column.find(km.hash);
			if (it == column.end()) continue;
			for (size_t s = 0; s < N; ++s)
				if (g[s] == 0) insert(s, it->second, MULTI * 2);
				else if (g[s] == 1) insert(s, it->second, MULTI);
		}
		for (const Kmer &km : kmers(varWin)) {
			auto it = column.find(km.hash);
			if (it == column.end()) continue;
			for (size_t s = 0; s < N; ++s)
				if (g[s] == 2) insert(s, it->second, MULTI * 2);
				else if (g[s] == 1) insert(s, it->second, MULTI);
		}
	}

	/* the matrix: per site and sample the ratio of the REF maximum to both maxima; an undefined cell prints the row's
	 * mean (over all samples) with 19 digits, and the stream keeps that precision */
	std::ofstream out(prefix + "_matrix.tsv"), centerFile(prefix + "_center.txt");
	out << "alleleID";
	for (const std::string &s : samples) out << "\t" << s;
	out << "\n";
	const double UNDEF = -1.0;
	for (size_t i = 0; i < ids.size(); ++i) {
		std::vector<double> v(N);
		double sum = 0.0;
		std::vector<uint64_t> rc, vc;
		for (uint64_t h : refList[i]) rc.push_back(column.at(h));
		for (uint64_t h : varList[i]) vc.push_back(column.at(h));
		for (size_t s = 0; s < N; ++s) {
			unsigned mr = 0, mv = 0;
			for (uint64_t col : rc) mr = std::max<unsigned>(mr, mat[col + columns * s]);
			for (uint64_t col : vc) mv = std::max<unsigned>(mv, mat[col + columns * s]);
			if (mr + mv == 0) v[s] = UNDEF;
			else { v[s] = double(mr) / double(mr + mv); sum += v[s]; }
		}
		const long double center = sum / (long double) N;
		out << ids[i];
		for (size_t s = 0; s < N; ++s) {
			if (v[s] == UNDEF) out << "\t" << std::setprecision(19) << center;
			else out << "\t" << v[s];
		}
		out << "\n";
		centerFile << std::setprecision(19) << center << "\n";
	}
	return 0;
}
