/*
 * eval_index_check.cpp -- the writer and the reader of ntsm_amd/csrc/host/eval_index.hpp driven on their own, for a host
 * sanitizer run (`make index_check`: -fsanitize=address,undefined, no HIP, no GPU):
 *
 *     build/eval_index_check DIR
 *
 * writes 12 small counts files into DIR, packs 8 of them into DIR/check.store and indexes it with synthetic clouds and
 * tallies (the projection is the device's; the file does not care where its numbers come from), reads the index back cell
 * by cell, appends the other 4 samples to the store -- the index is now stale --, extends the index and compares it byte for
 * byte with the index of a 12-sample store written at once, then asks for every validity failure: magic, version, a byte
 * short, a byte long, offsets, other loci (n_sites and CRC), more samples than the store, fewer (stale).  Prints one line per
 * step; exit status 0 when all held.
 */
#include <cstdio>
#include <fstream>
#include <iterator>

#include "../ntsm_amd/csrc/host/eval_index.hpp"

namespace st = ntsm::eval_store;
namespace ix = ntsm::eval_index;

static std::string bytes_of(const std::string &path)
{
	std::ifstream f(path, std::ios::binary);
	return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

static void put(const std::string &path, const std::string &bytes)
{
	std::ofstream f(path, std::ios::binary);
	f.write(bytes.data(), (std::streamsize) bytes.size());
}

template <class F> static bool refused(const char *what, F f)
{
	try { f(); } catch (const st::Error &e) { printf("refused (%s): %s\n", what, e.what()); return true; }
	printf("NOT refused: %s\n", what);
	return false;
}

/* a counts file over `m` loci; `prefix` names them */
static std::string counts_file(const std::string &dir, int i, unsigned m, const char *prefix = "rs")
{
	const std::string path = dir + "/idx" + std::to_string(i) + ".txt";
	std::ofstream f(path);
	f << "#@TK\t" << 100000 + i << "\n#@KS\t19\n#locusID\tcountAT\tcountCG\tsumAT\tsumCG\tdistinctAT\tdistinctCG\n";
	for (unsigned s = 0; s < m; ++s)
		f << prefix << s << "\t" << (s * 7 + i * 3) % 11 << "\t" << (s * 5 + i) % 13 << "\t" << s + i << "\t" << s + 2 * i << "\t" << 1 + s % 4 << "\t2\n";
	return path;
}

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: eval_index_check DIR\n"); return 2; }
	const std::string dir = argv[1], store = dir + "/check.store", once = dir + "/check.once", alien = dir + "/check.alien", bad = dir + "/check.bad";
	const unsigned m = 37, dim = 3, min_cov = 2, n = 12;
	std::vector<std::string> files, scratch = { store, once, alien, bad, ix::path_of(store), ix::path_of(once), ix::path_of(bad) };
	for (const std::string &p : scratch) unlink(p.c_str());
	for (unsigned i = 0; i < n; ++i) files.push_back(counts_file(dir, (int) i, m));
	const std::string other = counts_file(dir, 99, m, "xs");

	/* synthetic matrices (an exact third has a full 64-bit significand), clouds and tallies */
	std::vector<long double> norm(m), rot((size_t) dim * m);
	for (unsigned s = 0; s < m; ++s) norm[s] = (long double) (s + 1) / 3.0L;
	for (size_t t = 0; t < rot.size(); ++t) rot[t] = -1.0L / (long double) (t + 7);
	std::vector<double> cloud((size_t) n * dim);
	std::vector<uint32_t> geno((size_t) n * 3);
	for (size_t t = 0; t < cloud.size(); ++t) cloud[t] = 0.25 * (double) t - 3.0;
	for (size_t t = 0; t < geno.size(); ++t) geno[t] = (uint32_t) (t * 2654435761u);
	const std::vector<char> matrices = ix::matrix_bytes(norm, rot);

	bool ok = true;
	st::pack(store, std::vector<std::string>(files.begin(), files.begin() + 8));
	st::pack(once, files);
	{
		st::View v;
		v.open(store);
		ix::write(ix::path_of(store), v, dim, min_cov, matrices, nullptr, 0, cloud.data(), geno.data(), 8);
	}
	{                                                     /* read back: header, matrices, every record */
		st::View v;
		v.open(store);
		ix::View x;
		x.open(ix::path_of(store));
		x.check_store(ix::path_of(store), v, false);
		std::vector<long double> norm2, rot2;
		x.matrices(norm2, rot2);
		bool same = x.h.n_samples == 8 && x.h.dim == dim && x.h.min_cov == min_cov && x.h.n_sites == m && norm2 == norm && rot2 == rot
		            && x.matrix_size() == matrices.size() && memcmp(x.matrices(), matrices.data(), matrices.size()) == 0;
		for (uint64_t r = 0; r < 8; ++r) {
			const ix::Entry e = x.entry(r);
			same = same && memcmp(e.cloud, &cloud[r * dim], 8 * dim) == 0 && e.hets == geno[3 * r] && e.homs == geno[3 * r + 1] && e.miss == geno[3 * r + 2];
		}
		printf("index of 8 samples reads back %s, %zu bytes\n", same ? "as written" : "DIFFERENT", bytes_of(ix::path_of(store)).size());
		ok = ok && same;
	}
	const std::string eight = bytes_of(ix::path_of(store));
	st::pack(store, std::vector<std::string>(files.begin() + 8, files.end()));
	ok = refused("a stale index", [&] { st::View v; v.open(store); ix::View x; x.open(ix::path_of(store)); x.check_store(ix::path_of(store), v, false); }) && ok;
	{                                                     /* append: the old records kept, four new ones */
		st::View v;
		v.open(store);
		ix::View x;
		x.open(ix::path_of(store));
		x.check_store(ix::path_of(store), v, true);
		ix::write(ix::path_of(store), v, dim, min_cov, matrices, x.records(), x.h.n_samples, &cloud[8 * dim], &geno[8 * 3], 4);
		st::View w;
		w.open(once);
		ix::write(ix::path_of(once), w, dim, min_cov, matrices, nullptr, 0, cloud.data(), geno.data(), n);
	}
	const std::string full = bytes_of(ix::path_of(store));
	const bool same = full == bytes_of(ix::path_of(once)) && full.size() == ix::first_of(m, dim) + n * ix::stride_of(dim);
	printf("extended index %s index written at once, %zu bytes\n", same ? "==" : "!=", full.size());
	ok = ok && same;

	/* validity failures: each a copy of the good index with one thing wrong, opened against the 12-sample store */
	const auto check = [&](const std::string &bytes) {
		put(ix::path_of(bad), bytes);
		st::View v;
		v.open(store);
		ix::View x;
		x.open(ix::path_of(bad));
		x.check_store(ix::path_of(bad), v, false);
	};
	const auto with = [&](size_t at, uint64_t value, size_t width) { std::string b = full; memcpy(&b[at], &value, width); return b; };
	ok = refused("magic", [&] { check("NTSMPCX2" + full.substr(8)); }) && ok;
	ok = refused("version", [&] { check(with(8, 2, 4)); }) && ok;
	ok = refused("a byte short", [&] { check(full.substr(0, full.size() - 1)); }) && ok;
	ok = refused("a byte long", [&] { check(full + std::string(1, '\0')); }) && ok;
	ok = refused("shorter than a header", [&] { check(full.substr(0, 40)); }) && ok;
	ok = refused("first record offset", [&] { check(with(40, ix::first_of(m, dim) + 16, 8)); }) && ok;
	ok = refused("record stride", [&] { check(with(48, ix::stride_of(dim) + 8, 8)); }) && ok;
	ok = refused("dim 0", [&] { check(with(24, 0, 4)); }) && ok;
	ok = refused("other number of sites", [&] { check(with(12, m + 1, 4)); }) && ok;
	ok = refused("CRC of the locus section", [&] { std::string b = full; b[32] = (char) (b[32] ^ 1); check(b); }) && ok;
	ok = refused("more samples than the store", [&] { check(with(16, n + 1, 8) + std::string(ix::stride_of(dim), '\0')); }) && ok;
	ok = refused("fewer samples than the store", [&] { check(eight); }) && ok;
	ok = refused("no index", [&] { ix::View x; x.open(dir + "/check.none.pcaidx"); }) && ok;
	{                                                     /* a store over other loci of the same number: only the CRC tells */
		st::pack(alien, { other });
		ok = refused("a store with other loci", [&] { st::View v; v.open(alien); ix::View x; x.open(ix::path_of(store)); x.check_store("index", v, true); }) && ok;
	}
	const bool kept = full == bytes_of(ix::path_of(store)) && !std::ifstream(ix::path_of(store) + ".tmp").good();
	printf("the index is %s after the refusals\n", kept ? "unchanged" : "CHANGED");
	ok = ok && kept;
	for (const std::string &p : scratch) unlink(p.c_str());
	for (const std::string &p : files) unlink(p.c_str());
	unlink(other.c_str());
	printf(ok ? "ok\n" : "FAILED\n");
	return ok ? 0 : 1;
}
