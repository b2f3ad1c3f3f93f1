/*
 * eval_store_check.cpp -- the writer and the reader of ntsm_amd/csrc/host/eval_store.hpp driven on their own, for a host
 * sanitizer run (`make store_check`: -fsanitize=address,undefined, no HIP, no GPU):
 *
 *     build/eval_store_check DIR FILES...
 *
 * packs FILES into DIR/check.store in two steps (the first half creates it, the second half is appended) and into
 * DIR/check.once at once, compares the two byte for byte, maps the result and walks every locus, scalar, name and count,
 * then asks for the refusals (a name already in the store, a truncated copy, an unknown locus when one of FILES is given a
 * second time under the name DIR/alien.txt by the caller).  Prints one line per step; exit status 0 when all held.
 */
#include <cstdio>
#include <fstream>
#include <iterator>

#include "../ntsm_amd/csrc/host/eval_store.hpp"

namespace st = ntsm::eval_store;

static std::string bytes_of(const std::string &path)
{
	std::ifstream f(path, std::ios::binary);
	return std::string(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

template <class F> static bool refused(const char *what, F f)
{
	try { f(); } catch (const st::Error &e) { printf("refused (%s): %s\n", what, e.what()); return true; }
	printf("NOT refused: %s\n", what);
	return false;
}

int main(int argc, char **argv)
{
	if (argc < 4) { fprintf(stderr, "usage: eval_store_check DIR FILE FILE...\n"); return 2; }
	const std::string dir = argv[1], a = dir + "/check.store", b = dir + "/check.once", cut = dir + "/check.cut";
	const std::vector<std::string> files(argv + 2, argv + argc);
	const size_t half = files.size() / 2;
	for (const std::string &p : { a, b, cut }) unlink(p.c_str());
	bool ok = true;
	st::pack(a, std::vector<std::string>(files.begin(), files.begin() + half));
	st::pack(a, std::vector<std::string>(files.begin() + half, files.end()));
	st::pack(b, files);
	const std::string bytes = bytes_of(a);
	ok = ok && bytes == bytes_of(b);
	printf("two steps %s one step, %zu bytes\n", ok ? "==" : "!=", bytes.size());
	{
		st::View v;
		v.open(a);
		ok = ok && v.h.n_samples == files.size();
		uint64_t sum = 0, distinct = st::sum_of_pairs(v.distinct, v.h.n_sites);
		size_t name_bytes = 0, locus_bytes = 0;
		for (const std::string &l : v.locus) locus_bytes += l.size();
		const st::LocusIndex ix = v.index();
		for (uint64_t r = 0; r < v.h.n_samples; ++r) {
			ok = ok && v.name(r) == files[r];
			name_bytes += v.name(r).size();
			sum += st::sum_of_pairs(v.counts(r), v.h.n_sites);
			const st::RecordHead &h = v.head(r);
			printf("%s: TK %llu, total %llu, sums %llu, k %u, error rate %.6f\n", v.name(r).c_str(), (unsigned long long) h.raw_total,
			       (unsigned long long) h.total, (unsigned long long) h.sum_of_sums, h.kmer_size,
			       st::error_rate(h.raw_total, h.kmer_size, h.sum_of_sums, distinct, 6200000000ull));
		}
		printf("%u sites (%zu locus bytes, %zu indexed), %llu samples (%zu name bytes), counts sum to %llu\n", v.h.n_sites, locus_bytes, ix.size(),
		       (unsigned long long) v.h.n_samples, name_bytes, (unsigned long long) sum);
	}
	ok = refused("a name already in the store", [&] { st::pack(a, { files[0] }); }) && ok;
	ok = refused("no input files", [&] { st::pack(a, {}); }) && ok;
	ok = refused("a name of 1,024 bytes", [&] { st::pack(a, { std::string(1024, 'x') }); }) && ok;
	{ std::ofstream f(cut, std::ios::binary); f.write(bytes.data(), (std::streamsize) bytes.size() - 1); }
	ok = refused("a store one byte short", [&] { st::View v; v.open(cut); }) && ok;
	{ std::ofstream f(cut, std::ios::binary); f.write(bytes.data(), 70); }
	ok = refused("a store cut inside its locus section", [&] { st::View v; v.open(cut); }) && ok;
	if (std::ifstream(dir + "/alien.txt").good())
		ok = refused("a locus the store does not know", [&] { st::pack(a, { dir + "/alien.txt" }); }) && ok;
	ok = ok && bytes == bytes_of(a);
	printf("the store is %s after the refusals\n", bytes == bytes_of(a) ? "unchanged" : "CHANGED");
	for (const std::string &p : { a, b, cut }) unlink(p.c_str());
	printf(ok ? "ok\n" : "FAILED\n");
	return ok ? 0 : 1;
}
