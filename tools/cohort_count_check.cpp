/*
 * cohort_count_check.cpp -- the host side of `ntsmCount --cohort` (ntsm_amd/csrc/host/cohort.hpp) driven on its own, for a
 * host sanitizer run (`make cohort_check`: -fsanitize=address,undefined, no HIP, no GPU):
 *
 *     build/cohort_count_check DIR
 *
 * 1. the manifest parser: a manifest with comments, empty lines and several read files per sample, and every shape it refuses;
 * 2. the site set as lists: offsets, indices and distinct columns of a small set, and the three sets it refuses;
 * 3. the record builder against the route it replaces: random per-site counts and sums (with pairs whose sum wraps at 2^32)
 *    are turned into records and appended to a store the way a cohort run does it -- all at once, and in two runs --, the same
 *    arrays are printed as counts text with print_counts_max's formatting and packed with eval_store::pack, and the stores
 *    are compared byte for byte; then the stores a run must refuse to append to.
 * Prints one line per step; exit status 0 when all held.
 */
#include <cstdio>
#include <fstream>
#include <iterator>
#include <random>
#include <sstream>

#include "../ntsm_amd/csrc/host/cohort.hpp"
#include "../ntsm_amd/csrc/host/report.hpp"

namespace st = ntsm::eval_store;
namespace co = ntsm::cohort;

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

static std::vector<co::Sample> manifest_of(const std::string &text)
{
	std::istringstream in(text);
	return co::parse_manifest(in, "MANIFEST");
}

struct Sample {
	std::string name;
	uint64_t raw_total;
	std::vector<uint32_t> counts, sums;
};

/* the two sums as the contract of ntsm_sites_reduce states them */
static uint64_t wrapped_pairs(const std::vector<uint32_t> &v)
{
	uint64_t s = 0;
	for (size_t i = 0; i + 1 < v.size(); i += 2) s += (uint64_t) (uint32_t) (v[i] + v[i + 1]);
	return s;
}

static void append_samples(const std::string &path, const std::vector<std::string> &ids, const std::vector<uint32_t> &distinct,
		const std::vector<Sample> &samples, size_t from, size_t to, unsigned k)
{
	co::Store store;
	store.open_existing(path);
	store.check(ids, distinct);
	store.begin(ids, distinct);
	std::vector<char> rec;
	for (size_t i = from; i < to; ++i) {
		const Sample &s = samples[i];
		co::build_record(rec, store.header(), s.name, s.raw_total, k, s.counts.data(), wrapped_pairs(s.counts), wrapped_pairs(s.sums));
		store.append(rec, s.name);
	}
}

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: cohort_count_check DIR\n"); return 2; }
	const std::string dir = argv[1];
	bool ok = true;

	/* 1. the manifest */
	{
		const std::vector<co::Sample> m = manifest_of("# a cohort\n\nalpha\ta_1.fq\ta_2.fq\r\nbeta\tb.fq.gz\n#gamma\tc.fq\ndelta one\td.fq");
		const bool good = m.size() == 3 && m[0].name == "alpha" && m[0].reads == std::vector<std::string>({ "a_1.fq", "a_2.fq" }) && m[1].name == "beta"
		                  && m[1].reads.size() == 1 && m[2].name == "delta one" && m[2].reads[0] == "d.fq";
		printf("manifest: %zu samples %s\n", m.size(), good ? "as written" : "FAILED");
		ok = ok && good;
		ok = refused("a line without read files", [] { manifest_of("alpha\n"); }) && ok;
		ok = refused("an empty read file field", [] { manifest_of("alpha\ta.fq\t\n"); }) && ok;
		ok = refused("an empty name", [] { manifest_of("\ta.fq\n"); }) && ok;
		ok = refused("spaces instead of a tab", [] { manifest_of("alpha a.fq\n"); }) && ok;
		ok = refused("no sample", [] { manifest_of("# nothing\n\n"); }) && ok;
		ok = refused("a name listed twice", [] { manifest_of("alpha\ta.fq\nbeta\tb.fq\nalpha\tc.fq\n"); }) && ok;
		ok = refused("a name of 1,024 bytes", [] { manifest_of(std::string(1024, 'x') + "\ta.fq\n"); }) && ok;
		const bool longest = manifest_of(std::string(1023, 'x') + "\ta.fq\n").size() == 1;
		printf("a name of 1,023 bytes %s\n", longest ? "accepted" : "FAILED");
		ok = ok && longest;
		ok = refused("a read file that does not exist", [&] { co::check_reads_exist(manifest_of("alpha\t" + dir + "/no_such_reads.fq\n")); }) && ok;
	}

	/* 2. the site set as lists */
	{
		ntsm::SiteSet s;
		s.ids = { "rs1", "rs2", "rs3" };
		s.ref = { { 0, 1, 2 }, {}, { 5 } };
		s.var = { { 3 }, {}, { 4, 6 } };
		s.keys.assign(7, 0);
		const co::SiteLists l = co::site_lists(s);
		const bool good = l.offsets == std::vector<uint32_t>({ 0, 3, 4, 4, 4, 5, 7 }) && l.kmer_ix == std::vector<uint32_t>({ 0, 1, 2, 3, 5, 4, 6 })
		                  && l.distinct == std::vector<uint32_t>({ 3, 1, 0, 0, 1, 2 });
		printf("site lists: %zu offsets, %zu indices %s\n", l.offsets.size(), l.kmer_ix.size(), good ? "as expected" : "FAILED");
		ok = ok && good;
		ntsm::SiteSet erased = s, twice = s, odd = s;
		erased.ref[2][0] = ntsm::SiteSet::kErased;
		twice.ids[2] = "rs1";
		odd.var.pop_back();
		ok = refused("an erased k-mer", [&] { co::site_lists(erased); }) && ok;
		ok = refused("a repeated locus", [&] { co::site_lists(twice); }) && ok;
		ok = refused("a REF record without VAR", [&] { co::site_lists(odd); }) && ok;
		ntsm::SiteSet none;
		const co::SiteLists e = co::site_lists(none);
		ok = ok && e.offsets.size() == 1 && e.kmer_ix.empty();
	}

	/* 3. records against counts text + pack */
	std::mt19937_64 rng(20261019);
	for (const size_t n_sites : { (size_t) 37, (size_t) 1, (size_t) 0 }) {
		const unsigned k = 19;
		const size_t n_samples = 5, split = 2;
		std::vector<std::string> ids;
		std::vector<uint32_t> distinct;
		for (size_t i = 0; i < n_sites; ++i) {
			ids.push_back("rs" + std::to_string(1000 + 7 * i));
			distinct.push_back((uint32_t) (rng() % 37));
			distinct.push_back((uint32_t) (rng() % 37));
		}
		std::vector<Sample> samples(n_samples);
		std::vector<std::string> files;
		for (size_t r = 0; r < n_samples; ++r) {
			Sample &s = samples[r];
			s.name = dir + "/n" + std::to_string(n_sites) + "_sample" + std::to_string(r) + ".txt";
			s.raw_total = r == 3 ? 0 : rng() >> (r * 9);
			for (size_t i = 0; i < 2 * n_sites; ++i) {
				const unsigned kind = (unsigned) (rng() % 6);
				const uint32_t small = (uint32_t) (rng() % 200), big = (uint32_t) rng();
				s.counts.push_back(kind == 0 ? 0u : kind == 1 ? 0xFFFFFFFFu : kind == 2 ? 0x80000000u + small : kind == 3 ? big : small);
				s.sums.push_back(kind == 0 ? 0u : kind == 1 ? 0xFFFFFFFFu : kind == 2 ? 0x80000001u : kind == 3 ? (uint32_t) rng() : small * 3u);
			}
			if (n_sites >= 2) {                                /* pairs whose sum wraps, exactly to 0 and past it */
				s.counts[0] = 0xFFFFFFFFu; s.counts[1] = 1u; s.counts[2] = 0xFFFFFFF0u; s.counts[3] = 0x20u;
				s.sums[0] = 0x80000000u; s.sums[1] = 0x80000000u; s.sums[2] = 0xFFFFFFFFu; s.sums[3] = 0xFFFFFFFFu;
			}
			std::ofstream out(s.name, std::ios::binary);
			ntsm::print_optional_header(out, s.raw_total, k);
			ntsm::print_counts_rows(out, ids, s.counts.data(), s.sums.data(), distinct.data());
			files.push_back(s.name);
		}
		const std::string tag = dir + "/n" + std::to_string(n_sites);
		const std::string once = tag + ".cohort_once", two = tag + ".cohort_two", packed = tag + ".packed", packed_two = tag + ".packed_two";
		for (const std::string &p : { once, two, packed, packed_two }) unlink(p.c_str());
		append_samples(once, ids, distinct, samples, 0, n_samples, k);
		append_samples(two, ids, distinct, samples, 0, split, k);
		const std::string after_first = bytes_of(two);
		append_samples(two, ids, distinct, samples, split, n_samples, k);
		{
			st::pack(packed, files);
			st::pack(packed_two, std::vector<std::string>(files.begin(), files.begin() + split));
			const bool first_same = bytes_of(packed_two) == after_first;
			st::pack(packed_two, std::vector<std::string>(files.begin() + split, files.end()));
			const std::string want = bytes_of(packed);
			const bool same = !want.empty() && bytes_of(once) == want && bytes_of(two) == want && bytes_of(packed_two) == want && first_same;
			printf("%zu sites, %zu samples: cohort store %s packed store (%zu bytes; created at once, appended in two runs, after the first run)\n", n_sites,
			       n_samples, same ? "==" : "!= FAILED", want.size());
			ok = ok && same;
			st::View v;
			v.open(once);
			uint64_t wraps = 0;
			for (uint64_t r = 0; r < v.h.n_samples; ++r) {
				uint64_t plain = 0;
				for (size_t i = 0; i < 2 * n_sites; ++i) plain += v.counts(r)[i];
				wraps += plain != v.head(r).total ? 1 : 0;
				ok = ok && v.head(r).total == wrapped_pairs(samples[r].counts) && v.head(r).sum_of_sums == wrapped_pairs(samples[r].sums);
			}
			printf("%llu of %llu records hold a total that wrapped at 2^32\n", (unsigned long long) wraps, (unsigned long long) v.h.n_samples);
			ok = ok && (n_sites < 2 || wraps == v.h.n_samples);
		}
		if (n_sites == 37) {                                   /* what a run refuses to append to, each leaving the store as it was */
			const std::string before = bytes_of(once);
			std::vector<std::string> fewer(ids.begin(), ids.end() - 1), renamed = ids, swapped = ids;
			renamed[5] = "rsX";
			std::swap(swapped[1], swapped[2]);
			std::vector<uint32_t> other = distinct;
			other[11] += 1;
			auto against = [&](const std::vector<std::string> &i, const std::vector<uint32_t> &d) {
				co::Store s;
				s.open_existing(once);
				s.check(i, d);
			};
			ok = refused("a store with another number of loci", [&] { against(fewer, std::vector<uint32_t>(distinct.begin(), distinct.end() - 2)); }) && ok;
			ok = refused("a store with another locus", [&] { against(renamed, distinct); }) && ok;
			ok = refused("a store with the loci in another order", [&] { against(swapped, distinct); }) && ok;
			ok = refused("a store with other distinct columns", [&] { against(ids, other); }) && ok;
			const std::string cut = tag + ".cut";
			{ std::ofstream f(cut, std::ios::binary); f.write(before.data(), (std::streamsize) before.size() - 8); }
			ok = refused("a truncated store", [&] { co::Store s; s.open_existing(cut); }) && ok;
			co::Store s;
			s.open_existing(once);
			const bool holds = s.holds(samples[1].name) && !s.holds("elsewhere") && s.n_samples() == n_samples;
			printf("names of the store %s\n", holds ? "found" : "FAILED");
			ok = ok && holds && bytes_of(once) == before;
		}
	}
	printf("%s\n", ok ? "ok" : "FAILED");
	return ok ? 0 : 1;
}
