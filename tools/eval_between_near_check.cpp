/*
 * tools/eval_between_near_check.cpp -- what ntsmEval --between-near decides on the host, as a program
 * of its own under the host sanitizers (`make between_near_check`; tests/test_eval_between_near.py runs it).  No GPU, no files.
 *   B's index: ntsm::eval_between::b_index_usable says yes for an index that exists, is valid and current, over A's locus
 *              table, with A's -d, -c and matrix bytes -- and no for each of those facts alone turned the other way;
 *   dense runs: dense_runs groups the samples of A whose radius is DBL_MAX into runs of consecutive rows, against a linear
 *              scan over random radii of the three classes, and on none, all, the first and the last sample;
 *   pass cut:  eval_within.hpp's pack_passes on random lists that name one sample of each store in the numbering of the
 *              concatenation, either orientation, with a hub sample of each store: contiguous passes in list order, at most
 *              `chunk` distinct samples of both stores together, slots that name the pair's samples, greedy.
 * Prints one line per part and "ok"; any failure prints what failed and exits 1.
 */
#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "../ntsm_amd/csrc/host/eval_between.hpp"
#include "../ntsm_amd/csrc/host/eval_within.hpp"

namespace b = ntsm::eval_between;
namespace w = ntsm::eval_within;

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static void b_index()
{
	const std::vector<char> mat { 1, 2, 3, 4, 5, 6, 7, 8 }, same = mat;
	std::vector<char> other = mat, shorter(mat.begin(), mat.end() - 1);
	other[5] ^= 1;
	b::BIndexFacts yes;
	yes.exists = yes.valid = yes.current = yes.identical_loci = true;
	yes.dim_a = yes.dim_b = 20;
	yes.min_cov_a = yes.min_cov_b = 1;
	yes.matrices_a = mat.data(); yes.matrix_size_a = mat.size();
	yes.matrices_b = same.data(); yes.matrix_size_b = same.size();             /* equal bytes at another address */
	CHECK(b::b_index_usable(yes), "an index that fits in every respect serves");

	unsigned reasons = 0;
	const auto no = [&](b::BIndexFacts f, const char *what) {
		CHECK(!b::b_index_usable(f), "%s: the index must not serve", what);
		++reasons;
	};
	b::BIndexFacts f = yes; f.exists = false; no(f, "no index");
	f = yes; f.valid = false; no(f, "an invalid index");
	f = yes; f.current = false; no(f, "a stale index");
	f = yes; f.identical_loci = false; no(f, "a mapped B");
	f = yes; f.dim_b = 19; no(f, "another -d");
	f = yes; f.dim_a = 21; no(f, "another -d, from A's side");
	f = yes; f.min_cov_b = 2; no(f, "another -c");
	f = yes; f.matrices_b = other.data(); no(f, "other matrix bytes");
	f = yes; f.matrices_b = shorter.data(); f.matrix_size_b = shorter.size(); no(f, "matrices of another size");
	f = yes; f.matrices_b = nullptr; no(f, "no matrices");
	f = b::BIndexFacts {}; no(f, "nothing known");
	f = yes; f.exists = false; f.valid = false; f.current = false; no(f, "absent, whatever else is said");
	printf("B's index: serves when every fact fits; %u single reasons each say no\n", reasons);
}

static void dense_rows()
{
	const double small = 4.0, large = 225.0, all = DBL_MAX;
	typedef std::vector<std::pair<uint32_t, uint32_t>> Runs;
	CHECK(b::dense_runs(nullptr, 0, all).empty(), "no sample, no run");
	const double none[] = { small, large, small }, every[] = { all, all, all, all }, ends[] = { all, small, all, all, large, all };
	CHECK(b::dense_runs(none, 3, all).empty(), "no search-all sample");
	CHECK(b::dense_runs(every, 4, all) == (Runs { { 0, 4 } }), "every sample: one run");
	CHECK(b::dense_runs(ends, 6, all) == (Runs { { 0, 1 }, { 2, 2 }, { 5, 1 } }), "first, a pair, last");
	CHECK(b::dense_runs(every, 1, all) == (Runs { { 0, 1 } }), "one sample");

	std::mt19937_64 rng(95);
	uint64_t lists = 0, total_runs = 0;
	for (int round = 0; round < 500; ++round) {
		const uint32_t n = (uint32_t) (rng() % 70);
		const unsigned odds = 1 + (unsigned) (rng() % 6);                       /* from mostly dense to mostly not */
		std::vector<double> radius(n);
		for (double &r : radius) r = rng() % odds == 0 ? all : rng() % 2 ? small : large;
		const Runs runs = b::dense_runs(radius.data(), n, all);
		std::vector<bool> covered(n, false);                                    /* the linear scan: every dense row in exactly one run, runs maximal and ascending */
		uint32_t next = 0;
		for (const auto &run : runs) {
			CHECK(run.second >= 1 && run.first >= next && (uint64_t) run.first + run.second <= n, "round %d: run (%u, %u)", round, run.first, run.second);
			CHECK(run.first == 0 || radius[run.first - 1] < all, "round %d: run at %u starts late", round, run.first);
			CHECK(run.first + run.second == n || radius[run.first + run.second] < all, "round %d: run at %u ends early", round, run.first);
			for (uint32_t r = 0; r < run.second; ++r) covered[run.first + r] = true;
			next = run.first + run.second + 1;
		}
		for (uint32_t a = 0; a < n; ++a) CHECK(covered[a] == !(radius[a] < all), "round %d: sample %u", round, a);
		total_runs += runs.size();
		++lists;
	}
	printf("dense runs: none, all, the ends; %llu random radius lists in %llu runs equal the linear scan\n", (unsigned long long) lists,
	       (unsigned long long) total_runs);
}

static void pass_cut()
{
	std::mt19937_64 rng(96);
	uint64_t lists = 0, passes = 0;
	for (int round = 0; round < 400; ++round) {
		const uint32_t n_a = 1 + (uint32_t) (rng() % 30), n_b = 1 + (uint32_t) (rng() % 40), chunk = 2 + (uint32_t) (rng() % 12);
		const uint64_t n_pairs = rng() % 200;
		std::vector<uint32_t> pi(n_pairs), pk(n_pairs);
		const uint32_t hub_a = (uint32_t) (rng() % n_a), hub_b = n_a + (uint32_t) (rng() % n_b);   /* a sample of each store that many pairs name */
		for (uint64_t p = 0; p < n_pairs; ++p) {
			uint32_t a = rng() % 4 == 0 ? hub_a : (uint32_t) (rng() % n_a), bb = rng() % 4 == 0 ? hub_b : n_a + (uint32_t) (rng() % n_b);
			if (rng() % 2) std::swap(a, bb);                                    /* the owner rule puts either store first */
			pi[p] = a;
			pk[p] = bb;
		}
		const w::Passes cut = w::pack_passes(pi.data(), pk.data(), n_pairs, n_a + n_b, chunk);
		CHECK(cut.pair_begin.size() == cut.sample_begin.size() && cut.slot_i.size() == n_pairs && cut.slot_k.size() == n_pairs, "sizes");
		if (n_pairs == 0) { CHECK(cut.passes() == 0, "an empty list has no pass"); continue; }
		CHECK(cut.pair_begin[0] == 0 && cut.pair_begin.back() == n_pairs && cut.sample_begin.back() == cut.sample.size(), "the passes cover the list");
		for (size_t x = 0; x < cut.passes(); ++x) {
			const uint64_t p0 = cut.pair_begin[x], p1 = cut.pair_begin[x + 1], s0 = cut.sample_begin[x], s1 = cut.sample_begin[x + 1];
			CHECK(p0 < p1 && s0 < s1 && s1 - s0 <= chunk, "pass %zu: %llu pairs over %llu samples, chunk %u", x, (unsigned long long) (p1 - p0),
			      (unsigned long long) (s1 - s0), chunk);
			std::set<uint32_t> named, held(cut.sample.begin() + s0, cut.sample.begin() + s1);
			CHECK(held.size() == s1 - s0 && *held.rbegin() < n_a + n_b, "pass %zu holds a sample twice or one past both stores", x);
			for (uint64_t p = p0; p < p1; ++p) {
				CHECK(cut.slot_i[p] < s1 - s0 && cut.sample[s0 + cut.slot_i[p]] == pi[p], "pair %llu: slot of sample 1", (unsigned long long) p);
				CHECK(cut.slot_k[p] < s1 - s0 && cut.sample[s0 + cut.slot_k[p]] == pk[p], "pair %llu: slot of sample 2", (unsigned long long) p);
				CHECK((pi[p] < n_a) != (pk[p] < n_a), "pair %llu names one store twice", (unsigned long long) p);
				named.insert(pi[p]);
				named.insert(pk[p]);
			}
			CHECK(named == held, "pass %zu holds a sample no pair of it names", x);
			if (p1 < n_pairs) {                                                 /* greedy: the next pair did not fit */
				named.insert(pi[p1]);
				named.insert(pk[p1]);
				CHECK(named.size() > chunk, "pass %zu closed although pair %llu fits", x, (unsigned long long) p1);
			}
			++passes;
		}
		++lists;
	}
	printf("pass cut: %llu random two-store lists in %llu passes\n", (unsigned long long) lists, (unsigned long long) passes);
}

int main()
{
	b_index();
	dense_rows();
	pass_cut();
	printf("ok\n");
	return 0;
}
