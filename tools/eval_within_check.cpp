/*
 * tools/eval_within_check.cpp -- ntsm_amd/csrc/host/eval_within.hpp against brute force, as a program of its own under the
 * host sanitizers (`make within_check`; tests/test_eval_within.py runs it).  No GPU, no files.
 *   band offsets: for n = 1 ... 70 and every (row_first, n_rows), the band's records are exactly the pairs of its rows, in
 *                 ntsm_eval_pair_index order, each at its band_offset;
 *   band rule:    band_rows against a linear scan for small limits, the 1 GiB rule on 4,096 and 100,000 samples, and the
 *                 bands of a triangle tiling it;
 *   pass packing: random lists -- every pair in exactly one pass, passes contiguous and in list order, both samples of a
 *                 pair in its pass at the slots it names, distinct samples per pass <= chunk, and no pass closed early.
 * Prints one line per part and "ok"; any failure prints what failed and exits 1.
 */
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "../include/ntsm_eval_hip.h"
#include "../ntsm_amd/csrc/host/eval_within.hpp"

namespace w = ntsm::eval_within;

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static void band_offsets()
{
	uint64_t bands = 0;
	for (uint32_t n = 1; n <= 70; ++n) {
		CHECK(w::band_base(n, n) == (uint64_t) n * (n - 1) / 2, "n %u", n);
		for (uint32_t first = 0; first < n; ++first)
			for (uint32_t rows = 1; first + rows <= n; ++rows) {
				uint64_t at = 0;                                                /* brute force: walk the band's pairs in order */
				for (uint32_t i = first; i < first + rows; ++i)
					for (uint32_t j = i + 1; j < n; ++j, ++at) {
						CHECK(w::band_offset(i, j, first, n) == at, "n %u band (%u, %u) pair (%u, %u)", n, first, rows, i, j);
						CHECK(ntsm_eval_pair_index(i, j, n) - ntsm_eval_pair_index(first, first + 1, n) == at, "n %u pair (%u, %u)", n, i, j);
					}
				CHECK(w::band_records(first, rows, n) == at, "n %u band (%u, %u): %llu records, %llu pairs", n, first, rows,
				      (unsigned long long) w::band_records(first, rows, n), (unsigned long long) at);
				++bands;
			}
	}
	printf("band offsets: %llu bands of n = 1 ... 70 equal the walk over their pairs\n", (unsigned long long) bands);
}

static void band_rule()
{
	uint64_t asked = 0;
	for (uint32_t n = 2; n <= 40; ++n)
		for (uint32_t first = 0; first < n; ++first)
			for (uint64_t limit = 0; limit <= (uint64_t) n * n / 2 + 1; ++limit, ++asked) {
				uint32_t want = 1;                                              /* the most rows that fit, and at least one */
				while (first + want < n && w::band_records(first, want + 1, n) <= limit) ++want;
				CHECK(w::band_rows(first, n, limit) == want, "n %u first %u limit %llu: %u, want %u", n, first, (unsigned long long) limit,
				      w::band_rows(first, n, limit), want);
			}
	CHECK(w::kBandRecords * sizeof(ntsm_eval_record) == 1ull << 30, "the rule is 1 GiB of records");
	CHECK(w::band_rows(0, 4096, w::kBandRecords) == 4096, "4,096 samples are one band");
	CHECK(w::band_records(0, 4096, 4096) * 64 == 536739840ull, "... of 537 MB");
	for (const uint32_t n : { 5794u, 100000u, 4000000000u }) {                  /* the bands tile the triangle, each within the rule */
		uint64_t total = 0;
		uint32_t bands = 0;
		for (uint32_t first = 0; first < n; ++bands) {
			const uint32_t rows = w::band_rows(first, n, w::kBandRecords);
			CHECK(rows >= 1 && (uint64_t) first + rows <= n, "n %u first %u rows %u", n, first, rows);
			const uint64_t rec = w::band_records(first, rows, n);
			CHECK(rec <= w::kBandRecords || rows == 1, "n %u first %u: %llu records", n, first, (unsigned long long) rec);
			if ((uint64_t) first + rows < n) CHECK(w::band_records(first, rows + 1, n) > w::kBandRecords, "n %u first %u: a row more fits", n, first);
			total += rec;
			first += rows;
			if (n > 1000000u && bands == 3) { total = w::band_base(n, n); break; }   /* a row of 4e9 pairs is a band of its own: a few suffice */
		}
		CHECK(total == w::band_base(n, n), "n %u: the bands hold %llu records", n, (unsigned long long) total);
	}
	printf("band rule: %llu (n, row_first, limit) equal the linear scan; 4,096 samples are one band of 537 MB\n", (unsigned long long) asked);
}

static void pass_packing()
{
	std::mt19937_64 rng(22);
	uint64_t lists = 0, passes = 0;
	for (int round = 0; round < 400; ++round) {
		const uint32_t n_db = 2 + (uint32_t) (rng() % 60), chunk = 2 + (uint32_t) (rng() % 12);
		const uint64_t n_pairs = rng() % 200;
		std::vector<uint32_t> pi(n_pairs), pk(n_pairs);
		const uint32_t hub = (uint32_t) (rng() % n_db);                         /* a sample named by many pairs */
		for (uint64_t p = 0; p < n_pairs; ++p) {
			pi[p] = rng() % 3 == 0 ? hub : (uint32_t) (rng() % n_db);
			do pk[p] = (uint32_t) (rng() % n_db); while (pk[p] == pi[p]);
		}
		const w::Passes cut = w::pack_passes(pi.data(), pk.data(), n_pairs, n_db, chunk);
		CHECK(cut.pair_begin.size() == cut.sample_begin.size() && cut.slot_i.size() == n_pairs && cut.slot_k.size() == n_pairs, "sizes");
		CHECK(cut.pair_begin[0] == 0 && cut.sample_begin[0] == 0, "the first pass starts the list");
		if (n_pairs == 0) { CHECK(cut.passes() == 0, "an empty list has no pass"); continue; }
		CHECK(cut.pair_begin.back() == n_pairs && cut.sample_begin.back() == cut.sample.size(), "the last pass ends the list");
		for (size_t x = 0; x < cut.passes(); ++x) {
			const uint64_t p0 = cut.pair_begin[x], p1 = cut.pair_begin[x + 1], s0 = cut.sample_begin[x], s1 = cut.sample_begin[x + 1];
			CHECK(p0 < p1 && s0 < s1, "pass %zu is empty", x);                    /* contiguous and ascending: every pair in exactly one pass, in list order */
			CHECK(s1 - s0 <= chunk, "pass %zu holds %llu samples, chunk %u", x, (unsigned long long) (s1 - s0), chunk);
			std::set<uint32_t> named, held(cut.sample.begin() + s0, cut.sample.begin() + s1);
			CHECK(held.size() == s1 - s0, "pass %zu holds a sample twice", x);
			for (uint64_t p = p0; p < p1; ++p) {
				CHECK(cut.slot_i[p] < s1 - s0 && cut.sample[s0 + cut.slot_i[p]] == pi[p], "pair %llu: slot of sample 1", (unsigned long long) p);
				CHECK(cut.slot_k[p] < s1 - s0 && cut.sample[s0 + cut.slot_k[p]] == pk[p], "pair %llu: slot of sample 2", (unsigned long long) p);
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
	printf("pass packing: %llu random lists in %llu passes\n", (unsigned long long) lists, (unsigned long long) passes);
}

int main()
{
	band_offsets();
	band_rule();
	pass_packing();
	printf("ok\n");
	return 0;
}
