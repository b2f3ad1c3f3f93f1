/*
 * tools/eval_between_check.cpp -- ntsm_amd/csrc/host/eval_between.hpp on its cases, as a program of its own under the host
 * sanitizers (`make between_check`; tests/test_eval_between.py runs it).  No GPU, no files.
 *   locus map: identical tables; a permutation; B lacking A's first and last locus; a locus of B that A lacks; a locus that
 *              stands twice, in A and in B; tables of one site; random tables against a linear search; what valid_map takes;
 *   band rule: a rectangle whose one row passes the limit gives 1 row, one that fits whole gives all rows, and the bands of
 *              a rectangle tile it, each within the rule and none a row short.
 * Prints one line per part and "ok"; any failure prints what failed and exits 1.
 */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../include/ntsm_eval_hip.h"
#include "../ntsm_amd/csrc/host/eval_between.hpp"

namespace b = ntsm::eval_between;
typedef std::vector<std::string> Loci;

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

/* the refusal's sentence, or "" where the map is built */
static std::string refusal(const Loci &a, const Loci &bb)
{
	try {
		(void) b::map_loci(a, bb, "A.store", "B.store");
	} catch (const ntsm::eval_store::Error &e) {
		return e.what();
	}
	return "";
}

static bool has(const std::string &s, const char *part) { return s.find(part) != std::string::npos; }

static void locus_map()
{
	const Loci a { "rs1", "rs2", "rs3", "rs4", "rs5" };
	b::LocusMap m = b::map_loci(a, a, "A", "B");                                /* identity */
	CHECK(m.identical && m.site_map.empty() && m.lacking == 0 && m.data() == nullptr, "identical tables are the identity");

	m = b::map_loci(a, Loci { "rs4", "rs1", "rs5", "rs3", "rs2" }, "A", "B");   /* a permutation */
	CHECK(!m.identical && m.lacking == 0 && m.site_map == (std::vector<uint32_t> { 1, 4, 3, 0, 2 }) && m.data() == m.site_map.data(), "permutation");
	CHECK(b::valid_map(m.data(), 5, 5), "a permutation is a valid map");

	m = b::map_loci(a, Loci { "rs2", "rs3", "rs4" }, "A", "B");                 /* B lacks A's first and last locus */
	CHECK(!m.identical && m.lacking == 2 && m.site_map == (std::vector<uint32_t> { b::kLacks, 0, 1, 2, b::kLacks }), "first and last lacking");
	CHECK(b::valid_map(m.data(), 5, 3), "... is a valid map");

	m = b::map_loci(a, Loci {}, "A", "B");                                      /* B without loci lacks them all */
	CHECK(!m.identical && m.lacking == 5 && std::count(m.site_map.begin(), m.site_map.end(), b::kLacks) == 5, "an empty B");

	std::string why = refusal(a, Loci { "rs1", "rsX", "rs2" });                 /* an unknown ID */
	CHECK(has(why, "rsX") && has(why, "B.store") && has(why, "is not in A.store"), "unknown ID: %s", why.c_str());
	why = refusal(a, Loci { "rs1", "rs2", "rs1" });                             /* a duplicate ID in B */
	CHECK(has(why, "rs1") && has(why, "twice in B.store"), "duplicate in B: %s", why.c_str());
	why = refusal(Loci { "rs1", "rs2", "rs2" }, Loci { "rs1", "rs2" });         /* ... in A */
	CHECK(has(why, "rs2") && has(why, "twice in A.store"), "duplicate in A: %s", why.c_str());
	why = refusal(Loci { "rs7", "rs7" }, Loci { "rs7", "rs7" });                /* ... in both, the tables identical */
	CHECK(has(why, "rs7") && has(why, "twice in A.store"), "duplicate in identical tables: %s", why.c_str());

	m = b::map_loci(Loci { "only" }, Loci { "only" }, "A", "B");                /* one site */
	CHECK(m.identical, "one site, identical");
	m = b::map_loci(Loci { "only" }, Loci {}, "A", "B");
	CHECK(!m.identical && m.lacking == 1 && m.site_map == (std::vector<uint32_t> { b::kLacks }), "one site, lacking");
	CHECK(has(refusal(Loci { "only" }, Loci { "other" }), "other"), "one site, unknown");

	std::mt19937_64 rng(94);                                                    /* random tables against a linear search */
	uint64_t tables = 0;
	for (int round = 0; round < 200; ++round) {
		const size_t n = 1 + rng() % 80;
		Loci ta(n), tb;
		for (size_t s = 0; s < n; ++s) ta[s] = "rs" + std::to_string(1000 + s * 7);
		for (size_t s = 0; s < n; ++s)
			if (rng() % 5) tb.push_back(ta[s]);
		std::shuffle(tb.begin(), tb.end(), rng);
		m = b::map_loci(ta, tb, "A", "B");
		CHECK(m.identical == (ta == tb), "round %d: identity", round);
		if (m.identical) continue;
		CHECK(m.site_map.size() == n && m.lacking == n - tb.size() && b::valid_map(m.data(), (uint32_t) n, (uint32_t) tb.size()), "round %d: sizes", round);
		for (size_t s = 0; s < n; ++s) {
			const auto at = std::find(tb.begin(), tb.end(), ta[s]);
			CHECK(m.site_map[s] == (at == tb.end() ? b::kLacks : (uint32_t) (at - tb.begin())), "round %d: site %zu", round, s);
		}
		++tables;
	}

	const uint32_t twice[] = { 0, b::kLacks, 0 }, past[] = { 0, 3, 1 }, fine[] = { 2, b::kLacks, 0 };
	CHECK(!b::valid_map(twice, 3, 3) && !b::valid_map(past, 3, 3) && b::valid_map(fine, 3, 3) && b::valid_map(fine, 0, 0), "valid_map");
	printf("locus map: identity, permutation, lacking ends, unknown and duplicate IDs, one site; %llu random tables equal the linear search\n",
	       (unsigned long long) tables);
}

static void band_rule()
{
	CHECK(b::kBandRecords * sizeof(ntsm_eval_record) == 1ull << 30, "the rule is 1 GiB of records");
	CHECK(b::band_rows(0, 1000, 4096, 4095) == 1 && b::band_rows(0, 1000, 4096, 0) == 1, "a row of more records than the limit is a band of its own");
	CHECK(b::band_rows(0, 8, 0x10000000u, b::kBandRecords) == 1, "2^28 samples of B: 1 row");
	CHECK(b::band_rows(0, 1024, 4096, b::kBandRecords) == 1024, "1,024 x 4,096 is one band");
	CHECK(b::band_rows(0, 4096, 4096, b::kBandRecords) == 4096, "4,096 x 4,096 fits exactly");
	CHECK(b::band_rows(0, 4097, 4096, b::kBandRecords) == 4096 && b::band_rows(4096, 4097, 4096, b::kBandRecords) == 1, "4,097 x 4,096 is two bands");
	uint64_t asked = 0;
	for (uint32_t n_a = 1; n_a <= 40; ++n_a)
		for (uint32_t n_b = 1; n_b <= 12; ++n_b)
			for (uint64_t limit = 0; limit <= (uint64_t) n_a * n_b + 1; limit += 1 + limit / 7) {
				uint64_t total = 0;
				for (uint32_t first = 0; first < n_a; ++asked) {                    /* the bands tile the rectangle, each within the rule, none a row short */
					const uint32_t rows = b::band_rows(first, n_a, n_b, limit);
					CHECK(rows >= 1 && first + rows <= n_a, "%u x %u limit %llu first %u: %u rows", n_a, n_b, (unsigned long long) limit, first, rows);
					CHECK((uint64_t) rows * n_b <= limit || rows == 1, "%u x %u limit %llu first %u: %u rows pass the limit", n_a, n_b, (unsigned long long) limit, first, rows);
					if (first + rows < n_a) CHECK((uint64_t) (rows + 1) * n_b > limit, "%u x %u limit %llu first %u: a row more fits", n_a, n_b, (unsigned long long) limit, first);
					total += (uint64_t) rows * n_b;
					first += rows;
				}
				CHECK(total == (uint64_t) n_a * n_b, "%u x %u: the bands hold %llu records", n_a, n_b, (unsigned long long) total);
			}
	printf("band rule: 1 row where a row passes the limit, all rows where the rectangle fits; %llu bands tile their rectangles\n", (unsigned long long) asked);
}

int main()
{
	locus_map();
	band_rule();
	printf("ok\n");
	return 0;
}
