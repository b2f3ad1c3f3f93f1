/*
 * tools/eval_contam_check.cpp -- ntsm_amd/csrc/host/eval_contam.hpp on its cases, as a program of its own under the host
 * sanitizers (`make contam_check`).  No GPU, no files.
 *   band rule:  band_rows against a linear scan for small limits, the 1 GiB rule on 4,096, 8,192 and 100,000 samples, and the
 *               bands of a rectangle tiling it;
 *   row text:   a line against one formed here with snprintf("%f") from the same integers -- NA where a depth is 0, where
 *               the target has no informative site and where rateAll is 0, sums past 2^53, a row exactly at excess == X and
 *               one exactly at explained == Y (printed), rows just below (not printed), -a; and the band's lines in order
 *               without the diagonal;
 *   sample text.
 * Prints one line per part and "ok"; any failure prints what failed and exits 1.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/ntsm_eval_hip.h"
#include "../ntsm_amd/csrc/host/eval_contam.hpp"

namespace ct = ntsm::eval_contam;

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static void band_rule()
{
	uint64_t asked = 0;
	for (uint32_t n = 1; n <= 40; ++n)
		for (uint32_t first = 0; first < n; ++first)
			for (uint64_t limit = 0; limit <= (uint64_t) n * n + 1; ++limit, ++asked) {
				uint32_t want = 1;                                              /* the most rows that fit, and at least one */
				while (first + want < n && (uint64_t) (want + 1) * n <= limit) ++want;
				CHECK(ct::band_rows(first, n, limit) == want, "n %u first %u limit %llu: %u, want %u", n, first, (unsigned long long) limit,
				      ct::band_rows(first, n, limit), want);
			}
	CHECK(ct::kBandRecords * sizeof(ntsm_eval_contam_record) == 1ull << 30, "the rule is 1 GiB of records");
	CHECK(sizeof(ntsm_eval_contam_record) == 64, "a record is 64 bytes");
	CHECK(ct::band_rows(0, 4096, ct::kBandRecords) == 4096, "4,096 samples are one band");
	CHECK(ct::band_rows(0, 8192, ct::kBandRecords) == 2048, "8,192 samples are four");
	for (const uint32_t n : { 5794u, 100000u, 4000000000u }) {                  /* the bands tile the rectangle, each within the rule */
		uint64_t bands = 0;
		uint32_t first = 0;
		while (first < n) {
			const uint32_t rows = ct::band_rows(first, n, ct::kBandRecords);
			CHECK(rows >= 1 && rows <= n - first && ((uint64_t) rows * n <= ct::kBandRecords || rows == 1), "n %u first %u rows %u", n, first, rows);
			first += rows;
			if (n == 4000000000u && ++bands == 1000) break;                     /* one row per band, and so on */
		}
		CHECK(n == 4000000000u || first == n, "n %u ends at %u", n, first);
	}
	printf("band rule: %llu questions equal the scan; the 1 GiB bands tile 5,794 and 100,000 samples\n", (unsigned long long) asked);
}

static ntsm_eval_contam_record rec(uint64_t m0, uint64_t m1, uint64_t m2, uint64_t d0, uint64_t d1, uint64_t d2, uint32_t s0 = 1, uint32_t s1 = 2, uint32_t s2 = 3)
{
	ntsm_eval_contam_record r;
	memset(&r, 0, sizeof r);
	r.minor[0] = m0; r.minor[1] = m1; r.minor[2] = m2;
	r.depth[0] = d0; r.depth[1] = d1; r.depth[2] = d2;
	r.sites[0] = s0; r.sites[1] = s1; r.sites[2] = s2;
	return r;
}

static std::string f(bool has, double v)
{
	char buf[512];
	if (!has) return "NA";
	snprintf(buf, sizeof buf, "%f", v);
	return buf;
}

/* the line formed here; *printed as the filter decides */
static std::string want_line(const ntsm_eval_contam_record &r, const uint64_t t[3], double x, double y, bool *printed)
{
	const bool h0 = r.depth[0] != 0, h1 = r.depth[1] != 0, h2 = r.depth[2] != 0, ha = t[2] != 0;
	const double r0 = h0 ? (double) r.minor[0] / (double) r.depth[0] : 0, r1 = h1 ? (double) r.minor[1] / (double) r.depth[1] : 0,
	             r2 = h2 ? (double) r.minor[2] / (double) r.depth[2] : 0, ra = ha ? (double) t[1] / (double) t[2] : 0;
	const bool he = h0 && h2, hx = h0 && ha && ra != 0;
	const double excess = he ? r2 - r0 : 0, explained = hx ? 1 - r0 / ra : 0;
	*printed = he && hx && excess >= x && explained >= y;
	return "target\tsource\t" + std::to_string(r.sites[0]) + "\t" + std::to_string(r.sites[1]) + "\t" + std::to_string(r.sites[2]) + "\t" + f(h0, r0) + "\t"
	       + f(h1, r1) + "\t" + f(h2, r2) + "\t" + f(he, excess) + "\t" + f(hx, explained) + "\n";
}

static void row_text()
{
	const uint64_t big = (1ull << 53) + 1;
	struct Case { ntsm_eval_contam_record r; uint64_t t[3]; int printed; const char *line; };
	const Case cases[] = {
		{ rec(0, 0, 0, 0, 0, 0, 0, 0, 0), { 0, 0, 0 }, 0, "target\tsource\t0\t0\t0\tNA\tNA\tNA\tNA\tNA\n" },
		{ rec(1, 2, 3, 0, 10, 10), { 5, 6, 20 }, 0, "target\tsource\t1\t2\t3\tNA\t0.200000\t0.300000\tNA\tNA\n" },
		{ rec(1, 2, 3, 10, 0, 10), { 5, 6, 20 }, 1, "target\tsource\t1\t2\t3\t0.100000\tNA\t0.300000\t0.200000\t0.666667\n" },
		{ rec(1, 2, 3, 10, 10, 0), { 5, 6, 20 }, 0, "target\tsource\t1\t2\t3\t0.100000\t0.200000\tNA\tNA\t0.666667\n" },
		{ rec(0, 0, 0, 10, 10, 10), { 5, 0, 30 }, 0, "target\tsource\t1\t2\t3\t0.000000\t0.000000\t0.000000\t0.000000\tNA\n" },
		{ rec(1, 2, 3, 10, 10, 10), { 0, 0, 0 }, 0, "target\tsource\t1\t2\t3\t0.100000\t0.200000\t0.300000\t0.200000\tNA\n" },
		{ rec(big, 2 * big, 3 * big, 3 * big, 3 * big, 4 * big + 3), { 7, 1ull << 63, UINT64_MAX }, 0, nullptr },
		{ rec(1, 1, 2, 3, 3, 3), { 9, 4, 9 }, 0, "target\tsource\t1\t2\t3\t0.333333\t0.333333\t0.666667\t0.333333\t0.250000\n" },
		{ rec(0, 5, 1, 100, 100, 100), { 9, 6, 300 }, 1, "target\tsource\t1\t2\t3\t0.000000\t0.050000\t0.010000\t0.010000\t1.000000\n" },   /* excess == X */
		{ rec(0, 5, 1, 100, 100, 101), { 9, 6, 300 }, 0, nullptr },
		{ rec(1, 5, 1, 100, 100, 10), { 9, 2, 100 }, 1, "target\tsource\t1\t2\t3\t0.010000\t0.050000\t0.100000\t0.090000\t0.500000\n" },    /* explained == Y */
		{ rec(1, 5, 1, 100, 100, 10), { 9, 2, 101 }, 0, nullptr },
		{ rec(9, 5, 1, 100, 100, 100), { 9, 15, 300 }, 0, "target\tsource\t1\t2\t3\t0.090000\t0.050000\t0.010000\t-0.080000\t-0.800000\n" },
		{ rec(1, 5, 30, 100, 100, 100), { 9, 36, 300 }, 1, nullptr },
	};
	size_t n = 0;
	for (const Case &c : cases) {
		bool printed = false;
		const std::string want = want_line(c.r, c.t, ct::kMinExcess, ct::kMinExplained, &printed);
		CHECK(printed == (c.printed != 0), "case %zu: the filter here says %d", n, (int) printed);
		CHECK(!c.line || want == c.line, "case %zu: formed %s", n, want.c_str());
		std::string all, kept;
		CHECK(ct::row_line(all, "target", "source", c.r, c.t, true, ct::kMinExcess, ct::kMinExplained), "case %zu: -a prints every row", n);
		CHECK(all == want, "case %zu: %s, want %s", n, all.c_str(), want.c_str());
		CHECK(ct::row_line(kept, "target", "source", c.r, c.t, false, ct::kMinExcess, ct::kMinExplained) == printed, "case %zu: kept or not", n);
		CHECK(kept == (printed ? want : std::string()), "case %zu: %s", n, kept.c_str());
		++n;
	}
	/* a band of two targets (rows 1 and 2) of three samples: the sources in order, the diagonal skipped */
	const char *names[3] = { "a", "b", "c" };
	std::vector<ntsm_eval_contam_record> band(6, cases[13].r);
	const uint64_t tally[6] = { 9, 36, 300, 9, 36, 300 };
	std::string text;
	ct::band_text(text, names, 3, 1, 2, band.data(), tally, false, ct::kMinExcess, ct::kMinExplained);
	const std::string tail = "\t1\t2\t3\t0.010000\t0.050000\t0.300000\t0.290000\t0.916667\n";
	CHECK(text == "b\ta" + tail + "b\tc" + tail + "c\ta" + tail + "c\tb" + tail, "%s", text.c_str());
	text.clear();
	ct::band_text(text, names, 3, 0, 0, band.data(), tally, true, 0, 0);
	CHECK(text.empty(), "no rows, no text");
	printf("row text: %zu cases equal the lines formed from their integers, kept or dropped as the cut says\n", n);
}

static void sample_text()
{
	std::string text = ct::kSampleHeader;
	const uint64_t t[3][3] = { { 0, 0, 0 }, { 9, 4, 9 }, { 7, 1ull << 63, UINT64_MAX } };
	const char *names[3] = { "cohort/a.txt", "b", "c" };
	for (int i = 0; i < 3; ++i) ct::sample_line(text, names[i], t[i]);
	CHECK(text == "#sample\tsites\tminorReads\tdepth\trateAll\ncohort/a.txt\t0\t0\t0\tNA\nb\t9\t4\t9\t0.444444\nc\t7\t9223372036854775808\t18446744073709551615\t0.500000\n",
	      "%s", text.c_str());
	printf("sample text: three lines\n");
}

int main()
{
	band_rule();
	row_text();
	sample_text();
	printf("ok\n");
	return 0;
}
