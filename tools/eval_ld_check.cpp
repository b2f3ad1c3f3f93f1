/*
 * tools/eval_ld_check.cpp -- ntsm_amd/csrc/host/eval_ld.hpp on its cases, as a program of its own under the host sanitizers
 * (`make ld_check`).  No GPU, no files: where the header asks the device, a model over dosages answers.
 *   moments:    the moments and r^2 of records formed here from dosage lists against a floating-point-free restatement: n == M
 *               (defined) and M - 1 (not), vx == 0, identical sites (r2 exactly 1.0), an inverse (cov < 0), counts at 2^24;
 *   bands:      the walk against a scan over every small row-count vector and budget: the capacity is the budget, never below
 *               n_sites; a call beyond it is halved and run again, down to one row; the bands partition the rows in order;
 *   row text:   lines against ones formed here with snprintf("%f");
 *   prune:      chains (a-b and b-c selected, a-c not: a and c kept), a site dropped only by a kept site, nothing above r2 = 1;
 *   run:        a cohort of 40 samples x 24 sites in blocks through walk, rows_text and Prune at three budgets -- the same text
 *               and the same kept sites -- with the model's select sorted as the library's is.
 * Prints one line per part and "ok"; any failure prints what failed and exits 1.
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/ntsm_eval_hip.h"
#include "../ntsm_amd/csrc/host/eval_ld.hpp"

namespace ld = ntsm::eval_ld;

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

/* the record of two sites from their dosages, -1 = not called */
static ntsm_eval_ld_record record_of(const std::vector<int> &x, const std::vector<int> &y)
{
	ntsm_eval_ld_record r {};
	for (size_t i = 0; i < x.size(); ++i) {
		const int u = x[i], v = y[i];
		r.n += u >= 0 && v >= 0;
		r.hs += u == 1 && v >= 0; r.gs += u == 2 && v >= 0;
		r.ht += u >= 0 && v == 1; r.gt += u >= 0 && v == 2;
		r.hh += u == 1 && v == 1; r.hg += (u == 1 && v == 2) || (u == 2 && v == 1); r.gg += u == 2 && v == 2;
	}
	return r;
}

/* the moments straight from the dosages, over the samples called at both */
static ld::Moments moments_from(const std::vector<int> &x, const std::vector<int> &y)
{
	int64_t n = 0, sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
	for (size_t i = 0; i < x.size(); ++i) {
		if (x[i] < 0 || y[i] < 0) continue;
		++n; sx += x[i]; sy += y[i]; sxx += x[i] * x[i]; syy += y[i] * y[i]; sxy += x[i] * y[i];
	}
	return ld::Moments { n, n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy };
}

static std::vector<int> cycle(const std::vector<int> &v, size_t n) { std::vector<int> out(n); for (size_t i = 0; i < n; ++i) out[i] = v[i % v.size()]; return out; }

static void moments_and_r2()
{
	const std::vector<int> x = cycle({ 0, 1, 2, 1, 0, 2, 1, 1, 0, 2 }, 20), some = cycle({ 0, 1, 2, 2, 0, 1, 1, 0, 0, 2 }, 20), flat(20, 1);
	std::vector<int> flip(20), gaps = x;
	for (size_t i = 0; i < 20; ++i) flip[i] = 2 - x[i];
	gaps[0] = -1; gaps[7] = -1;
	const std::vector<int> *sites[] = { &x, &some, &flat, &flip, &gaps };
	for (const std::vector<int> *a : sites)
		for (const std::vector<int> *b : sites) {
			const ld::Moments got = ld::moments_of(record_of(*a, *b)), want = moments_from(*a, *b);
			CHECK(got.n == want.n && got.cov == want.cov && got.vx == want.vx && got.vy == want.vy, "moments differ");
			CHECK(got.vx >= 0 && got.vy >= 0, "a variance below 0");
			if (ld::r2_defined(got, 0)) CHECK(ld::r2_of(got) >= 0.0 && ld::r2_of(got) <= 1.0, "r2 %f", ld::r2_of(got));
		}
	const ld::Moments same = ld::moments_of(record_of(x, x)), inverse = ld::moments_of(record_of(x, flip));
	CHECK(same.n == 20 && ld::r2_defined(same, 20) && !ld::r2_defined(same, 21) && ld::r2_of(same) == 1.0, "identical sites");
	CHECK(inverse.cov < 0 && ld::r2_of(inverse) == 1.0, "the inverse");
	CHECK(!ld::r2_defined(ld::moments_of(record_of(flat, x)), 0) && !ld::r2_defined(ld::moments_of(record_of(x, flat)), 0), "vx == 0, vy == 0");
	CHECK(ld::selected(record_of(x, x), 20, 1.0) && !ld::selected(record_of(x, x), 20, std::nextafter(1.0, 2.0)), "T at and above 1.0");
	const double own = ld::r2_of(ld::moments_of(record_of(x, some)));
	CHECK(own > 0 && own < 1 && ld::selected(record_of(x, some), 20, own) && !ld::selected(record_of(x, some), 20, std::nextafter(own, 2.0)), "T at and above a pair's own r2");
	/* 2^24 samples, half het and half homCG at one site, all het at the other side's complement: the products stay in int64 */
	const uint32_t big = 1u << 24;
	const ntsm_eval_ld_record r { big, big / 2, big / 2, big / 2, big / 2, big / 2, 0, big / 2 };
	const ld::Moments m = ld::moments_of(r);
	CHECK(m.vx == (int64_t) big * (big / 2 + 2 * (int64_t) big) - (int64_t) (big / 2 + big) * (big / 2 + big) && m.vx > 0 && m.cov == m.vx && ld::r2_of(m) == 1.0, "2^24 samples");
	printf("moments: 25 pairs of sites against the dosages, the edges of M, vx == 0, r2 == 1.0 both ways, T at a pair's own r2, 2^24 samples\n");
}

/* a device that selects row_pairs[a] pairs in row a; it records its calls */
struct Call { uint32_t first, rows; int rc; };
static ld::Device counting_device(const std::vector<uint64_t> &row_pairs, std::vector<Call> &calls)
{
	ld::Device dev;
	dev.select = [&](uint32_t first, uint32_t rows, uint64_t cap, ntsm_eval_ld_pair *, uint64_t *found) {
		*found = 0;
		for (uint32_t r = 0; r < rows; ++r) *found += row_pairs[first + r];
		calls.push_back(Call { first, rows, *found > cap });
		return (int) (*found > cap);
	};
	return dev;
}

static void bands()
{
	uint64_t walks = 0, reruns = 0;
	for (uint32_t n = 1; n <= 7; ++n) {
		std::vector<uint64_t> rp(n);
		/* every vector with 0 ... min(2, n - 1 - a) pairs in row a, by counting in base 3 */
		uint64_t combos = 1;
		for (uint32_t a = 0; a < n; ++a) combos *= 3;
		for (uint64_t code = 0; code < combos; ++code) {
			uint64_t c = code, total = 0;
			for (uint32_t a = 0; a < n; ++a, c /= 3) { rp[a] = std::min<uint64_t>(c % 3, n - 1 - a); total += rp[a]; }
			for (uint64_t budget = 0; budget <= total + 1; ++budget, ++walks) {
				std::vector<Call> calls;
				ld::Stats st;
				uint64_t handed = 0;
				const int rc = ld::walk(counting_device(rp, calls), n, budget, [&](const ntsm_eval_ld_pair *, uint64_t count) { handed += count; }, st);
				CHECK(rc == 0 && handed == total && st.pairs == total, "n %u budget %llu: %d", n, (unsigned long long) budget, rc);
				/* the scan */
				const uint64_t cap = std::max<uint64_t>(budget, n);
				uint32_t first = 0, rows = n;
				size_t at = 0;
				uint64_t done = 0, again = 0;
				while (first < n) {
					rows = std::min(rows, n - first);
					uint64_t found = 0;
					for (uint32_t r = 0; r < rows; ++r) found += rp[first + r];
					CHECK(at < calls.size() && calls[at].first == first && calls[at].rows == rows && calls[at].rc == (found > cap), "call %zu", at);
					++at;
					if (found > cap) { CHECK(rows > 1, "one row beyond the capacity"); rows /= 2; ++again; } else { first += rows; ++done; }
				}
				CHECK(at == calls.size() && st.bands == done && st.reruns == again, "calls");
				reruns += again;
			}
		}
	}
	CHECK(ld::pair_cap(96287, ld::kPairBudget) == (1ull << 30) / 40 && ld::pair_cap(96287, 1) == 96287 && ld::halved(1) == 1 && ld::halved(7) == 3, "constants");
	/* a device that fails ends the walk with its code */
	ld::Device broken;
	broken.select = [](uint32_t, uint32_t, uint64_t, ntsm_eval_ld_pair *, uint64_t *) { return -2; };
	ld::Stats st;
	CHECK(ld::walk(broken, 5, 10, [](const ntsm_eval_ld_pair *, uint64_t) {}, st) == -2 && st.bands == 0, "a failing device");
	printf("bands: %llu walks against the scan, %llu re-runs among them, the capacity never below n_sites\n", (unsigned long long) walks, (unsigned long long) reruns);
}

static std::string expect_line(const char *a, const char *b, const ntsm_eval_ld_record &r)
{
	const ld::Moments m = ld::moments_of(r);
	char buf[256];
	snprintf(buf, sizeof buf, "%s\t%s\t%u\t%f\t%s\n", a, b, r.n, ((double) m.cov * (double) m.cov) / ((double) m.vx * (double) m.vy), m.cov > 0 ? "+" : "-");
	return buf;
}

static void row_text()
{
	const std::vector<int> x = cycle({ 0, 1, 2, 1, 0, 2, 1, 1, 0, 2 }, 20), some = cycle({ 0, 1, 2, 2, 0, 1, 1, 0, 0, 2 }, 20), third = cycle({ 0, 0, 1 }, 20);
	std::vector<int> flip(20);
	for (size_t i = 0; i < 20; ++i) flip[i] = 2 - x[i];
	const char *locus[] = { "rs1", "rs4", "chr2:77", "x" };
	const ntsm_eval_ld_pair pairs[] = { { 0, 1, record_of(x, x) }, { 0, 2, record_of(x, flip) }, { 1, 3, record_of(x, some) }, { 2, 3, record_of(x, third) } };
	std::string got, want;
	ld::rows_text(got, locus, pairs, 4);
	for (const ntsm_eval_ld_pair &p : pairs) want += expect_line(locus[p.a], locus[p.b], p.rec);
	CHECK(got == want, "%s", got.c_str());
	CHECK(got.rfind("rs1\trs4\t20\t1.000000\t+\nrs1\tchr2:77\t20\t1.000000\t-\n", 0) == 0, "%s", got.c_str());
	std::string none;
	ld::rows_text(none, locus, pairs, 0);
	CHECK(none.empty() && std::string(ld::kHeader) == "siteA\tsiteB\tn\tr2\tdir\n", "no pair, no line");
	printf("row text: 4 lines against snprintf, r2 == 1.0 of either dir, digits that round\n");
}

static void prune_rule()
{
	const std::vector<int> x = cycle({ 0, 1, 2, 1, 0, 2, 1, 1, 0, 2 }, 20), some = cycle({ 0, 1, 2, 2, 0, 1, 1, 0, 0, 2 }, 20);
	const ntsm_eval_ld_record one = record_of(x, x), part = record_of(x, some);
	const double own = ld::r2_of(ld::moments_of(part));
	const ntsm_eval_ld_pair chain[] = { { 0, 1, part }, { 1, 2, part } };
	ld::Prune a(3);
	a.add(chain, 2, 20, own);
	CHECK(a.kept == std::vector<uint8_t>({ 1, 0, 1 }) && a.n_kept() == 2, "a-b, b-c: a and c stay");
	ld::Prune b(3);
	b.add(chain, 2, 20, std::nextafter(own, 2.0));
	CHECK(b.n_kept() == 3, "just above the pairs' r2");
	ld::Prune c(3);
	c.add(chain, 2, 21, own);
	CHECK(c.n_kept() == 3, "n below M");
	const ntsm_eval_ld_pair fan[] = { { 0, 1, one }, { 0, 2, one }, { 1, 3, one }, { 2, 3, one }, { 3, 4, one } };
	ld::Prune d(6);
	d.add(fan, 2, 20, 0.5);                                                       /* in two parts, as bands hand them over */
	d.add(fan + 2, 3, 20, 0.5);
	CHECK(d.kept == std::vector<uint8_t>({ 1, 0, 0, 1, 0, 1 }), "a site that pairs only with dropped sites stays, and drops the next");
	ld::Prune e(6);
	e.add(fan, 5, 20, std::nextafter(1.0, 2.0));
	CHECK(e.n_kept() == 6, "nothing is selected above 1.0");
	const char *locus[] = { "a", "b", "c", "d", "e", "f" };
	CHECK(d.text(locus) == "a\nd\nf\n" && ld::Prune(0).text(locus).empty(), "the kept IDs");
	printf("prune: chains, a site dropped only by a kept site, the cuts at a pair's own r2 and at M, the text\n");
}

static void whole_run()
{
	/* 40 samples x 24 sites: blocks of a base site, its copy, a copy with every fifth sample redrawn and its inverse; 1 in 17 cells missing */
	const uint32_t n = 40, m = 24;
	std::vector<std::vector<int>> site(m, std::vector<int>(n));
	uint32_t state = 12345;
	auto next = [&] { state = state * 1664525u + 1013904223u; return state >> 16; };
	for (uint32_t s = 0; s < m; s += 4)
		for (uint32_t i = 0; i < n; ++i) {
			const int g = (int) (next() % 3);
			site[s][i] = g; site[s + 1][i] = g; site[s + 2][i] = i % 5 == 0 ? (int) (next() % 3) : g; site[s + 3][i] = 2 - g;
		}
	for (uint32_t s = 0; s < m; ++s)
		for (uint32_t i = 0; i < n; ++i)
			if (next() % 17 == 0) site[s][i] = -1;
	std::vector<std::string> ids(m);
	std::vector<const char *> locus(m);
	for (uint32_t s = 0; s < m; ++s) { ids[s] = "site" + std::to_string(s); locus[s] = ids[s].c_str(); }
	const uint32_t min_called = 20;
	const double cut = 0.5;
	/* the device: the band's selected pairs, appended column by column (not in (a, b) order) and then sorted as the library sorts */
	ld::Device dev;
	dev.select = [&](uint32_t first, uint32_t rows, uint64_t cap, ntsm_eval_ld_pair *out, uint64_t *found) {
		std::vector<ntsm_eval_ld_pair> got;
		for (uint32_t b = m; b-- > 0;)
			for (uint32_t a = first; a < first + rows && a < b; ++a) {
				const ntsm_eval_ld_record r = record_of(site[a], site[b]);
				if (ld::selected(r, min_called, cut)) got.push_back(ntsm_eval_ld_pair { a, b, r });
			}
		*found = got.size();
		if (got.size() > cap) return 1;
		std::sort(got.begin(), got.end(), [](const ntsm_eval_ld_pair &x, const ntsm_eval_ld_pair &y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
		std::copy(got.begin(), got.end(), out);
		return 0;
	};
	std::string first_text, first_kept;
	uint64_t pairs = 0;
	for (const uint64_t budget : { ld::kPairBudget / 1024, (uint64_t) 26, (uint64_t) 0 }) {   /* 26 and n_sites = 24 pairs a call: below what there is */
		std::string text = ld::kHeader;
		ld::Prune prune(m);
		ld::Stats st;
		const int rc = ld::walk(dev, m, budget, [&](const ntsm_eval_ld_pair *p, uint64_t count) { ld::rows_text(text, locus.data(), p, count); prune.add(p, count, min_called, cut); }, st);
		CHECK(rc == 0, "walk %d", rc);
		if (first_text.empty()) { first_text = text; first_kept = prune.text(locus.data()); pairs = st.pairs; CHECK(st.bands == 1 && st.reruns == 0, "one band"); }
		else CHECK(st.reruns > 0 && st.bands > 1, "budget %llu: no halving", (unsigned long long) budget);
		CHECK(text == first_text && prune.text(locus.data()) == first_kept && st.pairs == pairs, "budget %llu changes the output", (unsigned long long) budget);
	}
	/* brute force: the pairs in (a, b) order and the prune site by site */
	std::string want = ld::kHeader;
	std::vector<uint8_t> kept(m, 1);
	uint64_t count = 0;
	for (uint32_t a = 0; a < m; ++a)
		for (uint32_t b = a + 1; b < m; ++b) {
			const ntsm_eval_ld_record r = record_of(site[a], site[b]);
			if (!ld::selected(r, min_called, cut)) continue;
			want += expect_line(locus[a], locus[b], r);
			++count;
		}
	for (uint32_t t = 0; t < m; ++t)
		for (uint32_t s = 0; s < t; ++s)
			if (kept[s] && ld::selected(record_of(site[s], site[t]), min_called, cut)) { kept[t] = 0; break; }
	std::string want_kept;
	for (uint32_t s = 0; s < m; ++s) if (kept[s]) want_kept += ids[s] + "\n";
	CHECK(first_text == want && first_kept == want_kept && count == pairs && count >= 12, "%llu pairs", (unsigned long long) count);
	CHECK(want.find("\t-\n") != std::string::npos && want.find("\t+\n") != std::string::npos, "both dirs");
	printf("run: %llu pairs of 24 sites, the same text and kept sites at three budgets and by brute force\n", (unsigned long long) count);
}

int main()
{
	moments_and_r2();
	bands();
	row_text();
	prune_rule();
	whole_run();
	printf("ok\n");
	return 0;
}
