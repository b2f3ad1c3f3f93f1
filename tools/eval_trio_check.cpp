/*
 * tools/eval_trio_check.cpp -- ntsm_amd/csrc/host/eval_trio.hpp on its cases, as a program of its own under the host sanitizers
 * (`make trio_check`).  No GPU, no files: where the header asks the device, a model over genotype classes answers.
 *   candidates:   the rule on a row with every edge (the child itself, called below and at M, the rate at and above Y, called 0);
 *   batches:      cut_batches against a scan for small limits, a list that alone exceeds the limit, the 1 GiB constants;
 *   pedigree:     tabs and spaces, a comment, a 0 parent, an empty line, a last line without newline, a short line;
 *   names:        each of the three levels, an ambiguous basename, an unknown ID, somebody their own parent;
 *   row text:     lines against ones formed here with snprintf("%f") -- called == 0, a row exactly at rate == X and one exactly
 *                 at called == M (printed), rows just outside (not printed), -a, each of the three verdicts;
 *   runs:         a family of six (two founders' two children, an unrelated pair) through search by candidates and exhaustively
 *                 -- the same rows -- in one batch and in batches of one list, and through pedigree.
 * Prints one line per part and "ok"; any failure prints what failed and exits 1.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/ntsm_eval_hip.h"
#include "../ntsm_amd/csrc/host/eval_trio.hpp"

namespace tr = ntsm::eval_trio;

#define CHECK(cond, ...) do { if (!(cond)) { printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

static ntsm_eval_trio_duo duo(uint32_t called, uint32_t opp) { ntsm_eval_trio_duo d; d.called = called; d.opp = opp; return d; }
static ntsm_eval_trio_record rec(uint32_t called, uint32_t eh, uint32_t et) { ntsm_eval_trio_record r; r.called = called; r.err_hom = eh; r.err_het = et; r.pad = 0; return r; }

static void candidate_rule()
{
	/* child 2; M = 200, Y = 0.02 */
	const ntsm_eval_trio_duo row[] = { duo(200, 4), duo(199, 0), duo(5000, 0), duo(200, 5), duo(0, 0), duo(1000, 20), duo(1000, 21), duo(4000000000u, 80000000u) };
	std::vector<uint32_t> got;
	CHECK(tr::candidates(row, 8, 2, 200, 0.02, got) == 3 && got == std::vector<uint32_t>({ 0, 5, 7 }), "%zu candidates", got.size());
	got.clear();
	CHECK(tr::candidates(row, 8, 2, 0, 1.0, got) == 6 && got == std::vector<uint32_t>({ 0, 1, 3, 5, 6, 7 }), "M = 0: called == 0 is still none");
	got.clear();
	CHECK(tr::candidates(row, 0, 0, 0, 1.0, got) == 0 && got.empty(), "no row, no candidate");
	printf("candidates: the child, called at and below M, the rate at and above Y, called == 0\n");
}

static void batches()
{
	uint64_t asked = 0;
	const uint32_t k[] = { 3, 0, 2, 5, 1, 4, 4, 2 };                                /* 3, 0, 1, 10, 0, 6, 6, 1 records */
	for (size_t n = 0; n <= 8; ++n)
		for (uint64_t limit = 0; limit <= 30; ++limit, ++asked) {
			std::vector<size_t> ends, want;
			size_t bad = n;
			uint64_t held = 0;
			for (size_t i = 0; i < n && bad == n; ++i) {                            /* the scan: greedy, in order */
				const uint64_t t = (uint64_t) k[i] * (k[i] ? k[i] - 1 : 0) / 2;
				if (t > limit) { bad = i; break; }
				if (held + t > limit) { want.push_back(i); held = 0; }
				held += t;
			}
			const size_t got = tr::cut_batches(k, n, limit, ends);
			CHECK(got == bad, "n %zu limit %llu: %zu, want %zu", n, (unsigned long long) limit, got, bad);
			if (bad != n) continue;
			if (n) want.push_back(n);
			CHECK(ends == want, "n %zu limit %llu: %zu batches, want %zu", n, (unsigned long long) limit, ends.size(), want.size());
			size_t begin = 0;
			for (const size_t end : ends) {                                         /* every batch within the limit, none empty */
				uint64_t sum = 0;
				for (size_t i = begin; i < end; ++i) sum += tr::triples_of(k[i]);
				CHECK(end > begin && sum <= limit, "batch [%zu, %zu) holds %llu", begin, end, (unsigned long long) sum);
				begin = end;
			}
		}
	CHECK(sizeof(ntsm_eval_trio_duo) == 8 && sizeof(ntsm_eval_trio_record) == 16, "the records are 8 and 16 bytes");
	CHECK(tr::kDuoBandRecords * 8 == 1ull << 30 && tr::kBatchRecords * 16 == 1ull << 30, "both limits are 1 GiB of records");
	const uint32_t longList[] = { 4, 11586, 4 };                                    /* 11,586 * 11,585 / 2 > 2^26 */
	std::vector<size_t> ends;
	CHECK(tr::cut_batches(longList, 3, tr::kBatchRecords, ends) == 1, "a list of 11,586 exceeds one batch");
	const uint32_t fits[] = { 11585, 11585 };
	ends.clear();
	CHECK(tr::cut_batches(fits, 2, tr::kBatchRecords, ends) == 2 && ends == std::vector<size_t>({ 1, 2 }), "two lists of 11,585 are two batches");
	CHECK(tr::band_rows(0, 4096, tr::kDuoBandRecords) == 4096 && tr::band_rows(0, 16384, tr::kDuoBandRecords) == 8192 && tr::band_rows(5, 10, 0) == 1, "the band rule");
	printf("batches: %llu questions equal the scan\n", (unsigned long long) asked);
}

static void pedigree_text()
{
	const std::string text = "# family\tone\nF1 kid dad mum 1 0\nF1\tdad\t0\t0\t1\t0\n\n  F1  mum 0 gran 2 0 \r\nF2 kid2 dad mum\n#last\nF2 kid3 mum dad 0 0";
	const tr::Ped ped = tr::parse_ped(text);
	CHECK(ped.comments == 2 && ped.founders == 2 && ped.trios.size() == 3, "%llu comments, %llu founders, %zu trios", (unsigned long long) ped.comments,
	      (unsigned long long) ped.founders, ped.trios.size());
	CHECK(ped.trios[0].id == "kid" && ped.trios[0].father == "dad" && ped.trios[0].mother == "mum", "the first trio");
	CHECK(ped.trios[1].id == "kid2" && ped.trios[2].id == "kid3" && ped.trios[2].father == "mum" && ped.trios[2].mother == "dad", "file order, columns 3 and 4");
	CHECK(tr::parse_ped("").trios.empty() && tr::parse_ped("\n\n").trios.empty(), "an empty file has no trio");
	bool threw = false;
	try { tr::parse_ped("F1 kid dad mum\nF1 kid dad\n"); } catch (const tr::Error &e) { threw = strstr(e.what(), "line 2") != nullptr; }
	CHECK(threw, "a line of three columns is refused by its number");
	printf("pedigree: tabs and spaces, comments, 0 parents, an empty line, no last newline, a short line\n");
}

static void name_matching()
{
	const std::vector<std::string> names = { "cohort/a.txt", "cohort/b_counts.txt", "other/b_counts.txt", "c.counts.txt", "d", "x/e.txt", "y/e.txt.txt", "b" };
	CHECK(tr::match_name(names, "cohort/a.txt") == 0 && tr::match_name(names, "d") == 4, "the stored name");
	CHECK(tr::match_name(names, "a.txt") == 0 && tr::match_name(names, "c.counts.txt") == 3, "the basename");
	CHECK(tr::match_name(names, "a") == 0 && tr::match_name(names, "c") == 3 && tr::match_name(names, "e") == 5, "the stem");
	CHECK(tr::match_name(names, "e.txt") == 5, "e.txt is a basename before it is y/e.txt.txt's stem: one suffix is removed, once");
	CHECK(tr::match_name(names, "b_counts.txt") == tr::kAmbiguous, "an ambiguous basename");
	CHECK(tr::match_name(names, "b") == 7, "the stored name b comes before the two stems b");
	CHECK(tr::match_name(names, "nobody") == tr::kUnknown && tr::match_name(names, "") == tr::kUnknown && tr::match_name({}, "a") == tr::kUnknown, "unknown IDs");
	for (const char *id : { "nobody", "b_counts.txt" }) {
		bool named = false;
		try { tr::sample_of(names, id); } catch (const tr::Error &e) { named = strstr(e.what(), id) != nullptr; }
		CHECK(named, "the refusal names %s", id);
	}
	tr::Ped ped;
	ped.trios.push_back(tr::PedLine { "a", "d", "c" });
	const std::vector<tr::PedTrio> t = tr::resolve(ped, names);
	CHECK(t.size() == 1 && t[0].child == 0 && t[0].father == 4 && t[0].mother == 3, "resolved");
	ped.trios.push_back(tr::PedLine { "a", "a.txt", "c" });
	bool own = false;
	try { tr::resolve(ped, names); } catch (const tr::Error &e) { own = strstr(e.what(), "its own parent") != nullptr; }
	CHECK(own, "nobody is their own parent");
	printf("names: three levels, ambiguous, unknown, own parent\n");
}

static std::string want_line(const ntsm_eval_trio_record &r, const ntsm_eval_trio_duo &a, const ntsm_eval_trio_duo &b, const char *verdict)
{
	char buf[1024], rate[64];
	if (r.called) snprintf(rate, sizeof rate, "%f", (double) ((uint64_t) r.err_hom + r.err_het) / (double) r.called);
	else snprintf(rate, sizeof rate, "NA");
	snprintf(buf, sizeof buf, "kid\tdad\tmum\t%u\t%u\t%u\t%s\t%u\t%u\t%u\t%u%s%s\n", r.called, r.err_hom, r.err_het, rate, a.called, a.opp, b.called, b.opp,
	         verdict ? "\t" : "", verdict ? verdict : "");
	return buf;
}

static void row_text()
{
	struct Case { ntsm_eval_trio_record r; int printed; const char *verdict; const char *line; };
	const Case cases[] = {                                                          /* M = 200, X = 0.02 */
		{ rec(0, 0, 0), 0, "lowcov", "kid\tdad\tmum\t0\t0\t0\tNA\t7\t1\t9\t2\n" },
		{ rec(2000, 0, 0), 1, "ok", "kid\tdad\tmum\t2000\t0\t0\t0.000000\t7\t1\t9\t2\n" },
		{ rec(200, 3, 1), 1, "ok", "kid\tdad\tmum\t200\t3\t1\t0.020000\t7\t1\t9\t2\n" },    /* exactly at called == M and at rate == X */
		{ rec(199, 0, 0), 0, "lowcov", nullptr },                                   /* just below M */
		{ rec(250, 3, 2), 1, "ok", nullptr },                                       /* 5 / 250: the double 0.02 */
		{ rec(249, 3, 2), 0, "fail", nullptr },                                     /* just above X */
		{ rec(3, 1, 0), 0, "lowcov", "kid\tdad\tmum\t3\t1\t0\t0.333333\t7\t1\t9\t2\n" },
		{ rec(4000000000u, 4000000000u, 4000000000u), 0, "fail", "kid\tdad\tmum\t4000000000\t4000000000\t4000000000\t2.000000\t7\t1\t9\t2\n" },   /* the sum is taken in 64 bits */
	};
	const char *names[3] = { "kid", "dad", "mum" };
	const uint32_t c = 0, a = 1, b = 2;
	const ntsm_eval_trio_duo da = duo(7, 1), db = duo(9, 2);
	size_t n = 0;
	for (const Case &k : cases) {
		const std::string want = want_line(k.r, da, db, nullptr);
		CHECK(!k.line || want == k.line, "case %zu: formed %s", n, want.c_str());
		std::string all, kept, ped;
		tr::rows_text(all, names, 1, &c, &a, &b, &k.r, &da, &db, false, true, 200, 0.02);
		tr::rows_text(kept, names, 1, &c, &a, &b, &k.r, &da, &db, false, false, 200, 0.02);
		tr::rows_text(ped, names, 1, &c, &a, &b, &k.r, &da, &db, true, false, 200, 0.02);
		CHECK(all == want, "case %zu: %s, want %s", n, all.c_str(), want.c_str());
		CHECK(kept == (k.printed ? want : std::string()), "case %zu: kept %s", n, kept.c_str());
		CHECK(ped == want_line(k.r, da, db, k.verdict), "case %zu: %s", n, ped.c_str());
		++n;
	}
	CHECK(std::string(tr::verdict_of(rec(0, 0, 0), 0, 1.0)) == "fail", "no site and no least: there is no rate to pass");
	CHECK(tr::header_line(false) == "child\tparentA\tparentB\tcalled\terrHom\terrHet\trate\tcalledA\toppA\tcalledB\toppB\n" &&
	      tr::header_line(true) == "child\tparentA\tparentB\tcalled\terrHom\terrHet\trate\tcalledA\toppA\tcalledB\toppB\tverdict\n", "the headers");
	printf("row text: %zu cases equal the lines formed from their integers, kept or dropped as the cuts say, each verdict\n", n);
}

/* a model of the device over genotype classes [sample][site]: 0 homAT, 1 het, 2 homCG, 3 miss */
struct Model {
	std::vector<std::vector<int>> cls;
	uint64_t duo_calls = 0, score_calls = 0;
	ntsm_eval_trio_duo duo_of(uint32_t x, uint32_t y) const
	{
		ntsm_eval_trio_duo d = duo(0, 0);
		for (size_t s = 0; s < cls[x].size(); ++s) {
			const int a = cls[x][s], b = cls[y][s];
			if (a == 3 || b == 3) continue;
			d.called++;
			d.opp += (a == 0 && b == 2) || (a == 2 && b == 0);
		}
		return d;
	}
	ntsm_eval_trio_record trio_of(uint32_t k, uint32_t x, uint32_t y) const
	{
		ntsm_eval_trio_record r = rec(0, 0, 0);
		for (size_t s = 0; s < cls[k].size(); ++s) {
			const int c = cls[k][s], a = cls[x][s], b = cls[y][s];
			if (c == 3 || a == 3 || b == 3) continue;
			r.called++;
			r.err_hom += (c == 0 && (a == 2 || b == 2)) || (c == 2 && (a == 0 || b == 0));
			r.err_het += c == 1 && ((a == 0 && b == 0) || (a == 2 && b == 2));
		}
		return r;
	}
	tr::Device device()
	{
		tr::Device d;
		d.duos = [this](uint32_t first, uint32_t rows, ntsm_eval_trio_duo *out) {
			++duo_calls;
			for (uint32_t r = 0; r < rows; ++r)
				for (uint32_t y = 0; y < cls.size(); ++y) out[(size_t) r * cls.size() + y] = duo_of(first + r, y);
			return 0;
		};
		d.score = [this](const uint32_t *child, const uint64_t *offset, const uint32_t *cand, uint32_t n, ntsm_eval_trio_record *out) {
			++score_calls;
			for (uint32_t i = 0; i < n; ++i)
				for (uint64_t p = offset[i]; p < offset[i + 1]; ++p)
					for (uint64_t q = p + 1; q < offset[i + 1]; ++q) *out++ = trio_of(child[i], cand[p], cand[q]);
			return 0;
		};
		return d;
	}
};

static void runs()
{
	/* 0, 1: founders; 2, 3: their children; 4, 5: unrelated.  400 sites; sample 5 misses every second site. */
	Model m;
	m.cls.assign(6, std::vector<int>(400));
	uint32_t x = 12345;
	auto bit = [&]() { x = x * 1664525u + 1013904223u; return (x >> 16) & 1; };
	std::vector<std::vector<int>> hap(12, std::vector<int>(400));
	for (int s = 0; s < 400; ++s) {
		for (int f : { 0, 1, 4, 5 }) { hap[2 * f][s] = bit(); hap[2 * f + 1][s] = bit(); }
		for (int c : { 2, 3 }) { hap[2 * c][s] = hap[0 + bit()][s]; hap[2 * c + 1][s] = hap[2 + bit()][s]; }
		for (int i = 0; i < 6; ++i) m.cls[i][s] = hap[2 * i][s] + hap[2 * i + 1][s] == 2 ? 0 : hap[2 * i][s] + hap[2 * i + 1][s] == 1 ? 1 : 2;
		if (s % 2) m.cls[5][s] = 3;
	}
	const std::vector<std::string> names = { "f/dad.txt", "f/mum.txt", "f/kid1.txt", "f/kid2.txt", "g/u1.txt", "g/u2.txt" };
	const tr::Device dev = m.device();
	std::string text[4];
	tr::Stats st[4];
	int i = 0;
	for (const bool exhaustive : { false, true })
		for (const uint64_t batch : { tr::kBatchRecords, (uint64_t) 10 }) {
			tr::Cuts cuts;
			cuts.exhaustive = exhaustive;
			cuts.batch_limit = batch;
			cuts.band_limit = exhaustive ? 6 : 13;                                  /* bands of two rows; exhaustive: one row per fetch */
			CHECK(tr::search(dev, names, cuts, [&](const std::string &t) { text[i] += t; }, st[i]) == 0, "the search ends well");
			++i;
		}
	const ntsm_eval_trio_record r2 = m.trio_of(2, 0, 1), r3 = m.trio_of(3, 0, 1);
	CHECK(r2.called == 400 && r2.err_hom == 0 && r2.err_het == 0 && r3.called == 400 && r3.err_hom + r3.err_het == 0, "the true trios have no error");
	std::string want = tr::header_line(false);
	tr::row_line(want, "f/kid1.txt", "f/dad.txt", "f/mum.txt", r2, m.duo_of(2, 0), m.duo_of(2, 1), nullptr);
	tr::row_line(want, "f/kid2.txt", "f/dad.txt", "f/mum.txt", r3, m.duo_of(3, 0), m.duo_of(3, 1), nullptr);
	for (int j = 0; j < 4; ++j) CHECK(text[j] == want, "run %d prints\n%swant\n%s", j, text[j].c_str(), want.c_str());
	CHECK(st[0].bands == 3 && st[0].rows == 2 && st[1].triples == st[0].triples && st[0].triples < 60, "by candidates: %llu bands, %llu triples",
	      (unsigned long long) st[0].bands, (unsigned long long) st[0].triples);
	CHECK(st[2].children == 6 && st[2].triples == 60 && st[3].triples == 60 && st[2].bands == 2, "exhaustively: 6 x 10 triples, the two children's rows fetched");
	{                                                                               /* -a: every evaluated triple, parentA < parentB inside a child */
		tr::Cuts cuts;
		cuts.all = cuts.exhaustive = true;
		std::string all;
		tr::Stats s;
		CHECK(tr::search(dev, names, cuts, [&](const std::string &t) { all += t; }, s) == 0 && s.rows == 60, "-a prints the 60");
		CHECK(all.find("f/dad.txt\tf/mum.txt\tf/kid1.txt\t") < all.find("f/dad.txt\tf/mum.txt\tf/kid2.txt\t") && all.find("f/dad.txt\tf/mum.txt\tf/kid2.txt\t") < all.find("f/dad.txt\tf/kid1.txt\tf/kid2.txt\t"),
		      "store order");
		cuts.batch_limit = 9;                                                       /* a list of 5 has 10 records */
		bool refused = false;
		try { tr::search(dev, names, cuts, [&](const std::string &) {}, s); } catch (const tr::Error &e) { refused = strstr(e.what(), "without --trio-exhaustive") && strstr(e.what(), "f/dad.txt"); }
		CHECK(refused, "an exhaustive list that no batch takes is refused, naming --trio-exhaustive");
		cuts.exhaustive = false;
		cuts.min_called = 0; cuts.max_duo = 1.0;                                    /* by candidates: everybody with a shared site, lists of 5 */
		refused = false;
		try { tr::search(dev, names, cuts, [&](const std::string &) {}, s); } catch (const tr::Error &e) { refused = strstr(e.what(), "give a lower --trio-duo") != nullptr; }
		CHECK(refused, "a candidate list that no batch takes is refused, naming --trio-duo");
	}
	{                                                                               /* nothing printed: the header alone */
		tr::Cuts cuts;
		cuts.max_duo = -1;
		std::string none;
		tr::Stats s;
		CHECK(tr::search(dev, names, cuts, [&](const std::string &t) { none += t; }, s) == 0 && none == tr::header_line(false) && s.children == 0, "the header alone");
	}
	{
		const std::vector<tr::PedTrio> trios = { { 2, 0, 1 }, { 3, 1, 0 }, { 2, 4, 0 }, { 4, 5, 5 }, { 2, 1, 0 } };
		tr::Cuts cuts;
		cuts.min_called = 300;                                                      /* u2 has 200 sites */
		std::string ped, pedWant = tr::header_line(true);
		tr::Stats s;
		const uint64_t before = m.duo_calls;
		CHECK(tr::pedigree(dev, names, trios, cuts, [&](const std::string &t) { ped += t; }, s) == 0, "the pedigree run ends well");
		for (const tr::PedTrio &t : trios) {
			const ntsm_eval_trio_record r = m.trio_of(t.child, t.father, t.mother);
			tr::row_line(pedWant, names[t.child].c_str(), names[t.father].c_str(), names[t.mother].c_str(), r, m.duo_of(t.child, t.father), m.duo_of(t.child, t.mother),
			             tr::verdict_of(r, cuts.min_called, cuts.max_rate));
		}
		CHECK(ped == pedWant, "the pedigree prints\n%swant\n%s", ped.c_str(), pedWant.c_str());
		CHECK(ped.find("\tok\n") != std::string::npos && ped.find("\tfail\n") != std::string::npos && ped.find("\tlowcov\n") != std::string::npos, "each verdict occurs");
		CHECK(m.duo_calls - before == 3 && s.rows == 5, "one duo row per distinct child");
	}
	printf("runs: by candidates and exhaustively the same two rows, in one batch and in batches of one list; -a; the pedigree's verdicts\n");
}

int main()
{
	candidate_rule();
	batches();
	pedigree_text();
	name_matching();
	row_text();
	runs();
	printf("ok\n");
	return 0;
}
