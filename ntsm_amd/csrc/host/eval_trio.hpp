/*
 * eval_trio.hpp -- the host side of ntsmEval --trios: which samples are a child's candidate parents, how
 * the children's lists are cut into batches, the pedigree file and how its IDs find their samples, and the text of the table.
 * Header only, host only, no HIP: the integers are the device's (include/ntsm_eval_hip.h: ntsm_eval_trio_duos / _score), the
 * doubles are formed here from them, each in one stated expression and printed with std::to_string, so that a model can
 * reproduce the bytes.  tools/eval_trio_check.cpp holds it against its cases under the host sanitizers (`make trio_check`).
 *
 *   child parentA parentB called errHom errHet rate calledA oppA calledB oppB [verdict]      (tabs between the fields)
 *   rate = double(errHom + errHet) / double(called), NA where called == 0
 *   calledA, oppA = the duo record (child, parentA); calledB, oppB = (child, parentB)
 * A row of the search is printed under `all`; otherwise when called >= min_called and rate <= max_rate (a row whose rate is NA
 * is not).  A row of --ped is always printed and ends in its verdict: lowcov when called < min_called, else ok when
 * rate <= max_rate, else fail (called == 0 under min_called == 0: fail, there is no rate to pass).
 *
 * A candidate parent of child k is a sample p != k with duo.called >= min_called and double(opp) / double(called) <= max_duo
 * (called == 0 is never a candidate: it has no rate).
 */
#ifndef NTSM_EVAL_TRIO_HPP
#define NTSM_EVAL_TRIO_HPP

#include <algorithm>
#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/ntsm_eval_hip.h"
#include "eval_contam.hpp"

namespace ntsm {
namespace eval_trio {

constexpr const char *kHeader = "child\tparentA\tparentB\tcalled\terrHom\terrHet\trate\tcalledA\toppA\tcalledB\toppB";
constexpr uint64_t kDuoBandRecords = (1ull << 30) / sizeof(ntsm_eval_trio_duo);     /* 1 GiB of records, as --within's bands */
constexpr uint64_t kBatchRecords = (1ull << 30) / sizeof(ntsm_eval_trio_record);    /* and as much per batch of trio records */
/* the defaults of --trio-max, --trio-duo, --trio-called and --trio-depth: conventions a user overrides, chosen from one
 * simulation (a three-generation family among 9 samples x 2,000 sites at 30x and at 10x), not from real
 * data */
constexpr double kMaxRate = 0.02, kMaxDuo = 0.02;
constexpr uint32_t kMinCalled = 200, kMinDepth = 8;

struct Error : std::runtime_error { using std::runtime_error::runtime_error; };

using eval_contam::band_rows;               /* the band rule of the duo rectangle is --contam's, at this record's size */

inline bool is_candidate(const ntsm_eval_trio_duo &d, uint32_t min_called, double max_duo)
{
	return d.called != 0 && d.called >= min_called && double(d.opp) / double(d.called) <= max_duo;
}

/* the candidates of child k out of its duo row [n_db], in store order, appended to out; returns how many */
inline uint32_t candidates(const ntsm_eval_trio_duo *row, uint32_t n_db, uint32_t k, uint32_t min_called, double max_duo, std::vector<uint32_t> &out)
{
	uint32_t n = 0;
	for (uint32_t p = 0; p < n_db; ++p)
		if (p != k && is_candidate(row[p], min_called, max_duo)) { out.push_back(p); ++n; }
	return n;
}

inline uint64_t triples_of(uint64_t k) { return k < 2 ? 0 : k * (k - 1) / 2; }

/* The batch cutter: lists of lengths k[0 ... n) in order, cut into batches [begin, end) so that a batch's records -- the sum of
 * k (k - 1) / 2 -- stay within `limit`; the ends are appended to `ends`.  A single list beyond the limit cannot be scored:
 * returns its position, else n. */
inline size_t cut_batches(const uint32_t *k, size_t n, uint64_t limit, std::vector<size_t> &ends)
{
	uint64_t held = 0;
	for (size_t i = 0; i < n; ++i) {
		const uint64_t t = triples_of(k[i]);
		if (t > limit) return i;
		if (held + t > limit) { ends.push_back(i); held = 0; }
		held += t;
	}
	if (n) ends.push_back(n);
	return n;
}

inline bool has_rate(const ntsm_eval_trio_record &r) { return r.called != 0; }
inline double rate_of(const ntsm_eval_trio_record &r) { return double(uint64_t(r.err_hom) + uint64_t(r.err_het)) / double(r.called); }

/* whether the search prints the row */
inline bool row_printed(const ntsm_eval_trio_record &r, bool all, uint32_t min_called, double max_rate)
{
	return all || (has_rate(r) && r.called >= min_called && rate_of(r) <= max_rate);
}

inline const char *verdict_of(const ntsm_eval_trio_record &r, uint32_t min_called, double max_rate)
{
	return r.called < min_called ? "lowcov" : has_rate(r) && rate_of(r) <= max_rate ? "ok" : "fail";
}

/* one line, appended to out; verdict (may be NULL) is the last column of --ped */
inline void row_line(std::string &out, const char *child, const char *a, const char *b, const ntsm_eval_trio_record &r, const ntsm_eval_trio_duo &da,
		const ntsm_eval_trio_duo &db, const char *verdict)
{
	out += child; out += "\t"; out += a; out += "\t"; out += b;
	out += "\t"; out += std::to_string(r.called); out += "\t"; out += std::to_string(r.err_hom); out += "\t"; out += std::to_string(r.err_het);
	out += "\t"; out += has_rate(r) ? std::to_string(rate_of(r)) : "NA";
	out += "\t"; out += std::to_string(da.called); out += "\t"; out += std::to_string(da.opp);
	out += "\t"; out += std::to_string(db.called); out += "\t"; out += std::to_string(db.opp);
	if (verdict) { out += "\t"; out += verdict; }
	out += "\n";
}

/* The lines of n evaluated triples, in order: triple i is (child[i]; pa[i], pb[i]) with its record and the duo records (child,
 * parentA) and (child, parentB).  ped: every line, with its verdict; else the search's print rule. */
inline void rows_text(std::string &out, const char *const *names, size_t n, const uint32_t *child, const uint32_t *pa, const uint32_t *pb,
		const ntsm_eval_trio_record *rec, const ntsm_eval_trio_duo *da, const ntsm_eval_trio_duo *db, bool ped, bool all, uint32_t min_called, double max_rate)
{
	for (size_t i = 0; i < n; ++i)
		if (ped) row_line(out, names[child[i]], names[pa[i]], names[pb[i]], rec[i], da[i], db[i], verdict_of(rec[i], min_called, max_rate));
		else if (row_printed(rec[i], all, min_called, max_rate)) row_line(out, names[child[i]], names[pa[i]], names[pb[i]], rec[i], da[i], db[i], nullptr);
}

/* ---- the pedigree file */
struct PedLine { std::string id, father, mother; };
struct Ped { std::vector<PedLine> trios; uint64_t comments = 0, founders = 0; };

/* A six-column PED, white-space separated: columns 2 - 4 = individual, father, mother.  Lines starting with '#' and lines with 0
 * as father or mother are skipped and counted; empty lines are skipped; a line of fewer than four columns throws. */
inline Ped parse_ped(const std::string &text)
{
	Ped ped;
	size_t at = 0, line_no = 0;
	while (at < text.size()) {
		size_t end = text.find('\n', at);
		if (end == std::string::npos) end = text.size();
		++line_no;
		std::vector<std::string> col;
		for (size_t i = at; i < end && col.size() < 4;) {
			while (i < end && (text[i] == ' ' || text[i] == '\t' || text[i] == '\r')) ++i;
			size_t j = i;
			while (j < end && text[j] != ' ' && text[j] != '\t' && text[j] != '\r') ++j;
			if (j > i) col.push_back(text.substr(i, j - i));
			i = j;
		}
		const bool comment = end > at && text[at] == '#';
		at = end + 1;
		if (comment) { ++ped.comments; continue; }
		if (col.empty()) continue;
		if (col.size() < 4) throw Error("line " + std::to_string(line_no) + " of the pedigree file has fewer than four columns");
		if (col[2] == "0" || col[3] == "0") { ++ped.founders; continue; }
		ped.trios.push_back(PedLine { col[1], col[2], col[3] });
	}
	return ped;
}

inline std::string basename_of(const std::string &name)
{
	const size_t slash = name.rfind('/');
	return slash == std::string::npos ? name : name.substr(slash + 1);
}

inline std::string stem_of(const std::string &base)   /* the basename with one trailing _counts.txt, .counts.txt or .txt removed */
{
	for (const char *suffix : { "_counts.txt", ".counts.txt", ".txt" }) {
		const size_t n = std::string(suffix).size();
		if (base.size() >= n && base.compare(base.size() - n, n, suffix) == 0) return base.substr(0, base.size() - n);
	}
	return base;
}

constexpr int64_t kUnknown = -1, kAmbiguous = -2;

/* The sample an ID names: it equals, tried in this order, the stored name, the name's basename, or that basename's stem.  The
 * first level at which any sample matches decides: one match is the sample, more are kAmbiguous; no level: kUnknown. */
inline int64_t match_name(const std::vector<std::string> &names, const std::string &id)
{
	for (int level = 0; level < 3; ++level) {
		int64_t found = kUnknown;
		for (size_t i = 0; i < names.size(); ++i) {
			const std::string key = level == 0 ? names[i] : level == 1 ? basename_of(names[i]) : stem_of(basename_of(names[i]));
			if (key != id) continue;
			if (found != kUnknown) return kAmbiguous;
			found = (int64_t) i;
		}
		if (found != kUnknown) return found;
	}
	return kUnknown;
}

/* match_name, or the refusal that names the ID */
inline uint32_t sample_of(const std::vector<std::string> &names, const std::string &id)
{
	const int64_t s = match_name(names, id);
	if (s == kUnknown) throw Error("the pedigree names " + id + ", which matches no sample of the store");
	if (s == kAmbiguous) throw Error("the pedigree names " + id + ", which matches more than one sample of the store");
	return (uint32_t) s;
}

/* ---- the two runs, over whatever answers the device's two questions: the library in ntsmEval, a model in the check */
struct Device {
	/* ntsm_eval_trio_duos and ntsm_eval_trio_score without the session and the time: 0, or the code the run ends with */
	std::function<int(uint32_t row_first, uint32_t n_rows, ntsm_eval_trio_duo *out)> duos;
	std::function<int(const uint32_t *child, const uint64_t *offset, const uint32_t *cand, uint32_t n_children, ntsm_eval_trio_record *out)> score;
};
struct Cuts {
	uint32_t min_called = kMinCalled;
	double max_rate = kMaxRate, max_duo = kMaxDuo;
	bool all = false, exhaustive = false;
	uint64_t band_limit = kDuoBandRecords, batch_limit = kBatchRecords;
};
struct Stats { uint64_t bands = 0, children = 0, triples = 0, rows = 0; };
typedef std::function<void(const std::string &)> Sink;

inline std::string header_line(bool ped) { return std::string(kHeader) + (ped ? "\tverdict\n" : "\n"); }

/* The search: the duo rectangle in bands and each child's candidates (or, exhaustive, every other sample), the lists in
 * batches to `score`, and the rows that print, children in store order and within a child parentA < parentB.  The header goes
 * out with the first text, or alone.  Returns 0 or the device's code; throws Error for a list that no batch takes. */
inline int search(const Device &dev, const std::vector<std::string> &name_of, const Cuts &cuts, const Sink &sink, Stats &st)
{
	const uint32_t n = (uint32_t) name_of.size();
	std::vector<const char *> names(n);
	for (uint32_t i = 0; i < n; ++i) names[i] = name_of[i].c_str();
	std::vector<uint32_t> children, length, cand;                                  /* the children with two candidates or more; CSR by `length` */
	std::vector<ntsm_eval_trio_duo> cand_duo;                                      /* the duo (child, candidate) of every list position */
	std::vector<ntsm_eval_trio_duo> band;
	if (cuts.exhaustive) {
		if (n >= 3) for (uint32_t k = 0; k < n; ++k) { children.push_back(k); length.push_back(n - 1); }
	} else {
		for (uint32_t first = 0; first < n; ++st.bands) {
			const uint32_t rows = band_rows(first, n, cuts.band_limit);
			band.resize((size_t) rows * n);
			const int rc = dev.duos(first, rows, band.data());
			if (rc) return rc;
			for (uint32_t r = 0; r < rows; ++r) {
				const ntsm_eval_trio_duo *row = band.data() + (size_t) r * n;
				const size_t before = cand.size();
				if (candidates(row, n, first + r, cuts.min_called, cuts.max_duo, cand) < 2) { cand.resize(before); continue; }
				children.push_back(first + r);
				length.push_back((uint32_t) (cand.size() - before));
				for (size_t c = before; c < cand.size(); ++c) cand_duo.push_back(row[cand[c]]);
			}
			first += rows;
		}
	}
	st.children = children.size();
	std::vector<size_t> ends;
	const size_t bad = cut_batches(length.data(), length.size(), cuts.batch_limit, ends);
	if (bad != length.size())
		throw Error("the candidate list of " + name_of[children[bad]] + " has " + std::to_string(length[bad]) + " samples, and its "
		            + std::to_string(triples_of(length[bad])) + " trios are more than the " + std::to_string(cuts.batch_limit)
		            + " records of one batch: " + (cuts.exhaustive ? "run without --trio-exhaustive" : "give a lower --trio-duo"));
	bool headed = false;
	std::string text;
	std::vector<uint64_t> offset;
	std::vector<uint32_t> list, tc, ta, tb;
	std::vector<ntsm_eval_trio_record> rec, kept;
	std::vector<ntsm_eval_trio_duo> da, db, row;
	size_t begin = 0, list_at = 0;                                                 /* list_at: the batch's first position in cand / cand_duo */
	for (const size_t end : ends) {
		offset.assign(1, 0);
		const uint32_t *lists = cand.data() + list_at;
		if (cuts.exhaustive) {
			list.clear();
			for (size_t i = begin; i < end; ++i)
				for (uint32_t p = 0; p < n; ++p) if (p != children[i]) list.push_back(p);
			lists = list.data();
		}
		for (size_t i = begin; i < end; ++i) offset.push_back(offset.back() + length[i]);
		uint64_t records = 0;
		for (size_t i = begin; i < end; ++i) records += triples_of(length[i]);
		rec.resize(records);
		const int rc = dev.score(children.data() + begin, offset.data(), lists, (uint32_t) (end - begin), rec.data());
		if (rc) return rc;
		st.triples += records;
		/* the triples that print, with the list positions of their parents */
		tc.clear(); ta.clear(); tb.clear(); kept.clear(); da.clear(); db.clear();
		std::vector<uint64_t> pos_a, pos_b;
		uint64_t at = 0;
		for (size_t i = begin; i < end; ++i) {
			const uint32_t k = length[i];
			const uint32_t *l = lists + offset[i - begin];
			for (uint32_t p = 0; p < k; ++p)
				for (uint32_t q = p + 1; q < k; ++q, ++at) {
					if (!row_printed(rec[at], cuts.all, cuts.min_called, cuts.max_rate)) continue;
					tc.push_back(children[i]); ta.push_back(l[p]); tb.push_back(l[q]); kept.push_back(rec[at]);
					pos_a.push_back(offset[i - begin] + p); pos_b.push_back(offset[i - begin] + q);
				}
		}
		if (!cuts.exhaustive) {
			for (size_t t = 0; t < kept.size(); ++t) { da.push_back(cand_duo[list_at + pos_a[t]]); db.push_back(cand_duo[list_at + pos_b[t]]); }
		} else {                                                                   /* the duo rows of the children that print, in runs of neighbours */
			da.resize(kept.size()); db.resize(kept.size());
			for (size_t t = 0; t < kept.size();) {
				uint32_t first = tc[t], last = first;
				size_t u = t;
				while (u < kept.size() && (tc[u] == last || tc[u] == last + 1) && (uint64_t) (tc[u] - first + 1) * n <= std::max<uint64_t>(cuts.band_limit, n)) last = tc[u++];
				row.resize((size_t) (last - first + 1) * n);
				const int rd = dev.duos(first, last - first + 1, row.data());
				if (rd) return rd;
				++st.bands;
				for (; t < u; ++t) { da[t] = row[(size_t) (tc[t] - first) * n + ta[t]]; db[t] = row[(size_t) (tc[t] - first) * n + tb[t]]; }
			}
		}
		text.clear();
		if (!headed) { text = header_line(false); headed = true; }
		rows_text(text, names.data(), kept.size(), tc.data(), ta.data(), tb.data(), kept.data(), da.data(), db.data(), false, true, cuts.min_called, cuts.max_rate);
		st.rows += kept.size();
		sink(text);
		list_at += offset.back();
		begin = end;
	}
	if (!headed) sink(header_line(false));
	return 0;
}

/* --ped: one entry per complete trio (child; father, mother), in file order, every line printed with its verdict; the duo rows
 * of the children come from `duos`, one row per distinct child. */
struct PedTrio { uint32_t child, father, mother; };
inline int pedigree(const Device &dev, const std::vector<std::string> &name_of, const std::vector<PedTrio> &trios, const Cuts &cuts, const Sink &sink, Stats &st)
{
	const uint32_t n = (uint32_t) name_of.size();
	std::vector<const char *> names(n);
	for (uint32_t i = 0; i < n; ++i) names[i] = name_of[i].c_str();
	const size_t t = trios.size();
	std::vector<uint32_t> child(t), pa(t), pb(t), cand(2 * t);
	std::vector<uint64_t> offset(t + 1, 0);
	for (size_t i = 0; i < t; ++i) {
		child[i] = trios[i].child; pa[i] = trios[i].father; pb[i] = trios[i].mother;
		cand[2 * i] = pa[i]; cand[2 * i + 1] = pb[i];
		offset[i + 1] = 2 * (i + 1);
	}
	std::vector<ntsm_eval_trio_record> rec(t);
	const size_t step = (size_t) std::min<uint64_t>(std::max<uint64_t>(cuts.batch_limit, 1), UINT32_MAX);
	std::vector<uint64_t> part;
	for (size_t i = 0; i < t; i += step) {                                         /* one record per entry: a batch is that many entries */
		const size_t m = std::min(step, t - i);
		part.assign(m + 1, 0);
		for (size_t j = 0; j <= m; ++j) part[j] = 2 * j;
		const int rc = dev.score(child.data() + i, part.data(), cand.data() + 2 * i, (uint32_t) m, rec.data() + i);
		if (rc) return rc;
	}
	st.children = st.triples = st.rows = t;
	std::vector<ntsm_eval_trio_duo> da(t), db(t), row(n);
	std::vector<size_t> order(t);
	for (size_t i = 0; i < t; ++i) order[i] = i;
	std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return child[a] != child[b] ? child[a] < child[b] : a < b; });
	for (size_t o = 0; o < t; ++o) {
		const size_t i = order[o];
		if (o == 0 || child[order[o - 1]] != child[i]) {
			const int rc = dev.duos(child[i], 1, row.data());
			if (rc) return rc;
			++st.bands;
		}
		da[i] = row[pa[i]]; db[i] = row[pb[i]];
	}
	std::string text = header_line(true);
	rows_text(text, names.data(), t, child.data(), pa.data(), pb.data(), rec.data(), da.data(), db.data(), true, false, cuts.min_called, cuts.max_rate);
	sink(text);
	return 0;
}

/* the trios of a parsed pedigree as samples of the store: every ID matched (sample_of's refusals), and nobody their own parent */
inline std::vector<PedTrio> resolve(const Ped &ped, const std::vector<std::string> &name_of)
{
	std::vector<PedTrio> out;
	for (const PedLine &l : ped.trios) {
		const PedTrio t { sample_of(name_of, l.id), sample_of(name_of, l.father), sample_of(name_of, l.mother) };
		if (t.father == t.child || t.mother == t.child) throw Error("the pedigree names " + l.id + " as its own parent");
		out.push_back(t);
	}
	return out;
}

}  // namespace eval_trio
}  // namespace ntsm

#endif
