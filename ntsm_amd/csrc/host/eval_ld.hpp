/*
 * eval_ld.hpp -- the host side of ntsmEval --ld: the moments and r^2 of a site pair's record, the band
 * rule of the selection and its halving, the text of the table, and the prune.  Header only, no HIP call: the integers are the
 * device's (include/ntsm_eval_hip.h: ntsm_eval_ld_select), the double is formed here from them in one stated expression and
 * printed with std::to_string, so that a model can reproduce the bytes.  ntsm_eval_ld.hip compiles the same expressions for the
 * device's test of a pair (NTSM_LD_HD is empty for a host compiler).  tools/eval_ld_check.cpp holds the header against its cases
 * under the host sanitizers (`make ld_check`).
 *
 *   siteA siteB n r2 dir                                                              (tabs between the fields)
 *   r2 = (double(cov) * double(cov)) / (double(vx) * double(vy)); dir = + when cov > 0, else -
 * Rows are the selected pairs in (a, b) order; under `all` every pair a < b with a defined r2.
 */
#ifndef NTSM_EVAL_LD_HPP
#define NTSM_EVAL_LD_HPP

#include <algorithm>
#include <cstdint>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/ntsm_eval_hip.h"

#ifdef __HIPCC__
#define NTSM_LD_HD __host__ __device__
#else
#define NTSM_LD_HD
#endif

namespace ntsm {
namespace eval_ld {

constexpr const char *kHeader = "siteA\tsiteB\tn\tr2\tdir\n";
constexpr uint64_t kPairBudget = (1ull << 30) / sizeof(ntsm_eval_ld_pair);           /* 1 GiB of selected pairs per call */
/* the defaults of --ld-min, --ld-called and --ld-depth: conventions a user overrides (r^2 >= 0.5 is a common prune cut, 20
 * samples the least at which an r^2 says anything, 8 reads the depth gate of --trios), not tuned on data */
constexpr double kMinR2 = 0.5;
constexpr uint32_t kMinCalled = 20, kMinDepth = 8;

struct Error : std::runtime_error { using std::runtime_error::runtime_error; };

/* the moments of a record, in int64: exact for counts up to 2^24 (n * Sxx <= 2^50) */
struct Moments { int64_t n, cov, vx, vy; };
NTSM_LD_HD inline Moments moments_of(const ntsm_eval_ld_record &r)
{
	const int64_t n = r.n, sx = (int64_t) r.hs + 2 * (int64_t) r.gs, sy = (int64_t) r.ht + 2 * (int64_t) r.gt;
	const int64_t sxx = (int64_t) r.hs + 4 * (int64_t) r.gs, syy = (int64_t) r.ht + 4 * (int64_t) r.gt;
	const int64_t sxy = (int64_t) r.hh + 2 * (int64_t) r.hg + 4 * (int64_t) r.gg;
	return Moments { n, n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy };
}
NTSM_LD_HD inline bool r2_defined(const Moments &m, uint32_t min_called) { return m.n >= (int64_t) min_called && m.vx != 0 && m.vy != 0; }
/* two multiplications and one division, each rounded once: every unit that includes this is compiled without contraction */
NTSM_LD_HD inline double r2_of(const Moments &m) { return ((double) m.cov * (double) m.cov) / ((double) m.vx * (double) m.vy); }
/* whether the pair of this record is selected, its order a < b aside */
NTSM_LD_HD inline bool selected(const ntsm_eval_ld_record &r, uint32_t min_called, double r2_min)
{
	const Moments m = moments_of(r);
	return r2_defined(m, min_called) && r2_of(m) >= r2_min;
}

/* ---- the band rule.  A call's capacity is the pair budget, never below n_sites pairs, so that one row always fits.  The walk
 * starts with every remaining row in one call; a call that finds more than the capacity (return 1) is run again over half the
 * rows, down to one row, and the following bands keep that size. */
inline uint64_t pair_cap(uint32_t n_sites, uint64_t budget) { return std::max<uint64_t>(budget, n_sites); }
inline uint32_t halved(uint32_t rows) { return rows > 1 ? rows / 2 : 1; }

struct Device {
	/* ntsm_eval_ld_select without the session and the time: 0, 1 (more than cap found) or the code the run ends with */
	std::function<int(uint32_t row_first, uint32_t n_rows, uint64_t cap, ntsm_eval_ld_pair *out, uint64_t *n_found)> select;
};
struct Stats { uint64_t bands = 0, reruns = 0, pairs = 0; };
typedef std::function<void(const ntsm_eval_ld_pair *, uint64_t)> PairSink;

/* every selected pair of the store, in (a, b) order, handed to `sink` band by band.  Returns 0 or the device's code. */
inline int walk(const Device &dev, uint32_t n_sites, uint64_t budget, const PairSink &sink, Stats &st)
{
	const uint64_t cap = pair_cap(n_sites, budget);
	/* no call finds more than the store's pairs a < b, so a small store asks for a small buffer; not touched beyond what a call writes */
	const uint64_t room = std::min<uint64_t>(cap, (uint64_t) n_sites * (n_sites ? n_sites - 1 : 0) / 2 + 1);
	std::unique_ptr<ntsm_eval_ld_pair[]> buf(new ntsm_eval_ld_pair[room]);
	uint32_t rows = n_sites;
	for (uint32_t first = 0; first < n_sites;) {
		rows = std::min(rows, n_sites - first);
		uint64_t found = 0;
		const int rc = dev.select(first, rows, cap, buf.get(), &found);
		if (rc == 1 && rows > 1) { rows = halved(rows); ++st.reruns; continue; }
		if (rc) return rc == 1 ? -1 : rc;                                              /* one row beyond n_sites pairs: not a thing the device can say */
		++st.bands;
		st.pairs += found;
		sink(buf.get(), found);
		first += rows;
	}
	return 0;
}

/* ---- the text */
inline void row_line(std::string &out, const char *a, const char *b, const ntsm_eval_ld_record &r)
{
	const Moments m = moments_of(r);
	out += a; out += "\t"; out += b; out += "\t"; out += std::to_string(r.n); out += "\t"; out += std::to_string(r2_of(m));
	out += m.cov > 0 ? "\t+\n" : "\t-\n";
}

/* the lines of these pairs, in their order; every pair has a defined r2 (the device selected it) */
inline void rows_text(std::string &out, const char *const *locus, const ntsm_eval_ld_pair *pairs, uint64_t n)
{
	for (uint64_t i = 0; i < n; ++i) row_line(out, locus[pairs[i].a], locus[pairs[i].b], pairs[i].rec);
}

/* ---- the prune: the sites in store order; site t is dropped when some selected pair (s, t), s < t, has s kept.  The pairs
 * arrive in (a, b) order, so when a pair (a, b) arrives every pair (s, a) has been seen and `kept[a]` is final. */
struct Prune {
	std::vector<uint8_t> kept;
	explicit Prune(uint32_t n_sites) : kept(n_sites, 1) {}
	/* the pairs among these that are selected at (min_called, r2_min): under -a the device's cut is lower than the prune's */
	void add(const ntsm_eval_ld_pair *pairs, uint64_t n, uint32_t min_called, double r2_min)
	{
		for (uint64_t i = 0; i < n; ++i)
			if (pairs[i].a < pairs[i].b && kept[pairs[i].a] && selected(pairs[i].rec, min_called, r2_min)) kept[pairs[i].b] = 0;
	}
	uint32_t n_kept() const { return (uint32_t) std::count(kept.begin(), kept.end(), 1); }
	std::string text(const char *const *locus) const
	{
		std::string out;
		for (size_t s = 0; s < kept.size(); ++s)
			if (kept[s]) { out += locus[s]; out += "\n"; }
		return out;
	}
};

}  // namespace eval_ld
}  // namespace ntsm

#endif
