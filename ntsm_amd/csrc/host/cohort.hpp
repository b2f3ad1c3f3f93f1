/*
 * cohort.hpp -- the host side of `ntsmCount --cohort MANIFEST --store STORE` that needs no device: the
 * manifest, the site set's lists in the form ntsm_sites_attach takes, and the store as a cohort run writes it -- one record
 * per finished sample, built from the device-reduced per-site values, appended through the same steps as `ntsmEval --pack`
 * (eval_store.hpp).  Header only, host only, no HIP.
 *
 * The contract: for a manifest the mode accepts, STORE is byte for byte what `ntsmCount [flags] READS... > NAME` per line and
 * then `ntsmEval --pack STORE NAME...` in manifest order give.  The reference has neither a manifest nor a store; what is
 * mirrored is what those two steps compute: printCountsMax's rows (src/FingerPrint.hpp:270-311) read back by
 * src/CompareCounts.hpp:71-114.
 */
#ifndef NTSM_COHORT_HPP
#define NTSM_COHORT_HPP

#include <unistd.h>

#include <cstdint>
#include <istream>
#include <string>
#include <unordered_set>
#include <vector>

#include "eval_store.hpp"
#include "site_set.hpp"

namespace ntsm {
namespace cohort {

using eval_store::Error;

struct Sample {
	std::string name;                          /* what the store records and ntsmEval prints */
	std::vector<std::string> reads;
};

/* MANIFEST: one sample per line, NAME<TAB>READS[<TAB>READS...]; empty lines and lines that start with '#' are skipped.
 * Throws Error for a line of another shape, a name the store cannot hold, a name listed twice and a manifest without a
 * sample.  `path` only names the manifest in the messages. */
inline std::vector<Sample> parse_manifest(std::istream &in, const std::string &path)
{
	std::vector<Sample> samples;
	std::unordered_set<std::string> names;
	std::string line;
	for (size_t no = 1; std::getline(in, line); ++no) {
		if (!line.empty() && line.back() == '\r') line.pop_back();
		if (line.empty() || line[0] == '#') continue;
		Sample s;
		size_t at = 0;
		bool first = true, bad = false;
		while (at <= line.size()) {
			const size_t tab = std::min(line.find('\t', at), line.size());
			const std::string field = line.substr(at, tab - at);
			if (field.empty()) bad = true;
			else if (first) s.name = field;
			else s.reads.push_back(field);
			first = false;
			at = tab + 1;
		}
		if (bad || s.reads.empty()) throw Error(path + " line " + std::to_string(no) + " is not NAME<TAB>READS[<TAB>READS...]");
		eval_store::check_name(s.name);
		if (!names.insert(s.name).second) throw Error("the name " + s.name + " is listed twice in " + path);
		samples.push_back(std::move(s));
	}
	if (samples.empty()) throw Error(path + " lists no sample");
	return samples;
}

inline void check_reads_exist(const std::vector<Sample> &samples)
{
	for (const Sample &s : samples)
		for (const std::string &r : s.reads)
			if (access(r.c_str(), R_OK) != 0) throw Error("input file " + r + " of sample " + s.name + " does not exist");
}

/* The site set as ntsm_sites_attach takes it, and the distinct columns of its rows.  A set the single run cannot print
 * (an erased k-mer in a list, a REF record without VAR: print_counts_max returns false) is refused here, before anything is
 * counted; so is a repeated locus ID, which --pack would give its last line and an empty slot. */
struct SiteLists {
	std::vector<uint32_t> offsets, kmer_ix, distinct;        /* 2n + 1, the lists end to end, [n][2] */
};

inline SiteLists site_lists(const SiteSet &sites)
{
	const size_t n = sites.ids.size();
	if (sites.ref.size() != n || sites.var.size() != n) throw Error("the sites file has an odd number of records: its counts cannot be printed");
	if (n > 0x7FFFFFFFull) throw Error("the sites file has more than 2^31 - 1 sites");
	std::unordered_set<std::string> ids;
	SiteLists l;
	l.offsets.reserve(2 * n + 1);
	l.distinct.reserve(2 * n);
	l.offsets.push_back(0);
	for (size_t i = 0; i < n; ++i) {
		if (!ids.insert(sites.ids[i]).second) throw Error("the locus " + sites.ids[i] + " is in the sites file twice: a cohort store needs distinct locus IDs");
		for (const auto *side : { &sites.ref[i], &sites.var[i] }) {
			for (const int64_t ix : *side) {
				if (ix == SiteSet::kErased)
					throw Error("the sites file has k-mers shared between sites (locus " + sites.ids[i] + "): its counts cannot be printed, rerun with -d");
				l.kmer_ix.push_back((uint32_t) ix);
			}
			if (l.kmer_ix.size() > 0xFFFFFFFFull) throw Error("the sites file has more than 2^32 - 1 k-mer places");
			l.offsets.push_back((uint32_t) l.kmer_ix.size());
			l.distinct.push_back((uint32_t) side->size());
		}
	}
	return l;
}

/* One finished sample as a store record (h.stride bytes): counts is [n_sites][2]; total and sum_of_sums are the two wrapped sums
 * the packer forms from the printed rows (eval_store.hpp: parse_counts_file, sum_of_pairs), here as the device delivered them. */
inline void build_record(std::vector<char> &rec, const eval_store::Header &h, const std::string &name, uint64_t raw_total, unsigned kmer_size,
		const uint32_t *counts, uint64_t total, uint64_t sum_of_sums)
{
	rec.assign(h.stride, 0);
	eval_store::fill_record_head(rec.data(), name, raw_total, kmer_size, total, sum_of_sums);
	if (h.n_sites) memcpy(rec.data() + eval_store::kRecordHead, counts, 8ull * h.n_sites);
}

/* The store of a cohort run.  check() is everything that can be said before anything is counted and writes nothing; begin()
 * creates a missing store (header, loci, no sample: STORE.tmp renamed) and opens it for appending; append() puts one record
 * behind the last and then writes n_samples, so that an interrupted run leaves a valid store of the finished samples. */
class Store {
	std::string path_;
	eval_store::Header h_ {};
	bool exists_ = false;
	std::unordered_set<std::string> held_;
	eval_store::Appender to_;
public:
	/* an existing store must be valid; returns false when there is none */
	bool open_existing(const std::string &path)
	{
		path_ = path;
		struct stat st;
		exists_ = stat(path.c_str(), &st) == 0;
		if (!exists_) return false;
		eval_store::View v;
		v.open(path);
		h_ = v.h;
		for (uint64_t r = 0; r < h_.n_samples; ++r) held_.insert(v.name(r));
		return true;
	}
	bool holds(const std::string &name) const { return held_.count(name) != 0; }
	uint64_t n_samples() const { return h_.n_samples; }
	const eval_store::Header &header() const { return h_; }
	/* an existing store holds exactly these loci in this order and the same distinct columns; a missing one gets its header */
	void check(const std::vector<std::string> &ids, const std::vector<uint32_t> &distinct)
	{
		if (!exists_) { h_ = eval_store::new_header(ids); return; }
		eval_store::View v;
		v.open(path_);
		if (v.h.n_sites != ids.size()) throw Error(path_ + " holds " + std::to_string(v.h.n_sites) + " loci, the sites file has " + std::to_string(ids.size()));
		for (size_t i = 0; i < ids.size(); ++i)
			if (v.locus[i] != ids[i]) throw Error("locus " + std::to_string(i + 1) + " of " + path_ + " is " + v.locus[i] + ", the sites file has " + ids[i] + " there");
		if (!ids.empty() && memcmp(v.distinct, distinct.data(), 8 * ids.size()) != 0)
			throw Error("the distinct columns of " + path_ + " are not those of the sites file");
	}
	void begin(const std::vector<std::string> &ids, const std::vector<uint32_t> &distinct)
	{
		if (!exists_) {
			const std::string tmp = path_ + ".tmp";
			const int fd = ::open(tmp.c_str(), O_CREAT | O_TRUNC | O_RDWR, 0644);
			if (fd < 0) throw Error("cannot write " + tmp);
			const bool ok = eval_store::write_head(fd, h_, ids, distinct.data());
			close(fd);
			if (!ok || rename(tmp.c_str(), path_.c_str()) != 0) { unlink(tmp.c_str()); throw Error("cannot write " + path_); }
			exists_ = true;
		}
		to_.open(path_, h_);
	}
	void append(const std::vector<char> &rec, const std::string &name)
	{
		to_.write(rec.data(), rec.size());
		h_.n_samples = to_.commit(1);
		held_.insert(name);
	}
};

} // namespace cohort
} // namespace ntsm
#endif
