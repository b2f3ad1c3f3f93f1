/*
 * eval_store.hpp -- the cohort store of ntsmEval (--pack / --against) and the reader of one counts
 * file that the all-pairs path, the packer and the query share.  Header only, host only, no HIP.
 *
 * The store is one little-endian binary file, no compression, no pointers:
 *
 *   header, 64 bytes
 *       0   char[8]   magic "NTSMCOH1"
 *       8   uint32    version = 1
 *      12   uint32    n_sites
 *      16   uint64    n_samples
 *      24   uint64    byte offset of the first sample record
 *      32   uint64    record stride in bytes (a multiple of 8) = 1056 + 8 * n_sites
 *      40   24 bytes  zero
 *   locus section, from byte 64
 *       the n_sites locus IDs in order, each NUL-terminated; zero bytes up to the next multiple of 8;
 *       distinct[n_sites][2] as uint32 (distinctAT, distinctCG of the file that fixed the loci)
 *   sample records, n_samples of them, record r at first + r * stride
 *       0   uint64    raw_total    (#@TK; 0 where the file has no such line)
 *       8   uint64    total        (sum over the file's lines of uint32(countAT + countCG): wraps at 2^32 per line, then widens)
 *      16   uint64    sum_of_sums  (sum over the sites of uint32(sumAT + sumCG), the same wrap)
 *      24   uint32    kmer_size    (#@KS; 0 where the file has no such line)
 *      28   uint32    reserved, zero
 *      32   char[1024] the sample's name (the input path as given), NUL-padded; at most 1023 bytes
 *    1056   uint32    counts[n_sites][2]
 *
 * The stride is the same for every record, so the counts of consecutive samples lie at a constant pitch and a mapped store
 * goes to the device with one 2-D copy per chunk.  The per-site sums are not stored: mergeCounts is their only reader and
 * merging from a store is refused.  A store is valid when magic and version match, the locus section parses inside the file,
 * first and stride are the values the layout gives for n_sites, and the file's size is first + n_samples * stride exactly.
 */
#ifndef NTSM_EVAL_STORE_HPP
#define NTSM_EVAL_STORE_HPP

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

namespace ntsm {
namespace eval_store {

constexpr char kMagic[8] = { 'N', 'T', 'S', 'M', 'C', 'O', 'H', '1' };
constexpr uint32_t kVersion = 1;
constexpr size_t kHeaderBytes = 64, kNameBytes = 1024, kRecordHead = 32 + kNameBytes;

struct Header {
	char magic[8];
	uint32_t version, n_sites;
	uint64_t n_samples, first, stride;
	uint8_t zero[24];
};
static_assert(sizeof(Header) == kHeaderBytes, "the store header is 64 bytes");

struct RecordHead {
	uint64_t raw_total, total, sum_of_sums;
	uint32_t kmer_size, reserved;
	char name[kNameBytes];
};
static_assert(sizeof(RecordHead) == kRecordHead, "a record's head is 1056 bytes");

/* what a refusal of --pack / --against carries; the all-pairs path never sees one */
struct Error : std::runtime_error { using std::runtime_error::runtime_error; };

typedef std::unordered_map<std::string, unsigned> LocusIndex;

/* src/CompareCounts.hpp:934-940 */
inline std::pair<unsigned, unsigned> loadPair(std::stringstream &ss, std::string &item)
{
	const unsigned a = (unsigned) std::stoul(item);
	std::getline(ss, item, '\t');
	const unsigned b = (unsigned) std::stoul(item);
	std::getline(ss, item, '\t');
	return std::make_pair(a, b);
}

/* src/CompareCounts.hpp:30-70: the first file of a run fixes the loci and the distinct columns */
inline void read_locus_table(const std::string &path, LocusIndex &index, std::vector<std::string> &locus, std::vector<uint32_t> &distinct)
{
	std::ifstream fh(path);
	std::string line;
	while (fh.is_open() && std::getline(fh, line)) {
		if (line.empty() || line[0] == '#') continue;
		std::stringstream ss(line);
		std::string item;
		std::getline(ss, item, '\t');
		index[item] = (unsigned) locus.size();
		locus.push_back(item);
		for (int s = 0; s < 5; ++s) std::getline(ss, item, '\t');
		const auto d = loadPair(ss, item);
		distinct.push_back(d.first);
		distinct.push_back(d.second);
	}
}

struct Scalars { uint64_t raw_total = 0, total = 0; unsigned kmer_size = 0; };

/* src/CompareCounts.hpp:71-114: one counts file against a given locus index.  counts and sums are the sample's rows,
 * [n_sites][2], zero on entry: a locus the file lacks stays 0, a locus it repeats keeps the last line and adds both to the
 * total.  An unknown locus is std::out_of_range, as in the reference; with `refuse_unknown` it is an Error that names it. */
inline void parse_counts_file(const std::string &path, const LocusIndex &index, uint32_t *counts, uint32_t *sums, Scalars &sc,
		bool refuse_unknown = false)
{
	std::ifstream fh(path);
	std::string line;
	while (fh.is_open() && std::getline(fh, line)) {
		if (line.empty()) continue;
		std::stringstream ss(line);
		std::string item;
		std::getline(ss, item, '\t');
		if (line[0] == '#') {
			if (item == "#@TK") { std::getline(ss, item, '\t'); sc.raw_total = std::stoull(item); }
			else if (item == "#@KS") { std::getline(ss, item, '\t'); sc.kmer_size = (unsigned) std::stoull(item); }
			continue;
		}
		if (refuse_unknown && !index.count(item)) throw Error("locus " + item + " of " + path + " is not in the store");
		const size_t s = index.at(item);                           /* unknown locus: std::out_of_range, as in the reference */
		std::getline(ss, item, '\t');
		const auto cnt = loadPair(ss, item);
		counts[s * 2] = cnt.first;
		counts[s * 2 + 1] = cnt.second;
		sc.total += cnt.first + cnt.second;                        /* :104-106 unsigned + unsigned: wraps at 2^32, then widens */
		const auto sm = loadPair(ss, item);
		sums[s * 2] = sm.first;
		sums[s * 2 + 1] = sm.second;
	}
}

/* the sum computeErrorRate forms over [n_sites][2] (:1198-1216): the two columns of a site are added as unsigned, then widened */
inline uint64_t sum_of_pairs(const uint32_t *v, size_t n_sites)
{
	uint64_t sum = 0;
	for (size_t s = 0; s < n_sites; ++s) sum += v[2 * s] + v[2 * s + 1];
	return sum;
}

/* computeErrorRate (:1198-1216), stated once: a sample from files and a sample from a store go through here */
inline double error_rate(uint64_t raw_total, unsigned kmer_size, uint64_t sum_of_sums, uint64_t distinct_sum, uint64_t genome_size)
{
	if (!(raw_total > 0 && kmer_size > 0)) return -1.0;
	const double expected = double(raw_total) * double(distinct_sum) / double(genome_size);
	return 1.0 - std::pow(double(sum_of_sums) / expected, 1.0 / double(kmer_size));
}

inline size_t pad8(size_t x) { return (x + 7) & ~(size_t) 7; }

/* a store mapped read-only */
class View {
	void *map_ = nullptr;
	size_t size_ = 0;
public:
	Header h {};
	std::vector<std::string> locus;
	const uint32_t *distinct = nullptr;          /* [n_sites][2], inside the mapping */
	View() = default;
	View(const View &) = delete;
	View &operator=(const View &) = delete;
	~View() { if (map_) munmap(map_, size_); }

	/* maps and validates; throws Error with the reason */
	void open(const std::string &path)
	{
		const int fd = ::open(path.c_str(), O_RDONLY);
		if (fd < 0) throw Error("cannot open store " + path);
		struct stat st;
		if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { close(fd); throw Error(path + " is not a regular file"); }
		size_ = (size_t) st.st_size;
		if (size_ < kHeaderBytes) { close(fd); size_ = 0; throw Error(path + " is not a cohort store (shorter than its header)"); }
		map_ = mmap(nullptr, size_, PROT_READ, MAP_PRIVATE, fd, 0);
		close(fd);
		if (map_ == MAP_FAILED) { map_ = nullptr; throw Error("cannot map store " + path); }
		const char *base = (const char *) map_;
		memcpy(&h, base, kHeaderBytes);
		if (memcmp(h.magic, kMagic, 8) != 0) throw Error(path + " is not a cohort store (magic)");
		if (h.version != kVersion) throw Error(path + ": store version " + std::to_string(h.version) + ", this build reads " + std::to_string(kVersion));
		size_t at = kHeaderBytes;
		locus.reserve(h.n_sites);
		for (uint32_t s = 0; s < h.n_sites; ++s) {
			const void *nul = at < size_ ? memchr(base + at, 0, size_ - at) : nullptr;
			if (!nul) throw Error(path + ": the locus section runs past the end of the file");
			locus.emplace_back(base + at, (const char *) nul);
			at = (size_t) ((const char *) nul - base) + 1;
		}
		at = pad8(at);
		const uint64_t first = (uint64_t) at + 8ull * h.n_sites, stride = kRecordHead + 8ull * h.n_sites;
		if (h.first != first || h.stride != stride) throw Error(path + ": offsets in the header disagree with its locus section");
		if (h.n_samples > (UINT64_MAX - first) / stride || first + h.n_samples * stride != (uint64_t) size_)
			throw Error(path + ": " + std::to_string(size_) + " bytes, but its header describes " + std::to_string(h.n_samples) + " samples");
		distinct = (const uint32_t *) (base + at);
	}
	const char *base() const { return (const char *) map_; }                         /* the locus section is bytes 64 ... h.first */
	const RecordHead &head(uint64_t r) const { return *(const RecordHead *) ((const char *) map_ + h.first + r * h.stride); }
	const uint32_t *counts(uint64_t r) const { return (const uint32_t *) ((const char *) map_ + h.first + r * h.stride + kRecordHead); }
	std::string name(uint64_t r) const { const char *n = head(r).name; return std::string(n, strnlen(n, kNameBytes)); }
	LocusIndex index() const
	{
		LocusIndex ix;
		for (size_t s = 0; s < locus.size(); ++s) ix[locus[s]] = (unsigned) s;   /* a repeated ID keeps its last site, as in a run */
		return ix;
	}
};

inline bool write_all(int fd, const void *p, size_t n, uint64_t off)
{
	const char *c = (const char *) p;
	while (n) {
		const ssize_t w = pwrite(fd, c, n, (off_t) off);
		if (w <= 0) return false;
		c += w; n -= (size_t) w; off += (uint64_t) w;
	}
	return true;
}

/* ---- writing a store: the three steps --pack and `ntsmCount --cohort` (host/cohort.hpp) share ------------------------------ */

/* the header of a store with these loci and no sample yet */
inline Header new_header(const std::vector<std::string> &locus)
{
	Header h {};
	memcpy(h.magic, kMagic, 8);
	h.version = kVersion;
	h.n_sites = (uint32_t) locus.size();
	size_t at = kHeaderBytes;
	for (const std::string &l : locus) at += l.size() + 1;
	h.first = pad8(at) + 8ull * h.n_sites;
	h.stride = kRecordHead + 8ull * h.n_sites;
	return h;
}

/* header and locus section, bytes [0, h.first) of the file behind fd; distinct is [n_sites][2] */
inline bool write_head(int fd, const Header &h, const std::vector<std::string> &locus, const uint32_t *distinct)
{
	std::vector<char> head(h.first, 0);
	memcpy(head.data(), &h, kHeaderBytes);
	size_t at = kHeaderBytes;
	for (const std::string &l : locus) { memcpy(head.data() + at, l.c_str(), l.size() + 1); at += l.size() + 1; }
	if (h.n_sites) memcpy(head.data() + pad8(at), distinct, 8ull * h.n_sites);
	return write_all(fd, head.data(), head.size(), 0);
}

/* the head of a finished record; `rec` is h.stride zeroed bytes whose counts (from kRecordHead on) the caller fills */
inline void fill_record_head(char *rec, const std::string &name, uint64_t raw_total, unsigned kmer_size, uint64_t total, uint64_t sum_of_sums)
{
	RecordHead *rh = (RecordHead *) rec;
	rh->raw_total = raw_total;
	rh->total = total;
	rh->sum_of_sums = sum_of_sums;
	rh->kmer_size = kmer_size;
	memcpy(rh->name, name.data(), name.size());
}

inline void check_name(const std::string &f)
{
	if (f.size() >= kNameBytes) throw Error("the name " + f.substr(0, 40) + "... has " + std::to_string(f.size()) + " bytes; a store holds names of at most 1023");
}

/* Append finished records to an existing store: their bytes go behind the last record (write, any number of calls, whole
 * records or pieces of them), then commit() writes n_samples -- records first, the count last, so that a run that ends in
 * between leaves the store it found.  --pack commits once, with all its records; a cohort run commits every sample. */
class Appender {
	int fd_ = -1;
	std::string path_;
	uint64_t n_samples_ = 0, dst_ = 0;
public:
	Appender() = default;
	Appender(const Appender &) = delete;
	Appender &operator=(const Appender &) = delete;
	~Appender() { if (fd_ >= 0) close(fd_); }
	void open(const std::string &store, const Header &h)
	{
		path_ = store;
		fd_ = ::open(store.c_str(), O_WRONLY);
		if (fd_ < 0) throw Error("cannot write " + store);
		n_samples_ = h.n_samples;
		dst_ = h.first + h.n_samples * h.stride;
	}
	void write(const void *p, size_t n)
	{
		if (!write_all(fd_, p, n, dst_)) throw Error("cannot write " + path_);
		dst_ += n;
	}
	uint64_t commit(uint64_t n_more)
	{
		n_samples_ += n_more;
		if (!write_all(fd_, &n_samples_, 8, offsetof(Header, n_samples))) throw Error("cannot write " + path_);
		return n_samples_;
	}
};

/* --pack STORE FILES...: create the store, or append to it.  Every new record goes to STORE.tmp first, one sample in
 * memory at a time; only when all files have been read does STORE change (creation: the finished STORE.tmp is renamed;
 * append: the records are copied behind the last one, then n_samples is written).  Any refusal throws Error before that
 * point and leaves STORE as it was.  Returns the number of samples now in the store. */
inline uint64_t pack(const std::string &store, const std::vector<std::string> &files)
{
	if (files.empty()) throw Error("--pack needs input files");
	struct stat st;
	const bool exists = stat(store.c_str(), &st) == 0;
	Header h {};
	LocusIndex index;
	std::vector<std::string> locus;
	std::vector<uint32_t> distinct;
	std::unordered_set<std::string> names;
	if (exists) {
		View v;
		v.open(store);
		h = v.h;
		index = v.index();
		for (uint64_t r = 0; r < h.n_samples; ++r) names.insert(v.name(r));
	} else {
		read_locus_table(files[0], index, locus, distinct);
		h = new_header(locus);
	}
	for (const std::string &f : files) {
		check_name(f);
		if (!names.insert(f).second) throw Error("the name " + f + " is already in the store");
	}
	const size_t m = h.n_sites;
	const std::string tmp = store + ".tmp";
	const int fd = ::open(tmp.c_str(), O_CREAT | O_TRUNC | O_RDWR, 0644);
	if (fd < 0) throw Error("cannot write " + tmp);
	struct Cleanup { int fd; const std::string &path; bool keep = false; ~Cleanup() { close(fd); if (!keep) unlink(path.c_str()); } } tidy { fd, tmp };
	uint64_t off = 0;
	if (!exists) {                                   /* header (n_samples still 0) and locus section */
		if (!write_head(fd, h, locus, distinct.data())) throw Error("cannot write " + tmp);
		off = h.first;
	}
	std::vector<char> rec(h.stride);
	std::vector<uint32_t> sums(2 * m);
	for (const std::string &f : files) {
		std::fill(rec.begin(), rec.end(), 0);
		std::fill(sums.begin(), sums.end(), 0u);
		Scalars sc;
		parse_counts_file(f, index, (uint32_t *) (rec.data() + kRecordHead), sums.data(), sc, true);
		fill_record_head(rec.data(), f, sc.raw_total, sc.kmer_size, sc.total, sum_of_pairs(sums.data(), m));
		if (!write_all(fd, rec.data(), rec.size(), off)) throw Error("cannot write " + tmp);
		off += h.stride;
	}
	if (!exists) {
		const uint64_t total = files.size();
		if (!write_all(fd, &total, 8, offsetof(Header, n_samples))) throw Error("cannot write " + tmp);
		if (rename(tmp.c_str(), store.c_str()) != 0) throw Error("cannot rename " + tmp + " to " + store);
		tidy.keep = true;
		return total;
	}
	Appender to;
	to.open(store, h);
	std::vector<char> buf((size_t) 1 << 22);
	for (uint64_t src = 0; src < off;) {
		const ssize_t n = pread(fd, buf.data(), (size_t) std::min<uint64_t>(buf.size(), off - src), (off_t) src);
		if (n <= 0) throw Error("cannot write " + store);
		to.write(buf.data(), (size_t) n);
		src += (uint64_t) n;
	}
	return to.commit(files.size());
}

}  // namespace eval_store
}  // namespace ntsm

#endif
