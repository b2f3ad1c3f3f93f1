/*
 * eval_index.hpp -- the PCA index of a cohort store (ntsmEval --index / --near): the projections of
 * the store's samples, computed once and kept beside the store as STORE.pcaidx, together with the centre and rotation they
 * were computed with -- a query is projected with the same matrices by construction.  Header only, host only, no HIP.
 *
 * One little-endian binary file, no compression, no pointers:
 *
 *   header, 64 bytes
 *       0   char[8]   magic "NTSMPCX1"
 *       8   uint32    version = 1
 *      12   uint32    n_sites
 *      16   uint64    n_samples
 *      24   uint32    dim      (-d of the run that wrote it)
 *      28   uint32    min_cov  (-c of the run that wrote it)
 *      32   uint32    CRC-32 of the store's locus section (bytes 64 ... first record of the store)
 *      36   uint32    zero
 *      40   uint64    byte offset of the first record = 64 + 16 * n_sites * (1 + dim)
 *      48   uint64    record stride = 8 * dim + 16
 *      56   8 bytes   zero
 *   norm[n_sites], then rot[dim][n_sites]: what loadPCA gives for this -d, x87 80-bit numbers in 16-byte cells whose 6
 *       padding bytes are zero (two runs write the same bytes)
 *   records, n_samples of them
 *       0          double  cloud[dim]
 *       8 * dim    uint32  hets, homs, miss at min_cov (calcHomHetMiss, src/CompareCounts.hpp:742-767)
 *       8 * dim+12 uint32  zero
 *
 * The file's size is first + n_samples * stride exactly.  An index belongs to a store when magic, version and size fit,
 * n_sites and the CRC-32 of the locus section are the store's and n_samples equals the store's; with fewer samples it is
 * stale (the store has been appended to) and --index extends it.
 */
#ifndef NTSM_EVAL_INDEX_HPP
#define NTSM_EVAL_INDEX_HPP

#include "crc32_fast.hpp"
#include "eval_store.hpp"

namespace ntsm {
namespace eval_index {

using eval_store::Error;

constexpr char kMagic[8] = { 'N', 'T', 'S', 'M', 'P', 'C', 'X', '1' };
constexpr uint32_t kVersion = 1;
constexpr size_t kHeaderBytes = 64, kCell = 16, kCellUsed = 10;

struct Header {
	char magic[8];
	uint32_t version, n_sites;
	uint64_t n_samples;
	uint32_t dim, min_cov, locus_crc, zero;
	uint64_t first, stride;
	uint8_t pad[8];
};
static_assert(sizeof(Header) == kHeaderBytes, "the index header is 64 bytes");

inline std::string path_of(const std::string &store) { return store + ".pcaidx"; }
inline uint64_t first_of(uint32_t n_sites, uint32_t dim) { return kHeaderBytes + (uint64_t) kCell * n_sites * (1 + (uint64_t) dim); }
inline uint64_t stride_of(uint32_t dim) { return 8ull * dim + 16; }

inline uint32_t locus_crc(const eval_store::View &store)
{
	return crc32_fast(0, (const uint8_t *) store.base() + eval_store::kHeaderBytes, (size_t) store.h.first - eval_store::kHeaderBytes);
}

/* norm[n_sites] then rot[dim][n_sites] as the file holds them: 16-byte cells, the padding zero */
inline std::vector<char> matrix_bytes(const std::vector<long double> &norm, const std::vector<long double> &rot)
{
	static_assert(sizeof(long double) == kCell, "the index holds x87 numbers in 16-byte cells");
	std::vector<char> out((norm.size() + rot.size()) * kCell, 0);
	char *at = out.data();
	for (const std::vector<long double> *v : { &norm, &rot })
		for (const long double &x : *v) { memcpy(at, &x, kCellUsed); at += kCell; }
	return out;
}

/* one sample's record */
struct Entry { const double *cloud; uint32_t hets, homs, miss; };

/* an index mapped read-only */
class View {
	void *map_ = nullptr;
	size_t size_ = 0;
public:
	Header h {};
	View() = default;
	View(const View &) = delete;
	View &operator=(const View &) = delete;
	~View() { if (map_) munmap(map_, size_); }

	/* maps and validates the file on its own; throws Error with the reason */
	void open(const std::string &path)
	{
		const int fd = ::open(path.c_str(), O_RDONLY);
		if (fd < 0) throw Error("cannot open index " + path);
		struct stat st;
		if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { close(fd); throw Error(path + " is not a regular file"); }
		size_ = (size_t) st.st_size;
		if (size_ < kHeaderBytes) { close(fd); size_ = 0; throw Error(path + " is not a PCA index (shorter than its header)"); }
		map_ = mmap(nullptr, size_, PROT_READ, MAP_PRIVATE, fd, 0);
		close(fd);
		if (map_ == MAP_FAILED) { map_ = nullptr; throw Error("cannot map index " + path); }
		memcpy(&h, map_, kHeaderBytes);
		if (memcmp(h.magic, kMagic, 8) != 0) throw Error(path + " is not a PCA index (magic)");
		if (h.version != kVersion) throw Error(path + ": index version " + std::to_string(h.version) + ", this build reads " + std::to_string(kVersion));
		if (h.dim == 0 || h.first != first_of(h.n_sites, h.dim) || h.stride != stride_of(h.dim))
			throw Error(path + ": offsets in the header disagree with its sites and dimensions");
		if (h.n_samples > (UINT64_MAX - h.first) / h.stride || h.first + h.n_samples * h.stride != (uint64_t) size_)
			throw Error(path + ": " + std::to_string(size_) + " bytes, but its header describes " + std::to_string(h.n_samples) + " samples");
	}
	/* does it describe this store?  `stale_ok`: fewer samples than the store are accepted (--index extends it) */
	void check_store(const std::string &path, const eval_store::View &store, bool stale_ok) const
	{
		if (h.n_sites != store.h.n_sites || h.locus_crc != locus_crc(store)) throw Error(path + " was written for a store with other loci");
		if (h.n_samples > store.h.n_samples)
			throw Error(path + " holds " + std::to_string(h.n_samples) + " samples, the store " + std::to_string(store.h.n_samples) + ": delete " + path);
		if (h.n_samples < store.h.n_samples && !stale_ok)
			throw Error(path + " is stale: it holds " + std::to_string(h.n_samples) + " of the store's " + std::to_string(store.h.n_samples)
			            + " samples; run --index on the store again");
	}
	const char *matrices() const { return (const char *) map_ + kHeaderBytes; }
	size_t matrix_size() const { return (size_t) h.first - kHeaderBytes; }
	const char *records() const { return (const char *) map_ + h.first; }
	Entry entry(uint64_t r) const
	{
		const char *p = records() + r * h.stride;
		Entry e;
		e.cloud = (const double *) p;
		memcpy(&e.hets, p + 8ull * h.dim, 12);
		return e;
	}
	/* norm[n_sites] and rot[dim][n_sites] as long double again */
	void matrices(std::vector<long double> &norm, std::vector<long double> &rot) const
	{
		norm.assign(h.n_sites, 0.0L);
		rot.assign((size_t) h.dim * h.n_sites, 0.0L);
		const char *at = matrices();
		for (std::vector<long double> *v : { &norm, &rot })
			for (long double &x : *v) { memcpy(&x, at, kCellUsed); at += kCell; }
	}
};

/* Write the index of `store` for n_samples = kept + added samples: the header, the matrices, the first `kept` records taken
 * from `old_records` (an existing index that is being extended; NULL when kept == 0) and `added` new ones from cloud
 * [added][dim] and geno [added][3].  Goes through PATH.tmp and a rename, so the index is either the old or the new one; the
 * bytes are those of indexing the longer store at once. */
inline void write(const std::string &path, const eval_store::View &store, uint32_t dim, uint32_t min_cov, const std::vector<char> &matrices,
		const char *old_records, uint64_t kept, const double *cloud, const uint32_t *geno, uint64_t added)
{
	Header h {};
	memcpy(h.magic, kMagic, 8);
	h.version = kVersion;
	h.n_sites = store.h.n_sites;
	h.n_samples = kept + added;
	h.dim = dim;
	h.min_cov = min_cov;
	h.locus_crc = locus_crc(store);
	h.first = first_of(h.n_sites, dim);
	h.stride = stride_of(dim);
	if (matrices.size() != h.first - kHeaderBytes) throw Error("the matrices of " + path + " do not fit its sites and dimensions");
	const std::string tmp = path + ".tmp";
	const int fd = ::open(tmp.c_str(), O_CREAT | O_TRUNC | O_RDWR, 0644);
	if (fd < 0) throw Error("cannot write " + tmp);
	struct Cleanup { int fd; const std::string &path; bool keep = false; ~Cleanup() { close(fd); if (!keep) unlink(path.c_str()); } } tidy { fd, tmp };
	bool ok = eval_store::write_all(fd, &h, kHeaderBytes, 0) && eval_store::write_all(fd, matrices.data(), matrices.size(), kHeaderBytes);
	if (ok && kept) ok = eval_store::write_all(fd, old_records, (size_t) (kept * h.stride), h.first);
	std::vector<char> rec((size_t) h.stride);
	for (uint64_t r = 0; ok && r < added; ++r) {
		std::fill(rec.begin(), rec.end(), 0);
		memcpy(rec.data(), cloud + r * dim, 8ull * dim);
		memcpy(rec.data() + 8ull * dim, geno + r * 3, 12);
		ok = eval_store::write_all(fd, rec.data(), rec.size(), h.first + (kept + r) * h.stride);
	}
	if (!ok) throw Error("cannot write " + tmp);
	if (rename(tmp.c_str(), path.c_str()) != 0) throw Error("cannot rename " + tmp + " to " + path);
	tidy.keep = true;
}

}  // namespace eval_index
}  // namespace ntsm

#endif
