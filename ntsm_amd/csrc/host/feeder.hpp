/*
 * feeder.hpp -- the staging batch one host thread is filling for a GPU context (include/ntsm_hip.h): the context's own
 * slots (single-threaded and -m runs), a producer lane of it that takes raw bytes, or one that takes packed codes
 * (pack2.hpp; -t N: all threads count into the same context).  Driven by one thread.
 *
 * The three modes share ONE slot lifecycle (Feeder::reserve): submit what is staged when the next item does not fit, hand
 * back a slot that is held but empty and too small, grow the slots when the item is larger than they are configured,
 * acquire.  They differ in the unit (bytes + 1 terminator, or positions), in the library calls and in the append.
 */
#ifndef NTSM_FEEDER_HPP
#define NTSM_FEEDER_HPP
#include <algorithm>
#include <cstdint>
#include <string>

#include "../../../include/ntsm_hip.h"
#include "options.hpp"

namespace ntsm {

/* A run that cannot go on ends with ONE message and exit status 1 (the reference: `exit(1)` where it cannot open a file,
 * src/FingerPrint.hpp:51-57).  The caller may be one of several feeder threads that all see the same failure (a lost lane
 * batch marks the whole context failed): the first one reports, the others wait for it.  _exit, not exit: the other threads
 * are inside the HIP runtime and nothing has been written to stdout yet (counts are printed only after everything is
 * counted), so there is nothing to flush and no destructor worth racing them for. */
[[noreturn]] void fatal(const std::string &message);
/* one whole line on stderr from a thread that may not be the only one writing there */
void say(const std::string &line);

/* Staging slot of a producer lane (-t N): 8 MiB, less when many threads would pin more than 512 MiB in total
 * (pinning costs 0.16 ms/MiB and competes with the table upload for the runtime's lock) */
inline uint64_t lane_bytes(unsigned threads)
{
	uint64_t b = 8ull << 20;
	while (b > (1ull << 20) && 2ull * threads * b > (512ull << 20)) b >>= 1;
	return b;
}

class Feeder {
public:
	Feeder(const Options &opt, ntsm_ctx *ctx, uint64_t max_hits, bool lane);
	~Feeder();
	Feeder(const Feeder &) = delete;
	Feeder &operator=(const Feeder &) = delete;
	/* Size of a slot in bytes (positions of a packed lane): -b with a floor; N producers share the GPU, so a lane's is
	 * clamped -- smaller slots keep the pinned footprint (and its allocation time) flat */
	static uint64_t slot_bytes(const Options &opt, bool lane)
	{
		const uint64_t b = std::max<uint64_t>(4096, opt.batch_bytes);
		return lane ? std::min<uint64_t>(b, lane_bytes(opt.threads)) : b;
	}
	/* a batch that was packed in ordinary memory before this lane existed (early_ingest.hpp): copied into a slot and submitted */
	void submitChunk(const struct PackedChunk &c);
	/* One read (insertCount(seq.s, seq.l), src/FingerPrint.hpp:89-103): append to the staging batch. */
	void feedRead(const char *seq, uint64_t len);
	void flush();
	/* Sink interface of the block-parallel ingest (parallel_fastq.hpp) */
	bool has_room(uint64_t len) const { return !m_bases || fits(extent(len)); }
	void feed(const char *seq, uint64_t len) { feedRead(seq, len); }
	/* Drop what is staged.  The slot stays acquired (it is handed back by the next submit), so reserve() must still
	 * be able to grow it: it tests the fit whenever a slot is held, not only when no slot is. */
	void discard() { m_fill = 0; m_nReads = 0; m_nBases = 0; }
	void begin_block(size_t) { }
	/* flush + close the lane (its totals fold into the context); the Feeder must not be fed afterwards */
	void finish();
	bool earlyTerm() const { return m_earlyTerm; }
	/* -vvv: "Current Total: ..." after `reads` reads (src/FingerPrint.hpp:70-78); submits and waits, context mode only */
	void progressLine(uint64_t reads);

private:
	[[noreturn]] void die(int rc, const char *what) const;
	/* what a read of len bytes may write beyond m_fill: the read and its terminator, or pack2_extent's whole groups */
	uint64_t extent(uint64_t len) const { return m_packed ? (len & ~31ull) + 32 : len + 1; }
	bool fits(uint64_t ext) const { return ext <= m_cap - m_fill && m_nReads < m_capReads; }   /* of the slot held: m_fill <= m_cap */
	bool reserve(uint64_t ext, uint64_t need);
	void submit(uint64_t n, uint32_t n_reads, uint64_t n_bases, const char *what);
	void open(const char *what);
	void closeLane(const char *what);

	const Options &m_opt;
	ntsm_ctx *m_ctx = nullptr;
	ntsm_lane *m_lane = nullptr;
	const bool m_useLane, m_packed;            /* packed (Options::pack): lanes only */
	uint64_t m_maxCounts = 0;
	uint64_t m_cfgBytes = 0;                   /* the size the slots are opened with; grows with the longest read */
	/* the slot held (m_bases != nullptr): bytes + read ends, or the codes and validity planes of a packed one */
	uint8_t *m_bases = nullptr, *m_valid = nullptr;
	uint64_t *m_readEnd = nullptr;
	uint64_t m_cap = 0, m_capReads = ~0ull;    /* bytes or positions; a packed slot has no limit of reads */
	uint64_t m_fill = 0, m_nBases = 0;         /* bytes or positions staged; packed: the sum of the read lengths */
	uint32_t m_nReads = 0;
	bool m_earlyTerm = false;
};

} // namespace ntsm
#endif
