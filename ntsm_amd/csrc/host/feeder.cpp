#include "feeder.hpp"

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <mutex>
#include <sstream>
#include <thread>
#include <unistd.h>

#include "early_ingest.hpp"
#include "pack2.hpp"

namespace ntsm {

static std::mutex g_stderr;

void say(const std::string &line)
{
	std::lock_guard<std::mutex> lk(g_stderr);
	std::cerr << line << std::endl;
}

[[noreturn]] void fatal(const std::string &message)
{
	static std::atomic<bool> dying { false };
	if (dying.exchange(true)) for (;;) std::this_thread::sleep_for(std::chrono::seconds(1));
	say(message);
	fflush(nullptr);
	_exit(1);
}

void Feeder::die(int rc, const char *what) const
{
	std::ostringstream m;
	m << "ntsmCount: " << what << ": " << ntsm_strerror(rc);
	if (rc == NTSM_ERR_HIP) m << " (hipError " << ntsm_last_hip_error() << ")";
	fatal(m.str());
}

Feeder::Feeder(const Options &opt, ntsm_ctx *ctx, uint64_t max_hits, bool lane)
	: m_opt(opt), m_ctx(ctx), m_useLane(lane), m_packed(lane && opt.pack), m_maxCounts(max_hits), m_cfgBytes(slot_bytes(opt, lane))
{
	open("cannot size staging buffers");
}

/* the two slots at m_cfgBytes: a lane of their own, or the context's.  `what` names the failure of resizing the context's slots
 * (first sizing or growth); a lane that cannot be opened says so itself, whatever it was opened for */
void Feeder::open(const char *what)
{
	const uint64_t cap_reads = m_cfgBytes / 64 + 16;
	const int rc = !m_useLane ? ntsm_set_batch_capacity(m_ctx, m_cfgBytes, cap_reads)
	             : m_packed ? ntsm_lane_open_packed(m_ctx, m_cfgBytes, &m_lane) : ntsm_lane_open(m_ctx, m_cfgBytes, cap_reads, &m_lane);
	if (rc) die(rc, m_useLane ? "cannot open a producer lane" : what);
}

void Feeder::closeLane(const char *what)
{
	if (!m_lane) return;
	const int rc = ntsm_lane_close(m_lane);
	m_lane = nullptr;
	if (rc) die(rc, what);
}

Feeder::~Feeder() { if (m_lane) ntsm_lane_close(m_lane); }

void Feeder::finish()
{
	flush();
	closeLane("cannot close a producer lane");
}

/* hand the held slot to the library with n bytes / positions of n_reads reads in it (0, 0: back empty) and forget it */
void Feeder::submit(uint64_t n, uint32_t n_reads, uint64_t n_bases, const char *what)
{
	const int rc = m_packed ? ntsm_lane_submit_packed(m_lane, n, n_reads, n_bases)
	             : m_useLane ? ntsm_lane_submit(m_lane, n, n_reads) : ntsm_submit_staged(m_ctx, n, n_reads);
	if (rc) die(rc, what);
	m_bases = nullptr;
	discard();
}

void Feeder::flush()
{
	if (!m_bases || m_nReads == 0) return;
	submit(m_fill, m_nReads, m_nBases, "submit failed");
	if (m_maxCounts != 0) {                              /* armed: submission was synchronous */
		ntsm_totals t;
		const int rc = ntsm_sync(m_ctx, &t);
		if (rc) die(rc, "sync failed");
		if (t.early_stop) {
			/* the reference prints m_totalReads here, a counter it only advances under -vvv and only after a read has been
			 * processed (src/FingerPrint.hpp:70-72): 0 for -v / -vv, the reads before the crossing one for -vvv */
			if (m_opt.verbose > 0)
				std::cerr << "max count reached at " << (m_opt.verbose > 2 ? t.reads_consumed - 1 : 0) << " reads, " << t.total_kmers
				          << " k-mers, " << t.total_hits << " total counts, and " << t.total_bases
				          << " total bases " << std::endl;
			m_earlyTerm = true;
		}
	}
}

void Feeder::progressLine(uint64_t reads)
{
	flush();                                               /* may trip the -m threshold: the line is printed all the same, like the reference's */
	ntsm_totals t;
	const int rc = ntsm_sync(m_ctx, &t);
	if (rc) die(rc, "sync failed");
	std::cerr << "Current Total: " << reads << " reads, " << t.total_kmers << " k-mers, " << t.total_hits
	          << " total counts, and " << t.total_bases << " total bases " << std::endl;
}

/* Make the held slot one that takes `ext` more bytes / positions; `need` is the slot size that item asks for.  False:
 * the -m threshold tripped on the way (nothing is held then, and nothing more is counted). */
bool Feeder::reserve(uint64_t ext, uint64_t need)
{
	if (m_bases && !fits(ext)) flush();
	if (m_earlyTerm) return false;
	/* still held: an acquired but empty slot (after discard(): flush() has nothing to submit and keeps it) that is too
	 * small.  Hand it back empty, so that the grow path below runs instead of a write past its end */
	if (m_bases && !fits(ext)) submit(0, 0, 0, "cannot return an empty staging slot");
	if (m_bases) return true;
	if (need > (m_packed ? m_cfgBytes & ~31ull : m_cfgBytes)) {   /* longer than a slot (a packed one: whole groups of 32): grow both slots */
		m_cfgBytes = need + need / 2;
		const char *const what = "cannot grow staging buffers";
		closeLane(what);
		open(what);
	}
	const int rc = m_packed ? ntsm_lane_acquire_packed(m_lane, &m_bases, &m_valid, &m_cap)
	             : m_useLane ? ntsm_lane_acquire(m_lane, &m_bases, &m_cap, &m_readEnd, &m_capReads)
	                         : ntsm_staging_acquire(m_ctx, &m_bases, &m_cap, &m_readEnd, &m_capReads);
	if (rc) die(rc, "cannot acquire staging");
	return true;
}

void Feeder::feedRead(const char *seq, uint64_t len)
{
	if (!(m_bases && fits(extent(len))) && !reserve(extent(len), m_packed ? len + 64 : len + 1)) return;
	if (m_packed) {
		m_fill = pack2_append(m_bases, m_valid, m_fill, seq, len);
		m_nBases += len;
		++m_nReads;
		return;
	}
	memcpy(m_bases + m_fill, seq, len);
	m_fill += len;
	m_bases[m_fill] = 'N';                               /* read terminator */
	m_readEnd[m_nReads++] = m_fill;
	m_fill += 1;
}

void Feeder::submitChunk(const PackedChunk &c)
{
	if (!m_packed || c.n_reads == 0) return;
	const uint64_t need = (c.pos + 31) & ~31ull;               /* pack2 writes whole groups of 32 positions */
	/* an extent that no slot has: whatever is held goes (own staging submitted, an empty slot handed back), the chunk gets a fresh slot */
	reserve(~0ull, need);
	if (m_cap < need) die(NTSM_ERR_ARG, "staging slot smaller than an early chunk");
	memcpy(m_bases, c.codes, need / 4);
	memcpy(m_valid, c.valid, need / 8);
	submit(c.pos, c.n_reads, c.n_bases, "submit failed");
}

} // namespace ntsm
