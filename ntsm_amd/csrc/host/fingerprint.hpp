/*
 * fingerprint.hpp -- host mirror of the reference's FingerPrint class for the ntsmCount path
 * (src/FingerPrint.hpp): same public calls in the same order as src/ntSeqMatchCount.cpp:177-181,
 * same stdout/stderr bytes; the per-read insertCount loop is replaced by batched submission to
 * the HIP library (include/ntsm_hip.h).
 */
#ifndef NTSM_FINGERPRINT_HPP
#define NTSM_FINGERPRINT_HPP
#include <cstdint>
#include <functional>
#include <iosfwd>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "feeder.hpp"
#include "host_shape.hpp"
#include "site_set.hpp"

namespace ntsm {

class FingerPrint {
public:
	/* What the caller has to say about the site set before any device is touched: a message refuses the run (one line on
	 * stderr, exit status 1; the loader's collision warnings are printed only where the run goes on). */
	typedef std::function<std::string(const SiteSet &)> SiteCheck;
	explicit FingerPrint(const Options &opt, const SiteCheck &check = nullptr);   /* FingerPrint(), :35-44 */
	~FingerPrint();
	void computeCounts(const std::vector<std::string> &filenames);   /* :46-87 */
	void printOptionalHeader(std::ostream &out) const;   /* :261-268 */
	void printCountsMax(std::ostream &out) const;        /* :270-311 */
	std::string printInfoSummary();                      /* :313-349 */
	uint64_t maxCounts() const { return m_maxCounts; }
	const SiteSet &sites() const { return m_sites; }
	/* ---- more than one sample on the same contexts (`--cohort`; the reference counts one sample per process) ----
	 * the site set's lists on the device (ntsm_sites_attach on context [0]: offsets has 2 * n_sites + 1 entries) */
	void attachSites(const uint32_t *offsets, const uint32_t *kmer_ix, uint32_t n_sites);
	/* Start the next sample: every context forgets its counts and totals (the tables and the attached lists stay), -m is
	 * armed again, and computeCounts finds the feeders as it finds them in a fresh process. */
	void nextSample();
	/* The sample just counted as its per-site record, reduced on the device (ntsm_sites_reduce; after ntsm_allreduce where
	 * there are several contexts): what printCountsMax's rows hold, the two sums ntsmEval forms from them, the covered
	 * sites, and the run's totals (total_kmers is the #@TK value). */
	struct SiteRecord {
		std::vector<uint32_t> counts, sums;              /* [n_sites][2] */
		ntsm_site_totals sites {};
		ntsm_totals run {};
		double wait_s = 0, reduce_s = 0, kernel_ms = 0;  /* NTSM_PHASE_TIMES: the sync, reduce + download, the kernel by HIP events */
	};
	SiteRecord siteRecord();

private:
	void fetchResults();

	Options m_opt;
	IngestPlan m_plan { 1, 1, 1, 1 };                       /* thread counts from the CPUs granted (host_shape.hpp) */
	SiteSet m_sites;
	uint64_t m_maxCounts = 0;
	/* the routing rules of computeCounts, each stated once */
	bool lanesPossible() const;                          /* -t N without -m or -vvv, as far as the command line tells */
	size_t parsers() const { return std::min<size_t>(m_opt.threads, std::max(1u, m_plan.feeders)); }   /* threads that parse ONE file, lane runs */
	uint64_t blockBytes() const { return std::min<uint64_t>(m_opt.block_bytes, 2 * lane_bytes(m_opt.threads)); }
	bool sideBySide(const std::vector<std::string> &files, size_t threads) const;
	void shareDecoders(size_t readers, size_t n_files) const;
	Feeder &feederFor(size_t t);                         /* thread t's lane on device devices[t % n] (created on first use) */
	std::vector<Feeder *> openFeeders(size_t first, size_t n);
	/* Count every record a reader delivers (src/FingerPrint.hpp:49-81); stops early once the -m threshold tripped. */
	void feedReads(Feeder &f, class SeqReader &rd);
	void feedFile(Feeder &f, const std::string &path, uint64_t offset = 0);
	uint64_t m_totalReads = 0;                           /* the reference's m_totalReads: advanced under -vvv only */
	void closeLanes();
	void joinPrep();
	[[noreturn]] void quit(const std::string &message);
	std::vector<std::thread> m_prep;                     /* per device: GPU bring-up, streams, pinned pool while the sites are parsed */
	std::vector<ntsm_ctx *> m_ctx;                       /* one GPU context per distinct -g device, [0] = first device */
	std::vector<int> m_ctxDevice;
	std::unique_ptr<Feeder> m_main;                      /* context [0]'s own staging: single-threaded and -m runs */
	std::vector<std::unique_ptr<Feeder>> m_lanes;        /* -t N: one producer lane per host thread */
	std::unique_ptr<class EarlyIngest> m_early;          /* the first input file, parsed while the sites load (early_ingest.hpp) */
	/* A finished gzip stream holds 0.5-0.8 GB of buffers it touched (symbol buffers of the decoder pool, pieces): giving them
	 * back costs the kernel 0.07-0.1 s per stream, which used to sit between two files and in front of the last line.  Streams
	 * are therefore destroyed on a side thread while the next file is read (joined by the destructor; _exit does not wait). */
	std::vector<std::thread> m_retire;
	template <class T> void retireLater(std::unique_ptr<T> p)
	{
		if (p) m_retire.emplace_back([q = std::shared_ptr<T>(std::move(p))]() mutable { q.reset(); });
	}
	/* the routes of computeCounts */
	void countOrdered(const std::vector<std::string> &files);
	void drainEarly();
	std::vector<std::string> countBlockParallel(const std::vector<std::string> &files);   /* these two return the files they left */
	std::vector<std::string> countBigGzip(const std::vector<std::string> &files);
	void countOnePerThread(const std::vector<std::string> &files);
	void countGzStream(std::unique_ptr<class GzStream> gz, const std::string &fn, size_t first_feeder, size_t n_feeders);                                   /* its chunks -> the lanes */
	/* results */
	bool m_fetched = false;
	ntsm_totals m_totals {};
	std::vector<uint64_t> m_counts;
};

} // namespace ntsm
#endif
