#include "fingerprint.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <set>
#include <sstream>
#include <thread>
#include <sys/stat.h>

#include "early_ingest.hpp"
#include "gz_stream.hpp"
#include "parallel_fastq.hpp"
#include "parallel_gz_fastq.hpp"
#include "report.hpp"
#include "seq_reader.hpp"

namespace ntsm {

/* `(m_counts.size() * opt::covThresh) / 2` assigned to a uint64_t (src/FingerPrint.hpp:41-43).
 * Out-of-range doubles (the DBL_MAX default, negatives) are undefined behaviour in the
 * reference; every such value yields a threshold that never trips, which is what is kept. */
static uint64_t threshold_from(double n_distinct, double cov)
{
	if (cov == 0) return 0;
	const double x = (n_distinct * cov) / 2;
	if (!(x == x) || x >= 18446744073709551616.0) return 0;
	if (x < 0) return UINT64_MAX;
	return (uint64_t) x;
}

namespace {
/* a regular file of at least min_bytes that starts with the gzip magic: gets the decoder pool (plain or BGZF) */
bool big_gzip_input(const std::string &fn, uint64_t min_bytes)
{
	struct stat st;
	return stat(fn.c_str(), &st) == 0 && S_ISREG(st.st_mode) && (uint64_t) st.st_size >= min_bytes && GzStream::is_gzip(fn);
}
/* from this many big .gz inputs on they are read side by side, one reader per file, instead of one after the other with the whole pool */
size_t side_by_side_from(unsigned threads) { return std::max<size_t>(3, threads / 4); }

/* seconds since the last call (the first: since it was made), for the [phase] lines of NTSM_PHASE_TIMES */
struct Lap {
	std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
	double operator()()
	{
		const auto was = t;
		t = std::chrono::steady_clock::now();
		return std::chrono::duration<double>(t - was).count();
	}
};
} // namespace

/* Lanes take a run with -t N and neither -m nor -vvv.  This is what the command line tells before the sites are loaded. */
bool FingerPrint::lanesPossible() const
{
	const bool maybe_armed = m_opt.covThresh != 0 && m_opt.covThresh < 1e300;
	return m_opt.threads > 1 && !maybe_armed && m_opt.verbose <= 2;
}

/* Many big .gz files (a lane's worth of .fq.gz: four or more with -t 16) are better off side by side, one reader per file
 * with the -t threads' worth of decoders shared out among them, than one after the other with the whole pool each: every
 * file pays the pool's start and its drain, and the in-order share of the decoding is the cheapest (no block search, no
 * marker pass).  Measured, 8 x 262 MB of .gz, -t 16: 1.49 s one after the other; with 8 / 4 files of 4e7 reads in total
 * 0.97 / 1.03 s against 1.07 / 1.35 s with the first file taken early and alone. */
bool FingerPrint::sideBySide(const std::vector<std::string> &files, size_t threads) const
{
	if (getenv("NTSM_ZLIB_ONLY")) return false;
	size_t n_big = 0;
	for (const std::string &fn : files) n_big += big_gzip_input(fn, m_opt.gz_parallel_min_bytes) ? 1 : 0;
	return n_big >= side_by_side_from((unsigned) threads);
}

/* BGZF (bgzip) input is inflated block-parallel: share the -t threads among the files that are read at once */
void FingerPrint::shareDecoders(size_t readers, size_t n_files) const
{
	GzStream::set_decoder_threads((unsigned) std::max<size_t>(1, m_opt.threads / std::max<size_t>(1, std::min(readers, n_files))));
}

void FingerPrint::quit(const std::string &message)
{
	std::cerr << message << std::endl;
	joinPrep();                                            /* never exit() under a thread that is inside the HIP runtime */
	exit(1);
}

FingerPrint::FingerPrint(const Options &opt, const SiteCheck &check) : m_opt(opt)
{
	/* -t N is a ceiling: the threads that parse follow the CPUs this process is granted (affinity mask, cgroup quota), and the
	 * decoder pools follow them (host_shape.hpp); counting into one table does not depend on the number */
	m_plan = ingest_plan(std::max(1u, m_opt.threads), granted_cpus());
	if (m_opt.threads > 1) m_opt.threads = std::max(2u, std::min(m_opt.threads, std::max(m_plan.feeders, 2u)));   /* 2 at least: keeps the lane path (and its tests) on a 1-CPU grant */
	if (m_opt.devices.empty()) m_opt.devices.push_back(m_opt.device);
	m_ctxDevice = m_opt.devices;                          /* one context per LISTED device: `-g 0,0` = two contexts on device 0, merged on the device (ntsm_allreduce) */
	Lap lap;
	const bool lanes = lanesPossible();
	/* A caller with a say about the site set hears it before any device is touched: the sites are loaded first (their
	 * warnings held back until the run is known to go on), and only then do the side threads below start. */
	bool loaded = false;
	if (check) {
		std::ostringstream warnings;
		if (!m_sites.load(m_opt.snp, m_opt.k, m_opt.dupes, warnings)) quit("file " + m_opt.snp + " cannot be opened");
		const std::string refusal = check(m_sites);
		if (!refusal.empty()) quit(refusal);
		std::cerr << warnings.str();
		loaded = true;
	}
	/* Side threads, one per device, prepare everything that does not depend on the sites while this thread parses
	 * them: runtime + device context, the three streams of a context, the pinned staging pool (first device),
	 * the two streams its lanes share.  They are joined when the first batch is about to be staged (computeCounts). */
	{
		const uint64_t slot = Feeder::slot_bytes(m_opt, false), lane_slot = Feeder::slot_bytes(m_opt, true);
		const uint64_t pool_bytes = lanes ? (uint64_t) m_opt.threads * 2 * ((m_opt.pack ? lane_slot * 3 / 8 : lane_slot) + 8192)   /* packed lanes pin 3/8 byte per position */
		                                  : 2 * (slot + 8192 + (slot / 64 + 16) * 8 + 8192);
		const int lanes_per_dev = lanes ? (int) ((m_opt.threads + m_ctxDevice.size() - 1) / m_ctxDevice.size()) : 0;
		for (size_t i = 0; i < m_ctxDevice.size(); ++i) {
			const int d = m_ctxDevice[i];
			const bool first = i == 0;
			m_prep.emplace_back([d, first, pool_bytes, lanes_per_dev]() {
				if (ntsm_warmup(d, lanes_per_dev ? 6 : 4) != NTSM_OK) return;   /* a context's 4 streams (two slots, resident, copy) + its 2 lane streams; ntsm_create reports failures */
				if (first) (void) ntsm_staging_pool(pool_bytes);
			});
		}
	}
	/* the first input file starts being parsed now, into ordinary memory (early_ingest.hpp): -t N, no -m, no -vvv; not where
	 * several big .gz inputs are read side by side (computeCounts), the first one included */
	if (m_opt.early && m_opt.pack && lanes && !m_opt.inputs.empty() && !sideBySide(m_opt.inputs, m_opt.threads)) {
		/* fewer than later, the start-up has threads of its own -- but the stream keeps these decoders to its end, also behind
		 * the hand-over: 8 / 10 / 12 / 14 / 16 of them take the 12.6 GB file through in 1.29 / 1.14 / 1.00 / 0.91 / 0.94 s
		 * (medians of five, one box, interleaved: profiles/r04_gz3/decoders_ab.txt) */
		const unsigned n_dec = m_opt.gz_decoders ? m_opt.gz_decoders : m_plan.early_decoders;
		const uint64_t chunk_pos = Feeder::slot_bytes(m_opt, true) & ~31ull;
		/* 1.5 GiB of packed reads at most (4 Gbases): a gzip stream is handed over when the context is
		 * there, so the chunks only ever hold what was parsed during the start-up -- 0.6 GB for the 12.6 GB file at 12 GB/s
		 * of text and 0.25 s; a slower start-up makes the parsers wait, not the host swap */
		const size_t max_chunks = (size_t) std::max<uint64_t>(4 * parsers(), (3ull << 29) / (chunk_pos * 3 / 8 + 1));
		m_early.reset(new EarlyIngest(m_opt.inputs[0], (unsigned) parsers(), n_dec, blockBytes(), m_opt.gz_parallel_min_bytes, chunk_pos, max_chunks, m_opt.early_kinds));
		if (!m_early->taken()) m_early.reset();
	}
	if (!loaded && !m_sites.load(m_opt.snp, m_opt.k, m_opt.dupes, std::cerr)) quit("file " + m_opt.snp + " cannot be opened");   /* :493-499 */
	const double t_sites = lap();
	if (m_opt.verbose) std::cerr << "Opening " << m_opt.snp << std::endl;
	m_maxCounts = threshold_from((double) m_sites.n_distinct(), m_opt.covThresh);
	if (m_sites.keys.size() > 0xFFFFFFFFull) quit("ntsmCount: too many site k-mers");
	/* one context per listed device; with -m everything runs on the first one */
	if (m_maxCounts != 0) m_ctxDevice.resize(1);
	m_ctx.assign(m_ctxDevice.size(), nullptr);
	std::vector<int> rcs(m_ctxDevice.size(), 0);
	std::vector<std::thread> mk;
	for (size_t i = 0; i < m_ctxDevice.size(); ++i)
		mk.emplace_back([&, i]() {
			rcs[i] = ntsm_create(&m_ctx[i], m_ctxDevice[i], (int) m_opt.k, m_sites.keys.data(), (uint32_t) m_sites.keys.size(),
					NTSM_KEYS_CANONICAL, m_maxCounts);
		});
	for (auto &t : mk) t.join();
	/* several devices end with one RCCL SUM (fetchResults): bind the library now, so that a host without it hears
	 * about it before the work, not after (the host-side sum of fetchResults takes over in that case) */
	const size_t n_distinct_devices = std::set<int>(m_ctxDevice.begin(), m_ctxDevice.end()).size();   /* contexts on ONE device are merged without RCCL */
	if (n_distinct_devices > 1 && ntsm_rccl_probe() != NTSM_OK)
		std::cerr << "ntsmCount: warning: RCCL could not be loaded; the devices' counts will be summed on the host" << std::endl;
	if (m_opt.phase_times)
		std::cerr << "[phase] sites parsed " << t_sites << " s, contexts (tables + upload) " << lap() << " s" << std::endl;
	for (const int rc : rcs)
		if (rc)
			quit(std::string("ntsmCount: cannot create GPU context: ") + ntsm_strerror(rc)
			     + (rc == NTSM_ERR_HIP ? " (hipError " + std::to_string(ntsm_last_hip_error()) + ")" : ""));
	if (m_opt.debug_kernel >= 0)
		for (auto *ctx : m_ctx) {
			const int rc = ntsm_set_kernel(ctx, m_opt.debug_kernel);
			if (rc) quit("ntsmCount: --debug-kernel " + std::to_string(m_opt.debug_kernel) + ": " + ntsm_strerror(rc));
		}
}

FingerPrint::~FingerPrint()
{
	joinPrep();
	for (auto &t : m_retire) if (t.joinable()) t.join();
	m_main.reset();
	m_lanes.clear();
	for (ntsm_ctx *c : m_ctx) ntsm_destroy(c);
}

void FingerPrint::joinPrep()
{
	for (auto &t : m_prep) if (t.joinable()) t.join();
	m_prep.clear();
}

Feeder &FingerPrint::feederFor(size_t t)
{
	if (!m_lanes[t]) {
		m_lanes[t].reset(new Feeder(m_opt, m_ctx[t % m_ctx.size()], 0, true));   /* threads round-robin over the contexts */
	}
	return *m_lanes[t];
}

/* the feeders [first, first + n), one per parsing thread */
std::vector<Feeder *> FingerPrint::openFeeders(size_t first, size_t n)
{
	std::vector<std::thread> mk;                             /* lanes (pinned staging) are allocated in parallel */
	for (size_t t = first; t < first + n; ++t) mk.emplace_back([this, t]() { (void) feederFor(t); });
	for (auto &th : mk) th.join();
	std::vector<Feeder *> feeders;
	for (size_t t = first; t < first + n; ++t) feeders.push_back(&feederFor(t));
	return feeders;
}

void FingerPrint::closeLanes()
{
	for (auto &f : m_lanes) if (f) f->finish();
	m_lanes.clear();
}

void FingerPrint::feedReads(Feeder &f, SeqReader &rd)
{
	int64_t l = rd.next();
	while (l >= 0 && !f.earlyTerm()) {
		f.feedRead(rd.seq_data(), (uint64_t) l);
		l = rd.next();
		/* -vvv: "Current Total" after every 1,000,000th read (src/FingerPrint.hpp:70-78: m_totalReads only advances at this
		 * verbosity, after the read has been processed and the next one fetched).  The totals have to be those after exactly
		 * that many reads, so the batch is submitted and waited for here -- a debugging verbosity, run on one thread. */
		if (m_opt.verbose > 2 && (++m_totalReads % 1000000) == 0) f.progressLine(m_totalReads);
	}
}

void FingerPrint::feedFile(Feeder &f, const std::string &fn, uint64_t offset)
{
	SeqReader rd;
	if (!rd.open(fn, offset)) fatal("file " + fn + " cannot be opened");
	if (m_opt.verbose && offset == 0) say("Opening " + fn);
	feedReads(f, rd);
}

void FingerPrint::computeCounts(const std::vector<std::string> &filenames)
{
	/* The reference runs this loop under `omp parallel for` over files (:47) with ONE shared m_counts and atomic
	 * increments: -t N means N files at a time.  Same here when no -m threshold is armed: N host threads, each
	 * with its own producer lane (pinned staging + stream) of the SAME GPU context, pull work from a shared
	 * index; the counts meet in the context's table (one context per device with -g a,b: summed at the end).
	 * With -m the reference's parallel schedule is a race; the only defined semantics is
	 * argv order on one thread, which is what an armed run always uses. */
	/* -vvv prints running totals at exact read counts (Feeder::progressLine): one ordered stream as well.
	 * Not lanesPossible(): whether -m arms a threshold is known only now that the sites are loaded. */
	const size_t want = m_maxCounts != 0 || m_opt.verbose > 2 ? 1 : std::max(1u, m_opt.threads);
	shareDecoders(want, filenames.size());
	if (!m_prep.empty()) {
		Lap lap;
		joinPrep();
		if (m_opt.phase_times) std::cerr << "[phase] waited " << lap() << " s for streams + pinned pool" << std::endl;
	}
	if (want <= 1) {
		countOrdered(filenames);
		return;
	}
	m_lanes.resize(want);
	std::vector<std::string> todo(filenames);
	if (m_early && !todo.empty() && todo[0] == m_opt.inputs[0]) {
		drainEarly();                                            /* the first file has been in the works since the process started */
		todo.erase(todo.begin());
	}
	retireLater(std::move(m_early));
	todo = countBlockParallel(todo);
	if (!getenv("NTSM_ZLIB_ONLY")) todo = countBigGzip(todo);
	countOnePerThread(todo);
	Lap lap;
	closeLanes();
	if (m_opt.phase_times) std::cerr << "[phase] lanes closed in " << lap() << " s" << std::endl;
}

/* -m, -vvv, -t 1: argv order through the context's own slots */
void FingerPrint::countOrdered(const std::vector<std::string> &files)
{
	if (!m_main) m_main.reset(new Feeder(m_opt, m_ctx[0], m_maxCounts, false));
	for (const std::string &fn : files) feedFile(*m_main, fn);    /* after a stop: still opened, nothing counted (:66) */
	m_main->flush();
	if (m_main->earlyTerm()) std::cerr << "Reached desired (-m) threshold" << std::endl;   /* :84-86 */
}

/* Big plain FASTQ files are cut into blocks and parsed by all threads (parallel_fastq.hpp); files that are not
 * eligible (gzip, FASTA, wrapped or CR lines, small) are returned: they are taken whole. */
std::vector<std::string> FingerPrint::countBlockParallel(const std::vector<std::string> &files)
{
	std::vector<std::string> rest;
	for (const std::string &fn : files) {
		ParallelFastq pf;
		/* a block's sequences + terminators (at most half its bytes: a record is header + SEQ + '+' line + QUAL) must
		 * fit one lane slot, so that no thread waits for its predecessor in the middle of a block */
		if (!pf.open(fn, blockBytes())) { rest.push_back(fn); continue; }
		Lap lap;
		/* One plain FASTQ is parsed by at most 16 threads however many -t asks for (host_shape.hpp's largest row): measured
		 * on a 256-thread host, 16 feeders parse + count at 50 Gbases/s, 32 at 40, 64 at 25 (they queue up on the runtime's
		 * submission path and on the memory of the socket that holds the page cache); the result does not depend on the number. */
		if (m_opt.verbose) std::cerr << "Opening " << fn << "\n" << "block-parallel: " << pf.n_blocks() << " blocks, " << parsers() << " threads" << std::endl;
		const std::vector<Feeder *> sinks = openFeeders(0, parsers());
		const double t_lanes = lap();
		const ParallelFastq::Result r = pf.run(sinks);
		const double t_parse = lap();
		if (!r.complete) {                                      /* the rest of the file is not plain 4-line FASTQ */
			if (m_opt.verbose) std::cerr << "block-parallel: sequential from byte " << r.resume << std::endl;
			feedFile(*sinks[0], fn, r.resume);
			sinks[0]->flush();
		}
		if (m_opt.phase_times)
			std::cerr << "[phase] " << fn << ": lanes " << t_lanes << " s, parse+count " << t_parse << " s (" << r.records << " records in parallel)" << std::endl;
	}
	return rest;
}

/* A big gzip file (plain or BGZF) is inflated by a pool of decoder threads (gz_stream.hpp) and the text is parsed piece-
 * parallel by the same feeders (parallel_gz_fastq.hpp), one file after the other; small ones, and all of them where
 * they are many (sideBySide), are returned: they stay one thread per file. */
std::vector<std::string> FingerPrint::countBigGzip(const std::vector<std::string> &files)
{
	std::vector<std::string> rest;
	const bool side_by_side = sideBySide(files, m_opt.threads);
	for (const std::string &fn : files) {
		if (side_by_side || !big_gzip_input(fn, m_opt.gz_parallel_min_bytes)) { rest.push_back(fn); continue; }
		/* decoder threads: as many as the grant has CPUs, at most twice the feeders (host_shape.hpp) -- measured under a 16-CPU
		 * quota on a 2 x 64-core host (6.3 GB of text, 1 MiB chunks, 16 feeders): 8 / 12 / 16 / 20 / 24 / 32 decoders inflate +
		 * parse + count in 0.74 / 0.51 / 0.42 / 0.48 / 0.47 / 0.52 s */
		unsigned n_dec = (unsigned) std::max<size_t>(1, std::min<size_t>(m_plan.decoders, 2 * parsers()));
		if (m_opt.gz_decoders) n_dec = m_opt.gz_decoders;
		GzStream::set_decoder_threads(n_dec);
		std::unique_ptr<GzStream> gz(new GzStream());
		if (!gz->open(fn)) { rest.push_back(fn); continue; }
		if (m_opt.verbose) std::cerr << "Opening " << fn << "\n" << "parallel gzip: " << n_dec << " decoder threads, " << parsers() << " parsing threads" << std::endl;
		countGzStream(std::move(gz), fn, 0, parsers());
	}
	shareDecoders(m_opt.threads, rest.size());
	return rest;
}

/* everything else: the threads pull whole files from a shared index */
void FingerPrint::countOnePerThread(const std::vector<std::string> &files)
{
	std::atomic<size_t> next(0);
	std::vector<std::thread> pool;
	for (size_t t = 0; t < std::min<size_t>(m_opt.threads, files.size()); ++t)
		pool.emplace_back([&, t]() {
			Feeder &f = feederFor(t);
			for (size_t i = next++; i < files.size(); i = next++) feedFile(f, files[i]);
			f.flush();
		});
	for (auto &th : pool) th.join();
}

/* An open gzip stream nobody has read from yet (or that stands at a record boundary): its pieces are parsed by the feeders
 * in parallel (parallel_gz_fastq.hpp), what they cannot take by the sequential reader on the same object. */
void FingerPrint::countGzStream(std::unique_ptr<GzStream> gz, const std::string &fn, size_t first, size_t n_par)
{
	Lap lap;
	const std::vector<Feeder *> sinks = openFeeders(first, n_par);
	const double t_lanes = lap();
	ParallelGzFastq pg(gz.get());
	const ParallelGzFastq::Result r = pg.run(sinks);
	const double t_parse = lap();
	if (!r.complete) {                                      /* what is left is not plain 4-line FASTQ (or the last record has no newline) */
		if (m_opt.verbose) std::cerr << "parallel gzip: sequential after " << r.records << " records" << std::endl;
		SeqReader rd;
		if (rd.open_stream(std::move(gz))) feedReads(*sinks[0], rd);
		sinks[0]->flush();
	}
	if (m_opt.phase_times) {
		uint64_t ps[2];
		GzStream::last_parallel_stats(ps);
		std::cerr << "[phase] " << fn << ": lanes " << t_lanes << " s, inflate+parse+count " << t_parse << " s (" << r.records << " records in "
		          << r.pieces << " pieces in parallel, " << ps[0] << " chunks spliced, " << ps[1] << " dropped), rest " << lap() << " s" << std::endl;
	}
	retireLater(std::move(gz));                                 /* null if the sequential reader took it over (and closed it) */
}

void FingerPrint::drainEarly()
{
	Lap lap;
	const size_t n_par = parsers();
	if (m_opt.verbose) std::cerr << "Opening " << m_opt.inputs[0] << "\n" << "early ingest (" << m_early->how() << "): parsed while the sites were loading" << std::endl;
	const std::vector<Feeder *> feeders = openFeeders(0, n_par);
	const double t_lanes = lap();
	/* The consumers are there.  A gzip stream stops being parsed into chunks at the next record boundary: a quarter of the
	 * feeders submit the chunks that are waiting (a copy into a lane each) while the others parse the rest of the stream
	 * straight into their lanes -- one copy and gigabytes of first-touched memory less than taking the whole file through
	 * the chunks (14.3 -> 13.x CPU-seconds for the 12.6 GB file under the pod's 16-CPU quota). */
	const size_t n_drain = n_par >= 8 ? n_par / 4 : n_par;
	m_early->hand_over();
	std::atomic<uint64_t> chunks(0);
	std::vector<std::thread> pool;
	for (size_t t = 0; t < n_drain; ++t)
		pool.emplace_back([this, f = feeders[t], &chunks]() {
			std::unique_ptr<PackedChunk> c;
			while (m_early->next(&c)) {
				f->submitChunk(*c);
				m_early->recycle(std::move(c));
				++chunks;
			}
		});
	std::unique_ptr<GzStream> rest = m_early->release_stream();   /* waits for the parsers to finish what they hold */
	const double t_handed = lap();
	if (rest && !m_early->failed()) {
		if (n_drain < n_par) {
			countGzStream(std::move(rest), m_opt.inputs[0], n_drain, n_par - n_drain);
			for (auto &th : pool) th.join();
		} else {                                                /* few threads: one after the other on the same lanes */
			for (auto &th : pool) th.join();
			countGzStream(std::move(rest), m_opt.inputs[0], 0, n_par);
		}
		pool.clear();
	}
	for (auto &th : pool) th.join();
	if (m_early->failed()) {                                    /* reads were lost (no memory for a chunk, the file's rest unreadable): never print counts */
		fatal("ntsmCount: " + m_early->error());                /* the message names its own cause (allocation or I/O) */
	}
	if (m_opt.phase_times)
		std::cerr << "[phase] " << m_opt.inputs[0] << ": early ingest (" << m_early->how() << ") parsed " << m_early->records() << " records ("
		          << m_early->parallel_records() << " in parallel) in " << m_early->parse_seconds() << " s beside the start-up; lanes "
		          << t_lanes << " s, " << chunks.load() << " chunks submitted, the stream handed over " << t_handed
		          << " s and everything done " << t_handed + lap() << " s after the context was ready" << std::endl;
}

void FingerPrint::fetchResults()
{
	if (m_fetched) return;
	m_main.reset();
	closeLanes();
	m_counts.assign(m_sites.keys.size(), 0);
	m_totals = ntsm_totals();
	/* Several devices (-g a,b,...): one RCCL SUM of the dense per-k-mer vectors + totals over xGMI, after which every
	 * context reports the job-wide result -- SUM, not MAX: the per-site maxima are taken from the summed counts, which is
	 * what one reference run over all reads computes (src/FingerPrint.hpp:281-294). */
	int rc = m_ctx.size() > 1 ? ntsm_allreduce(m_ctx.data(), (int) m_ctx.size()) : NTSM_OK;
	if (rc == NTSM_ERR_RCCL) {
		/* RCCL missing or failing must not cost a finished run its result: every context still holds its own counts
		 * (a failed ntsm_allreduce imports nothing), so they are summed here instead -- same SUM, over PCIe. */
		std::cerr << "ntsmCount: RCCL unavailable (" << ntsm_strerror(rc) << "), summing the " << m_ctx.size()
		          << " devices' counts on the host" << std::endl;
		std::vector<uint64_t> part(m_counts.size());
		rc = NTSM_OK;
		for (size_t d = 0; d < m_ctx.size() && rc == 0; ++d) {
			ntsm_totals t;
			rc = ntsm_sync(m_ctx[d], &t);
			if (rc == 0) rc = ntsm_counts(m_ctx[d], part.data());
			if (rc) break;
			for (size_t i = 0; i < part.size(); ++i) m_counts[i] += part[i];
			m_totals.total_kmers += t.total_kmers;
			m_totals.total_hits += t.total_hits;
			m_totals.total_bases += t.total_bases;
			m_totals.reads_consumed += t.reads_consumed;
			m_totals.early_stop |= t.early_stop;
		}
		if (rc == 0) { m_fetched = true; return; }
	}
	if (rc == 0) rc = ntsm_sync(m_ctx[0], &m_totals);
	if (rc == 0) rc = ntsm_counts(m_ctx[0], m_counts.data());
	if (rc) {
		fatal(std::string("ntsmCount: cannot fetch counts: ") + ntsm_strerror(rc));
	}
	m_fetched = true;
}

void FingerPrint::attachSites(const uint32_t *offsets, const uint32_t *kmer_ix, uint32_t n_sites)
{
	const int rc = ntsm_sites_attach(m_ctx[0], offsets, kmer_ix, n_sites);
	if (rc) fatal(std::string("ntsmCount: cannot upload the site lists: ") + ntsm_strerror(rc));
}

void FingerPrint::nextSample()
{
	m_main.reset();
	closeLanes();
	for (auto &t : m_retire) if (t.joinable()) t.join();
	m_retire.clear();
	for (ntsm_ctx *c : m_ctx) {
		int rc = ntsm_reset(c);
		if (rc == 0 && m_maxCounts != 0) rc = ntsm_set_max_hits(c, m_maxCounts, 1);
		if (rc) fatal(std::string("ntsmCount: cannot reset a GPU context: ") + ntsm_strerror(rc));
	}
	m_totals = ntsm_totals();
	m_totalReads = 0;
	m_fetched = false;
	m_counts.clear();
}

FingerPrint::SiteRecord FingerPrint::siteRecord()
{
	SiteRecord r;
	m_main.reset();
	closeLanes();
	Lap lap;
	/* several contexts: the same SUM as fetchResults, after which context [0] holds the job-wide vector and totals */
	int rc = m_ctx.size() > 1 ? ntsm_allreduce(m_ctx.data(), (int) m_ctx.size()) : NTSM_OK;
	if (rc == 0) rc = ntsm_sync(m_ctx[0], &r.run);
	r.wait_s = lap();
	r.counts.assign(2 * m_sites.ids.size(), 0);
	r.sums.assign(2 * m_sites.ids.size(), 0);
	if (rc == 0 && m_opt.phase_times) rc = ntsm_set_timing(m_ctx[0], 1);
	if (rc == 0) rc = ntsm_sites_reduce(m_ctx[0], r.counts.data(), r.sums.data(), &r.sites);
	if (rc == 0 && m_opt.phase_times) {
		rc = ntsm_sites_kernel_ms(m_ctx[0], &r.kernel_ms);
		if (rc == 0) rc = ntsm_set_timing(m_ctx[0], 0);
	}
	r.reduce_s = lap();
	if (rc) fatal(std::string("ntsmCount: cannot fetch the site record: ") + ntsm_strerror(rc));
	return r;
}

void FingerPrint::printOptionalHeader(std::ostream &out) const
{
	const_cast<FingerPrint *>(this)->fetchResults();
	print_optional_header(out, m_totals.total_kmers, m_opt.k);
}

void FingerPrint::printCountsMax(std::ostream &out) const
{
	const_cast<FingerPrint *>(this)->fetchResults();
	if (!print_counts_max(out, m_sites, m_counts)) {
		/* the reference's m_counts.at()/vector::at() throws here and the process aborts (exit 134) */
		out.flush();
		std::cerr << "terminate called after throwing an instance of 'std::out_of_range'\n"
		             "  what():  Couldn't find key.\n"
		             "ntsmCount: the sites file has duplicate k-mers (rerun with -d) or an odd number of records"
		          << std::endl;
		abort();
	}
}

std::string FingerPrint::printInfoSummary()
{
	fetchResults();
	const std::string s = info_summary(m_sites, m_counts, m_totals.total_bases, m_totals.total_kmers, m_totals.total_hits);
	if (!m_opt.summary.empty()) {
		std::ofstream fh(m_opt.summary);
		fh << s;
	}
	const double covPer = double(sites_covered(m_sites, m_counts)) / double(m_sites.ref.size());
	if (covPer < m_opt.siteCovThreshold)
		std::cerr << "Warning: site coverage is : " << covPer
		          << "(<75%). Data may be sorted or sparse along the genome. Any PCA projection may be inaccurate."
		          << std::endl;
	return s;
}

} // namespace ntsm
