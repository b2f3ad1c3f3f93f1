/*
 * ntsm_eval_main.cpp -- host mirror of the reference's ntsmEval (src/ntSeqMatchEval.cpp:86-349, src/CompareCounts.hpp):
 * same flags, same stdout bytes; the scoring is the HIP library's (include/ntsm_eval_hip.h).  This file holds the runs and
 * main; the command line -- options, the table of runs, the first refusal -- is eval_cli_args.hpp, the text of the rows is
 * eval_cli_rows.hpp.  Each run is one function here, named in its row of kRunTable, and its comment says what it prints:
 *   FILES... [-p ROT -n NORM] [-e FILE [-o]]   runFiles: ntsm_eval_pairs, or ntsm_eval_open / _project / _candidates / _score_pairs
 * This build only (DESIGN.md sections 9.1-9.9):
 *   --pack STORE FILES...              packStore: no GPU
 *   --against STORE FILES...           scoreAgainst: ntsm_eval_pairs, ntsm_eval_cross
 *   --index STORE -p ROT -n NORM       buildIndex: ntsm_eval_project_store
 *   --near STORE FILES...              searchNear: ntsm_eval_cross_candidates, then routeAndScore
 *   --within STORE                     scoreWithin: ntsm_eval_within_open / _rows in walkBands
 *   --within-near STORE                searchWithin: ntsm_eval_cross_candidates, then routeAndScore
 *   --between STORE_A STORE_B          scoreBetween: ntsm_eval_between_open / _rows in walkBands
 *   --between-near STORE_A STORE_B     searchBetween: ntsm_eval_between_candidates, then routeAndScore
 *   --qc STORE [--sites-out FILE]      qcStore: ntsm_eval_store_profile, ntsm_eval_project_store
 *   --contam STORE [--samples-out FILE]   contamStore: ntsm_eval_contam_open / _rows in walkBands
 *   --trios STORE [--ped FILE]         trioStore: ntsm_eval_trio_open / _duos / _score under eval_trio.hpp's runs
 *   --ld STORE [--ld-prune FILE]       ldStore: ntsm_eval_ld_open / _select under eval_ld.hpp's walk
 * Not built, and refused: -b (the debug ground-truth mode) and -p without a normalization file (the reference dies in an
 * assert).  Pinned to the reference: stdout equals, byte for byte, that of the unmodified scoring class
 * (oracle/ref_eval_driver.cpp -> oracle/_ref/ref_ntsmEval -t 1) and its recordings, tests/test_eval_reference.py (DESIGN.md
 * section 9); the command line to its own recordings, tests/test_eval_cli_args.py.
 */
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <iostream>
#include <sstream>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../../include/ntsm_eval_hip.h"
#include "cli.hpp"
#include "eval_between.hpp"
#include "eval_cli_args.hpp"
#include "eval_cli_rows.hpp"
#include "eval_contam.hpp"
#include "eval_index.hpp"
#include "eval_ld.hpp"
#include "eval_qc.hpp"
#include "eval_store.hpp"
#include "eval_trio.hpp"
#include "eval_within.hpp"

namespace {

/* src/CompareCounts.hpp:30-114: the first file fixes loci and distinct counts, then every file fills its row.  Under
 * --against the store has fixed them (c.locus, c.distinct and `index` come filled) and a locus it lacks is a refusal.  The
 * reading of one file is eval_store.hpp's, shared with --pack. */
void load(Counts &c, ntsm::eval_store::LocusIndex index = {}, bool fromStore = false)
{
	if (!fromStore) ntsm::eval_store::read_locus_table(c.files.at(0), index, c.locus, c.distinct);
	const size_t n = c.files.size(), m = c.nSites();
	c.counts.assign(n * m * 2, 0u);
	c.sums.assign(n * m * 2, 0u);
	c.rawTotal.assign(n, 0);
	c.total.assign(n, 0);
	c.kmerSize.assign(n, 0);
	for (size_t i = 0; i < n; ++i) {
		ntsm::eval_store::Scalars sc;
		ntsm::eval_store::parse_counts_file(c.files[i], index, c.counts.data() + i * m * 2, c.sums.data() + i * m * 2, sc, fromStore);
		c.rawTotal[i] = sc.raw_total;
		c.total[i] = sc.total;
		c.kmerSize[i] = sc.kmer_size;
	}
}

/* projectPCs' input files (:120-165): norm values (one long double per line, 0 where a line does not parse) and the first
 * opt.dim components of the rotation rows, matched to sites by position.  Stops the program where the reference asserts
 * (dim > components, rows != norm values) and where it would read past its arrays (fewer values than sites). */
void loadPCA(const Opt &opt, size_t nSites, std::vector<long double> &norm, std::vector<long double> &rot /*[dim][nSites]*/)
{
	if (opt.verbose > 0) std::cerr << "Projecting samples onto PCA" << std::endl;
	std::vector<long double> normVals;
	{
		std::ifstream fh(opt.norm);
		std::string line;
		while (fh.is_open() && std::getline(fh, line)) {
			std::stringstream ss(line);
			long double value = 0;
			ss >> value;
			normVals.push_back(value);
		}
	}
	unsigned compNum = 0;
	std::ifstream fh(opt.pca);
	std::string line;
	std::getline(fh, line);
	{
		std::stringstream ss(line);
		std::string val;
		ss >> val;
		while (ss >> val) ++compNum;
	}
	if (opt.verbose > 0) std::cerr << "Detected " << compNum << " components for " << normVals.size() << " sites" << std::endl;
	if (opt.dim > compNum) {                                 /* assert(opt::dim <= compNum), :153 */
		std::cerr << PROGRAM ": -d " << opt.dim << " exceeds the " << compNum << " components of " << opt.pca << std::endl;
		abort();
	}
	std::vector<std::vector<long double>> rows;             /* [row][dim] */
	while (std::getline(fh, line)) {
		std::stringstream ss(line);
		std::string rsID;
		ss >> rsID;
		std::vector<long double> v(opt.dim, 0.0L);
		for (unsigned d = 0; d < opt.dim; ++d) ss >> v[d];  /* after a failed read the rest stay 0, as in the reference */
		rows.push_back(std::move(v));
	}
	if (rows.size() != normVals.size()) {                   /* assert(index == normVals.size()), :165 */
		std::cerr << PROGRAM ": " << rows.size() << " rotation rows but " << normVals.size() << " normalization values" << std::endl;
		abort();
	}
	if (normVals.size() < nSites) {
		std::cerr << "Error: " << normVals.size() << " normalization values and rotation rows for " << nSites
		          << " sites; a PCA search with fewer values than sites is not part of this build" << std::endl;
		exit(EXIT_FAILURE);
	}
	norm.assign(normVals.begin(), normVals.begin() + nSites);
	rot.assign((size_t) opt.dim * nSites, 0.0L);
	for (size_t j = 0; j < nSites; ++j)
		for (unsigned d = 0; d < opt.dim; ++d) rot[(size_t) d * nSites + j] = rows[j][d];
}

int gpuFail(const char *what, int rc)
{
	std::cerr << PROGRAM ": " << what << " on the GPU failed (" << rc << "); there is no CPU path" << std::endl;
	return 3;
}

template <typename H, void (*Close)(H *)> struct Handle {   /* closes the library session it holds when its scope ends */
	H *h = nullptr;
	~Handle() { if (h) Close(h); }
};
typedef Handle<ntsm_eval_session, ntsm_eval_close> Session;
typedef Handle<ntsm_eval_within_session, ntsm_eval_within_close> WithinSession;
typedef Handle<ntsm_eval_between_session, ntsm_eval_between_close> BetweenSession;
typedef Handle<ntsm_eval_contam_session, ntsm_eval_contam_close> ContamSession;
typedef Handle<ntsm_eval_trio_session, ntsm_eval_trio_close> TrioSession;
typedef Handle<ntsm_eval_ld_session, ntsm_eval_ld_close> LdSession;

typedef std::chrono::steady_clock Clock;
double msSince(Clock::time_point t) { return std::chrono::duration<double, std::milli>(Clock::now() - t).count(); }

void printTime(Clock::time_point t0)         /* the last line of every run's stderr */
{
	std::cerr << "Time: " << std::chrono::duration<double>(Clock::now() - t0).count() << " s" << std::endl;
}

/* The refusals of a run that need its inputs: `open` maps, reads and checks them and throws the refusal (or a number that
 * does not parse); nothing has been written and no GPU work done.  Returns the ms it took: the map (+load) figure of -vv. */
template <typename Open> double openOrRefuse(Open open)
{
	const auto t = Clock::now();
	try {
		open();
	} catch (const std::exception &e) {
		ntsm::refuse(e.what());
	}
	return msSince(t);
}

/* A table a run writes beside its stdout (--sites-out, --samples-out, --ld-prune): opened before any GPU work and without
 * touching what it holds; a file this run made is removed again unless the table gets written. */
struct OutFile {
	std::string path;
	int fd = -1;
	bool created = false, written = false;
	~OutFile()
	{
		if (fd >= 0) close(fd);
		if (created && !written) unlink(path.c_str());
	}
	void open(const std::string &name)       /* throws the refusal */
	{
		path = name;
		struct stat sb;
		created = stat(name.c_str(), &sb) != 0;
		fd = ::open(name.c_str(), O_WRONLY | O_CREAT, 0644);
		if (fd < 0) throw ntsm::eval_store::Error("cannot write " + name);
	}
	bool write(const std::string &text)      /* false, its message printed: exit status 1 */
	{
		written = ftruncate(fd, 0) == 0 && ntsm::eval_store::write_all(fd, text.data(), text.size(), 0);
		if (!written) std::cerr << PROGRAM ": cannot write " << path << std::endl;
		return written;
	}
};

/* a library call that reports its kernel ms, timed: `call(&ms)`; both figures are added to sum */
struct CallTimes { double kernelMs = 0, callMs = 0; };
template <typename Call> int timedCall(CallTimes &sum, Call call)
{
	const auto t = Clock::now();
	double ms = 0;
	const int r = call(&ms);
	sum.kernelMs += ms; sum.callMs += msSince(t);
	return r;
}

/* projectPCs (:166-211) on the device: cloud [n][dim] */
int project(const Counts &c, const Opt &opt, ntsm_eval_session *h, const std::vector<long double> &norm, const std::vector<long double> &rot,
		std::vector<double> &cloud)
{
	cloud.assign(c.files.size() * (size_t) opt.dim, 0.0);
	double ms = 0;
	const int rc = ntsm_eval_project(h, norm.data(), rot.data(), opt.dim, cloud.data(), &ms);
	if (rc) return gpuFail("projection", rc);
	if (opt.verbose > 2)
		for (const std::string &f : c.files) std::cerr << "Normalizing " << f << std::endl;
	if (opt.verbose > 1) std::cerr << "projection kernel: " << ms << " ms" << std::endl << "Finished Normalization " << std::endl;
	return 0;
}

/* the squared search radius of every sample (:297-305; pow(x, 2) = x * x); DBL_MAX = search all */
std::vector<double> searchRadii(std::vector<Genotype> &g, size_t m, const Opt &opt)
{
	std::vector<double> radius(g.size());
	for (size_t i = 0; i < g.size(); ++i) {
		const double propMissing = double(g[i].miss) / double(m);
		g[i].radius = DBL_MAX;
		if (g[i].errorRate < opt.pcErrorThresh && propMissing < opt.pcMissSite1) g[i].radius = opt.pcSearchRadius1 * opt.pcSearchRadius1;
		else if (propMissing < opt.pcMissSite2) g[i].radius = opt.pcSearchRadius2 * opt.pcSearchRadius2;
		radius[i] = g[i].radius;
	}
	return radius;
}

/* A candidate list and the two calls that fetch it: ask the size with no room, allocate, ask again.  `call` is the library's
 * search with its inputs bound: (pi, pk, dist, capacity, &n_pairs, &kernel_ms). */
struct Candidates {
	std::vector<uint32_t> pi, pk;
	std::vector<double> dist;
	double kernelMs = 0;
	int search(const std::function<int(uint32_t *, uint32_t *, double *, uint64_t, uint64_t *, double *)> &call)
	{
		uint64_t np = 0;
		int rc = call(nullptr, nullptr, nullptr, 0, &np, &kernelMs);
		if (rc && rc != NTSM_EVAL_E_CAPACITY) return gpuFail("candidate search", rc);
		pi.resize(np); pk.resize(np); dist.resize(np);
		if (np && (rc = call(pi.data(), pk.data(), dist.data(), np, &np, &kernelMs)) != 0) return gpuFail("candidate search", rc);
		return 0;
	}
};

/* computeScorePCA (:285-398), the one-thread order of its rows */
int scorePCA(const Counts &c, std::vector<Genotype> &g, const Opt &opt, ntsm_eval_session *h, const std::vector<double> &cloud)
{
	if (opt.verbose > 1) std::cerr << "Generating kd-tree" << std::endl;
	const std::vector<double> radius = searchRadii(g, c.nSites(), opt);
	if (opt.verbose > 1) std::cerr << "Starting Score Computation with PCA" << std::endl;
	Candidates cand;
	int rc = cand.search([&](uint32_t *pi, uint32_t *pk, double *dist, uint64_t capacity, uint64_t *np, double *ms) {
		return ntsm_eval_candidates(h, cloud.data(), opt.dim, radius.data(), pi, pk, dist, capacity, np, ms);
	});
	if (rc) return rc;
	const uint64_t np = cand.pi.size();
	double msScore = 0;
	std::vector<ntsm_eval_record> rec(np);
	rc = ntsm_eval_score_pairs(h, cand.pi.data(), cand.pk.data(), np, rec.data(), &msScore);
	if (rc) return gpuFail("scoring", rc);
	if (opt.verbose > 1) std::cerr << "search kernels: " << cand.kernelMs << " ms, scoring kernel: " << msScore << " ms for " << np << " pairs" << std::endl;
	printCandidates(c, g, opt, cand.pi, cand.pk, cand.dist, rec.data());
	return 0;
}

/* --pack STORE FILES...: no GPU */
int packStore(Opt &opt, const Positionals &files)
{
	openOrRefuse([&] {                                       /* on a refusal the store is as it was */
		const uint64_t n = ntsm::eval_store::pack(opt.store, files);
		if (opt.verbose > 0) std::cerr << "Packed " << files.size() << " files; " << opt.store << " holds " << n << " samples" << std::endl;
	});
	return 0;
}

/* What every store run opens: the mapped store, refused when it is empty or holds more samples than a run with nFiles
 * further ones numbers ("... one run scores" / "... one run projects").  With c, its locus table and distinct columns play
 * the part of the first file.  Throws the refusal. */
void openStore(const std::string &name, size_t nFiles, const char *does, ntsm::eval_store::View &store, Counts *c)
{
	namespace st = ntsm::eval_store;
	store.open(name);
	if (store.h.n_samples == 0) throw st::Error(name + " holds no samples");
	if (store.h.n_samples + nFiles > UINT32_MAX) throw st::Error(name + " holds more samples than one run " + does);
	if (!c) return;
	c->locus = store.locus;
	c->distinct.assign(store.distinct, store.distinct + 2 * (size_t) store.h.n_sites);
}

/* the store's samples as samples nq ... of a run: names, summaries from the record scalars and the given tallies.  The sites
 * are the run's (c.locus: the table of the store that openStore gave c, which under --between is not this store's). */
typedef std::function<void(uint32_t, Genotype &)> Tallies;
void appendStoreSamples(Counts &c, std::vector<Genotype> &g, const ntsm::eval_store::View &store, const Opt &opt, const Tallies &tallies)
{
	namespace st = ntsm::eval_store;
	const uint32_t nq = (uint32_t) c.files.size(), nd = (uint32_t) store.h.n_samples, m = (uint32_t) c.nSites();
	const uint64_t distinctSum = st::sum_of_pairs(c.distinct.data(), m);
	g.resize((size_t) nq + nd);
	c.files.reserve((size_t) nq + nd);
	for (uint32_t d = 0; d < nd; ++d) {
		const st::RecordHead &h = store.head(d);
		Genotype &s = g[nq + d];
		tallies(d, s);
		s.errorRate = st::error_rate(h.raw_total, h.kmer_size, h.sum_of_sums, distinctSum, opt.genomeSize);
		s.cov = double(h.total) / double(m);
		c.files.push_back(store.name(d));
	}
}

/* the tallies of store sample d as the library wrote them, geno [n][3] */
Tallies talliesOf(const std::vector<uint32_t> &geno)
{
	return [&geno](uint32_t d, Genotype &s) { setTallies(s, &geno[3 * (size_t) d]); };
}

/* --against STORE FILES...: the rows of computeScore (:591-624) over [FILES..., the store's samples] whose sample 1 is one
 * of FILES -- a prefix of that run's output.  The store's locus table and distinct columns play the part of the first file. */
int scoreAgainst(Opt &opt, const Positionals &files)
{
	const auto t0 = Clock::now();
	ntsm::eval_store::View store;
	Counts c;
	c.files = files;
	const double mapMs = openOrRefuse([&] {                  /* mapping the store and reading the query files */
		openStore(opt.store, c.files.size(), "scores", store, &c);
		if (opt.verbose > 0) std::cerr << "Reading count files" << std::endl;
		load(c, store.index(), true);
	});
	std::vector<Genotype> g = summaries(c, opt);
	const uint32_t nq = (uint32_t) c.files.size(), nd = (uint32_t) store.h.n_samples, m = store.h.n_sites;
	if (opt.verbose > 1) std::cerr << "Finished loading files. Now comparing " << nq << " samples against the " << nd << " of " << opt.store << "." << std::endl;
	std::cerr << "Performing all-to-all score computation.\nSpecify -p (--pca) to enable faster comparisons." << std::endl;
	std::vector<ntsm_eval_record> qq((size_t) nq * (nq - 1) / 2), cross((size_t) nq * nd);
	std::vector<uint32_t> geno((size_t) nd * 3);
	double ms = 0;
	int rc = nq >= 2 ? ntsm_eval_pairs(opt.device, c.counts.data(), nq, m, opt.minCov, qq.data(), &ms) : 0;
	if (rc) return gpuFail("scoring", rc);
	ntsm_eval_cross_times times {};
	rc = ntsm_eval_cross(opt.device, c.counts.data(), nq, store.counts(0), store.h.stride, nd, m, opt.minCov, 0, cross.data(), geno.data(), &times);
	if (rc) return gpuFail("scoring against the store", rc);
	appendStoreSamples(c, g, store, opt, talliesOf(geno));
	const auto tPrint = Clock::now();
	printBlock(c, g, opt, true, 0, nq, 0, nq + nd, [&](uint32_t q, uint32_t j) -> const ntsm_eval_record & {
		return j < nq ? qq[ntsm_eval_pair_index(q, j, nq)] : cross[(size_t) q * nd + (j - nq)];
	});
	std::cout.flush();
	if (opt.verbose > 1)
		std::cerr << "store query: " << times.chunks << " chunks, map+load " << mapMs << " ms, query pairs " << ms << " ms, upload " << times.upload_ms
		          << " ms, prepare " << times.prepare_kernel_ms << " ms, cross kernel " << times.cross_kernel_ms << " ms, download " << times.download_ms
		          << " ms, print " << msSince(tPrint) << " ms" << std::endl;
	printTime(t0);
	return 0;
}

/* --index STORE -p ROT -n NORM [-d -c]: project the store's samples, or the tail an append added, into STORE.pcaidx */
int buildIndex(Opt &opt, const Positionals &)
{
	namespace st = ntsm::eval_store;
	namespace ix = ntsm::eval_index;
	const auto t0 = Clock::now();
	const std::string path = ix::path_of(opt.store);
	st::View store;
	ix::View old;
	bool extend = false;
	std::vector<char> matrices;
	std::vector<long double> norm, rot;
	openOrRefuse([&] {
		openStore(opt.store, 0, "projects", store, nullptr);
		loadPCA(opt, store.h.n_sites, norm, rot);
		matrices = ix::matrix_bytes(norm, rot);
		struct stat sb;
		if (stat(path.c_str(), &sb) != 0) return;
		try {                                                 /* an index is there: extend it, or refuse */
			old.open(path);
			old.check_store(path, store, true);
		} catch (const st::Error &e) {
			throw st::Error(std::string(e.what()) + "; delete " + path + " to index the store anew");
		}
		if (old.h.dim != opt.dim || old.h.min_cov != opt.minCov || old.matrix_size() != matrices.size()
		    || memcmp(old.matrices(), matrices.data(), matrices.size()) != 0)
			throw st::Error(path + " was written with another -d, -c, rotation or centre; delete " + path + " to index the store anew");
		extend = true;
	});
	const uint64_t kept = extend ? old.h.n_samples : 0, added = store.h.n_samples - kept;
	if (added == 0) {
		std::cerr << path << " is up to date: " << kept << " samples" << std::endl;
		return 0;
	}
	std::vector<double> cloud((size_t) added * opt.dim);
	std::vector<uint32_t> geno((size_t) added * 3);
	ntsm_eval_cross_times times {};
	const int rc = ntsm_eval_project_store(opt.device, store.counts(kept), store.h.stride, (uint32_t) added, store.h.n_sites, opt.minCov, norm.data(),
			rot.data(), opt.dim, 0, cloud.data(), geno.data(), &times);
	if (rc) return gpuFail("projecting the store", rc);
	openOrRefuse([&] { ix::write(path, store, opt.dim, opt.minCov, matrices, extend ? old.records() : nullptr, kept, cloud.data(), geno.data(), added); });
	if (opt.verbose > 0) std::cerr << "Projected " << added << " samples; " << path << " holds " << kept + added << std::endl;
	if (opt.verbose > 1)
		std::cerr << "store index: " << times.chunks << " chunks, upload " << times.upload_ms << " ms, prepare " << times.prepare_kernel_ms
		          << " ms, projection kernel " << times.cross_kernel_ms << " ms, download " << times.download_ms << " ms" << std::endl;
	printTime(t0);
	return 0;
}

/* What --near, --within-near and --between-near open: the store (openStore) and its index, valid, current and written with the
 * run's -c and -d where those are given; -c and -d are then the index's.  Throws the refusal. */
void openIndexOf(const std::string &name, const ntsm::eval_store::View &store, ntsm::eval_index::View &index, Opt &opt)
{
	namespace st = ntsm::eval_store;
	const std::string path = ntsm::eval_index::path_of(name);
	struct stat sb;
	if (stat(path.c_str(), &sb) != 0) throw st::Error("there is no index " + path + ": run --index on the store first");
	index.open(path);
	index.check_store(path, store, false);
	if (opt.minCovGiven && opt.minCov != index.h.min_cov)
		throw st::Error("-c " + std::to_string(opt.minCov) + ", but " + path + " was written with -c " + std::to_string(index.h.min_cov));
	if (opt.dimGiven && opt.dim != index.h.dim)
		throw st::Error("-d " + std::to_string(opt.dim) + ", but " + path + " was written with -d " + std::to_string(index.h.dim));
	opt.minCov = index.h.min_cov;
	opt.dim = index.h.dim;
}

void openIndexedStore(const std::string &name, Counts &c, ntsm::eval_store::View &store, ntsm::eval_index::View &index, Opt &opt)
{
	openStore(name, c.files.size(), "scores", store, &c);
	openIndexOf(name, store, index, opt);
}

/* a store of one sample has no pair */
void refuseOneSample(const ntsm::eval_store::View &store, const std::string &name)
{
	if (store.h.n_samples == 1) throw ntsm::eval_store::Error(name + " holds one sample: nothing to compare");
}

/* the store's samples appended from the index: tallies into the summaries, projections into cloud [n_samples][dim] */
std::vector<double> appendIndexedSamples(Counts &c, std::vector<Genotype> &g, const ntsm::eval_store::View &store, const ntsm::eval_index::View &index,
		const Opt &opt)
{
	std::vector<double> cloud((size_t) store.h.n_samples * opt.dim);
	appendStoreSamples(c, g, store, opt, [&](uint32_t d, Genotype &s) {
		const ntsm::eval_index::Entry e = index.entry(d);
		s.hets = e.hets; s.homs = e.homs; s.miss = e.miss;
		memcpy(&cloud[(size_t) d * opt.dim], e.cloud, sizeof(double) * opt.dim);
	});
	return cloud;
}

/* What differs between the three store searches once the candidates are known. */
struct RouteTimes {                          /* what routeAndScore did, for the report line */
	uint64_t pairs = 0, listed = 0;
	uint32_t denseRows = 0;
	ntsm_eval_cross_times list {}, dense {};
	double scoreMs = 0, printMs = 0;
};
struct Route {
	uint32_t nOwners;                        /* samples 0 ... nOwners - 1 may own a dense row: the query files, every store sample, or A's */
	uint32_t col0, nCols;                    /* a dense row's columns are samples col0 ... col0 + nCols - 1 of the run: the store, or B */
	/* the records of the dense rows, owner dense[r]'s at rect + r * nCols; it has said what failed where it does not return 0 */
	std::function<int(const std::vector<uint32_t> &dense, ntsm_eval_record *rect, ntsm_eval_cross_times *)> scoreDense;
	std::function<int(const uint32_t *, const uint32_t *, uint64_t, ntsm_eval_record *, ntsm_eval_cross_times *)> scoreList;   /* the list scorer */
	std::function<void(const RouteTimes &)> report;   /* the -vv line */
};

/* The second half of --near, --within-near and --between-near.  A sample whose radius is DBL_MAX owns whole rows of the other
 * side: those rows are scored densely (route.scoreDense: the owner is sample 1; identical records by the contracts of
 * ntsm_eval_cross and ntsm_eval_between_rows), so the other side is never gathered for them; every other pair goes through
 * the list scorer and its records are scattered back to list order.  Then the rows, the report line and the time.
 * A pair (i, k) lies in a dense row when i owns one and k is one of its columns, k >= col0.  Under --near a query i can pair
 * with a query k < col0, so the test is needed; under --within-near col0 is 0; and of a pair that
 * ntsm_eval_between_candidates returns one index is below n_a = col0 and the other is not, so i < n_a gives k >= col0: the
 * test is the same as none for every list --between-near can get. */
int routeAndScore(const Counts &c, const std::vector<Genotype> &g, const Opt &opt, const std::vector<double> &radius, const Candidates &cand, const Route &route,
		Clock::time_point t0)
{
	const auto t = Clock::now();
	RouteTimes rt;
	const uint64_t np = rt.pairs = cand.pi.size();
	std::vector<uint32_t> dense, denseRow(route.nOwners, UINT32_MAX);
	for (uint32_t i = 0; i < route.nOwners; ++i)
		if (!(radius[i] < DBL_MAX)) { denseRow[i] = (uint32_t) dense.size(); dense.push_back(i); }
	rt.denseRows = (uint32_t) dense.size();
	std::vector<ntsm_eval_record> rect((size_t) dense.size() * route.nCols), rec(np);
	if (!dense.empty())
		if (const int rc = route.scoreDense(dense, rect.data(), &rt.dense)) return rc;
	std::vector<uint32_t> li, lk;
	std::vector<uint64_t> where;
	for (uint64_t p = 0; p < np; ++p) {
		const uint32_t i = cand.pi[p], k = cand.pk[p];
		if (i < route.nOwners && k >= route.col0 && denseRow[i] != UINT32_MAX) rec[p] = rect[(size_t) denseRow[i] * route.nCols + (k - route.col0)];
		else { li.push_back(i); lk.push_back(k); where.push_back(p); }
	}
	rt.listed = li.size();
	std::vector<ntsm_eval_record> listed(li.size());
	const int rc = route.scoreList(li.data(), lk.data(), li.size(), listed.data(), &rt.list);
	if (rc) return gpuFail("scoring the candidate pairs", rc);
	for (size_t x = 0; x < where.size(); ++x) rec[where[x]] = listed[x];
	rt.scoreMs = msSince(t);

	const auto tPrint = Clock::now();
	printCandidates(c, g, opt, cand.pi, cand.pk, cand.dist, rec.data());
	std::cout.flush();
	rt.printMs = msSince(tPrint);
	if (opt.verbose > 1) route.report(rt);
	printTime(t0);
	return 0;
}

/* --near's and --within-near's dense rows: the owners' counts (owner i's [site][2] at owners + i * ownerStride bytes) go to a
 * dense block that ntsm_eval_cross scores against the whole store */
int crossDense(const Opt &opt, const void *owners, uint64_t ownerStride, const ntsm::eval_store::View &store, const std::vector<uint32_t> &dense,
		ntsm_eval_record *rect, ntsm_eval_cross_times *times)
{
	const uint32_t m = store.h.n_sites;
	std::vector<uint32_t> sub(dense.size() * (size_t) m * 2);
	for (size_t r = 0; r < dense.size(); ++r) memcpy(&sub[r * m * 2], (const char *) owners + dense[r] * ownerStride, sizeof(uint32_t) * m * 2);
	const int rc = ntsm_eval_cross(opt.device, sub.data(), (uint32_t) dense.size(), store.counts(0), store.h.stride, (uint32_t) store.h.n_samples, m, opt.minCov, 0, rect,
			nullptr, times);
	return rc ? gpuFail("scoring against the store", rc) : 0;
}

/* and their report line (mapMs, projectMs, searchMs: the caller's first half) */
void searchReport(const RouteTimes &rt, const Candidates &cand, double mapMs, double projectMs, double searchMs)
{
	std::cerr << "store search: " << rt.pairs << " pairs (" << rt.listed << " listed, " << rt.denseRows << " dense rows), map+load " << mapMs << " ms, project "
	          << projectMs << " ms, search " << searchMs << " ms (kernels " << cand.kernelMs << " ms), score " << rt.scoreMs << " ms (gather "
	          << rt.list.upload_ms << " ms, list kernel " << rt.list.cross_kernel_ms << " ms in " << rt.list.chunks << " passes, dense upload "
	          << rt.dense.upload_ms << " ms, dense kernel " << rt.dense.cross_kernel_ms << " ms), print " << rt.printMs << " ms" << std::endl;
}

/* --near STORE FILES...: the rows of computeScorePCA (:285-398) over [FILES..., the store's samples] in which sample 1 or
 * sample 2 is one of FILES, in that run's one-thread order.  The store's projections and tallies come from STORE.pcaidx, the
 * radii are formed here (scorePCA's), and only the counts of the candidates' samples leave the store -- except for a query
 * whose radius is DBL_MAX: it owns a whole row of the store (routeAndScore). */
int searchNear(Opt &opt, const Positionals &files)
{
	const auto t0 = Clock::now();
	ntsm::eval_store::View store;
	ntsm::eval_index::View index;
	Counts c;
	c.files = files;
	const double mapMs = openOrRefuse([&] {
		openIndexedStore(opt.store, c, store, index, opt);
		if (opt.verbose > 0) std::cerr << "Reading count files" << std::endl;
		load(c, store.index(), true);
	});
	std::vector<Genotype> g = summaries(c, opt);
	const uint32_t nq = (uint32_t) c.files.size(), nd = (uint32_t) store.h.n_samples, m = store.h.n_sites, dim = opt.dim;
	if (opt.verbose > 1) std::cerr << "Finished loading files. Now searching " << nq << " samples against the " << nd << " of " << opt.store << "." << std::endl;

	auto t = Clock::now();
	std::vector<double> qCloud;
	{
		std::vector<long double> norm, rot;
		index.matrices(norm, rot);
		Session session;
		int rc = ntsm_eval_open(opt.device, c.counts.data(), nq, m, opt.minCov, &session.h);
		if (rc) return gpuFail("session", rc);
		if ((rc = project(c, opt, session.h, norm, rot, qCloud)) != 0) return rc;
	}
	const double projectMs = msSince(t);

	t = Clock::now();
	const std::vector<double> dbCloud = appendIndexedSamples(c, g, store, index, opt);
	const std::vector<double> radius = searchRadii(g, m, opt);
	if (opt.verbose > 1) std::cerr << "Starting Score Computation with PCA" << std::endl;
	Candidates cand;
	const int rc = cand.search([&](uint32_t *pi, uint32_t *pk, double *dist, uint64_t capacity, uint64_t *np, double *ms) {
		return ntsm_eval_cross_candidates(opt.device, qCloud.data(), radius.data(), nq, dbCloud.data(), radius.data() + nq, nd, dim, pi, pk, dist, capacity, np, ms);
	});
	if (rc) return rc;
	const double searchMs = msSince(t);
	const Route route { nq, nq, nd,
		[&](const std::vector<uint32_t> &dense, ntsm_eval_record *rect, ntsm_eval_cross_times *times) {
			return crossDense(opt, c.counts.data(), 8ull * m, store, dense, rect, times);
		},
		[&](const uint32_t *li, const uint32_t *lk, uint64_t n, ntsm_eval_record *out, ntsm_eval_cross_times *times) {
			return ntsm_eval_cross_score_pairs(opt.device, c.counts.data(), nq, store.counts(0), store.h.stride, nd, m, opt.minCov, li, lk, n, 0, out, times);
		},
		[&](const RouteTimes &rt) { searchReport(rt, cand, mapMs, projectMs, searchMs); } };
	return routeAndScore(c, g, opt, radius, cand, route, t0);
}

/* one band's times added to a run's */
void addTimes(ntsm_eval_cross_times &sum, const ntsm_eval_cross_times &t)
{
	sum.upload_ms += t.upload_ms; sum.prepare_kernel_ms += t.prepare_kernel_ms; sum.cross_kernel_ms += t.cross_kernel_ms;
	sum.download_ms += t.download_ms; sum.chunks += t.chunks;
}

/* The band loop of --within, --between and --contam over rows 0 ... n - 1: a band has rowsGiven rows (the run's --*-rows) or,
 * at 0, rule(first); call(first, rows, &times) fetches it and print(first, rows) prints it, band by band.  Stops at the first
 * call that fails (rc).  The summed times, the bands and the ms spent printing are the report line's. */
struct BandWalk { ntsm_eval_cross_times sum {}; uint32_t bands = 0; double printMs = 0; int rc = 0; };
template <typename Rule, typename Call, typename Print> BandWalk walkBands(uint32_t n, uint32_t rowsGiven, Rule rule, Call call, Print print)
{
	BandWalk w;
	for (uint32_t first = 0; first < n; ++w.bands) {
		const uint32_t rows = rowsGiven ? std::min(rowsGiven, n - first) : rule(first);
		ntsm_eval_cross_times times {};
		if ((w.rc = call(first, rows, &times)) != 0) return w;
		addTimes(w.sum, times);
		const auto tPrint = Clock::now();
		print(first, rows);
		w.printMs += msSince(tPrint);
		first += rows;
	}
	return w;
}

/* and the end of their -vv lines, from "resident" / "streamed" on; `kernel` names the run's kernel */
void bandReport(const BandWalk &w, double mapMs, const char *kernel)
{
	std::cerr << (w.sum.chunks ? "streamed" : "resident") << ", " << w.bands << " bands, " << w.sum.chunks << " chunks, map " << mapMs << " ms, upload "
	          << w.sum.upload_ms << " ms, prepare " << w.sum.prepare_kernel_ms << " ms, " << kernel << " kernel " << w.sum.cross_kernel_ms << " ms, download "
	          << w.sum.download_ms << " ms, print " << w.printMs << " ms" << std::endl;
}

/* --within STORE: computeScore's rows (:591-624) over the store's samples in store order -- the stdout of the all-to-all run
 * over their files at one thread -- without reading a counts file.  The triangle comes in bands of rows (eval_within.hpp's
 * rule, or --within-rows), printed band by band, which is the reference's order; the first band's call brings every
 * sample's tallies. */
int scoreWithin(Opt &opt, const Positionals &)
{
	namespace band = ntsm::eval_within;
	const auto t0 = Clock::now();
	ntsm::eval_store::View store;
	Counts c;
	const double mapMs = openOrRefuse([&] {
		openStore(opt.store, 0, "scores", store, &c);
		refuseOneSample(store, opt.store);
	});
	const uint32_t n = (uint32_t) store.h.n_samples, m = store.h.n_sites;
	if (opt.verbose > 1) std::cerr << "Mapped " << opt.store << ". Now comparing its " << n << " samples." << std::endl;
	std::cerr << "Performing all-to-all score computation.\nSpecify -p (--pca) to enable faster comparisons." << std::endl;
	WithinSession session;
	const int rc = ntsm_eval_within_open(opt.device, store.counts(0), store.h.stride, n, m, opt.minCov, 0, &session.h);
	if (rc) return gpuFail("opening the store", rc);
	std::vector<uint32_t> geno((size_t) n * 3);
	std::vector<Genotype> g;
	std::vector<ntsm_eval_record> rec;
	const BandWalk w = walkBands(n, opt.withinRows, [&](uint32_t first) { return band::band_rows(first, n, band::kBandRecords); },
		[&](uint32_t first, uint32_t rows, ntsm_eval_cross_times *times) {
			rec.resize(band::band_records(first, rows, n));
			return ntsm_eval_within_rows(session.h, first, rows, rec.data(), first == 0 ? geno.data() : nullptr, times);
		},
		[&](uint32_t first, uint32_t rows) {
			if (first == 0) appendStoreSamples(c, g, store, opt, talliesOf(geno));
			printBlock(c, g, opt, first == 0, first, first + rows, 0, n,
				[&](uint32_t i, uint32_t j) -> const ntsm_eval_record & { return rec[band::band_offset(i, j, first, n)]; });
		});
	if (w.rc) return gpuFail("scoring the store", w.rc);
	std::cout.flush();
	if (opt.verbose > 1) { std::cerr << "store within: "; bandReport(w, mapMs, "pair"); }
	printTime(t0);
	return 0;
}

/* --within-near STORE: computeScorePCA's rows (:285-398) over the store's samples -- the stdout of the -p run over their
 * files with the index's rotation, centre, -d and -c.  Projections and tallies come from STORE.pcaidx and the radii are formed
 * here, so the search is ntsm_eval_cross_candidates with every sample a query and no database side: by its contract
 * ntsm_eval_candidates' list.  Any sample may own whole rows (routeAndScore); the other pairs are pairs of two store samples. */
int searchWithin(Opt &opt, const Positionals &)
{
	const auto t0 = Clock::now();
	ntsm::eval_store::View store;
	ntsm::eval_index::View index;
	Counts c;
	const double mapMs = openOrRefuse([&] {
		openIndexedStore(opt.store, c, store, index, opt);
		refuseOneSample(store, opt.store);
	});
	const uint32_t n = (uint32_t) store.h.n_samples, m = store.h.n_sites, dim = opt.dim;
	if (opt.verbose > 1) std::cerr << "Mapped " << opt.store << " and its index. Now searching its " << n << " samples." << std::endl;

	const auto t = Clock::now();
	std::vector<Genotype> g;
	const std::vector<double> cloud = appendIndexedSamples(c, g, store, index, opt);
	const std::vector<double> radius = searchRadii(g, m, opt);
	if (opt.verbose > 1) std::cerr << "Starting Score Computation with PCA" << std::endl;
	Candidates cand;
	const int rc = cand.search([&](uint32_t *pi, uint32_t *pk, double *dist, uint64_t capacity, uint64_t *np, double *ms) {
		return ntsm_eval_cross_candidates(opt.device, cloud.data(), radius.data(), n, nullptr, nullptr, 0, dim, pi, pk, dist, capacity, np, ms);
	});
	if (rc) return rc;
	const double searchMs = msSince(t);
	const Route route { n, 0, n,
		[&](const std::vector<uint32_t> &dense, ntsm_eval_record *rect, ntsm_eval_cross_times *times) {
			return crossDense(opt, store.counts(0), store.h.stride, store, dense, rect, times);
		},
		[&](const uint32_t *li, const uint32_t *lk, uint64_t np, ntsm_eval_record *out, ntsm_eval_cross_times *times) {
			return ntsm_eval_store_score_pairs(opt.device, store.counts(0), store.h.stride, n, m, opt.minCov, li, lk, np, 0, out, times);
		},
		[&](const RouteTimes &rt) { searchReport(rt, cand, mapMs, 0.0, searchMs); } };
	return routeAndScore(c, g, opt, radius, cand, route, t0);
}

/* --between STORE_A STORE_B: computeScore's rows (:591-624) over [A's samples, B's samples] whose sample 1 is of A and whose
 * sample 2 is of B, in that run's order, without reading a counts file.  A's locus table and distinct columns play the first
 * file's part and B's samples are later files of that run: their loci are matched to A's by ID (eval_between.hpp), on the
 * device.  The rectangle comes in bands of rows of A (that header's rule, or --between-rows), printed band by band; a band's
 * call brings the tallies of its rows and the first one those of B's samples, taken over A's sites. */
int scoreBetween(Opt &opt, const Positionals &files)
{
	namespace band = ntsm::eval_between;
	const auto t0 = Clock::now();
	const std::string &storeB = files[0];
	ntsm::eval_store::View a, b;
	band::LocusMap map;
	Counts c;
	const double mapMs = openOrRefuse([&] {
		openStore(opt.store, 0, "scores", a, &c);
		openStore(storeB, a.h.n_samples, "scores", b, nullptr);
		map = band::map_loci(a, b, opt.store, storeB);
	});
	const uint32_t na = (uint32_t) a.h.n_samples, nb = (uint32_t) b.h.n_samples;
	if (opt.verbose > 1) std::cerr << "Mapped " << opt.store << " and " << storeB << ". Now comparing " << na << " samples against " << nb << "." << std::endl;
	std::cerr << "Performing all-to-all score computation.\nSpecify -p (--pca) to enable faster comparisons." << std::endl;
	BetweenSession session;
	const int rc = ntsm_eval_between_open(opt.device, a.counts(0), a.h.stride, na, b.counts(0), b.h.stride, nb, a.h.n_sites, b.h.n_sites, map.data(), opt.minCov, 0,
			&session.h);
	if (rc) return gpuFail("opening the stores", rc);
	std::vector<Genotype> g;
	appendStoreSamples(c, g, a, opt, [](uint32_t, Genotype &) {});                /* A's tallies come with their bands */
	std::vector<uint32_t> genoA, genoB((size_t) nb * 3);
	std::vector<ntsm_eval_record> rec;
	const BandWalk w = walkBands(na, opt.betweenRows, [&](uint32_t first) { return band::band_rows(first, na, nb, band::kBandRecords); },
		[&](uint32_t first, uint32_t rows, ntsm_eval_cross_times *times) {
			rec.resize((size_t) rows * nb);
			genoA.resize((size_t) rows * 3);
			return ntsm_eval_between_rows(session.h, first, rows, rec.data(), genoA.data(), first == 0 ? genoB.data() : nullptr, times);
		},
		[&](uint32_t first, uint32_t rows) {
			if (first == 0) appendStoreSamples(c, g, b, opt, talliesOf(genoB));
			for (uint32_t r = 0; r < rows; ++r) setTallies(g[first + r], &genoA[3 * (size_t) r]);
			printBlock(c, g, opt, first == 0, first, first + rows, na, na + nb,
				[&](uint32_t i, uint32_t j) -> const ntsm_eval_record & { return rec[(size_t) (i - first) * nb + (j - na)]; });
		});
	if (w.rc) return gpuFail("scoring the stores", w.rc);
	std::cout.flush();
	if (opt.verbose > 1) {
		std::cerr << "store between: loci " << (map.identical ? "identical" : "mapped") << " (" << map.lacking << " of " << a.h.n_sites << " absent from " << storeB << "), B ";
		bandReport(w, mapMs, "pair");
	}
	printTime(t0);
	return 0;
}

/* --between-near STORE_A STORE_B: computeScorePCA's rows (:285-398) over [A's samples, B's samples] that pair a sample of one
 * store with a sample of the other, in that run's one-thread order, with the rotation, centre, -d and -c of A's index.  A's
 * locus table and distinct columns play the first file's part, as in --between.  A's projections and tallies come from its
 * index; B's from B's index where eval_between.hpp's rule says it serves, else from ntsm_eval_project_store_mapped, and
 * nothing is written.  A sample of A whose radius is DBL_MAX owns its whole row of B: runs of such rows go through
 * --between's session (identical records by its contract; B is never gathered for them); every other pair -- those owned by
 * a search-all sample of B among them, as (b, a) -- goes through ntsm_eval_between_score_pairs (routeAndScore). */
int searchBetween(Opt &opt, const Positionals &files)
{
	namespace st = ntsm::eval_store;
	namespace ix = ntsm::eval_index;
	namespace band = ntsm::eval_between;
	const auto t0 = Clock::now();
	const std::string &storeB = files[0];
	st::View a, b;
	ix::View indexA, indexB;
	band::LocusMap map;
	band::BIndexFacts facts;
	Counts c;
	const double mapMs = openOrRefuse([&] {
		openStore(opt.store, 0, "scores", a, &c);
		openStore(storeB, a.h.n_samples, "scores", b, nullptr);
		map = band::map_loci(a, b, opt.store, storeB);
		try {
			openIndexOf(opt.store, a, indexA, opt);
		} catch (const st::Error &e) {                       /* absent, invalid, stale, or another -c / -d */
			throw st::Error(std::string(e.what()) + " (--between-near searches through the index of store A: --index " + opt.store + " -p ROT -n NORM)");
		}
		const std::string pathB = ix::path_of(storeB);
		struct stat sb;
		facts.exists = stat(pathB.c_str(), &sb) == 0;
		if (facts.exists)
			try {
				indexB.open(pathB);
				facts.valid = true;
				indexB.check_store(pathB, b, false);
				facts.current = true;
			} catch (const st::Error &) {                    /* B is projected in the run instead */
			}
		facts.identical_loci = map.identical;
		facts.dim_a = indexA.h.dim; facts.min_cov_a = indexA.h.min_cov; facts.matrices_a = indexA.matrices(); facts.matrix_size_a = indexA.matrix_size();
		if (facts.valid) { facts.dim_b = indexB.h.dim; facts.min_cov_b = indexB.h.min_cov; facts.matrices_b = indexB.matrices(); facts.matrix_size_b = indexB.matrix_size(); }
	});
	const bool fromIndex = band::b_index_usable(facts);
	const uint32_t na = (uint32_t) a.h.n_samples, nb = (uint32_t) b.h.n_samples, m = a.h.n_sites, dim = opt.dim;
	if (opt.verbose > 1)
		std::cerr << "Mapped " << opt.store << ", its index and " << storeB << ". Now searching " << na << " samples against " << nb << "." << std::endl;

	auto t = Clock::now();
	std::vector<Genotype> g;
	const std::vector<double> cloudA = appendIndexedSamples(c, g, a, indexA, opt);
	std::vector<double> cloudB;
	if (fromIndex) cloudB = appendIndexedSamples(c, g, b, indexB, opt);
	else {
		std::vector<long double> norm, rot;
		indexA.matrices(norm, rot);
		cloudB.assign((size_t) nb * dim, 0.0);
		std::vector<uint32_t> geno((size_t) nb * 3);
		const int rc = ntsm_eval_project_store_mapped(opt.device, b.counts(0), b.h.stride, nb, m, b.h.n_sites, map.data(), opt.minCov, norm.data(), rot.data(), dim, 0,
				cloudB.data(), geno.data(), nullptr);
		if (rc) return gpuFail("projecting the second store", rc);
		appendStoreSamples(c, g, b, opt, talliesOf(geno));
	}
	const double projectMs = msSince(t);

	t = Clock::now();
	const std::vector<double> radius = searchRadii(g, m, opt);
	if (opt.verbose > 1) std::cerr << "Starting Score Computation with PCA" << std::endl;
	Candidates cand;
	const int rc = cand.search([&](uint32_t *pi, uint32_t *pk, double *dist, uint64_t capacity, uint64_t *np, double *ms) {
		return ntsm_eval_between_candidates(opt.device, cloudA.data(), radius.data(), na, cloudB.data(), radius.data() + na, nb, dim, pi, pk, dist, capacity, np, ms);
	});
	if (rc) return rc;
	const double searchMs = msSince(t);
	size_t nRuns = 0;
	const Route route { na, na, nb,
		[&](const std::vector<uint32_t> &, ntsm_eval_record *rect, ntsm_eval_cross_times *) {   /* the dense rows as runs of consecutive samples of A, each in bands */
			const std::vector<std::pair<uint32_t, uint32_t>> runs = band::dense_runs(radius.data(), na, DBL_MAX);
			nRuns = runs.size();
			BetweenSession session;
			int r = ntsm_eval_between_open(opt.device, a.counts(0), a.h.stride, na, b.counts(0), b.h.stride, nb, m, b.h.n_sites, map.data(), opt.minCov, 0, &session.h);
			if (r) return gpuFail("opening the stores", r);
			size_t done = 0;
			for (const auto &run : runs)
				for (uint32_t first = run.first, end = run.first + run.second; first < end;) {
					const uint32_t rows = band::band_rows(first, end, nb, band::kBandRecords);
					r = ntsm_eval_between_rows(session.h, first, rows, rect + done * nb, nullptr, nullptr, nullptr);
					if (r) return gpuFail("scoring the stores", r);
					first += rows;
					done += rows;
				}
			return 0;
		},
		[&](const uint32_t *li, const uint32_t *lk, uint64_t n, ntsm_eval_record *out, ntsm_eval_cross_times *times) {
			return ntsm_eval_between_score_pairs(opt.device, a.counts(0), a.h.stride, na, b.counts(0), b.h.stride, nb, m, b.h.n_sites, map.data(), opt.minCov, li, lk, n, 0,
					out, times);
		},
		[&](const RouteTimes &rt) {
			std::cerr << "store between-near: loci " << (map.identical ? "identical" : "mapped") << " (" << map.lacking << " of " << m << " absent from " << storeB
			          << "), B's projections " << (fromIndex ? "from index" : "projected") << ", " << rt.pairs << " candidates (" << rt.listed << " listed pairs in "
			          << rt.list.chunks << " passes, " << rt.denseRows << " dense rows of A in " << nRuns << " runs), map " << mapMs << " ms, project " << projectMs
			          << " ms, search " << searchMs << " ms (kernels " << cand.kernelMs << " ms), score " << rt.scoreMs << " ms (gather " << rt.list.upload_ms
			          << " ms, remap+terms " << rt.list.prepare_kernel_ms << " ms, list kernel " << rt.list.cross_kernel_ms << " ms), print " << rt.printMs
			          << " ms" << std::endl;
		} };
	return routeAndScore(c, g, opt, radius, cand, route, t0);
}

/* --qc STORE [-p ROT -n NORM] [--sites-out FILE]: computeScoreSingle (:541-585) with one row per sample of the store -- the row
 * the single-file run prints for a counts file whose loci and distinct columns are the store's --, each followed by "\n".  The
 * tallies of the samples and, for --sites-out, of the sites come from one pass over the store (ntsm_eval_store_profile); the
 * PC columns from ntsm_eval_project_store in the same run, STORE.pcaidx neither read nor written. */
int qcStore(Opt &opt, const Positionals &)
{
	const auto t0 = Clock::now();
	ntsm::eval_store::View store;
	Counts c;
	std::vector<long double> norm, rot;
	OutFile sites;
	const bool sitesOut = opt.has(gSitesOut);
	const unsigned dim = opt.pca.empty() ? 0 : opt.dim;   /* the PC columns */
	const double mapMs = openOrRefuse([&] {
		openStore(opt.store, 0, "scores", store, &c);
		if (!opt.pca.empty()) loadPCA(opt, store.h.n_sites, norm, rot);
		if (sitesOut) sites.open(opt.sitesOut);
	});
	const uint32_t n = (uint32_t) store.h.n_samples, m = store.h.n_sites;
	if (opt.verbose > 1) std::cerr << "Mapped " << opt.store << ". Providing only QC information for its " << n << " samples." << std::endl;
	std::vector<uint32_t> geno((size_t) n * 3), tally(sitesOut ? (size_t) m * 4 : 0);
	std::vector<uint64_t> siteCov(sitesOut ? m : 0);
	ntsm_eval_cross_times times {}, projectTimes {};
	int rc = ntsm_eval_store_profile(opt.device, store.counts(0), store.h.stride, n, m, opt.minCov, 0, geno.data(), sitesOut ? tally.data() : nullptr,
			sitesOut ? siteCov.data() : nullptr, &times);
	if (rc) return gpuFail("profiling the store", rc);
	std::vector<double> cloud;
	if (!opt.pca.empty()) {
		cloud.assign((size_t) n * opt.dim, 0.0);
		rc = ntsm_eval_project_store(opt.device, store.counts(0), store.h.stride, n, m, opt.minCov, norm.data(), rot.data(), opt.dim, 0, cloud.data(), nullptr,
				&projectTimes);
		if (rc) return gpuFail("projecting the store", rc);
	}
	const auto tPrint = Clock::now();
	std::vector<Genotype> g;
	appendStoreSamples(c, g, store, opt, talliesOf(geno));
	std::cout << qcHeader(dim) << std::endl;
	for (uint32_t i = 0; i < n; ++i) std::cout << qcRow(c.files[i], g[i], cloud.data() + (size_t) i * dim, dim) + "\n";
	std::cout.flush();
	if (sitesOut) {
		std::string text = ntsm::eval_qc::kSiteHeader;
		for (uint32_t s = 0; s < m; ++s) ntsm::eval_qc::site_line(text, c.locus[s].c_str(), &tally[(size_t) s * 4], siteCov[s], n);
		if (!sites.write(text)) return 1;
	}
	if (opt.verbose > 1)
		std::cerr << "store qc: " << times.chunks << " chunks, map+load " << mapMs << " ms, upload " << times.upload_ms << " ms, profile kernel " << times.cross_kernel_ms
		          << " ms, download " << times.download_ms << " ms, project " << projectTimes.upload_ms + projectTimes.prepare_kernel_ms + projectTimes.cross_kernel_ms
		             + projectTimes.download_ms << " ms (upload " << projectTimes.upload_ms << " ms, projection kernel " << projectTimes.cross_kernel_ms
		          << " ms), print " << msSince(tPrint) << " ms" << std::endl;
	printTime(t0);
	return 0;
}

/* --contam STORE [-c N] [--contam-depth D] [--contam-min X] [--contam-explained Y] [-a] [--contam-rows N] [--samples-out FILE]:
 * is a sample of the store a mixture, and of which other sample.  The rectangle of ordered pairs
 * (target, source) comes in bands of targets (eval_contam.hpp's rule, or --contam-rows), printed band by band, each band's call
 * bringing its targets' tallies; the rates, the filter and the text are that header's. */
int contamStore(Opt &opt, const Positionals &)
{
	namespace ct = ntsm::eval_contam;
	const auto t0 = Clock::now();
	ntsm::eval_store::View store;
	OutFile samples;
	const double mapMs = openOrRefuse([&] {
		openStore(opt.store, 0, "scores", store, nullptr);
		if (opt.has(gSamplesOut)) samples.open(opt.samplesOut);
	});
	const uint32_t n = (uint32_t) store.h.n_samples, m = store.h.n_sites;
	if (opt.verbose > 1) std::cerr << "Mapped " << opt.store << ". Now checking its " << n << " samples against each other." << std::endl;
	ContamSession session;
	const int rc = ntsm_eval_contam_open(opt.device, store.counts(0), store.h.stride, n, m, opt.minCov, opt.contamDepth, 0, &session.h);
	if (rc) return gpuFail("opening the store", rc);
	std::vector<std::string> nameOf(n);
	std::vector<const char *> names(n);
	for (uint32_t d = 0; d < n; ++d) { nameOf[d] = store.name(d); names[d] = nameOf[d].c_str(); }
	std::vector<ntsm_eval_contam_record> rec;
	std::vector<uint64_t> tally((size_t) n * 3);
	std::string temp;
	const BandWalk w = walkBands(n, opt.contamRows, [&](uint32_t first) { return ct::band_rows(first, n, ct::kBandRecords); },
		[&](uint32_t first, uint32_t rows, ntsm_eval_cross_times *times) {
			rec.resize((size_t) rows * n);
			return ntsm_eval_contam_rows(session.h, first, rows, rec.data(), tally.data() + (size_t) first * 3, times);
		},
		[&](uint32_t first, uint32_t rows) {
			if (first == 0) std::cout << ct::kHeader;
			temp.clear();
			ct::band_text(temp, names.data(), n, first, rows, rec.data(), tally.data() + (size_t) first * 3, opt.all, opt.contamMin, opt.contamExplained);
			std::cout << temp;
		});
	if (w.rc) return gpuFail("checking the store", w.rc);
	std::cout.flush();
	if (opt.has(gSamplesOut)) {
		std::string text = ct::kSampleHeader;
		for (uint32_t i = 0; i < n; ++i) ct::sample_line(text, names[i], &tally[(size_t) i * 3]);
		if (!samples.write(text)) return 1;
	}
	if (opt.verbose > 1) { std::cerr << "store contam: "; bandReport(w, mapMs, "rectangle"); }
	printTime(t0);
	return 0;
}

/* --trios STORE [-c N] [--trio-depth D] [--trio-max X] [--trio-duo Y] [--trio-called M] [--trio-exhaustive] [-a] [--ped FILE]:
 * which samples of the store form a parent-parent-child trio, or whether a pedigree's trios hold.  The
 * runs, their rules and the text are eval_trio.hpp's; this opens the store and the session and hands it the library's two entry
 * points.  Every refusal -- the store, the pedigree, its IDs -- comes before the session is opened. */
int trioStore(Opt &opt, const Positionals &)
{
	namespace tr = ntsm::eval_trio;
	const auto t0 = Clock::now();
	ntsm::eval_store::View store;
	std::vector<std::string> nameOf;
	std::vector<tr::PedTrio> pedTrios;
	tr::Ped ped;
	const bool pedGiven = opt.has(gPed);
	const double mapMs = openOrRefuse([&] {
		openStore(opt.store, 0, "scores", store, nullptr);
		if (store.h.n_samples < 3) throw tr::Error(opt.store + " holds fewer than 3 samples: there is no trio to look for");
		nameOf.resize(store.h.n_samples);
		for (uint32_t d = 0; d < nameOf.size(); ++d) nameOf[d] = store.name(d);
		if (!pedGiven) return;
		std::ifstream fh(opt.ped);
		struct stat sb;
		if (!fh.good() || stat(opt.ped.c_str(), &sb) != 0 || !S_ISREG(sb.st_mode)) throw tr::Error("cannot read the pedigree file " + opt.ped);
		std::stringstream text;
		text << fh.rdbuf();
		ped = tr::parse_ped(text.str());
		pedTrios = tr::resolve(ped, nameOf);
	});
	const uint32_t n = (uint32_t) store.h.n_samples, m = store.h.n_sites;
	if (opt.verbose > 0 && pedGiven)
		std::cerr << "Read " << pedTrios.size() << " trios from " << opt.ped << "; skipped " << ped.comments << " comment lines and " << ped.founders
		          << " lines without both parents" << std::endl;
	if (opt.verbose > 1) std::cerr << "Mapped " << opt.store << ". Now looking for trios among its " << n << " samples." << std::endl;
	TrioSession session;
	ntsm_eval_cross_times open {};
	int rc = ntsm_eval_trio_open(opt.device, store.counts(0), store.h.stride, n, m, opt.minCov, opt.trioDepth, 0, nullptr, &open, &session.h);
	if (rc) return gpuFail("opening the store", rc);
	CallTimes duo, score;
	double printMs = 0;
	tr::Device dev;
	dev.duos = [&](uint32_t first, uint32_t rows, ntsm_eval_trio_duo *out) {
		return timedCall(duo, [&](double *ms) { return ntsm_eval_trio_duos(session.h, first, rows, out, ms); });
	};
	dev.score = [&](const uint32_t *child, const uint64_t *offset, const uint32_t *cand, uint32_t count, ntsm_eval_trio_record *out) {
		return timedCall(score, [&](double *ms) { return ntsm_eval_trio_score(session.h, child, offset, cand, count, out, ms); });
	};
	const tr::Sink sink = [&](const std::string &text) { const auto t = Clock::now(); std::cout << text; printMs += msSince(t); };
	tr::Cuts cuts;
	cuts.min_called = opt.trioCalled; cuts.max_rate = opt.trioMax; cuts.max_duo = opt.trioDuo; cuts.all = opt.all; cuts.exhaustive = opt.trioExhaustive;
	tr::Stats st;
	try {
		rc = pedGiven ? tr::pedigree(dev, nameOf, pedTrios, cuts, sink, st) : tr::search(dev, nameOf, cuts, sink, st);
	} catch (const tr::Error &e) {
		ntsm::refuse(e.what());
	}
	if (rc) return gpuFail("looking for trios", rc);
	std::cout.flush();
	if (opt.verbose > 1)
		std::cerr << "store trios: planes " << 3ull * ((m + 63ull) / 64) * 8 * n << " bytes, " << open.chunks << " chunks, " << st.bands << " duo bands, "
		          << st.children << " children with 2 or more candidates, " << st.triples << " triples, " << st.rows << " rows, map " << mapMs << " ms, upload "
		          << open.upload_ms << " ms, plane kernel " << open.prepare_kernel_ms << " ms, duo " << duo.callMs << " ms (kernel " << duo.kernelMs << " ms), score "
		          << score.callMs << " ms (kernel " << score.kernelMs << " ms), print " << printMs << " ms" << std::endl;
	printTime(t0);
	return 0;
}

/* --ld STORE [-c N] [--ld-depth D] [--ld-min T] [--ld-called M] [--ld-prune FILE] [-a]: which pairs of sites of the store are
 * in linkage disequilibrium, and which sites a prune keeps.  The band walk, the text and the prune are
 * eval_ld.hpp's; this opens the store and the session and hands the walk the library's selection.  Every refusal comes before the
 * session is opened.  NTSM_LD_PAIR_BUDGET (tests): the pairs of one call, in place of 1 GiB of them. */
int ldStore(Opt &opt, const Positionals &)
{
	namespace ld = ntsm::eval_ld;
	const auto t0 = Clock::now();
	ntsm::eval_store::View store;
	OutFile prunedFile;
	const bool pruneGiven = opt.has(gLdPrune);
	const double mapMs = openOrRefuse([&] {
		openStore(opt.store, 0, "scores", store, nullptr);
		if (store.h.n_samples < 2) throw ld::Error(opt.store + " holds fewer than 2 samples: no site varies among them");
		if (store.h.n_samples > NTSM_EVAL_LD_MAX_SAMPLES) throw ld::Error(opt.store + " holds more than 16777216 samples: the moments of --ld are exact up to there");
		if (store.h.n_sites < 2) throw ld::Error(opt.store + " holds fewer than 2 sites: there is no pair of sites");
		if (pruneGiven) prunedFile.open(opt.ldPrune);
	});
	const uint32_t n = (uint32_t) store.h.n_samples, m = store.h.n_sites;
	uint64_t budget = ld::kPairBudget;
	if (const char *b = getenv("NTSM_LD_PAIR_BUDGET")) budget = strtoull(b, nullptr, 10);
	if (opt.verbose > 1) std::cerr << "Mapped " << opt.store << ". Now comparing its " << m << " sites over " << n << " samples." << std::endl;
	LdSession session;
	ntsm_eval_cross_times open {};
	int rc = ntsm_eval_ld_open(opt.device, store.counts(0), store.h.stride, n, m, opt.minCov, opt.ldDepth, 0, nullptr, &open, &session.h);
	if (rc) return gpuFail("opening the store", rc);
	std::vector<const char *> locus(m);
	for (uint32_t s = 0; s < m; ++s) locus[s] = store.locus[s].c_str();
	CallTimes select;
	double printMs = 0;
	const double cut = opt.all ? 0.0 : opt.ldMin;                                  /* r2 >= 0 wherever it is defined */
	ld::Device dev;
	dev.select = [&](uint32_t first, uint32_t rows, uint64_t cap, ntsm_eval_ld_pair *out, uint64_t *found) {
		return timedCall(select, [&](double *ms) { return ntsm_eval_ld_select(session.h, first, rows, opt.ldCalled, cut, cap, out, found, ms); });
	};
	ld::Prune prune(m);
	bool headed = false;
	std::string text;
	ld::Stats st;
	rc = ld::walk(dev, m, budget, [&](const ntsm_eval_ld_pair *pairs, uint64_t count) {
		const auto t = Clock::now();
		text.clear();
		if (!headed) { text = ld::kHeader; headed = true; }
		ld::rows_text(text, locus.data(), pairs, count);
		std::cout << text;
		if (pruneGiven) prune.add(pairs, count, opt.ldCalled, opt.ldMin);
		printMs += msSince(t);
	}, st);
	if (rc) return gpuFail("comparing the sites", rc);
	std::cout.flush();
	if (pruneGiven && !prunedFile.write(prune.text(locus.data()))) return 1;
	if (opt.verbose > 1) {
		std::cerr << "store ld: planes " << 3ull * ((n + 63ull) / 64) * 8 * m << " bytes, " << open.chunks << " chunks, " << st.bands << " bands, " << st.reruns
		          << " re-runs, " << st.pairs << " pairs";
		if (pruneGiven) std::cerr << ", " << prune.n_kept() << " kept sites";
		std::cerr << ", map " << mapMs << " ms, upload " << open.upload_ms << " ms, plane kernel " << open.prepare_kernel_ms << " ms, select " << select.callMs
		          << " ms (kernel " << select.kernelMs << " ms), print " << printMs << " ms" << std::endl;
	}
	printTime(t0);
	return 0;
}

/* FILES...: the reference's runs -- the QC row of one file, all pairs, the -p search, the merge */
int runFiles(Opt &opt, const Positionals &files)
{
	const auto t0 = Clock::now();
	Counts c;
	c.files = files;
	if (opt.verbose > 0) std::cerr << "Reading count files" << std::endl;
	load(c);
	std::vector<Genotype> g = summaries(c, opt);
	std::vector<long double> norm, rot;
	if (opt.pcaRuns) loadPCA(opt, c.nSites(), norm, rot);     /* every refusal and abort of the PCA inputs comes before the GPU */
	if (c.files.size() > 1 && opt.verbose > 1) std::cerr << "Finished loading files. Now comparing all samples." << std::endl;
	if (c.files.size() == 1) {                           /* computeScoreSingle, :541-585 */
		if (opt.verbose > 1) std::cerr << "Detected only 1 file, providing only QC information." << std::endl;
		std::vector<double> cloud;
		if (opt.pcaRuns) {                               /* projectPCs + the PC columns */
			Session session;
			int rc = ntsm_eval_open(opt.device, c.counts.data(), 1, (uint32_t) c.nSites(), opt.minCov, &session.h);
			if (rc) return gpuFail("session", rc);
			if ((rc = project(c, opt, session.h, norm, rot, cloud)) != 0) return rc;
		}
		std::cout << qcHeader(opt.pcaRuns ? opt.dim : 0) << std::endl;
		std::cout << qcRow(c.files[0], g[0], cloud.data(), (unsigned) cloud.size());
	} else if (opt.onlyMerge) {                          /* src/ntSeqMatchEval.cpp:314-322 */
		if (opt.merge.empty()) { std::cerr << "(-l) cannot be used without --merge (-e) option." << std::endl; exit(EXIT_FAILURE); }
		std::cerr << " (-l) option detected. Not performing analysis, only merging." << std::endl;
	} else if (opt.pcaRuns) {                            /* projectPCs + computeScorePCA, src/ntSeqMatchEval.cpp:333-341 */
		Session session;
		int rc = ntsm_eval_open(opt.device, c.counts.data(), (uint32_t) c.files.size(), (uint32_t) c.nSites(), opt.minCov, &session.h);
		if (rc) return gpuFail("session", rc);
		std::vector<double> cloud;
		rc = project(c, opt, session.h, norm, rot, cloud);
		if (!rc) rc = scorePCA(c, g, opt, session.h, cloud);
		if (rc) return rc;
	} else {                                             /* computeScore, :591-624 */
		std::cerr << "Performing all-to-all score computation.\nSpecify -p (--pca) to enable faster comparisons." << std::endl;
		const uint32_t n = (uint32_t) c.files.size();
		std::vector<ntsm_eval_record> rec((size_t) n * (n - 1) / 2);
		double ms = 0;
		const int rc = ntsm_eval_pairs(opt.device, c.counts.data(), n, (uint32_t) c.nSites(), opt.minCov, rec.data(), &ms);
		if (rc) return gpuFail("scoring", rc);
		if (opt.verbose > 1) std::cerr << "pair kernel: " << ms << " ms for " << rec.size() << " pairs" << std::endl;
		printBlock(c, g, opt, true, 0, n, 0, n, [&](uint32_t i, uint32_t j) -> const ntsm_eval_record & { return rec[ntsm_eval_pair_index(i, j, n)]; });
	}
	std::cout.flush();
	if (c.files.size() > 1 && !opt.merge.empty()) {      /* mergeCounts, :626-674 */
		for (size_t i = 0; i < c.kmerSize.size(); ++i)
			for (size_t j = i + 1; j < c.kmerSize.size(); ++j)
				if (c.kmerSize[i] != c.kmerSize[j]) { std::cerr << PROGRAM ": counts files with different k cannot be merged" << std::endl; abort(); }   /* assert, :631-635 */
		std::ofstream out(opt.merge);
		uint64_t tk = 0;
		for (uint64_t v : c.rawTotal) tk += v;
		out << "#@TK\t" << std::to_string(tk) << "\n#@KS\t" << std::to_string(c.kmerSize[0])
		    << "\n#locusID\tcountAT\tcountCG\tsumAT\tsumCG\tdistinctAT\tdistinctCG\n";
		const size_t m = c.nSites();
		for (size_t s = 0; s < m; ++s) {
			unsigned cAT = 0, cCG = 0, sAT = 0, sCG = 0;
			for (size_t j = 0; j < c.files.size(); ++j) {
				cAT += c.counts[(j * m + s) * 2]; cCG += c.counts[(j * m + s) * 2 + 1];
				sAT += c.sums[(j * m + s) * 2]; sCG += c.sums[(j * m + s) * 2 + 1];
			}
			out << c.locus[s] << "\t" << cAT << "\t" << cCG << "\t" << sAT << "\t" << sCG << "\t" << c.distinct[2 * s] << "\t" << c.distinct[2 * s + 1] << "\n";
		}
	}
	printTime(t0);
	return 0;
}

}  // namespace

/* read the flags; collect the positionals; the first refusal that needs no store, or the run's row; the run */
int main(int argc, char **argv)
{
	Opt opt;
	readFlags(argc, argv, opt);
	Positionals files;
	while (optind < argc) files.emplace_back(argv[optind++]);
	const RunRow &run = firstRefusal(opt, files);
	return run.perform(opt, files);
}
