/* options.hpp -- what ntsmCount was asked to do: the reference's opt:: fields and this port's own switches */
#ifndef NTSM_OPTIONS_HPP
#define NTSM_OPTIONS_HPP
#include <cstdint>
#include <string>
#include <vector>

namespace ntsm {

struct Options {                           /* the opt:: fields ntsmCount reads (src/Options.h:21-62) */
	int verbose = 0;
	unsigned threads = 1;
	unsigned k = 19;
	std::string snp, summary;
	float siteCovThreshold = 0.75f;
	double covThresh = 1.7976931348623157e308;   /* DBL_MAX: never stop */
	bool dupes = false;
	int device = 0;                        /* HIP device (new; the reference has no device concept) */
	int debug_kernel = -1;                 /* --debug-kernel V (tests only): ntsm_set_kernel(ctx, V) on every context, -1 = the library's choice */
	std::vector<int> devices;              /* -g 0,1,...: host threads (-t) are spread round-robin over these devices */
	uint64_t batch_bytes = 64ull << 20;    /* staging capacity per slot */
	bool phase_times = false;              /* NTSM_PHASE_TIMES: print where the wall time goes (stderr) */
	/* Block size of the block-parallel FASTQ ingest (-t N, plain files).  A block's sequences (< half its bytes) fit
	 * one 16 MiB lane slot, so a thread never has to wait for its predecessor in the middle of a block. */
	uint64_t block_bytes = 16ull << 20;
	/* Producer lanes send 2-bit codes + a validity bit per position (3/8 byte instead of 1 over PCIe; pack2.hpp) and the
	 * device unpacks them.  NTSM_NO_PACK=1 sends the raw bytes instead (same counts: A/B of the two ingest forms). */
	bool pack = true;
	/* gzip inputs of at least this many (compressed) bytes take the parallel route with -t N: decoder pool + piece-parallel
	 * parsing (gz_stream.hpp, parallel_gz_fastq.hpp); smaller ones are read one thread per file */
	uint64_t gz_parallel_min_bytes = 8ull << 20;
	unsigned gz_decoders = 0;              /* NTSM_GZ_DECODERS: decoder threads of that route (0 = automatic) */
	/* The input files, known before the sites are loaded: with -t N and no -m the first one is parsed into ordinary memory
	 * while the sites load and the tables build (early_ingest.hpp; NTSM_NO_EARLY=1 switches that off) */
	std::vector<std::string> inputs;
	bool early = true;
	/* which kind of first file: 1 plain FASTQ, 2 gzip, 3 both (NTSM_EARLY=plain|gz|all).  Default gzip only: measured on a
	 * 12.6 GB FASTQ, the early path parses into gigabytes of memory touched for the first time at 1/6 of the speed of the lane
	 * slots (reused, pinned, cache-warm) and loses (0.85 s against 0.41 s whole process); a .gz, whose inflate dominates, gains
	 * (2e7 / 4e7 reads: 0.68 / 1.22 s against 0.80 / 1.29 s) */
	int early_kinds = 2;
};

} // namespace ntsm
#endif
