/*
 * include/ntsm_host.h -- C ABI over the host-side pieces of ntsmCount (site loading, read
 * flattening, report formatting) so that tests and bench.py can drive them without the CLI.
 * None of these functions touches a GPU.  Reference behaviour each one reproduces:
 *   ntsm_sites_*          FingerPrint::initCountsHash            src/FingerPrint.hpp:490-564
 *   ntsm_host_flatten     kseq_read loop of computeCounts        src/FingerPrint.hpp:64-69, vendor/kseq.h:177-219
 *   ntsm_host_format_*    printOptionalHeader/printCountsMax/    src/FingerPrint.hpp:261-349
 *                         printInfoSummary
 *   ntsm_host_max_hits    m_maxCounts                            src/FingerPrint.hpp:41-43
 */
#ifndef NTSM_HOST_H
#define NTSM_HOST_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ntsm_sites ntsm_sites;

/* Load a sites file.  Returns 0, or -1 if it cannot be opened.  Collision warnings go to stderr. */
int ntsm_sites_load(const char *path, unsigned k, int allow_dupes, ntsm_sites **out);
void ntsm_sites_free(ntsm_sites *s);
uint64_t ntsm_sites_n_keys(const ntsm_sites *s);          /* m_counts.size() */
const uint64_t *ntsm_sites_keys(const ntsm_sites *s);     /* canonical codes, first-seen order */
uint64_t ntsm_sites_n_sites(const ntsm_sites *s);         /* m_alleleIDs.size() */
uint64_t ntsm_sites_n_erased(const ntsm_sites *s);        /* duplicates removed (no -d) */
/* The site -> k-mer lists in the form ntsm_sites_attach takes (include/ntsm_hip.h): offsets[2 * n_sites + 1] into kmer_ix,
 * site i's AT list first, then its CG list; indices into ntsm_sites_keys.  Both arrays are released with ntsm_host_free.
 * Returns 1, with nothing allocated, for a set whose rows cannot be printed or packed (an erased k-mer in a list, a REF record
 * without VAR, a repeated locus ID: host/cohort.hpp). */
int ntsm_sites_lists(const ntsm_sites *s, uint32_t **offsets, uint32_t **kmer_ix, uint64_t *n_ix);

/* m_maxCounts for a k-mer set size and the -m value (0 = disabled / never) */
uint64_t ntsm_host_max_hits(uint64_t n_distinct, double cov_thresh);

/* Parse one FASTA/FASTQ(.gz) file into the flat stream layout of include/ntsm_hip.h.
 * Buffers are malloc'ed; release with ntsm_host_free.  *last_rc = the reader's terminating code
 * (-1 EOF, -2 truncated quality, -3 stream error).  Returns 0, or -1 if the file cannot be opened. */
int ntsm_host_flatten(const char *path, uint8_t **bases, uint64_t *n_bytes, uint64_t **read_end,
		uint64_t *n_reads, int *last_rc);
void ntsm_host_free(void *p);
/* Test hook for the packed producer lanes (ntsm_amd/csrc/host/pack2.hpp; include/ntsm_hip.h ntsm_lane_acquire_packed):
 * append one read at position pos (a multiple of 8) of a packed batch -- 2-bit codes + 1 validity bit per position, the
 * five classes of vendor/KseqHashIterator.hpp:114-127 -- and return where the next read starts.  force_scalar: 0 = the best
 * implementation the CPU has (AVX-512 VBMI, AVX2, portable), 1 = the portable one, 2 = at most AVX2. */
uint64_t ntsm_host_pack2_append(uint8_t *codes, uint8_t *valid, uint64_t pos, const uint8_t *seq, uint64_t len, int force_scalar);
const char *ntsm_host_pack2_impl(void);
/* Test hook for the gzip ingest (ntsm_amd/csrc/host/gz_stream.hpp): decode `path` with the decoder thread
 * (engine 0; engine n >= 2: with n decoder threads for BGZF input) or with zlib's gzread (engine 1), reading
 * `chunk` bytes per call.  out / len receive the bytes delivered
 * (free with ntsm_host_free); returns the last read's result: 0 = clean end, -1 = error, -2 = cannot open. */
int ntsm_host_gunzip(const char *path, int engine, unsigned chunk, uint8_t **out, uint64_t *len);
/* Test hook: compressed bytes per chunk of the parallel decoder for plain (non-BGZF) gzip input that engine n >= 2 uses
 * (0 = the default 1 MiB; files shorter than two chunks are decoded in order).  stats, if not NULL, receives what the last
 * ntsm_host_gunzip call with engine >= 2 did: [0] chunks spliced in, [1] chunks dropped (no block start found in their
 * range, start not confirmed by the in-order decoder, or decoding failed). */
void ntsm_host_gunzip_parallel_chunk(uint64_t bytes);
void ntsm_host_gunzip_parallel_stats(uint64_t stats[2]);
/* Test hook for the parallel gzip ingest (parallel_gz_fastq.hpp over gz_stream.hpp): n_decoders decoder threads inflate
 * `path`, n_parsers threads parse the pieces (sinks of sink_bytes each), the sequential reader finishes what the parallel
 * phase left.  Reads come back piece by piece; INSIDE a piece the records carried over from the previous piece may stand
 * before or between the piece's own (the counting path does not depend on read order).  Returns 0, 1 if the file is not
 * gzip, -1 if it cannot be opened.  *n_parallel = records committed by the parallel phase. */
int ntsm_host_flatten_parallel_gz(const char *path, unsigned n_decoders, unsigned n_parsers, uint64_t sink_bytes, uint8_t **bases,
		uint64_t *n_bytes, uint64_t **read_end, uint64_t *n_reads, uint64_t *n_pieces, uint64_t *n_parallel, int *final_status);
/* Test hook for the early ingest (ntsm_amd/csrc/host/early_ingest.hpp): parse `path` (plain FASTQ or gzip) into packed chunks
 * of chunk_positions positions, at most max_chunks at once, drained by n_consumers threads.  *text receives every position of
 * every chunk as 'A' 'C' 'G' 'T' (valid) or 'N' (invalid / terminator), chunks separated by 'N' -- so the maximal runs of
 * letters are the maximal runs of valid bases of the reads.  Returns 0, 1 if the file is not taken by this path. */
int ntsm_host_early_ingest(const char *path, unsigned n_parsers, unsigned n_decoders, uint64_t block_bytes, uint64_t chunk_positions, uint64_t max_chunks,
		unsigned n_consumers, uint8_t **text, uint64_t *n_text, uint64_t *n_reads, uint64_t *n_bases, uint64_t *n_parallel);
/* The same with the hand-over of a gzip stream (EarlyIngest::hand_over / release_stream): once `hand_over_after` chunks have
 * been drained the consumers ask for the stream; what it still holds is read by the sequential reader and appended to *text in
 * the same alphabet.  *n_rest = reads that came that way (0: the whole file went through the chunks, or a plain file). */
int ntsm_host_early_ingest_hand_over(const char *path, unsigned n_parsers, unsigned n_decoders, uint64_t block_bytes, uint64_t chunk_positions,
		uint64_t max_chunks, unsigned n_consumers, uint64_t hand_over_after, uint8_t **text, uint64_t *n_text, uint64_t *n_reads, uint64_t *n_bases,
		uint64_t *n_parallel, uint64_t *n_rest);
/* Thread counts of the ingest pipeline (ntsm_amd/csrc/host/host_shape.hpp): the CPUs this process is granted = min(affinity
 * mask, cgroup CPU quota), and the plan `ntsmCount -t threads_asked` follows on such a host (cpus = 0: this host's grant):
 * out = { cpus, feeders, decoders of one big .gz, decoders while the sites still load }.  feeders + decoders <= 2 x cpus. */
unsigned ntsm_host_granted_cpus(void);
void ntsm_host_ingest_plan(unsigned threads_asked, unsigned cpus, unsigned out[4]);
/* Test hook: the n-th chunk allocation of an early ingest from now on fails (0 = off).  The hooks above then return -3:
 * an allocation failure must surface as a failed run, never as a shorter one (the CLI exits 1 with a message and prints no
 * counts, like the reference for a file it cannot read: src/FingerPrint.hpp:51-57). */
void ntsm_host_debug_early_alloc_fail(long nth);
/* Test hook: the longest unparsed rest a piece of the piece-parallel gzip parse may carry into the next link (0 = the default
 * 256 MiB); a piece whose rest is longer commits what it parsed and ends the parallel phase there. */
void ntsm_host_debug_gz_max_tail(uint64_t bytes);
/* Block-parallel variant for plain 4-line FASTQ (ntsm_amd/csrc/host/parallel_fastq.hpp), for tests: the records
 * the parallel phase commits (in file order) followed by what the sequential reader yields from *resume on.
 * Returns 0, 1 if the file is not eligible (callers use ntsm_host_flatten), -1 if it cannot be opened.
 * *n_parallel = records parsed by the parallel phase; *resume = byte offset it stopped at (file size if complete). */
int ntsm_host_flatten_parallel(const char *path, unsigned n_threads, uint64_t block_bytes, uint8_t **bases,
		uint64_t *n_bytes, uint64_t **read_end, uint64_t *n_reads, uint64_t *n_blocks, uint64_t *n_parallel,
		uint64_t *resume);

/* counts.txt bytes for per-k-mer counts in key order.  Returns 0, or 1 if the reference would
 * abort while printing (then *out holds the rows written before the abort). */
int ntsm_host_format_counts(const ntsm_sites *s, const uint64_t *counts, uint64_t total_kmers,
		char **out, size_t *len);
/* six-line summary; *covered receives "Sites Covered by at least one k-mer". */
int ntsm_host_format_summary(const ntsm_sites *s, const uint64_t *counts, uint64_t total_bases,
		uint64_t total_kmers, uint64_t total_hits, char **out, size_t *len, uint64_t *covered);

/* The per-site table of `ntsmEval --qc --sites-out` (ntsm_amd/csrc/host/eval_qc.hpp), header line included, for tests:
 * locus[n_sites] IDs, tally [n_sites][4] = homAT, homCG, het, miss and site_cov [n_sites] as ntsm_eval_store_profile gives them
 * (include/ntsm_eval_hip.h).  *out is freed with ntsm_host_free.  Returns 0, -1 for a NULL it needs. */
int ntsm_host_site_table(const char *const *locus, uint32_t n_sites, const uint32_t *tally, const uint64_t *site_cov, uint64_t n_samples,
		char **out, size_t *len);

/* The tables of `ntsmEval --contam` (ntsm_amd/csrc/host/eval_contam.hpp), for tests.  _rows: the lines of the band of targets
 * row_first ... row_first + n_rows - 1 as stdout has them, without the header: names[n_db]; rec [n_rows][n_db] and tally
 * [n_rows][3] as ntsm_eval_contam_rows gives them (include/ntsm_eval_hip.h; rec is an array of its 64-byte records); all,
 * min_excess, min_explained = -a, --contam-min, --contam-explained.  _sample_table: the --samples-out file, header line included,
 * tally [n_samples][3].  *out is freed with ntsm_host_free.  Both return 0, -1 for a NULL they need or a band past n_db.
 * _band_rows: the band rule, the targets a band from row_first takes under `limit` records; 0 where there is no such row. */
struct ntsm_eval_contam_record;
int ntsm_host_contam_rows(const char *const *names, uint32_t n_db, uint32_t row_first, uint32_t n_rows, const struct ntsm_eval_contam_record *rec,
		const uint64_t *tally, int all, double min_excess, double min_explained, char **out, size_t *len);
int ntsm_host_contam_sample_table(const char *const *names, uint32_t n_samples, const uint64_t *tally, char **out, size_t *len);
uint32_t ntsm_host_contam_band_rows(uint32_t row_first, uint32_t n_db, uint64_t limit);

/* The host side of `ntsmEval --trios` (ntsm_amd/csrc/host/eval_trio.hpp), for tests; records as include/ntsm_eval_hip.h has them.
 * _rows: the lines of n_rows evaluated triples (child[i]; pa[i], pb[i]), indices into names[n_names], with their trio records
 *   and the duo records (child, parentA) and (child, parentB), without the header.  ped != 0: every line, with its verdict;
 *   else the search's print rule under all, min_called, max_rate.  0, -1 for a NULL it needs or an index >= n_names.
 * _ped_parse: the complete trios of a pedigree file's text as samples of names[], *trios [*n_trios][3] = child, father,
 *   mother in file order; *comments and *founders (may be NULL) = the skipped lines.  0; 1 for a refusal, its sentence in
 *   *error; -1 for a NULL it needs.  *trios and *error are freed with ntsm_host_free.
 * _match: the sample an ID names (stored name, then basename, then the basename without _counts.txt / .counts.txt / .txt),
 *   -1 where none does, -2 where more than one does at the first level any does, -3 for a NULL.
 * _candidates: the candidate parents of `child` out of its duo row [n_db], in store order, into out [n_db]; returns how many,
 *   -1 for a NULL it needs.
 * _batches: lists of lengths k[n] cut into batches of at most `limit` records, the batches' ends into ends [n] and their
 *   number into *n_ends; returns n, or the position of a list that alone exceeds the limit, or SIZE_MAX for a NULL k.
 * The band rule of the duo rectangle is ntsm_host_contam_band_rows, asked at 2^27 records (1 GiB of 8 bytes). */
struct ntsm_eval_trio_record;
struct ntsm_eval_trio_duo;
int ntsm_host_trio_rows(const char *const *names, uint32_t n_names, size_t n_rows, const uint32_t *child, const uint32_t *pa, const uint32_t *pb,
		const struct ntsm_eval_trio_record *rec, const struct ntsm_eval_trio_duo *da, const struct ntsm_eval_trio_duo *db, int ped, int all,
		uint32_t min_called, double max_rate, char **out, size_t *len);
int ntsm_host_trio_ped_parse(const char *text, size_t text_len, const char *const *names, uint32_t n_names, uint32_t **trios, size_t *n_trios,
		uint64_t *comments, uint64_t *founders, char **error, size_t *error_len);
int64_t ntsm_host_trio_match(const char *const *names, uint32_t n_names, const char *id);
int64_t ntsm_host_trio_candidates(const struct ntsm_eval_trio_duo *row, uint32_t n_db, uint32_t child, uint32_t min_called, double max_duo, uint32_t *out);
size_t ntsm_host_trio_batches(const uint32_t *k, size_t n, uint64_t limit, size_t *ends, size_t *n_ends);

/* The host side of `ntsmEval --ld` (ntsm_amd/csrc/host/eval_ld.hpp), for tests; records as include/ntsm_eval_hip.h has them.
 * _r2: the moments of a record into moments [4] = n, cov, vx, vy (may be NULL); 1 and *r2 where r^2 is defined at min_called,
 *   0 where it is not (*r2 untouched), -1 for a NULL record.
 * _rows: the lines of these pairs in their order, locus[n_sites] the store's IDs, without the header.  0, -1 for a NULL it
 *   needs or an index >= n_sites.
 * _prune: kept [n_sites] = 1 / 0 after these pairs, which are in (a, b) order: b is dropped when the pair is selected at
 *   (min_called, r2_min) and a is kept.  0, -1.
 * _bands: the band walk over a model of the device that selects row_pairs[a] pairs in row a: every call's first row, rows and
 *   return (0, or 1 = more than the capacity) into calls [max_calls][3]; stats [3] (may be NULL) = bands, re-runs, pairs.
 *   Returns the number of calls, -1 for a NULL it needs. */
struct ntsm_eval_ld_record;
struct ntsm_eval_ld_pair;
int ntsm_host_ld_r2(const struct ntsm_eval_ld_record *rec, uint32_t min_called, int64_t *moments, double *r2);
int ntsm_host_ld_rows(const char *const *locus, uint32_t n_sites, const struct ntsm_eval_ld_pair *pairs, uint64_t n_pairs, char **out, size_t *len);
int ntsm_host_ld_prune(uint32_t n_sites, const struct ntsm_eval_ld_pair *pairs, uint64_t n_pairs, uint32_t min_called, double r2_min, uint8_t *kept);
int64_t ntsm_host_ld_bands(const uint64_t *row_pairs, uint32_t n_sites, uint64_t budget, uint32_t *calls, size_t max_calls, uint64_t *stats);

#ifdef __cplusplus
}
#endif
#endif
