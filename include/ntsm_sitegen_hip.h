/*
 * include/ntsm_sitegen_hip.h -- C ABI of the MI355X (gfx950) device step of ntsmSiteGen: for every candidate k-mer, the
 * number of places of a genome it matches with at most x substitutions (x = 0 or 1).
 *
 * Upstream's site generation (ntsm-scripts/makefile) asks this of `bwa aln -n 1` + `bwa samse` and reads the answer out of
 * the SAM tags X0 + X1 (ntsm-scripts/filterRepetiveSNP.pl:35-40).  This library answers it with a scan of the genome
 * against tables of the candidates; DESIGN.md section 13 has the method and the two intended deviations (substitutions
 * only, a byte outside ACGTacgt never matches).
 *
 * Definition.  A candidate q is a string of k bases over ACGT.  A genome window is k consecutive bytes of one record,
 * each of them one of ACGTacgt (case is ignored).  H(q) = the number of (window, strand) pairs with Hamming distance <= x
 * between q and the window (forward strand) or the window's reverse complement (reverse strand).  The library returns
 * min(H(q), 255) per candidate, in candidate order; duplicate candidates each get their own count.  Counts are integers
 * added with atomics, so the result is the same on every run.
 *
 * Packing of a candidate: base i (0 = leftmost) in bits 2(k-1-i) .. 2(k-1-i)+1 of a uint64_t, A = 0, C = 1, G = 2, T = 3,
 * forward orientation as the caller wants it reported (the library indexes the reverse complement itself).
 *
 * All functions return 0, -1 for a bad argument, -2 for a HIP error.
 *
 * Places that differ by a one-base gap (`ntsmSiteGen -g`) are counted by a second library: include/ntsm_sitegen_gap_hip.h.
 */
#ifndef NTSM_SITEGEN_HIP_H
#define NTSM_SITEGEN_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ntsm_sitegen ntsm_sitegen;   /* one session: one candidate set on one device */

typedef struct ntsm_sitegen_times {         /* milliseconds; upload / table build wall clock, kernel from HIP events */
	double table_build_ms;                   /* host: bucket sort of the three tables */
	double table_upload_ms;                  /* tables and bitmaps to the device */
	double stage_ms;                         /* host: genome bytes into the pinned staging buffer (separators, seam tails) */
	double upload_ms;                        /* genome bytes to the device */
	double kernel_ms;                        /* the scan kernel, summed over launches */
	double full_kernel_ms_min, full_kernel_ms_max;   /* over the launches on a full staging buffer (128 MiB), 0 if none */
	uint64_t launches, full_launches;
	uint64_t windows;                        /* valid windows scanned (k bases of ACGTacgt inside one record) */
	uint64_t bitmap_tests;                   /* bitmap bits read: 3 per window at x = 1, 1 at x = 0 */
	uint64_t probes;                         /* bucket entries compared (a window whose bit is clear compares none) */
	uint64_t genome_bytes;                   /* bytes submitted */
	uint64_t table_bytes;                    /* device bytes of tables + bitmaps */
} ntsm_sitegen_times;

/*
 * cands: host [n_cands] packed candidates (may be NULL when n_cands = 0: every submit is then a no-op scan).
 * k: 11 .. 31.  x: 0 or 1.  n_cands < 2^30.
 */
int ntsm_sitegen_open(int device, uint32_t k, uint32_t x, uint64_t n_cands, const uint64_t *cands, ntsm_sitegen **out);

/*
 * A chunk of genome: n bytes, the text of FASTA records without line ends.  ends[0 .. n_ends) are the ascending offsets
 * (0 .. n, exclusive ends; 0 ends the record that the previous chunk left open) at which a record ends inside this
 * chunk; bytes after the last end belong to a record that goes on in the next submit.  The session carries the last k - 1 bytes of an open record over to the next call, so a
 * window that crosses a chunk seam inside a record is counted exactly once and a genome of any size streams through bounded
 * staging.  A window never crosses a record end.  The call returns after the chunk's kernels have finished.
 */
int ntsm_sitegen_submit(ntsm_sitegen *s, const char *bases, uint64_t n, const uint64_t *ends, uint64_t n_ends);

/* hits: host out [n_cands], min(H, 255) of everything submitted so far */
int ntsm_sitegen_hits(ntsm_sitegen *s, uint8_t *hits);

int ntsm_sitegen_times_get(ntsm_sitegen *s, ntsm_sitegen_times *out);

void ntsm_sitegen_close(ntsm_sitegen *s);

#ifdef __cplusplus
}
#endif
#endif
