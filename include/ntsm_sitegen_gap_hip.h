/*
 * include/ntsm_sitegen_gap_hip.h -- C ABI of the second device library of ntsmSiteGen (`ntsmSiteGen -g`): for every
 * candidate k-mer, in one pass over the genome, H = the places it matches with at most one substitution (exactly the
 * x = 1 count of include/ntsm_sitegen_hip.h) and G = the places it matches with one one-base gap.
 *
 * Upstream asks `bwa aln -n 1` for the places of a candidate, and the one difference bwa allows may be a gap of one base;
 * filterRepetiveSNP.pl then drops a candidate with X0 + X1 > 1.  The end margin e mirrors `bwa aln -i 5` (no gap within
 * 5 bases of either end).  Beyond that the definition below is this project's own: parity with a real bwa run is unpinned.
 *
 * Definition.  q is a candidate of k bases over ACGT.  e is the end margin, 1 <= e and 2e <= k - 1.  A window is a run of
 * consecutive bytes of one record, each of them one of ACGTacgt (case is ignored), as in include/ntsm_sitegen_hip.h.
 * Half-open ranges of 0-based positions:
 *   a long window g, of k + 1 bases, is a gapped place of q if some p with e <= p <= k - e has
 *       g[0, p) = q[0, p)  and  g[p + 1, k + 1) = q[p, k)          (the genome holds one base more, at position p);
 *   a short window g, of k - 1 bases, is a gapped place of q if some p with e <= p <= k - 1 - e has
 *       g[0, p) = q[0, p)  and  g[p, k - 1) = q[p + 1, k)          (the genome lacks base p of q);
 *   reverse strand: the same with the reverse complement of q against g.
 * G(q) = the number of (window, strand) pairs that are gapped places.  A window counts once per strand however many p
 * qualify: a gap inside a homopolymer run is one place.  Long and short windows are not reconciled with each other, nor
 * with H.  Consequence: a k-mer whose own suffix or prefix of at least e bases is a homopolymer gains a gapped place
 * beside its exact one (its exact place and the genome's next base, where that continues the run, are a long window of
 * it; with a run of e + 1 bases its exact place less the last base is a short one).  Such a k-mer is low-complexity;
 * dropping it is intended.
 *
 * The library returns min(H, 255) and min(G, 255) as two arrays, in candidate order; duplicate candidates each get their
 * own counts.  Counts are integers added with atomics, so the result is the same on every run.
 *
 * Packing of a candidate, chunks, record ends and return codes (0, -1 for a bad argument, -2 for a HIP error) are those
 * of include/ntsm_sitegen_hip.h.
 */
#ifndef NTSM_SITEGEN_GAP_HIP_H
#define NTSM_SITEGEN_GAP_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ntsm_sitegap ntsm_sitegap;   /* one session: one candidate set on one device */

struct ntsm_sitegap_stats {                 /* the time fields of ntsm_sitegen_times, then the counts; the function below has
                                             the name, so the type is always written `struct ntsm_sitegap_stats` */
	double table_build_ms;                   /* host: bucket sort of the three tables */
	double table_upload_ms;                  /* tables and bitmaps to the device */
	double stage_ms;                         /* host: genome bytes into the pinned staging buffer (separators, seam tails) */
	double upload_ms;                        /* genome bytes to the device */
	double kernel_ms;                        /* the scan kernel, summed over launches */
	double full_kernel_ms_min, full_kernel_ms_max;   /* over the launches on a full staging buffer (128 MiB), 0 if none */
	uint64_t launches, full_launches;
	uint64_t windows;                        /* valid windows of k bases (ACGTacgt, inside one record) */
	uint64_t windows_long;                   /* valid windows of k + 1 bases */
	uint64_t windows_short;                  /* valid windows of k - 1 bases */
	uint64_t bitmap_tests;                   /* bitmap bits read; derived on the host from the three window counts: 7 at a byte that ends a window of each length */
	uint64_t probes;                         /* bucket entries compared */
	uint64_t genome_bytes;                   /* bytes submitted */
	uint64_t table_bytes;                    /* device bytes of tables + bitmaps */
};

/*
 * cands: host [n_cands] packed candidates (may be NULL when n_cands = 0).  k: 11 .. 31.  e: 1 .. (k - 1) / 2.
 * n_cands < 2^30.
 */
int ntsm_sitegap_open(int device, uint32_t k, uint32_t e, uint64_t n_cands, const uint64_t *cands, ntsm_sitegap **out);

/*
 * A chunk of genome, as ntsm_sitegen_submit takes it.  The session carries the last k bytes of an open record over to the
 * next launch (a long window needs k bytes before its last one), and a window of any of the three lengths belongs to the
 * launch in which its last byte is new: it is counted exactly once wherever the chunk seams fall.  No window crosses a
 * record end.  The call returns after the chunk's kernels have finished.
 */
int ntsm_sitegap_submit(ntsm_sitegap *s, const char *bases, uint64_t n, const uint64_t *ends, uint64_t n_ends);

/* sub, gap: host out [n_cands] each, min(H, 255) and min(G, 255) of everything submitted so far */
int ntsm_sitegap_hits(ntsm_sitegap *s, uint8_t *sub, uint8_t *gap);

int ntsm_sitegap_stats(ntsm_sitegap *s, struct ntsm_sitegap_stats *out);

void ntsm_sitegap_close(ntsm_sitegap *s);

#ifdef __cplusplus
}
#endif
#endif
