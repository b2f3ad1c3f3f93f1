/*
 * include/ntsm_vcf_hip.h -- C ABI of the MI355X (gfx950) device step of ntsmVCF (the reference's src/ntSeqMatchVCF.cpp,
 * src/VCFConvert.hpp, src/MultiCount.hpp).
 *
 * The reference fills a sample x k-mer byte matrix by one MultiCount::insertCount call per (window k-mer, sample)
 * (VCFConvert::count, VCFConvert.hpp:151-170), then walks the matrix again per (site, sample) for the maxima of the
 * site's REF and VAR k-mers (MultiCount::printNormMatrix, MultiCount.hpp:162-187).  This library replaces both passes.
 * The caller (ntsm_amd/csrc/host/ntsm_vcf_main.cpp) parses the VCF and turns every window k-mer that is a key into an
 * EVENT: (ordinal, line, side), ordinals counting the events in the reference's one-thread insertion order (lines in
 * file order; per line the REF window's k-mers in position order, then the VAR window's).  Events are grouped by key
 * (CSR), each key's list ascending in ordinal.  Because every key lies in exactly one allele list
 * (MultiCount::initCountsHash, :236-270), the byte state of a (key, sample) is computed exactly once, by the workgroup
 * of its site, with no sample x k-mer matrix and no atomics on the state: the result is deterministic.
 *
 * Per (key, sample), in ordinal order, an event of side REF inserts 2m for hom1 and m for het, one of side VAR inserts
 * 2m for hom2 and m for het (VCFConvert.hpp:151-170, m = -m, 2m in unsigned 32-bit arithmetic); insertCount
 * (MultiCount.hpp:51-68): a stored byte that is non-zero and differs from the untruncated value gives a warning and is
 * kept; otherwise the byte becomes (uint8_t) value.  The cell of (site, sample) is maxREF | maxVAR << 8, the maxima of
 * the final bytes over the site's REF and VAR keys (:163-178).  Per site, sum is the sequential IEEE double sum in sample
 * order of double(maxREF) / double(maxREF + maxVAR) over the cells with a non-zero denominator (:179-186; correctly
 * rounded division, no contraction), and first_undef the first sample whose denominator is 0 (n_samples if none).
 */
#ifndef NTSM_VCF_HIP_H
#define NTSM_VCF_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* genotype codes of a G row (VCFConvert.hpp:99, 137-148); NTSM_VCF_PAD marks the padding bytes of a row: no insert */
enum { NTSM_VCF_HOM1 = 0, NTSM_VCF_HET = 1, NTSM_VCF_HOM2 = 2, NTSM_VCF_PAD = 3 };

typedef struct ntsm_vcf_warning {   /* "Warning: Inconsistent k-mer counts ...: <old as char> vs <value>" (MultiCount.hpp:59) */
	uint32_t event;                  /* ordinal of the insert's event */
	uint32_t sample;
	uint32_t old;                    /* the stored byte */
	uint32_t value;                  /* the untruncated value of the insert */
} ntsm_vcf_warning;

typedef struct ntsm_vcf_times {     /* milliseconds; upload / download wall clock, kernels from HIP events */
	double upload_ms, state_kernel_ms, sum_kernel_ms, download_ms;
	uint64_t kernel_bytes;           /* bytes the state kernel reads and writes at least once (G rows, lists, cells) */
	uint64_t state_launches;         /* 1, or 2 when the device's warning buffer had to grow (the kernels ran again) */
} ntsm_vcf_times;

/*
 * geno:      host [n_lines][g_stride] genotype codes; g_stride a multiple of 16, >= n_samples; bytes past n_samples are
 *            NTSM_VCF_PAD.  A "line" is one used VCF line (one with at least one event).
 * key_off:   host [n_keys + 1]: the events of key q are ev_ord / ev_ls [key_off[q], key_off[q + 1]), ascending ordinals.
 * ev_ord:    host [n_events] event ordinals (< 2^32).
 * ev_ls:     host [n_events] line * 2 + side (side 0 = REF window, 1 = VAR window).
 * site_off:  host [2 * n_sites + 1]: site s's REF keys are site_keys[site_off[2s], site_off[2s + 1]), its VAR keys
 *            site_keys[site_off[2s + 1], site_off[2s + 2]).  Every key with events must lie in exactly one list: a
 *            key's events are walked once per list it is in, so a key in no list gives no warnings.
 * cells:     host out [n_sites][n_samples] maxREF | maxVAR << 8.
 * sums:      host out [n_sites];  first_undef: host out [n_sites].
 * warn:      host out, room for warn_cap records; *n_warn = the number of warnings (any order; sort by (event, sample)
 *            for the one-thread order).  If *n_warn > warn_cap nothing is written to warn, the call returns
 *            NTSM_VCF_E_CAPACITY and the caller calls again with room for *n_warn.  On the device the records go to a
 *            buffer of min(warn_cap, 65536) records; when more arrive it is grown to their number and both kernels run
 *            again (times->state_launches = 2), before any result is copied back.
 * times:     may be NULL.
 * Returns 0, -1 bad argument, -2 HIP error, NTSM_VCF_E_CAPACITY.
 */
enum { NTSM_VCF_E_CAPACITY = -3 };
int ntsm_vcf_run(int device, uint32_t n_samples, uint32_t multi,
		uint64_t n_lines, const uint8_t *geno, uint32_t g_stride,
		uint64_t n_keys, const uint64_t *key_off, uint64_t n_events, const uint32_t *ev_ord, const uint32_t *ev_ls,
		uint64_t n_sites, const uint64_t *site_off, const uint32_t *site_keys,
		uint16_t *cells, double *sums, uint32_t *first_undef,
		ntsm_vcf_warning *warn, uint64_t warn_cap, uint64_t *n_warn, ntsm_vcf_times *times);

/*
 * The counts records of a window of samples (MultiCount::printCountsMax, MultiCount.hpp:93-138): per (sample, site) the
 * two maxima of ntsm_vcf_run's cell and the two sums of the same final state bytes, sample-major, plus each sample's two
 * totals as a cohort store's record holds them (ntsm_amd/csrc/host/eval_store.hpp).  The insert rule is ntsm_vcf_run's;
 * warnings are not reported here (ntsm_vcf_run is their source).  All results are exact integers; the order in which the
 * device adds the totals cannot change them.
 */
typedef struct ntsm_vcf_records_times {   /* milliseconds; upload / download wall clock, the kernel from HIP events */
	double upload_ms, kernel_ms, download_ms;
	uint64_t kernel_bytes;           /* bytes the kernel reads and writes at least once (the window's G columns, lists, records) */
	uint64_t upload_bytes, download_bytes;
} ntsm_vcf_records_times;

/*
 * n_samples, multi, n_lines, geno, g_stride, n_keys, key_off, n_events, ev_ord, ev_ls, n_sites, site_off, site_keys:
 *            as for ntsm_vcf_run, with the same checks (ev_ord is not read: the lists are already in ordinal order).
 * s_begin:   first sample of the window, a multiple of 16.
 * s_count:   samples in the window, >= 1, s_begin + s_count <= n_samples.  Only the window's columns of geno are
 *            uploaded (one 2-D copy of s_count rounded up to 16 bytes per line).
 * counts:    host out: for sample j of the window (j = 0 is sample s_begin), n_sites pairs of uint32 (maxREF, maxVAR)
 *            at (char *) counts + j * counts_pitch.  Bytes of a row past 8 * n_sites are not written.
 * counts_pitch: bytes from one sample's row to the next; a multiple of 8, >= 8 * n_sites.
 * sums:      host out, may be NULL: the same shape, (sumREF, sumVAR) = the 32-bit sums over the site's REF / VAR keys
 *            of the final state bytes (the truncated uint8 values).
 * sums_pitch: as counts_pitch, for sums; not read when sums is NULL.
 * total:     host out [s_count]: sum over the sites of uint32(maxREF + maxVAR).
 * sum_of_sums: host out [s_count]: sum over the sites of uint32(sumREF + sumVAR); written whether or not sums is NULL.
 * times:     may be NULL.
 * Returns 0, -1 bad argument, -2 HIP error.
 */
int ntsm_vcf_records(int device, uint32_t n_samples, uint32_t multi,
		uint64_t n_lines, const uint8_t *geno, uint32_t g_stride,
		uint64_t n_keys, const uint64_t *key_off, uint64_t n_events, const uint32_t *ev_ord, const uint32_t *ev_ls,
		uint64_t n_sites, const uint64_t *site_off, const uint32_t *site_keys,
		uint32_t s_begin, uint32_t s_count,
		uint32_t *counts, uint64_t counts_pitch, uint32_t *sums, uint64_t sums_pitch,
		uint64_t *total, uint64_t *sum_of_sums, ntsm_vcf_records_times *times);

#ifdef __cplusplus
}
#endif
#endif
