/*
 * tests/vcf_step_standin.cpp -- a plain, single-threaded C++ definition of ntsm_vcf_run, written from the text of
 * include/ntsm_vcf_hip.h alone, so that the whole ntsmVCF program (ntsm_amd/csrc/host/ntsm_vcf_main.cpp) can be built
 * and run on a CPU, under ASan / UBSan (tests/test_vcf.py).  It shares no code with ntsm_amd/csrc/ntsm_vcf.hip: per
 * list of a site, per key, per sample it walks the key's events in the order they are stored (ascending ordinals) with
 * the insert rule of the header, then takes the maxima, the sequential double sum and first_undef.
 * With NTSM_STANDIN_FIRST_CAP=K in the environment the first call behaves as if warn_cap were at most K, so that a test
 * reaches the caller's NTSM_VCF_E_CAPACITY round trip without a million warnings.
 * ntsm_pca_run_cells is defined to fail with the HIP-error code: --rotation has no CPU form.
 * Compile with -ffp-contract=off (the sum is a sequence of IEEE divisions and additions).
 */
#include <cstddef>
#include <cstdlib>
#include <vector>

#include "../include/ntsm_pca_hip.h"
#include "../include/ntsm_vcf_hip.h"

extern "C" int ntsm_vcf_run(int device, uint32_t n_samples, uint32_t multi, uint64_t n_lines, const uint8_t *geno, uint32_t g_stride,
		uint64_t n_keys, const uint64_t *key_off, uint64_t n_events, const uint32_t *ev_ord, const uint32_t *ev_ls, uint64_t n_sites,
		const uint64_t *site_off, const uint32_t *site_keys, uint16_t *cells, double *sums, uint32_t *first_undef,
		ntsm_vcf_warning *warn, uint64_t warn_cap, uint64_t *n_warn, ntsm_vcf_times *times)
{
	if (device < 0 || g_stride % 16 || g_stride < n_samples || !key_off || !site_off || !n_warn) return -1;
	if (key_off[n_keys] != n_events) return -1;
	const uint32_t m1 = multi, m2 = multi * 2u;                  /* m and 2m in unsigned 32-bit arithmetic */
	std::vector<ntsm_vcf_warning> found;
	std::vector<uint8_t> best((size_t) n_sites * 2 * n_samples, 0);   /* [site][side][sample]: the maxima */
	for (uint64_t l = 0; l < 2 * n_sites; ++l)
		for (uint64_t at = site_off[l]; at < site_off[l + 1]; ++at) {
			const uint64_t q = site_keys[at];
			if (q >= n_keys) return -1;
			for (uint32_t j = 0; j < n_samples; ++j) {
				uint8_t byte = 0;
				for (uint64_t e = key_off[q]; e < key_off[q + 1]; ++e) {
					const uint64_t line = ev_ls[e] >> 1;
					const int side = ev_ls[e] & 1;
					if (line >= n_lines) return -1;
					const int code = geno[line * g_stride + j];
					uint32_t value;
					if (code == NTSM_VCF_HET) value = m1;
					else if (code == (side ? NTSM_VCF_HOM2 : NTSM_VCF_HOM1)) value = m2;
					else continue;                                     /* no insert */
					if (byte != 0 && byte != value) found.push_back(ntsm_vcf_warning { ev_ord[e], j, byte, value });
					else byte = (uint8_t) value;
				}
				uint8_t &b = best[(size_t) l * n_samples + j];
				if (byte > b) b = byte;
			}
		}
	*n_warn = found.size();
	static int calls = 0;                                        /* NTSM_STANDIN_FIRST_CAP=K: the first call has room for K only */
	const char *first_cap = getenv("NTSM_STANDIN_FIRST_CAP");
	if (calls++ == 0 && first_cap && (uint64_t) atoll(first_cap) < warn_cap) warn_cap = (uint64_t) atoll(first_cap);
	if (found.size() > warn_cap) return NTSM_VCF_E_CAPACITY;
	for (size_t i = 0; i < found.size(); ++i) warn[i] = found[i];
	for (uint64_t s = 0; s < n_sites; ++s) {
		double sum = 0.0;
		uint32_t undef = n_samples;
		for (uint32_t j = 0; j < n_samples; ++j) {
			const unsigned r = best[(size_t) (2 * s) * n_samples + j], v = best[(size_t) (2 * s + 1) * n_samples + j];
			cells[s * n_samples + j] = (uint16_t) (r | v << 8);
			if (r + v) sum += double(r) / double(r + v);
			else if (undef == n_samples) undef = j;
		}
		sums[s] = sum;
		first_undef[s] = undef;
	}
	if (times) {
		*times = ntsm_vcf_times {};
		times->state_launches = 1;
	}
	return 0;
}

extern "C" int ntsm_pca_run_cells(int, uint64_t, uint32_t, const uint16_t *, const double *, const double *, uint64_t, uint32_t, uint32_t,
		double *, double *, double *, uint32_t *, ntsm_pca_times *, double *)
{
	return NTSM_PCA_E_HIP;
}
