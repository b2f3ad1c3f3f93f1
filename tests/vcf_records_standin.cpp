/*
 * tests/vcf_records_standin.cpp -- a plain, single-threaded C++ definition of ntsm_vcf_records, written from the text of
 * include/ntsm_vcf_hip.h alone and linked beside tests/vcf_step_standin.cpp, so that `ntsmVCF --counts / --store`
 * (ntsm_amd/csrc/host/ntsm_vcf_main.cpp) can be built and run on a CPU under ASan / UBSan (tests/test_vcf_counts.py).  It
 * shares no code with ntsm_amd/csrc/ntsm_vcf.hip: per sample of the window, per site, per list, per key it walks the key's
 * events in the order they are stored with the insert rule of the header and takes the maximum and the sum of the final
 * bytes.  Only the 8 * n_sites bytes of a row are written, at the caller's pitch.
 */
#include <cstddef>
#include <cstring>

#include "../include/ntsm_vcf_hip.h"

extern "C" int ntsm_vcf_records(int device, uint32_t n_samples, uint32_t multi, uint64_t n_lines, const uint8_t *geno, uint32_t g_stride,
		uint64_t n_keys, const uint64_t *key_off, uint64_t n_events, const uint32_t *ev_ord, const uint32_t *ev_ls, uint64_t n_sites,
		const uint64_t *site_off, const uint32_t *site_keys, uint32_t s_begin, uint32_t s_count, uint32_t *counts, uint64_t counts_pitch,
		uint32_t *sums, uint64_t sums_pitch, uint64_t *total, uint64_t *sum_of_sums, ntsm_vcf_records_times *times)
{
	(void) ev_ord;
	if (device < 0 || g_stride % 16 || g_stride < n_samples || !key_off || !site_off || !total || !sum_of_sums) return -1;
	if (key_off[n_keys] != n_events) return -1;
	if (s_begin % 16 || s_count < 1 || (uint64_t) s_begin + s_count > n_samples) return -1;
	if (counts_pitch % 8 || counts_pitch < 8 * n_sites || (sums && (sums_pitch % 8 || sums_pitch < 8 * n_sites))) return -1;
	const uint32_t m1 = multi, m2 = multi * 2u;                  /* m and 2m in unsigned 32-bit arithmetic */
	for (uint32_t j = 0; j < s_count; ++j) {
		const uint32_t sample = s_begin + j;
		uint64_t tot = 0, sos = 0;
		for (uint64_t s = 0; s < n_sites; ++s) {
			uint32_t best[2] = { 0, 0 }, sum[2] = { 0, 0 };
			for (int list = 0; list < 2; ++list)
				for (uint64_t at = site_off[2 * s + list]; at < site_off[2 * s + list + 1]; ++at) {
					const uint64_t q = site_keys[at];
					if (q >= n_keys) return -1;
					uint8_t byte = 0;
					for (uint64_t e = key_off[q]; e < key_off[q + 1]; ++e) {
						const uint64_t line = ev_ls[e] >> 1;
						const int side = ev_ls[e] & 1;
						if (line >= n_lines) return -1;
						const int code = geno[line * g_stride + sample];
						uint32_t value;
						if (code == NTSM_VCF_HET) value = m1;
						else if (code == (side ? NTSM_VCF_HOM2 : NTSM_VCF_HOM1)) value = m2;
						else continue;                                 /* no insert */
						if (byte == 0) byte = (uint8_t) value;         /* a non-zero byte is kept */
					}
					if (byte > best[list]) best[list] = byte;
					sum[list] += byte;
				}
			memcpy((char *) counts + j * counts_pitch + 8 * s, best, 8);
			if (sums) memcpy((char *) sums + j * sums_pitch + 8 * s, sum, 8);
			tot += (uint32_t) (best[0] + best[1]);
			sos += (uint32_t) (sum[0] + sum[1]);
		}
		total[j] = tot;
		sum_of_sums[j] = sos;
	}
	if (times) *times = ntsm_vcf_records_times {};
	return 0;
}
