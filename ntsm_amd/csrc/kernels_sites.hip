/*
 * kernels_sites.hip -- from a context's dense per-k-mer count vector to the per-site record of a sample, on the device:
 * what printCountsMax (src/FingerPrint.hpp:270-311) and getSitesCoveredInSample (:389-413, printed by printInfoSummary,
 * :313-349) compute on the host from m_counts, and the two sums ntsmEval forms when it reads the printed rows back
 * (src/CompareCounts.hpp:104-106, :1198-1216).  The entry points are ntsm_sites_attach / ntsm_sites_reduce
 * (include/ntsm_hip.h); a cohort run (`ntsmCount --cohort`) downloads 16 bytes per site instead of 8 bytes per k-mer.
 *
 * One thread per (site, allele) list: lists are short (a site keeps at most 2k - 1 k-mers per allele) and the whole step is
 * microseconds of work -- it exists for what it saves around it, not for its own speed.  The two lists of a site sit in
 * neighbouring lanes, so the per-site terms of the totals are formed with one lane exchange; the totals are integer sums,
 * added per workgroup and then with one atomic per workgroup and total: the result does not depend on the order.
 */
#include <algorithm>

#include "kernels_common.h"
#include "ntsm_internal.h"

namespace {

constexpr int kSiteThreads = 256;                  /* 4 waves; 128 sites per workgroup */

/* vec: the context's d_vec; off: 2 * n_sites + 1 offsets into ix; list t = 2 * site + allele */
__global__ __launch_bounds__(kSiteThreads) void ntsm_sites_kernel(const unsigned long long *__restrict__ vec, const uint32_t *__restrict__ off,
		const uint32_t *__restrict__ ix, uint32_t n_lists, uint32_t *__restrict__ counts, uint32_t *__restrict__ sums,
		unsigned long long *__restrict__ totals)
{
	__shared__ unsigned long long part[3][kSiteThreads / 64];
	const uint32_t t = blockIdx.x * (uint32_t) kSiteThreads + threadIdx.x;
	uint32_t mx = 0, sm = 0, covered = 0;
	if (t < n_lists) {
		const uint32_t hi = off[t + 1];
		for (uint32_t j = off[t]; j < hi; ++j) {
			const unsigned long long v = vec[ix[j]];
			const uint32_t f = (uint32_t) v;           /* `unsigned freq = m_counts.at(..)`: the row shows the count mod 2^32 (:282) */
			mx = mx < f ? f : mx;
			sm += f;
			covered |= v != 0 ? 1u : 0u;               /* the 64-bit count decides (:399-405) */
		}
		counts[t] = mx;
		if (sums) sums[t] = sm;
	}
	/* the other allele of the same site: lane ^ 1 (n_lists is even, so a site is never split by the bound) */
	const uint32_t mx2 = (uint32_t) __shfl_xor((int) mx, 1, 64), sm2 = (uint32_t) __shfl_xor((int) sm, 1, 64);
	const uint32_t cov2 = (uint32_t) __shfl_xor((int) covered, 1, 64);
	unsigned long long a = 0, b = 0, c = 0;
	if ((threadIdx.x & 1) == 0 && t < n_lists) {
		a = (uint32_t) (mx + mx2);                     /* unsigned + unsigned wraps, then widens (src/CompareCounts.hpp:104-106) */
		b = (uint32_t) (sm + sm2);
		c = covered | cov2;
	}
	a = ntsm_wave_sum(a);
	b = ntsm_wave_sum(b);
	c = ntsm_wave_sum(c);
	const int wave = threadIdx.x >> 6;
	if ((threadIdx.x & 63) == 0) { part[0][wave] = a; part[1][wave] = b; part[2][wave] = c; }
	__syncthreads();
	if (threadIdx.x < 3) {
		unsigned long long s = 0;
		for (int w = 0; w < kSiteThreads / 64; ++w) s += part[threadIdx.x][w];
		if (s) atomicAdd(totals + threadIdx.x, s);
	}
}

void sites_release(ntsm_ctx *c)
{
	void *ptrs[] = { c->d_site_off, c->d_site_ix, c->d_site_out, c->d_site_totals };
	for (void *p : ptrs) if (p) (void) hipFree(p);
	c->d_site_off = c->d_site_ix = c->d_site_out = nullptr;
	c->d_site_totals = nullptr;
	c->n_sites = 0;
	c->sites_attached = false;
}

} // namespace

namespace ntsm_rt {
void sites_destroy(ntsm_ctx *c)
{
	sites_release(c);
	for (hipEvent_t &e : c->site_ev) if (e) { (void) hipEventDestroy(e); e = nullptr; }
}
} // namespace ntsm_rt

using namespace ntsm_rt;

extern "C" {

/* what ntsm_sites_attach asks of its lists, before any HIP call */
int ntsm_debug_sites_check(uint32_t n_kmers, const uint32_t *offsets, const uint32_t *kmer_ix, uint32_t n_sites)
{
	if (!offsets || n_sites > 0x7FFFFFFFu) return NTSM_ERR_ARG;
	const uint64_t n_off = 2ull * n_sites + 1;
	for (uint64_t i = 1; i < n_off; ++i) if (offsets[i] < offsets[i - 1]) return NTSM_ERR_ARG;
	const uint32_t lo = offsets[0], hi = offsets[n_off - 1];
	if (hi > lo && !kmer_ix) return NTSM_ERR_ARG;
	for (uint32_t j = lo; j < hi; ++j) if (kmer_ix[j] >= n_kmers) return NTSM_ERR_ARG;
	return NTSM_OK;
}

int ntsm_sites_attach(ntsm_ctx *c, const uint32_t *offsets, const uint32_t *kmer_ix, uint32_t n_sites)
{
	if (!c) return NTSM_ERR_ARG;
	const int bad = ntsm_debug_sites_check(c->n_kmers, offsets, kmer_ix, n_sites);
	if (bad) return bad;
	const uint64_t n_off = 2ull * n_sites + 1;
	const uint32_t hi = offsets[n_off - 1];
	if (c->failed) return NTSM_ERR_STATE;
	HIPCHK(hipSetDevice(c->device));
	HIPCHK(hipStreamSynchronize(c->rstream));                /* a reduce of the lists this call replaces has finished */
	sites_release(c);
	auto fail = [&]() { sites_release(c); return NTSM_ERR_HIP; };
	/* every buffer has at least one element, so that n_sites = 0 or a set of empty lists is no special case below */
	if (dev_malloc(&c->d_site_off, n_off * sizeof(uint32_t)) != hipSuccess) return fail();
	if (dev_malloc(&c->d_site_ix, std::max<uint64_t>(1, hi) * sizeof(uint32_t)) != hipSuccess) return fail();
	if (dev_malloc(&c->d_site_out, std::max<uint64_t>(1, 4ull * n_sites) * sizeof(uint32_t)) != hipSuccess) return fail();
	if (dev_malloc(&c->d_site_totals, 3 * sizeof(unsigned long long)) != hipSuccess) return fail();
	if (h2d(c->d_site_off, offsets, n_off * sizeof(uint32_t)) != hipSuccess) return fail();
	if (hi && h2d(c->d_site_ix, kmer_ix, (uint64_t) hi * sizeof(uint32_t)) != hipSuccess) return fail();
	c->n_sites = n_sites;
	c->sites_attached = true;
	return NTSM_OK;
}

int ntsm_sites_reduce(ntsm_ctx *c, uint32_t *counts, uint32_t *sums, ntsm_site_totals *out)
{
	if (!c || !counts || !c->sites_attached) return NTSM_ERR_ARG;
	int rc = ntsm_counts_device(c, nullptr, nullptr);         /* sync + gather into d_vec (an imported reduced vector stays as it is) */
	if (rc) return rc;
	ntsm_site_totals tot = { 0, 0, 0 };
	c->site_kernel_ms = 0;
	if (c->n_sites) {
		const uint32_t n_lists = 2 * c->n_sites;
		uint32_t *d_counts = c->d_site_out, *d_sums = sums ? c->d_site_out + n_lists : nullptr;
		hipStream_t st = c->rstream;                            /* the gather ran here: a null-stream launch would not be ordered against it (ntsm_reset) */
		HIPCHK(hipMemsetAsync(c->d_site_totals, 0, 3 * sizeof(unsigned long long), st));
		if (c->timing) {
			for (hipEvent_t &e : c->site_ev) if (!e) HIPCHK(hipEventCreate(&e));
			HIPCHK(hipEventRecord(c->site_ev[0], st));
		}
		hipLaunchKernelGGL(ntsm_sites_kernel, dim3((n_lists + kSiteThreads - 1) / kSiteThreads), dim3(kSiteThreads), 0, st,
				c->d_vec, c->d_site_off, c->d_site_ix, n_lists, d_counts, d_sums, c->d_site_totals);
		HIPCHK(hipGetLastError());
		if (c->timing) HIPCHK(hipEventRecord(c->site_ev[1], st));
		HIPCHK(hipMemcpyAsync(counts, d_counts, (uint64_t) n_lists * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
		if (sums) HIPCHK(hipMemcpyAsync(sums, d_sums, (uint64_t) n_lists * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
		unsigned long long h_tot[3] = { 0, 0, 0 };
		HIPCHK(hipMemcpyAsync(h_tot, c->d_site_totals, sizeof h_tot, hipMemcpyDeviceToHost, st));
		HIPCHK(hipStreamSynchronize(st));
		if (c->timing) {
			float ms = 0;
			HIPCHK(hipEventElapsedTime(&ms, c->site_ev[0], c->site_ev[1]));
			c->site_kernel_ms = ms;
		}
		tot.total = h_tot[0];
		tot.sum_of_sums = h_tot[1];
		tot.sites_covered = h_tot[2];
	}
	if (out) *out = tot;
	return NTSM_OK;
}

int ntsm_sites_kernel_ms(ntsm_ctx *c, double *ms)
{
	if (!c || !ms) return NTSM_ERR_ARG;
	*ms = c->site_kernel_ms;
	return NTSM_OK;
}

} // extern "C"
