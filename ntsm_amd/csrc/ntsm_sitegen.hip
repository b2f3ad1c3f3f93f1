/*
 * ntsm_sitegen.hip -- device step of ntsmSiteGen (include/ntsm_sitegen_hip.h): hit counts of candidate k-mers in a genome
 * with at most one substitution.  DESIGN.md section 13.
 *
 * Method ("two of three").  The k positions are cut into three parts A | B | C (k/3, k/3 and the rest; 6 + 6 + 7 at
 * k = 19).  One substitution leaves two parts intact, so a window within distance 1 of an entry agrees with it exactly on
 * AB, on AC or on BC.  Both orientations of every candidate are entries (ham(rc(g), q) = ham(g, rc(q)), so only forward
 * windows are scanned).  There are three tables, one per pair: the entries bucketed by the top lg bits of a hash of the
 * pair's bits, a bucket being a range of (k-mer, candidate index); in front of each table a bitmap indexed by the top
 * lg + 3 bits of the same hash (eight bits per bucket: with about one entry per bucket, one bit per bucket would be set
 * for every second window; eight make it a filter).  A window tests three bits and, for a set bit, walks the bucket:
 * pair equal, then the differing bases of the remaining part are counted.  A hit is counted exactly once: by table AB
 * when C differs in at most one base, by AC when B differs in exactly one, by BC when A differs in exactly one.  x = 0
 * uses table AB alone with "no base differs".
 *
 * The genome arrives as bytes; the host stages records with one separator byte between them, so "not ACGTacgt" is the
 * only thing that ends a run of valid bases and the kernel needs no record table (ntsm_sitegen_stage.h, its first
 * setting).  The tables are built and uploaded by ntsm_sitegen_tables.h, which ntsm_sitegen_gap.hip shares.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>

#include "../../include/ntsm_sitegen_hip.h"
#define NTSM_HIP_TAG "ntsm_sitegen"
#include "ntsm_sitegen_tables.h"

#define NTSM_API extern "C" __attribute__((visibility("default")))

namespace {

using namespace ntsm_site;

struct DevTables {
	const uint32_t *bitmap;                  /* [3][8 nb / 32] */
	const uint32_t *off;                     /* [3][nb + 1] */
	const uint64_t *kmer;                    /* [3][n_ent] */
	const uint32_t *idx;                     /* [3][n_ent] */
	uint32_t *hits;                          /* [n_cands] */
	unsigned long long *counters;            /* windows, probes */
	uint64_t pair_mask[3];
	uint64_t rest_mask[3];                   /* one bit per base (the even bit) of the part outside the pair */
	uint64_t kmask;
	uint64_t n_ent;
	uint32_t lg;                             /* nb = 1 << lg */
	uint32_t k, x;
};

__device__ inline void probe(const DevTables &t, uint64_t w, uint32_t &probes)
{
	const uint32_t ntab = t.x ? 3 : 1;
	const uint64_t nb = 1ull << t.lg;
	for (uint32_t i = 0; i < ntab; i++) {
		const uint32_t bit = bit_of(w & t.pair_mask[i], t.lg);
		if (!((t.bitmap[i * (nb >> (5 - kBitsLg)) + (bit >> 5)] >> (bit & 31)) & 1u))
			continue;
		const uint32_t h = bit >> kBitsLg;
		const uint32_t *off = t.off + i * (nb + 1);
		const uint32_t lo = off[h], hi = off[h + 1];
		for (uint32_t e = lo; e < hi; e++) {
			const uint64_t d = t.kmer[i * t.n_ent + e] ^ w;
			probes++;
			if (d & t.pair_mask[i])
				continue;
			const int cnt = __popcll((d | (d >> 1)) & t.rest_mask[i]);
			const bool hit = t.x == 0 ? cnt == 0 : (i == 0 ? cnt <= 1 : cnt == 1);
			if (!hit)
				continue;
			count(t.hits + t.idx[i * t.n_ent + e]);
		}
	}
}

/* g: n bytes, n a multiple of 16, 16-byte aligned.  Lane l owns the windows that END at bytes [l * kStretch, (l + 1) * kStretch). */
__global__ __launch_bounds__(kBlock) void scan_kernel(const uint8_t *__restrict__ g, uint64_t n, DevTables t)
{
	const uint64_t start = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * kStretch;
	if (start >= n)
		return;
	const uint64_t stop = start + kStretch < n ? start + kStretch : n;
	uint64_t w = 0;
	uint32_t run = 0, windows = 0, probes = 0;
	for (uint64_t pos = start >= kPreheat ? start - kPreheat : 0; pos < stop; pos += 16) {
		const uint4 v = *reinterpret_cast<const uint4 *>(g + pos);
		const uint32_t word[4] = {v.x, v.y, v.z, v.w};
		const bool own = pos >= start;
#pragma unroll
		for (int j = 0; j < 16; j++) {
			const uint32_t c = (word[j >> 2] >> (8 * (j & 3))) & 0xdfu;   /* upper case */
			const bool valid = c == 'A' || c == 'C' || c == 'G' || c == 'T';
			w = ((w << 2) | (((c >> 1) ^ (c >> 2)) & 3u)) & t.kmask;      /* A 0, C 1, G 2, T 3 */
			run = valid ? run + 1 : 0;
			if (own && run >= t.k) {
				windows++;
				probe(t, w, probes);
			}
		}
	}
	if (windows)
		atomicAdd(t.counters, (unsigned long long)windows);
	if (probes)
		atomicAdd(t.counters + 1, (unsigned long long)probes);
}

} // namespace

struct ntsm_sitegen {
	Scan scan;
	DevTables t{};
};

NTSM_API void ntsm_sitegen_close(ntsm_sitegen *s)
{
	if (!s)
		return;
	(void)hipSetDevice(s->scan.device);
	delete s;
}

NTSM_API int ntsm_sitegen_open(int device, uint32_t k, uint32_t x, uint64_t n_cands, const uint64_t *cands, ntsm_sitegen **out)
{
	if (!out || k < 11 || k > 31 || x > 1 || n_cands >= (1ull << 30) || (n_cands && !cands) || device < 0)
		return -1;
	*out = nullptr;
	HIPCHK(hipSetDevice(device));
	ntsm_sitegen *s = new (std::nothrow) ntsm_sitegen;
	if (!s)
		return -2;
	const int rc = s->scan.open(device, k, n_cands, cands, k, k - 1, 1, 2);
	if (rc) {
		ntsm_sitegen_close(s);
		return rc;
	}
	const Scan &sc = s->scan;
	DevTables &t = s->t;
	t.bitmap = sc.bitmap;
	t.off = sc.off;
	t.kmer = sc.kmer;
	t.idx = sc.idx;
	t.hits = sc.counts[0];
	t.counters = sc.counters;                            /* windows, probes */
	memcpy(t.pair_mask, sc.parts.pair_mask, sizeof t.pair_mask);
	memcpy(t.rest_mask, sc.parts.rest_mask, sizeof t.rest_mask);
	t.kmask = sc.parts.kmask;
	t.n_ent = sc.parts.n_ent;
	t.lg = sc.parts.lg;
	t.k = k;
	t.x = x;
	*out = s;
	return 0;
}

NTSM_API int ntsm_sitegen_submit(ntsm_sitegen *s, const char *bases, uint64_t n, const uint64_t *ends, uint64_t n_ends)
{
	if (!s)
		return -1;
	return s->scan.submit(bases, n, ends, n_ends, [s](uint32_t blocks, hipStream_t stream, const uint8_t *g, uint64_t len, uint32_t) {
		hipLaunchKernelGGL(scan_kernel, dim3(blocks), dim3(kBlock), 0, stream, g, len, s->t);
	});
}

NTSM_API int ntsm_sitegen_hits(ntsm_sitegen *s, uint8_t *hits)
{
	if (!s || (s->scan.n_cands && !hits))
		return -1;
	HIPCHK(hipSetDevice(s->scan.device));
	return s->scan.hits(0, hits);
}

NTSM_API int ntsm_sitegen_times_get(ntsm_sitegen *s, ntsm_sitegen_times *out)
{
	if (!s || !out)
		return -1;
	HIPCHK(hipSetDevice(s->scan.device));
	unsigned long long c[2];
	if (const int rc = s->scan.stats(out, c, 2))
		return rc;
	out->windows = c[0];
	out->probes = c[1];
	out->bitmap_tests = c[0] * (s->t.x ? 3 : 1);
	return 0;
}
