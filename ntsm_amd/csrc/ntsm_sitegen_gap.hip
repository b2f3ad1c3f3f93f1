/*
 * ntsm_sitegen_gap.hip -- the device step of `ntsmSiteGen -g` (include/ntsm_sitegen_gap_hip.h): per candidate k-mer, in
 * one pass over the genome, the places within one substitution (H, the x = 1 count of ntsm_sitegen.hip) and the places
 * with a one-base gap (G).  DESIGN.md section 13.
 *
 * The tables are those of ntsm_sitegen.hip, built by the same code (ntsm_sitegen_tables.h): parts A | B | C (k/3, k/3, the rest), both orientations
 * of every candidate as entries, three tables bucketed by a hash of the pair AB, AC or BC, a bitmap of eight bits per
 * bucket in front of each.  What is new is what a lane asks of them.  It rolls k + 1 bases (64 bits at k = 31), and a
 * byte can end three windows: of k bases (H), of k + 1 (the genome holds one base more than q) and of k - 1 (one less).
 * A one-base gap at position p leaves the parts before p where they are and shifts the parts after it by one base, so a
 * gapped place still agrees with its entry on a pair, if the parts in front of the gap are taken from the window's start
 * and the parts behind it from the window's end:
 *     AB from the start,   AC = A from the start + C from the end,   BC from the end.
 * BC from the end is the same key for all three lengths, so one bitmap test and one bucket walk serve them: 7 bitmap
 * tests per byte, where ntsm_sitegen.hip has 3.
 *
 * An entry whose pair agrees is verified without the parts.  L = the common prefix of entry and window (both aligned at
 * their first base), R = their common suffix (aligned at their last).  The p that qualify are
 *     long window:  max(e, k - R) .. min(L, k - e)         short window:  max(e, k - 1 - R) .. min(L, k - 1 - e)
 * and the window is a place when that interval is not empty.  It is counted once, by the table that owns the smallest
 * qualifying p (long / short): BC for p <= a / p < a, AC for p <= a + b / p < a + b, AB beyond; that table's pair does
 * agree for that p, so its walk meets the entry.
 *
 * Seams.  The host carries the last k bytes into the next launch (ntsm_sitegen_stage.h, its second setting), so the
 * kernel is given the carry's length and counts a window only if its last byte lies behind it.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <new>

#include "../../include/ntsm_sitegen_gap_hip.h"
#define NTSM_HIP_TAG "ntsm_sitegen_gap"
#include "ntsm_sitegen_tables.h"

#define NTSM_API extern "C" __attribute__((visibility("default")))

namespace {

using namespace ntsm_site;

constexpr uint32_t kCounters = 4;           /* windows of k, k + 1, k - 1 bases; probes */

enum : uint32_t { kSub = 1, kLong = 2, kShort = 4 };   /* what a walk checks its entries for */

struct DevTables {
	const uint32_t *bitmap;                  /* [3][8 nb / 32] */
	const uint32_t *off;                     /* [3][nb + 1] */
	const uint64_t *kmer;                    /* [3][n_ent] */
	const uint32_t *idx;                     /* [3][n_ent] */
	uint32_t *sub, *gap;                     /* [n_cands] each */
	unsigned long long *counters;            /* [kCounters] */
	uint64_t pair_mask[3];                   /* AB, AC, BC */
	uint64_t rest_mask[3];                   /* one bit per base (the even bit) of the part outside the pair */
	uint64_t kmask;                          /* k bases */
	uint64_t n_ent;
	uint32_t lg;                             /* nb = 1 << lg */
	uint32_t k, e, a;                        /* a = b = k / 3 */
};

/* bases on which two k-mers agree from the left / from the right, d = their difference; k when d = 0 */
__device__ inline int prefix_len(uint64_t d, int k) { return d ? (__clzll((long long)d) - (64 - 2 * k)) >> 1 : k; }
__device__ inline int suffix_len(uint64_t d, int k) { return d ? (__ffsll((unsigned long long)d) - 1) >> 1 : k; }

/*
 * One table, one key: test the bitmap, walk the bucket.  key carries the table's pair at the pair's own positions.  w is
 * the lane's k + 1 rolled bases; WHAT says which of the windows that end here take this key in this table.
 */
template <uint32_t TAB, uint32_t WHAT> __device__ inline void walk(const DevTables &t, uint64_t key, uint64_t w, uint32_t what, uint32_t &probes)
{
	const uint64_t nb = 1ull << t.lg;
	const uint32_t bit = bit_of(key & t.pair_mask[TAB], t.lg);
	if (!((t.bitmap[TAB * (nb >> (5 - kBitsLg)) + (bit >> 5)] >> (bit & 31)) & 1u))
		return;
	const int k = (int)t.k, e = (int)t.e, a = (int)t.a;
	const uint32_t h = bit >> kBitsLg;
	const uint32_t *off = t.off + TAB * (nb + 1);
	const uint32_t lo = off[h], hi = off[h + 1];
	for (uint32_t at = lo; at < hi; at++) {
		const uint64_t q = t.kmer[TAB * t.n_ent + at];
		probes++;
		if ((q ^ key) & t.pair_mask[TAB])
			continue;
		uint32_t n_sub = 0, n_gap = 0;
		if ((WHAT & kSub) && (what & kSub)) {                /* ntsm_sitegen.hip's rule: AB owns <= 1 in C, AC and BC exactly 1 */
			const uint64_t d = q ^ (w & t.kmask);
			const int cnt = __popcll((d | (d >> 1)) & t.rest_mask[TAB]);
			n_sub = TAB == 0 ? cnt <= 1 : cnt == 1;
		}
		if ((WHAT & kLong) && (what & kLong)) {              /* first k bases against q from the left, last k from the right */
			const int L = prefix_len(q ^ (w >> 2), k), R = suffix_len(q ^ (w & t.kmask), k);
			const int p = max(e, k - R);
			n_gap += p <= min(L, k - e) && (p <= a ? 2 : p <= 2 * a ? 1 : 0) == (int)TAB;
		}
		if ((WHAT & kShort) && (what & kShort)) {            /* k - 1 bases: a zero stands where the window has no base */
			const uint64_t s = w & (t.kmask >> 2);
			const int L = prefix_len(q ^ (s << 2), k), R = suffix_len(q ^ s, k);
			const int p = max(e, k - 1 - R);
			n_gap += p <= min(L, k - 1 - e) && (p < a ? 2 : p < 2 * a ? 1 : 0) == (int)TAB;
		}
		const uint32_t c = t.idx[TAB * t.n_ent + at];
		if (n_sub)
			count(t.sub + c);
		for (; n_gap; n_gap--)                               /* a long and a short window can both be places of one entry */
			count(t.gap + c);
	}
}

__device__ inline uint32_t wave_sum(uint32_t v)
{
	for (int d = 32; d; d >>= 1)
		v += __shfl_down(v, d, 64);
	return v;
}

/*
 * g: n bytes, n a multiple of 16, 16-byte aligned.  Lane l owns the windows that END at bytes [l * kStretch, (l + 1) * kStretch),
 * except those that end inside the first `carry` bytes: an earlier launch had them.
 */
__global__ __launch_bounds__(kBlock) void gap_scan_kernel(const uint8_t *__restrict__ g, uint64_t n, uint32_t carry, DevTables t)
{
	const uint64_t start = ((uint64_t)blockIdx.x * kBlock + threadIdx.x) * kStretch;
	const uint64_t stop = start + kStretch < n ? start + kStretch : (start < n ? n : start);
	const uint64_t first = start > carry ? start : carry;        /* the first byte that may end a window of this lane's */
	const uint64_t lmask = (t.kmask << 2) | 3;                      /* k + 1 bases */
	const uint64_t ma = t.pair_mask[0] & t.pair_mask[1], mc = t.pair_mask[1] & t.pair_mask[2];
	const uint32_t k = t.k;
	uint64_t w = 0;
	uint32_t run = 0, n_k = 0, n_long = 0, n_short = 0, probes = 0;
	if (start < stop)
		for (uint64_t pos = start >= kPreheat ? start - kPreheat : 0; pos < stop; pos += 16) {
			uint4 v = *reinterpret_cast<const uint4 *>(g + pos);
#pragma unroll 1
			for (uint32_t j = 0; j < 16; j++) {
				const uint32_t c = v.x & 0xdfu;                       /* upper case */
				v.x = (v.x >> 8) | (v.y << 24);
				v.y = (v.y >> 8) | (v.z << 24);
				v.z = (v.z >> 8) | (v.w << 24);
				v.w >>= 8;
				const bool valid = c == 'A' || c == 'C' || c == 'G' || c == 'T';
				w = ((w << 2) | (((c >> 1) ^ (c >> 2)) & 3u)) & lmask;   /* A 0, C 1, G 2, T 3 */
				run = valid ? run + 1 : 0;
				if (pos + j < first || run + 1 < k)
					continue;
				const uint32_t what = kShort | (run >= k ? kSub : 0) | (run > k ? kLong : 0);
				n_short++;
				walk<2, kSub | kLong | kShort>(t, w, w, what, probes);
				const uint64_t from_short = w << 2;                  /* the window's first base where a k-mer's is */
				walk<0, kShort>(t, from_short, w, what, probes);
				walk<1, kShort>(t, (from_short & ma) | (w & mc), w, what, probes);
				if (what & kSub) {
					n_k++;
					walk<0, kSub>(t, w, w, what, probes);
					walk<1, kSub>(t, w, w, what, probes);
				}
				if (what & kLong) {
					n_long++;
					const uint64_t from_long = w >> 2;
					walk<0, kLong>(t, from_long, w, what, probes);
					walk<1, kLong>(t, (from_long & ma) | (w & mc), w, what, probes);
				}
			}
		}
	/* one atomic per wave and counter */
	n_k = wave_sum(n_k);
	n_long = wave_sum(n_long);
	n_short = wave_sum(n_short);
	const unsigned long long all_probes = (unsigned long long)wave_sum(probes & 0xffffu) + ((unsigned long long)wave_sum(probes >> 16) << 16);
	if ((threadIdx.x & 63) == 0) {
		if (n_k) atomicAdd(t.counters, (unsigned long long)n_k);
		if (n_long) atomicAdd(t.counters + 1, (unsigned long long)n_long);
		if (n_short) atomicAdd(t.counters + 2, (unsigned long long)n_short);
		if (all_probes) atomicAdd(t.counters + 3, all_probes);
	}
}

} // namespace

struct ntsm_sitegap {
	Scan scan;
	DevTables t{};
};

NTSM_API void ntsm_sitegap_close(ntsm_sitegap *s)
{
	if (!s)
		return;
	(void)hipSetDevice(s->scan.device);
	delete s;
}

NTSM_API int ntsm_sitegap_open(int device, uint32_t k, uint32_t e, uint64_t n_cands, const uint64_t *cands, ntsm_sitegap **out)
{
	if (!out || k < 11 || k > 31 || e < 1 || 2 * (uint64_t)e > k - 1 || n_cands >= (1ull << 30) || (n_cands && !cands) || device < 0)
		return -1;
	*out = nullptr;
	HIPCHK(hipSetDevice(device));
	ntsm_sitegap *s = new (std::nothrow) ntsm_sitegap;
	if (!s)
		return -2;
	const int rc = s->scan.open(device, k, n_cands, cands, k - 1, k, 2, kCounters);
	if (rc) {
		ntsm_sitegap_close(s);
		return rc;
	}
	const Scan &sc = s->scan;
	DevTables &t = s->t;
	t.bitmap = sc.bitmap;
	t.off = sc.off;
	t.kmer = sc.kmer;
	t.idx = sc.idx;
	t.sub = sc.counts[0];
	t.gap = sc.counts[1];
	t.counters = sc.counters;
	memcpy(t.pair_mask, sc.parts.pair_mask, sizeof t.pair_mask);
	memcpy(t.rest_mask, sc.parts.rest_mask, sizeof t.rest_mask);
	t.kmask = sc.parts.kmask;
	t.n_ent = sc.parts.n_ent;
	t.lg = sc.parts.lg;
	t.k = k;
	t.e = e;
	t.a = sc.parts.a;
	*out = s;
	return 0;
}

NTSM_API int ntsm_sitegap_submit(ntsm_sitegap *s, const char *bases, uint64_t n, const uint64_t *ends, uint64_t n_ends)
{
	if (!s)
		return -1;
	return s->scan.submit(bases, n, ends, n_ends, [s](uint32_t blocks, hipStream_t stream, const uint8_t *g, uint64_t len, uint32_t carried) {
		hipLaunchKernelGGL(gap_scan_kernel, dim3(blocks), dim3(kBlock), 0, stream, g, len, carried, s->t);
	});
}

NTSM_API int ntsm_sitegap_hits(ntsm_sitegap *s, uint8_t *sub, uint8_t *gap)
{
	if (!s || (s->scan.n_cands && (!sub || !gap)))
		return -1;
	HIPCHK(hipSetDevice(s->scan.device));
	const int rc = s->scan.hits(0, sub);
	return rc ? rc : s->scan.hits(1, gap);
}

NTSM_API int ntsm_sitegap_stats(ntsm_sitegap *s, struct ntsm_sitegap_stats *out)
{
	if (!s || !out)
		return -1;
	HIPCHK(hipSetDevice(s->scan.device));
	unsigned long long c[kCounters];
	if (const int rc = s->scan.stats(out, c, kCounters))
		return rc;
	out->windows = c[0];
	out->windows_long = c[1];
	out->windows_short = c[2];
	out->probes = c[3];
	/* not counted by the kernel: a byte that ends a short window tests BC once and AB, AC for that window; each longer
	   window adds its AB and AC */
	out->bitmap_tests = 3 * c[2] + 2 * c[0] + 2 * c[1];
	return 0;
}
