/*
 * ntsm_sitegen_gap.hip -- the device step of `ntsmSiteGen -g` (include/ntsm_sitegen_gap_hip.h): per candidate k-mer, in
 * one pass over the genome, the places within one substitution (H, the x = 1 count of ntsm_sitegen.hip) and the places
 * with a one-base gap (G).  DESIGN.md section 13.
 *
 * The tables are those of ntsm_sitegen.hip, built the same way: parts A | B | C (k/3, k/3, the rest), both orientations
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
 * Seams.  The host carries the last k bytes into the next launch (a long window has k bytes before its last), so windows
 * of k and k - 1 bases can lie wholly inside the carry: the kernel is given the carry's length and counts a window only
 * if its last byte lies behind it.
 */
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/ntsm_sitegen_gap_hip.h"
#define NTSM_HIP_TAG "ntsm_sitegen_gap"
#include "ntsm_hip_scope.h"

#define NTSM_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr uint32_t kStretch = 128;          /* window ends per lane; a multiple of 16 */
constexpr uint32_t kPreheat = 32;           /* bytes a lane reads before its stretch: >= k, a multiple of 16 */
constexpr uint32_t kBlock = 256;
constexpr uint64_t kStageCap = 128ull << 20; /* staging buffer: bytes per launch, a multiple of kStretch */
constexpr uint64_t kEven = 0x5555555555555555ull;
constexpr uint32_t kBitsLg = 3;             /* bitmap bits per bucket, log2 */
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

/* the bitmap's bit of a pair value, as ntsm_sitegen.hip has it: the top lg + kBitsLg bits of its hash */
__host__ __device__ inline uint32_t bit_of(uint64_t v, uint32_t lg)
{
	v ^= v >> 33;
	v *= 0xff51afd7ed558ccdull;
	v ^= v >> 33;
	v *= 0xc4ceb9fe1a85ec53ull;
	return (uint32_t)(v >> (64 - lg - kBitsLg));
}

__device__ inline void count(uint32_t *word)
{
	/* the word only grows: a stale read costs an atomic, never a wrong count */
	if (__atomic_load_n(word, __ATOMIC_RELAXED) < 255u)
		atomicAdd(word, 1u);
}

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

uint64_t revcomp(uint64_t q, uint32_t k)
{
	uint64_t r = 0;
	for (uint32_t i = 0; i < k; i++) {
		r = (r << 2) | (3 - (q & 3));
		q >>= 2;
	}
	return r;
}

double now_ms()
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

} // namespace

struct ntsm_sitegap {
	int device = 0;
	uint32_t k = 0;
	uint64_t n_cands = 0;
	DevTables t{};
	ntsm_hip::Buffers dev;                   /* tables, counts, counters and the device end of the staging buffer */
	ntsm_hip::Events<2> ev;
	uint8_t *d_genome = nullptr;
	uint8_t *stage = nullptr;                /* pinned, kStageCap + 16 bytes */
	uint64_t fill = 0;                       /* staged bytes: the carried tail, then what came since the last launch */
	uint32_t carried = 0;                    /* of them, the bytes an earlier launch has seen: no window that ends there is new */
	bool fresh = false;                      /* bytes staged since the last launch */
	hipStream_t stream = nullptr;
	struct ntsm_sitegap_stats st{};
	~ntsm_sitegap()
	{
		if (stage) (void)hipHostFree(stage);
		if (stream) (void)hipStreamDestroy(stream);
	}
};

namespace {

int launch(ntsm_sitegap *s)
{
	if (s->fresh && s->fill + 1 >= s->k) {                        /* k - 1 bytes can hold a short window */
		const uint64_t n = (s->fill + 15) & ~15ull;
		memset(s->stage + s->fill, 'N', n - s->fill);
		double t0 = now_ms();
		HIPCHK(hipMemcpyAsync(s->d_genome, s->stage, n, hipMemcpyHostToDevice, s->stream));
		HIPCHK(hipStreamSynchronize(s->stream));
		s->st.upload_ms += now_ms() - t0;
		const uint64_t lanes = (n + kStretch - 1) / kStretch;
		const uint32_t blocks = (uint32_t)((lanes + kBlock - 1) / kBlock);
		HIPCHK(hipEventRecord(s->ev[0], s->stream));
		hipLaunchKernelGGL(gap_scan_kernel, dim3(blocks), dim3(kBlock), 0, s->stream, s->d_genome, n, s->carried, s->t);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(s->ev[1], s->stream));
		HIPCHK(hipEventSynchronize(s->ev[1]));
		float ms = 0;
		HIPCHK(hipEventElapsedTime(&ms, s->ev[0], s->ev[1]));
		s->st.kernel_ms += ms;
		if (n == kStageCap) {                            /* full launches only: their spread is the measurement's noise */
			if (!s->st.full_launches || ms < s->st.full_kernel_ms_min) s->st.full_kernel_ms_min = ms;
			if (ms > s->st.full_kernel_ms_max) s->st.full_kernel_ms_max = ms;
			s->st.full_launches++;
		}
		s->st.launches++;
	}
	/* the last k bytes open the next launch.  Where there was no launch, everything staged is shorter than any window, and
	   calling it "seen" loses none */
	const uint64_t carry = s->fill < s->k ? s->fill : s->k;
	memmove(s->stage, s->stage + s->fill - carry, carry);
	s->fill = carry;
	s->carried = (uint32_t)carry;
	s->fresh = false;
	return 0;
}

int put(ntsm_sitegap *s, const char *p, uint64_t len)
{
	while (len) {
		const uint64_t room = kStageCap - s->fill;
		const uint64_t take = len < room ? len : room;
		memcpy(s->stage + s->fill, p, take);
		s->fill += take;
		s->fresh = true;
		p += take;
		len -= take;
		if (s->fill == kStageCap) {
			int rc = launch(s);
			if (rc)
				return rc;
		}
	}
	return 0;
}

int build_tables(ntsm_sitegap *s, const uint64_t *cands, uint32_t e)
{
	const uint32_t k = s->k;
	const uint64_t n_ent = 2 * s->n_cands;
	DevTables &t = s->t;
	const uint32_t a = k / 3, b = k / 3, c = k - a - b;
	const uint64_t mc = (1ull << (2 * c)) - 1, mb = ((1ull << (2 * b)) - 1) << (2 * c), ma = ((1ull << (2 * a)) - 1) << (2 * (b + c));
	t.pair_mask[0] = ma | mb; t.rest_mask[0] = mc & kEven;
	t.pair_mask[1] = ma | mc; t.rest_mask[1] = mb & kEven;
	t.pair_mask[2] = mb | mc; t.rest_mask[2] = ma & kEven;
	t.kmask = ma | mb | mc;
	t.k = k;
	t.e = e;
	t.a = a;
	t.n_ent = n_ent;
	uint32_t lg = 10;
	while (lg < 28 && (1ull << lg) < n_ent)
		lg++;
	t.lg = lg;
	const uint64_t nb = 1ull << lg;

	double t0 = now_ms();
	std::vector<uint64_t> ent(n_ent ? n_ent : 1);
	for (uint64_t i = 0; i < s->n_cands; i++) {
		if (cands[i] & ~t.kmask)
			return -1;
		ent[2 * i] = cands[i];
		ent[2 * i + 1] = revcomp(cands[i], k);
	}
	std::vector<uint32_t> bitmap(3 * (nb >> (5 - kBitsLg)), 0), off(3 * (nb + 1), 0), idx(3 * (n_ent ? n_ent : 1)), bucket(n_ent ? n_ent : 1);
	std::vector<uint64_t> kmer(3 * (n_ent ? n_ent : 1));
	for (uint32_t i = 0; i < 3; i++) {
		uint32_t *o = off.data() + i * (nb + 1);
		for (uint64_t j = 0; j < n_ent; j++) {
			const uint32_t bit = bit_of(ent[j] & t.pair_mask[i], lg);
			bucket[j] = bit >> kBitsLg;
			o[bucket[j] + 1]++;
			bitmap[i * (nb >> (5 - kBitsLg)) + (bit >> 5)] |= 1u << (bit & 31);
		}
		for (uint64_t h = 0; h < nb; h++)
			o[h + 1] += o[h];
		std::vector<uint32_t> cur(o, o + nb);
		for (uint64_t j = 0; j < n_ent; j++) {          /* stable: a bucket keeps entry order */
			const uint32_t at = cur[bucket[j]]++;
			kmer[i * n_ent + at] = ent[j];
			idx[i * n_ent + at] = (uint32_t)(j >> 1);
		}
	}
	s->st.table_build_ms = now_ms() - t0;

	t0 = now_ms();
	uint32_t *d_bitmap, *d_off, *d_idx, *d_sub, *d_gap;
	uint64_t *d_kmer;
	unsigned long long *d_counters;
	HIPCHK(s->dev.alloc(&d_bitmap, bitmap.size()));
	HIPCHK(s->dev.alloc(&d_off, off.size()));
	HIPCHK(s->dev.alloc(&d_kmer, kmer.size()));
	HIPCHK(s->dev.alloc(&d_idx, idx.size()));
	HIPCHK(s->dev.alloc(&d_sub, s->n_cands));
	HIPCHK(s->dev.alloc(&d_gap, s->n_cands));
	HIPCHK(s->dev.alloc(&d_counters, kCounters));
	HIPCHK(hipMemcpy(d_bitmap, bitmap.data(), bitmap.size() * 4, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(d_kmer, kmer.data(), kmer.size() * 8, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(d_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
	HIPCHK(hipMemset(d_sub, 0, (s->n_cands ? s->n_cands : 1) * sizeof(uint32_t)));
	HIPCHK(hipMemset(d_gap, 0, (s->n_cands ? s->n_cands : 1) * sizeof(uint32_t)));
	HIPCHK(hipMemset(d_counters, 0, kCounters * sizeof(unsigned long long)));
	HIPCHK(hipDeviceSynchronize());
	s->st.table_upload_ms = now_ms() - t0;
	s->st.table_bytes = bitmap.size() * 4 + off.size() * 4 + kmer.size() * 8 + idx.size() * 4;
	t.bitmap = d_bitmap;
	t.off = d_off;
	t.kmer = d_kmer;
	t.idx = d_idx;
	t.sub = d_sub;
	t.gap = d_gap;
	t.counters = d_counters;
	return 0;
}

/* the stream, its two events and both ends of the staging buffer */
int open_stage(ntsm_sitegap *s)
{
	HIPCHK(hipStreamCreate(&s->stream));
	HIPCHK(s->ev.create());
	HIPCHK(hipHostMalloc((void **)&s->stage, kStageCap + 16, hipHostMallocDefault));
	HIPCHK(s->dev.alloc(&s->d_genome, kStageCap + 16));
	return 0;
}

} // namespace

NTSM_API void ntsm_sitegap_close(ntsm_sitegap *s)
{
	if (!s)
		return;
	(void)hipSetDevice(s->device);
	delete s;
}

NTSM_API int ntsm_sitegap_open(int device, uint32_t k, uint32_t e, uint64_t n_cands, const uint64_t *cands, ntsm_sitegap **out)
{
	if (!out || k < 11 || k > 31 || e < 1 || 2 * (uint64_t)e > k - 1 || n_cands >= (1ull << 30) || (n_cands && !cands) || device < 0)
		return -1;
	*out = nullptr;
	static_assert(kPreheat >= 31 && kPreheat % 16 == 0 && kStretch % 16 == 0 && kStageCap % kStretch == 0, "stretch geometry");
	HIPCHK(hipSetDevice(device));
	ntsm_sitegap *s = new (std::nothrow) ntsm_sitegap;
	if (!s)
		return -2;
	s->device = device;
	s->k = k;
	s->n_cands = n_cands;
	int rc = build_tables(s, cands, e);
	if (!rc)
		rc = open_stage(s);
	if (rc) {
		ntsm_sitegap_close(s);
		return rc;
	}
	*out = s;
	return 0;
}

NTSM_API int ntsm_sitegap_submit(ntsm_sitegap *s, const char *bases, uint64_t n, const uint64_t *ends, uint64_t n_ends)
{
	if (!s || (n && !bases) || (n_ends && !ends))
		return -1;
	uint64_t prev = 0;
	for (uint64_t i = 0; i < n_ends; i++) {
		if (ends[i] < prev || ends[i] > n || (i && ends[i] == prev))
			return -1;
		prev = ends[i];
	}
	HIPCHK(hipSetDevice(s->device));
	double t0 = now_ms();
	const double busy0 = s->st.upload_ms + s->st.kernel_ms;
	uint64_t at = 0;
	int rc = 0;
	for (uint64_t i = 0; i < n_ends && !rc; i++) {
		rc = put(s, bases + at, ends[i] - at);
		if (!rc)
			rc = put(s, "N", 1);                         /* the separator: no window crosses a record end */
		at = ends[i];
	}
	if (!rc)
		rc = put(s, bases + at, n - at);
	if (!rc)
		rc = launch(s);
	s->st.stage_ms += now_ms() - t0 - (s->st.upload_ms + s->st.kernel_ms - busy0);
	s->st.genome_bytes += n;
	return rc;
}

NTSM_API int ntsm_sitegap_hits(ntsm_sitegap *s, uint8_t *sub, uint8_t *gap)
{
	if (!s || (s->n_cands && (!sub || !gap)))
		return -1;
	HIPCHK(hipSetDevice(s->device));
	std::vector<uint32_t> h(s->n_cands ? s->n_cands : 1);
	uint8_t *const out[2] = {sub, gap};
	const uint32_t *const from[2] = {s->t.sub, s->t.gap};
	for (int j = 0; j < 2; j++) {
		HIPCHK(hipMemcpy(h.data(), from[j], h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
		for (uint64_t i = 0; i < s->n_cands; i++)
			out[j][i] = (uint8_t)(h[i] < 255 ? h[i] : 255);
	}
	return 0;
}

NTSM_API int ntsm_sitegap_stats(ntsm_sitegap *s, struct ntsm_sitegap_stats *out)
{
	if (!s || !out)
		return -1;
	HIPCHK(hipSetDevice(s->device));
	unsigned long long c[kCounters];
	HIPCHK(hipMemcpy(c, s->t.counters, sizeof c, hipMemcpyDeviceToHost));
	s->st.windows = c[0];
	s->st.windows_long = c[1];
	s->st.windows_short = c[2];
	s->st.probes = c[3];
	/* not counted by the kernel: a byte that ends a short window tests BC once and AB, AC for that window; each longer
	   window adds its AB and AC */
	s->st.bitmap_tests = 3 * c[2] + 2 * c[0] + 2 * c[1];
	*out = s->st;
	return 0;
}
