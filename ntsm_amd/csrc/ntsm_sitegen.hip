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
 * only thing that ends a run of valid bases and the kernel needs no record table.
 */
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/ntsm_sitegen_hip.h"
#define NTSM_HIP_TAG "ntsm_sitegen"
#include "ntsm_hip_scope.h"

#define NTSM_API extern "C" __attribute__((visibility("default")))

namespace {

constexpr uint32_t kStretch = 128;          /* window ends per lane; a multiple of 16 */
constexpr uint32_t kPreheat = 32;           /* bytes a lane reads before its stretch: >= k - 1, a multiple of 16 */
constexpr uint32_t kBlock = 256;
constexpr uint64_t kStageCap = 128ull << 20; /* staging buffer: bytes per launch, a multiple of kStretch: 2^20 lanes, two rounds of the machine's wave slots */
constexpr uint64_t kEven = 0x5555555555555555ull;

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

constexpr uint32_t kBitsLg = 3;             /* bitmap bits per bucket, log2 */

/* the bitmap's bit of a pair value: the top lg + kBitsLg bits of its hash; the bucket is that >> kBitsLg */
__host__ __device__ inline uint32_t bit_of(uint64_t v, uint32_t lg)
{
	v ^= v >> 33;
	v *= 0xff51afd7ed558ccdull;
	v ^= v >> 33;
	v *= 0xc4ceb9fe1a85ec53ull;
	return (uint32_t)(v >> (64 - lg - kBitsLg));
}

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
			uint32_t *word = t.hits + t.idx[i * t.n_ent + e];
			/* the word only grows: a stale read costs an atomic, never a wrong count */
			if (__atomic_load_n(word, __ATOMIC_RELAXED) < 255u)
				atomicAdd(word, 1u);
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

struct ntsm_sitegen {
	int device = 0;
	uint32_t k = 0, x = 0;
	uint64_t n_cands = 0;
	DevTables t{};
	void *d_bitmap = nullptr, *d_off = nullptr, *d_kmer = nullptr, *d_idx = nullptr, *d_hits = nullptr, *d_counters = nullptr;
	uint8_t *d_genome = nullptr;
	uint8_t *stage = nullptr;                /* pinned, kStageCap + 16 bytes */
	uint64_t fill = 0;                       /* staged bytes: the carried tail, then what came since the last launch */
	bool fresh = false;                      /* bytes staged since the last launch */
	hipStream_t stream = nullptr;
	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	ntsm_sitegen_times times{};
};

namespace {

int launch(ntsm_sitegen *s)
{
	if (s->fresh && s->fill >= s->k) {
		const uint64_t n = (s->fill + 15) & ~15ull;
		memset(s->stage + s->fill, 'N', n - s->fill);
		double t0 = now_ms();
		HIPCHK(hipMemcpyAsync(s->d_genome, s->stage, n, hipMemcpyHostToDevice, s->stream));
		HIPCHK(hipStreamSynchronize(s->stream));
		s->times.upload_ms += now_ms() - t0;
		const uint64_t lanes = (n + kStretch - 1) / kStretch;
		const uint32_t blocks = (uint32_t)((lanes + kBlock - 1) / kBlock);
		HIPCHK(hipEventRecord(s->ev0, s->stream));
		hipLaunchKernelGGL(scan_kernel, dim3(blocks), dim3(kBlock), 0, s->stream, s->d_genome, n, s->t);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(s->ev1, s->stream));
		HIPCHK(hipEventSynchronize(s->ev1));
		float ms = 0;
		HIPCHK(hipEventElapsedTime(&ms, s->ev0, s->ev1));
		s->times.kernel_ms += ms;
		if (n == kStageCap) {                            /* full launches only: their spread is the measurement's noise */
			if (!s->times.full_launches || ms < s->times.full_kernel_ms_min) s->times.full_kernel_ms_min = ms;
			if (ms > s->times.full_kernel_ms_max) s->times.full_kernel_ms_max = ms;
			s->times.full_launches++;
		}
		s->times.launches++;
	}
	/* the last k - 1 bytes open the next launch: no window lies wholly inside them, so none is counted twice */
	const uint64_t carry = s->fill < s->k - 1 ? s->fill : s->k - 1;
	memmove(s->stage, s->stage + s->fill - carry, carry);
	s->fill = carry;
	s->fresh = false;
	return 0;
}

int put(ntsm_sitegen *s, const char *p, uint64_t len)
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

int build_tables(ntsm_sitegen *s, const uint64_t *cands)
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
	t.x = s->x;
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
		for (uint64_t e = 0; e < n_ent; e++) {
			const uint32_t bit = bit_of(ent[e] & t.pair_mask[i], lg);
			bucket[e] = bit >> kBitsLg;
			o[bucket[e] + 1]++;
			bitmap[i * (nb >> (5 - kBitsLg)) + (bit >> 5)] |= 1u << (bit & 31);
		}
		for (uint64_t h = 0; h < nb; h++)
			o[h + 1] += o[h];
		std::vector<uint32_t> cur(o, o + nb);
		for (uint64_t e = 0; e < n_ent; e++) {          /* stable: a bucket keeps entry order */
			const uint32_t at = cur[bucket[e]]++;
			kmer[i * n_ent + at] = ent[e];
			idx[i * n_ent + at] = (uint32_t)(e >> 1);
		}
	}
	s->times.table_build_ms = now_ms() - t0;

	t0 = now_ms();
	const size_t hits_bytes = (s->n_cands ? s->n_cands : 1) * sizeof(uint32_t);
	HIPCHK(hipMalloc(&s->d_bitmap, bitmap.size() * 4));
	HIPCHK(hipMalloc(&s->d_off, off.size() * 4));
	HIPCHK(hipMalloc(&s->d_kmer, kmer.size() * 8));
	HIPCHK(hipMalloc(&s->d_idx, idx.size() * 4));
	HIPCHK(hipMalloc(&s->d_hits, hits_bytes));
	HIPCHK(hipMalloc(&s->d_counters, 2 * sizeof(unsigned long long)));
	HIPCHK(hipMemcpy(s->d_bitmap, bitmap.data(), bitmap.size() * 4, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(s->d_off, off.data(), off.size() * 4, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(s->d_kmer, kmer.data(), kmer.size() * 8, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy(s->d_idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice));
	HIPCHK(hipMemset(s->d_hits, 0, hits_bytes));
	HIPCHK(hipMemset(s->d_counters, 0, 2 * sizeof(unsigned long long)));
	HIPCHK(hipDeviceSynchronize());
	s->times.table_upload_ms = now_ms() - t0;
	s->times.table_bytes = bitmap.size() * 4 + off.size() * 4 + kmer.size() * 8 + idx.size() * 4;
	t.bitmap = (const uint32_t *)s->d_bitmap;
	t.off = (const uint32_t *)s->d_off;
	t.kmer = (const uint64_t *)s->d_kmer;
	t.idx = (const uint32_t *)s->d_idx;
	t.hits = (uint32_t *)s->d_hits;
	t.counters = (unsigned long long *)s->d_counters;
	return 0;
}

/* the stream, its two events and both ends of the staging buffer */
int open_stage(ntsm_sitegen *s)
{
	HIPCHK(hipStreamCreate(&s->stream));
	HIPCHK(hipEventCreate(&s->ev0));
	HIPCHK(hipEventCreate(&s->ev1));
	HIPCHK(hipHostMalloc((void **)&s->stage, kStageCap + 16, hipHostMallocDefault));
	HIPCHK(hipMalloc((void **)&s->d_genome, kStageCap + 16));
	return 0;
}

} // namespace

NTSM_API void ntsm_sitegen_close(ntsm_sitegen *s)
{
	if (!s)
		return;
	(void)hipSetDevice(s->device);
	(void)hipFree(s->d_bitmap); (void)hipFree(s->d_off); (void)hipFree(s->d_kmer); (void)hipFree(s->d_idx);
	(void)hipFree(s->d_hits); (void)hipFree(s->d_counters); (void)hipFree(s->d_genome);
	if (s->stage) (void)hipHostFree(s->stage);
	if (s->ev0) (void)hipEventDestroy(s->ev0);
	if (s->ev1) (void)hipEventDestroy(s->ev1);
	if (s->stream) (void)hipStreamDestroy(s->stream);
	delete s;
}

NTSM_API int ntsm_sitegen_open(int device, uint32_t k, uint32_t x, uint64_t n_cands, const uint64_t *cands, ntsm_sitegen **out)
{
	if (!out || k < 11 || k > 31 || x > 1 || n_cands >= (1ull << 30) || (n_cands && !cands) || device < 0)
		return -1;
	*out = nullptr;
	static_assert(kPreheat >= 30 && kPreheat % 16 == 0 && kStretch % 16 == 0 && kStageCap % kStretch == 0, "stretch geometry");
	HIPCHK(hipSetDevice(device));
	ntsm_sitegen *s = new (std::nothrow) ntsm_sitegen;
	if (!s)
		return -2;
	s->device = device;
	s->k = k;
	s->x = x;
	s->n_cands = n_cands;
	int rc = build_tables(s, cands);
	if (!rc)
		rc = open_stage(s);
	if (rc) {
		ntsm_sitegen_close(s);
		return rc;
	}
	*out = s;
	return 0;
}

NTSM_API int ntsm_sitegen_submit(ntsm_sitegen *s, const char *bases, uint64_t n, const uint64_t *ends, uint64_t n_ends)
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
	const double busy0 = s->times.upload_ms + s->times.kernel_ms;
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
	s->times.stage_ms += now_ms() - t0 - (s->times.upload_ms + s->times.kernel_ms - busy0);
	s->times.genome_bytes += n;
	return rc;
}

NTSM_API int ntsm_sitegen_hits(ntsm_sitegen *s, uint8_t *hits)
{
	if (!s || (s->n_cands && !hits))
		return -1;
	HIPCHK(hipSetDevice(s->device));
	std::vector<uint32_t> h(s->n_cands ? s->n_cands : 1);
	HIPCHK(hipMemcpy(h.data(), s->d_hits, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
	for (uint64_t i = 0; i < s->n_cands; i++)
		hits[i] = (uint8_t)(h[i] < 255 ? h[i] : 255);
	return 0;
}

NTSM_API int ntsm_sitegen_times_get(ntsm_sitegen *s, ntsm_sitegen_times *out)
{
	if (!s || !out)
		return -1;
	HIPCHK(hipSetDevice(s->device));
	unsigned long long c[2];
	HIPCHK(hipMemcpy(c, s->d_counters, sizeof c, hipMemcpyDeviceToHost));
	s->times.windows = c[0];
	s->times.probes = c[1];
	s->times.bitmap_tests = c[0] * (s->x ? 3 : 1);
	*out = s->times;
	return 0;
}
