/*
 * ntsm_sitegen_tables.h -- what the two device libraries of ntsmSiteGen (ntsm_sitegen.hip, ntsm_sitegen_gap.hip) share
 * on the HIP side: the launch geometry, the helpers their kernels and the table builder both use, the three tables of
 * ntsm_sitegen.hip's header comment built once on the host and uploaded once, and the scan session around the staging
 * state machine of ntsm_sitegen_stage.h (stream, pinned buffer, events, the timed launch, the counts' read-back).  A
 * library adds its kernel, the by-value argument struct that kernel reads, and its own counters.  Internal: not part of
 * include/.  The including file defines NTSM_HIP_TAG first (ntsm_hip_scope.h).
 */
#ifndef NTSM_SITEGEN_TABLES_H
#define NTSM_SITEGEN_TABLES_H

#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <vector>

#include "ntsm_hip_scope.h"
#include "ntsm_sitegen_stage.h"

namespace ntsm_site {

constexpr uint32_t kStretch = 128;          /* window ends per lane; a multiple of 16 */
constexpr uint32_t kPreheat = 32;           /* bytes a lane reads before its stretch: >= k (a window of k + 1 bases), a multiple of 16 */
constexpr uint32_t kBlock = 256;
constexpr uint64_t kStageCap = 128ull << 20; /* staging buffer: bytes per launch, a multiple of kStretch: 2^20 lanes, two rounds of the machine's wave slots */
constexpr uint64_t kEven = 0x5555555555555555ull;
constexpr uint32_t kBitsLg = 3;             /* bitmap bits per bucket, log2 */
static_assert(kPreheat >= 31 && kPreheat % 16 == 0 && kStretch % 16 == 0 && kStageCap % kStretch == 0, "stretch geometry");

/* the bitmap's bit of a pair value: the top lg + kBitsLg bits of its hash; the bucket is that >> kBitsLg */
__host__ __device__ inline uint32_t bit_of(uint64_t v, uint32_t lg)
{
	v ^= v >> 33;
	v *= 0xff51afd7ed558ccdull;
	v ^= v >> 33;
	v *= 0xc4ceb9fe1a85ec53ull;
	return (uint32_t)(v >> (64 - lg - kBitsLg));
}

/* one more place of a candidate, up to 255 */
__device__ inline void count(uint32_t *word)
{
	/* the word only grows: a stale read costs an atomic, never a wrong count */
	if (__atomic_load_n(word, __ATOMIC_RELAXED) < 255u)
		atomicAdd(word, 1u);
}

inline uint64_t revcomp(uint64_t q, uint32_t k)
{
	uint64_t r = 0;
	for (uint32_t i = 0; i < k; i++) {
		r = (r << 2) | (3 - (q & 3));
		q >>= 2;
	}
	return r;
}

inline double now_ms()
{
	return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

/* the parts A | B | C of a k-mer (k/3, k/3 and the rest) and the size of the tables: what a kernel needs beside the pointers */
struct Parts {
	uint64_t pair_mask[3];                   /* AB, AC, BC */
	uint64_t rest_mask[3];                   /* one bit per base (the even bit) of the part outside the pair */
	uint64_t kmask;                          /* k bases */
	uint64_t n_ent;                          /* both orientations of every candidate */
	uint32_t lg;                             /* nb = 1 << lg buckets per table */
	uint32_t a;                              /* a = b = k / 3 */
};

struct HostTables : Parts {
	std::vector<uint32_t> bitmap;            /* [3][8 nb / 32] */
	std::vector<uint32_t> off;               /* [3][nb + 1] */
	std::vector<uint64_t> kmer;              /* [3][n_ent] */
	std::vector<uint32_t> idx;               /* [3][n_ent] */

	/* -1: a candidate has bits outside its k bases */
	int build(uint32_t k, uint64_t n_cands, const uint64_t *cands)
	{
		a = k / 3;
		const uint32_t b = k / 3, c = k - a - b;
		const uint64_t mc = (1ull << (2 * c)) - 1, mb = ((1ull << (2 * b)) - 1) << (2 * c), ma = ((1ull << (2 * a)) - 1) << (2 * (b + c));
		pair_mask[0] = ma | mb; rest_mask[0] = mc & kEven;
		pair_mask[1] = ma | mc; rest_mask[1] = mb & kEven;
		pair_mask[2] = mb | mc; rest_mask[2] = ma & kEven;
		kmask = ma | mb | mc;
		n_ent = 2 * n_cands;
		lg = 10;
		while (lg < 28 && (1ull << lg) < n_ent)
			lg++;
		const uint64_t nb = 1ull << lg;
		std::vector<uint64_t> ent(n_ent ? n_ent : 1);
		for (uint64_t i = 0; i < n_cands; i++) {
			if (cands[i] & ~kmask)
				return -1;
			ent[2 * i] = cands[i];
			ent[2 * i + 1] = revcomp(cands[i], k);
		}
		std::vector<uint32_t> bucket(n_ent ? n_ent : 1);
		bitmap.assign(3 * (nb >> (5 - kBitsLg)), 0);
		off.assign(3 * (nb + 1), 0);
		idx.resize(3 * (n_ent ? n_ent : 1));
		kmer.resize(3 * (n_ent ? n_ent : 1));
		for (uint32_t i = 0; i < 3; i++) {
			uint32_t *o = off.data() + i * (nb + 1);
			for (uint64_t e = 0; e < n_ent; e++) {
				const uint32_t bit = bit_of(ent[e] & pair_mask[i], lg);
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
		return 0;
	}
};

/* the fields that ntsm_sitegen_times and ntsm_sitegap_stats share, under the names they have there; genome_bytes is the
   stage's `submitted` */
struct ScanTimes {
	double table_build_ms, table_upload_ms, stage_ms, upload_ms, kernel_ms, full_kernel_ms_min, full_kernel_ms_max;
	uint64_t launches, full_launches, table_bytes;
};

/* one session of either library: the tables and count words on the device, and the way genome bytes take to them */
struct Scan {
	int device = 0;
	uint32_t k = 0;
	uint64_t n_cands = 0;
	Parts parts{};
	ntsm_hip::Buffers dev;                   /* everything below that lives on the device */
	ntsm_hip::Events<2> ev;
	ntsm_hip::Stream stream;
	ntsm_hip::Pinned pinned;                 /* the staging buffer, kStageCap + 16 bytes */
	const uint32_t *bitmap = nullptr, *off = nullptr, *idx = nullptr;
	const uint64_t *kmer = nullptr;
	uint32_t *counts[2] = {};                /* [n_cands] each, as many as the library asked for */
	unsigned long long *counters = nullptr;
	uint8_t *d_genome = nullptr;             /* kStageCap + 16 bytes */
	Stage stage;
	ScanTimes times{};

	template <typename T> int upload(const std::vector<T> &v, const T **d)
	{
		T *p;
		HIPCHK(dev.alloc(&p, v.size()));
		HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
		*d = p;
		return 0;
	}

	template <typename T> int zeroed(T **d, uint64_t n)
	{
		HIPCHK(dev.alloc(d, n));
		HIPCHK(hipMemset(*d, 0, (n ? n : 1) * sizeof(T)));
		return 0;
	}

	/* tables of the candidates, n_counts zeroed count arrays and n_counters zeroed counters, then the staging buffers.
	   shortest, carry: the setting of ntsm_sitegen_stage.h.  The device is set. */
	int open(int device_, uint32_t k_, uint64_t n_cands_, const uint64_t *cands, uint32_t shortest, uint32_t carry, int n_counts, uint32_t n_counters)
	{
		device = device_;
		k = k_;
		n_cands = n_cands_;
		double t0 = now_ms();
		HostTables h;
		if (h.build(k, n_cands, cands))
			return -1;
		parts = h;
		times.table_build_ms = now_ms() - t0;

		t0 = now_ms();
		int rc = upload(h.bitmap, &bitmap);
		if (!rc) rc = upload(h.off, &off);
		if (!rc) rc = upload(h.kmer, &kmer);
		if (!rc) rc = upload(h.idx, &idx);
		for (int j = 0; j < n_counts && !rc; j++)
			rc = zeroed(&counts[j], n_cands);
		if (!rc) rc = zeroed(&counters, n_counters);
		if (rc)
			return rc;
		HIPCHK(hipDeviceSynchronize());
		times.table_upload_ms = now_ms() - t0;
		times.table_bytes = h.bitmap.size() * 4 + h.off.size() * 4 + h.kmer.size() * 8 + h.idx.size() * 4;

		HIPCHK(stream.create());
		HIPCHK(ev.create());
		HIPCHK(pinned.alloc(kStageCap + 16));
		HIPCHK(dev.alloc(&d_genome, kStageCap + 16));
		stage.buf = pinned.bytes();
		stage.cap = kStageCap;
		stage.shortest = shortest;
		stage.carry = carry;
		return 0;
	}

	/* one launch of the stage: the timed upload, then enqueue(blocks, stream, d_genome, n, carried) between two events */
	template <typename Enqueue> int launch(const uint8_t *bytes, uint64_t n, uint32_t carried, Enqueue &&enqueue)
	{
		double t0 = now_ms();
		HIPCHK(hipMemcpyAsync(d_genome, bytes, n, hipMemcpyHostToDevice, stream));
		HIPCHK(hipStreamSynchronize(stream));
		times.upload_ms += now_ms() - t0;
		const uint64_t lanes = (n + kStretch - 1) / kStretch;
		const uint32_t blocks = (uint32_t)((lanes + kBlock - 1) / kBlock);
		HIPCHK(hipEventRecord(ev[0], stream));
		enqueue(blocks, (hipStream_t)stream, (const uint8_t *)d_genome, n, carried);
		HIPCHK(hipGetLastError());
		HIPCHK(hipEventRecord(ev[1], stream));
		HIPCHK(hipEventSynchronize(ev[1]));
		float ms = 0;
		HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
		times.kernel_ms += ms;
		if (n == stage.cap) {                               /* full launches only: their spread is the measurement's noise */
			if (!times.full_launches || ms < times.full_kernel_ms_min) times.full_kernel_ms_min = ms;
			if (ms > times.full_kernel_ms_max) times.full_kernel_ms_max = ms;
			times.full_launches++;
		}
		times.launches++;
		return 0;
	}

	/* a chunk through the stage; returns after its kernels have finished.  stage_ms: the call less its uploads and kernels */
	template <typename Enqueue> int submit(const char *bases, uint64_t n, const uint64_t *ends, uint64_t n_ends, Enqueue &&enqueue)
	{
		HIPCHK(hipSetDevice(device));
		const double t0 = now_ms(), busy0 = times.upload_ms + times.kernel_ms;
		const int rc = stage.submit(bases, n, ends, n_ends,
		                            [&](const uint8_t *bytes, uint64_t len, uint32_t carried) { return launch(bytes, len, carried, enqueue); });
		if (rc != -1)
			times.stage_ms += now_ms() - t0 - (times.upload_ms + times.kernel_ms - busy0);
		return rc;
	}

	/* out: host [n_cands], min(count, 255) of count array j */
	int hits(int j, uint8_t *out)
	{
		std::vector<uint32_t> h(n_cands ? n_cands : 1);
		HIPCHK(hipMemcpy(h.data(), counts[j], h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
		for (uint64_t i = 0; i < n_cands; i++)
			out[i] = (uint8_t)(h[i] < 255 ? h[i] : 255);
		return 0;
	}

	/* the shared fields of a library's public struct, and its first n counters into c */
	template <typename Public> int stats(Public *out, unsigned long long *c, uint32_t n)
	{
		HIPCHK(hipMemcpy(c, counters, n * sizeof *c, hipMemcpyDeviceToHost));
		out->table_build_ms = times.table_build_ms;
		out->table_upload_ms = times.table_upload_ms;
		out->stage_ms = times.stage_ms;
		out->upload_ms = times.upload_ms;
		out->kernel_ms = times.kernel_ms;
		out->full_kernel_ms_min = times.full_kernel_ms_min;
		out->full_kernel_ms_max = times.full_kernel_ms_max;
		out->launches = times.launches;
		out->full_launches = times.full_launches;
		out->genome_bytes = stage.submitted;
		out->table_bytes = times.table_bytes;
		return 0;
	}
};

}  // namespace ntsm_site

#endif
