/*
 * kernels_common.h -- what the gfx950 count kernels share, each piece stated once: launch geometry, the boundary-safe 16-byte
 * stream load, the swizzled LDS tile address, the four-bit filter test, the queue-push rank, the key-table slot look-up,
 * per-read attribution, the in-wave sum of equal hits and the totals.  Device code only; included by every
 * kernel translation unit (kernels_generic.hip, kernels_mz.hip with ntsm_tab_kernel.inc, kernels_run.hip).
 *
 * Replaces nothing of the reference by itself: the kernels built on it replace the loop of FingerPrint::insertCount
 * (src/FingerPrint.hpp:89-103).
 */
#ifndef NTSM_KERNELS_COMMON_H
#define NTSM_KERNELS_COMMON_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ntsm_device.h"
#include "ntsm_hooks.h"

typedef uint32_t ntsm_u32x4 __attribute__((ext_vector_type(4)));
typedef int ntsm_i32x4 __attribute__((ext_vector_type(4)));
/* buffer_load_dwordx4 ... idxen: clang has a builtin for the raw (byte offset) form only, so the LLVM intrinsic is
 * declared by name.  (descriptor, index, byte offset inside the element, scalar offset, cache policy) */
__device__ ntsm_u32x4 ntsm_struct_buffer_load_b128(ntsm_i32x4 rsrc, int vindex, int voffset, int soffset, int aux)
		__asm("llvm.amdgcn.struct.buffer.load.v4i32");
__device__ uint32_t ntsm_struct_buffer_load_b32(ntsm_i32x4 rsrc, int vindex, int voffset, int soffset, int aux)
		__asm("llvm.amdgcn.struct.buffer.load.i32");

namespace {

#ifndef NTSM_STREAM_NT
#define NTSM_STREAM_NT 1                                /* read stream: non-temporal loads (read once) */
#endif
#if NTSM_STREAM_NT && !defined(NTSM_STREAM_AUX)
#define NTSM_STREAM_AUX 2                               /* minimizer-blocked kernels, interior tiles: buffer loads with the nt bit */
#endif
constexpr int kThreads = 256;
constexpr uint32_t kN4 = 0x4E4E4E4Eu;      /* "NNNN" */

__device__ __forceinline__ uint4 ntsm_load_vec(const NtsmCountParams &p, long long o)
{
	uint4 r = make_uint4(kN4, kN4, kN4, kN4);
	if (o + 16 > p.lo && o < p.hi) {
#if NTSM_STREAM_NT
		const ntsm_u32x4 nt = __builtin_nontemporal_load(reinterpret_cast<const ntsm_u32x4 *>(p.base + o));
#else
		const ntsm_u32x4 nt = *reinterpret_cast<const ntsm_u32x4 *>(p.base + o);
#endif
		r = make_uint4(nt.x, nt.y, nt.z, nt.w);
		if (o < p.lo || o + 16 > p.hi) {                    /* first / last vector of the range */
			uint32_t w[4] = { r.x, r.y, r.z, r.w };
			for (int b = 0; b < 16; ++b) {
				long long pos = o + b;
				if (pos < p.lo || pos >= p.hi)
					w[b >> 2] = (w[b >> 2] & ~(0xFFu << ((b & 3) * 8))) | (0x4Eu << ((b & 3) * 8));
			}
			r = make_uint4(w[0], w[1], w[2], w[3]);
		}
	}
	return r;
}

/* LDS image of a tile: row r (C bytes) = stream bytes of thread r-1 (row 0 = the 32 bytes in front of the tile, in its
 * last two slots).  The 16-byte slots of a row are permuted per row so that the per-thread ds_read_b64 of "slot s of my
 * row" spreads over the banks without padding: C = 128: slot s sits at s ^ ((r >> 1) & 7) (conflict free); other C:
 * rotated by r >> 3 (two-way). */
template <int C>
__device__ __forceinline__ int ntsm_tile_addr(int row, int byte_in_row)
{
	if (C == 128) return row * C + ((((byte_in_row >> 4) ^ (row >> 1)) & 7) << 4) + (byte_in_row & 15);
	return row * C + (int) ((((uint32_t) (byte_in_row >> 4) + ((uint32_t) row >> 3)) % (uint32_t) (C / 16)) << 4) + (byte_in_row & 15);
}

/* reverse complement of a 16-base word (oldest base in the top bits): complement, reverse the bits, swap inside the pairs */
__device__ __forceinline__ uint32_t ntsm_rc16(uint32_t w)
{
	const uint32_t y = __builtin_bitreverse32(~w);
	return ((y >> 1) & 0x55555555u) | ((y & 0x55555555u) << 1);
}

/* Four-bit test of a 128-bit filter block: word << field (NTSM_KBITn: bit 31 - field) puts the tested bit in the sign
 * position -- the shifter takes the low five bits of the selected byte, so the fields need no mask -- and the sign of the
 * AND of the four is the verdict.  u: the k-mer's (anchored 16-mer's) strand-symmetric sum, um = ntsm_kmer_mix(u). */
__device__ __forceinline__ bool ntsm_block_test(const uint32_t &u, const uint32_t &um, const uint4 &blk)
{
	uint32_t s0, s1, s2, s3;
	asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(s0) : "v"(u), "v"(blk.x));
	asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_3 src1_sel:DWORD" : "=v"(s1) : "v"(um), "v"(blk.y));
	asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2 src1_sel:DWORD" : "=v"(s2) : "v"(um), "v"(blk.z));
	asm("v_lshlrev_b32_sdwa %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:DWORD" : "=v"(s3) : "v"(um), "v"(blk.w));
	return (int32_t) (__builtin_amdgcn_bitop3_b32(s0, s1, s2, 0x80) & s3) < 0;
}

/* queue push: base + the number of lanes below this one that are set in the ballot mask */
__device__ __forceinline__ uint32_t ntsm_mask_rank(unsigned long long mask, uint32_t base)
{
	return __builtin_amdgcn_mbcnt_hi((uint32_t) (mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) mask, base));
}

/* Key table layout: 32-byte buckets { key0, key1, count0, count1 } -- the counter of a slot sits in the cache line
 * its key was just read from, so the atomic of a hit finds the line in L2 instead of costing a second
 * Infinity-Cache access.  Slot s = 2 * bucket + position. */
__device__ __forceinline__ unsigned long long *ntsm_count_ptr(const uint64_t *table, long long slot)
{
	return const_cast<unsigned long long *>(reinterpret_cast<const unsigned long long *>(table)) + 4 * (slot >> 1) + 2 + (slot & 1);
}

/* slot of key { klo, khi } in bucket b (first slot 2 * b, its two keys in `bucket`), or -1: for the kernel that has both buckets
 * loaded (kernels_generic.hip) */
__device__ __forceinline__ long long ntsm_slot_in_bucket(const uint4 &bucket, unsigned long long b, uint32_t klo, uint32_t khi)
{
	if (bucket.x == klo && bucket.y == khi) return (long long) b;
	if (bucket.z == klo && bucket.w == khi) return (long long) b + 1;
	return -1;
}

/* Slot of a key whose first bucket b1 has been loaded (ba), or -1.  The second bucket (hash g2) is read only when the first
 * is full and does not hold the key: the host places a key in the first empty slot of bucket 1, then of bucket 2, keys are
 * never removed, and a key evicted by the cuckoo walk is placed by the same rule (tables.cpp, the `placed` loop of the
 * table build) -- so a key sits in bucket 2 only if bucket 1 was full when it went in, and is full still.  An empty slot's
 * key is all ones.  One else-if chain, not two calls of ntsm_slot_in_bucket: built on that helper the look-up compiles to
 * selects where this compiles to branches, different code in every count kernel (profiles/r13_count_kernels/forms.txt). */
__device__ __forceinline__ long long ntsm_find_slot(const uint64_t *keys, const uint4 &ba, unsigned long long b1, uint32_t g2, uint32_t bshift,
		uint32_t klo, uint32_t khi)
{
	long long slot = -1;
	if (ba.x == klo && ba.y == khi) slot = (long long) b1;
	else if (ba.z == klo && ba.w == khi) slot = (long long) b1 + 1;
	else if ((ba.x & ba.y) != 0xFFFFFFFFu && (ba.z & ba.w) != 0xFFFFFFFFu) {
		const unsigned long long b2 = 2ull * (g2 >> bshift);
		const uint4 bb = *reinterpret_cast<const uint4 *>(keys + 2ull * b2);
		if (bb.x == klo && bb.y == khi) slot = (long long) b2;
		else if (bb.z == klo && bb.w == khi) slot = (long long) b2 + 1;
	}
	return slot;
}

/* first read whose terminator lies beyond byte offset pos */
__device__ __forceinline__ unsigned long long ntsm_read_of(const NtsmCountParams &p, unsigned long long pos)
{
	unsigned long long lo = 0, hi = p.n_reads;
	while (lo < hi) {
		unsigned long long mid = (lo + hi) >> 1;
		if (p.read_end[mid] > pos) hi = mid; else lo = mid + 1;
	}
	return lo;
}

/* Counter update of the lanes that found their k-mer (slot >= 0; every lane of the wave must call this together).
 * One 64-bit atomic per hit -- unless lanes of this wave hit the SAME counter (low-complexity input whose k-mer is a site
 * k-mer: every lane, every time): equal slots are added up inside the wave first.  Rounds: the lowest lane that still has
 * a hit broadcasts its slot, the lanes with that slot are counted by a ballot and leave, the lowest lane adds their number.
 * A round that finds a single lane ends the search (ordinary traffic: hits spread over 1.5 M counters, one round of ~8
 * scalar / vector instructions); whoever is left adds 1 by itself.  (A workgroup-wide LDS accumulator behind this was built and
 * measured out: inlined or as a call it pushed the k = 19 kernel from 122 VGPRs to 128 + scratch.)  src/FingerPrint.hpp:94-95 (`m_counts[*itr] += 1`
 * under `omp atomic`) with the same result: integer adds commute. */
__device__ __forceinline__ void ntsm_add_hits(const NtsmCountParams &p, long long slot, int lane)
{
	bool act = slot >= 0;
	unsigned long long am = __builtin_amdgcn_ballot_w64(act);
	while (am) {
		const int leader = __builtin_ctzll(am);
		const uint32_t lo = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) slot, leader);
		const uint32_t hi = (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) ((unsigned long long) slot >> 32), leader);
		const bool same = act && (uint32_t) slot == lo && (uint32_t) ((unsigned long long) slot >> 32) == hi;
		const unsigned long long grp = __builtin_amdgcn_ballot_w64(same);
		const unsigned long long cnt = (unsigned long long) __popcll(grp);
		if (lane == leader)
			__hip_atomic_fetch_add(ntsm_count_ptr(p.keys, slot), p.sign * cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
		act = act && !same;
		am &= ~grp;
		if (cnt == 1) break;
	}
	if (act) __hip_atomic_fetch_add(ntsm_count_ptr(p.keys, slot), p.sign, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* sum of a per-lane value over the wave; lane 0 holds it */
template <typename T>
__device__ __forceinline__ T ntsm_wave_sum(T v)
{
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
	return v;
}

/* A wave's valid windows and hits into p.totals: one 64-bit atomic per wave and counter, by the wave's first lane.  The
 * caller says how its numbers come: wave-uniform as they are, per-lane through ntsm_wave_sum().  (Generic and tabulated
 * kernels; the minimizer-blocked and run-anchored kernels keep their own three lines, see there.) */
__device__ __forceinline__ void ntsm_add_totals(const NtsmCountParams &p, unsigned long long nk_wave, unsigned long long nh_wave, int t)
{
	if ((t & 63) == 0) {
		if (nk_wave) atomicAdd(p.totals + 0, p.sign * nk_wave);
		if (nh_wave) atomicAdd(p.totals + 1, p.sign * nh_wave);
	}
}

} // namespace
#endif
