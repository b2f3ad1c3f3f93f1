/*
 * xprec.h -- the x87 extended-precision accumulation step of ntsmEval's PCA projection, in integer arithmetic, for the
 * host and the device (include/ntsm_eval_hip.h: ntsm_eval_project).
 *
 * The reference projects a sample with  m_cloud[i][d] = inner_product(vals, rotVals[d], 0.0)  (src/CompareCounts.hpp:
 * 207-210): the accumulator is a double, the rotation values are long double, so on x86-64 every step is
 *   acc = RN53(RN64(acc + RN64(v_j * rot[d][j])))
 * (x87 product and sum rounded to the 64-bit significand, then stored to a double).  The host computes the products with
 * real long double (ntsm_x64_from_ld); ntsm_x87_acc does the rest with integers: the two operands are aligned in a
 * 128-bit window with a sticky bit, added or subtracted, normalised by clz, rounded to 64 bits (RNE) and then to a double
 * (RNE, gradual underflow, overflow to infinity).  Correct for every finite p and every acc: the x87 exponent range is taken
 * as unbounded, which it is for every sum of a double and an x87 product of a double and a finite long double that does
 * not itself underflow the x87 range.  An accumulator that has overflowed stays where it is, as on the x87: acc = +-inf or
 * NaN is returned unchanged (inf +- finite = inf).  Outside the promise: a p that is itself infinite or NaN (ntsm_x64 has no
 * encoding for one), i.e. RN64(v * rot) beyond the x87 range, and a centre value beyond DBL_MAX.  Plain C++: compiled by g++
 * for the CPU test (tests/xprec_check.cpp through tests/test_eval_pca.py) and by hipcc for the kernel.
 *
 * NTSM_XP_COUNT(taken, branch) marks what nothing outside the function can see (the shift amount, the remainder, tie and carry of
 * the RN64 step, the RN53 tie) for tests/xprec_check.cpp, which defines it before the include to count them; it expands
 * to nothing everywhere else.
 */
#ifndef NTSM_XPREC_H
#define NTSM_XPREC_H
#include <stdint.h>

#ifndef NTSM_XP_COUNT
#define NTSM_XP_COUNT(taken, branch)
#endif

#if defined(__HIPCC__)
#define NTSM_XP_FN __host__ __device__ inline
#else
#define NTSM_XP_FN inline
#endif

/* value = (-1)^sign * sig * 2^exp; sig == 0 is a zero of that sign (sig need not be normalised) */
typedef struct ntsm_x64 {
	uint64_t sig;
	int32_t exp;
	uint32_t sign;
} ntsm_x64;

typedef unsigned __int128 ntsm_u128;

NTSM_XP_FN int ntsm_xp_clz64(uint64_t x) { return x ? __builtin_clzll(x) : 64; }

NTSM_XP_FN double ntsm_xp_bits_to_double(uint64_t b)
{
	double d;
	__builtin_memcpy(&d, &b, sizeof d);
	return d;
}

/* RN53 of (-1)^sign * sig * 2^e, sig with bit 63 set */
NTSM_XP_FN double ntsm_xp_rn53(uint32_t sign, uint64_t sig, int e)
{
	const uint64_t s = (uint64_t) (sign & 1u) << 63;
	int shift = (e + 63 >= -1022) ? 11 : -1074 - e;             /* bits dropped: to 53 bits, or to the 2^-1074 quantum */
	if (shift > 64) return ntsm_xp_bits_to_double(s);           /* below 2^-1075: rounds to a zero */
	uint64_t q, rem, half;
	if (shift == 64) { q = 0; rem = sig; half = 1ull << 63; }
	else { q = sig >> shift; rem = sig & ((1ull << shift) - 1); half = 1ull << (shift - 1); }
	NTSM_XP_COUNT(rem == half, rn53_tie);
	if (rem > half || (rem == half && (q & 1))) ++q;
	if (shift != 11) return ntsm_xp_bits_to_double(s | q);    /* subnormal (q == 2^52 is the smallest normal: the carry is the exponent) */
	int be = e + 63 + 1023;
	if (q == (1ull << 53)) { q >>= 1; ++be; }
	if (be >= 2047) return ntsm_xp_bits_to_double(s | (0x7ffull << 52));
	return ntsm_xp_bits_to_double(s | ((uint64_t) be << 52) | (q & ((1ull << 52) - 1)));
}

/* RN53(RN64(acc + p)) for finite p; acc = +-inf or NaN comes back unchanged */
NTSM_XP_FN double ntsm_x87_acc(double acc, ntsm_x64 p)
{
	uint64_t ab;
	__builtin_memcpy(&ab, &acc, sizeof ab);
	uint32_t sa = (uint32_t) (ab >> 63), sb = p.sign & 1u;
	const uint32_t be = (uint32_t) (ab >> 52) & 0x7ffu;
	uint64_t ma = ab & ((1ull << 52) - 1), mb = p.sig;
	int ea = -1074, eb = p.exp;
	if (be == 0x7ffu) return acc;                                               /* inf +- finite = inf; NaN stays NaN */
	if (be) { ma |= 1ull << 52; ea = (int) be - 1075; }
	if (mb == 0) {
		if (ma == 0) return ntsm_xp_bits_to_double((uint64_t) (sa & sb) << 63);   /* (-0) + (-0) = -0, else +0 */
		return acc;                                                             /* exact */
	}
	int lz = ntsm_xp_clz64(mb);
	mb <<= lz; eb -= lz;
	if (ma == 0) return ntsm_xp_rn53(sb, mb, eb);                               /* p has 64 bits: RN64(p) = p */
	lz = ntsm_xp_clz64(ma);
	ma <<= lz; ea -= lz;
	if (ea < eb || (ea == eb && ma < mb)) {                                     /* a: the larger magnitude */
		uint64_t t = ma; ma = mb; mb = t;
		int te = ea; ea = eb; eb = te;
		uint32_t ts = sa; sa = sb; sb = ts;
	}
	/* window: a at bits 126..63 (weight of bit 0: 2^(ea-63)), b shifted right by the exponent gap; bits shifted out
	 * are jammed into bit 0 (they exist only for a gap > 63, where the result keeps its top bit at 126 or 127 and the
	 * rounding position lies far above bit 0) */
	const ntsm_u128 X = (ntsm_u128) ma << 63, B = (ntsm_u128) mb << 63;
	const int d = ea - eb;
	ntsm_u128 Y;
	if (d == 0) Y = B;
	else if (d < 128) Y = (B >> d) | (ntsm_u128) ((B & (((ntsm_u128) 1 << d) - 1)) != 0);
	else Y = 1;
	ntsm_u128 R = sa == sb ? X + Y : X - Y;
	if (R == 0) return 0.0;                                                     /* exact cancellation: +0 */
	const uint64_t rh = (uint64_t) (R >> 64), rl = (uint64_t) R;
	const int n = rh ? ntsm_xp_clz64(rh) : 64 + ntsm_xp_clz64(rl);
	NTSM_XP_COUNT(n >= 64, shift64);
	NTSM_XP_COUNT(n > 64, shift65);                                             /* 65 at the most: 2^k against 2^k - 2^(k-64) */
	R <<= n;
	uint64_t hi = (uint64_t) (R >> 64);
	const uint64_t lo = (uint64_t) R;
	int e = ea + 1 - n;                                                         /* value = hi * 2^e (+ lo) */
	NTSM_XP_COUNT(lo != 0, rn64_inexact);
	NTSM_XP_COUNT(lo == (1ull << 63), rn64_tie);
	if (lo > (1ull << 63) || (lo == (1ull << 63) && (hi & 1))) {               /* RN64 */
		if (++hi == 0) { hi = 1ull << 63; ++e; NTSM_XP_COUNT(true, rn64_carry); }
	}
	return ntsm_xp_rn53(sa, hi, e);
}

#if defined(__HIPCC__)
#define NTSM_XP_HOST __host__ static inline
#else
#define NTSM_XP_HOST static inline
#endif
#include <string.h>
/* an x87 long double (80-bit, 16-byte storage on x86-64; host only) as an ntsm_x64 (finite values) */
NTSM_XP_HOST ntsm_x64 ntsm_x64_from_ld(long double x)
{
	unsigned char b[16];
	memcpy(b, &x, sizeof b);
	uint64_t sig;
	uint16_t se;
	memcpy(&sig, b, 8);
	memcpy(&se, b + 8, 2);
	const int e = se & 0x7fff;
	ntsm_x64 r;
	r.sig = sig;
	r.exp = (e ? e : 1) - 16383 - 63;
	r.sign = se >> 15;
	return r;
}

#endif
