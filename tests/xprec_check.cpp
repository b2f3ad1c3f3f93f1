// tests/xprec_check.cpp -- ntsm_amd/csrc/xprec.h against the x87 itself: for every case, ntsm_x87_acc(acc, p) must have the
// bits of  (double) ((long double) acc + p)  (an x87 add rounded to the 64-bit significand, then stored to a double).
// Built by tests/test_eval_pca.py with g++ -O2 -std=c++11 -ffp-contract=off on x86-64.  Usage: xprec_check N_RANDOM SEED
// Prints "ok <cases>" or the first mismatches, and exits 1 on any mismatch.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../ntsm_amd/csrc/xprec.h"

static uint64_t g_state;
static uint64_t rnd()
{
	g_state += 0x9e3779b97f4a7c15ull;
	uint64_t z = g_state;
	z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
	z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
	return z ^ (z >> 31);
}

static uint64_t g_cases, g_bad;

static void check(double acc, long double p)
{
	volatile long double s = (long double) acc + p;
	const double want = (double) s;
	const double got = ntsm_x87_acc(acc, ntsm_x64_from_ld(p));
	++g_cases;
	if (std::memcmp(&want, &got, sizeof want) != 0) {
		if (g_bad++ < 10)
			std::printf("MISMATCH acc=%a p=%La want=%a got=%a\n", acc, p, want, got);
	}
}

static double dbl_of_bits(uint64_t b) { double d; std::memcpy(&d, &b, 8); return d; }

static long double ld_make(int sign, uint64_t sig, int e)   // (-1)^sign * sig * 2^e, sig with bit 63 set (exact)
{
	const long double v = std::ldexp((long double) sig, e);
	return sign ? -v : v;
}

static double rnd_double_near(int lo, int hi)   // random normal double with unbiased exponent in [lo, hi]
{
	const int e = lo + (int) (rnd() % (uint64_t) (hi - lo + 1));
	const uint64_t b = ((uint64_t) (e + 1023) << 52) | (rnd() & ((1ull << 52) - 1)) | (rnd() & 1ull) << 63;
	return dbl_of_bits(b);
}

int main(int argc, char **argv)
{
	const uint64_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 10000000ull;
	g_state = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
	const double zeros[2] = { 0.0, -0.0 };
	// signed zeros on both sides, zero against non-zero
	for (double a : zeros) {
		for (double b : zeros) check(a, (long double) b);
		check(a, 1.0L); check(a, -3.25L); check(a, ld_make(0, 0xffffffffffffffffull, -1100)); check(a, ld_make(1, 0x8000000000000001ull, -1140));
		check(1.5, (long double) a); check(-dbl_of_bits(1), (long double) a);
	}
	// exact cancellation, and cancellation down to a few bits
	for (int t = 0; t < 20000; ++t) {
		const double a = rnd_double_near(-1100 + 1023 + 80 > 0 ? -1020 : -1020, 1000);
		check(a, -(long double) a);
		const long double nb = -(long double) a;
		check(a, std::nextafter(nb, 0.0L));
		check(a, std::nextafter(nb, nb * 2));
	}
	// exponent gaps -130 ... +130 between p and acc, random significands
	for (int g = -130; g <= 130; ++g)
		for (int t = 0; t < 2000; ++t) {
			const double a = rnd_double_near(-900, 900);
			int ea;
			std::frexp(a, &ea);
			check(a, ld_make((int) (rnd() & 1), rnd() | (1ull << 63), ea - 64 + g));
		}
	// ties at bit 64 (the RN64 step) and at bit 53 after RN64 (double rounding)
	for (int t = 0; t < 200000; ++t) {
		const double a = rnd_double_near(-1000, 1000);
		int ea;
		std::frexp(a, &ea);                      // |a| in [2^(ea-1), 2^ea)
		const int sa = a < 0;
		// half an ulp of the 64-bit significand of a, with low bits chosen so that the sum is a tie or near it
		const uint64_t extra = rnd() & 7;
		check(a, ld_make(sa ^ (int) (rnd() & 1), (1ull << 63) | extra, ea - 1 - 64 - 63));
		check(a, ld_make(sa ^ (int) (rnd() & 1), 0xc000000000000000ull | (extra << 10), ea - 1 - 64 - 63 + 1));
		// exact sum = a +- 2^(ea-54) (half a double ulp) +- something below 2^(ea-64): RN64 may land on the 53-bit tie
		const uint64_t lowbits = rnd() & 0x3ff;
		check(a, ld_make(sa ^ (int) (rnd() & 1), (1ull << 63) | lowbits, ea - 54 - 63));
		check(a, ld_make(sa ^ (int) (rnd() & 1), (1ull << 63) | (lowbits << 40), ea - 54 - 63));
		check(a, ld_make(sa ^ (int) (rnd() & 1), 0xffffffffffffffffull ^ lowbits, ea - 55 - 63));
	}
	// results in and around the double subnormal range
	for (int t = 0; t < 200000; ++t) {
		const double a = (rnd() & 3) ? rnd_double_near(-1022, -1000) : dbl_of_bits((rnd() & ((1ull << 52) - 1)) | (rnd() & 1ull) << 63);
		const int e = -1150 + (int) (rnd() % 140);
		check(a, ld_make((int) (rnd() & 1), rnd() | (1ull << 63), e - 63));
		check(a, -(long double) a + ld_make((int) (rnd() & 1), rnd() | (1ull << 63), -1074 - 63 - (int) (rnd() % 4)));
	}
	// overflow to infinity
	check(1.7976931348623157e308, 1.7976931348623157e308L);
	check(-1.7976931348623157e308, ld_make(1, 0xfffffffffffffc00ull, 1024 - 64));
	check(1.7976931348623157e308, ld_make(0, 0x8000000000000000ull, 970 - 63));
	// random operands of the projection's kind: acc = a running sum, p = RN64(v * rot) with v = c - norm, rot long double
	for (uint64_t t = 0; t < n; ++t) {
		const uint64_t r = rnd();
		double a;
		long double p;
		switch (r & 3) {
		case 0: {                                // the projection's own operands
			const long double norm = std::ldexp((long double) (rnd() | (1ull << 63)), -64);
			const double v = (double) ((long double) ((rnd() % 3) * 0.5) - norm);
			const long double rot = std::ldexp((long double) (rnd() | (1ull << 63)), -64 - (int) (rnd() % 12)) * ((rnd() & 1) ? -1 : 1);
			a = rnd_double_near(-20, 8);
			p = (long double) v * rot;
			break;
		}
		case 1:                                  // anywhere in the range
			a = rnd_double_near(-1022, 1000);
			p = ld_make((int) (rnd() & 1), rnd() | (1ull << 63), -1022 - 63 + (int) (rnd() % 2000));
			break;
		case 2: {                                // nearby exponents
			a = rnd_double_near(-60, 60);
			int ea;
			std::frexp(a, &ea);
			p = ld_make((int) (rnd() & 1), rnd() | (1ull << 63), ea - 64 + (int) (rnd() % 141) - 70);
			break;
		}
		default:                                 // short significands (exact sums are common)
			a = (double) (int64_t) (rnd() % 2000001 - 1000000) * std::ldexp(1.0, (int) (rnd() % 40) - 20);
			p = ld_make((int) (rnd() & 1), (rnd() & 0xffff000000000000ull) | (1ull << 63), (int) (rnd() % 40) - 20 - 63);
			break;
		}
		check(a, p);
	}
	if (g_bad) { std::printf("%llu of %llu cases differ\n", (unsigned long long) g_bad, (unsigned long long) g_cases); return 1; }
	std::printf("ok %llu\n", (unsigned long long) g_cases);
	return 0;
}
