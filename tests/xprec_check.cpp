// tests/xprec_check.cpp -- ntsm_amd/csrc/xprec.h against the x87 itself: for every case, ntsm_x87_acc(acc, p) must have the
// bits of  (double) ((long double) acc + p)  (an x87 add rounded to the 64-bit significand, then stored to a double); for
// acc = NaN both must be NaN.  Built by tests/test_eval_pca.py with g++ -O2 -std=c++11 -ffp-contract=off on x86-64, and by
// `make xprec_check` under the address and undefined-behaviour sanitizers.
//
//   xprec_check [N_RANDOM [SEED]]
//       every constructed class and N_RANDOM random operands.  Prints "ok <cases>" or the first mismatches, then one line
//       "class NAME CASES" per class and one line "branch NAME COUNT" per branch of ntsm_x87_acc (see Branch
//       below); exits 1 on any mismatch and on any branch that no case reached.
//   xprec_check dump FILE PER_CLASS SEED
//       the same cases, thinned to at most PER_CLASS of each class (evenly over the class's own order; the four random kinds
//       are classes too), written to FILE as records { double acc; long double p (16 bytes); double want } with want from
//       the x87, as above.  The class with acc = NaN is not written: no finite input of the projection leads to
//       one.  The class lines read "class NAME WRITTEN", in the file's order, and the branch counts are those of the
//       written cases alone.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

// The branches of ntsm_x87_acc.  Those that the operands and the x87's own result decide are counted here, from them
// (classify); the shift amount, the remainder, tie and carry of the RN64 step and the RN53 tie show only inside the function,
// which marks them with NTSM_XP_COUNT.
enum Branch { BR_nonfinite, BR_p_zero, BR_acc_zero, BR_swap, BR_sub, BR_gap64, BR_gap128, BR_cancel, BR_shift64, BR_shift65, BR_rn64_inexact,
              BR_rn64_tie, BR_rn64_carry, BR_rn53_tie, BR_subnormal, BR_underflow, BR_overflow, BR_rn53_tie_after_rn64, BR_COUNT };
static const char *const kBranchName[BR_COUNT] = { "nonfinite_acc", "p_zero", "acc_zero", "swap", "subtraction", "gap_ge_64", "gap_ge_128",
                                                   "exact_cancellation", "shift_ge_64", "shift_gt_64", "rn64_inexact", "rn64_tie", "rn64_carry_out", "rn53_tie",
                                                   "subnormal_result", "underflow_to_zero", "overflow", "rn53_tie_after_rn64" };
static uint64_t g_branch[BR_COUNT];
static bool g_rn64_inexact;                      // within the current ntsm_x87_acc call (check() clears it)
static void branch_hit(Branch b)
{
	++g_branch[b];
	if (b == BR_rn64_inexact) g_rn64_inexact = true;
	if (b == BR_rn53_tie && g_rn64_inexact) ++g_branch[BR_rn53_tie_after_rn64];   // the double-rounding case
}
#define NTSM_XP_COUNT(taken, branch) do { if (taken) branch_hit(BR_##branch); } while (0)

#include "../ntsm_amd/csrc/xprec.h"

static uint64_t g_state, g_seed;
static uint64_t mix(uint64_t z)
{
	z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
	z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
	return z ^ (z >> 31);
}
static uint64_t rnd()
{
	g_state += 0x9e3779b97f4a7c15ull;
	return mix(g_state);
}

enum Class { C_ZEROS, C_CANCEL, C_GAPS, C_TIES, C_SUBNORMAL, C_OVERFLOW, C_CARRY, C_NONFINITE, C_NAN, C_RND_PROJECTION, C_RND_ANYWHERE, C_RND_NEARBY,
             C_RND_SHORT, C_COUNT };
static const char *const kClassName[C_COUNT] = { "signed_zeros", "cancellation", "exponent_gaps", "ties", "subnormal_results", "overflow",
                                                 "rn64_carry_out", "infinite_acc", "nan_acc", "random_projection", "random_anywhere", "random_nearby",
                                                 "random_short" };

static_assert(sizeof(long double) == 16, "x86-64: a long double is stored in 16 bytes");

static uint64_t g_cases, g_bad;
static uint64_t g_total[C_COUNT];                // dump mode: the size of each class, from a first pass
static uint64_t g_seen[C_COUNT], g_written[C_COUNT];
static uint64_t g_per_class;
static FILE *g_dump;
static bool g_counting;                          // the first pass of dump mode: sizes only

// the branches that acc, p, their x87 sum and its double say by themselves
static void classify(double acc, long double p, long double sum, double want)
{
	if (!std::isfinite(acc)) { ++g_branch[BR_nonfinite]; return; }
	if (p == 0) { ++g_branch[BR_p_zero]; return; }
	if (want == 0 && sum != 0) ++g_branch[BR_underflow];
	if (want != 0 && std::fabs(want) < 2.2250738585072014e-308) ++g_branch[BR_subnormal];
	if (std::isinf(want)) ++g_branch[BR_overflow];
	if (acc == 0) { ++g_branch[BR_acc_zero]; return; }
	int ea, ep;
	std::frexp((long double) acc, &ea);
	std::frexp(p, &ep);
	if (std::fabs((long double) acc) < std::fabs(p)) ++g_branch[BR_swap];
	if (std::abs(ea - ep) >= 64) ++g_branch[BR_gap64];
	if (std::abs(ea - ep) >= 128) ++g_branch[BR_gap128];
	if (std::signbit(acc) != std::signbit(p)) ++g_branch[BR_sub];
	if (sum == 0) ++g_branch[BR_cancel];         // the x87 sum of two non-zero operands is zero only where it is exact
}

static void check(Class c, double acc, long double p)
{
	const uint64_t k = g_seen[c]++;
	if (g_counting) return;
	if (g_dump) {                                // the class is cut into per_class even shares; one case of each share is written
		const uint64_t total = g_total[c], per = g_per_class < total ? g_per_class : total;
		if (c == C_NAN || per == 0) return;
		const uint64_t share = (uint64_t) ((unsigned __int128) k * per / total);
		const uint64_t first = (uint64_t) (((unsigned __int128) share * total + per - 1) / per);
		const uint64_t end = (uint64_t) (((unsigned __int128) (share + 1) * total + per - 1) / per);
		if (k != first + mix(g_seed ^ ((uint64_t) c << 56) ^ share) % (end - first)) return;   // which one: a hash, so that no period of the class's loop lines up with the shares
	}
	volatile long double s = (long double) acc + p;
	const double want = (double) s;
	g_rn64_inexact = false;
	const double got = ntsm_x87_acc(acc, ntsm_x64_from_ld(p));
	classify(acc, p, s, want);
	++g_cases;
	const bool same = std::isnan(acc) ? std::isnan(want) && std::isnan(got) : std::memcmp(&want, &got, sizeof want) == 0;
	if (!same) {
		if (g_bad++ < 10)
			std::printf("MISMATCH %s acc=%a p=%La want=%a got=%a\n", kClassName[c], acc, p, want, got);
	}
	if (g_dump) {
		unsigned char r[32];                     // acc, p, want without padding between them; the six spare bytes of p are 0
		std::memset(r, 0, sizeof r);
		std::memcpy(r, &acc, 8);
		std::memcpy(r + 8, &p, 10);
		std::memcpy(r + 24, &want, 8);
		if (std::fwrite(r, sizeof r, 1, g_dump) != 1) { std::fprintf(stderr, "write failed\n"); std::exit(2); }
		++g_written[c];
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

static long double rnd_p_anywhere()   // a finite p of either sign anywhere in and beyond the double range
{
	return ld_make((int) (rnd() & 1), rnd() | (1ull << 63), -1200 - 63 + (int) (rnd() % 2400));
}

static void cases(uint64_t n)
{
	const double zeros[2] = { 0.0, -0.0 };
	// signed zeros on both sides, zero against non-zero
	for (double a : zeros) {
		for (double b : zeros) check(C_ZEROS, a, (long double) b);
		check(C_ZEROS, a, 1.0L); check(C_ZEROS, a, -3.25L); check(C_ZEROS, a, ld_make(0, 0xffffffffffffffffull, -1100));
		check(C_ZEROS, a, ld_make(1, 0x8000000000000001ull, -1140));
		check(C_ZEROS, 1.5, (long double) a); check(C_ZEROS, -dbl_of_bits(1), (long double) a);
	}
	for (int t = 0; t < 1000; ++t) {
		const double z = zeros[rnd() & 1];
		check(C_ZEROS, z, (long double) zeros[rnd() & 1]);
		check(C_ZEROS, z, rnd_p_anywhere());                                     // RN53 of p alone: subnormal, zero and infinite results too
		check(C_ZEROS, z, (long double) rnd_double_near(-1022, 1023));
		check(C_ZEROS, rnd_double_near(-1022, 1023), (long double) z);
		check(C_ZEROS, dbl_of_bits((rnd() & ((1ull << 52) - 1)) | (rnd() & 1ull) << 63), (long double) z);
	}
	// exact cancellation, and cancellation down to a few bits
	for (int t = 0; t < 20000; ++t) {
		const double a = rnd_double_near(-1020, 1000);
		check(C_CANCEL, a, -(long double) a);
		const long double nb = -(long double) a;
		check(C_CANCEL, a, std::nextafter(nb, 0.0L));
		check(C_CANCEL, a, std::nextafter(nb, nb * 2));
		// across a binade: +-2^k against 2^k - j * 2^(k-64) of the other sign; j = 1 leaves 2^(k-64), 65 bits below the window's top
		const int k = -1000 + (int) (rnd() % 2000), sk = (int) (rnd() & 1);
		check(C_CANCEL, sk ? -std::ldexp(1.0, k) : std::ldexp(1.0, k), ld_make(sk ^ 1, 0ull - (1 + rnd() % 4), k - 64));
	}
	// exponent gaps -130 ... +130 between p and acc, random significands
	for (int g = -130; g <= 130; ++g)
		for (int t = 0; t < 2000; ++t) {
			const double a = rnd_double_near(-900, 900);
			int ea;
			std::frexp(a, &ea);
			check(C_GAPS, a, ld_make((int) (rnd() & 1), rnd() | (1ull << 63), ea - 64 + g));
		}
	// ties at bit 64 (the RN64 step) and at bit 53 after RN64 (double rounding)
	for (int t = 0; t < 200000; ++t) {
		const double a = rnd_double_near(-1000, 1000);
		int ea;
		std::frexp(a, &ea);                      // |a| in [2^(ea-1), 2^ea)
		const int sa = a < 0;
		// half an ulp of the 64-bit significand of a, with low bits chosen so that the sum is a tie or near it
		const uint64_t extra = rnd() & 7;
		check(C_TIES, a, ld_make(sa ^ (int) (rnd() & 1), (1ull << 63) | extra, ea - 1 - 64 - 63));
		check(C_TIES, a, ld_make(sa ^ (int) (rnd() & 1), 0xc000000000000000ull | (extra << 10), ea - 1 - 64 - 63 + 1));
		// exact sum = a +- 2^(ea-54) (half a double ulp) +- something below 2^(ea-64): RN64 may land on the 53-bit tie
		const uint64_t lowbits = rnd() & 0x3ff;
		check(C_TIES, a, ld_make(sa ^ (int) (rnd() & 1), (1ull << 63) | lowbits, ea - 54 - 63));
		check(C_TIES, a, ld_make(sa ^ (int) (rnd() & 1), (1ull << 63) | (lowbits << 40), ea - 54 - 63));
		check(C_TIES, a, ld_make(sa ^ (int) (rnd() & 1), 0xffffffffffffffffull ^ lowbits, ea - 55 - 63));
		// exact sum = a +- (2^(ea-54) +- 2^(ea-65)): a tie at bit 64 whose either resolution is the tie at bit 53, so the evenness
		// rule of the RN64 step decides the double
		check(C_TIES, a, ld_make(sa ^ (int) (rnd() & 1), 2049ull << 52, ea - 65 - 52));
		check(C_TIES, a, ld_make(sa ^ (int) (rnd() & 1), 2047ull << 53, ea - 65 - 53));
	}
	// results in and around the double subnormal range
	for (int t = 0; t < 200000; ++t) {
		const double a = (rnd() & 3) ? rnd_double_near(-1022, -1000) : dbl_of_bits((rnd() & ((1ull << 52) - 1)) | (rnd() & 1ull) << 63);
		const int e = -1150 + (int) (rnd() % 140);
		check(C_SUBNORMAL, a, ld_make((int) (rnd() & 1), rnd() | (1ull << 63), e - 63));
		check(C_SUBNORMAL, a, -(long double) a + ld_make((int) (rnd() & 1), rnd() | (1ull << 63), -1074 - 63 - (int) (rnd() % 4)));
	}
	// overflow to infinity, and sums that stop just short of it
	check(C_OVERFLOW, 1.7976931348623157e308, 1.7976931348623157e308L);
	check(C_OVERFLOW, -1.7976931348623157e308, ld_make(1, 0xfffffffffffffc00ull, 1024 - 64));
	check(C_OVERFLOW, 1.7976931348623157e308, ld_make(0, 0x8000000000000000ull, 970 - 63));
	for (int t = 0; t < 2000; ++t) {
		const double a = rnd_double_near(1020, 1023);
		const int sa = a < 0;
		check(C_OVERFLOW, a, ld_make(sa, rnd() | (1ull << 63), 1018 - 63 + (int) (rnd() % 12)));       // same sign: most overflow
		check(C_OVERFLOW, a, ld_make(sa ^ (int) (rnd() & 1), rnd() | (1ull << 63), 1024 - 63 + (int) (rnd() % 40)));   // p beyond the double range
		// around half an ulp above the largest double: RN53 decides between DBL_MAX and infinity
		const double big = sa ? -1.7976931348623157e308 : 1.7976931348623157e308;
		check(C_OVERFLOW, big, ld_make(sa, (1ull << 63) | (rnd() & 3) << (rnd() % 62), 970 - 63 - (int) (rnd() % 2)));
	}
	// the RN64 increment carries out of the 64-bit significand: the exact sum lies within half a 64-bit ulp below a power of two
	check(C_CARRY, 1.0, -std::ldexp(1.0L, -65));
	check(C_CARRY, -4.0, std::ldexp(1.0L, -63));
	check(C_CARRY, dbl_of_bits(0x409fffffffffffffull), ld_make(0, 0xffffffffffffffffull, -46 - 60));   // 0x1.fffffffffffffp+10 + 0xf.fffffffffffffffp-46
	for (int t = 0; t < 4000; ++t) {
		const int k = -1000 + (int) (rnd() % 2024);                              // up to 2^1023: the carry may be the overflow
		const int sa = (int) (rnd() & 1);
		// +-2^k against a p of the other sign with |p| <= 2^(k-65), down to a gap beyond the window
		const double pow2 = sa ? -std::ldexp(1.0, k) : std::ldexp(1.0, k);
		const int drop = (rnd() & 3) ? (int) (rnd() % 8) : (int) (rnd() % 200);
		check(C_CARRY, pow2, ld_make(sa ^ 1, drop == 0 ? 1ull << 63 : rnd() | (1ull << 63), k - 65 - 63 - drop));
		// +-(2^(k+1) - 2^(k-52)), all 53 bits set, against a p of the same sign just below 2^(k-52): (2^64 - j) * 2^(k-116), j <= 2^52
		const double ones = dbl_of_bits(((uint64_t) sa << 63) | ((uint64_t) (k + 1023) << 52) | ((1ull << 52) - 1));
		const uint64_t j = (rnd() & 1) ? 1 + rnd() % 4096 : 1 + rnd() % (1ull << 52);
		check(C_CARRY, ones, ld_make(sa, 0ull - j, k - 116));
		// a random double in [2^(k-1), 2^k) and the p that brings it to all 64 ones plus half an ulp (a tie that rounds up) or
		// plus three quarters of one: target - a is exact, and below 2^(k-1) or 2^(k-3) it leaves p room for the extra bits
		const bool tie = rnd() & 1;
		const uint64_t frac = tie ? rnd() & ((1ull << 51) - 1) : (3ull << 50) | (rnd() & ((1ull << 50) - 1));
		const double a = dbl_of_bits(((uint64_t) sa << 63) | ((uint64_t) (k - 1 + 1023) << 52) | frac);
		const long double target = ld_make(sa, 0xffffffffffffffffull, k - 64);  // 2^k - 2^(k-64)
		check(C_CARRY, a, (target - (long double) a) + ld_make(sa, tie ? 1ull << 63 : 3ull << 62, k - 65 - 63));
	}
	// an accumulator that has overflowed stays where it is, whatever finite p follows
	const double inf = HUGE_VAL, nan = std::nan("");
	for (double a : { inf, -inf }) {
		check(C_NONFINITE, a, 0.0L); check(C_NONFINITE, a, -0.0L);
		check(C_NONFINITE, a, -1e308L); check(C_NONFINITE, a, 1.7e308L); check(C_NONFINITE, a, -1.7e308L);
		check(C_NONFINITE, a, std::ldexp(1.0L, 1024)); check(C_NONFINITE, a, -std::ldexp(1.0L, 1024)); check(C_NONFINITE, a, std::ldexp(1.0L, 1023));
		check(C_NONFINITE, a, -std::ldexp(1.0L, 1025));
		check(C_NONFINITE, a, 1.0L); check(C_NONFINITE, a, -1.0L); check(C_NONFINITE, a, std::ldexp(1.0L, -1074)); check(C_NONFINITE, a, -std::ldexp(1.0L, -1200));
	}
	for (int t = 0; t < 1000; ++t) {
		const double a = (rnd() & 1) ? inf : -inf;
		check(C_NONFINITE, a, rnd_p_anywhere());
		check(C_NONFINITE, a, ld_make((int) (rnd() & 1), rnd() | (1ull << 63), 1000 - 63 + (int) (rnd() % 60)));   // around 2^1024, both signs
		check(C_NONFINITE, a, (long double) rnd_double_near(-1022, 1023));
		check(C_NONFINITE, a, (long double) zeros[rnd() & 1]);
	}
	// NaN stays NaN, whatever its sign and payload (compared as NaN, not by bits; not dumped)
	for (int t = 0; t < 200; ++t) {
		const double a = t < 2 ? (t ? -nan : nan) : dbl_of_bits((0x7ffull << 52) | (1 + rnd() % ((1ull << 52) - 1)) | (rnd() & 1ull) << 63);
		check(C_NAN, a, t & 1 ? rnd_p_anywhere() : (long double) zeros[(t >> 1) & 1]);
	}
	// random operands of the projection's kind: acc = a running sum, p = RN64(v * rot) with v = c - norm, rot long double
	for (uint64_t t = 0; t < n; ++t) {
		const uint64_t r = rnd();
		double a;
		long double p;
		Class c;
		switch (r & 3) {
		case 0: {                                // the projection's own operands
			const long double norm = std::ldexp((long double) (rnd() | (1ull << 63)), -64);
			const double v = (double) ((long double) ((rnd() % 3) * 0.5) - norm);
			const long double rot = std::ldexp((long double) (rnd() | (1ull << 63)), -64 - (int) (rnd() % 12)) * ((rnd() & 1) ? -1 : 1);
			a = rnd_double_near(-20, 8);
			p = (long double) v * rot;
			c = C_RND_PROJECTION;
			break;
		}
		case 1:                                  // anywhere in the range
			a = rnd_double_near(-1022, 1000);
			p = ld_make((int) (rnd() & 1), rnd() | (1ull << 63), -1022 - 63 + (int) (rnd() % 2000));
			c = C_RND_ANYWHERE;
			break;
		case 2: {                                // nearby exponents
			a = rnd_double_near(-60, 60);
			int ea;
			std::frexp(a, &ea);
			p = ld_make((int) (rnd() & 1), rnd() | (1ull << 63), ea - 64 + (int) (rnd() % 141) - 70);
			c = C_RND_NEARBY;
			break;
		}
		default:                                 // short significands (exact sums are common)
			a = (double) (int64_t) (rnd() % 2000001 - 1000000) * std::ldexp(1.0, (int) (rnd() % 40) - 20);
			p = ld_make((int) (rnd() & 1), (rnd() & 0xffff000000000000ull) | (1ull << 63), (int) (rnd() % 40) - 20 - 63);
			c = C_RND_SHORT;
			break;
		}
		check(c, a, p);
	}
}

int main(int argc, char **argv)
{
	const bool dump = argc > 1 && std::strcmp(argv[1], "dump") == 0;
	if (dump && argc != 5) { std::fprintf(stderr, "usage: xprec_check [N_RANDOM [SEED]] | xprec_check dump FILE PER_CLASS SEED\n"); return 2; }
	uint64_t n = !dump && argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 10000000ull;
	g_seed = dump ? std::strtoull(argv[4], nullptr, 10) : argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1;
	if (dump) {
		g_per_class = std::strtoull(argv[3], nullptr, 10);
		n = 8 * g_per_class;                     // about twice PER_CLASS of each random kind
		g_counting = true;
		g_state = g_seed;
		cases(n);
		std::memcpy(g_total, g_seen, sizeof g_total);
		std::memset(g_seen, 0, sizeof g_seen);
		g_counting = false;
		g_dump = std::fopen(argv[2], "wb");
		if (!g_dump) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
	}
	g_state = g_seed;
	cases(n);
	if (g_dump && std::fclose(g_dump) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
	if (g_bad) { std::printf("%llu of %llu cases differ\n", (unsigned long long) g_bad, (unsigned long long) g_cases); return 1; }
	std::printf("ok %llu\n", (unsigned long long) g_cases);
	for (int c = 0; c < C_COUNT; ++c) std::printf("class %s %llu\n", kClassName[c], (unsigned long long) (dump ? g_written[c] : g_seen[c]));
	int unreached = 0;
	for (int b = 0; b < BR_COUNT; ++b) {
		std::printf("branch %s %llu\n", kBranchName[b], (unsigned long long) g_branch[b]);
		unreached += g_branch[b] == 0;
	}
	if (unreached) { std::printf("%d branches were reached by no case\n", unreached); return 1; }
	return 0;
}
