/*
 * tests/sitegen_stage_check.cpp -- the staging state machine of ntsmSiteGen's device libraries
 * (ntsm_amd/csrc/ntsm_sitegen_stage.h) on the CPU, with buffers of 64 and 256 bytes where the libraries have 2^27.
 * Built with -fsanitize=address,undefined and run by tests/test_sitegen.py.
 *
 * For k in {11, 19, 31}, both settings (shortest k, carry k - 1; shortest k - 1, carry k) and both capacities, a text over
 * ACGTacgtN in records of 0, 1, k - 2, k - 1, k, k + 1, cap - 1, cap, cap + 1 and 3 cap + 7 bytes and some more, one of
 * which ends at a buffer fill of cap - 1 (its separator is the last byte of a launch) and one at cap (its separator is the
 * first fresh byte of the next), goes through submit whole and in chunks of 1, k - 1, k, k + 1, cap - 1, cap and cap + 1
 * bytes; an end on a chunk seam is passed as offset 0 of the chunk behind it.  Checked:
 *  (a) every launch: n a multiple of 16, at most cap + 15, 'N' from the staged bytes to n, carried at most the carry;
 *  (b) for m in {k - 1, k, k + 1} (m = k alone in the first setting) the windows of m valid bytes that end at a byte
 *      >= carried of a launch, summed over the launches, are as many as a split of the records at the other bytes gives;
 *  (c) descending ends, an end beyond n and a repeated end return -1 and stage nothing;
 *  (d) `submitted` is the sum of the accepted submits.
 * Prints "stage check ok: <cases> cases, <launches> launches" and exits 0, or the first failure and exits 1.
 */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../ntsm_amd/csrc/ntsm_sitegen_stage.h"

using ntsm_site::Stage;

static uint64_t rng_state = 12345;
static uint32_t rnd(uint32_t n)
{
	rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
	return (uint32_t)((rng_state >> 33) % n);
}

static bool valid(uint8_t c)
{
	c &= 0xdf;
	return c == 'A' || c == 'C' || c == 'G' || c == 'T';
}

static std::string bases(uint64_t len, bool with_n)
{
	std::string s(len, 'A');
	for (char &c : s)
		c = with_n && rnd(40) == 0 ? 'N' : "ACGTacgt"[rnd(8)];
	return s;
}

/* windows of m valid bytes that end in [from, n) of g */
static uint64_t windows(const uint8_t *g, uint64_t n, uint64_t from, uint32_t m)
{
	uint64_t run = 0, count = 0;
	for (uint64_t p = 0; p < n; p++) {
		run = valid(g[p]) ? run + 1 : 0;
		count += p >= from && run >= m;
	}
	return count;
}

struct Launch {
	std::vector<uint8_t> bytes;
	uint32_t carried;
};

struct Harness {
	uint32_t k, shortest, carry;
	uint64_t cap;
	Stage st;
	std::vector<Launch> launches;
	std::string why;

	Harness(uint32_t k_, bool second, uint64_t cap_) : k(k_), shortest(second ? k_ - 1 : k_), carry(second ? k_ : k_ - 1), cap(cap_)
	{
		st.buf = (uint8_t *)malloc(cap + 16);
		st.cap = cap;
		st.shortest = shortest;
		st.carry = carry;
	}
	~Harness() { free(st.buf); }
	Harness(const Harness &) = delete;

	int submit(const char *p, uint64_t n, const uint64_t *ends, uint64_t n_ends)
	{
		return st.submit(p, n, ends, n_ends, [this](const uint8_t *g, uint64_t len, uint32_t carried) {
			if (len % 16 || len > cap + 15 || len < st.fill || carried > carry || carried > st.fill || st.fill < shortest)   /* (a) */
				why = "launch shape";
			for (uint64_t i = st.fill; i < len; i++)
				if (g[i] != 'N')
					why = "padding";
			launches.push_back({std::vector<uint8_t>(g, g + len), carried});
			return 0;
		});
	}
};

/* the text of one case and its record ends; the last record stays open */
static void make_text(uint32_t k, bool second, uint64_t cap, std::string &text, std::vector<uint64_t> &ends)
{
	Harness shadow(k, second, cap);                              /* the fill a whole submit will see */
	auto add = [&](const std::string &rec) {
		text += rec;
		ends.push_back(text.size());
		shadow.st.put(rec.data(), rec.size(), [](const uint8_t *, uint64_t, uint32_t) { return 0; });
		shadow.st.put("N", 1, [](const uint8_t *, uint64_t, uint32_t) { return 0; });
	};
	const uint64_t lens[] = {0, 1, k - 2, k - 1, k, k + 1, cap - 1, cap, cap + 1, 3 * cap + 7, 5, 2 * k};
	for (uint64_t len : lens)
		add(bases(len, len > 2 * k));
	for (int which = 0; which < 2; which++) {
		add(bases(k + rnd(20), false));
		while (cap - shadow.st.fill < 3)                            /* room for a record of at least one byte */
			add(bases(3, false));
		const uint64_t room = cap - shadow.st.fill;                /* >= 1: a full buffer is flushed at once */
		const std::string rec = bases(which ? room : room - 1, false);
		text += rec;
		ends.push_back(text.size());
		shadow.st.put(rec.data(), rec.size(), [](const uint8_t *, uint64_t, uint32_t) { return 0; });
		if (which ? shadow.st.fresh : shadow.st.fill != cap - 1)    /* ended at cap: flushed, nothing fresh */
			abort();
		shadow.st.put("N", 1, [](const uint8_t *, uint64_t, uint32_t) { return 0; });
		if (which ? shadow.st.fill != shadow.st.carried + 1 : shadow.st.fresh)
			abort();
		add(bases(2 * k, false));                                   /* what follows the separator: a window that must not bridge it */
	}
	for (int i = 0; i < 6; i++)
		add(bases(1 + rnd(120), true));
	text += bases(k + 3, false);                                    /* open */
}

static int fail(const char *what, uint32_t k, bool second, uint64_t cap, uint64_t chunk, unsigned long long got, unsigned long long want)
{
	printf("FAILED %s: k %u, setting %d, cap %llu, chunk %llu: %llu, expected %llu\n", what, k, second ? 2 : 1, (unsigned long long)cap,
	       (unsigned long long)chunk, got, want);
	return 1;
}

int main()
{
	unsigned long long cases = 0, n_launches = 0;
	const uint32_t ks[] = {11, 19, 31};
	const uint64_t caps[] = {64, 256};
	for (uint32_t k : ks)
		for (int second = 0; second < 2; second++)
			for (uint64_t cap : caps) {
				std::string text;
				std::vector<uint64_t> ends;
				make_text(k, second, cap, text, ends);
				const uint64_t total = text.size();
				/* the direct count: the records with their separators, split at every byte that is no base */
				std::string joined;
				uint64_t at = 0;
				for (uint64_t e : ends) {
					joined += text.substr(at, e - at) + "N";
					at = e;
				}
				joined += text.substr(at);
				const uint64_t chunks[] = {total ? total : 1, 1, k - 1, k, k + 1, cap - 1, cap, cap + 1};
				for (uint64_t chunk : chunks) {
					Harness h(k, second, cap);
					size_t next = 0;
					for (uint64_t a = 0; a < total; a += chunk) {
						const uint64_t b = a + chunk < total ? a + chunk : total;
						std::vector<uint64_t> mine;                  /* a <= end < b, and the end of the text */
						while (next < ends.size() && (ends[next] < b || b == total))
							mine.push_back(ends[next++] - a);
						if (h.submit(text.data() + a, b - a, mine.data(), mine.size()))
							return fail("submit", k, second, cap, chunk, 1, 0);
					}
					if (!h.why.empty()) {
						printf("(a) %s\n", h.why.c_str());
						return fail("(a)", k, second, cap, chunk, 0, 0);
					}
					for (uint32_t m = second ? k - 1 : k; m <= (second ? k + 1 : k); m++) {              /* (b) */
						uint64_t got = 0;
						for (const Launch &l : h.launches)
							got += windows(l.bytes.data(), l.bytes.size(), l.carried, m);
						const uint64_t want = windows((const uint8_t *)joined.data(), joined.size(), 0, m);
						if (got != want || !want)
							return fail("(b)", k, second, cap, chunk, got, want);
					}
					if (h.st.submitted != total)                                                         /* (d) */
						return fail("(d)", k, second, cap, chunk, h.st.submitted, total);
					/* (c): nothing staged, nothing launched, nothing counted */
					const Stage before = h.st;
					const std::vector<uint8_t> held(h.st.buf, h.st.buf + h.st.fill);
					const size_t launched = h.launches.size();
					const uint64_t bad[3][2] = {{5, 3}, {4, 9}, {4, 4}};
					for (const auto &e : bad)
						if (h.submit("ACGTACGT", 8, e, 2) != -1)
							return fail("(c) accepted", k, second, cap, chunk, e[0], e[1]);
					if (h.st.fill != before.fill || h.st.carried != before.carried || h.st.fresh != before.fresh || h.st.submitted != before.submitted ||
					    h.launches.size() != launched || (held.size() && memcmp(held.data(), h.st.buf, held.size())))
						return fail("(c) staged", k, second, cap, chunk, h.st.fill, before.fill);
					cases++;
					n_launches += launched;
				}
			}
	printf("stage check ok: %llu cases, %llu launches\n", cases, n_launches);
	return 0;
}
