/*
 * ntsm_sitegen_stage.h -- the staging state machine of both device libraries of ntsmSiteGen (ntsm_sitegen.hip,
 * ntsm_sitegen_gap.hip): genome text arrives in chunks of any size, goes into one bounded buffer with a separator byte
 * behind every record, and leaves it in launches.  Pure host C++, no HIP: tests/sitegen_stage_check.cpp runs it on a
 * buffer of 64 bytes.  Internal: not part of include/.
 *
 * Seams.  A launch scans the windows that END in its bytes [carried, n); the first `carried` bytes are the tail of what
 * the launch before it saw, there so that a window may begin in them.  After every flush the last `carry` staged bytes
 * move to the front and count as seen.  A launch is skipped while nothing is fresh or while fewer than `shortest` bytes
 * are staged: then everything staged is shorter than any window and at most `carry` long, so all of it is carried and
 * calling it seen loses no window.  The two settings:
 *   ntsm_sitegen.hip      shortest k,     carry k - 1   windows of k bytes.  None lies wholly inside k - 1 bytes, so none
 *                                                       is counted twice and the kernel need not know `carried`.
 *   ntsm_sitegen_gap.hip  shortest k - 1, carry k       windows of k - 1, k and k + 1 bytes; the longest has k bytes before
 *                                                       its last.  Windows of k and k - 1 bytes can lie wholly inside the
 *                                                       carry, so the kernel is given `carried` and counts a window only
 *                                                       if its last byte lies behind it.
 * Either way a window is counted by the one launch in which its last byte is new, and its first byte is there: carry is
 * at least the longest window less one.  No window crosses a record end, because the separator is no base.
 */
#ifndef NTSM_SITEGEN_STAGE_H
#define NTSM_SITEGEN_STAGE_H

#include <cstdint>
#include <cstring>

namespace ntsm_site {

struct Stage {
	uint8_t *buf = nullptr;                  /* cap + 16 bytes, owned by the caller */
	uint64_t cap = 0;                        /* bytes per launch at the most, a multiple of 16 */
	uint32_t shortest = 0, carry = 0;        /* the shortest window, and the bytes that open the next launch */
	uint64_t fill = 0;                       /* staged bytes: the carried tail, then what came since the last launch */
	uint32_t carried = 0;                    /* of them, the bytes an earlier launch has seen: no window that ends there is new */
	bool fresh = false;                      /* bytes staged since the last launch */
	uint64_t submitted = 0;                  /* bytes of every accepted submit */

	/* launch(bytes, n, carried): n a multiple of 16, padded with 'N' behind the staged bytes; 0 or the error to return */
	template <typename Launch> int flush(Launch &&launch)
	{
		if (fresh && fill >= shortest) {
			const uint64_t n = (fill + 15) & ~15ull;
			memset(buf + fill, 'N', n - fill);
			if (const int rc = launch((const uint8_t *)buf, n, carried))
				return rc;
		}
		const uint64_t keep = fill < carry ? fill : carry;
		memmove(buf, buf + fill - keep, keep);
		fill = keep;
		carried = (uint32_t)keep;
		fresh = false;
		return 0;
	}

	template <typename Launch> int put(const char *p, uint64_t len, Launch &&launch)
	{
		while (len) {
			const uint64_t room = cap - fill;
			const uint64_t take = len < room ? len : room;
			memcpy(buf + fill, p, take);
			fill += take;
			fresh = true;
			p += take;
			len -= take;
			if (fill == cap)
				if (const int rc = flush(launch))
					return rc;
		}
		return 0;
	}

	/* a chunk as include/ntsm_sitegen_hip.h describes it.  -1: a bad argument, nothing was staged; else what launch returned */
	template <typename Launch> int submit(const char *bases, uint64_t n, const uint64_t *ends, uint64_t n_ends, Launch &&launch)
	{
		if ((n && !bases) || (n_ends && !ends))
			return -1;
		uint64_t prev = 0;
		for (uint64_t i = 0; i < n_ends; i++) {
			if (ends[i] < prev || ends[i] > n || (i && ends[i] == prev))
				return -1;
			prev = ends[i];
		}
		submitted += n;
		uint64_t at = 0;
		int rc = 0;
		for (uint64_t i = 0; i < n_ends && !rc; i++) {
			rc = put(bases + at, ends[i] - at, launch);
			if (!rc)
				rc = put("N", 1, launch);                   /* the separator: no window crosses a record end */
			at = ends[i];
		}
		if (!rc)
			rc = put(bases + at, n - at, launch);
		return rc ? rc : flush(launch);
	}
};

}  // namespace ntsm_site

#endif
