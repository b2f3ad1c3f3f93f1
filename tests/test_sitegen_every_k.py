"""ntsmSiteGen's two device libraries (ntsm_amd/csrc/ntsm_sitegen.hip, ntsm_sitegen_gap.hip) at every k from 11 to 31.

Nearly everything the two kernels decide is a function of k: the split A | B | C = k/3, k/3, rest with its pair and rest
masks, kmask and the (k + 1)-base register of the gap kernel (64 bits at k = 31), the clz / ffs arithmetic of prefix_len /
suffix_len, the owner thresholds a and 2a, the end margin e <= (k - 1)/2.  The other device tests reach k = 11, 13, 19, 25
and 31: all odd, and all but 11 with k mod 3 = 1.  Here every k is run, even ones included (only there can a candidate be
its own reverse complement: both of its entries are then one k-mer in one bucket and every place counts twice), with
inputs that put a substitution and a gap at every position:

  A  the whole Hamming ball of a k-mer: each of the three tables must own exactly its positions, for every part split
  B  the whole gap ball: a base put in before and taken out at every position, three end margins
  C  candidates that resemble themselves: palindromes, homopolymers, short periods, and their reverse complements
  D  counts of 254, 255 and 256: the `< 255` test of count() and the clamp, at its edge
  E  buckets of hundreds of entries with one pair, and candidate numbers on both sides of a power of two (and 1 and 2)
  F  all 256 byte values where a base could stand

Expected values are the brute forces of tests/sitegen_restatement.cpp and tests/sitegen_gap_restatement.cpp, never the
device's; every comparison is exact equality of min(count, 255) per candidate.  Each family has an unmarked test that runs
the brute force alone and asserts what the family's inputs are meant to contain, so that a seed that misses shows on a
machine without a GPU, and a gpu test that compares both libraries with the same brute-force values (computed once per
session and shared)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_sitegen import brute as sub_brute, device_hits  # noqa: E402
from test_sitegen import restatement as sub_restatement  # noqa: E402,F401  (a fixture, under the name it has here)
from test_sitegen_gap import brute as gap_brute, gap_hits, random_bases, rc, removed, window_counts  # noqa: E402
from test_sitegen_gap import restatement as gap_restatement  # noqa: E402,F401  (a fixture)

ALL_K = list(range(11, 32))
EDGE_K = [12, 19, 31]                                          # k mod 3 = 0, 1, 1; the first one even, the last the widest


def margin(k):
    """the default end margin where k allows it, else the widest one"""
    return min(5, (k - 1) // 2)


def no_equal_neighbours(rng, k):
    """a random k-mer with q[i] != q[i + 1] for all i, redrawn until it is so: every gap position is a place of its own"""
    while True:
        codes = rng.integers(0, 4, size=k)
        if (codes[1:] != codes[:-1]).all():
            return "".join("ACGT"[c] for c in codes)


def other_base(rng, b):
    return str(rng.choice([c for c in "ACGT" if c != b]))


class Reference:
    """the two restatements, every answer computed once per session and read-only from then on"""

    def __init__(self, sub_exe, gap_exe, work):
        self.sub_exe, self.gap_exe, self.work, self.memo = sub_exe, gap_exe, work, {}

    def _once(self, key, compute):
        if key not in self.memo:
            got = compute("r%d" % len(self.memo))
            for a in (got if isinstance(got, tuple) else (got,)):
                a.setflags(write=False)
            self.memo[key] = got
        return self.memo[key]

    def sub(self, name, records, cands, k, x, method="naive"):
        """min(H, 255) within x substitutions"""
        return self._once(("sub", name, k, x, method), lambda tag: sub_brute(self.sub_exe, self.work, records, cands, k, x, method, tag))

    def gap(self, name, records, cands, k, e, method="naive"):
        """(min(H, 255) within one substitution, min(G, 255) at end margin e)"""
        return self._once(("gap", name, k, e, method), lambda tag: gap_brute(self.gap_exe, self.work, records, cands, k, e, method, tag))


@pytest.fixture(scope="module")
def ref(sub_restatement, gap_restatement, tmp_path_factory):
    return Reference(sub_restatement, gap_restatement, tmp_path_factory.mktemp("every_k"))


def differing(cands, got, want):
    return [(int(c), cands[c], int(got[c]), int(want[c])) for c in np.flatnonzero(np.asarray(got) != np.asarray(want))[:10]]


# ------------------------------------------------------------------------------------------------ A: the Hamming ball
@functools.lru_cache(maxsize=None)
def hamming_ball(k):
    """q, the 3k strings at one substitution from it, 2k at exactly two; q on both strands (the reverse one in lower case)
    between random flanks, then q, the ball and the pairs, each a run of its own: (records, candidates)"""
    rng = np.random.default_rng(500 + k)
    q = random_bases(rng, k)
    ball = [q[:i] + b + q[i + 1:] for i in range(k) for b in "ACGT" if b != q[i]]
    two = []
    for _ in range(2 * k):
        m = list(q)
        for o in rng.choice(k, size=2, replace=False):
            m[o] = other_base(rng, q[o])
        two.append("".join(m))
    records = [random_bases(rng, 40) + q + random_bases(rng, 40) + rc(q).lower() + random_bases(rng, 40), "N".join([q] + ball + two)]
    return records, [q] + ball + two + [rc(q)]


@pytest.mark.parametrize("k", ALL_K)
def test_hamming_ball_premises(ref, k):
    """q is met twice as it stands, once reversed and once by each ball member; a ball member by itself, q (three times)
    and the two other bases at its position; a pair by itself and the two ball members between it and q"""
    records, cands = hamming_ball(k)
    one, none = ref.sub("A", records, cands, k, 1), ref.sub("A", records, cands, k, 0)
    assert one[0] == 3 * k + 3 and one[-1] == one[0]
    assert (one[1:1 + 3 * k] >= 6).all() and (one[1 + 3 * k:-1] >= 3).all()
    assert none[0] == 3 and (none[1:1 + 3 * k] == 1).all()
    sub, _ = ref.gap("A", records, cands, k, margin(k))
    assert np.array_equal(sub, one)


@pytest.mark.gpu
@pytest.mark.parametrize("k", ALL_K)
def test_hamming_ball_on_the_device(built, ref, k):
    """a substitution at every position with every base: x = 0 and x = 1, whole and in chunks of k bytes; the gap library's
    substitution count equal to x = 1 and its gap count to the brute force"""
    records, cands = hamming_ball(k)
    windows = window_counts(records, k)
    for x in (0, 1):
        want = ref.sub("A", records, cands, k, x)
        for chunk in (None, k):
            got, t = device_hits(cands, k, x, records, chunk)
            assert np.array_equal(got, want), (x, chunk, differing(cands, got, want))
            assert t.windows == windows[0] and t.bitmap_tests == t.windows * (3 if x else 1), (x, chunk)
    want_sub, want_gap = ref.gap("A", records, cands, k, margin(k))
    sub, gap, st = gap_hits(cands, k, margin(k), records)
    assert np.array_equal(sub, ref.sub("A", records, cands, k, 1)), differing(cands, sub, want_sub)
    assert np.array_equal(gap, want_gap), differing(cands, gap, want_gap)
    assert (st.windows, st.windows_long, st.windows_short) == windows


# ------------------------------------------------------------------------------------------------ B: the gap ball
def margins(k):
    return sorted({1, 2, (k - 1) // 2})


@functools.lru_cache(maxsize=None)
def gap_ball(k):
    """q with each of the four bases put in before every position 0 .. k, q without each of its bases, 60 random bases;
    candidates q, its reverse complement and q with its middle base changed: (records, candidates)"""
    rng = np.random.default_rng(600 + k)
    q = no_equal_neighbours(rng, k)
    longer = "N".join(q[:p] + b + q[p:] for p in range(k + 1) for b in "ACGT")
    shorter = "N".join(removed(q, p) for p in range(k))
    changed = q[:k // 2] + other_base(rng, q[k // 2]) + q[k // 2 + 1:]
    return [longer, shorter, random_bases(rng, 60)], [q, rc(q), changed]


@pytest.mark.parametrize("k", ALL_K)
def test_gap_ball_premises(ref, k):
    """a wider margin leaves fewer places and the widest still some; both strands alike; H(q) is 18 whatever the margin:
    a base put in before position 0, 1, k - 1 or k leaves a window of k bases within one substitution of q (16 of them),
    and so does q's second base put in behind itself and its last but one put in before itself (2)"""
    records, cands = gap_ball(k)
    e1, e2, e_max = margins(k)
    g = {}
    for e in margins(k):
        sub, gap = ref.gap("B", records, cands, k, e)
        sub2, gap2 = ref.gap("B", records, cands, k, e, "neighbours")
        assert np.array_equal(sub, sub2) and np.array_equal(gap, gap2)
        assert sub[0] == 18 and gap[1] == gap[0] and gap.max() < 255
        g[e] = int(gap[0])
    print("k = %d: G(q) = %s" % (k, g))
    assert g[e1] > g[e2] > g[e_max] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("k,e", [(k, e) for k in ALL_K for e in margins(k)])
def test_gap_ball_on_the_device(built, ref, k, e):
    """a gap at every position, long and short, at the narrowest margins and the widest: G and H equal to the brute force
    whole and in chunks of k + 1 bytes, the three window counts as a split of the records gives them"""
    records, cands = gap_ball(k)
    want_sub, want_gap = ref.gap("B", records, cands, k, e)
    for chunk in (None, k + 1):
        sub, gap, st = gap_hits(cands, k, e, records, chunk)
        assert np.array_equal(gap, want_gap), (chunk, differing(cands, gap, want_gap))
        assert np.array_equal(sub, want_sub), (chunk, differing(cands, sub, want_sub))
        assert (st.windows, st.windows_long, st.windows_short) == window_counts(records, k), chunk


# ------------------------------------------------------------------------------------------------ C: self-similar candidates
def cut(unit, k):
    return (unit * k)[:k]


@functools.lru_cache(maxsize=None)
def self_similar(k):
    """nine candidates and then the reverse complement of each.  The first is its own reverse complement for even k and
    one base from it for odd k; for even k (AT)* is its own as well: (records, candidates)"""
    rng = np.random.default_rng(700 + k)
    half = random_bases(rng, k // 2)
    pal = half + rc(half) if k % 2 == 0 else half + "A" + rc(half)
    family = [pal, "A" * k, "T" * k, cut("AC", k), cut("AT", k), cut("ACG", k), cut("AACC", k), "A" * (k - 1) + "C", "C" + "A" * (k - 1)]
    records = [random_bases(rng, 30) + pal + random_bases(rng, 30) + pal[:k // 2] + "G" + pal[k // 2:] + random_bases(rng, 30),
               "A" * (k + 40) + "C" + "A" * (k - 1) + "G" + "T" * (k + 1),
               "AC" * (k + 20), "AT" * (k + 20), "ACG" * (k + 20), "AACC" * (k + 10), cut("AC", k) + cut("CA", k)]
    return records, family + [rc(m) for m in family]


@pytest.mark.parametrize("k", ALL_K)
def test_self_similar_premises(ref, k):
    records, cands = self_similar(k)
    assert (rc(cands[0]) == cands[0]) == (k % 2 == 0) and (rc(cands[4]) == cands[4]) == (k % 2 == 0)
    none, one = ref.sub("C", records, cands, k, 0), ref.sub("C", records, cands, k, 1)
    sub, gap = ref.gap("C", records, cands, k, margin(k))
    assert np.array_equal(sub, one)
    for counts in (none, one, gap):
        assert np.array_equal(counts[:9], counts[9:]) and counts.max() < 255
    assert none[0] == (2 if k % 2 == 0 else 1)                  # the palindrome's one place counts on both strands
    for homopolymer in (1, 2):
        assert gap[homopolymer] > none[homopolymer] > 1
    print("k = %d: H0 %s H1 %s G %s" % (k, none[:9].tolist(), one[:9].tolist(), gap[:9].tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize("k", ALL_K)
def test_self_similar_on_the_device(built, ref, k):
    """duplicate entries in one bucket (a candidate that is its own reverse complement, a candidate and its reverse
    complement both in the list), runs in which every position of a gap is the same place, periods of 2, 3 and 4"""
    records, cands = self_similar(k)
    for x in (0, 1):
        want = ref.sub("C", records, cands, k, x)
        got, _ = device_hits(cands, k, x, records)
        assert np.array_equal(got, want), (x, differing(cands, got, want))
        assert np.array_equal(got[:9], got[9:])
    want_sub, want_gap = ref.gap("C", records, cands, k, margin(k))
    for chunk in (None, k - 1):
        sub, gap, st = gap_hits(cands, k, margin(k), records, chunk)
        assert np.array_equal(gap, want_gap), (chunk, differing(cands, gap, want_gap))
        assert np.array_equal(sub, want_sub), (chunk, differing(cands, sub, want_sub))
        assert (st.windows, st.windows_long, st.windows_short) == window_counts(records, k), chunk


# ------------------------------------------------------------------------------------------------ D: the clamp at its edge
@functools.lru_cache(maxsize=None)
def clamp_edge(k):
    """six random k-mers: the first three 254, 255 and 256 times as they stand, the last three as often with a base put in
    before position 9, or before the last position the margin allows where that is smaller (k = 12: 7): (records, candidates)"""
    rng = np.random.default_rng(800 + k)
    qs = [random_bases(rng, k) for _ in range(6)]
    at = min(9, k - margin(k))
    records = ["N".join([qs[i]] * n) for i, n in enumerate((254, 255, 256))]
    records += ["N".join(qs[3 + i][:at] + "ACGT"[j % 4] + qs[3 + i][at:] for j in range(n)) for i, n in enumerate((254, 255, 256))]
    return records, qs


CLAMP_H, CLAMP_G = [254, 255, 255, 0, 0, 0], [0, 0, 0, 254, 255, 255]


@pytest.mark.parametrize("k", EDGE_K)
def test_clamp_edge_premises(ref, k):
    records, cands = clamp_edge(k)
    sub, gap = ref.gap("D", records, cands, k, margin(k), "neighbours")
    assert sub.tolist() == CLAMP_H and gap.tolist() == CLAMP_G
    assert ref.sub("D", records, cands, k, 1, "neighbours").tolist() == CLAMP_H


@pytest.mark.gpu
@pytest.mark.parametrize("k", EDGE_K)
def test_clamp_edge_on_the_device(built, ref, k):
    """one below the clamp, at it and one above, for both count words; twice, each time on a session of its own"""
    records, cands = clamp_edge(k)
    want_sub, want_gap = ref.gap("D", records, cands, k, margin(k), "neighbours")
    assert want_sub.tolist() == CLAMP_H and want_gap.tolist() == CLAMP_G
    for _ in range(2):
        got, _ = device_hits(cands, k, 1, records)
        assert got.tolist() == CLAMP_H
        sub, gap, _ = gap_hits(cands, k, margin(k), records)
        assert sub.tolist() == CLAMP_H and gap.tolist() == CLAMP_G


# ------------------------------------------------------------------------------------------------ E: long buckets, table sizes
BUCKET_K = [12, 19]


@functools.lru_cache(maxsize=None)
def long_buckets(k):
    """for each pair AB, AC, BC up to 300 distinct candidates that equal one k-mer on the pair and are random on the third
    part (384 at k = 12, 900 at k = 19): one bucket per table holds a whole group.  Every third candidate is in the genome."""
    rng = np.random.default_rng(900 + k)
    a = k // 3
    base = random_bases(rng, k)
    cands, seen = [], set()
    for lo, hi in ((2 * a, k), (a, 2 * a), (0, a)):             # the part outside AB, AC, BC
        want = len(cands) + min(300, 4 ** (hi - lo) // 2)
        while len(cands) < want:
            c = base[:lo] + random_bases(rng, hi - lo) + base[hi:]
            if c not in seen:
                seen.add(c)
                cands.append(c)
    return ["N".join(cands[::3]), random_bases(rng, 500)], cands


@pytest.mark.parametrize("k", BUCKET_K)
def test_long_buckets_premises(ref, k):
    records, cands = long_buckets(k)
    assert len(cands) == {12: 384, 19: 900}[k] and len(cands) % 3 == 0
    none, one = ref.sub("E", records, cands, k, 0), ref.sub("E", records, cands, k, 1)
    in_genome = np.arange(len(cands)) % 3 == 0
    assert (none[in_genome] == 1).all() and (none[~in_genome] == 0).all()
    assert (one > 1).sum() >= 50 and (one == 0).sum() >= 10
    sub, gap = ref.gap("E", records, cands, k, margin(k))
    assert np.array_equal(sub, one) and gap.max() < 255


@pytest.mark.gpu
@pytest.mark.parametrize("k", BUCKET_K)
def test_long_buckets_on_the_device(built, ref, k):
    """a window of the first record walks a bucket of a hundred entries and more in the table of its group's pair"""
    records, cands = long_buckets(k)
    first = window_counts(records[:1], k)[0]
    for x in (0, 1):
        want = ref.sub("E", records, cands, k, x)
        got, t = device_hits(cands, k, x, records)
        assert np.array_equal(got, want), (x, differing(cands, got, want))
        if x:
            assert t.probes >= 100 * first, (t.probes, first)
    want_sub, want_gap = ref.gap("E", records, cands, k, margin(k))
    sub, gap, st = gap_hits(cands, k, margin(k), records)
    assert np.array_equal(gap, want_gap), differing(cands, gap, want_gap)
    assert np.array_equal(sub, want_sub), differing(cands, sub, want_sub)
    assert st.probes >= 100 * first, (st.probes, first)


TABLE_K = 19
TABLE_SIZES = [1, 2, 511, 512, 513]                            # entries 2 and 4; 1,022 and 1,024 (2^10 buckets); 1,026 (2^11)


@functools.lru_cache(maxsize=None)
def table_sizes():
    """513 windows of a genome of 4,000 random bases, in one fixed order: (records, candidates)"""
    rng = np.random.default_rng(1000 + TABLE_K)
    genome = random_bases(rng, 4000)
    return [genome], [genome[at:at + TABLE_K] for at in rng.integers(0, 4000 - TABLE_K + 1, size=max(TABLE_SIZES))]


def test_table_sizes_premises(ref):
    """a candidate's count does not depend on the others: the brute force of the first n is the first n of the brute force"""
    records, cands = table_sizes()
    want = ref.sub("T", records, cands, TABLE_K, 1)
    assert (want >= 1).all() and want.max() < 255
    for n in TABLE_SIZES[:2]:
        assert np.array_equal(ref.sub("T%d" % n, records, cands[:n], TABLE_K, 1), want[:n])
    sub, gap = ref.gap("T", records, cands, TABLE_K, margin(TABLE_K))
    assert np.array_equal(sub, want)


@pytest.mark.gpu
@pytest.mark.parametrize("library", ["substitutions", "gaps"])
def test_table_sizes_on_the_device(built, ref, library):
    """one candidate, two, and candidate numbers just below, at and just above the step from 2^10 to 2^11 buckets: each equal
    to the brute force, so the first n counts of a larger n are the counts of the smaller n"""
    records, cands = table_sizes()
    want_sub, want_gap = ref.gap("T", records, cands, TABLE_K, margin(TABLE_K))
    assert np.array_equal(want_sub, ref.sub("T", records, cands, TABLE_K, 1))
    earlier = []
    for n in TABLE_SIZES:
        if library == "substitutions":
            got = [device_hits(cands[:n], TABLE_K, 1, records)[0]]
        else:
            got = list(gap_hits(cands[:n], TABLE_K, margin(TABLE_K), records)[:2])
        for have, want in zip(got, (want_sub, want_gap)):
            assert np.array_equal(have, want[:n]), (n, differing(cands, have, want[:n]))
        for m, before in earlier:
            assert all(np.array_equal(have[:m], old) for have, old in zip(got, before)), (m, n)
        earlier.append((n, got))


# ------------------------------------------------------------------------------------------------ F: every byte value
@functools.lru_cache(maxsize=None)
def every_byte(k):
    """one record: for every byte value, q with that byte in place of its middle base and q with that byte put in before
    its middle base, an N after each: (the bytes, the same text with every byte outside ACGTacgt as N, candidates)"""
    rng = np.random.default_rng(1100 + k)
    q = no_equal_neighbours(rng, k)
    raw, p = q.encode(), k // 2
    text = b"".join(raw[:p] + bytes([b]) + raw[p + 1:] + b"N" + raw[:p] + bytes([b]) + raw[p:] + b"N" for b in range(256))
    clean = bytes(c if c in b"ACGTacgt" else ord("N") for c in text).decode()
    return text, clean, [q, rc(q)]


@pytest.mark.parametrize("k", EDGE_K)
def test_every_byte_premises(ref, k):
    """the eight bytes that are bases give eight places each way, the other 248 none"""
    text, clean, cands = every_byte(k)
    assert len(text) == 256 * (2 * k + 3) == len(clean) and sum(a != b for a, b in zip(text, clean.encode())) == 2 * 247
    sub, gap = ref.gap("F", [clean], cands, k, margin(k))
    assert sub.tolist() == [8, 8] and gap.tolist() == [8, 8]
    assert ref.sub("F", [clean], cands, k, 1).tolist() == [8, 8] and ref.sub("F", [clean], cands, k, 0).tolist() == [2, 2]


@pytest.mark.gpu
@pytest.mark.parametrize("k", EDGE_K)
def test_every_byte_on_the_device(built, ref, k):
    """byte & 0xdf compared with A, C, G, T: the bytes one bit from a base (@, `, E, 0xC1, 0xE1, 0x01 ...) and all the rest
    must end a run exactly as an N does"""
    import ntsm_amd.sitegen as S
    text, clean, cands = every_byte(k)
    want_sub, want_gap = ref.gap("F", [clean], cands, k, margin(k))
    for x in (0, 1):
        with S.Session(cands, k, x) as s:
            s.submit(text, [len(text)])
            got, t = s.hits().astype(np.int64), s.times()
        assert np.array_equal(got, ref.sub("F", [clean], cands, k, x)), (x, got)
        assert t.windows == window_counts([clean], k)[0]
    with S.GapSession(cands, k, margin(k)) as s:
        s.submit(text, [len(text)])
        sub, gap = s.hits()
        st = s.stats()
    assert np.array_equal(sub, want_sub) and np.array_equal(gap, want_gap), (sub, gap)
    assert (st.windows, st.windows_long, st.windows_short) == window_counts([clean], k)
