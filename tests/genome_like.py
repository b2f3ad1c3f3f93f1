"""A seeded, genome-like input family for the count kernels (test infrastructure only; pure numpy / Python, no conftest).

Every other parity test feeds the kernels i.i.d. uniform bases.  This module models what real reads add to that: about a third of
the bases in repeats (dispersed elements with poly-A tails, microsatellites, homopolymers, segmental duplications), 40 % GC, gaps
of N, site k-mers that repeat across sites and across the genome -- and, as the extreme, pure satellite arrays in which every
window of a read is a site k-mer.  `dict_model` is the definition of the count the kernels and the oracle are held to.
Seeds go through np.random.default_rng(seed) only."""
import collections

import numpy as np

KINDS = ("unique", "element", "micro", "homo", "segdup", "gap")
WEIGHTS = (0.40, 0.30, 0.15, 0.08, 0.04, 0.03)
BASE_P = (0.295, 0.205, 0.205, 0.295)                      # A C G T: 41 % GC
SATELLITE_UNITS = {1: b"A", 2: b"AC", 3: b"AAT", 4: b"AAAG", 6: b"AACCCT", 7: b"AAACCCT"}     # 12 and 171 are seeded random
N_NEIGHBOURS = 6

_ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
_CODE = np.full(256, 4, dtype=np.uint8)
_CODE[_ACGT] = np.arange(4, dtype=np.uint8)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def revcomp(seq):
    return seq.translate(_COMP)[::-1]


def _iid(rng, n):
    return _ACGT[rng.choice(4, size=n, p=BASE_P)].tobytes()


def _substitute(rng, seq, p, alphabet):
    """Every base replaced with probability p by a letter drawn from `alphabet` (which may draw the base itself)."""
    a = np.frombuffer(seq, dtype=np.uint8).copy()
    at = np.flatnonzero(rng.random(len(a)) < p)
    a[at] = np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=len(at))]
    return a.tobytes()


def genome(seed, length=60_000):
    """(bytes, [(start, end, kind)]): segments drawn with WEIGHTS until `length` bases stand.  A unique stretch is log-uniform in
    200 .. 1,500 bases (short stretches are the common ones, which keeps a third of the bases in repeats)."""
    rng = np.random.default_rng(seed)
    consensus = [_iid(rng, 280) for _ in range(3)]
    g, ann = bytearray(), []
    while len(g) < length:
        kind = KINDS[rng.choice(len(KINDS), p=WEIGHTS)]
        if kind == "unique":
            seg = _iid(rng, int(round(np.exp(rng.uniform(np.log(200), np.log(1500))))))
        elif kind == "element":
            seg = consensus[rng.integers(3)] + b"A" * int(rng.integers(15, 41))
            seg = _substitute(rng, seg, rng.uniform(0.02, 0.15), b"ACGT")
            if rng.random() < 0.5:
                seg = revcomp(seg)
        elif kind == "micro":
            unit = _iid(rng, int(rng.integers(1, 7)))
            n = int(rng.integers(20, 201))
            seg = (unit * n)[:n]
        elif kind == "homo":
            seg = _iid(rng, 1) * int(rng.integers(12, 61))
        elif kind == "segdup":
            if len(g) < 3000:
                continue
            at = int(rng.integers(0, len(g) - 1000 + 1))
            seg = bytes(g[at:at + 1000])
            if rng.random() < 0.5:
                seg = revcomp(seg)
        else:
            seg = b"N" * int(rng.integers(1, 31))
        seg = seg[:length - len(g)]
        ann.append((len(g), len(g) + len(seg), kind))
        g += seg
    return bytes(g), ann


def canonical_kmers(seq, k):
    """(canonical 2-bit codes uint64[n], index of the window's last base int64[n]) of every window of k bases of ACGT in `seq`:
    A C G T = 0 1 2 3, first base in the highest bits, the smaller of the window and its reverse complement (13 <= k <= 31)."""
    c = _CODE[np.frombuffer(seq, dtype=np.uint8)]
    n = len(c) - k + 1
    if n <= 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.int64)
    bad = np.concatenate(([0], np.cumsum(c > 3)))
    ok = bad[k:] == bad[:-k]
    c = (c & 3).astype(np.uint64)
    fw, rv = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    for j in range(k):
        fw = (fw << np.uint64(2)) | c[j:j + n]
        rv |= (np.uint64(3) - c[j:j + n]) << np.uint64(2 * j)
    return np.minimum(fw, rv)[ok], np.flatnonzero(ok) + (k - 1)


def sites(genome, seed, k, n_sites, clean):
    """n_sites (REF, ALT) pairs: REF is the 2k - 1 bases around a drawn position (no N), ALT has another base at the centre.
    clean: the reference pipeline's uniqueness rule -- every k-mer of REF occurs exactly once in the genome (either strand), none
    of ALT occurs at all.  Not clean: no filter, so sites sit in elements, arrays and duplications as often as the genome does."""
    rng = np.random.default_rng(seed)
    canon, last = canonical_kmers(genome, k)
    uniq, cnt = np.unique(canon, return_counts=True)
    times = np.zeros(len(genome), dtype=np.int64)                     # times[i]: occurrences of the k-mer that ENDS at i, 0 = not valid
    times[last] = cnt[np.searchsorted(uniq, canon)]
    out = []
    for centre in rng.permutation(np.arange(k - 1, len(genome) - k + 1)):
        if len(out) == n_sites:
            break
        ref = genome[centre - k + 1:centre + k]
        if b"N" in ref:
            continue
        alt_base = b"ACGT".replace(ref[k - 1:k], b"")[rng.integers(3)]
        alt = ref[:k - 1] + bytes([alt_base]) + ref[k:]
        if clean and (np.any(times[centre:centre + k] != 1) or np.any(np.isin(canonical_kmers(alt, k)[0], uniq))):
            continue
        out.append((ref, alt))
    assert len(out) == n_sites, "the genome has too few admissible positions"
    return out


def site_records(pairs):
    return [w for pair in pairs for w in pair]


def write_site_fasta(path, records):
    """Two records per name, REF then ALT: what nt.Sites and OracleFP read."""
    with open(path, "wb") as f:
        for i, r in enumerate(records):
            f.write(b">s%d\n%s\n" % (i // 2, r))


def write_fastq(path, reads):
    with open(path, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, r, b"I" * len(r)))


def short_reads(genome, seed, n, length=150, p_sub=0.01):
    """n substrings of the genome, either strand, each base replaced with probability p_sub by a letter drawn from ACGTN."""
    rng = np.random.default_rng(seed)
    length = min(length, len(genome))
    starts = rng.integers(0, len(genome) - length + 1, size=n)
    flip = rng.random(n) < 0.5
    out = []
    for s, f in zip(starts.tolist(), flip.tolist()):
        r = genome[s:s + length]
        r = revcomp(r) if f else r
        out.append(_substitute(rng, r, p_sub, b"ACGTN") if p_sub > 0 else r)
    return out


def satellite_stream(k, seed, array_bytes):
    """(site records, reads, neighbour k-mers).  Per unit (period 1, 2, 3, 4, 6, 7, 12 and 171, the alpha-satellite length): two
    reads, the pure array cut at array_bytes and its reverse complement; one site record that holds every k-mer of the array; and
    N_NEIGHBOURS records of one k-mer each -- a k-mer of the array with one base changed that does not itself occur in the array
    on either strand: the hot non-site k-mers' mirror image, site keys one base away from the hottest k-mers of the stream."""
    rng = np.random.default_rng(seed)
    units = dict(SATELLITE_UNITS)
    for period in (12, 171):
        while True:
            u = _iid(rng, period)
            if all(u != (u[:d] * period)[:period] for d in range(1, period) if period % d == 0):      # no shorter period
                break
        units[period] = u
    records, reads, neighbours = [], [], []
    for period in sorted(units):
        u = units[period]
        array = (u * (array_bytes // period + 1))[:array_bytes]
        reads += [array, revcomp(array)]
        records.append((u * (2 * k + 2))[:period + 2 * k])
        own = set(canonical_kmers(records[-1], k)[0].tolist())
        mine = []
        while len(mine) < N_NEIGHBOURS:
            at, pos = int(rng.integers(0, period)), int(rng.integers(0, k))
            kmer = bytearray(records[-1][at:at + k])
            kmer[pos] = b"ACGT".replace(bytes(kmer[pos:pos + 1]), b"")[rng.integers(3)]
            kmer = bytes(kmer)
            if int(canonical_kmers(kmer, k)[0][0]) not in own and kmer not in mine and revcomp(kmer) not in mine:
                mine.append(kmer)
        records += mine
        neighbours += mine
    return records, reads, neighbours


def dense(genome, k, start, span):
    """(site records, stretch): records of 2k - 1 bases that tile genome[start:start + span] with overlap k - 1, so every valid
    window of the stretch is a site k-mer.  Reads for it are drawn from the stretch only."""
    stretch = genome[start:start + span]
    records = [stretch[i:i + 2 * k - 1] for i in range(0, len(stretch) - k + 1, k)]
    return records, stretch


def dict_model(records, reads, k, max_hits=0):
    """The definition.  counts: a Counter over the canonical k-mers of the reads, restricted to the k-mers of the site records;
    total_kmers: windows of k bases of ACGT; total_hits: those in the site set; max_hits (-m, 0 = off): reads after the first
    one that lifts the hits strictly above it contribute nothing (reads_processed counts up to and including that read)."""
    site = np.unique(np.concatenate([canonical_kmers(r, k)[0] for r in records]))
    ends = np.cumsum([len(r) + 1 for r in reads]) - 1              # one N after every read: no window spans two reads
    canon, last = canonical_kmers(b"".join(r + b"N" for r in reads), k)
    read_of = np.searchsorted(ends, last)
    hit = np.isin(canon, site)
    n_reads = len(reads)
    if max_hits:
        over = np.flatnonzero(np.cumsum(np.bincount(read_of[hit], minlength=len(reads))) > max_hits)
        if len(over):
            n_reads = int(over[0]) + 1
    keep = read_of < n_reads
    counts = collections.Counter(canon[hit & keep].tolist())
    return dict(counts=counts, total_kmers=int(keep.sum()), total_hits=int((hit & keep).sum()),
                total_bases=sum(len(r) for r in reads[:n_reads]), reads_processed=n_reads, n_keys=len(site))
