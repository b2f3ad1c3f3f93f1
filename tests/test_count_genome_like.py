"""The count kernels on genome-like input (tests/genome_like.py): repeats, satellites, 40 % GC, site k-mers that repeat.

Every other parity test of kernels_generic.hip, kernels_mz.hip and kernels_run.hip feeds them i.i.d. uniform bases -- the
friendliest input a minimizer / Bloom design can get.  The paths that only low-complexity input reaches are the branchy ones: ties
of the order hash (a poly-A 12-mer has order hash 0, an array makes every candidate of a window tie), minimizer runs of hundreds
of positions, a filter block that hundreds of site k-mers share (the queues at 64 .. 127 entries, the drain taken at every
position), ntsm_add_hits with all 64 lanes on a few counters, and a -m stop inside a read that a whole wave attributes hits to.

The CPU part (unmarked) pins the generator, shows on the generator's output and the oracle alone that the family is what it claims
to be, and holds the oracle to the thirty-line definition on it.  The GPU part compares every kernel form with the oracle: counts
with np.array_equal, totals and the -m state with ==, no tolerance anywhere; debug_stats() says that the form a case names ran.
A case that differs does not stop its test: the test reports every case that differs, with the keys and hits that are off
(profiles/r20_genome_like/mutation.txt is made of those lines)."""
import hashlib
import os
import subprocess
import types

import numpy as np
import pytest

import genome_like as gl
from oracle_binding import OracleFP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GENOME_SEED, READ_SEED, SITE_SEED, SATELLITE_SEED, DENSE_SEED = 1, 2, 3, 4, 5
N_SITES, N_READS = 600, 10_000
ARRAY_BYTES = 3 * 32_768                      # three tiles of the minimizer-blocked kernel: whole workgroups lie inside one array

# written down when the generator was final (test_generator_is_pinned)
SHA_GENOME = "74925b71372bb4ed0f79f4ef51607ee6baf97ad4e34cc99793e294c7cc97becb"
SHA_SITES_UNFILTERED = "452c05ac124466d02853896bc5b6f6e5500b7b9f00060d492020371f95ae40b5"
SHA_SITES_CLEAN = "3a9ac742bd9e19d2cb765dfde836cda9832df129b8e750fd2765dd7f5239ae82"
SHA_READS_1000 = "c6518c685dc68f133322b87b57803f5787d1229bebfab414b4b52c15c74b3a75"


def _sha(b):
    return hashlib.sha256(b).hexdigest()


def _oracle(path, k, reads, max_hits=0):
    """The oracle's state after `reads` (dupes on, like every site set here); max_hits arms its -m stop at exactly that value."""
    fp = OracleFP(path, k=k, dupes=True)
    n_keys = fp.n_distinct
    fp.close()
    fp = OracleFP(path, k=k, dupes=True, cov=2.0 * (max_hits + 0.5) / n_keys) if max_hits else OracleFP(path, k=k, dupes=True)
    assert not max_hits or fp.max_hits == max_hits
    for r in reads:
        if fp.early_term:
            break
        fp.process(r)
    canon, _, counts = fp.kmers()
    counts.setflags(write=False)
    out = types.SimpleNamespace(canon=canon, counts=counts, totals=(fp.total_kmers, fp.total_hits, fp.total_bases), total_kmers=fp.total_kmers,
                                total_hits=fp.total_hits, early=fp.early_term, reads_processed=fp.reads_processed, stdout=fp.print_counts()[1])
    fp.close()
    return out


class Family:
    """The module's inputs, made once: genome(1), its reads, site files per (k, clean) and oracle results per (file, k, reads, -m)."""

    def __init__(self, tmp):
        self.tmp = tmp
        self.genome, self.ann = gl.genome(GENOME_SEED)
        self.reads = gl.short_reads(self.genome, READ_SEED, N_READS)
        self._files, self._oracle = {}, {}

    def write(self, name, records):
        if name not in self._files:
            path = str(self.tmp / (name + ".fa"))
            gl.write_site_fasta(path, records)
            self._files[name] = (path, records)
        return self._files[name]

    def sites(self, k, clean):
        name = "sites_k%d_%s" % (k, "clean" if clean else "unfiltered")
        if name not in self._files:
            self.write(name, gl.site_records(gl.sites(self.genome, SITE_SEED, k, N_SITES, clean)))
        return self._files[name]

    def satellite(self, k):
        name = "satellite_k%d" % k
        if name not in self._files:
            records, reads, neighbours = gl.satellite_stream(k, SATELLITE_SEED, ARRAY_BYTES)
            self.write(name, records)
            self._files[name] += (reads, neighbours)
        return self._files[name]

    def dense(self, k):
        """8,000 bases around the first gap behind 10 kb: N inside, repeats on both sides"""
        name = "dense_k%d" % k
        if name not in self._files:
            start = next(s for s, _, kind in self.ann if kind == "gap" and s > 10_000) - 3_000
            records, stretch = gl.dense(self.genome, k, start, 8_000)
            self.write(name, records)
            self._files[name] += (gl.short_reads(stretch, DENSE_SEED, 3_000, p_sub=0.0),)
        return self._files[name]

    def oracle(self, path, k, reads, tag, max_hits=0):
        """tag names the read list (the cache key beside path and -m value)"""
        key = (path, k, tag, max_hits)
        if key not in self._oracle:
            self._oracle[key] = _oracle(path, k, reads, max_hits)
        return self._oracle[key]


@pytest.fixture(scope="module")
def fam(tmp_path_factory):
    return Family(tmp_path_factory.mktemp("genome_like"))


# ---- CPU part: the generator, the family's properties, oracle = definition ---------------------------------------------------

def test_generator_is_pinned(fam):
    """Same seed, same bytes: the genome, both k = 19 site files and the first 1,000 reads."""
    assert len(fam.genome) == 60_000 and fam.ann[0][0] == 0 and fam.ann[-1][1] == 60_000
    assert all(a[1] == b[0] for a, b in zip(fam.ann, fam.ann[1:])) and {kind for _, _, kind in fam.ann} == set(gl.KINDS)
    assert _sha(fam.genome) == SHA_GENOME
    assert _sha(open(fam.sites(19, False)[0], "rb").read()) == SHA_SITES_UNFILTERED
    assert _sha(open(fam.sites(19, True)[0], "rb").read()) == SHA_SITES_CLEAN
    assert _sha(b"\n".join(fam.reads[:1000])) == SHA_READS_1000
    assert gl.genome(GENOME_SEED)[0] == fam.genome and gl.genome(GENOME_SEED + 1)[0] != fam.genome


def test_family_is_what_it_claims(fam):
    """On the generator's output and the oracle alone (measured values in parentheses): GC 0.37 .. 0.44 (0.402); >= 30 % of the
    bases outside `unique` (32.8 %); unfiltered sites at k = 19: >= 15 % of the valid windows hit (23.6 %), largest counter >= 1,000
    (13,276) where the clean set's is <= 200 (37), >= 50 site k-mers that hold A^12 or T^12 (395); the first two at k = 13 (22.3 %,
    20,115) and k = 31 (27.0 %, 6,274) as well."""
    g = fam.genome
    gc = sum(g.count(c) for c in b"CG") / sum(g.count(c) for c in b"ACGT")
    assert 0.37 <= gc <= 0.44, gc
    outside = 1.0 - sum(e - s for s, e, kind in fam.ann if kind == "unique") / len(g)
    assert outside >= 0.30, outside
    for k in (19, 13, 31):
        path, records = fam.sites(k, False)
        assert all(len(r) == 2 * k - 1 and b"N" not in r for r in records) and len(records) == 2 * N_SITES
        assert all(sum(a != b for a, b in zip(ref, alt)) == 1 and ref[k - 1] != alt[k - 1] for ref, alt in zip(records[::2], records[1::2]))
        o = fam.oracle(path, k, fam.reads, "all")
        assert o.total_hits >= 0.15 * o.total_kmers, (k, o.totals)
        assert int(o.counts.max()) >= 1_000, (k, int(o.counts.max()))
    path, records = fam.sites(19, True)
    assert int(fam.oracle(path, 19, fam.reads, "all").counts.max()) <= 200
    # the uniqueness rule, restated by brute force on the bytes
    both = fam.genome + b"N" + gl.revcomp(fam.genome)
    for ref, alt in list(zip(records[::2], records[1::2]))[:50]:
        assert all(both.count(ref[i:i + 19]) == 1 for i in range(19)) and not any(alt[i:i + 19] in both for i in range(19))
    kmers = {r[i:i + 19] for r in fam.sites(19, False)[1] for i in range(19)}
    assert sum(1 for x in kmers if b"A" * 12 in x or b"T" * 12 in x) >= 50


def test_satellite_stream_is_what_it_claims(fam):
    """k = 19, arrays of 98,304 bytes, both strands: every valid window hits (1,572,576 of 1,572,576), every neighbour key counts 0
    (48 zero keys of 254), the largest counter is >= 100,000 (196,572: the poly-A array, both strands on one key)."""
    path, records, reads, neighbours = fam.satellite(19)
    assert len(reads) == 16 and all(len(r) == ARRAY_BYTES for r in reads) and len(neighbours) == 8 * gl.N_NEIGHBOURS
    o = fam.oracle(path, 19, reads, "satellite")
    assert o.total_hits == o.total_kmers == 16 * (ARRAY_BYTES - 18)
    near = np.isin(o.canon, [int(gl.canonical_kmers(x, 19)[0][0]) for x in neighbours])
    assert near.sum() == len(neighbours) and not o.counts[near].any() and o.counts[~near].all()
    assert int(o.counts.max()) >= 100_000


@pytest.mark.parametrize("clean", (False, True), ids=("unfiltered", "clean"))
@pytest.mark.parametrize("k", (13, 19, 31))
def test_oracle_is_the_definition_on_the_family(fam, k, clean):
    """OracleFP against dict_model on 2,000 reads: per-key counts through the canonical keys, the totals, and with a threshold at
    40 % of the hits the read the -m stop falls on (k = 19: 60,869 and 38,580 hits of 252,995 windows)."""
    path, records = fam.sites(k, clean)
    reads = fam.reads[:2000]
    o = fam.oracle(path, k, reads, "2000")
    m = gl.dict_model(records, reads, k)
    assert m["n_keys"] == len(o.canon) == len(set(o.canon.tolist()))
    assert (m["total_kmers"], m["total_hits"], m["total_bases"]) == o.totals and o.total_hits > 20_000
    assert all(m["counts"][c] == v for c, v in zip(o.canon.tolist(), o.counts.tolist())) and sum(m["counts"].values()) == o.total_hits
    thr = o.total_hits * 2 // 5
    om = fam.oracle(path, k, reads, "2000", max_hits=thr)
    mm = gl.dict_model(records, reads, k, max_hits=thr)
    assert om.early and 0 < om.reads_processed < 2000 and mm["reads_processed"] == om.reads_processed
    assert (mm["total_kmers"], mm["total_hits"], mm["total_bases"]) == om.totals and thr < om.total_hits
    assert all(mm["counts"][c] == v for c, v in zip(om.canon.tolist(), om.counts.tolist()))


# ---- GPU part ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nt(built):
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    import ntsm_amd
    return ntsm_amd


def _context(nt, keys, k, variant, grid=0, max_hits=0):
    ctx = nt.Context(keys, k=k, max_hits=max_hits)
    if variant:
        ctx.set_kernel(variant)
    if grid:
        ctx.set_tuning(0, grid)
    return ctx


def _ran_its_form(ctx, variant):
    """the launch counters and the form of the tables say that the context ran the kernel its variant names (0: a set this small
    takes the one-level minimizer-blocked kernel)"""
    st = ctx.debug_stats()
    assert (st["launches_generic"] > 0, st["launches_k19"] > 0, st["launches_tab"]) == (variant == 1, variant != 1, 0), (variant, st)
    assert (st["two_level"], st["run_form"]) == (variant == 4, variant == 5), (variant, st)


def _differs(ctx, want, label, times=1, armed=False):
    """[] when the context holds `times` times the oracle's state, else one line that says how far off it is"""
    t, got = ctx.sync(), ctx.counts()
    exp = want.counts * np.uint64(times)
    state = (t.total_kmers, t.total_hits, t.total_bases) + ((t.early_stop, t.reads_consumed) if armed else ())
    exp_state = tuple(times * x for x in want.totals) + ((int(want.early), want.reads_processed) if armed else ())
    if np.array_equal(got, exp) and state == exp_state:
        return []
    return ["%s: %d of %d keys differ (%d lower, %d higher), counts sum to %d of %d, state %s, oracle %s"
            % (label, int((got != exp).sum()), len(exp), int((got < exp).sum()), int((got > exp).sum()), int(got.sum()), int(exp.sum()), state, exp_state)]


def _cut(ends, n_reads):
    """byte offset behind read n_reads - 1 and its terminator"""
    return int(ends[n_reads - 1]) + 1


@pytest.mark.gpu
def test_family_k19_every_form(nt, fam):
    """10,000 reads of the 60 kb genome (1.5 MB: 46 tiles of the minimizer-blocked kernel, 73 of the run-anchored one) against 600
    unfiltered sites -- in elements, arrays and duplications; 24 % of the windows hit, one counter takes 13,276 -- and against 600
    clean ones, through the generic kernel (1), the minimizer-blocked one with one (2) and two levels (4) and the run-anchored one
    (5); default grid, three workgroups, and one workgroup that carries its queues through every tile; as one batch, then split at
    a read boundary at one third on the same context."""
    bases, ends = nt.capi.flatten_reads(fam.reads)
    assert len(bases) > 46 * 32_768 and len(bases) > 73 * 20_480
    bad = []
    for clean in (False, True):
        path, _ = fam.sites(19, clean)
        keys = nt.Sites(path, k=19, allow_dupes=True).keys
        want = fam.oracle(path, 19, fam.reads, "all")
        for variant in (1, 2, 4, 5):
            for grid in (0, 1, 3):
                label = "%s sites, variant %d, grid %d" % ("clean" if clean else "unfiltered", variant, grid)
                ctx = _context(nt, keys, 19, variant, grid)
                ctx.submit(bases, ends)
                bad += _differs(ctx, want, label + ", one batch")
                cut = N_READS // 3
                ctx.submit(bases[:_cut(ends, cut)], ends[:cut])
                ctx.submit(bases[_cut(ends, cut):], ends[cut:] - np.uint64(_cut(ends, cut)))
                bad += _differs(ctx, want, label + ", again in two batches", times=2)
                _ran_its_form(ctx, variant)
                ctx.close()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(13, 32))
def test_family_every_k(nt, fam, k):
    """Every k of ntsm_fast_plan (each KMODE, with and without the candidate offset, 64-bit rolling words) on 4,000 reads against 600
    unfiltered sites with windows of 2k - 1: automatic form (0), generic kernel (1) and, from k = 15, the two-level form (4).
    k = 16, 24, 31 also armed at 40 % of the oracle's hits: the per-read instantiations of the two-level and the automatic form."""
    path, _ = fam.sites(k, False)
    keys = nt.Sites(path, k=k, allow_dupes=True).keys
    reads = fam.reads[:4000]
    bases, ends = nt.capi.flatten_reads(reads)
    want = fam.oracle(path, k, reads, "4000")
    assert want.total_hits > 50_000 and int(want.counts.max()) > 1_000
    bad = []
    for variant in (0, 1) + ((4,) if k >= 15 else ()):
        ctx = _context(nt, keys, k, variant)
        ctx.submit(bases, ends)
        bad += _differs(ctx, want, "k %d, variant %d" % (k, variant))
        _ran_its_form(ctx, variant)
        ctx.close()
    if k in (16, 24, 31):
        thr = want.total_hits * 2 // 5
        stop = fam.oracle(path, k, reads, "4000", max_hits=thr)
        assert stop.early and 0 < stop.reads_processed < 4000
        for variant in (4, 0):
            ctx = _context(nt, keys, k, variant, max_hits=thr)
            ctx.submit(bases, ends)
            bad += _differs(ctx, stop, "k %d, variant %d, -m %d" % (k, variant, thr), armed=True)
            _ran_its_form(ctx, variant)
            ctx.close()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (19, 16, 25))
def test_satellite_arrays_fill_every_lane(nt, fam, k):
    """Pure arrays of period 1, 2, 3, 4, 6, 7, 12 and 171, 98,304 bytes each, both strands: whole workgroups lie inside one array,
    every lane of every wave hits at every position, on `period` counters -- ntsm_add_hits with 64 active lanes in 1 .. 7 groups
    and more, the queues full at every position, every candidate of a window tied (period 1) or the minimum repeated inside the
    k-mer (periods up to 7).  Every valid window is a hit; the site keys one base away from the hottest k-mers stay exactly 0.
    Submitted three times on one context: three times the counts."""
    path, _, reads, neighbours = fam.satellite(k)
    keys = nt.Sites(path, k=k, allow_dupes=True).keys
    bases, ends = nt.capi.flatten_reads(reads)
    want = fam.oracle(path, k, reads, "satellite")
    assert want.total_hits == want.total_kmers == 16 * (ARRAY_BYTES - k + 1)
    near = np.isin(want.canon, [int(gl.canonical_kmers(x, k)[0][0]) for x in neighbours])
    assert near.sum() == len(neighbours) and np.array_equal(want.canon, keys)
    bad = []
    for variant in (1, 2, 4, 5) if k == 19 else (0, 1, 4):
        ctx = _context(nt, keys, k, variant)
        for _ in range(3):
            ctx.submit(bases, ends)
        bad += _differs(ctx, want, "k %d, variant %d, arrays three times" % (k, variant), times=3)
        t, got = ctx.sync(), ctx.counts()
        if t.total_hits != t.total_kmers or got[near].any():
            bad.append("k %d, variant %d: %d hits of %d windows, neighbour keys sum to %d" % (k, variant, t.total_hits, t.total_kmers, int(got[near].sum())))
        _ran_its_form(ctx, variant)
        ctx.close()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("k", (19, 14, 27))
def test_dense_stretch_saturates_the_queues(nt, fam, k):
    """Site records that tile 8,000 bases of the genome (a gap of N inside, repeats around it) and 3,000 error-free reads of that
    stretch alone: every valid window is a hit, so every position of every lane queues a look-up and the drain runs all the time.
    k = 19 through variants 1, 2, 4, 5, k = 14 and 27 through the automatic form; default grid and a single workgroup."""
    path, _, reads = fam.dense(k)
    keys = nt.Sites(path, k=k, allow_dupes=True).keys
    bases, ends = nt.capi.flatten_reads(reads)
    want = fam.oracle(path, k, reads, "dense")
    assert want.total_hits == want.total_kmers > 300_000 and any(b"N" in r for r in reads)
    bad = []
    for variant in (1, 2, 4, 5) if k == 19 else (0,):
        for grid in (0, 1):
            ctx = _context(nt, keys, k, variant, grid)
            ctx.submit(bases, ends)
            bad += _differs(ctx, want, "k %d, variant %d, grid %d, dense stretch" % (k, variant, grid))
            _ran_its_form(ctx, variant)
            ctx.close()
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_armed_stop_inside_repeats(nt, fam):
    """-m on 2,000 family reads, the 16 array reads, 2,000 more family reads, against the unfiltered sites and the arrays' records
    in one set.  Two thresholds, placed from the oracle: the stop read is a family read, and the stop read is one of the arrays
    -- 98,286 hits that whole waves attribute to one read, all of which count.  Variants 1, 2, 4, 5 (an armed context of the run
    form attributes with the minimizer-blocked kernel), small and default armed chunk, one batch and three (the second boundary
    between two arrays)."""
    _, site_records = fam.sites(19, False)
    _, sat_records, sat_reads, _ = fam.satellite(19)
    path, _ = fam.write("sites_and_arrays_k19", site_records + sat_records)
    keys = nt.Sites(path, k=19, allow_dupes=True).keys
    reads = fam.reads[:2000] + sat_reads + fam.reads[2000:4000]
    bases, ends = nt.capi.flatten_reads(reads)
    head = fam.oracle(path, 19, reads[:2000], "armed head")
    full = fam.oracle(path, 19, reads, "armed")
    thresholds = (head.total_hits // 2, head.total_hits + 7 * (ARRAY_BYTES - 18) // 2)        # half of the head; the head and 3.5 arrays
    stops = [fam.oracle(path, 19, reads, "armed", max_hits=thr) for thr in thresholds]
    assert all(s.early for s in stops) and 0 < stops[0].reads_processed <= 2000 < stops[1].reads_processed == 2004
    assert stops[1].total_hits == head.total_hits + 4 * (ARRAY_BYTES - 18) < full.total_hits
    bad = []
    for thr, want in zip(thresholds, stops):
        for variant in (1, 2, 4, 5):
            for chunk in (1 << 12, 0):
                for cuts in ((), (1000, 2008)):
                    ctx = _context(nt, keys, 19, variant, max_hits=thr)
                    ctx.set_armed_chunk(chunk)
                    lo = 0
                    for hi in cuts + (len(reads),):
                        b0 = _cut(ends, lo) if lo else 0
                        ctx.submit(bases[b0:_cut(ends, hi)], ends[lo:hi] - np.uint64(b0))
                        lo = hi
                    bad += _differs(ctx, want, "stop at read %d, variant %d, armed chunk %d, %d batches" % (want.reads_processed, variant, chunk, len(cuts) + 1), armed=True)
                    _ran_its_form(ctx, variant)
                    ctx.close()
    assert not bad, "\n".join(bad)


def _summary(err):
    keep = (b"Total ", b"Distinct ", b"Sites Covered", b"Warning: site coverage", b"Reached desired", b"Warning: ")
    return [l for l in err.split(b"\n") if l.startswith(keep)]


@pytest.mark.gpu
def test_cli_on_the_family(nt, fam):
    """build/ntsmCount -d against oracle/ntsm_oracle -d on the 10,000 reads as FASTQ and the unfiltered k = 19 sites: the bytes of
    counts.txt and the summary lines (collision warnings included), through --debug-kernel 1 / 2 / 4 / 5 and with -m."""
    path, _ = fam.sites(19, False)
    fq = str(fam.tmp / "reads.fq")
    gl.write_fastq(fq, fam.reads)
    want = fam.oracle(path, 19, fam.reads, "all")
    thr = want.total_hits * 2 // 5
    cov = repr(2.0 * (thr + 0.5) / len(want.canon))
    stop = fam.oracle(path, 19, fam.reads, "all", max_hits=thr)
    assert stop.early and 0 < stop.reads_processed < N_READS
    run = lambda exe, extra: subprocess.run([os.path.join(ROOT, exe), "-d", "-s", path] + extra + [fq], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    for m in ([], ["-m", cov]):
        ref = run("oracle/ntsm_oracle", m)
        assert ref.returncode == 0 and ref.stdout == (stop if m else want).stdout and (b"Reached desired (-m) threshold" in ref.stderr) == bool(m)
        for form in (1, 2, 4, 5) if not m else (0,):
            p = run("build/ntsmCount", m + (["--debug-kernel", str(form)] if form else []))
            assert p.returncode == 0, (form, p.stderr[-300:])
            assert p.stdout == ref.stdout, (form, m)
            assert _summary(p.stderr) == _summary(ref.stderr), (form, m)
