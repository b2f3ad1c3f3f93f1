"""ntsmEval --between STORE_A STORE_B: every sample of one cohort store against every sample of
another, B's loci matched to A's by ID, without reading a counts file.  Device side: ntsm_eval_between_open / _rows / _close /
_tune (ntsm_amd/csrc/ntsm_eval_between.hip); host side: ntsm_amd/csrc/host/eval_between.hpp.

CPU: the surface, every refusal, the calls that need no device, and eval_between.hpp on its cases under the host sanitizers
(`make between_check`).
GPU: every band of the rectangle as raw bytes against ntsm_eval_pairs on the dense concatenation [A; B remapped to A's sites],
both tallies against ntsm_eval_cross, one shape against the numpy model, the pairs i < j of Between(S, S) against Within(S),
and the CLI's stdout byte for byte against the oracle's rows over [A's files, B's files] that pair a file of A with one of B.
No comparison has a tolerance."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle_binding import ROOT
from test_eval import EVAL, ORACLE_CLI, files_for, mismatches, random_samples, vec_pairs, write_counts
from test_eval_near import HEAD, gpu, sig  # noqa: F401
from test_eval_store import FLAGS, read_store, run, seven_files, snapshot, unchanged

SYMBOLS = ("ntsm_eval_between_open", "ntsm_eval_between_rows", "ntsm_eval_between_close", "ntsm_eval_between_tune")
LACKS = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------- CPU
def test_surface():
    """The four entry points are exported and declared; the help text names the run and its band flag, and says where STORE_B
    goes."""
    import ntsm_amd.eval as ev
    lib = ev.lib
    assert lib._name == os.path.join(ROOT, "ntsm_amd", "libntsm_eval_hip.so")
    hdr = open(os.path.join(ROOT, "include", "ntsm_eval_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert " %s(" % name in hdr, name
    assert "typedef struct ntsm_eval_between_session ntsm_eval_between_session;" in hdr
    p = subprocess.run([EVAL, "--help"], capture_output=True)
    assert p.returncode == 0 and p.stdout == b""
    ours = p.stderr.split(b"This build only")[1]
    assert b"--between = STORE_A STORE_B" in ours and b"--between-rows = INT" in ours and b"positional" in ours
    assert b"--within = STORE" in ours and b"--pack" in ours and b"against a store" in ours    # and what was there is


def test_refusals(tmp_path):
    """Every refusal of --between and --between-rows: its sentence, exit 1, one 'Error:' line, nothing on stdout, no GPU work
    (this test runs without one), both stores -- bytes and mtime -- as they were.  S and T are good stores over the same 40
    loci; `alien` lists a locus S lacks, `dup` lists one twice (a counts file with a repeated line fixed its table), `empty`
    holds no sample, `trunc` is a byte short."""
    names = seven_files(tmp_path)[0]
    at = lambda x: str(tmp_path / x)  # noqa: E731
    assert run(["--pack", "S"] + names[:4], tmp_path).returncode == 0
    assert run(["--pack", "T"] + names[4:6], tmp_path).returncode == 0
    line = "rs%d\t3\t4\t3\t4\t1\t1\n"
    with open(at("alien.txt"), "w") as f:
        f.write("#@TK\t5\n#@KS\t19\n" + "".join(line % s for s in range(40)) + "rsUnknown\t3\t4\t3\t4\t1\t1\n")
    with open(at("dup.txt"), "w") as f:
        f.write("#@TK\t5\n#@KS\t19\n" + "".join(line % s for s in range(40)) + line % 17)
    assert run(["--pack", "alien", "alien.txt"], tmp_path).returncode == 0
    assert run(["--pack", "dup", "dup.txt"], tmp_path).returncode == 0
    assert read_store(at("alien"))["loci"][-1] == "rsUnknown" and read_store(at("dup"))["loci"].count("rs17") == 2
    store = open(at("S"), "rb").read()
    with open(at("empty"), "wb") as f:
        f.write(store[:16] + struct.pack("<Q", 0) + store[24:read_store(at("S"))["first"]])
    with open(at("trunc"), "wb") as f:
        f.write(store[:-1])
    P = ["-p", "rot.tsv", "-n", "norm.txt", "-d", "2"]
    q = names[6]
    seven, pca, build = b"are seven runs: give one of them", b"a PCA-guided search between two stores is not part of this build", b"is not part of this build"
    cases = [
        (["--between", "S", "T", q], b"takes STORE_B and no input files"),               # FILES given
        (["--between", "S", "T", q, names[5]], b"takes STORE_B and no input files"),
        (["--between", "S"], b"needs the second store"),                                # STORE_B missing
        (["--between", "S", "--pack", "S", "T"], seven),                                # more than one of the seven runs
        (["--between", "S", "--against", "S", "T"], seven),
        (["--between", "S", "--index", "S", "T"] + P, seven),
        (["--between", "S", "--near", "S", "T"], seven),
        (["--between", "S", "--within", "S", "T"], seven),
        (["--between", "S", "--within-near", "S", "T"], seven),
        (["--within", "S", "--within-near", "S"], seven),                               # the sentence is the same from the other side
        (["--between", "S", "T", "-p", "rot.tsv"], pca),
        (["--between", "S", "T", "-n", "norm.txt"], pca),
        (["--between", "S", "T"] + P, pca),
        (["--between", "S", "T", "-b", "truth.tsv"], b"-b with --between " + build),
        (["--between", "S", "T", "-e", "merged.txt"], b"merging (-e, -o) with --between " + build),
        (["--between", "S", "T", "-o"], b"merging (-e, -o) with --between " + build),
        (["--between", "trunc", "T"], b"trunc"),                                        # either store invalid ...
        (["--between", "S", "trunc"], b"trunc"),
        (["--between", "nowhere", "T"], b"cannot open store nowhere"),
        (["--between", "S", "nowhere"], b"cannot open store nowhere"),
        (["--between", "empty", "T"], b"empty holds no samples"),                       # ... or empty
        (["--between", "S", "empty"], b"empty holds no samples"),
        (["--between", "S", "alien"], b"locus rsUnknown of alien is not in S"),         # B holds a locus A lacks: named
        (["--between", "dup", "T"], b"locus rs17 stands twice in dup"),                 # a duplicate locus ID, in A ...
        (["--between", "S", "dup"], b"locus rs17 stands twice in dup"),                 # ... in B ...
        (["--between", "dup", "dup"], b"locus rs17 stands twice in dup"),               # ... and in both, the tables identical
        (["--between-rows", "3", "--within", "S"], b"--between-rows sets the bands of --between"),
        (["--between-rows", "3", q, names[5]], b"--between-rows sets the bands of --between"),
        (["--between-rows", "3", "--against", "S", q], b"--between-rows sets the bands of --between"),
        (["--between", "S", "T", "--between-rows", "0"], b"--between-rows takes a number of rows of at least 1"),
        (["--between", "S", "T", "--between-rows", "x"], b"--between-rows takes a number of rows of at least 1"),
        (["--between", "S", "T", "--within-rows", "3"], b"--within-rows sets the bands of --within"),
    ]
    stores = ("S", "T", "alien", "dup", "empty", "trunc")
    for args, sentence in cases:
        before = {s: snapshot(at(s)) for s in stores}
        p = run(args, tmp_path)
        assert p.returncode == 1 and p.stdout == b"", (args, p.returncode, p.stdout[:100], p.stderr[-300:])
        errors = [line for line in p.stderr.split(b"\n") if line.startswith(b"Error: ")]
        assert len(errors) == 1 and sentence in errors[0], (args, p.stderr)
        assert all(unchanged(at(s), before[s]) for s in stores), args
        assert not any(os.path.exists(at(s + ".tmp")) for s in stores) and not os.path.exists(at("merged.txt")), args
    # the sentences the other runs always had
    p = run(["--index", "S", "--near", "S"] + P, tmp_path)
    assert p.returncode == 1 and b"are four runs" in p.stderr
    p = run(["--within-rows", "3", q, names[5]], tmp_path)
    assert p.returncode == 1 and b"--within-rows sets the bands of --within" in p.stderr


def test_map_and_band_rule_under_the_host_sanitizers():
    """`make between_check`: tools/eval_between_check.cpp -- eval_between.hpp's locus map (identity, a permutation, B lacking
    the first and last locus, an unknown ID, a duplicate ID, one site, random tables against a linear search) and its band
    rule (1 row, all rows, bands that tile) -- built with -fsanitize=address,undefined as a program of its own, run once by
    the target and once here for its lines."""
    subprocess.run(["make", "-s", "between_check"], cwd=ROOT, check=True, stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(ROOT, "build", "eval_between_check")], capture_output=True)
    assert p.returncode == 0 and p.stdout.endswith(b"ok\n") and b"FAILED" not in p.stdout and p.stderr == b"", (p.stdout[-600:], p.stderr[-600:])
    for part in (b"locus map: ", b"band rule: "):
        assert part in p.stdout


def test_nothing_to_score_needs_no_device():
    """n_a == 0, n_b == 0 and n_sites == 0: sessions without device work and zeroed outputs, on a machine without a GPU"""
    import ntsm_amd.eval as ev
    ones = np.ones((3, 5, 2), dtype=np.uint32)
    with ev.Between(np.zeros((0, 5, 2), dtype=np.uint32), ones) as s:                   # no sample of A: (0, 0) is the one range
        rec, a_geno, b_geno, times = s.rows(0, 0)
        assert rec.shape == (0, 3) and a_geno.shape == (0, 3) and not b_geno.any() and times.chunks == 0
        with pytest.raises(RuntimeError, match="failed: -1"):
            s.rows(0, 1)
    with ev.Between(ones, np.zeros((0, 5, 2), dtype=np.uint32), b_chunk=2) as s:        # no sample of B
        rec, a_geno, b_geno, times = s.rows(1, 2)
        assert rec.shape == (2, 0) and not a_geno.any() and b_geno.shape == (0, 3) and times.chunks == 0
    none = np.zeros((4, 0, 2), dtype=np.uint32)
    with ev.Between(ev.Records.of(none, HEAD), ev.Records.of(none[:2], HEAD)) as s:     # no site
        rec, a_geno, b_geno, times = s.rows(1, 3)
        assert rec.tobytes() == bytes(6 * 64) and a_geno.shape == (3, 3) and not a_geno.any() and not b_geno.any() and times.chunks == 0
    with ev.Between(ev.Records.of(none, HEAD), ones, site_map=np.zeros(0, dtype=np.uint32)) as s:    # no site of A, five of B
        assert s.rows(0, 4)[0].tobytes() == bytes(12 * 64)
    with pytest.raises(ValueError):
        ev.between_tune(128)
    ev.between_tune(0)


def test_bad_arguments_need_no_device():
    """-1, before any HIP call, for each bad argument of the contract: a NULL the call needs, a stride below 8 * n_sites or
    not a multiple of 4, a map entry past B's sites, a map that names a site of B twice, no map although the site counts
    differ; a row range past n_a, n_rows == 0, no room for the records"""
    import ntsm_amd.eval as ev
    a, b = np.ones((4, 5, 2), dtype=np.uint32), np.ones((3, 3, 2), dtype=np.uint32)
    good = np.array([0, LACKS, 1, LACKS, 2], dtype=np.uint32)
    h = ctypes.c_void_p()

    def opened(a_ptr=a.ctypes.data, a_stride=40, b_ptr=b.ctypes.data, b_stride=24, site_map=good, n_sites_b=3, handle=ctypes.byref(h)):
        return ev.lib.ntsm_eval_between_open(0, a_ptr, a_stride, 4, b_ptr, b_stride, 3, 5, n_sites_b, None if site_map is None else site_map.ctypes.data, 1, 0,
                                             handle)
    for bad in (dict(handle=None), dict(a_ptr=None), dict(b_ptr=None), dict(a_stride=36), dict(a_stride=42), dict(b_stride=20), dict(b_stride=26),
                dict(site_map=np.array([0, 3, 1, LACKS, 2], dtype=np.uint32)), dict(site_map=np.array([0, LACKS, 1, 0, 2], dtype=np.uint32)),
                dict(site_map=None), dict(site_map=None, n_sites_b=4, b_stride=32)):
        assert opened(**bad) == -1 and not h.value, bad
    for bad_map in ([0, 3, 1, LACKS, 2], [0, LACKS, 1, 0, 2]):
        with pytest.raises(RuntimeError, match="failed: -1"):
            ev.Between(a, b, site_map=bad_map)
    with ev.Between(a, np.zeros((0, 3, 2), dtype=np.uint32), site_map=good) as s:       # a session without device work: the ranges
        for first, rows in ((0, 0), (2, 0), (0, 5), (4, 1), (3, 2), (5, 0)):
            with pytest.raises(RuntimeError, match="failed: -1"):
                s.rows(first, rows)
        assert s.rows(3, 1)[0].shape == (1, 0)
    none = np.zeros((2, 0, 2), dtype=np.uint32)
    with ev.Between(none, none) as s:                                                   # four records and no room for them
        assert ev.lib.ntsm_eval_between_rows(s.h, 0, 2, None, None, None, None) == -1
        assert ev.lib.ntsm_eval_between_rows(None, 0, 2, None, None, None, None) == -1


# ---------------------------------------------------------------------------------------------------- GPU: the rectangle
# (n_a, n_b, sites, min_cov): one pair over one site; a lane short of a wave; exactly a wave; one lane past it; row counts that
# are no multiple of kTI = 4 (1, 3, 5, 9, 6, 1030); 257 columns (five one-wave tiles, two of 256 threads); each side past 1,024
SHAPES = [(1, 1, 1, 1), (3, 63, 7, 0), (5, 64, 300, 1), (4, 65, 300, 1), (9, 257, 200, 3), (6, 1030, 30, 1), (1030, 3, 30, 1)]
_rectangles = {}


def rectangle(shape):
    """(A, B, ntsm_eval_pairs' records of the rectangle on the concatenation [n_a][n_b], a_geno and b_geno as ntsm_eval_cross
    returns them): computed once per shape and left unchanged"""
    import ntsm_amd.eval as ev
    if shape not in _rectangles:
        n_a, n_b, m, c = shape
        rng = np.random.default_rng(list(shape))
        both = random_samples(rng, n_a + n_b, m, depth=30.0 if max(n_a, n_b) > 1000 else 8.0)
        if n_b > 4:
            both[n_a] = 0                                                               # a sample of B without any coverage
            both[n_a + 1] = both[0]                                                     # a copy of a sample of A
            both[n_a + 2] = rng.integers(2**31, 2**32, size=(m, 2)).astype(np.uint32)   # counts at and beyond 2^31
        n = n_a + n_b
        pairs = ev.pairs(both, min_cov=c)[0]
        where = np.array([[ev.pair_index(i, n_a + j, n) for j in range(n_b)] for i in range(n_a)])
        want = pairs[where]
        if max(n_a, n_b) > 1000:
            assert want["n_valid"][:, 3 if n_b > 4 else 0:].min() > 0                   # a record never written cannot pass
        a, b = both[:n_a].copy(), both[n_a:].copy()
        a_geno, b_geno = ev.cross(b[:1], a, min_cov=c)[1], ev.cross(a[:1], b, min_cov=c)[1]
        for x in (a, b, want, a_geno, b_geno):
            x.setflags(write=False)
        _rectangles[shape] = (a, b, want, a_geno, b_geno)
    return _rectangles[shape]


def ragged(n):
    """(row_first, n_rows): 1 row, then 2, then the rest"""
    starts = [s for s in (0, 1, 3) if s < n]
    return [(s, e - s) for s, e in zip(starts, starts[1:] + [n])]


def check_rows(a, b, want, a_geno, b_geno, c, chunk, bands, width=0, site_map=None):
    """Every band's records as raw bytes against the rows of `want`, both tallies, and the chunk count"""
    import ntsm_amd.eval as ev
    n_a, n_b = want.shape
    streamed = 0 < chunk < n_b
    ev.between_tune(width)
    try:
        with ev.Between(a, b, site_map=site_map, min_cov=c, b_chunk=chunk) as s:
            for first, rows in bands:
                rec, ag, bg, times = s.rows(first, rows)
                assert rec.shape == (rows, n_b)
                assert rec.tobytes() == want[first:first + rows].tobytes(), (want.shape, chunk, width, first, rows)
                assert np.array_equal(ag, a_geno[first:first + rows]) and np.array_equal(bg, b_geno), (want.shape, chunk, first)
                assert times.chunks == (-(-n_b // chunk) if streamed else 0), (want.shape, chunk, first, times.chunks)
    finally:
        ev.between_tune(0)


def ragged_chunk(n_b):
    """a chunk size that leaves a ragged last chunk: 100 for 257 and 1,030, 40 for 63 ... 65, 2 for 3"""
    return 100 if n_b > 100 else 40 if n_b > 40 else max(1, n_b - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=["a%d_b%d_m%d_c%d" % s for s in SHAPES])
def test_between_bands_equal_pairs_bits(shape):
    """ntsm_eval_between_rows on two sets of samples laid out at a store's stride against ntsm_eval_pairs on the dense
    concatenation, raw record bytes, and both tallies against ntsm_eval_cross: as one band and in ragged bands (1 row, 2, the
    rest), with B resident and streamed in ragged chunks, each at forced widths 64 and 256 and once under the library's rule;
    once from dense arrays."""
    import ntsm_amd.eval as ev
    a, b, want, a_geno, b_geno = rectangle(shape)
    n_a, n_b, m, c = shape
    ra, rb = ev.Records.of(a, HEAD), ev.Records.of(b, HEAD)
    assert ra.stride == HEAD + 8 * m
    one, bands, chunk = [(0, n_a)], ragged(n_a), ragged_chunk(n_b)
    assert sum(r for _, r in bands) == n_a and (n_b == 1 or -(-n_b // chunk) > 1)
    check_rows(ra, rb, want, a_geno, b_geno, c, 0, one + bands)                         # resident, the width rule
    check_rows(a, b, want, a_geno, b_geno, c, 0, one)                                   # ... from dense arrays
    for width in (64, 256):
        check_rows(ra, rb, want, a_geno, b_geno, c, 0, one + bands, width)
        check_rows(ra, rb, want, a_geno, b_geno, c, chunk, bands + one, width)          # streamed (resident where n_b is 1)


@pytest.mark.gpu
def test_between_records_equal_the_model_on_every_field():
    """5 x 65 x 300 against vec_pairs, the numpy model of tests/test_eval.py: every field of every record, doubles by their
    bits, with B resident and streamed"""
    import ntsm_amd.eval as ev
    n_a, n_b, m, c = shape = (5, 65, 300, 1)
    rng = np.random.default_rng(list(shape))
    both = random_samples(rng, n_a + n_b, m, depth=8.0)
    both[n_a] = 0
    both[n_a + 1] = both[0]
    model = vec_pairs(both, c)
    iu = np.triu_indices(n_a + n_b, 1)
    keep = np.flatnonzero((iu[0] < n_a) & (iu[1] >= n_a))                               # row-major over (a, b): the rectangle's order
    for chunk in (0, 16):
        with ev.Between(ev.Records.of(both[:n_a], HEAD), ev.Records.of(both[n_a:], HEAD), min_cov=c, b_chunk=chunk) as s:
            rec = s.rows(0, n_a)[0]
        bad = mismatches(rec.reshape(-1), {f: v[keep] for f, v in model.items()})
        assert not bad, (chunk, bad[:10])
    assert rec["n_valid"].max() > 0


# ---------------------------------------------------------------------------------------------------- GPU: a B with its own locus table
def remapped(b, site_map):
    """B over A's sites, as the contract states it: site s of A holds B's site site_map[s], 0 / 0 where B lacks it"""
    out = np.zeros((b.shape[0], len(site_map), 2), dtype=np.uint32)
    have = site_map != LACKS
    out[:, have] = b[:, site_map[have]]
    return out


def mapped_case(n_a, n_b, m, lacking, seed):
    rng = np.random.default_rng(seed)
    a = random_samples(rng, n_a, m, depth=8.0)
    kept = np.setdiff1d(np.arange(m), lacking)
    order = rng.permutation(kept)                                                       # B's site t is A's site order[t]
    site_map = np.full(m, LACKS, dtype=np.uint32)
    site_map[order] = np.arange(len(order), dtype=np.uint32)
    b = random_samples(rng, n_b, len(order), depth=8.0)
    if n_b > 2 and len(order) > 1:
        b[1] = a[0][order]                                                              # a sample of A, seen through B's table
        b[2] = rng.integers(2**31, 2**32, size=(len(order), 2)).astype(np.uint32)
    return a, b, site_map


def check_mapped(a, b, site_map, c, chunks):
    import ntsm_amd.eval as ev
    n_a, n_b = len(a), len(b)
    dense = remapped(b, site_map)
    both = np.concatenate([a, dense])
    pairs = ev.pairs(both, min_cov=c)[0]
    want = pairs[np.array([[ev.pair_index(i, n_a + j, n_a + n_b) for j in range(n_b)] for i in range(n_a)])]
    a_geno, b_geno = ev.cross(dense[:1], a, min_cov=c)[1], ev.cross(a[:1], dense, min_cov=c)[1]
    assert b_geno[:, 2].min() >= int((site_map == LACKS).sum())                         # a site B lacks is a missing site
    for chunk in chunks:
        check_rows(ev.Records.of(a, HEAD), ev.Records.of(b, HEAD), want, a_geno, b_geno, c, chunk, [(0, n_a)] + ragged(n_a), site_map=site_map)
    return want


@pytest.mark.gpu
def test_between_mapped_staging():
    """B's sites a random permutation of A's 300 with 17 removed, site 0 and the last among them, 70 samples (two tiles of the
    transpose, the second ragged; five tiles of sites, the last ragged): records and both tallies bytewise against
    ntsm_eval_pairs and ntsm_eval_cross on B remapped by numpy, with B resident and streamed in chunks of 16 and 64.  Then a B
    of exactly one site, A's site 4.  Then the identity given as a map: the bytes of site_map = NULL."""
    import ntsm_amd.eval as ev
    m = 300
    lacking = np.concatenate([[0, m - 1], np.random.default_rng(8).choice(np.arange(1, m - 1), size=15, replace=False)])
    a, b, site_map = mapped_case(7, 70, m, lacking, 17)
    assert (site_map == LACKS).sum() == 17 and site_map[0] == LACKS and site_map[-1] == LACKS and b.shape[1] == 283
    assert (np.diff(site_map[site_map != LACKS].astype(np.int64)) < 0).any()            # not monotone: a real permutation
    want = check_mapped(a, b, site_map, 1, (0, 16, 64))
    assert want["n_valid"].max() > 0
    a1, b1, map1 = mapped_case(5, 66, 40, np.setdiff1d(np.arange(40), [4]), 18)         # B holds one site
    assert b1.shape[1] == 1 and map1[4] == 0 and (map1 == LACKS).sum() == 39
    check_mapped(a1, b1, map1, 0, (0, 16))
    a2, b2 = a, remapped(b, site_map)                                                   # identical tables: the map says so, or NULL does
    out = []
    for given in (None, np.arange(m, dtype=np.uint32)):
        for chunk in (0, 16):
            with ev.Between(ev.Records.of(a2, HEAD), ev.Records.of(b2, HEAD), site_map=given, b_chunk=chunk) as s:
                rec, ag, bg, _ = s.rows(0, len(a2))
            out.append(rec.tobytes() + ag.tobytes() + bg.tobytes())
    assert len(set(out)) == 1 and out[0][:want.nbytes] == want.tobytes()


@pytest.mark.gpu
def test_between_a_store_and_itself_equals_within():
    """A store S of 65 samples: Between(S, S)'s record (i, j) for every i < j is Within(S)'s, as bytes; the diagonal is each
    sample against itself"""
    import ntsm_amd.eval as ev
    rng = np.random.default_rng(65)
    db = random_samples(rng, 65, 300, depth=8.0)
    db[0] = 0
    db[3] = db[1]
    recs = ev.Records.of(db, HEAD)
    with ev.Within(recs) as w:
        tri = w.rows(0, 65)[0]
    with ev.Between(recs, recs) as s:
        square, a_geno, b_geno, _ = s.rows(0, 65)
    iu = np.triu_indices(65, 1)
    assert square[iu].tobytes() == tri.tobytes() and np.array_equal(a_geno, b_geno)
    diag = square[np.arange(65), np.arange(65)]
    assert np.array_equal(diag["hets1"], diag["hets2"]) and np.array_equal(diag["ibs2"], diag["n_valid"].astype(np.uint32)) and not diag["ibs0"].any()


# ---------------------------------------------------------------------------------------------------- GPU: the CLI
def between_rows_of(files_a, files_b, args, cwd):
    """header + the oracle's rows over [A's files, B's files] whose sample 1 is a file of A and whose sample 2 one of B: for
    each a ascending, b ascending"""
    out = str(cwd / "oracle.out")
    with open(out, "wb") as fh:
        p = subprocess.run([ORACLE_CLI] + args + files_a + files_b, stdout=fh, stderr=subprocess.PIPE, cwd=str(cwd))
    assert p.returncode == 0, p.stderr[-300:]
    lines = open(out, "rb").read().split(b"\n")
    assert lines[-1] == b""
    sa, sb = set(f.encode() for f in files_a), set(f.encode() for f in files_b)
    keep = [r for r in lines[1:-1] if r.split(b"\t", 2)[0] in sa and r.split(b"\t", 2)[1] in sb]
    return b"".join(x + b"\n" for x in [lines[0]] + keep), len(keep)


def planted_cohort(tmp_path, n_a, n_b, m):
    """the counts files of test_eval_store.test_cli_against_equals_oracle_rows: sample n_a + 4 a copy of sample 0, sample
    n_a + 7 drawn a second time from sample 0's genotypes"""
    rng = np.random.default_rng(31 + n_a)
    samples = random_samples(rng, n_a + n_b, m, depth=30.0 if n_b > 1000 else 8.0)
    g = rng.integers(0, 3, size=m)
    lam = np.stack([np.where(g == 0, 30.0, np.where(g == 1, 15.0, 0.02)), np.where(g == 2, 30.0, np.where(g == 1, 15.0, 0.02))], axis=1)
    samples[0] = rng.poisson(lam)
    samples[n_a + 4] = samples[0]
    samples[n_a + 7] = rng.poisson(lam)
    files = [os.path.basename(f) for f in files_for(tmp_path, samples)]
    return samples, files[:n_a], files[n_a:]


COHORTS = [(3, 12, 3000), (1, 12, 3000), (2, 1030, 30)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_a,n_b,m", COHORTS, ids=["%dx%dx%d" % c for c in COHORTS])
def test_cli_between_equals_oracle_rows(gpu, tmp_path, n_a, n_b, m):
    """build/ntsmEval --between A.store B.store against oracle/ntsm_eval_oracle over [A's files, B's files]: the header and the
    rows that pair a file of A with one of B, stdout byte for byte, the four flag sets, each at -t 1 and -t 4; the 1,030-sample
    store by length, line count and SHA-256.  The default run prints at least the two planted rows.  Both stores stay as they
    were."""
    _, fa, fb = planted_cohort(tmp_path, n_a, n_b, m)
    assert run(["--pack", "A.store"] + fa, tmp_path).returncode == 0
    assert run(["--pack", "B.store"] + fb, tmp_path).returncode == 0
    before = snapshot(str(tmp_path / "A.store")), snapshot(str(tmp_path / "B.store"))
    for args in FLAGS:
        want, n_rows = between_rows_of(fa, fb, args, tmp_path)
        assert n_rows == n_a * n_b if "-a" in args else n_rows >= 2                     # the default threshold is not vacuous
        for t in ("1", "4"):
            p = run(args + ["-t", t, "--between", "A.store", "B.store"], tmp_path)
            assert p.returncode == 0, (args, p.stderr[-300:])
            assert b"Performing all-to-all score computation." in p.stderr
            assert (sig(p.stdout) == sig(want)) if n_b > 1000 else (p.stdout == want), (args, t)
    p = run(["-a", "-v", "-v", "--between", "A.store", "B.store"], tmp_path)
    assert p.returncode == 0 and b"store between: loci identical (0 of %d absent from B.store), B resident, 1 bands, 0 chunks" % m in p.stderr
    for part in (b"map ", b"upload ", b"prepare ", b"pair kernel ", b"download ", b"print "):
        assert part in p.stderr.split(b"store between: ")[1], part
    assert unchanged(str(tmp_path / "A.store"), before[0]) and unchanged(str(tmp_path / "B.store"), before[1])


@pytest.mark.gpu
def test_cli_between_mapped_store_and_bands(gpu, tmp_path):
    """B packed from files written in another locus order and lacking 23 of A's 3,000 loci, the first and the last among them,
    so its table differs from A's: stdout byte for byte against the oracle's rows over the text files under the four flag sets;
    -vv says "mapped" and how many loci B lacks.  --between-rows 1 and 2 (3 and 2 bands) give the bytes of the default
    banding.  A store against itself prints the full square, as two sets of files of the same content score."""
    n_a, n_b, m = 3, 12, 3000
    samples, fa, _ = planted_cohort(tmp_path, n_a, n_b, m)
    rng = np.random.default_rng(77)
    lacking = np.concatenate([[0, m - 1], rng.choice(np.arange(1, m - 1), size=21, replace=False)])
    order = rng.permutation(np.setdiff1d(np.arange(m), lacking))
    fb = []
    for j in range(n_b):
        fb.append("b%03d.txt" % j)
        write_counts(str(tmp_path / fb[-1]), samples[n_a + j][order], loci=["rs%d" % s for s in order])
    assert run(["--pack", "A.store"] + fa, tmp_path).returncode == 0
    assert run(["--pack", "B.store"] + fb, tmp_path).returncode == 0
    assert read_store(str(tmp_path / "B.store"))["loci"] == ["rs%d" % s for s in order] and read_store(str(tmp_path / "A.store"))["m"] == m
    for args in FLAGS:
        want, n_rows = between_rows_of(fa, fb, args, tmp_path)
        assert n_rows == n_a * n_b if "-a" in args else n_rows >= 2
        p = run(args + ["-v", "-v", "--between", "A.store", "B.store"], tmp_path)
        assert p.returncode == 0 and p.stdout == want, (args, p.stderr[-300:])
        assert b"store between: loci mapped (23 of 3000 absent from B.store), B resident, 1 bands, 0 chunks" in p.stderr
        for rows, bands in (("1", 3), ("2", 2)):
            p = run(args + ["-v", "-v", "--between-rows", rows, "--between", "A.store", "B.store"], tmp_path)
            assert p.returncode == 0 and p.stdout == want and b", %d bands, " % bands in p.stderr, (args, rows, p.stderr[-300:])
    p = run(["--between", "B.store", "A.store"], tmp_path)                              # A's loci that B lacks: B cannot play the first file
    assert p.returncode == 1 and p.stdout == b"" and b"of A.store is not in B.store" in p.stderr
    copies = []                                                                         # S against S: the files of A under a second set of names
    for f in fa:
        copies.append("copy_" + f)
        open(str(tmp_path / copies[-1]), "wb").write(open(str(tmp_path / f), "rb").read())
    want, n_rows = between_rows_of(fa, copies, ["-a"], tmp_path)
    p = run(["-a", "--between", "A.store", "A.store"], tmp_path)
    strip = lambda text: [r.split(b"\t")[2:] for r in text.split(b"\n")]  # noqa: E731
    assert p.returncode == 0 and n_rows == 9 and strip(p.stdout) == strip(want)
    assert [r.split(b"\t")[:2] for r in p.stdout.split(b"\n")[1:-1]] == [[a.encode(), b.encode()] for a in fa for b in fa]


@pytest.mark.gpu
def test_panel_store_against_run_store_end_to_end(gpu, tmp_path):
    """The route the run exists for, on tests/golden/vcf/plain (6 samples): `ntsmVCF --counts DIR --store panel.store` builds B
    from the genotypes; A is `--pack` of the same samples' counts files under other names (run0.txt ...), as a batch of
    sequencing runs would be filed.  With default flags --between prints exactly the six pairs (run i, sample i), each with
    same = 1 -- the oracle over the twelve text files says the same --, and -a prints all 36."""
    import shutil
    gold = os.path.join(ROOT, "tests", "golden", "vcf", "plain")
    for f in ("sites.fa", "genome.fa", "in.vcf"):
        shutil.copy(os.path.join(gold, f), str(tmp_path / f))
    os.mkdir(str(tmp_path / "DIR"))
    p = subprocess.run([os.path.join(ROOT, "build", "ntsmVCF"), "-s", "sites.fa", "-r", "genome.fa", "--counts", "DIR", "--store", "panel.store", "in.vcf"],
                       cwd=str(tmp_path), capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-500:]
    panel = ["DIR/S%d.counts.txt" % i for i in range(6)]
    assert [s["name"] for s in read_store(str(tmp_path / "panel.store"))["samples"]] == panel
    runs = []
    for i, f in enumerate(panel):
        runs.append("run%d.txt" % i)
        shutil.copy(str(tmp_path / f), str(tmp_path / runs[-1]))
    assert run(["--pack", "runs.store"] + runs, tmp_path).returncode == 0
    p = run(["--between", "runs.store", "panel.store"], tmp_path)
    assert p.returncode == 0, p.stderr[-300:]
    rows = [r.split(b"\t") for r in p.stdout.split(b"\n")[1:-1]]
    assert [(r[0], r[1], r[3]) for r in rows] == [(a.encode(), b.encode(), b"1") for a, b in zip(runs, panel)]
    assert p.stdout == between_rows_of(runs, panel, [], tmp_path)[0]
    p = run(["-a", "--between", "runs.store", "panel.store"], tmp_path)
    want, n_rows = between_rows_of(runs, panel, ["-a"], tmp_path)
    assert p.returncode == 0 and p.stdout == want and n_rows == 36
