"""ntsmEval's runs inside a cohort store: `--within STORE` prints the all-to-all run over the store's
own samples and `--within-near STORE` the -p run over them through STORE.pcaidx, both without reading a counts file.  Device
side: ntsm_eval_within_open / _rows / _close / _tune (ntsm_amd/csrc/ntsm_eval_within.hip) and ntsm_eval_store_score_pairs
(ntsm_eval_near.hip); host side: ntsm_amd/csrc/host/eval_within.hpp.

CPU: the surface, every refusal (indexes are written here from the documented layout), the calls that need no device, and
eval_within.hpp against brute force under the host sanitizers (`make within_check`).
GPU: every band of the triangle as raw bytes against the matching slice of ntsm_eval_pairs on the dense samples, listed pairs
against ntsm_eval_score_pairs, and the CLI's stdout byte for byte against `build/ntsmEval [flags] files...` -- paths this
feature does not touch and that tests/test_eval_reference.py holds to the reference class --, against the oracle's printer
and, where it is built, against oracle/_ref/ref_ntsmEval itself.  No comparison has a tolerance."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle_binding import ROOT
from test_eval import EVAL, ORACLE_CLI, files_for, mismatches, random_samples, vec_pairs
from test_eval_near import HEAD, gpu, index_args, index_bytes, loaded_pca, make_store, read_index, sig, without_pca  # noqa: F401
from test_eval_pca import write_pca
from test_eval_reference import (BIG_PCA, REF_EVAL, TIE_FREE, WIDE, cohorts, duplicate_cases, reference, restatement,  # noqa: F401
                                 same_up_to_tie_order, stdout_of, tie_free_args)
from test_eval_store import FLAGS, read_store, run, seven_files, snapshot, unchanged

SYMBOLS = ("ntsm_eval_within_open", "ntsm_eval_within_rows", "ntsm_eval_within_close", "ntsm_eval_within_tune", "ntsm_eval_store_score_pairs")


# ---------------------------------------------------------------------------------------------------- CPU
def test_surface():
    """The five entry points are exported and declared; the help text names both runs under its "This build only" part."""
    import ctypes
    lib = ctypes.CDLL(os.path.join(ROOT, "ntsm_amd", "libntsm_eval_hip.so"))
    hdr = open(os.path.join(ROOT, "include", "ntsm_eval_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert " %s(" % name in hdr, name
    assert "typedef struct ntsm_eval_within_session ntsm_eval_within_session;" in hdr
    p = subprocess.run([EVAL, "--help"], capture_output=True)
    assert p.returncode == 0 and p.stdout == b""
    ours = p.stderr.split(b"This build only")[1]
    assert b"--within = STORE" in ours and b"--within-near = STORE" in ours and b"--within-rows" in ours
    assert b"--pack" in ours and b"--near = STORE" in ours and b"against a store" in ours        # and what was there is


def test_refusals(tmp_path):
    """Every refusal of --within, --within-near and --within-rows: exit 1, an 'Error:' line, nothing on stdout, no GPU work
    (this test runs without one), the store and the index -- bytes and mtime -- as they were, no .tmp left.  The indexes are
    written here from the layout: a current one (S), a stale one (T: 3 of 4 samples), one with a broken magic (U), one a byte
    short (W), a current one of a one-sample store (one)."""
    names = seven_files(tmp_path)[0]
    write_pca(tmp_path, 40, 3, np.random.default_rng(5))
    for s in "STUW":
        assert run(["--pack", s] + names[:4], tmp_path).returncode == 0
    assert run(["--pack", "one"] + names[:1], tmp_path).returncode == 0
    assert run(["--pack", "bare"] + names[:2], tmp_path).returncode == 0               # a store without any index
    at = lambda x: str(tmp_path / x)  # noqa: E731
    norm, rot = loaded_pca(tmp_path, 40, 2)
    good = index_bytes(at("S"), 4, 2, 1, norm, rot)
    open(at("S.pcaidx"), "wb").write(good)
    open(at("T.pcaidx"), "wb").write(index_bytes(at("T"), 3, 2, 1, norm, rot))
    open(at("U.pcaidx"), "wb").write(b"NTSMPCX2" + good[8:])
    open(at("W.pcaidx"), "wb").write(good[:-1])
    open(at("one.pcaidx"), "wb").write(index_bytes(at("one"), 1, 2, 1, norm, rot))
    store = open(at("S"), "rb").read()
    with open(at("empty"), "wb") as f:                                                  # a valid store without samples
        f.write(store[:16] + struct.pack("<Q", 0) + store[24:read_store(at("S"))["first"]])
    with open(at("trunc"), "wb") as f:
        f.write(store[:-1])
    for x in ("empty", "trunc"):                                                        # an index does not make them stores
        open(at(x + ".pcaidx"), "wb").write(good)
    P = ["-p", "rot.tsv", "-n", "norm.txt", "-d", "2"]
    q = names[5]
    cases = []
    for mode in ("--within", "--within-near"):
        cases += [
            ([mode, "S", q], "S"),                                                      # FILES given
            ([mode, "S", "--pack", "S"], "S"),                                          # more than one of the six runs
            ([mode, "S", "--pack", "S", q], "S"),
            ([mode, "S", "--against", "S", q], "S"),
            ([mode, "S", "--index", "S"] + P, "S"),
            ([mode, "S", "--near", "S", q], "S"),
            ([mode, "S", "-p", "rot.tsv"], "S"),
            ([mode, "S", "-n", "norm.txt"], "S"),
            ([mode, "S"] + P, "S"),
            ([mode, "S", "-b", "truth.tsv"], "S"),
            ([mode, "S", "-e", "merged.txt"], "S"),
            ([mode, "S", "-o"], "S"),
            ([mode, "trunc"], "trunc"),                                                 # an invalid store
            ([mode, "nowhere"], "S"),                                                   # none at all
            ([mode, "empty"], "empty"),
            ([mode, "one"], "one"),                                                     # nothing to compare
        ]
    cases += [
        (["--within", "S", "--within-near", "S"], "S"),
        (["--within-near", "S", "--within-rows", "3"], "S"),                            # --within-rows without --within
        (["--within-rows", "3", q, names[6]], "S"),
        (["--within-rows", "3", "--against", "S", q], "S"),
        (["--within", "S", "--within-rows", "x"], "S"),
        (["--within-near", "bare"], "bare"),                                            # the index is absent
        (["--within-near", "U"], "U"),                                                  # invalid: magic
        (["--within-near", "W"], "W"),                                                  # invalid: size
        (["--within-near", "T"], "T"),                                                  # stale
        (["--within-near", "S", "-c", "2"], "S"),                                       # the index says -c 1
        (["--within-near", "S", "-d", "3"], "S"),                                       # the index says -d 2
    ]
    for args, touched in cases:
        path, idx = at(touched), at(touched + ".pcaidx")
        before = snapshot(path), (snapshot(idx) if os.path.exists(idx) else None)
        p = run(args, tmp_path)
        assert p.returncode == 1 and p.stdout == b"", (args, p.returncode, p.stdout[:100], p.stderr[-300:])
        assert any(line.startswith(b"Error: ") for line in p.stderr.split(b"\n")), (args, p.stderr)
        assert unchanged(path, before[0]), args
        assert (unchanged(idx, before[1]) if before[1] else not os.path.exists(idx)), args
        assert not os.path.exists(idx + ".tmp") and not os.path.exists(path + ".tmp") and not os.path.exists(at("merged.txt")), args
    assert b"--index" in run(["--within-near", "T"], tmp_path).stderr                   # the stale refusal says what to run
    assert b"--index" in run(["--within-near", "bare"], tmp_path).stderr
    assert b"--within-near" in run(["--within", "S", "-p", "rot.tsv"], tmp_path).stderr  # ... and this one which run takes -p's part
    assert b"nothing to compare" in run(["--within", "one"], tmp_path).stderr
    assert b"nothing to compare" in run(["--within-near", "one"], tmp_path).stderr
    assert b"--within-rows" in run(["--within-rows", "3", q, names[6]], tmp_path).stderr
    # the sentences the other runs always had
    p = run(["--against", "S", "-p", "rot.tsv", "-n", "norm.txt", q], tmp_path)
    assert p.returncode == 1 and b"against a store is not part of this build" in p.stderr
    p = run(["--pack", "S", "-p", "rot.tsv", q], tmp_path)
    assert p.returncode == 1 and b"with --pack is not part of this build" in p.stderr
    p = run(["--index", "S", "--near", "S"] + P, tmp_path)
    assert p.returncode == 1 and b"are four runs" in p.stderr


def test_band_and_pass_arithmetic_under_the_host_sanitizers():
    """`make within_check`: tools/eval_within_check.cpp -- eval_within.hpp's band offsets for n = 1 ... 70 and every
    (row_first, n_rows), the band rule, and the pass packing on random lists, each against brute force -- built with
    -fsanitize=address,undefined as a program of its own, run once by the target and once here for its lines."""
    subprocess.run(["make", "-s", "within_check"], cwd=ROOT, check=True, stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(ROOT, "build", "eval_within_check")], capture_output=True)
    assert p.returncode == 0 and p.stdout.endswith(b"ok\n") and b"FAILED" not in p.stdout and p.stderr == b"", (p.stdout[-600:], p.stderr[-600:])
    for part in (b"band offsets: ", b"band rule: ", b"pass packing: "):
        assert part in p.stdout


def test_no_pair_needs_no_device():
    """No sample, one sample, no site: sessions without device work, zeroed outputs; the rows a band may not name: -1"""
    import ntsm_amd.eval as ev
    with ev.Within(np.zeros((0, 5, 2), dtype=np.uint32)) as w:
        for first, rows in ((0, 0), (0, 1)):
            with pytest.raises(RuntimeError, match="failed: -1"):
                w.rows(first, rows)
    with ev.Within(np.ones((1, 5, 2), dtype=np.uint32)) as w:
        rec, geno, times = w.rows(0, 1)
        assert len(rec) == 0 and not geno.any() and times.chunks == 0
        with pytest.raises(RuntimeError, match="failed: -1"):
            w.rows(0, 2)
    with ev.Within(ev.Records.of(np.zeros((4, 0, 2), dtype=np.uint32), HEAD), db_chunk=2) as w:
        rec, geno, times = w.rows(1, 2)
        assert rec.tobytes() == bytes(3 * 64) and not geno.any() and times.chunks == 0
        for first, rows in ((0, 0), (0, 5), (4, 1), (3, 2)):
            with pytest.raises(RuntimeError, match="failed: -1"):
                w.rows(first, rows)
    with pytest.raises(ValueError):
        ev.within_tune(128)
    ev.within_tune(0)


def test_store_score_pairs_bad_lists_need_no_device():
    """-1 for an index out of range, for pi == pk and for db_chunk 1 (a pair needs two samples at once); an empty list is no
    work"""
    import ntsm_amd.eval as ev
    db = np.ones((4, 5, 2), dtype=np.uint32)
    for pi, pk in (([0], [4]), ([4], [0]), ([1], [1]), ([0, 2], [1, 2])):
        with pytest.raises(RuntimeError, match="failed: -1"):
            ev.store_score_pairs(db, pi, pk)
    with pytest.raises(RuntimeError, match="failed: -1"):
        ev.store_score_pairs(db, [0], [1], db_chunk=1)
    out, times = ev.store_score_pairs(db, [], [])
    assert len(out) == 0 and times.chunks == 0


# ---------------------------------------------------------------------------------------------------- GPU: the triangle
# (n, sites, min_cov): one pair; a wave less one; a full wave; one past it; 257 samples (five one-wave tiles); 1,025 and
# 1,030 samples: past 1,024 columns, where ntsm_eval_pairs switches to 256 threads (here the forced width does), five tiles
# of 256 columns, the last with one and with six live lanes
SHAPES = [(2, 1, 1), (63, 7, 0), (64, 300, 1), (65, 300, 1), (257, 200, 3), (1025, 24, 1), (1030, 30, 1)]
_triangles = {}


def triangle(shape):
    """(db, ntsm_eval_pairs' records on it, the tallies from a numpy count): computed once per shape and left unchanged"""
    import ntsm_amd.eval as ev
    if shape not in _triangles:
        n, m, c = shape
        rng = np.random.default_rng(list(shape))
        db = random_samples(rng, n, m, depth=30.0 if n > 1000 else 8.0)
        if n > 4:
            db[0] = 0                                                                   # a sample without any coverage
            db[3] = db[1]                                                               # a copy
            db[2] = rng.integers(2**31, 2**32, size=(m, 2)).astype(np.uint32)           # counts at and beyond 2^31 in one sample
            db[2, 0] = (2**31, 2**31)
        a, b = db[:, :, 0] > c, db[:, :, 1] > c
        geno = np.stack([(a & b).sum(1), (a ^ b).sum(1), (~a & ~b).sum(1)], axis=1).astype(np.uint32)
        want = ev.pairs(db, min_cov=c)[0]
        if n > 1000:
            assert want["n_valid"][ev.pair_index(4, 5, n):].min() > 0                   # a record never written cannot pass
        for x in (db, want, geno):
            x.setflags(write=False)
        _triangles[shape] = (db, want, geno)
    return _triangles[shape]


def ragged_bands(n):
    """(row_first, n_rows) tiling 0 ... n - 1 with bands that start off a multiple of 4 -- 0, 5, 66, 197, ... -- and end in two
    bands of one row: n - 2 (one pair) and n - 1 (none)"""
    starts = [s for s in (0, 5, 66, 197, 454, 967) if s < n - 2] + [n - 2, n - 1]
    starts = sorted(set(s for s in starts if s >= 0))
    return [(s, e - s) for s, e in zip(starts, starts[1:] + [n])]


def check_bands(shape, records, chunk, bands, width=0):
    """Every band's records as raw bytes against the slice of ntsm_eval_pairs, its tallies from row_first on, its chunk count"""
    import ntsm_amd.eval as ev
    db, want, tallies = triangle(shape)
    n, m, c = shape
    base = lambda r: r * n - r * (r + 1) // 2  # noqa: E731
    streamed = 0 < chunk < n
    ev.within_tune(width)
    try:
        with ev.Within(records, min_cov=c, db_chunk=chunk) as w:
            for first, rows in bands:
                rec, geno, times = w.rows(first, rows)
                assert len(rec) == base(first + rows) - base(first)
                assert rec.tobytes() == want[base(first):base(first + rows)].tobytes(), (shape, chunk, width, first, rows)
                assert np.array_equal(geno[first:], tallies[first:]) and not geno[:first].any(), (shape, chunk, first)
                assert times.chunks == (-(-(n - first) // chunk) if streamed else 0), (shape, chunk, first, times.chunks)
    finally:
        ev.within_tune(0)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=["n%d_m%d_c%d" % s for s in SHAPES])
def test_within_bands_equal_pairs_bits(shape):
    """ntsm_eval_within_rows on samples laid out at a store's stride (1,056 filler bytes in front of each) against
    ntsm_eval_pairs on the dense samples, raw record bytes and tallies: resident as one band and in ragged bands (starts 0, 5,
    66, ... and two last bands of one row); streamed with db_chunk 64 and 100 (ragged chunks, and chunks that begin mid-tile
    behind the diagonal) in the same bands and as one; each holding at forced widths 64 and 256; once from a dense array."""
    import ntsm_amd.eval as ev
    db = triangle(shape)[0]
    n = shape[0]
    rec = ev.Records.of(db, HEAD)
    assert rec.stride == HEAD + 8 * shape[1]
    one, ragged = [(0, n)], ragged_bands(n)
    assert sum(r for _, r in ragged) == n and ragged[-1] == (n - 1, 1) and (n < 8 or ragged[1][0] == 5)
    check_bands(shape, rec, 0, one + ragged)                                            # resident, the width rule
    check_bands(shape, db, 0, one)                                                      # ... from a dense array
    check_bands(shape, rec, 64, ragged + one)                                           # streamed (resident where 64 >= n)
    check_bands(shape, rec, 100, one + ragged[1:3])
    for width in (64, 256):
        check_bands(shape, rec, 0, one + ragged[1:2], width)
        check_bands(shape, rec, 100, one + ragged[1:2], width)


@pytest.mark.gpu
def test_within_records_equal_the_model_on_every_field():
    """65 x 300 against vec_pairs, the numpy model of tests/test_eval.py: every field of every pair, doubles by their bits"""
    import ntsm_amd.eval as ev
    shape = SHAPES[3]
    db = triangle(shape)[0]
    model = vec_pairs(db, shape[2])
    for chunk in (0, 16):
        with ev.Within(ev.Records.of(db, HEAD), min_cov=shape[2], db_chunk=chunk) as w:
            rec = w.rows(0, shape[0])[0]
        bad = mismatches(rec, model)
        assert not bad, (chunk, bad[:10])
    assert rec["n_valid"].max() > 0


# ---------------------------------------------------------------------------------------------------- GPU: listed pairs
def greedy_passes(pi, pk, chunk):
    """the passes of the contract: a pair joins while the pass's distinct samples stay <= chunk"""
    passes, held = 0, set()
    for a, b in zip(pi, pk):
        if not held or len(held | {int(a), int(b)}) > chunk:
            passes, held = passes + 1, set()
        held |= {int(a), int(b)}
    return passes


def check_store_pairs(db, pi, pk, c, chunk, passes=None):
    import ntsm_amd.eval as ev
    pi, pk = np.asarray(pi, dtype=np.uint32), np.asarray(pk, dtype=np.uint32)
    want = ev.score_pairs(db, pi, pk, min_cov=c)[0]
    got, times = ev.store_score_pairs(ev.Records.of(db, HEAD), pi, pk, min_cov=c, db_chunk=chunk)
    assert got.tobytes() == want.tobytes(), chunk
    assert times.chunks == (greedy_passes(pi, pk, chunk) if passes is None else passes), chunk
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 7, 300])
def test_store_score_pairs_equal_session_records(m):
    """65 samples (one without coverage, one a copy, one with counts beyond 2^31), 14 pairs in both orientations, sample 17
    named by six of them: records as raw bytes against ntsm_eval_score_pairs on the dense samples with db_chunk 2 (a pass per
    pair), 3 (greedy passes of up to three samples) and 0 (one pass)."""
    rng = np.random.default_rng([9, m])
    db = random_samples(rng, 65, m, depth=8.0)
    db[0] = 0
    db[40] = db[17]
    db[64] = rng.integers(2**31, 2**32, size=(m, 2)).astype(np.uint32)
    pairs = [(17, 3), (17, 40), (3, 17), (64, 17), (5, 17), (17, 0), (0, 64), (1, 2), (64, 0), (2, 1), (33, 34), (34, 17), (63, 62), (1, 64)]
    pi, pk = [p[0] for p in pairs], [p[1] for p in pairs]
    assert all(set(a) != set(b) for a, b in zip(pairs, pairs[1:]))                      # no two neighbours name the same two samples
    assert greedy_passes(pi, pk, 2) == len(pairs)
    for chunk, passes in ((2, len(pairs)), (3, None), (0, 1)):
        got = check_store_pairs(db, pi, pk, 1, chunk, passes)
    assert 1 < greedy_passes(pi, pk, 3) < len(pairs)
    if m > 1:
        assert got["n_valid"].max() > 0


@pytest.mark.gpu
def test_store_score_pairs_many_samples_in_passes():
    """1,030 x 24 sites with db_chunk 64: 1,500 random pairs in alternating orientation, every sample named, in dozens of
    passes whose records go back to list order; then the same list in one pass."""
    rng = np.random.default_rng(78)
    n, m = 1030, 24
    db = random_samples(rng, n, m, depth=30.0)
    a = np.concatenate([rng.permutation(n), rng.integers(0, n, size=470)])
    b = (a + 1 + rng.integers(0, n - 1, size=len(a))) % n
    pi, pk = np.where(np.arange(len(a)) % 2, a, b), np.where(np.arange(len(a)) % 2, b, a)
    assert (pi != pk).all() and greedy_passes(pi, pk, 64) > 20
    got = check_store_pairs(db, pi, pk, 1, 64)
    assert got["n_valid"].min() > 0                                                     # a record never written cannot pass
    assert check_store_pairs(db, pi, pk, 1, 0, 1).tobytes() == got.tobytes()


# ---------------------------------------------------------------------------------------------------- GPU: the CLI, --within
@pytest.fixture(scope="module")
def planted(tmp_path_factory, gpu):
    """The cohort of test_eval_store.test_cli_against_equals_oracle_rows, 15 x 3,000 with its two planted matches (sample 7 a
    copy of sample 0, sample 10 drawn a second time from sample 0's genotypes), packed whole -- once at a stroke and once as
    10 files and an append of 5."""
    d = tmp_path_factory.mktemp("planted")
    n_q, n_db, m = 3, 12, 3000
    rng = np.random.default_rng(31 + n_q)
    samples = random_samples(rng, n_q + n_db, m, depth=8.0)
    g = rng.integers(0, 3, size=m)
    lam = np.stack([np.where(g == 0, 30.0, np.where(g == 1, 15.0, 0.02)), np.where(g == 2, 30.0, np.where(g == 1, 15.0, 0.02))], axis=1)
    samples[0] = rng.poisson(lam)
    samples[n_q + 4] = samples[0]
    samples[n_q + 7] = rng.poisson(lam)
    files = [os.path.basename(f) for f in files_for(d, samples)]
    assert run(["--pack", "cohort.store"] + files, d).returncode == 0
    assert run(["--pack", "grown.store"] + files[:10], d).returncode == 0
    assert run(["--pack", "grown.store"] + files[10:], d).returncode == 0
    return d, files


@pytest.mark.gpu
@pytest.mark.parametrize("flags", FLAGS, ids=["default", "a", "a_s_w_c", "s_g_w"])
def test_cli_within_equals_the_run_over_the_files(planted, flags):
    """--within STORE against `build/ntsmEval [flags] files...`, against oracle/ntsm_eval_oracle and, where it is built,
    against oracle/_ref/ref_ntsmEval -t 1: stdout byte for byte at -t 1 and -t 4, with --within-rows absent, 1 and 7 (one, 15
    and 3 bands).  The default threshold prints at least the two planted rows."""
    d, files = planted
    want = stdout_of(EVAL, ["-t", "1"] + flags, files, d)
    assert stdout_of(ORACLE_CLI, flags, files, d) == want
    if os.path.isfile(REF_EVAL):
        assert reference(flags, files, d) == want
    rows = want.count(b"\n") - 1
    assert rows == 15 * 14 // 2 if "-a" in flags else rows >= 2                         # the threshold is not vacuous
    for t in ("1", "4"):
        for bands in ([], ["--within-rows", "1"], ["--within-rows", "7"]):
            p = run(["-t", t] + flags + bands + ["--within", "cohort.store"], d)
            assert p.returncode == 0 and p.stdout == want, (t, bands, p.stderr[-300:])
            assert b"Performing all-to-all score computation." in p.stderr


@pytest.mark.gpu
def test_cli_within_appended_store_and_its_report(planted):
    """A store built by --pack and an append holds the bytes of one --pack and prints the same rows; -vv reports the holding,
    the bands and the phases."""
    d, files = planted
    assert open(str(d / "grown.store"), "rb").read() == open(str(d / "cohort.store"), "rb").read()
    want = stdout_of(EVAL, ["-a"], files, d)
    before = snapshot(str(d / "grown.store"))
    p = run(["-a", "-v", "-v", "--within", "grown.store"], d)
    assert p.returncode == 0 and p.stdout == want and unchanged(str(d / "grown.store"), before), p.stderr[-300:]
    assert b"store within: resident, 1 bands, 0 chunks" in p.stderr and b"pair kernel" in p.stderr and b"print" in p.stderr
    p = run(["-a", "-v", "-v", "--within-rows", "7", "--within", "grown.store"], d)
    assert p.returncode == 0 and p.stdout == want and b"store within: resident, 3 bands" in p.stderr


@pytest.mark.gpu
def test_cli_within_wide_cohort(gpu, built, cohorts):
    """1,030 x 30 under -a (530,000 rows; seventeen one-wave tiles of columns in the first bands): length, line count and SHA-256 against
    the run over the files, the oracle and, where built, the reference; as one band and in 148 bands of 7 rows."""
    d, names, _ = cohorts.get(WIDE)
    assert run(["--pack", "wide.store"] + names, d).returncode == 0
    want = sig(stdout_of(EVAL, ["-t", "1", "-a"], names, d))
    assert want[1] == 1 + 1030 * 1029 // 2 and sig(stdout_of(ORACLE_CLI, ["-a"], names, d)) == want
    if os.path.isfile(REF_EVAL):
        assert sig(reference(["-a"], names, d)) == want
    for bands in ([], ["--within-rows", "7"]):
        p = run(["-a"] + bands + ["--within", "wide.store"], d)
        assert p.returncode == 0 and sig(p.stdout) == want, (bands, p.stderr[-300:])


# ---------------------------------------------------------------------------------------------------- GPU: the CLI, --within-near
def within_near(args, store, d, extra=()):
    return stdout_of(EVAL, list(extra) + without_pca(args) + ["--within-near", store], [], d)


@pytest.mark.gpu
@pytest.mark.parametrize("spec", TIE_FREE, ids=lambda s: "n%d_m%d_d%d" % (s[1], s[2], s[4]))
def test_cli_within_near_equals_the_pca_run(gpu, built, cohorts, restatement, spec):
    """--pack of all files, --index, --within-near on the tie-free cohorts, -a, radii at the 15th and 60th percentile: stdout
    byte for byte, at -t 1 and -t 4, against `ntsmEval -p -n ... files...` and, where it is built, the reference class."""
    d, names, s, args = tie_free_args(restatement, cohorts, spec)
    make_store(d, "within.store", names, args)
    want = stdout_of(EVAL, ["-t", "1"] + args, names, d)
    assert want.count(b"\n") > len(names)
    for t in ("1", "4"):
        assert within_near(args, "within.store", d, ["-t", t]) == want, t
    if os.path.isfile(REF_EVAL):
        assert reference(args, names, d) == want
    assert read_index(os.path.join(str(d), "within.store.pcaidx"))["n"] == len(names)


@pytest.mark.gpu
def test_cli_within_near_duplicate_cohort(gpu, built, cohorts, restatement):
    """The planted-duplicate cohort (40 x 3,000; sample 39 a copy of sample 0, sample 3 empty) under the five flag sets of
    DUPLICATE_CASES (the index is rebuilt where -d or -c change): byte for byte against this build's -p run -- exact ties
    come out by k on both sides -- and the same rows up to the order among ties against the reference."""
    d, names, cases = duplicate_cases(restatement, cohorts)
    for args in cases:
        make_store(d, "dupw.store", names, args)
        want = stdout_of(EVAL, ["-t", "1"] + args, names, d)
        assert want.count(b"\n") >= 2, args
        got = within_near(args, "dupw.store", d)
        assert got == want, args
        if os.path.isfile(REF_EVAL):
            assert same_up_to_tie_order(got, reference(args, names, d)), args


@pytest.mark.gpu
def test_cli_within_near_big_cohort(gpu, built, cohorts, restatement):
    """1,030 x 64 sites, dim 3, by length, line count and SHA-256: the empty sample 3 is a search-all row, whose 1,029 pairs
    come out of the dense rectangle; the rest are listed pairs."""
    d, names, s, args = tie_free_args(restatement, cohorts, BIG_PCA)
    make_store(d, "bigw.store", names, args)
    text = stdout_of(EVAL, ["-t", "1"] + args, names, d)
    own = [r for r in text.split(b"\n")[1:-1] if r.split(b"\t", 1)[0] == names[3].encode()]
    assert len(own) == 1029                                                             # the search-all row: every other sample, under -a
    p = run(["-v", "-v"] + without_pca(args) + ["--within-near", "bigw.store"], d)
    assert p.returncode == 0 and sig(p.stdout) == sig(text), p.stderr[-300:]
    assert b"1 dense rows" in p.stderr and b" listed, " in p.stderr and b"0 listed" not in p.stderr
    if os.path.isfile(REF_EVAL):
        assert sig(reference(args, names, d)) == sig(text)


@pytest.mark.gpu
def test_cli_within_near_after_an_append(gpu, built, cohorts, restatement):
    """Pack 9 samples and index them; pack 4 more: --within-near refuses the stale index and names --index; after --index its
    output is that of the 13-sample cohort."""
    d, names, s, args = tie_free_args(restatement, cohorts, TIE_FREE[2])
    first, more = names[:9], names[9:13]
    make_store(d, "groww.store", first, args)
    assert within_near(args, "groww.store", d) == stdout_of(EVAL, ["-t", "1"] + args, first, d)
    assert run(["--pack", "groww.store"] + more, d).returncode == 0
    p = run(without_pca(args) + ["--within-near", "groww.store"], d)
    assert p.returncode == 1 and p.stdout == b"" and b"Error: " in p.stderr and b"--index" in p.stderr
    p = run(["-v", "--index", "groww.store"] + index_args(args), d)
    assert p.returncode == 0 and b"Projected 4 samples" in p.stderr, p.stderr[-300:]
    assert within_near(args, "groww.store", d) == stdout_of(EVAL, ["-t", "1"] + args, first + more, d)
