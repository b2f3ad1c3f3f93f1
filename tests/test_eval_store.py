"""ntsmEval's cohort store and query mode: `--pack STORE FILES...` writes the binary store of
ntsm_amd/csrc/host/eval_store.hpp, `--against STORE FILES...` scores the query files against the store's samples in
ntsm_eval_cross (include/ntsm_eval_hip.h, ntsm_amd/csrc/ntsm_eval_cross.hip) and prints the rows that the all-pairs run over
[queries..., store samples...] prints for the queries.

CPU: the store's bytes against a reader written here from the documented layout, append identity, every refusal, the surface.
GPU: the records of the rectangle bit for bit against ntsm_eval_pairs on the concatenation and against vec_pairs (the numpy
model of tests/test_eval.py), and the CLI's stdout byte for byte against the oracle's rows."""
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle_binding import ROOT
from test_eval import EVAL, ORACLE_CLI, files_for, mismatches, random_samples, vec_pairs, write_counts

HEAD, NAME = 64, 1024


def run(args, cwd):
    return subprocess.run([EVAL] + list(args), capture_output=True, cwd=str(cwd))


def read_store(path):
    """The layout as eval_store.hpp and DESIGN.md section 9 document it, read independently of the package."""
    b = open(path, "rb").read()
    assert b[:8] == b"NTSMCOH1"
    version, m, n, first, stride = struct.unpack_from("<IIQQQ", b, 8)
    assert version == 1 and b[40:64] == bytes(24) and stride % 8 == 0 and stride == 32 + NAME + 8 * m
    at, loci = HEAD, []
    for _ in range(m):
        end = b.index(b"\0", at)
        loci.append(b[at:end].decode())
        at = end + 1
    pad = (at + 7) // 8 * 8
    assert b[at:pad] == bytes(pad - at)
    distinct = np.frombuffer(b, dtype="<u4", count=2 * m, offset=pad).reshape(m, 2)
    assert first == pad + 8 * m and len(b) == first + n * stride
    samples = []
    for r in range(n):
        o = first + r * stride
        raw_total, total, sum_of_sums, ks, reserved = struct.unpack_from("<QQQII", b, o)
        name = b[o + 32:o + 32 + NAME]
        assert reserved == 0 and name.rstrip(b"\0") + bytes(NAME - len(name.rstrip(b"\0"))) == name
        counts = np.frombuffer(b, dtype="<u4", count=2 * m, offset=o + 32 + NAME).reshape(m, 2)
        samples.append(dict(name=name.rstrip(b"\0").decode(), raw_total=raw_total, total=total, sum_of_sums=sum_of_sums, ks=ks, counts=counts))
    return dict(loci=loci, distinct=distinct, samples=samples, first=first, stride=stride, n=n, m=m)


def wrapped_sum(x):
    """sum over the sites of uint32(x[:, 0] + x[:, 1]), widened: what the reader's `unsigned + unsigned` gives"""
    x = np.asarray(x, dtype=np.uint32)
    return int((x[:, 0] + x[:, 1]).astype(np.uint64).sum())


def seven_files(tmp_path):
    """7 counts files over 40 sites and what a store must hold for each: (names, counts, sums, raw_total, ks, distinct)"""
    rng = np.random.default_rng(21)
    m = 40
    counts = rng.integers(0, 40, size=(7, m, 2)).astype(np.uint32)
    sums = (counts * 3 + 1).astype(np.uint32)
    counts[4, :10] = rng.integers(2**31, 2**32, size=(10, 2)).astype(np.uint32)        # both columns at and beyond 2^31: the total wraps
    counts[4, 10] = (2**31, 2**31)
    sums[4, :10] = rng.integers(2**31, 2**32, size=(10, 2)).astype(np.uint32)
    distinct = rng.integers(1, 30, size=(m, 2)).astype(np.uint32)
    tk, ks = [1000 + i for i in range(7)], [19, 0, 21, 19, 19, 25, 19]
    names = ["f%d.txt" % i for i in range(7)]
    for i in (0, 4, 5, 6):
        write_counts(str(tmp_path / names[i]), counts[i], sums=sums[i], distinct=distinct, tk=tk[i], ks=ks[i])
    with open(str(tmp_path / names[1]), "w") as f:                                      # no #@TK / #@KS, no column header
        for s in range(m):
            f.write("rs%d\t%d\t%d\t%d\t%d\t1\t1\n" % (s, counts[1, s, 0], counts[1, s, 1], sums[1, s, 0], sums[1, s, 1]))
    tk[1] = 0
    order = rng.permutation(m)
    with open(str(tmp_path / names[2]), "w") as f:                                      # the loci in another order, tags after the sites
        f.write("#locusID\tcountAT\tcountCG\tsumAT\tsumCG\tdistinctAT\tdistinctCG\n")
        for s in order:
            f.write("rs%d\t%d\t%d\t%d\t%d\t7\t7\n" % (s, counts[2, s, 0], counts[2, s, 1], sums[2, s, 0], sums[2, s, 1]))
        f.write("#@KS\t21\n#@TK\t%d\n" % tk[2])
    lacking = (3, 17, 39)
    with open(str(tmp_path / names[3]), "w") as f:                                      # three loci absent
        f.write("#@TK\t%d\n#@KS\t%d\n" % (tk[3], ks[3]))
        for s in range(m):
            if s not in lacking:
                f.write("rs%d\t%d\t%d\t%d\t%d\t1\t1\n" % (s, counts[3, s, 0], counts[3, s, 1], sums[3, s, 0], sums[3, s, 1]))
    for s in lacking:
        counts[3, s] = 0
        sums[3, s] = 0
    return names, counts, sums, tk, ks, distinct


def unchanged(path, before):
    st = os.stat(path)
    return (open(path, "rb").read(), st.st_mtime_ns) == before


def snapshot(path):
    return (open(path, "rb").read(), os.stat(path).st_mtime_ns)


# ---------------------------------------------------------------------------------------------------- CPU
def test_pack_round_trip(tmp_path):
    """--pack of 7 files x 40 sites (one without tag lines, one in another locus order, one lacking three loci, one whose
    counts and sums pass 2^31 in both columns) read back by read_store: names, raw_total, total and sum_of_sums (recomputed
    with uint32 wrap-around), k, distinct, every count; packing twice gives identical bytes."""
    names, counts, sums, tk, ks, distinct = seven_files(tmp_path)
    p = run(["--pack", "S"] + names, tmp_path)
    assert p.returncode == 0 and p.stdout == b"", p.stderr
    s = read_store(str(tmp_path / "S"))
    assert (s["n"], s["m"]) == (7, 40) and s["loci"] == ["rs%d" % i for i in range(40)]
    assert np.array_equal(s["distinct"], distinct)
    for i, r in enumerate(s["samples"]):
        assert r["name"] == names[i]
        assert (r["raw_total"], r["ks"]) == (tk[i], ks[i]), i
        assert r["total"] == wrapped_sum(counts[i]) and r["sum_of_sums"] == wrapped_sum(sums[i]), i
        assert np.array_equal(r["counts"], counts[i]), i
    assert s["samples"][4]["total"] < int(counts[4].astype(np.uint64).sum())            # the wrap happened
    q = run(["--pack", "T"] + names, tmp_path)
    assert q.returncode == 0 and open(str(tmp_path / "S"), "rb").read() == open(str(tmp_path / "T"), "rb").read()
    assert not os.path.exists(str(tmp_path / "S.tmp"))


def test_append_equals_packing_at_once(tmp_path):
    """--pack S a b c, then --pack S d e: the bytes of --pack S2 a b c d e.  The appended files are read against the
    store's locus table, as later files of a run are read against the first."""
    names = seven_files(tmp_path)[0]
    assert run(["--pack", "S"] + names[:3], tmp_path).returncode == 0
    assert run(["--pack", "S"] + names[3:5], tmp_path).returncode == 0
    assert run(["--pack", "S2"] + names[:5], tmp_path).returncode == 0
    a, b = open(str(tmp_path / "S"), "rb").read(), open(str(tmp_path / "S2"), "rb").read()
    assert a == b and read_store(str(tmp_path / "S"))["n"] == 5


def test_refusals(tmp_path):
    """Every refusal of --pack and --against: exit 1, an 'Error:' line, nothing on stdout, no GPU work (this test runs
    without one), and the store -- bytes and mtime -- as it was."""
    names = seven_files(tmp_path)[0]
    assert run(["--pack", "S"] + names[:4], tmp_path).returncode == 0
    store = str(tmp_path / "S")
    good = open(store, "rb").read()
    layout = read_store(store)
    with open(str(tmp_path / "trunc"), "wb") as f:
        f.write(good[:-1])
    with open(str(tmp_path / "magic"), "wb") as f:
        f.write(b"NTSMCOH2" + good[8:])
    with open(str(tmp_path / "version"), "wb") as f:
        f.write(good[:8] + struct.pack("<I", 2) + good[12:])
    with open(str(tmp_path / "longer"), "wb") as f:
        f.write(good + bytes(8))
    with open(str(tmp_path / "empty"), "wb") as f:                                      # a valid store without samples
        f.write(good[:16] + struct.pack("<Q", 0) + good[24:layout["first"]])
    assert read_store(str(tmp_path / "empty"))["n"] == 0
    with open(str(tmp_path / "alien.txt"), "w") as f:
        f.write("#@TK\t5\n#@KS\t19\nrs1\t3\t4\t3\t4\t1\t1\nrsUnknown\t3\t4\t3\t4\t1\t1\n")
    long_name = "./" * 510 + names[5]
    assert len(long_name) >= 1024 and os.path.exists(os.path.join(str(tmp_path), long_name))
    cases = [
        (["--pack", "S"], "S"),                                                          # no input files
        (["--pack", "trunc", names[5]], "trunc"),
        (["--pack", "magic", names[5]], "magic"),
        (["--pack", "version", names[5]], "version"),
        (["--pack", "longer", names[5]], "longer"),
        (["--pack", "S", names[5], "alien.txt"], "S"),                                  # a locus the store does not know, after a good file
        (["--pack", "S", names[5], names[1]], "S"),                                     # a name already in the store
        (["--pack", "S", names[5], names[5]], "S"),                                     # the same name twice in one call
        (["--pack", "S", long_name], "S"),
        (["--pack", "S", "--against", "S", names[5]], "S"),
        (["--pack", "S", "-p", "rot.tsv", names[5]], "S"),
        (["--pack", "S", "-e", "merged.txt", names[5]], "S"),
        (["--pack", "S", "-o", names[5]], "S"),
        (["--against", "trunc", names[5]], "trunc"),
        (["--against", "magic", names[5]], "magic"),
        (["--against", "empty", names[5]], "empty"),
        (["--against", "S"], "S"),                                                       # no query file
        (["--against", "S", "-p", "rot.tsv", "-n", "norm.txt", names[5]], "S"),
        (["--against", "S", "-b", "truth.tsv", names[5]], "S"),
        (["--against", "S", "-e", "merged.txt", names[5]], "S"),
        (["--against", "S", "-o", names[5]], "S"),
        (["--against", "S", names[5], "alien.txt"], "S"),                               # an unknown locus in a query file
    ]
    for args, touched in cases:
        path = str(tmp_path / touched)
        before = snapshot(path)
        p = run(args, tmp_path)
        assert p.returncode == 1 and p.stdout == b"", (args, p.returncode, p.stdout[:100], p.stderr[-300:])
        assert any(line.startswith(b"Error: ") for line in p.stderr.split(b"\n")), (args, p.stderr)
        assert unchanged(path, before), args
        assert not os.path.exists(path + ".tmp") and not os.path.exists(str(tmp_path / "merged.txt")), args
    p = run(["--pack", "fresh", "alien.txt", names[5]], tmp_path)                       # creation refused: no store appears
    assert p.returncode == 1 and b"Error: " in p.stderr and not os.path.exists(str(tmp_path / "fresh")) and not os.path.exists(str(tmp_path / "fresh.tmp"))
    p = run(["-a", "-p", "rot.tsv", "--against", "S", names[5]], tmp_path)
    assert b"not part of this build" in p.stderr


def test_surface():
    """The library exports ntsm_eval_cross, the header declares it and its times, the help text names both options."""
    import ctypes
    lib = ctypes.CDLL(os.path.join(ROOT, "ntsm_amd", "libntsm_eval_hip.so"))
    assert hasattr(lib, "ntsm_eval_cross") and hasattr(lib, "ntsm_eval_pairs")
    hdr = open(os.path.join(ROOT, "include", "ntsm_eval_hip.h")).read()
    assert "int ntsm_eval_cross(int device, const uint32_t *q_counts, uint32_t n_q, const void *db_counts, uint64_t db_stride_bytes," in hdr
    assert "typedef struct ntsm_eval_cross_times" in hdr
    p = subprocess.run([EVAL, "--help"], capture_output=True)
    assert p.returncode == 0 and p.stdout == b""
    assert b"--pack" in p.stderr and b"--against" in p.stderr and b"This build only" in p.stderr
    assert b"against a store" in p.stderr                                              # the PCA-guided search against a store: not in this build


# ---------------------------------------------------------------------------------------------------- GPU
# (n_q, n_db, sites, min_cov, db_chunk).  The cross kernel runs 64-thread workgroups at every size (the all-pairs kernel
# switches to 256 past 1,024 samples; this one has no such switch), so 1,024 / 1,025 are a full last wave and one lane past it.
SHAPES = [(1, 1, 1, 1, 0), (1, 63, 7, 0, 0), (4, 64, 300, 1, 0), (5, 65, 300, 1, 64), (3, 257, 200, 3, 100),
          (2, 1283, 24, 1, 512), (9, 1030, 24, 1, 0), (2, 1024, 24, 1, 0), (2, 1025, 24, 1, 0)]
_cohorts = {}


def cohort(shape):
    """(q, db, records of ntsm_eval_pairs on the concatenation, vec_pairs of the concatenation): computed once per shape"""
    import ntsm_amd.eval as ev
    if shape not in _cohorts:
        n_q, n_db, m, c, _ = shape
        rng = np.random.default_rng(list(shape))
        wide = n_db > 1000
        samples = random_samples(rng, n_q + n_db, m, depth=30.0 if wide else 8.0)
        q, db = samples[:n_q].copy(), samples[n_q:].copy()
        if wide:
            db[4] = q[0]
        elif n_db > 4:
            db[0] = 0                                                                   # a sample without any coverage
            db[1] = q[0]                                                                # a copy of a query
            db[2] = rng.integers(2**31, 2**32, size=(m, 2)).astype(np.uint32)           # counts beyond 2^31
        both = np.concatenate([q, db])
        model = vec_pairs(both, c)
        if wide:
            assert model["n_valid"].min() > 0                                           # a record never written cannot pass
        _cohorts[shape] = (q, db, ev.pairs(both, min_cov=c)[0], model)
        for a in _cohorts[shape][:2]:
            a.setflags(write=False)
    return _cohorts[shape]


def check_cross(shape, rec, geno):
    import ntsm_amd.eval as ev
    n_q, n_db, m, c, _ = shape
    q, db, pairs, model = cohort(shape)
    n = n_q + n_db
    assert rec.shape == (n_q, n_db)
    where = np.array([[ev.pair_index(qi, n_q + d, n) for d in range(n_db)] for qi in range(n_q)])
    assert rec.tobytes() == pairs[where].tobytes(), shape                               # raw record bytes against ntsm_eval_pairs
    bad = mismatches(rec.reshape(-1), {f: v[where.reshape(-1)] for f, v in model.items()})
    assert not bad, (shape, bad[:10])                                                   # every field against the numpy model
    a, b = db[:, :, 0] > c, db[:, :, 1] > c
    want = np.stack([(a & b).sum(1), (a ^ b).sum(1), (~a & ~b).sum(1)], axis=1)
    assert np.array_equal(geno, want), shape


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=["q%d_db%d_m%d_c%d_chunk%d" % s for s in SHAPES])
def test_cross_records_bit_for_bit(shape):
    """ev.cross(q, db, c, chunk) against ev.pairs on the concatenation (raw record bytes at pair_index(q, n_q + d)) and
    against vec_pairs of the concatenation (every field, doubles by their bits); geno against a numpy count; the chunk
    count.  The launch has no width switch (64-thread workgroups at every size; the 256-thread form is
    test_cross_every_launch_shape's), so beside the shapes past 1,024 samples only (2, 1024) and (2, 1025) are added:
    where the all-pairs kernel switches."""
    import ntsm_amd.eval as ev
    n_q, n_db, m, c, chunk = shape
    q, db = cohort(shape)[:2]
    rec, geno, times = ev.cross(q, db, min_cov=c, db_chunk=chunk)
    check_cross(shape, rec, geno)
    assert times.chunks == (-(-n_db // chunk) if chunk else 1)                          # these fit the device in one pass


FORCED = [(SHAPES[3], 64, 4), (SHAPES[3], 64, 2), (SHAPES[3], 256, 1), (SHAPES[6], 256, 4), (SHAPES[6], 64, 2), (SHAPES[6], 64, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,width,group", FORCED, ids=["q%d_db%d_w%d_g%d" % (s[0], s[1], w, g) for s, w, g in FORCED])
def test_cross_every_launch_shape(shape, width, group):
    """The library picks the query group (1, 2 or 4 queries per workgroup) by how full the launch is, and rectangles as
    small as a test's always get single queries; ntsm_eval_cross_tune forces the other instantiations: 5 and 9 queries
    against groups of 4 and 2 (a ragged last group), both widths."""
    import ntsm_amd.eval as ev
    q, db = cohort(shape)[:2]
    assert ev.lib.ntsm_eval_cross_tune(3, 0) == -1 and ev.lib.ntsm_eval_cross_tune(0, 3) == -1
    assert ev.lib.ntsm_eval_cross_tune(width, group) == 0
    try:
        rec, geno, times = ev.cross(q, db, min_cov=shape[3], db_chunk=shape[4])
    finally:
        assert ev.lib.ntsm_eval_cross_tune(0, 0) == 0
    check_cross(shape, rec, geno)


@pytest.mark.gpu
def test_cross_empty_sides():
    """n_q, n_db or the sites empty: zeroed outputs of the right shape"""
    import ntsm_amd.eval as ev
    z = np.zeros((0, 5, 2), dtype=np.uint32)
    s = np.ones((3, 5, 2), dtype=np.uint32)
    assert ev.cross(z, s)[0].shape == (0, 3) and ev.cross(s, z)[0].shape == (3, 0)
    rec, geno, times = ev.cross(np.zeros((2, 0, 2), dtype=np.uint32), np.zeros((3, 0, 2), dtype=np.uint32))
    assert rec.tobytes() == bytes(6 * 64) and not geno.any() and times.chunks == 0


def oracle_rows(files, args, queries, cwd):
    """header + the oracle's rows over `files` whose sample 1 is a query; they are a prefix of its rows"""
    out = str(cwd / "oracle.out")
    with open(out, "wb") as fh:
        p = subprocess.run([ORACLE_CLI] + args + files, stdout=fh, stderr=subprocess.PIPE, cwd=str(cwd))
    assert p.returncode == 0, p.stderr[-300:]
    lines = open(out, "rb").read().split(b"\n")
    assert lines[-1] == b""
    rows = lines[1:-1]
    names = set(f.encode() for f in queries)
    keep = [r for r in rows if r.split(b"\t", 1)[0] in names]
    assert rows[:len(keep)] == keep
    return b"".join(x + b"\n" for x in [lines[0]] + keep), len(keep)


FLAGS = [[], ["-a"], ["-a", "-s", "0.1", "-w", "0", "-c", "2"], ["-s", "5", "-g", "3100000000", "-w", "0.5"]]
COHORTS = [(3, 12, 3000), (1, 12, 3000), (2, 1030, 30)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_q,n_db,m", COHORTS, ids=["%dx%dx%d" % c for c in COHORTS])
def test_cli_against_equals_oracle_rows(tmp_path, n_q, n_db, m):
    """build/ntsmEval --against STORE QUERIES against oracle/ntsm_eval_oracle over [queries..., database files...]: the
    header and the rows whose sample 1 is a query (asserted to be a prefix of the oracle's rows), stdout byte for byte, four
    flag sets, each also with -t 4; the 1,030-sample store by length, line count and SHA-256.  Plain random_samples at
    depth 8 puts no pair of 15 x 3,000 below the default threshold 0.5, so two are planted: a database sample that is a
    copy of query 0, and one drawn a second time (Poisson, depth 30) from the genotype vector query 0 was drawn from --
    the default run prints at least those two rows."""
    rng = np.random.default_rng(31 + n_q)
    samples = random_samples(rng, n_q + n_db, m, depth=30.0 if n_db > 1000 else 8.0)
    g = rng.integers(0, 3, size=m)
    lam = np.stack([np.where(g == 0, 30.0, np.where(g == 1, 15.0, 0.02)), np.where(g == 2, 30.0, np.where(g == 1, 15.0, 0.02))], axis=1)
    samples[0] = rng.poisson(lam)
    samples[n_q + 4] = samples[0]
    samples[n_q + 7] = rng.poisson(lam)
    files = [os.path.basename(f) for f in files_for(tmp_path, samples)]
    queries, database = files[:n_q], files[n_q:]
    assert run(["--pack", "cohort.store"] + database, tmp_path).returncode == 0
    for args in FLAGS:
        want, n_rows = oracle_rows(files, args, queries, tmp_path)
        if not args:
            assert n_rows >= 2                                                          # the default threshold is not vacuous
        if "-a" in args:
            assert n_rows == n_q * (n_q - 1) // 2 + n_q * n_db
        for extra in ([], ["-t", "4"]):
            p = run(args + extra + ["--against", "cohort.store"] + queries, tmp_path)
            assert p.returncode == 0, (args, p.stderr[-300:])
            assert b"Performing all-to-all score computation." in p.stderr
            if n_db > 1000:
                sig = lambda d: (len(d), d.count(b"\n"), hashlib.sha256(d).hexdigest())  # noqa: E731
                assert sig(p.stdout) == sig(want), (args, extra)
            else:
                assert p.stdout == want, (args, extra)
    p = run(["-a", "-v", "-v", "--against", "cohort.store"] + queries, tmp_path)
    assert p.returncode == 0 and b"store query: 1 chunks" in p.stderr and b"cross kernel" in p.stderr


@pytest.mark.gpu
def test_cli_against_counts_from_the_counting_tool(tmp_path):
    """Three counts files from build/ntsmCount (the SynthShort recipe of test_cli_equals_oracle_cli_bytes): two packed,
    the third as the query with -a: the oracle's rows for that query."""
    import ntsm_amd as nt
    sp = str(tmp_path / "sites.fa")
    nt.SynthShort(sites_seed=5, n_sites=2000, read_seed=1, p_embed=0.9, sites_path=sp)
    outs = []
    for i, seed in enumerate((1, 2, 3)):
        fq, out = str(tmp_path / ("r%d.fq" % i)), "c%d.txt" % i
        nt.SynthShort(sites_seed=5, n_sites=2000, read_seed=seed, p_embed=0.9).write_fastq(fq, 0, 60000)
        with open(str(tmp_path / out), "wb") as fh:
            subprocess.run([os.path.join(ROOT, "build", "ntsmCount"), "-s", sp, fq], stdout=fh, stderr=subprocess.DEVNULL, check=True)
        outs.append(out)
    assert run(["--pack", "two.store"] + outs[:2], tmp_path).returncode == 0
    want, n_rows = oracle_rows([outs[2]] + outs[:2], ["-a"], [outs[2]], tmp_path)
    p = run(["-a", "--against", "two.store", outs[2]], tmp_path)
    assert p.returncode == 0 and p.stdout == want and n_rows == 2, p.stderr[-300:]
