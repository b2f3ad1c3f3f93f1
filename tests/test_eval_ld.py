"""`ntsmEval --ld STORE`: which pairs of sites of a cohort store are in linkage disequilibrium, and which
sites does a prune keep?  Device side: ntsm_eval_ld_open / _rows / _select (ntsm_amd/csrc/ntsm_eval_ld.hip): bit-planes with the
samples along the bits and a popcount GEMM over sites x sites; host side: ntsm_amd/csrc/host/eval_ld.hpp.  The reference has no
such run: the oracle is Model below, an exact numpy statement of the contract in include/ntsm_eval_hip.h, itself held against a
scalar restatement of that text.

CPU, devices hidden: the surface, every refusal, the failure without a device, the bad-argument returns and empty shapes, r^2,
the rows and the prune through libntsm_host.so against the Python expressions, the band walk against brute force, and the
premise of the LD fixture.
GPU: open, _rows and _select against the model at the shapes where their kernels can go wrong, in bands, in chunks, under every
forced register block; the CLI byte for byte against the model's text.
Every accumulated quantity is an integer and r^2 is one stated double expression: no comparison has a tolerance."""
import ctypes
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle_binding import ROOT
from test_eval_qc import COUNT, EVAL, HEAD, HIDDEN, RECORD_HEAD, qc_cohort, run, write_store
from test_eval_store import read_store, snapshot, unchanged
from test_eval_trio import edge_cells

HEADER = "siteA\tsiteB\tn\tr2\tdir\n"
FIELDS = ("n", "hs", "gs", "ht", "gt", "hh", "hg", "gg")
RECORD = np.dtype([(f, "<u4") for f in FIELDS])
PAIR = np.dtype([("a", "<u4"), ("b", "<u4"), ("rec", RECORD)])
T, M, DEPTH = 0.5, 20, 8                                                                     # the defaults of --ld-min, --ld-called, --ld-depth
BLOCKS = ((0, 0), (2, 2), (4, 2), (2, 4))                                                    # ntsm_eval_ld_tune: the rule and every forced block


# ---------------------------------------------------------------------------------------------------- the models
def moments(r):
    """The contract's moments in Python integers: (n, cov, vx, vy)"""
    n, hs, gs, ht, gt, hh, hg, gg = (int(r[f]) for f in FIELDS)
    sx, sy, sxx, syy, sxy = hs + 2 * gs, ht + 2 * gt, hs + 4 * gs, ht + 4 * gt, hh + 2 * hg + 4 * gg
    return n, n * sxy - sx * sy, n * sxx - sx * sx, n * syy - sy * sy


def r2_of(r, m=M):
    """None where r^2 is undefined; else the double of the contract.  Python floats are IEEE doubles, int -> float rounds to
    nearest, and a * a / (b * c) is two multiplications and one division, as the C++ expression is."""
    n, cov, vx, vy = moments(r)
    if n < m or vx == 0 or vy == 0:
        return None
    return float(cov) * float(cov) / (float(vx) * float(vy))


class Model:
    """The contract of include/ntsm_eval_hip.h in numpy: boolean matrices H, G, C [n][m] from the class rule, the eight counts of
    every ordered site pair as int64 matrix products, site_geno [m][4]"""

    def __init__(self, db, c, depth):
        db = np.asarray(db, dtype=np.uint32)
        a, g = db[:, :, 0], db[:, :, 1]
        A, G = a > c, g > c
        deep = a.astype(np.uint64) + g.astype(np.uint64) >= np.uint64(depth)
        self.H, self.G, at = A & G, ~A & G & deep, A & ~G & deep
        self.C = self.H | self.G | at
        self.n, self.m = db.shape[0], db.shape[1]
        self._defined = {}
        H, G_, C = (p.astype(np.int64) for p in (self.H, self.G, self.C))
        self.rec = np.zeros((self.m, self.m), dtype=RECORD)
        self.rec["n"], self.rec["hs"], self.rec["gs"], self.rec["ht"], self.rec["gt"] = C.T @ C, H.T @ C, G_.T @ C, C.T @ H, C.T @ G_
        self.rec["hh"], self.rec["hg"], self.rec["gg"] = H.T @ H, H.T @ G_ + G_.T @ H, G_.T @ G_
        self.site_geno = np.stack([self.H.sum(0), self.G.sum(0), self.C.sum(0), at.sum(0)], axis=1).astype(np.uint32).reshape(self.m, 4)

    def defined(self, m=M):
        """(a, b, r2) of every pair a < b whose r^2 is defined at m, in (a, b) order; formed once per m"""
        if m not in self._defined:
            self._defined[m] = [(a, b, r) for a in range(self.m) for b in range(a + 1, self.m) for r in [r2_of(self.rec[a, b], m)] if r is not None]
        return self._defined[m]

    def pairs(self, t=T, m=M, first=0, rows=None):
        """The selected pairs (a, b), a in the band, a < b, in (a, b) order, as PAIR records"""
        last = self.m if rows is None else first + rows
        out = [(a, b, self.rec[a, b]) for a, b, r in self.defined(m) if first <= a < last and r >= t]
        return np.array(out, dtype=PAIR) if out else np.zeros(0, dtype=PAIR)


def scalar_records(db, c, depth):
    """The same contract one sample at a time, in Python integers: rec[s][t] = the eight counts"""
    def cls(a, g):
        A, G, t = a > c, g > c, a + g
        return 1 if A and G else 0 if A and not G and t >= depth else 2 if not A and G and t >= depth else 3
    k = [[cls(int(a), int(g)) for a, g in row] for row in db]
    n, m = len(k), len(k[0])
    rec = [[[0] * 8 for _ in range(m)] for _ in range(m)]
    for i in range(n):
        for s in range(m):
            for t in range(m):
                u, v, r = k[i][s], k[i][t], rec[s][t]
                if u != 3 and v != 3:
                    r[0] += 1
                if v != 3:
                    r[1] += u == 1
                    r[2] += u == 2
                if u != 3:
                    r[3] += v == 1
                    r[4] += v == 2
                r[5] += u == 1 and v == 1
                r[6] += (u, v) in ((1, 2), (2, 1))
                r[7] += u == 2 and v == 2
    return rec


def line(loci, p, m=M):
    r2 = r2_of(p["rec"], m)
    return "%s\t%s\t%d\t%f\t%s\n" % (loci[int(p["a"])], loci[int(p["b"])], int(p["rec"]["n"]), r2, "+" if moments(p["rec"])[1] > 0 else "-")   # std::to_string prints %f


def ld_text(model, loci, t=T, m=M, all_rows=False):
    """stdout of `ntsmEval --ld` from the model"""
    return (HEADER + "".join(line(loci, p, m) for p in model.pairs(0.0 if all_rows else t, m))).encode()


def prune(model_pairs, n_sites):
    """The prune of the contract, site by site: t is dropped when some selected pair (s, t), s < t, has s kept"""
    by_b = {}
    for p in model_pairs:
        by_b.setdefault(int(p["b"]), []).append(int(p["a"]))
    kept = []
    for t in range(n_sites):
        kept.append(not any(kept[s] for s in by_b.get(t, [])))
    return kept


def walk(row_pairs, budget):
    """The band walk of eval_ld.hpp, restated: every call as (first, rows, return)"""
    n = len(row_pairs)
    cap, rows, first, calls = max(budget, n), n, 0, []
    while first < n:
        rows = min(rows, n - first)
        over = int(sum(row_pairs[first:first + rows]) > cap)
        calls.append((first, rows, over))
        if over:
            assert rows > 1
            rows //= 2
        else:
            first += rows
    return calls


def rec_of(*v):
    r = np.zeros((), dtype=RECORD)
    for f, x in zip(FIELDS, v):
        r[f] = x
    return r


def rec_from(x, y):
    """The record of two sites from their dosage lists (None = not called)"""
    both = [(u, v) for u, v in zip(x, y) if u is not None and v is not None]
    return rec_of(len(both), sum(u == 1 for u, v in both), sum(u == 2 for u, v in both), sum(v == 1 for u, v in both), sum(v == 2 for u, v in both),
                  sum(u == 1 and v == 1 for u, v in both), sum((u, v) in ((1, 2), (2, 1)) for u, v in both), sum(u == 2 and v == 2 for u, v in both))


def ld_cohort(seed=11, n=200, blocks=49, cov=30.0, err=0.002):
    """The LD fixture: blocks of six sites -- a base site in Hardy-Weinberg proportions at an allele frequency uniform in [0.1,
    0.9], copies of it with genotypes redrawn at rates 0, 0.02, 0.1 and 0.3, and an inverted copy (dosage 2 - x) --, then a
    monomorphic site, a site nobody is called at and four independent sites: 300 sites, 200 samples at depth Poisson(30), 3 % of
    the cells missing."""
    rng = np.random.default_rng(seed)

    def draw(p, size):
        return (rng.random(size) < p).astype(np.int64) + (rng.random(size) < p).astype(np.int64)
    cols = []
    for _ in range(blocks):
        p = rng.uniform(0.1, 0.9)
        base = draw(p, n)
        cols.append(base)
        for rate in (0.0, 0.02, 0.1, 0.3):
            cols.append(np.where(rng.random(n) < rate, draw(p, n), base))
        cols.append(2 - base)
    mono = len(cols)
    cols.append(np.zeros(n, dtype=np.int64))                                                # monomorphic: everybody homAT, no stray read
    never = len(cols)
    cols.append(draw(0.5, n))                                                               # never called: emptied below
    for _ in range(4):
        cols.append(draw(rng.uniform(0.1, 0.9), n))
    dose = np.stack(cols, axis=1)                                                           # [n][m], the CG dosage
    frac = dose / 2.0 * (1 - err) + (1 - dose / 2.0) * err
    depth = rng.poisson(cov, size=dose.shape)
    cg = rng.binomial(depth, frac)
    db = np.stack([depth - cg, cg], axis=2).astype(np.uint32)
    db[rng.random(dose.shape) < 0.03] = 0
    db[:, never] = 0
    db[:, mono, 1] = 0
    return db


@pytest.fixture(scope="module")
def fixture_model():
    db = ld_cohort()
    return db, Model(db, 1, DEPTH)


# ---------------------------------------------------------------------------------------------------- CPU
def test_surface():
    """The five entry points are exported and declared, the records are 32 and 40 bytes here and in the binding, the host
    functions are exported by libntsm_host.so, the genotype rule is one function that both bit-plane libraries include, and the
    help text names the flags under "This build only" and says that the defaults are conventions."""
    lib = ctypes.CDLL(os.path.join(ROOT, "ntsm_amd", "libntsm_eval_hip.so"))
    host = ctypes.CDLL(os.path.join(ROOT, "ntsm_amd", "libntsm_host.so"))
    hdr = open(os.path.join(ROOT, "include", "ntsm_eval_hip.h")).read()
    for name in ("ntsm_eval_ld_open", "ntsm_eval_ld_rows", "ntsm_eval_ld_select", "ntsm_eval_ld_close", "ntsm_eval_ld_tune"):
        assert hasattr(lib, name) and name + "(" in hdr, name
    for name in ("ntsm_host_ld_r2", "ntsm_host_ld_rows", "ntsm_host_ld_prune", "ntsm_host_ld_bands"):
        assert hasattr(host, name), name
    assert "typedef struct ntsm_eval_ld_record { uint32_t n, hs, gs, ht, gt, hh, hg, gg; } ntsm_eval_ld_record;" in hdr
    assert "typedef struct ntsm_eval_ld_pair { uint32_t a, b; ntsm_eval_ld_record rec; } ntsm_eval_ld_pair;" in hdr
    assert RECORD.itemsize == 32 and PAIR.itemsize == 40
    import ntsm_amd.eval as ev
    assert ev.LD_RECORD == RECORD and ev.LD_PAIR == PAIR
    for f in (ev.Ld, ev.ld_tune, ev.ld_r2, ev.ld_rows_text, ev.ld_prune, ev.ld_bands):
        assert callable(f)
    tune = ev.lib.ntsm_eval_ld_tune
    assert tune(4, 4) == -1 and tune(1, 1) == -1 and tune(0, 2) == -1 and all(tune(r, c) == 0 for r, c in BLOCKS[1:] + BLOCKS[:1])
    csrc = os.path.join(ROOT, "ntsm_amd", "csrc")
    for unit in ("ntsm_eval_trio.hip", "ntsm_eval_ld.hip"):                                  # the rule once, not as a copy
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "ntsm_eval_geno.h"' in text and "ntsm_eval_class_of(" in text and "min_depth) return 3" not in text, unit
    p = subprocess.run([EVAL, "--help"], capture_output=True, env=HIDDEN)
    assert p.returncode == 0 and p.stdout == b""
    ours = p.stderr.split(b"This build only")[1]
    for flag in (b"--ld = STORE", b"--ld-depth = INT", b"--ld-min = FLOAT", b"--ld-called = INT", b"--ld-prune = FILE"):
        assert flag in ours, flag
    assert b"[8 reads]" in ours and b"[0.500000]" in ours and b"[20 samples]" in ours and b"All three defaults are conventions to override" in ours
    assert b"--trios = STORE" in ours and b"--contam = STORE" in ours                            # and what was there is


def huge_store(path, n, m=1):
    """A store whose header describes n samples of m sites, as a sparse file: valid to the reader, never read further"""
    section = b"".join(b"rs%d\0" % s for s in range(m))
    section += bytes(-(HEAD + len(section)) % 8) + bytes(8 * m)
    first, stride = HEAD + len(section), RECORD_HEAD + 8 * m
    with open(str(path), "wb") as f:
        f.write(b"NTSMCOH1" + struct.pack("<IIQQQ", 1, m, n, first, stride) + bytes(24) + section)
        f.truncate(first + n * stride)


def test_refusals(tmp_path):
    """Every refusal of --ld and its flags: exit 1, its own 'Error:' sentence, nothing on stdout, no GPU work (devices are
    hidden), the store -- bytes and mtime -- as it was, no --ld-prune file made and one that was there as it was."""
    rng = np.random.default_rng(5)
    db = rng.integers(0, 30, size=(4, 40, 2)).astype(np.uint32)
    write_store(tmp_path / "S", db, rng)
    write_store(tmp_path / "one", db[:1], rng)
    write_store(tmp_path / "site", db[:, :1], rng)
    write_store(tmp_path / "empty", db[:0], rng)
    huge_store(tmp_path / "huge", (1 << 24) + 1)
    good = open(str(tmp_path / "S"), "rb").read()
    open(str(tmp_path / "trunc"), "wb").write(good[:-1])
    open(str(tmp_path / "magic"), "wb").write(b"NTSMCOH2" + good[8:])
    open(str(tmp_path / "q.txt"), "w").write("#@TK\t5\n#@KS\t19\nrs1\t1\t2\t1\t2\t1\t1\n")
    open(str(tmp_path / "rot.tsv"), "w").write("x\n")
    open(str(tmp_path / "norm.txt"), "w").write("0\n")
    open(str(tmp_path / "fam.ped"), "w").write("F run0002 run0000 run0001 0 0\n")
    open(str(tmp_path / "old.txt"), "w").write("kept\n")
    os.mkdir(str(tmp_path / "dir"))
    own = b"--ld compares the sites of one store and is a run of its own"
    flags = b"belong to --ld: give them with --ld STORE"
    cases = [
        (["--ld", "S", "--pack", "S", "q.txt"], "S", own),                                   # with any other store run
        (["--ld", "S", "--against", "S", "q.txt"], "S", own),
        (["--ld", "S", "--index", "S", "-p", "rot.tsv", "-n", "norm.txt"], "S", own),
        (["--ld", "S", "--near", "S", "q.txt"], "S", own),
        (["--ld", "S", "--within", "S"], "S", own),
        (["--ld", "S", "--within-near", "S"], "S", own),
        (["--ld", "S", "--between", "S", "S"], "S", own),
        (["--between-near", "S", "--ld", "S", "S"], "S", own),
        (["--qc", "S", "--ld", "S"], "S", own),
        (["--contam", "S", "--ld", "S"], "S", own),
        (["--trios", "S", "--ld", "S"], "S", own),
        (["--ld-depth", "4", "--within", "S"], "S", flags),                                  # its flags without it
        (["--ld-min", "0.1", "--qc", "S"], "S", flags),
        (["--ld-called", "2", "q.txt"], "S", flags),
        (["--ld-prune", "kept.txt", "--trios", "S"], "S", flags),
        (["--ld", "S", "q.txt"], "S", b"--ld takes no input files"),
        (["--ld", "S", "-p", "rot.tsv", "-n", "norm.txt"], "S", b"--ld reads allele counts, not projections, and takes no -p and no -n"),
        (["--ld", "S", "-p", "rot.tsv"], "S", b"takes no -p and no -n"),
        (["--ld", "S", "-n", "norm.txt"], "S", b"takes no -p and no -n"),
        (["--ld", "S", "-b", "truth.tsv"], "S", b"-b with --ld is not part of this build"),
        (["--ld", "S", "-e", "merged.txt"], "S", b"merging (-e, -o) with --ld is not part of this build"),
        (["--ld", "S", "-o"], "S", b"merging (-e, -o) with --ld is not part of this build"),
        (["--ld", "trunc"], "trunc", b"its header describes"),                               # an invalid store
        (["--ld", "magic"], "magic", b"not a cohort store"),
        (["--ld", "nowhere"], "S", b"cannot open store nowhere"),
        (["--ld", "empty"], "empty", b"empty holds no samples"),
        (["--ld", "one"], "one", b"one holds fewer than 2 samples"),
        (["--ld", "site"], "site", b"site holds fewer than 2 sites"),
        (["--ld", "huge"], None, b"huge holds more than 16777216 samples"),
        (["--ld", "S", "--ld-min", "half"], "S", b"--ld-min takes a number, not half"),        # a value that does not parse
        (["--ld", "S", "--ld-min", "0.5x"], "S", b"--ld-min takes a number, not 0.5x"),
        (["--ld", "S", "--ld-min", ""], "S", b"--ld-min takes a number, not "),
        (["--ld", "S", "--ld-min", "nan"], "S", b"--ld-min takes a number, not nan"),           # not finite
        (["--ld", "S", "--ld-min", "inf"], "S", b"--ld-min takes a number, not inf"),
        (["--ld", "S", "--ld-min", "-inf"], "S", b"--ld-min takes a number, not -inf"),
        (["--ld", "S", "--ld-depth", "-1"], "S", b"--ld-depth takes a number of reads, not -1"),
        (["--ld", "S", "--ld-depth", "4294967296"], "S", b"--ld-depth takes a number of reads, not 4294967296"),
        (["--ld", "S", "--ld-called", "two"], "S", b"--ld-called takes a number of samples, not two"),
        (["--ld", "S", "--ld-called", "-3"], "S", b"--ld-called takes a number of samples, not -3"),
        (["--ld", "S", "--ld-prune", "dir"], "S", b"cannot write dir"),                       # an unwritable --ld-prune path
        (["--ld", "S", "--ld-prune", "nowhere/kept.txt"], "S", b"cannot write nowhere/kept.txt"),
        (["--ld", "S", "--ped", "fam.ped"], "S", b"belong to --trios"),
        (["--ld", "S", "--samples-out", "samples.tsv"], "S", b"--samples-out is the per-sample table of --contam"),
        (["--ld", "S", "--sites-out", "sites.tsv"], "S", b"--sites-out is the per-site table of --qc"),
        (["--ld", "S", "--within-rows", "3"], "S", b"--within-rows sets the bands of --within"),
        (["--ld", "S", "--between-rows", "3"], "S", b"--between-rows sets the bands of --between"),
    ]
    huge = os.stat(str(tmp_path / "huge"))
    for args, touched, sentence in cases:
        before = snapshot(str(tmp_path / touched)) if touched else None
        p = run(args, tmp_path, env=HIDDEN)
        assert p.returncode == 1 and p.stdout == b"", (args, p.returncode, p.stdout[:100], p.stderr[-300:])
        errors = [l for l in p.stderr.split(b"\n") if l.startswith(b"Error: ")]
        assert len(errors) == 1 and sentence in errors[0], (args, p.stderr)
        if touched:
            assert unchanged(str(tmp_path / touched), before), args
        for left in ("kept.txt", "samples.tsv", "sites.tsv", "merged.txt", "S.pcaidx", "S.tmp"):
            assert not os.path.exists(str(tmp_path / left)), (args, left)
    now = os.stat(str(tmp_path / "huge"))
    assert (now.st_size, now.st_mtime_ns) == (huge.st_size, huge.st_mtime_ns)
    # a refusal that comes after the prune file's path was given leaves a file that was there as it was
    p = run(["--ld", "one", "--ld-prune", "old.txt"], tmp_path, env=HIDDEN)
    assert p.returncode == 1 and open(str(tmp_path / "old.txt")).read() == "kept\n"
    # the sentences the other runs always had
    p = run(["--qc", "S", "--trios", "S"], tmp_path, env=HIDDEN)
    assert p.returncode == 1 and b"--trios looks for parent-child trios in one store and is a run of its own" in p.stderr


def test_ld_without_a_device_fails_and_prints_nothing(tmp_path):
    """A valid --ld where no device can be opened: the GPU failure message, exit 3, no header on stdout, the store as it was, no
    --ld-prune file made -- and one that was there keeps its bytes."""
    rng = np.random.default_rng(6)
    write_store(tmp_path / "S", rng.integers(0, 30, size=(4, 40, 2)).astype(np.uint32), rng)
    open(str(tmp_path / "old.txt"), "w").write("kept\n")
    before = snapshot(str(tmp_path / "S"))
    for args in ([], ["-a", "-c", "0", "--ld-depth", "0", "--ld-min", "-1", "--ld-called", "0", "-v", "-v"], ["--ld-prune", "kept.txt"], ["--ld-prune", "old.txt"]):
        p = run(["--ld", "S"] + args, tmp_path, env=HIDDEN)
        assert p.returncode == 3 and p.stdout == b"", (args, p.returncode, p.stdout[:100], p.stderr[-300:])
        assert b"on the GPU failed" in p.stderr and b"there is no CPU path" in p.stderr, (args, p.stderr)
        assert unchanged(str(tmp_path / "S"), before) and not os.path.exists(str(tmp_path / "kept.txt"))
        assert open(str(tmp_path / "old.txt")).read() == "kept\n"


def test_bad_arguments_and_empty_shapes_need_no_device():
    """-1 before any HIP call: open with a stride below 8 * n_sites, one that is no multiple of 4, counts NULL, the handle's place
    NULL, n_db > 2^24; rows and select with a range past n_sites, no rows, a NULL they need, the handle NULL; select with a
    non-finite r2_min.  A store without samples gives zeroed records and selects nothing, one without sites has no range to take
    -- none touches a device."""
    import ntsm_amd.eval as ev
    opn, rows, select, close = ev.lib.ntsm_eval_ld_open, ev.lib.ntsm_eval_ld_rows, ev.lib.ntsm_eval_ld_select, ev.lib.ntsm_eval_ld_close
    m, n = 5, 4
    db = np.ones((n, m, 2), dtype=np.uint32)
    h = ctypes.c_void_p(1)
    assert opn(0, db.ctypes.data, 8 * m - 8, n, m, 1, 8, 0, None, None, ctypes.byref(h)) == -1 and h.value is None
    assert opn(0, db.ctypes.data, 8 * m - 4, n, m, 1, 8, 0, None, None, ctypes.byref(h)) == -1
    assert opn(0, db.ctypes.data, 8 * m + 2, n, m, 1, 8, 0, None, None, ctypes.byref(h)) == -1
    assert opn(0, None, 8 * m, n, m, 1, 8, 0, None, None, ctypes.byref(h)) == -1
    assert opn(0, db.ctypes.data, 8 * m, n, m, 1, 8, 0, None, None, None) == -1
    assert opn(0, db.ctypes.data, 8 * m, (1 << 24) + 1, m, 1, 8, 0, None, None, ctypes.byref(h)) == -1 and h.value is None
    out = np.frombuffer(b"\x07" * (32 * m * m), dtype=RECORD).copy().reshape(m, m)
    pairs = np.frombuffer(b"\x07" * (40 * 8), dtype=PAIR).copy()
    found, ms = ctypes.c_uint64(9), ctypes.c_double(5.0)
    assert rows(None, 0, 1, out.ctypes.data, None) == -1 and select(None, 0, 1, M, T, 8, pairs.ctypes.data, ctypes.byref(found), None) == -1
    geno = np.full((m, 4), 7, np.uint32)
    times = ev.CrossTimes(1.0, 1.0, 1.0, 1.0, 9)
    assert opn(0, None, 8 * m, 0, m, 1, 8, 0, geno.ctypes.data, ctypes.byref(times), ctypes.byref(h)) == 0 and h.value   # no sample: a session without device work
    assert not geno.any() and times.chunks == 0 and times.upload_ms == 0
    assert rows(h, 0, 0, out.ctypes.data, None) == -1 and rows(h, 1, m, out.ctypes.data, None) == -1 and rows(h, m, 1, out.ctypes.data, None) == -1
    assert rows(h, 0, m, None, None) == -1 and out.tobytes() == b"\x07" * (32 * m * m)
    assert rows(h, 1, 2, out.ctypes.data, ctypes.byref(ms)) == 0 and ms.value == 0
    assert out[:2].tobytes() == bytes(32 * m * 2) and out[2:].tobytes() == b"\x07" * (32 * m * 3)
    sel = lambda first, count, t, cap, p, f: select(h, first, count, 0, t, cap, p, f, None)  # noqa: E731
    fp = ctypes.byref(found)
    assert sel(0, 0, T, 8, pairs.ctypes.data, fp) == -1 and sel(1, m, T, 8, pairs.ctypes.data, fp) == -1 and sel(m, 1, T, 8, pairs.ctypes.data, fp) == -1
    assert sel(0, m, T, 8, None, fp) == -1 and sel(0, m, T, 8, pairs.ctypes.data, None) == -1
    for bad in (math.nan, math.inf, -math.inf):
        assert sel(0, m, bad, 8, pairs.ctypes.data, fp) == -1
    found.value = 9
    assert sel(0, m, -1.0, 8, pairs.ctypes.data, fp) == 0 and found.value == 0 and sel(0, m, 0.0, 0, None, fp) == 0
    assert pairs.tobytes() == b"\x07" * (40 * 8)
    close(h)
    assert opn(0, None, 0, n, 0, 1, 8, 0, None, None, ctypes.byref(h)) == 0 and h.value                        # no site
    assert rows(h, 0, 0, out.ctypes.data, None) == -1 and rows(h, 0, 1, out.ctypes.data, None) == -1
    assert sel(0, 1, T, 8, pairs.ctypes.data, fp) == -1
    close(h)
    close(None)


def test_the_model_is_the_contract_sample_by_sample():
    """Model (matrix products, what the GPU tests compare with) against scalar_records() (the header's text, one sample and one
    site pair at a time) on edge cells: 70 samples x 9 sites at three (min_cov, min_depth) and at D = 0xFFFFFFFF; the transpose
    rule; the diagonal; every class occurs."""
    rng = np.random.default_rng(80)
    for c, depth in ((0, 0), (1, 8), (5, 1), (1, 0xFFFFFFFF)):
        db = edge_cells(rng, 70, 9, c, depth)
        mod = Model(db, c, depth)
        want = scalar_records(db.tolist(), c, depth)
        got = [[[int(mod.rec[s, t][f]) for f in FIELDS] for t in range(9)] for s in range(9)]
        assert got == want, (c, depth)
        tr = mod.rec.T
        for f, g in zip(FIELDS, ("n", "ht", "gt", "hs", "gs", "hh", "hg", "gg")):
            assert np.array_equal(mod.rec[f], tr[g]), f
        d = np.arange(9)
        diag = mod.rec[d, d]
        assert np.array_equal(diag["n"], mod.site_geno[:, 2]) and np.array_equal(diag["hs"], mod.site_geno[:, 0]) and np.array_equal(diag["gg"], mod.site_geno[:, 1])
        assert np.array_equal(diag["hh"], diag["hs"]) and not diag["hg"].any()
        assert (mod.site_geno.sum(0)[[0, 2]] > 0).all() and int(mod.rec["hg"].sum()) > 0 if depth != 0xFFFFFFFF else True


def test_fixture_premise_on_the_model_alone(fixture_model):
    """A condition on the input, checked without the code under test: under the defaults the LD fixture selects at least 20
    pairs, leaves at least 20 defined pairs unselected, has a selected pair of each dir, and the prune drops at least 5 and
    keeps at least 5 sites; its monomorphic and its never-called site have no defined pair and are kept."""
    db, mod = fixture_model
    assert db.shape == (200, 300, 2)
    sel = mod.pairs()
    every = mod.pairs(0.0)
    assert len(sel) >= 20 and len(every) - len(sel) >= 20
    dirs = [moments(p["rec"])[1] > 0 for p in sel]
    assert any(dirs) and not all(dirs)
    kept = prune(sel, mod.m)
    assert kept.count(False) >= 5 and kept.count(True) >= 5
    mono, never = 49 * 6, 49 * 6 + 1
    assert mod.site_geno[never].tolist() == [0, 0, 0, 0] and mod.site_geno[mono][:3].tolist()[:2] == [0, 0] and mod.site_geno[mono][2] > 150
    assert not any(int(p["a"]) in (mono, never) or int(p["b"]) in (mono, never) for p in every) and kept[mono] and kept[never]
    assert all(0.0 <= r2_of(p["rec"]) <= 1.0 for p in every)


def test_r2_rows_and_prune_through_the_host_library():
    """eval_ld.hpp through libntsm_host.so against the Python expressions on given records: n == M (defined) and M - 1 (not),
    vx == 0, two identical sites (r2 exactly 1.0; T = nextafter(1.0, 2) selects nothing), T equal to one pair's own r2
    (selected) and nextafter above it (not), a pair with cov < 0, thirds (digits that round); the rows' text; prune chains: a-b
    and b-c selected but a-c not keeps a and c."""
    import ntsm_amd.eval as ev
    x = [0, 1, 2, 1, 0, 2, 1, 1, 0, 2] * 2                                                   # 20 samples
    flip = [2 - v for v in x]
    some = [0, 1, 2, 2, 0, 1, 1, 0, 0, 2] * 2
    third = [0, 0, 1] * 6 + [2, 1]
    cases = {"same": rec_from(x, x), "short": rec_from(x[:19], x[:19]), "flat": rec_from([1] * 20, x), "inverse": rec_from(x, flip), "some": rec_from(x, some),
             "third": rec_from(x, third), "gaps": rec_from([None] + x[1:], x[:-1] + [None])}
    for name, r in cases.items():
        mom, r2 = ev.ld_r2(r, M)
        assert mom == moments(r) and r2 == r2_of(r), name
    assert ev.ld_r2(cases["same"])[1] == 1.0 and ev.ld_r2(cases["inverse"])[1] == 1.0 and moments(cases["inverse"])[1] < 0
    assert int(cases["same"]["n"]) == M and ev.ld_r2(cases["short"])[1] is None and ev.ld_r2(cases["short"], 19)[1] == 1.0
    assert moments(cases["flat"])[2] == 0 and ev.ld_r2(cases["flat"])[1] is None and ev.ld_r2(cases["gaps"])[1] is None and ev.ld_r2(cases["gaps"], 18)[1] is not None
    own = r2_of(cases["some"])
    assert 0.0 < own < 1.0 and r2_of(cases["third"]) not in (None, 0.0, 1.0)
    loci = ["rs%d" % s for s in range(6)]
    listed = [(0, 1, "same"), (0, 2, "inverse"), (1, 2, "some"), (2, 5, "third"), (3, 4, "same")]
    pairs = np.array([(a, b, cases[k]) for a, b, k in listed], dtype=PAIR)
    text = ev.ld_rows_text(loci, pairs)
    assert text == "".join(line(loci, p) for p in pairs).encode()
    assert text.split(b"\n")[0] == b"rs0\trs1\t20\t1.000000\t+" and text.split(b"\n")[1] == b"rs0\trs2\t20\t1.000000\t-"
    assert ev.ld_rows_text(loci, pairs[:0]) == b""
    with pytest.raises(RuntimeError, match="failed: -1"):
        ev.ld_rows_text(loci[:5], pairs)
    # the prune: selection is r2 >= T on a defined r2, evaluated from the record
    up = math.nextafter(1.0, 2.0)
    assert ev.ld_prune(6, pairs, M, up).all()                                                # nothing is selected above 1.0
    assert ev.ld_prune(6, pairs, M, 1.0).tolist() == [True, False, False, True, False, True]
    assert ev.ld_prune(6, pairs, M, own).tolist() == [True, False, False, True, False, True]
    chain = np.array([(0, 1, cases["some"]), (1, 2, cases["some"])], dtype=PAIR)               # a-b and b-c, not a-c
    assert ev.ld_prune(3, chain, M, own).tolist() == [True, False, True] == prune(chain, 3)
    assert ev.ld_prune(3, chain, M, math.nextafter(own, 2.0)).all()                          # just above the pair's own r2: not selected
    assert ev.ld_prune(3, chain, M + 1, own).all()                                           # n == M is defined, M + 1 is not
    fan = np.array([(0, 1, cases["same"]), (0, 2, cases["same"]), (1, 3, cases["same"]), (2, 3, cases["same"]), (3, 4, cases["same"])], dtype=PAIR)
    assert ev.ld_prune(5, fan).tolist() == [True, False, False, True, False] == prune(fan, 5)   # 3 pairs only with dropped sites: kept, and drops 4
    assert ev.ld_prune(0, fan[:0]).tolist() == [] and ev.ld_prune(4, fan[:0]).all()


def test_band_walk_against_brute_force():
    """eval_ld.hpp's walk over a model device that selects a given number of pairs per row, against walk() above: the capacity is
    the budget, never below n_sites; everything in one call where it fits; a call beyond the capacity is halved and run again,
    down to one row; the bands partition the rows in order; random rows and budgets."""
    import ntsm_amd.eval as ev
    assert ev.ld_bands([3, 0, 2, 1], 6) == ([(0, 4, 0)], (1, 0, 6))
    assert ev.ld_bands([3, 0, 2, 1], 5) == ([(0, 4, 1), (0, 2, 0), (2, 2, 0)], (2, 1, 6))
    assert ev.ld_bands([3, 0, 2, 1], 0) == ([(0, 4, 1), (0, 2, 0), (2, 2, 0)], (2, 1, 6))      # the budget is raised to n_sites = 4
    assert ev.ld_bands([5, 4, 3, 2, 1, 0], 6) == ([(0, 6, 1), (0, 3, 1), (0, 1, 0), (1, 1, 0), (2, 1, 0), (3, 1, 0), (4, 1, 0), (5, 1, 0)], (6, 2, 15))
    assert ev.ld_bands([], 5) == ([], (0, 0, 0)) and ev.ld_bands([0], 0) == ([(0, 1, 0)], (1, 0, 0))
    rng = np.random.default_rng(81)
    for _ in range(200):
        n = int(rng.integers(1, 40))
        rp = [int(rng.integers(0, n - a)) if n - a > 1 else 0 for a in range(n)]                # at most the pairs a < b of the row
        budget = int(rng.integers(0, 3 * n))
        calls, (bands, reruns, pairs) = ev.ld_bands(rp, budget)
        assert calls == walk(rp, budget), (rp, budget)
        done = [c for c in calls if c[2] == 0]
        assert bands == len(done) and reruns == len(calls) - len(done) and pairs == sum(rp)
        assert [c[0] for c in done] == [sum(d[1] for d in done[:i]) for i in range(len(done))] and sum(d[1] for d in done) == n


def test_host_side_under_the_host_sanitizers():
    """`make ld_check`: tools/eval_ld_check.cpp -- eval_ld.hpp's moments, band walk, row text and prune over a CPU model of the
    device -- built with -fsanitize=address,undefined as a program of its own, run once by the target and once here for its
    lines."""
    subprocess.run(["make", "-s", "ld_check"], cwd=ROOT, check=True, stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(ROOT, "build", "eval_ld_check")], capture_output=True)
    assert p.returncode == 0 and p.stdout.endswith(b"ok\n") and b"FAILED" not in p.stdout and p.stderr == b"", (p.stdout[-600:], p.stderr[-600:])
    for part in (b"moments: ", b"bands: ", b"row text: ", b"prune: ", b"run: "):
        assert part in p.stdout


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gpu(built):
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    import ntsm_amd.eval as ev
    return ev


def same_rec(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for name in FIELDS:
        assert np.array_equal(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:5].tolist())


def same_pairs(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    assert got.tobytes() == want.tobytes(), (what, [i for i in range(len(got)) if got[i] != want[i]][:5])


SETTINGS = [(c, depth) for c in (0, 1, 5) for depth in (0, 1, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, 127, 128, 129, 257])
def test_open_and_rows_equal_the_model(gpu, m):
    """ntsm_eval_ld_open's site_geno and ntsm_eval_ld_rows' rectangle against Model, as integers.  Sites 1 ... 257 stand either
    side of the 32- and 64-site tile edges, samples 2 ... 257 either side of the 64-sample word edges; (min_cov, min_depth) in
    {0, 1, 5} x {0, 1, 8} over edge_cells, which plants distinct classes on both sides of every such edge; the pitch dense and a
    store's (a 1,056-byte head).  65 x 65 and 257 x 129 (samples x sites) take all nine settings at both pitches; every other
    shape takes three settings that between them hold every value, the pitch alternating.  The transpose rule and the diagonal
    hold on the device's own records."""
    rng = np.random.default_rng([m, 91])
    for i, n in enumerate((2, 3, 63, 64, 65, 128, 129, 257)):
        full = (n, m) in ((65, 65), (257, 129))
        for j, (c, depth) in enumerate(SETTINGS if full else [(0, 8), (1, 0), (5, 1)]):
            db = edge_cells(rng, n, m, c, depth)
            want = Model(db, c, depth)
            for head in ((0, RECORD_HEAD) if full else ((0, RECORD_HEAD)[(i + j) % 2],)):
                with gpu.Ld(gpu.Records.of(db, head), c, depth) as s:
                    rec, _ = s.rows(0, m)
                what = (n, m, c, depth, head)
                assert np.array_equal(s.site_geno, want.site_geno), (what, np.argwhere(s.site_geno != want.site_geno)[:5].tolist())
                assert s.times.chunks == 1
                same_rec(rec, want.rec, what)
                tr = rec.T
                for f, g in zip(FIELDS, ("n", "ht", "gt", "hs", "gs", "hh", "hg", "gg")):
                    assert np.array_equal(rec[f], tr[g]), (what, f)
                d = np.arange(m)
                assert np.array_equal(rec["n"][d, d], s.site_geno[:, 2]) and np.array_equal(rec["hh"][d, d], s.site_geno[:, 0]) and not rec["hg"][d, d].any()


@pytest.fixture(scope="module")
def edge257(gpu):
    """129 samples x 257 sites and 257 samples x 130 sites at min_cov 1, min_depth 8 in a store's pitch: (cells, records, model)
    once for the tests that share them.  Random cells hold no LD, so some is planted across the tile edges: site 70 is site 5's
    copy, site 129 site 31's, site 100 site 64's inverse (AT and CG swapped), and site 128 is site 2's copy in 9 of 10 samples."""
    out = []
    for seed, (n, m) in ((92, (129, 257)), (93, (257, 130))):
        db = edge_cells(np.random.default_rng(seed), n, m, 1, 8)
        db[:, 70], db[:, 129], db[:, 100] = db[:, 5], db[:, 31], db[:, 64, ::-1]
        db[np.arange(n) % 10 != 0, 128] = db[np.arange(n) % 10 != 0, 2]
        out.append((db, gpu.Records.of(db, RECORD_HEAD), Model(db, 1, 8)))
    return out


@pytest.mark.gpu
def test_bands_chunks_blocks_and_repeats_give_identical_bytes(gpu, edge257):
    """On 129 x 257: the whole rectangle in one call; bands whose first row and rows are off every tile size, whose concatenation
    equals the one call as bytes; every forced register block; two calls; site_geno NULL.  Chunks: 20 samples opened with
    db_chunk 0, 1 and 7 (a word shared by several chunks), 130 samples in chunks of 64 (a chunk ending on a word edge), 257 in
    chunks of 100 -- the same planes, hence the same bytes."""
    db, rec, want = edge257[0]
    try:
        with gpu.Ld(rec, 1, 8) as s:
            one, _ = s.rows(0, 257)
            same_rec(one, want.rec, "whole")
            bands = ((0, 1), (1, 30), (31, 33), (64, 67), (131, 126))
            for block in BLOCKS + BLOCKS[:1]:
                gpu.ld_tune(*block)
                parts = [s.rows(first, rows)[0] for first, rows in bands]
                assert b"".join(p.tobytes() for p in parts) == one.tobytes(), block
                assert s.rows(0, 257)[0].tobytes() == one.tobytes(), block
                assert s.rows(254, 3)[0].tobytes() == one[254:].tobytes(), block                  # a band that ends at n_sites
    finally:
        gpu.ld_tune(0, 0)
    with gpu.Ld(rec, 1, 8, site_geno=False) as bare:
        assert bare.site_geno is None and bare.rows(0, 257)[0].tobytes() == one.tobytes()
    for n, tries in ((20, ((0, 1), (1, 20), (7, 3), (20, 1))), (130, ((64, 3),)), (257, ((100, 3),))):
        cells = edge_cells(np.random.default_rng([n, 94]), n, 65, 1, 8)
        model = Model(cells, 1, 8)
        for chunk, chunks in tries:
            with gpu.Ld(gpu.Records.of(cells, RECORD_HEAD), 1, 8, chunk) as s:
                assert s.times.chunks == chunks and np.array_equal(s.site_geno, model.site_geno), (n, chunk)
                assert s.rows(0, 65)[0].tobytes() == model.rec.tobytes(), (n, chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("which", [0, 1])
def test_select_equals_the_filtered_sorted_model(gpu, edge257, which):
    """ntsm_eval_ld_select on 129 x 257 and 257 x 130 (samples x sites) against Model.pairs: T = 0 (every defined pair), 0.5 and
    1.0 at M = 20 and M = 100; cap exact, one short (return 1, the true n_found) and 0; bands off the tile size whose
    concatenation is the whole; every forced register block; two calls give identical bytes."""
    db, rec, want = edge257[which]
    m = want.m
    try:
        with gpu.Ld(rec, 1, 8) as s:
            for t, called in ((0.0, M), (0.5, M), (1.0, M), (0.5, 100)):
                expect = want.pairs(t, called)
                rc, got, found, _ = s.select(0, m, called, t)
                assert rc == 0 and found == len(expect), (t, called, found, len(expect))
                same_pairs(got, expect, (t, called))
                if len(expect):
                    rc, got, found, _ = s.select(0, m, called, t, cap=len(expect))
                    assert rc == 0 and found == len(expect) and got.tobytes() == expect.tobytes()
                    rc, got, found, _ = s.select(0, m, called, t, cap=len(expect) - 1)
                    assert rc == 1 and found == len(expect) and len(got) == 0
                    rc, got, found, _ = s.select(0, m, called, t, cap=0)
                    assert rc == 1 and found == len(expect)
            expect = want.pairs(0.0, M)
            assert len(expect) > 1000 and len(want.pairs(0.5, M)) > 0
            bands = ((0, 1), (1, 30), (31, 33), (64, 67), (131, m - 131)) if m > 131 else ((0, 1), (1, 30), (31, 33), (64, m - 64))
            for block in BLOCKS + BLOCKS[:1]:
                gpu.ld_tune(*block)
                parts = [s.select(first, rows, M, 0.0) for first, rows in bands]
                assert all(p[0] == 0 for p in parts) and b"".join(p[1].tobytes() for p in parts) == expect.tobytes(), block
                for (first, rows), p in zip(bands, parts):
                    assert p[2] == len(want.pairs(0.0, M, first, rows)), (block, first)
                assert s.select(0, m, M, 0.0)[1].tobytes() == expect.tobytes(), block
                assert s.select(m - 1, 1, M, 0.0)[2] == 0                                        # the last site alone has no pair
    finally:
        gpu.ld_tune(0, 0)


@pytest.mark.gpu
def test_r2_edges_go_through_the_device(gpu):
    """The two r^2 edge cases on the device's own test: 70 samples x 40 sites in which site 1 is site 0's copy and site 2 its
    inverse (r2 exactly 1.0: selected at T = 1.0, nothing at nextafter(1.0, 2)); for a pair with 0 < r2 < 1, T equal to its own r2
    selects it and nextafter above does not; M equal to a pair's n selects it and M + 1 does not."""
    rng = np.random.default_rng(95)
    dose = rng.integers(0, 3, size=(70, 40))
    dose[:, 1] = dose[:, 0]
    dose[:, 2] = 2 - dose[:, 0]
    db = np.stack([np.where(dose < 2, 20, 0), np.where(dose > 0, 20, 0)], axis=2).astype(np.uint32)
    db[rng.random(dose.shape) < 0.05] = 0
    db[:, :3] = np.stack([np.where(dose[:, :3] < 2, 20, 0), np.where(dose[:, :3] > 0, 20, 0)], axis=2)
    want = Model(db, 1, 8)
    assert r2_of(want.rec[0, 1]) == 1.0 and r2_of(want.rec[0, 2]) == 1.0 and moments(want.rec[0, 2])[1] < 0
    own = r2_of(want.rec[5, 9])
    n59 = int(want.rec[5, 9]["n"])
    assert 0.0 < own < 1.0 and n59 < 70
    with gpu.Ld(db, 1, 8) as s:
        for t, called in ((1.0, M), (math.nextafter(1.0, 2.0), M), (own, M), (math.nextafter(own, 2.0), M), (0.0, n59), (0.0, n59 + 1)):
            rc, got, found, _ = s.select(0, 40, called, t)
            expect = want.pairs(t, called)
            assert rc == 0 and found == len(expect)
            same_pairs(got, expect, (t, called))
        ones = s.select(0, 40, M, 1.0)[1]
        assert [(int(p["a"]), int(p["b"])) for p in ones] == [(0, 1), (0, 2), (1, 2)] and s.select(0, 40, M, math.nextafter(1.0, 2.0))[2] == 0
        at = lambda t, c: {(int(p["a"]), int(p["b"])) for p in s.select(0, 40, c, t)[1]}  # noqa: E731
        assert (5, 9) in at(own, M) and (5, 9) not in at(math.nextafter(own, 2.0), M)
        assert (5, 9) in at(0.0, n59) and (5, 9) not in at(0.0, n59 + 1)


def ld(args, d, env=None):
    p = run(["--ld"] + args, d, env=env)
    assert p.returncode == 0, p.stderr[-400:]
    return p


def report(p):
    lines = [l for l in p.stderr.split(b"\n") if l.startswith(b"store ld: ")]
    assert len(lines) == 1
    return lines[0]


@pytest.mark.gpu
def test_cli_on_the_ld_fixture(gpu, tmp_path, fixture_model):
    """The LD fixture written as a store: the defaults, -a, --ld-min 0.9 --ld-called 150, and --ld-prune (also under -a, where it
    is still the prune at T), each byte for byte the model's text; -vv reports the shape of the run on one stderr line; with the
    pair budget forced small the band is halved and run again and the output is unchanged."""
    db, mod = fixture_model
    loci, _ = write_store(tmp_path / "L", db, np.random.default_rng(96))
    want = ld_text(mod, loci)
    sel = mod.pairs()
    p = ld(["L", "-v", "-v"], tmp_path)
    assert p.stdout == want and p.stdout.count(b"\n") == 1 + len(sel)
    assert b"planes %d bytes, 1 chunks, 1 bands, 0 re-runs, %d pairs, map" % (3 * 4 * 8 * 300, len(sel)) in report(p)
    assert b"plane kernel" in report(p) and b"upload" in report(p) and b"select" in report(p)
    everything = ld_text(mod, loci, all_rows=True)
    assert ld(["L", "-a"], tmp_path).stdout == everything and everything.count(b"\n") > 20000
    assert ld(["L", "--ld-min", "0.9", "--ld-called", "150"], tmp_path).stdout == ld_text(mod, loci, 0.9, 150)
    assert ld(["L", "--ld-min", "-1"], tmp_path).stdout == everything                            # r2 >= 0 wherever it is defined
    kept = "".join(l + "\n" for l, k in zip(loci, prune(sel, 300)) if k).encode()
    p = ld(["L", "--ld-prune", "kept.txt", "-v", "-v"], tmp_path)
    assert p.stdout == want and open(str(tmp_path / "kept.txt"), "rb").read() == kept and b", %d kept sites, map" % kept.count(b"\n") in report(p)
    open(str(tmp_path / "kept.txt"), "w").write("something much longer than the list\n" * 100)   # an old file is replaced, not overlaid
    assert ld(["L", "-a", "--ld-prune", "kept.txt"], tmp_path).stdout == everything and open(str(tmp_path / "kept.txt"), "rb").read() == kept
    strict = "".join(l + "\n" for l, k in zip(loci, prune(mod.pairs(0.9, 150), 300)) if k).encode()
    ld(["L", "--ld-min", "0.9", "--ld-called", "150", "--ld-prune", "strict.txt"], tmp_path)
    assert open(str(tmp_path / "strict.txt"), "rb").read() == strict != kept
    small = dict(os.environ, NTSM_LD_PAIR_BUDGET="1")                                           # raised to n_sites = 300 pairs per call
    p = ld(["L", "-a", "--ld-prune", "small.txt", "-v", "-v"], tmp_path, env=small)
    assert p.stdout == everything and open(str(tmp_path / "small.txt"), "rb").read() == kept
    calls = walk([len(mod.pairs(0.0, M, a, 1)) for a in range(300)], 1)
    done = [c for c in calls if c[2] == 0]
    assert len(calls) > len(done) > 1 and b" %d bands, %d re-runs, %d pairs" % (len(done), len(calls) - len(done), everything.count(b"\n") - 1) in report(p)


@pytest.mark.gpu
def test_cli_on_an_edge_store(gpu, tmp_path):
    """70 samples x 130 sites of edge cells, one sample empty, at -c 2 --ld-depth 3: the defaults' cuts, -a, and M = 0 under -a
    (every pair that varies at both sites), each the model's text."""
    rng = np.random.default_rng(97)
    db = edge_cells(rng, 70, 130, 2, 3)
    db[7] = 0
    loci, _ = write_store(tmp_path / "W", db, rng)
    mod = Model(db, 2, 3)
    base = ["W", "-c", "2", "--ld-depth", "3"]
    assert ld(base, tmp_path).stdout == ld_text(mod, loci)
    want = ld_text(mod, loci, all_rows=True)
    assert ld(base + ["-a"], tmp_path).stdout == want and want.count(b"\n") > 1000
    assert ld(base + ["-a", "--ld-called", "0"], tmp_path).stdout == ld_text(mod, loci, m=0, all_rows=True)
    assert ld(base + ["--ld-min", "0.05", "--ld-called", "30"], tmp_path).stdout == ld_text(mod, loci, 0.05, 30)


def stored(path):
    s = read_store(str(path))
    return s["loci"], np.stack([r["counts"] for r in s["samples"]]).reshape(s["n"], s["m"], 2)


@pytest.mark.gpu
def test_cli_on_a_packed_and_appended_store(gpu, tmp_path):
    """A store packed by --pack from six counts files (one with counts beyond 2^31, one empty) and the same files packed in two
    runs: the same stdout, the model's text over the counts and locus IDs the store holds."""
    _, files = qc_cohort(tmp_path)
    assert run(["--pack", "S2"] + files[:4], tmp_path).returncode == 0
    assert run(["--pack", "S2"] + files[4:], tmp_path).returncode == 0
    loci, db = stored(tmp_path / "S2")
    assert db.shape == (6, 130, 2)
    mod = Model(db, 1, DEPTH)
    cuts = ["-a", "--ld-called", "3"]
    a, b = ld(["S2"] + cuts, tmp_path), ld(["S"] + cuts, tmp_path)
    want = ld_text(mod, loci, m=3, all_rows=True)
    assert a.stdout == b.stdout == want and want.count(b"\n") > 1
    assert ld(["S2"], tmp_path).stdout == HEADER.encode()                                        # six samples never reach M = 20
    assert ld(["S2", "--ld-called", "3", "--ld-min", "0.8"], tmp_path).stdout == ld_text(mod, loci, 0.8, 3)


@pytest.mark.gpu
def test_cli_on_a_store_written_by_the_cohort_counter(gpu, tmp_path):
    """`ntsmCount --cohort --store` over three tiny samples: --ld of its store equals the model's text over what it holds."""
    import ntsm_amd
    d = tmp_path
    s = ntsm_amd.SynthShort(sites_seed=20261021, n_sites=200, read_seed=7, sites_path=str(d / "sites.fa"))
    s.write_fastq(str(d / "one.fq"), 0, 4000)
    s.write_fastq(str(d / "two.fq"), 4000, 5000)
    s.write_fastq(str(d / "three.fq"), 9000, 4500)
    open(str(d / "m.tsv"), "w").write("one.txt\tone.fq\ntwo.txt\ttwo.fq\nthree.txt\tthree.fq\n")
    p = subprocess.run([COUNT, "-s", "sites.fa", "--cohort", "m.tsv", "--store", "CS"], cwd=str(d), capture_output=True)
    assert p.returncode == 0, p.stderr[-400:]
    loci, db = stored(d / "CS")
    assert db.shape == (3, 200, 2) and int(db.sum()) > 0
    for c, depth in ((1, DEPTH), (0, 2)):
        mod = Model(db, c, depth)
        q = ld(["CS", "-a", "-c", c, "--ld-depth", depth, "--ld-called", "2", "--ld-prune", "kept.txt"], d)
        assert q.stdout == ld_text(mod, loci, m=2, all_rows=True)
        kept = prune(mod.pairs(T, 2), 200)
        assert open(str(d / "kept.txt"), "rb").read() == "".join(l + "\n" for l, k in zip(loci, kept) if k).encode()
