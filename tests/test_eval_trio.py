"""`ntsmEval --trios STORE`: which samples of a cohort store form a parent-parent-child trio, and do the
trios of a pedigree hold?  Device side: ntsm_eval_trio_open / _duos / _score (ntsm_amd/csrc/ntsm_eval_trio.hip): bit-planes of
genotype classes and popcounts over site words; host side: ntsm_amd/csrc/host/eval_trio.hpp.  The reference has no such run: the
oracle is Model below, an exact numpy statement of the contract in include/ntsm_eval_hip.h, itself held against a scalar
restatement of that text.

CPU, devices hidden: the surface, every refusal, the failure without a device, the bad-argument returns and empty shapes, the
table's and the pedigree's text against a Python model of their expressions, name matching, pedigree parsing, the candidate rule,
the batch cutter, and the premise of the family fixture.
GPU: the entry points against the model at the shapes where their kernels can go wrong, in bands, in chunks, under both forced
widths; the duo records against --within's tallies at D = 0; the CLI byte for byte against the model's text on the family
cohort, an edge store, a packed and appended store and one written by `ntsmCount --cohort`.
Every accumulated quantity is an integer: no comparison has a tolerance."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle_binding import ROOT
from test_eval_qc import COUNT, EVAL, HIDDEN, RECORD_HEAD, qc_cohort, run, write_store
from test_eval_store import read_store, snapshot, unchanged

HEADER = "child\tparentA\tparentB\tcalled\terrHom\terrHet\trate\tcalledA\toppA\tcalledB\toppB\n"
PED_HEADER = HEADER[:-1] + "\tverdict\n"
DUO = np.dtype([("called", "<u4"), ("opp", "<u4")])
RECORD = np.dtype([("called", "<u4"), ("err_hom", "<u4"), ("err_het", "<u4"), ("pad", "<u4")])
FULL = 0xFFFFFFFF
X, Y, M, DEPTH = 0.02, 0.02, 200, 8                                                        # the defaults of --trio-max, --trio-duo, --trio-called, --trio-depth


# ---------------------------------------------------------------------------------------------------- the models
class Model:
    """The contract of include/ntsm_eval_hip.h in numpy: boolean planes [n][m], geno [n][4], the duo rectangle, and trio()"""

    def __init__(self, db, c, depth):
        db = np.asarray(db, dtype=np.uint32)
        a, g = db[:, :, 0], db[:, :, 1]
        A, G = a > c, g > c
        deep = a.astype(np.uint64) + g.astype(np.uint64) >= np.uint64(depth)
        self.het, self.at, self.cg = A & G, A & ~G & deep, ~A & G & deep
        self.called = self.het | self.at | self.cg
        self.n, self.m = db.shape[0], db.shape[1]
        self.geno = np.stack([self.at.sum(1), self.het.sum(1), self.cg.sum(1), (~self.called).sum(1)], axis=1).astype(np.uint32).reshape(self.n, 4)
        i = lambda p: p.astype(np.int64)  # noqa: E731
        self.duo = np.zeros((self.n, self.n), dtype=DUO)
        self.duo["called"] = i(self.called) @ i(self.called).T
        self.duo["opp"] = i(self.at) @ i(self.cg).T + i(self.cg) @ i(self.at).T

    def trio(self, child, lst):
        """The records of one entry: pairs of list positions p < q, p ascending, q ascending inside p"""
        lst = np.asarray(lst, dtype=np.int64)
        out = np.zeros(len(lst) * (len(lst) - 1) // 2 if len(lst) > 1 else 0, dtype=RECORD)
        if not len(out):
            return out
        P, Q = np.triu_indices(len(lst), 1)
        K0, K1, K2, cK = self.at[child], self.het[child], self.cg[child], self.called[child]
        X0, X2, cX = self.at[lst], self.cg[lst], self.called[lst]
        cl = cK & cX[P] & cX[Q]
        out["called"] = cl.sum(1)
        out["err_hom"] = (cl & ((K0 & (X2[P] | X2[Q])) | (K2 & (X0[P] | X0[Q])))).sum(1)
        out["err_het"] = (cl & K1 & ((X0[P] & X0[Q]) | (X2[P] & X2[Q]))).sum(1)
        return out

    def score(self, children, lists):
        return np.concatenate([self.trio(k, l) for k, l in zip(children, lists)] + [np.zeros(0, dtype=RECORD)])


def scalar_model(db, c, depth):
    """The same contract one sample, one pair, one triple and one site at a time, in Python integers:
    (classes [n][m] with 0 homAT / 1 het / 2 homCG / 3 miss, duo(x, y), trio(k, x, y))"""
    def cls(a, g):
        A, G, t = a > c, g > c, a + g
        return 1 if A and G else 0 if A and not G and t >= depth else 2 if not A and G and t >= depth else 3
    k = [[cls(int(a), int(g)) for a, g in row] for row in db]

    def duo(x, y):
        called = opp = 0
        for u, v in zip(k[x], k[y]):
            if u != 3 and v != 3:
                called += 1
                opp += (u, v) in ((0, 2), (2, 0))
        return called, opp

    def trio(kid, x, y):
        called = eh = et = 0
        for ch, u, v in zip(k[kid], k[x], k[y]):
            if 3 in (ch, u, v):
                continue
            called += 1
            eh += (ch == 0 and 2 in (u, v)) or (ch == 2 and 0 in (u, v))
            et += ch == 1 and (u, v) in ((0, 0), (2, 2))
        return called, eh, et
    return k, duo, trio


def rate(r):
    """Python floats are IEEE doubles and int -> float rounds to nearest, as the C++ conversions do"""
    return float(int(r["err_hom"]) + int(r["err_het"])) / float(int(r["called"])) if int(r["called"]) else None


def printed(r, all_rows, m, x):
    return all_rows or (rate(r) is not None and int(r["called"]) >= m and rate(r) <= x)


def verdict(r, m, x):
    return "lowcov" if int(r["called"]) < m else "ok" if rate(r) is not None and rate(r) <= x else "fail"


def line(names, k, a, b, r, da, db, last=None):
    f = "NA" if rate(r) is None else "%f" % rate(r)                                         # std::to_string prints %f
    cols = [names[k], names[a], names[b]] + ["%d" % r[n] for n in ("called", "err_hom", "err_het")] + [f] + ["%d" % v for v in (da["called"], da["opp"], db["called"], db["opp"])]
    return "\t".join(cols + ([last] if last else [])) + "\n"


def candidates(row, k, m=M, y=Y):
    return [p for p in range(len(row)) if p != k and int(row[p]["called"]) and int(row[p]["called"]) >= m
            and float(int(row[p]["opp"])) / float(int(row[p]["called"])) <= y]


def search_text(model, names, all_rows=False, exhaustive=False, x=X, y=Y, m=M):
    """stdout of `ntsmEval --trios` from the model: (bytes, evaluated triples, candidate lists of the children that have two)"""
    out, triples, lists = [HEADER], 0, {}
    for k in range(model.n):
        lst = [p for p in range(model.n) if p != k] if exhaustive else candidates(model.duo[k], k, m, y)
        if len(lst) < 2:
            continue
        lists[k] = lst
        rec, at = model.trio(k, lst), 0
        triples += len(rec)
        for p in range(len(lst)):
            for q in range(p + 1, len(lst)):
                if printed(rec[at], all_rows, m, x):
                    out.append(line(names, k, lst[p], lst[q], rec[at], model.duo[k, lst[p]], model.duo[k, lst[q]]))
                at += 1
    return "".join(out).encode(), triples, lists


def ped_text(model, names, trios, x=X, m=M):
    out = [PED_HEADER]
    for k, f, mo in trios:
        r = model.trio(k, [f, mo])[0]
        out.append(line(names, k, f, mo, r, model.duo[k, f], model.duo[k, mo], verdict(r, m, x)))
    return "".join(out).encode()


def edges(n, step=64):
    """0, n - 1 and both sides of every multiple of step below n"""
    return sorted({0, n - 1} | {e for k in range(step, n + 1, step) for e in (k - 2, k - 1, k, k + 1) if 0 <= e < n})


def edge_cells(rng, n, m, c, depth):
    """[n][m][2] with every cell drawn from {0, c, c + 1, D - 1, D, 3e9, 0xFFFFFFFF}.  At the sites on both sides of every 32- and
    64-site edge, the samples on both sides of every 64-sample edge carry, rotating from site to site: (D, 0) and (D - 1, 0), (0, D)
    and (0, D - 1) -- a hom at and just below the depth --, the four cells whose counts sit at c and c + 1, (0xFFFFFFFF, 1), where
    t = 2^32 and a 32-bit sum would call it a miss, (0xFFFFFFFF, 0xFFFFFFFF), and (0xFFFFFFFE, 1) and (0xFFFFFFFE, 0), which sit at
    and just below D = 0xFFFFFFFF."""
    low = max(depth, 1) - 1
    values = sorted({0, c, c + 1, low, depth, 3000000000, FULL})
    db = rng.choice(np.array(values, dtype=np.uint32), size=(n, m, 2))
    planted = [(depth, 0), (low, 0), (0, depth), (0, low), (c, c), (c, c + 1), (c + 1, c), (c + 1, c + 1), (FULL, 1), (FULL, FULL), (FULL - 1, 1), (FULL - 1, 0),
               (c + 1, c + 1)]
    for i, s in enumerate(edges(m, 32)):
        for j, r in enumerate(edges(n)):
            db[r, s] = planted[(i + j) % len(planted)]
    return db


def child_of(rng, f, mo, m):
    pf = rng.integers(0, 2, m)
    pm = rng.integers(0, 2, m)
    return np.stack([np.where(pf, f[1], f[0]), np.where(pm, mo[1], mo[0])])


def family_cohort(seed=7, m=2000, cov=30.0, err=0.002):
    """The simulated cohort of DESIGN.md section 9.8: six unrelated founders 0 ... 5, 6 and 7 the children of 0 and 1, 8 the child
    of 6 and 2; allele frequencies uniform in [0.1, 0.9], depth Poisson(cov), reads of the AT allele binomial in its true share
    bent by the error rate."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, size=m)
    hap = list(rng.random((6, 2, m)) < p)                                                   # True = the AT allele
    hap.append(child_of(rng, hap[0], hap[1], m))
    hap.append(child_of(rng, hap[0], hap[1], m))
    hap.append(child_of(rng, hap[6], hap[2], m))
    hap = np.array(hap)
    frac = hap.sum(1) / 2.0
    frac = frac * (1 - err) + (1 - frac) * err
    depth = rng.poisson(cov, size=hap.shape[::2])
    at = rng.binomial(depth, frac)
    return np.stack([at, depth - at], axis=2).astype(np.uint32)


NAMES9 = ["cohort/run%04d.txt" % r for r in range(9)]
TRUE_TRIOS = [(6, 0, 1), (7, 0, 1), (8, 2, 6)]


# ---------------------------------------------------------------------------------------------------- CPU
def test_surface():
    """The five entry points are exported and declared, the records are 8 and 16 bytes here and in the binding, the host
    functions are exported by libntsm_host.so, and the help text names the flags under "This build only" and says what the
    defaults are."""
    lib = ctypes.CDLL(os.path.join(ROOT, "ntsm_amd", "libntsm_eval_hip.so"))
    hdr = open(os.path.join(ROOT, "include", "ntsm_eval_hip.h")).read()
    for name in ("ntsm_eval_trio_open", "ntsm_eval_trio_duos", "ntsm_eval_trio_score", "ntsm_eval_trio_close", "ntsm_eval_trio_tune"):
        assert hasattr(lib, name) and name + "(" in hdr, name
    assert "typedef struct ntsm_eval_trio_duo { uint32_t called, opp; } ntsm_eval_trio_duo;" in hdr
    assert "typedef struct ntsm_eval_trio_record { uint32_t called, err_hom, err_het, pad /* 0 */; } ntsm_eval_trio_record;" in hdr
    assert DUO.itemsize == 8 and RECORD.itemsize == 16
    import ntsm_amd.eval as ev
    assert ev.TRIO_DUO == DUO and ev.TRIO_RECORD == RECORD
    for f in (ev.Trio, ev.trio_tune, ev.trio_rows_text, ev.trio_ped_parse, ev.trio_match, ev.trio_candidates, ev.trio_batches):
        assert callable(f)
    assert ev.lib.ntsm_eval_trio_tune(128) == -1 and ev.lib.ntsm_eval_trio_tune(1) == -1 and ev.lib.ntsm_eval_trio_tune(0) == 0
    p = subprocess.run([EVAL, "--help"], capture_output=True, env=HIDDEN)
    assert p.returncode == 0 and p.stdout == b""
    ours = p.stderr.split(b"This build only")[1]
    for flag in (b"--trios = STORE", b"--trio-depth = INT", b"--trio-max = FLOAT", b"--trio-duo = FLOAT", b"--trio-called = INT", b"--trio-exhaustive", b"--ped = FILE"):
        assert flag in ours, flag
    assert ours.count(b"[0.020000]") == 2 and b"[200]" in ours and ours.count(b"[8]") == 2 and b"conventions" in ours
    assert ours.count(b"not from real data") == 2
    assert b"--contam = STORE" in ours and b"--qc = STORE" in ours                               # and what was there is


def test_refusals(tmp_path):
    """Every refusal of --trios and its flags: exit 1, its own 'Error:' sentence, nothing on stdout, no GPU work (devices are
    hidden), the store -- bytes and mtime -- as it was."""
    rng = np.random.default_rng(5)
    db = rng.integers(0, 30, size=(4, 40, 2)).astype(np.uint32)
    write_store(tmp_path / "S", db, rng)
    write_store(tmp_path / "two", db[:2], rng)
    write_store(tmp_path / "empty", db[:0], rng)
    good = open(str(tmp_path / "S"), "rb").read()
    open(str(tmp_path / "trunc"), "wb").write(good[:-1])
    open(str(tmp_path / "magic"), "wb").write(b"NTSMCOH2" + good[8:])
    open(str(tmp_path / "q.txt"), "w").write("#@TK\t5\n#@KS\t19\nrs1\t1\t2\t1\t2\t1\t1\n")
    open(str(tmp_path / "rot.tsv"), "w").write("x\n")
    open(str(tmp_path / "norm.txt"), "w").write("0\n")
    os.mkdir(str(tmp_path / "dir"))
    open(str(tmp_path / "ok.ped"), "w").write("F run0002 run0000 run0001 0 0\n")
    open(str(tmp_path / "unknown.ped"), "w").write("F run0002 run0000 nobody 0 0\n")
    open(str(tmp_path / "own.ped"), "w").write("F run0002 run0002.txt run0001 0 0\n")
    open(str(tmp_path / "short.ped"), "w").write("F run0002 run0000\n")
    # a second store whose samples 0 and 1 share a basename
    names = ["a/x.txt", "b/x.txt", "c/y.txt"]
    from test_eval_qc import store_bytes
    total = db[:3].astype(np.uint64).sum(axis=(1, 2))
    open(str(tmp_path / "twins"), "wb").write(store_bytes(db[:3], ["rs%d" % s for s in range(40)], names, total, total, np.full(3, 19), np.ones((40, 2))))
    open(str(tmp_path / "twins.ped"), "w").write("F y x.txt c/y.txt 0 0\n")
    own = b"--trios looks for parent-child trios in one store and is a run of its own"
    flags = b"belong to --trios: give them with --trios STORE"
    cases = [
        (["--trios", "S", "--pack", "S", "q.txt"], "S", own),                                # with any other store run
        (["--trios", "S", "--against", "S", "q.txt"], "S", own),
        (["--trios", "S", "--index", "S", "-p", "rot.tsv", "-n", "norm.txt"], "S", own),
        (["--trios", "S", "--near", "S", "q.txt"], "S", own),
        (["--trios", "S", "--within", "S"], "S", own),
        (["--trios", "S", "--within-near", "S"], "S", own),
        (["--trios", "S", "--between", "S", "S"], "S", own),
        (["--between-near", "S", "--trios", "S", "S"], "S", own),
        (["--qc", "S", "--trios", "S"], "S", own),
        (["--contam", "S", "--trios", "S"], "S", own),
        (["--trio-depth", "4", "--within", "S"], "S", flags),                                # its flags without it
        (["--trio-max", "0.1", "--qc", "S"], "S", flags),
        (["--trio-duo", "0.1", "q.txt"], "S", flags),
        (["--trio-called", "2", "--contam", "S"], "S", flags),
        (["--trio-exhaustive", "--within", "S"], "S", flags),
        (["--ped", "ok.ped", "--within", "S"], "S", flags),
        (["--ped", "ok.ped", "q.txt"], "S", flags),
        (["--trios", "S", "q.txt"], "S", b"--trios takes no input files"),
        (["--trios", "S", "-p", "rot.tsv", "-n", "norm.txt"], "S", b"--trios reads allele counts, not projections, and takes no -p and no -n"),
        (["--trios", "S", "-p", "rot.tsv"], "S", b"takes no -p and no -n"),
        (["--trios", "S", "-n", "norm.txt"], "S", b"takes no -p and no -n"),
        (["--trios", "S", "-b", "truth.tsv"], "S", b"-b with --trios is not part of this build"),
        (["--trios", "S", "-e", "merged.txt"], "S", b"merging (-e, -o) with --trios is not part of this build"),
        (["--trios", "S", "-o"], "S", b"merging (-e, -o) with --trios is not part of this build"),
        (["--trios", "S", "--ped", "ok.ped", "--trio-exhaustive"], "S", b"it does not go with --trio-exhaustive"),
        (["--trios", "S", "--ped", "ok.ped", "-a"], "S", b"it does not go with -a"),
        (["--trios", "trunc"], "trunc", b"its header describes"),                            # an invalid store
        (["--trios", "magic"], "magic", b"not a cohort store"),
        (["--trios", "nowhere"], "S", b"cannot open store nowhere"),
        (["--trios", "empty"], "empty", b"empty holds no samples"),
        (["--trios", "two"], "two", b"two holds fewer than 3 samples"),
        (["--trios", "S", "--trio-max", "half"], "S", b"--trio-max takes a number, not half"),
        (["--trios", "S", "--trio-max", "0.5x"], "S", b"--trio-max takes a number, not 0.5x"),
        (["--trios", "S", "--trio-duo", "1e"], "S", b"--trio-duo takes a number, not 1e"),
        (["--trios", "S", "--trio-duo", ""], "S", b"--trio-duo takes a number, not "),
        (["--trios", "S", "--trio-duo", "nan"], "S", b"--trio-duo takes a number, not nan"),   # not finite: every comparison would be false
        (["--trios", "S", "--trio-max", "inf"], "S", b"--trio-max takes a number, not inf"),
        (["--trios", "S", "--trio-max", "-inf"], "S", b"--trio-max takes a number, not -inf"),
        (["--trios", "S", "--trio-depth", "-1"], "S", b"--trio-depth takes a number of reads, not -1"),
        (["--trios", "S", "--trio-depth", "4294967296"], "S", b"--trio-depth takes a number of reads, not 4294967296"),
        (["--trios", "S", "--trio-called", "two"], "S", b"--trio-called takes a number of sites, not two"),
        (["--trios", "S", "--ped", "nowhere.ped"], "S", b"cannot read the pedigree file nowhere.ped"),   # an unreadable PED
        (["--trios", "S", "--ped", "dir"], "S", b"cannot read the pedigree file dir"),
        (["--trios", "S", "--ped", "short.ped"], "S", b"line 1 of the pedigree file has fewer than four columns"),
        (["--trios", "S", "--ped", "unknown.ped"], "S", b"the pedigree names nobody, which matches no sample of the store"),
        (["--trios", "twins", "--ped", "twins.ped"], "twins", b"the pedigree names x.txt, which matches more than one sample of the store"),
        (["--trios", "S", "--ped", "own.ped"], "S", b"the pedigree names run0002 as its own parent"),
        (["--trios", "S", "--samples-out", "samples.tsv"], "S", b"--samples-out is the per-sample table of --contam"),
        (["--trios", "S", "--sites-out", "sites.tsv"], "S", b"--sites-out is the per-site table of --qc"),
        (["--trios", "S", "--within-rows", "3"], "S", b"--within-rows sets the bands of --within"),
        (["--trios", "S", "--between-rows", "3"], "S", b"--between-rows sets the bands of --between"),
    ]
    for args, touched, sentence in cases:
        path = str(tmp_path / touched)
        before = snapshot(path)
        p = run(args, tmp_path, env=HIDDEN)
        assert p.returncode == 1 and p.stdout == b"", (args, p.returncode, p.stdout[:100], p.stderr[-300:])
        errors = [l for l in p.stderr.split(b"\n") if l.startswith(b"Error: ")]
        assert len(errors) == 1 and sentence in errors[0], (args, p.stderr)
        assert unchanged(path, before), args
        for left in ("samples.tsv", "sites.tsv", "merged.txt", touched + ".pcaidx", touched + ".tmp"):
            assert not os.path.exists(str(tmp_path / left)), (args, left)
    # the sentences the other runs always had
    p = run(["--qc", "S", "--contam", "S"], tmp_path, env=HIDDEN)
    assert p.returncode == 1 and b"--contam checks one store for cross-sample contamination and is a run of its own" in p.stderr
    p = run(["--within", "S", "--pack", "S"], tmp_path, env=HIDDEN)
    assert p.returncode == 1 and b"are seven runs: give one of them" in p.stderr


def test_trios_without_a_device_fails_and_prints_nothing(tmp_path):
    """A valid --trios where no device can be opened: the GPU failure message, exit 3, no header on stdout, the store as it was."""
    rng = np.random.default_rng(6)
    write_store(tmp_path / "S", rng.integers(0, 30, size=(4, 40, 2)).astype(np.uint32), rng)
    open(str(tmp_path / "ok.ped"), "w").write("# a comment\nF run0002 cohort/run0000.txt run0001.txt 0 0\nF run0000 0 0 0 0\n")
    before = snapshot(str(tmp_path / "S"))
    for args in ([], ["-a", "-c", "0", "--trio-depth", "0", "--trio-max", "-1", "--trio-duo", "1e-3", "--trio-called", "0", "-v", "-v"], ["--trio-exhaustive"],
                 ["--ped", "ok.ped", "-v"]):
        p = run(["--trios", "S"] + args, tmp_path, env=HIDDEN)
        assert p.returncode == 3 and p.stdout == b"", (args, p.returncode, p.stdout[:100], p.stderr[-300:])
        assert b"on the GPU failed" in p.stderr and b"there is no CPU path" in p.stderr, (args, p.stderr)
        assert unchanged(str(tmp_path / "S"), before)
    assert b"Read 1 trios from ok.ped; skipped 1 comment lines and 1 lines without both parents" in p.stderr


def test_bad_arguments_and_empty_shapes_need_no_device():
    """-1 before any HIP call: open with a stride below 8 * n_sites, one that is no multiple of 4, counts NULL, the handle's place
    NULL; duos with a range past n_db, no rows, out NULL, the handle NULL; score with an index >= n_db, a candidate equal to its
    entry's child, a decreasing offset, offset[0] != 0, a NULL it needs.  A store without sites gives zeroed outputs, one without
    samples has no range to take, lists of 0 or 1 give no records, n_children == 0 returns 0 -- none touches a device."""
    import ntsm_amd.eval as ev
    opn, duos, score, close = ev.lib.ntsm_eval_trio_open, ev.lib.ntsm_eval_trio_duos, ev.lib.ntsm_eval_trio_score, ev.lib.ntsm_eval_trio_close
    m, n = 5, 4
    db = np.ones((n, m, 2), dtype=np.uint32)
    h = ctypes.c_void_p(1)
    assert opn(0, db.ctypes.data, 8 * m - 8, n, m, 1, 8, 0, None, None, ctypes.byref(h)) == -1 and h.value is None
    assert opn(0, db.ctypes.data, 8 * m - 4, n, m, 1, 8, 0, None, None, ctypes.byref(h)) == -1
    assert opn(0, db.ctypes.data, 8 * m + 2, n, m, 1, 8, 0, None, None, ctypes.byref(h)) == -1
    assert opn(0, None, 8 * m, n, m, 1, 8, 0, None, None, ctypes.byref(h)) == -1
    assert opn(0, db.ctypes.data, 8 * m, n, m, 1, 8, 0, None, None, None) == -1
    out = np.frombuffer(b"\x07" * (8 * n * n), dtype=DUO).copy().reshape(n, n)
    assert duos(None, 0, 1, out.ctypes.data, None) == -1
    geno = np.full((n, 4), 7, np.uint32)
    times = ev.CrossTimes(1.0, 1.0, 1.0, 1.0, 9)
    assert opn(0, db.ctypes.data, 0, n, 0, 1, 8, 0, geno.ctypes.data, ctypes.byref(times), ctypes.byref(h)) == 0 and h.value   # no site: a session without device work
    assert not geno.any() and times.chunks == 0 and times.upload_ms == 0
    assert duos(h, 0, 0, out.ctypes.data, None) == -1 and duos(h, 1, n, out.ctypes.data, None) == -1 and duos(h, n, 1, out.ctypes.data, None) == -1
    assert duos(h, 0, n, None, None) == -1 and out.tobytes() == b"\x07" * (8 * n * n)
    ms = ctypes.c_double(5.0)
    assert duos(h, 1, 2, out.ctypes.data, ctypes.byref(ms)) == 0 and ms.value == 0
    assert out[:2].tobytes() == bytes(8 * n * 2) and out[2:].tobytes() == b"\x07" * (8 * n * 2)

    def sc(child, offset, cand, rec, n_children=None):
        child, offset, cand = np.array(child, np.uint32), np.array(offset, np.uint64), np.array(cand, np.uint32)
        return score(h, child.ctypes.data, offset.ctypes.data, cand.ctypes.data, len(child) if n_children is None else n_children,
                     None if rec is None else rec.ctypes.data, None)
    rec = np.frombuffer(b"\x07" * (16 * 8), dtype=RECORD).copy()
    assert sc([0], [0, 3], [1, 2, 4], rec) == -1                                              # a candidate >= n_db
    assert sc([4], [0, 2], [1, 2], rec) == -1                                                 # a child >= n_db
    assert sc([4], [0, 0], [], rec) == -1                                                     # ... of an empty list too
    assert sc([1], [0, 3], [0, 1, 2], rec) == -1                                              # a candidate that is the child
    assert sc([0, 1], [0, 3, 2], [1, 2, 3], rec) == -1                                        # a decreasing offset
    assert sc([0], [1, 3], [1, 2, 3], rec) == -1                                              # offset[0] != 0
    assert sc([0], [0, 2], [1, 2], None) == -1                                                # records and nowhere to put them
    assert score(h, None, None, None, 1, rec.ctypes.data, None) == -1 and score(None, None, None, None, 0, None, None) == -1
    assert rec.tobytes() == b"\x07" * (16 * 8)
    assert score(h, None, None, None, 0, None, None) == 0                                     # nothing to do
    assert sc([0, 1, 2], [0, 0, 1, 1], [3], None) == 0 and rec.tobytes() == b"\x07" * (16 * 8)    # lists of 0, 1 and 0: no records
    assert sc([0, 3, 0], [0, 3, 5, 7], [1, 2, 3, 0, 0, 2, 1], rec) == 0                       # 3 + 1 + 1 records of a store without sites: zeros
    assert rec[:5].tobytes() == bytes(16 * 5) and rec[5:].tobytes() == b"\x07" * (16 * 3)
    close(h)
    assert opn(0, None, 8 * m, 0, m, 1, 8, 0, None, None, ctypes.byref(h)) == 0 and h.value                 # no sample
    assert duos(h, 0, 0, out.ctypes.data, None) == -1 and duos(h, 0, 1, out.ctypes.data, None) == -1
    assert sc([0], [0, 0], [], rec) == -1 and score(h, None, None, None, 0, None, None) == 0
    close(h)
    close(None)


def test_the_model_is_the_contract_site_by_site():
    """Model (vectorised, what the GPU tests compare with) against scalar_model() (the header's text, one triple and one site at
    a time) on edge cells: 7 samples x 70 sites at three (min_cov, min_depth) and at D = 0xFFFFFFFF: the classes, every duo, and
    every triple of every child's exhaustive list."""
    rng = np.random.default_rng(80)
    for c, depth in ((0, 0), (1, 8), (5, 1), (1, FULL)):
        db = edge_cells(rng, 7, 70, c, depth)
        mod = Model(db, c, depth)
        cls, duo, trio = scalar_model(db.tolist(), c, depth)
        assert mod.geno.tolist() == [[row.count(k) for k in range(4)] for row in cls]
        assert [[(int(mod.duo[x, y]["called"]), int(mod.duo[x, y]["opp"])) for y in range(7)] for x in range(7)] == [[duo(x, y) for y in range(7)] for x in range(7)]
        for k in range(7):
            lst = [p for p in range(7) if p != k]
            got = mod.trio(k, lst)
            want = [trio(k, lst[p], lst[q]) for p in range(6) for q in range(p + 1, 6)]
            assert [(int(r["called"]), int(r["err_hom"]), int(r["err_het"])) for r in got] == want and not got["pad"].any()
        rec = mod.score(range(7), [[p for p in range(7) if p != k] for k in range(7)])
        assert (mod.geno[:, :3] > 0).all() and int(mod.duo["opp"].sum()) > 0                 # every class occurs
        if depth != FULL:
            assert int(rec["err_hom"].sum()) > 0 and int(rec["err_het"].sum()) > 0
    assert np.array_equal(mod.geno.sum(1), np.full(7, 70))
    cell = Model(np.array([[[FULL, 1], [FULL - 1, 1], [FULL - 1, 0], [FULL, FULL]]], dtype=np.uint32), 1, FULL)   # t = 2^32, t = D, t = D - 1, a het
    assert cell.at[0].tolist() == [True, True, False, False] and cell.het[0].tolist() == [False, False, False, True] and cell.geno[0].tolist() == [2, 1, 0, 1]


def test_family_premise_on_the_model_alone():
    """A condition on the input, checked without the code under test: in the simulated family (default_rng(7); 9 samples x 2,000
    sites, 30x, 0.2 % error) the model under the defaults prints exactly the three true trios, by candidates and exhaustively, with
    these counts; the candidate lists are these; 12 triples against 252; the lowest other triple is (6; 0, 8) at 0.053; and at 10x
    the same three rows with these counts, the lowest other at 0.054."""
    mod = Model(family_cohort(), 1, DEPTH)
    text, triples, lists = search_text(mod, NAMES9)
    rows = [l.split("\t") for l in text.decode().split("\n")[1:-1]]
    assert [(r[0], r[1], r[2]) for r in rows] == [tuple(NAMES9[i] for i in t) for t in TRUE_TRIOS]
    assert [[int(v) for v in r[3:6]] for r in rows] == [[2000, 0, 0], [2000, 0, 2], [2000, 0, 1]]
    assert lists == {0: [6, 7], 1: [6, 7], 6: [0, 1, 7, 8], 7: [0, 1, 6], 8: [2, 6]} and candidates(mod.duo[2], 2) == [8] and triples == 12
    sib = mod.duo[6, 7]
    assert 0.0185 < int(sib["opp"]) / int(sib["called"]) <= Y                                # the siblings' duo rate, just inside Y
    full, all_triples, _ = search_text(mod, NAMES9, exhaustive=True)
    assert full == text and all_triples == 252
    assert search_text(mod, NAMES9, all_rows=True)[0].count(b"\n") == 13 and search_text(mod, NAMES9, all_rows=True, exhaustive=True)[0].count(b"\n") == 253
    others = [(rate(r), k, lst[p], lst[q]) for k in range(9) for lst in [[s for s in range(9) if s != k]]
              for r, (p, q) in zip(mod.trio(k, lst), zip(*np.triu_indices(8, 1))) if (k, lst[p], lst[q]) not in TRUE_TRIOS]
    assert min(others)[1:] == (6, 0, 8) and 0.0525 < min(others)[0] < 0.0535
    low = Model(family_cohort(cov=10.0), 1, DEPTH)
    text, _, _ = search_text(low, NAMES9)
    rows = [l.split("\t") for l in text.decode().split("\n")[1:-1]]
    assert [(r[0], r[1], r[2]) for r in rows] == [tuple(NAMES9[i] for i in t) for t in TRUE_TRIOS]
    assert [[int(v) for v in r[3:6]] for r in rows] == [[1235, 7, 2], [1206, 12, 3], [1185, 12, 0]]
    assert search_text(low, NAMES9, exhaustive=True)[0] == text
    others = [rate(r) for k in range(9) for lst in [[s for s in range(9) if s != k]]
              for r, (p, q) in zip(low.trio(k, lst), zip(*np.triu_indices(8, 1))) if (k, lst[p], lst[q]) not in TRUE_TRIOS]
    assert 0.0535 < min(others) < 0.0545
    # why D exists: without it the true trios at 10x sit at 0.034 - 0.041, with it at no more than 0.0124 (to the digits given)
    bare = Model(family_cohort(cov=10.0), 1, 0)
    assert all(0.0335 <= rate(bare.trio(k, [a, b])[0]) < 0.0415 for k, a, b in TRUE_TRIOS) and all(rate(low.trio(k, [a, b])[0]) < 0.01245 for k, a, b in TRUE_TRIOS)


def rec_of(called, eh, et):
    r = np.zeros((), dtype=RECORD)
    r["called"], r["err_hom"], r["err_het"] = called, eh, et
    return r


def duo_of(called, opp):
    d = np.zeros((), dtype=DUO)
    d["called"], d["opp"] = called, opp
    return d


def test_row_and_ped_text_against_the_model():
    """eval_trio.hpp's lines (through libntsm_host.so) against line() on given integers: called == 0 (NA), a row exactly at
    rate == X and one exactly at called == M (printed), rows just outside (not printed), thirds (digits that round), counts near
    2^32 whose error sum passes it; under -a and under the cuts; and as --ped's lines each of the three verdicts."""
    import ntsm_amd.eval as ev
    cases = [(rec_of(0, 0, 0), False, "lowcov"), (rec_of(2000, 0, 0), True, "ok"), (rec_of(200, 3, 1), True, "ok"), (rec_of(199, 0, 0), False, "lowcov"),
             (rec_of(250, 3, 2), True, "ok"), (rec_of(249, 3, 2), False, "fail"), (rec_of(250, 6, 0), False, "fail"), (rec_of(3, 1, 0), False, "lowcov"),
             (rec_of(4000000000, 4000000000, 4000000000), False, "fail"), (rec_of(4000000000, 40000000, 40000000), True, "ok")]
    assert rate(cases[2][0]) == X and rate(cases[4][0]) == X and rate(cases[5][0]) > X and int(cases[2][0]["called"]) == M
    names = ["fam/kid%d.txt" % i for i in range(len(cases))] + ["fam/dad.txt", "fam/mum.txt"]
    dad, mum = len(cases), len(cases) + 1
    child, pa, pb = list(range(len(cases))), [dad] * len(cases), [mum] * len(cases)
    rec = np.array([c[0] for c in cases], dtype=RECORD)
    da = np.array([duo_of(2000 + i, i) for i in range(len(cases))], dtype=DUO)
    db = np.array([duo_of(FULL, FULL - i) for i in range(len(cases))], dtype=DUO)
    every = "".join(line(names, i, dad, mum, rec[i], da[i], db[i]) for i in range(len(cases))).encode()
    kept = "".join(line(names, i, dad, mum, rec[i], da[i], db[i]) for i in range(len(cases)) if cases[i][1]).encode()
    assert [printed(c[0], False, M, X) for c in cases] == [c[1] for c in cases] and [verdict(c[0], M, X) for c in cases] == [c[2] for c in cases]
    assert ev.trio_rows_text(names, child, pa, pb, rec, da, db, all_rows=True) == every
    assert ev.trio_rows_text(names, child, pa, pb, rec, da, db) == kept and kept.count(b"\n") == 4
    ped = ev.trio_rows_text(names, child, pa, pb, rec, da, db, ped=True)
    assert ped == "".join(line(names, i, dad, mum, rec[i], da[i], db[i], cases[i][2]) for i in range(len(cases))).encode()
    lines = ped.decode().split("\n")
    assert lines[0] == "fam/kid0.txt\tfam/dad.txt\tfam/mum.txt\t0\t0\t0\tNA\t2000\t0\t4294967295\t4294967295\tlowcov"
    assert lines[2] == "fam/kid2.txt\tfam/dad.txt\tfam/mum.txt\t200\t3\t1\t0.020000\t2002\t2\t4294967295\t4294967293\tok"
    assert lines[7] == "fam/kid7.txt\tfam/dad.txt\tfam/mum.txt\t3\t1\t0\t0.333333\t2007\t7\t4294967295\t4294967288\tlowcov"
    assert lines[8].split("\t")[3:7] == ["4000000000", "4000000000", "4000000000", "2.000000"] and lines[8].endswith("\tfail")
    # other cuts: M = 0 prints every row that has a rate within X; X = 1 every row with 200 sites
    assert ev.trio_rows_text(names, child, pa, pb, rec, da, db, min_called=0).count(b"\n") == 5
    assert ev.trio_rows_text(names, child, pa, pb, rec, da, db, max_rate=1.0).count(b"\n") == 6
    assert ev.trio_rows_text(names, child, pa, pb, rec, da, db, ped=True, min_called=0).decode().split("\n")[0].endswith("\tfail")
    assert ev.trio_rows_text(names, [], [], [], rec[:0], da[:0], db[:0], all_rows=True) == b""


def test_name_matching_and_pedigree_parsing():
    """An ID names the sample whose stored name, then basename, then basename without one _counts.txt / .counts.txt / .txt it
    equals: each level, an ambiguous basename, an unknown ID.  The pedigree: tabs and spaces, a comment, a 0 parent, an empty line,
    a last line without newline; a short line, an unknown ID, an ambiguous one and somebody their own parent are refused by name."""
    import ntsm_amd.eval as ev
    names = ["cohort/a.txt", "cohort/b_counts.txt", "other/b_counts.txt", "c.counts.txt", "d", "x/e.txt", "y/e.txt.txt", "b"]
    assert [ev.trio_match(names, i) for i in ("cohort/a.txt", "d", "a.txt", "c.counts.txt", "a", "c", "e", "e.txt", "b")] == [0, 4, 0, 3, 0, 3, 5, 5, 7]
    assert ev.trio_match(names, "b_counts.txt") == -2 and ev.trio_match(names, "nobody") == -1 and ev.trio_match(names, "") == -1 and ev.trio_match([], "a") == -1
    text = b"# family\tone\nF1 a d c 1 0\nF1\td\t0\t0\t1\t0\n\n  F1  c 0 gran 2 0 \r\nF2 e.txt d c.counts.txt\n#last\nF2 cohort/a.txt c d 0 0"
    assert ev.trio_ped_parse(text, names) == ([(0, 4, 3), (5, 4, 3), (0, 3, 4)], 2, 2)
    assert ev.trio_ped_parse(b"", names) == ([], 0, 0) and ev.trio_ped_parse(b"F a 0 0\n", []) == ([], 0, 1)
    for bad, sentence in ((b"F a d c\nF a d\n", "line 2 of the pedigree file has fewer than four columns"),
                          (b"F a d nobody\n", "the pedigree names nobody, which matches no sample of the store"),
                          (b"F a b_counts.txt d\n", "the pedigree names b_counts.txt, which matches more than one sample of the store"),
                          (b"F a d a.txt\n", "the pedigree names a as its own parent")):
        with pytest.raises(ValueError, match=sentence):
            ev.trio_ped_parse(bad, names)


def test_candidate_rule_and_batch_cutter():
    """A candidate is another sample with called >= M and opp / called <= Y, in store order.  Batches hold at most the limit of
    records, in order, none empty; a list that alone exceeds it is reported; the default limit is 1 GiB of 16-byte records.  The
    duo rectangle's bands are --contam's rule at 1 GiB of 8-byte records."""
    import ntsm_amd.eval as ev
    row = np.array([duo_of(*d) for d in ((200, 4), (199, 0), (5000, 0), (200, 5), (0, 0), (1000, 20), (1000, 21), (4000000000, 80000000))], dtype=DUO)
    assert ev.trio_candidates(row, 2) == [0, 5, 7] == candidates(row, 2)
    assert ev.trio_candidates(row, 0) == [2, 5, 7] and ev.trio_candidates(row, 2, 0, 1.0) == [0, 1, 3, 5, 6, 7] == candidates(row, 2, 0, 1.0)
    assert ev.trio_candidates(row[:0], 0) == []
    k = [3, 0, 2, 5, 1, 4, 4, 2]                                                              # 3, 0, 1, 10, 0, 6, 6, 1 records
    assert ev.trio_batches(k, 27) == ([8], None) and ev.trio_batches(k, 26) == ([7, 8], None) and ev.trio_batches(k, 10) == ([3, 5, 6, 8], None)
    assert ev.trio_batches(k, 9) == (None, 3) and ev.trio_batches(k[:3], 3) == ([2, 3], None) and ev.trio_batches([], 5) == ([], None)
    for limit in range(10, 30):
        ends, bad = ev.trio_batches(k, limit)
        assert bad is None and ends[-1] == 8 and all(b > a for a, b in zip([0] + ends, ends))
        assert all(sum(v * (v - 1) // 2 for v in k[a:b]) <= limit for a, b in zip([0] + ends, ends))
    assert ev.trio_batches([4, 11586, 4]) == (None, 1) and ev.trio_batches([11585, 11585]) == ([1, 2], None)
    assert ev.contam_band_rows(0, 4096, 2**27) == 4096 and ev.contam_band_rows(0, 16384, 2**27) == 8192 and ev.contam_band_rows(9000, 16384, 2**27) == 7384


def test_host_side_under_the_host_sanitizers():
    """`make trio_check`: tools/eval_trio_check.cpp -- eval_trio.hpp's candidate rule, batch cutter, pedigree parser, name matcher,
    row text and both runs over a model of the device -- built with -fsanitize=address,undefined as a program of its own, run once
    by the target and once here for its lines."""
    subprocess.run(["make", "-s", "trio_check"], cwd=ROOT, check=True, stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(ROOT, "build", "eval_trio_check")], capture_output=True)
    assert p.returncode == 0 and p.stdout.endswith(b"ok\n") and b"FAILED" not in p.stdout and p.stderr == b"", (p.stdout[-600:], p.stderr[-600:])
    for part in (b"candidates: ", b"batches: ", b"pedigree: ", b"names: ", b"row text: ", b"runs: "):
        assert part in p.stdout


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gpu(built):
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    import ntsm_amd.eval as ev
    return ev


def same_duo(got, want, what):
    for name in ("called", "opp"):
        assert np.array_equal(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:5].tolist())


def same_rec(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for name in ("called", "err_hom", "err_het", "pad"):
        assert np.array_equal(got[name], want[name]), (what, name, np.argwhere(got[name] != want[name])[:5].tolist())


SETTINGS = [(c, depth) for c in (0, 1, 5) for depth in (0, 1, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 31, 32, 33, 63, 64, 65, 130, 257])
def test_open_and_duos_equal_the_model(gpu, m):
    """ntsm_eval_trio_open's geno and ntsm_eval_trio_duos' rectangle against Model, as integers.  Sites 1 ... 257 stand either
    side of the 32- and 64-site edges of a plane word; samples 3, 4, 63, 64, 65, 130 and 257 either side of one wave of columns
    and of the builder's 64-sample tile (every launch here has one row per wave: the row groups of 2 and 4 are
    test_duo_row_groups_of_two_and_four's); (min_cov, min_depth) in {0, 1, 5} x {0, 1, 8} over edge_cells, and
    D = 0xFFFFFFFF at c = 1; the pitch dense and a store's (a 1,056-byte head).  65 x 65 and 257 x 130 take all nine settings at
    both pitches; every other shape takes three settings that between them hold every value, the pitch alternating.  geno's
    columns sum to n_sites; the rectangle is symmetric; the diagonal is the sample's called sites and no opposite."""
    rng = np.random.default_rng([m, 81])
    for i, n in enumerate((3, 4, 63, 64, 65, 130, 257)):
        full = (n, m) in ((65, 65), (257, 130))
        extra = [(1, FULL)] if n == 65 else []
        for j, (c, depth) in enumerate((SETTINGS if full else [(0, 8), (1, 0), (5, 1)]) + extra):
            db = edge_cells(rng, n, m, c, depth)
            want = Model(db, c, depth)
            for head in ((0, RECORD_HEAD) if full else ((0, RECORD_HEAD)[(i + j) % 2],)):
                with gpu.Trio(gpu.Records.of(db, head), c, depth) as s:
                    duo, _ = s.duos(0, n)
                what = (n, m, c, depth, head)
                assert np.array_equal(s.geno, want.geno), (what, np.argwhere(s.geno != want.geno)[:5].tolist())
                assert (s.geno.sum(1, dtype=np.uint64) == m).all() and s.times.chunks == 1
                same_duo(duo, want.duo, what)
                assert duo.tobytes() == duo.T.copy().tobytes()
                d = np.arange(n)
                assert np.array_equal(duo["called"][d, d], want.geno[:, :3].sum(1)) and not duo["opp"][d, d].any()


@pytest.fixture(scope="module")
def edge130(gpu):
    """130 samples x 65 sites at min_cov 1, min_depth 8 in a store's pitch: (cells, records, model) once for the tests that share it"""
    db = edge_cells(np.random.default_rng(82), 130, 65, 1, 8)
    return db, gpu.Records.of(db, RECORD_HEAD), Model(db, 1, 8)


@pytest.mark.gpu
def test_bands_chunks_widths_and_repeats_give_identical_bytes(gpu, edge130):
    """On 130 x 65: the whole rectangle in one call; the band (0, 1), a middle band and one ending at n_db, whose concatenation
    equals the one call as bytes; both forced widths; two calls; geno NULL; the store opened in chunks of 64 (of 130) -- the same
    planes, hence the same bytes.  On 20 x 65: db_chunk 0 against 1 against 7."""
    db, rec, want = edge130
    try:
        with gpu.Trio(rec, 1, 8) as s:
            one, _ = s.duos(0, 130)
            same_duo(one, want.duo, "whole")
            bands = ((0, 1), (1, 39), (40, 60), (100, 30))
            parts = [s.duos(first, rows)[0] for first, rows in bands]
            for (first, rows), part in zip(bands, parts):
                same_duo(part, want.duo[first:first + rows], first)
            assert b"".join(p.tobytes() for p in parts) == one.tobytes()
            for width in (64, 256, 0):
                gpu.trio_tune(width)
                assert s.duos(0, 130)[0].tobytes() == one.tobytes(), width
                assert s.duos(127, 3)[0].tobytes() == one[127:].tobytes(), width                  # a band that ends at n_db
            assert s.duos(0, 130)[0].tobytes() == one.tobytes()
    finally:
        gpu.trio_tune(0)
    lists = [[p for p in range(130) if p != k][:5] for k in (0, 64, 129)]
    with gpu.Trio(rec, 1, 8, geno=False) as bare, gpu.Trio(rec, 1, 8, 64) as chunked:
        assert bare.geno is None and bare.duos(0, 130)[0].tobytes() == one.tobytes()
        assert chunked.times.chunks == 3 and np.array_equal(chunked.geno, want.geno) and chunked.duos(0, 130)[0].tobytes() == one.tobytes()
        assert chunked.score([0, 64, 129], lists)[0].tobytes() == bare.score([0, 64, 129], lists)[0].tobytes() == want.score([0, 64, 129], lists).tobytes()
    small = edge_cells(np.random.default_rng(83), 20, 65, 1, 8)
    model = Model(small, 1, 8)
    for chunk, chunks in ((0, 1), (1, 20), (7, 3), (20, 1)):
        with gpu.Trio(gpu.Records.of(small, RECORD_HEAD), 1, 8, chunk) as s:
            assert s.times.chunks == chunks and np.array_equal(s.geno, model.geno) and s.duos(0, 20)[0].tobytes() == model.duo.tobytes(), chunk


@pytest.mark.gpu
@pytest.mark.parametrize("n, group", [(400, 2), (521, 4)])
def test_duo_row_groups_of_two_and_four(gpu, n, group):
    """The duo kernel's row groups, which every cohort of about 512 samples or more takes.  The launch rule takes the widest group
    t of 4, 2, 1 with ceil(n_db / 64) * ceil(n_rows / t) >= 1,024: 400 samples give 7 * 200 >= 1,024 > 7 * 100, a group of 2; 521
    give 9 * 131 >= 1,024, a group of 4.  Against Model on n x 65 edge cells: the whole rectangle; a band whose rows are no
    multiple of the group, so that its last group runs past the band, from an odd first row and ending at n_db; a band of as many
    rows from row 0; under the library's width and both forced ones (the rule's group does not depend on the width)."""
    waves = -(-n // 64)
    rule = lambda rows: next(t for t in (4, 2, 1) if t == 1 or (t // 2 < rows and waves * -(-rows // t) >= 1024))  # noqa: E731
    ragged = n - 3                                                                          # 397 = 2 * 198 + 1; 518 = 4 * 129 + 2
    assert rule(n) == group and rule(ragged) == group and ragged % group
    db = edge_cells(np.random.default_rng([n, 91]), n, 65, 1, 8)
    want = Model(db, 1, 8)
    try:
        with gpu.Trio(gpu.Records.of(db, RECORD_HEAD), 1, 8) as s:
            assert np.array_equal(s.geno, want.geno)
            for width in (0, 64, 256):
                gpu.trio_tune(width)
                one, _ = s.duos(0, n)
                same_duo(one, want.duo, (n, width, "whole"))
                same_duo(s.duos(3, ragged)[0], want.duo[3:], (n, width, "ragged to the end"))
                same_duo(s.duos(0, ragged)[0], want.duo[:ragged], (n, width, "ragged from 0"))
    finally:
        gpu.trio_tune(0)


@pytest.mark.gpu
def test_duos_at_depth_0_are_the_tallies_of_within(gpu):
    """At D = 0 the rule is calcHomHetMiss / calcRelatedness's classing: `called` and `opp` equal n_valid and ibs0 of
    ntsm_eval_within_rows on the same store, for every pair, at min_cov 0, 1 and 5."""
    rng = np.random.default_rng(84)
    for c in (0, 1, 5):
        db = edge_cells(rng, 65, 130, c, 0)
        rec = gpu.Records.of(db, RECORD_HEAD)
        with gpu.Trio(rec, c, 0) as s, gpu.Within(rec, c) as w:
            duo, _ = s.duos(0, 65)
            pairs, _, _ = w.rows(0, 65)
        i, j = np.triu_indices(65, 1)
        assert np.array_equal(duo["called"][i, j], pairs["n_valid"]) and np.array_equal(duo["opp"][i, j], pairs["ibs0"]), c
        assert int(pairs["ibs0"].sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("n, m", [(65, 130), (20, 257)])
def test_score_every_record_of_the_exhaustive_lists(gpu, n, m):
    """Every record of the exhaustive lists of every child -- 65 x 2,016 triples on 65 samples x 130 sites, 20 x 171 on 20 x 257 --
    against Model, under the library's rule and both forced widths; two calls give the same bytes."""
    db = edge_cells(np.random.default_rng([n, 85]), n, m, 1, 8)
    want = Model(db, 1, 8)
    children = list(range(n))
    lists = [[p for p in range(n) if p != k] for k in children]
    expect = want.score(children, lists)
    assert len(expect) == n * (n - 1) * (n - 2) // 2 and int(expect["err_hom"].sum()) > 0 and int(expect["err_het"].sum()) > 0
    try:
        with gpu.Trio(gpu.Records.of(db, RECORD_HEAD), 1, 8) as s:
            for width in (0, 64, 256, 0):
                gpu.trio_tune(width)
                got, _ = s.score(children, lists)
                same_rec(got, expect, (n, m, width))
    finally:
        gpu.trio_tune(0)


@pytest.mark.gpu
def test_score_list_shapes(gpu, edge130):
    """On 130 x 65: lists of 0, 1, 2, 3, 64, 65 and 129 for one child in one call -- 2,016, 2,080 and 8,256 pairs cross every edge
    of both tiles --; n_children 0 and 1; 300 entries of length 2; an unsorted list, a list that repeats a sample, a child in two
    entries; under the library's rule and both forced widths."""
    db, rec, want = edge130
    rng = np.random.default_rng(86)
    others = [p for p in range(130) if p != 7]
    shapes = [others[:k] for k in (0, 1, 2, 3, 64, 65, 129, 16, 17)]
    unsorted = [int(v) for v in rng.permutation(others)[:40]]
    repeats = [5, 9, 5, 5, 100, 9]
    twos = [[int(v) for v in rng.choice([p for p in range(130) if p != k % 130], 2, replace=False)] for k in range(300)]
    try:
        with gpu.Trio(rec, 1, 8) as s:
            for width in (0, 64, 256):
                gpu.trio_tune(width)
                got, _ = s.score([7] * len(shapes), shapes)
                same_rec(got, want.score([7] * len(shapes), shapes), ("shapes", width))
                assert len(got) == 0 + 0 + 1 + 3 + 2016 + 2080 + 8256 + 120 + 136
                assert len(s.score([], [])[0]) == 0
                same_rec(s.score([7], [others])[0], want.trio(7, others), ("one", width))
                same_rec(s.score([k % 130 for k in range(300)], twos)[0], want.score([k % 130 for k in range(300)], twos), ("twos", width))
                mixed = s.score([7, 7, 9, 7], [unsorted, repeats, others[:4], sorted(unsorted)])[0]
                same_rec(mixed, want.score([7, 7, 9, 7], [unsorted, repeats, others[:4], sorted(unsorted)]), ("mixed", width))
                again = s.score([7, 7, 9, 7], [unsorted, repeats, others[:4], sorted(unsorted)])[0]
                assert again.tobytes() == mixed.tobytes()
            with pytest.raises(RuntimeError, match="failed: -1"):
                s.score([7], [[1, 130]])
            with pytest.raises(RuntimeError, match="failed: -1"):
                s.score([7], [[1, 7]])
    finally:
        gpu.trio_tune(0)


@pytest.mark.gpu
def test_a_record_is_symmetric_in_the_parents_and_not_in_the_child(gpu):
    """On the family fixture: (6; 0, 1) equals (6; 1, 0) and differs from (0; 1, 6) and (1; 6, 0); the three true trios have the
    model's counts."""
    db = family_cohort()
    want = Model(db, 1, DEPTH)
    with gpu.Trio(db, 1, DEPTH) as s:
        got, _ = s.score([6, 6, 0, 1, 7, 8], [[0, 1], [1, 0], [1, 6], [6, 0], [0, 1], [2, 6]])
        duo, _ = s.duos(0, 9)
    same_rec(got, want.score([6, 6, 0, 1, 7, 8], [[0, 1], [1, 0], [1, 6], [6, 0], [0, 1], [2, 6]]), "family")
    same_duo(duo, want.duo, "family")
    assert got[0].tobytes() == got[1].tobytes() and got[0].tobytes() != got[2].tobytes() and got[0].tobytes() != got[3].tobytes()
    assert [(int(r["called"]), int(r["err_hom"]), int(r["err_het"])) for r in got[[0, 4, 5]]] == [(2000, 0, 0), (2000, 0, 2), (2000, 0, 1)]


def trios(args, d):
    p = run(["--trios"] + args, d)
    assert p.returncode == 0, p.stderr[-400:]
    return p


@pytest.mark.gpu
def test_cli_on_the_family_cohort(gpu, tmp_path):
    """The simulated family written as a store: under the defaults stdout is the header and the three true trios, and the same
    under --trio-exhaustive; under -a 12 rows, under -a --trio-exhaustive 252; at 10x the same three; other cut-offs; each byte for
    byte the model's text.  -vv reports the shape of the run on one stderr line."""
    db = family_cohort()
    _, names = write_store(tmp_path / "F", db, np.random.default_rng(87))
    assert names == NAMES9
    mod = Model(db, 1, DEPTH)
    want = search_text(mod, names)[0]
    p = trios(["F", "-v", "-v"], tmp_path)
    assert p.stdout == want and p.stdout.count(b"\n") == 4
    report = [l for l in p.stderr.split(b"\n") if l.startswith(b"store trios: ")]
    assert len(report) == 1 and b"planes %d bytes, 1 chunks, 1 duo bands, 5 children with 2 or more candidates, 12 triples, 3 rows" % (3 * 32 * 8 * 9) in report[0]
    assert b"plane kernel" in report[0] and b"upload" in report[0] and b"score" in report[0]
    p = trios(["F", "--trio-exhaustive", "-v", "-v"], tmp_path)
    assert p.stdout == want and b"9 children with 2 or more candidates, 252 triples, 3 rows" in p.stderr
    p = trios(["F", "-a"], tmp_path)
    assert p.stdout == search_text(mod, names, all_rows=True)[0] and p.stdout.count(b"\n") == 13
    p = trios(["F", "-a", "--trio-exhaustive"], tmp_path)
    assert p.stdout == search_text(mod, names, all_rows=True, exhaustive=True)[0] and p.stdout.count(b"\n") == 253
    mod2 = Model(db, 2, 20)
    for x, y, m in ((0.06, 0.02, 200), (0.5, 0.05, 1990), (0.0, 1.0, 0)):
        p = trios(["F", "-c", "2", "--trio-depth", "20", "--trio-max", x, "--trio-duo", y, "--trio-called", m], tmp_path)
        assert p.stdout == search_text(mod2, names, x=x, y=y, m=m)[0], (x, y, m)
    assert trios(["F", "--trio-duo", "-1"], tmp_path).stdout == HEADER.encode()                  # nobody has a candidate: the header alone
    low = family_cohort(cov=10.0)
    write_store(tmp_path / "L", low, np.random.default_rng(88))
    want = search_text(Model(low, 1, DEPTH), names)[0]
    assert trios(["L"], tmp_path).stdout == want == trios(["L", "--trio-exhaustive"], tmp_path).stdout and want.count(b"\n") == 4


@pytest.mark.gpu
def test_cli_with_a_pedigree(gpu, tmp_path):
    """--ped with the three true trios, named at each of the three levels, among a comment and founders' lines (ok); with one wrong
    line, (6; 2, 3) (fail); and on a store whose sample 5 is empty, with a line that names it (lowcov): the model's text in file
    order, exit status 0."""
    db = family_cohort()
    db[5] = 0
    _, names = write_store(tmp_path / "F", db, np.random.default_rng(89))
    mod = Model(db, 1, DEPTH)
    open(str(tmp_path / "fam.ped"), "w").write("# the family\nF run0000 0 0 1 0\nF\trun0008\trun0002.txt\tcohort/run0006.txt\t0\t0\nF run0006 run0000 run0001 2 0\n"
                                               "F run0007 run0000 run0001 1 0\nF run0006 run0002 run0003 2 0\nF run0005 run0000 run0001 0 0\nF run0001 0 run0004 0 0")
    listed = [(8, 2, 6), (6, 0, 1), (7, 0, 1), (6, 2, 3), (5, 0, 1)]
    p = trios(["F", "--ped", "fam.ped", "-v", "-v"], tmp_path)
    assert p.stdout == ped_text(mod, names, listed)
    assert [l.split(b"\t")[-1] for l in p.stdout.split(b"\n")[1:-1]] == [b"ok", b"ok", b"ok", b"fail", b"lowcov"]
    assert b"Read 5 trios from fam.ped; skipped 1 comment lines and 2 lines without both parents" in p.stderr
    assert b"4 duo bands, 5 children" in [l for l in p.stderr.split(b"\n") if l.startswith(b"store trios: ")][0]
    p = trios(["F", "--ped", "fam.ped", "--trio-max", "0.5", "--trio-called", "2001", "-c", "0", "--trio-depth", "0"], tmp_path)
    assert p.stdout == ped_text(Model(db, 0, 0), names, listed, 0.5, 2001)


@pytest.mark.gpu
def test_cli_on_an_edge_store(gpu, tmp_path):
    """70 x 65 edge cells, one sample empty, at -c 2 --trio-depth 3 -a: with the default cuts (nobody shares 200 of 65 sites: the
    header alone), with cuts that 65 sites can meet, and exhaustively -- 70 x 2,346 rows -- each the model's text."""
    rng = np.random.default_rng(90)
    db = edge_cells(rng, 70, 65, 2, 3)
    db[7] = 0
    _, names = write_store(tmp_path / "W", db, rng)
    mod = Model(db, 2, 3)
    assert trios(["W", "-c", "2", "--trio-depth", "3", "-a"], tmp_path).stdout == search_text(mod, names, all_rows=True)[0] == HEADER.encode()
    want, triples, lists = search_text(mod, names, all_rows=True, y=0.2, m=10)
    assert triples > 1000 and max(len(l) for l in lists.values()) > 16
    assert trios(["W", "-c", "2", "--trio-depth", "3", "-a", "--trio-duo", "0.2", "--trio-called", "10"], tmp_path).stdout == want
    want = search_text(mod, names, x=0.3, y=0.2, m=10)[0]
    assert trios(["W", "-c", "2", "--trio-depth", "3", "--trio-max", "0.3", "--trio-duo", "0.2", "--trio-called", "10"], tmp_path).stdout == want and want.count(b"\n") > 1
    want = search_text(mod, names, all_rows=True, exhaustive=True)[0]
    assert trios(["W", "-c", "2", "--trio-depth", "3", "-a", "--trio-exhaustive"], tmp_path).stdout == want and want.count(b"\n") == 1 + 70 * 2346
    assert (names[7] + "\t" + names[0] + "\t" + names[1] + "\t0\t0\t0\tNA\t0\t0\t0\t0\n").encode() in want


def stored(path):
    s = read_store(str(path))
    return [r["name"] for r in s["samples"]], np.stack([r["counts"] for r in s["samples"]]).reshape(s["n"], s["m"], 2)


@pytest.mark.gpu
def test_cli_on_a_packed_and_appended_store(gpu, tmp_path):
    """A store packed by --pack from six counts files (one with counts beyond 2^31, one empty) and the same files packed in two
    runs: the same stdout, the model's text over the counts and names the store holds; and a pedigree whose IDs are the files'
    stems."""
    _, files = qc_cohort(tmp_path)
    assert run(["--pack", "S2"] + files[:4], tmp_path).returncode == 0
    assert run(["--pack", "S2"] + files[4:], tmp_path).returncode == 0
    names, db = stored(tmp_path / "S2")
    assert names == files and db.shape == (6, 130, 2)
    mod = Model(db, 1, DEPTH)
    cuts = ["--trio-duo", "1", "--trio-called", "1"]
    a, b = trios(["S2", "-a"] + cuts, tmp_path), trios(["S", "-a"] + cuts, tmp_path)
    want, triples, _ = search_text(mod, names, all_rows=True, y=1.0, m=1)
    assert a.stdout == b.stdout == want and triples > 0
    assert trios(["S2", "-a", "--trio-exhaustive"], tmp_path).stdout == search_text(mod, names, all_rows=True, exhaustive=True)[0]
    assert trios(["S2"], tmp_path).stdout == search_text(mod, names)[0]
    stem = lambda f: os.path.basename(f).rsplit(".txt", 1)[0]  # noqa: E731
    open(str(tmp_path / "s.ped"), "w").write("F %s %s %s\n" % (stem(files[0]), stem(files[1]), files[2]))
    assert trios(["S2", "--ped", "s.ped"], tmp_path).stdout == ped_text(mod, names, [(0, 1, 2)])


@pytest.mark.gpu
def test_cli_on_a_store_written_by_the_cohort_counter(gpu, tmp_path):
    """`ntsmCount --cohort --store` over three tiny samples: --trios of its store equals the model's text over what it holds."""
    import ntsm_amd
    d = tmp_path
    s = ntsm_amd.SynthShort(sites_seed=20261021, n_sites=200, read_seed=7, sites_path=str(d / "sites.fa"))
    s.write_fastq(str(d / "one.fq"), 0, 4000)
    s.write_fastq(str(d / "two.fq"), 4000, 5000)
    s.write_fastq(str(d / "three.fq"), 9000, 4500)
    open(str(d / "m.tsv"), "w").write("one.txt\tone.fq\ntwo.txt\ttwo.fq\nthree.txt\tthree.fq\n")
    p = subprocess.run([COUNT, "-s", "sites.fa", "--cohort", "m.tsv", "--store", "CS"], cwd=str(d), capture_output=True)
    assert p.returncode == 0, p.stderr[-400:]
    names, db = stored(d / "CS")
    assert names == ["one.txt", "two.txt", "three.txt"] and int(db.sum()) > 0
    for c, depth in ((1, DEPTH), (0, 2)):
        mod = Model(db, c, depth)
        q = trios(["CS", "-a", "-c", c, "--trio-depth", depth, "--trio-duo", "1", "--trio-called", "1"], d)
        assert q.stdout == search_text(mod, names, all_rows=True, y=1.0, m=1)[0]
        q = trios(["CS", "-a", "-c", c, "--trio-depth", depth, "--trio-exhaustive"], d)
        assert q.stdout == search_text(mod, names, all_rows=True, exhaustive=True)[0] and q.stdout.count(b"\n") == 4
        open(str(d / "cs.ped"), "w").write("F two one three\n")
        assert trios(["CS", "--ped", "cs.ped", "-c", c, "--trio-depth", depth], d).stdout == ped_text(mod, names, [(1, 0, 2)])
