"""`ntsmEval --contam STORE`: is a sample of a cohort store a mixture, and of which other sample?  For
every ordered pair (target, source) the target's minor-allele reads and depth at its homozygous-looking sites, in three classes
by what the source carries there.  Device side: ntsm_eval_contam_open / _rows (ntsm_amd/csrc/ntsm_eval_contam.hip); host side:
ntsm_amd/csrc/host/eval_contam.hpp.  The reference has no such run: the oracle is model() below, an exact numpy statement of
the contract in include/ntsm_eval_hip.h, itself held against a scalar restatement of that text.

CPU, devices hidden: the surface, every refusal, the failure without a device, the bad-argument returns and empty shapes, both
tables' text against a Python model of their expressions, the band rule, and the premise of the mixture fixture.
GPU: the entry point against the model at the shapes where its kernel can go wrong, in bands, resident against streamed, under
every forced launch; the CLI byte for byte against the model's text on the mixture cohort, an edge store, a packed and
appended store and one written by `ntsmCount --cohort`.
Every accumulated quantity is an integer: no comparison has a tolerance."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle_binding import ROOT
from test_eval_qc import COUNT, EVAL, HIDDEN, RECORD_HEAD, qc_cohort, run, write_store
from test_eval_store import read_store, snapshot, unchanged

HEADER = "sample\tsource\tsitesLack\tsitesHet\tsitesOpp\trateLack\trateHet\trateOpp\texcess\texplained\n"
SAMPLE_HEADER = "#sample\tsites\tminorReads\tdepth\trateAll\n"
RECORD = np.dtype([("minor", "<u8", 3), ("depth", "<u8", 3), ("sites", "<u4", 3), ("pad", "<u4")])
FULL = 0xFFFFFFFF
X, Y, DEPTH = 0.01, 0.5, 8                                                                 # the defaults of --contam-min, --contam-explained, --contam-depth


# ---------------------------------------------------------------------------------------------------- the models
def model(db, c, depth):
    """ntsm_eval_contam_rows over the whole store as include/ntsm_eval_hip.h states it, in numpy: (records [n][n], tally [n][3])"""
    db = np.asarray(db, dtype=np.uint32)
    n = db.shape[0]
    a, g = db[:, :, 0].astype(np.uint64), db[:, :, 1].astype(np.uint64)
    t, mn = a + g, np.minimum(a, g)
    informative = (t >= np.uint64(depth)) & (np.uint64(4) * mn < t)
    major_at = a > g
    zero = np.uint64(0)
    tally = np.stack([informative.sum(1).astype(np.uint64), np.where(informative, mn, zero).sum(1, dtype=np.uint64),
                      np.where(informative, t, zero).sum(1, dtype=np.uint64)], axis=1).reshape(n, 3)
    rec = np.zeros((n, n), dtype=RECORD)
    for q in range(n):
        x = np.where(major_at[q], db[:, :, 1], db[:, :, 0])                                 # every source's count of q's minor allele
        y = np.where(major_at[q], db[:, :, 0], db[:, :, 1])
        carries, has_major = x > c, y > c
        for k, cls in enumerate((~carries & has_major, carries & has_major, carries & ~has_major)):
            mask = cls & informative[q]
            rec["sites"][q, :, k] = mask.sum(1)
            rec["minor"][q, :, k] = np.where(mask, mn[q], zero).sum(1, dtype=np.uint64)
            rec["depth"][q, :, k] = np.where(mask, t[q], zero).sum(1, dtype=np.uint64)
    return rec, tally


def scalar_model(db, c, depth):
    """The same contract one pair and one site at a time, in Python integers"""
    n, m = len(db), len(db[0]) if len(db) else 0
    rec = [[[[0] * 3, [0] * 3, [0] * 3] for _ in range(n)] for _ in range(n)]               # minor, depth, sites
    tally = [[0, 0, 0] for _ in range(n)]
    for q in range(n):
        for s in range(m):
            a, g = int(db[q][s][0]), int(db[q][s][1])
            t, mn = a + g, min(a, g)
            if not (t >= depth and 4 * mn < t):
                continue
            tally[q][0] += 1
            tally[q][1] += mn
            tally[q][2] += t
            for d in range(n):
                sa, sg = int(db[d][s][0]), int(db[d][s][1])
                x, y = (sg, sa) if a > g else (sa, sg)
                carries, has_major = x > c, y > c
                if not carries and not has_major:
                    continue
                k = 0 if not carries else 1 if has_major else 2
                rec[q][d][0][k] += mn
                rec[q][d][1][k] += t
                rec[q][d][2][k] += 1
    return rec, tally


def fields(r, tally):
    """The doubles of eval_contam.hpp from one record's integers: (rates [3], excess, explained), None where NA.  Python floats
    are IEEE doubles and int -> float rounds to nearest, as the C++ conversions do."""
    rate = [float(int(mn)) / float(int(dp)) if int(dp) else None for mn, dp in zip(r["minor"], r["depth"])]
    rate_all = float(int(tally[1])) / float(int(tally[2])) if int(tally[2]) else None
    excess = rate[2] - rate[0] if rate[2] is not None and rate[0] is not None else None
    explained = 1 - rate[0] / rate_all if rate[0] is not None and rate_all is not None and rate_all != 0.0 else None
    return rate, excess, explained


def rows_text(names, rec, tally, row_first=0, all_rows=False, x=X, y=Y):
    """The stdout lines (no header) of the band rec [rows][n], tally [rows][3]: std::to_string prints %f"""
    f = lambda v: "NA" if v is None else "%f" % v  # noqa: E731
    out = []
    for r in range(rec.shape[0]):
        for d in range(len(names)):
            if d == row_first + r:
                continue
            rate, excess, explained = fields(rec[r, d], tally[r])
            if not all_rows and not (excess is not None and explained is not None and excess >= x and explained >= y):
                continue
            out.append("\t".join([names[row_first + r], names[d]] + ["%d" % v for v in rec[r, d]["sites"]] + [f(v) for v in rate] + [f(excess), f(explained)])
                       + "\n")
    return "".join(out).encode()


def samples_text(names, tally):
    return (SAMPLE_HEADER + "".join("%s\t%d\t%d\t%d\t%s\n" % (name, t[0], t[1], t[2], "%f" % (float(int(t[1])) / float(int(t[2]))) if int(t[2]) else "NA")
                                    for name, t in zip(names, tally))).encode()


def edges(n):
    """0, n - 1 and both sides of every multiple of 64 below n"""
    return sorted({0, n - 1} | {e for k in range(64, n + 1, 64) for e in (k - 2, k - 1, k, k + 1) if 0 <= e < n})


def edge_cells(rng, n, m, c, depth):
    """[n][m][2] with every cell drawn from {0, c, c + 1, D - 1, D, 3e9, 0xFFFFFFFF}.  At the sites on both sides of every 64-site
    edge, the samples on both sides of every 64-sample edge carry, rotating from site to site: (3, 1) (t = 4, not informative),
    (4, 1) (informative), (1, 4) (major CG), t = D - 1 and t = D, (0xFFFFFFFF, 5) (t passes 2^32), (0xFFFFFFFF, 0xFFFFFFFF), and
    the four sources whose two counts sit at c and c + 1 -- every class, on both sides of the strict comparison."""
    values = sorted({0, c, c + 1, max(depth, 1) - 1, depth, 3000000000, FULL})
    db = rng.choice(np.array(values, dtype=np.uint32), size=(n, m, 2))
    planted = [(3, 1), (4, 1), (1, 4), (max(depth, 1) - 1, 0), (0, depth), (FULL, 5), (FULL, FULL), (c, c), (c, c + 1), (c + 1, c), (c + 1, c + 1),
               (5, FULL), (depth, 0)]
    for i, s in enumerate(edges(m)):
        for j, r in enumerate(edges(n)):
            db[r, s] = planted[(i + j) % len(planted)]
    return db


def mixture_cohort(seed=7, n=8, m=2000, cov=30.0, err=0.002, target=0, source=3, share=0.10):
    """The simulated cohort of DESIGN.md section 9.7: n unrelated samples x m sites, genotypes from allele frequencies uniform in
    [0.1, 0.9], depth Poisson(cov), reads of the AT allele binomial in its true share bent by the error rate; the target's reads
    are 1 - share its own and share the source's."""
    rng = np.random.default_rng(seed)
    p = rng.uniform(0.1, 0.9, size=m)
    geno = rng.binomial(2, p, size=(n, m)) / 2.0                                            # the share of AT in the sample's DNA
    frac = geno.copy()
    frac[target] = (1 - share) * geno[target] + share * geno[source]
    frac = frac * (1 - err) + (1 - frac) * err
    depth = rng.poisson(cov, size=(n, m))
    at = rng.binomial(depth, frac)
    return np.stack([at, depth - at], axis=2).astype(np.uint32)


# ---------------------------------------------------------------------------------------------------- CPU
def test_surface():
    """The four entry points are exported and declared, the record is 64 bytes here and in the binding, the text functions are
    exported by libntsm_host.so, and the help text names the flags under "This build only" and says what the defaults are."""
    lib = ctypes.CDLL(os.path.join(ROOT, "ntsm_amd", "libntsm_eval_hip.so"))
    hdr = open(os.path.join(ROOT, "include", "ntsm_eval_hip.h")).read()
    for name in ("ntsm_eval_contam_open", "ntsm_eval_contam_rows", "ntsm_eval_contam_close", "ntsm_eval_contam_tune"):
        assert hasattr(lib, name) and name + "(" in hdr, name
    assert "typedef struct ntsm_eval_contam_record { uint64_t minor[3], depth[3]; uint32_t sites[3], pad /* 0 */; } ntsm_eval_contam_record;" in hdr
    assert RECORD.itemsize == 64
    import ntsm_amd.eval as ev
    assert ev.CONTAM_RECORD == RECORD
    assert callable(ev.Contam) and callable(ev.contam_tune) and callable(ev.contam_rows_text) and callable(ev.contam_sample_table_text)
    assert ev.lib.ntsm_eval_contam_tune(128, 0) == -1 and ev.lib.ntsm_eval_contam_tune(64, 3) == -1 and ev.lib.ntsm_eval_contam_tune(0, 0) == 0
    p = subprocess.run([EVAL, "--help"], capture_output=True, env=HIDDEN)
    assert p.returncode == 0 and p.stdout == b""
    ours = p.stderr.split(b"This build only")[1]
    for flag in (b"--contam = STORE", b"--contam-depth = INT", b"--contam-min = FLOAT", b"--contam-explained = FLOAT", b"--contam-rows = INT",
                 b"--samples-out = FILE"):
        assert flag in ours, flag
    assert b"[0.010000]" in ours and b"[0.500000]" in ours and b"[8]" in ours and b"conventions" in ours and b"not from real data" in ours
    assert b"--qc = STORE" in ours and b"--between-near = STORE_A STORE_B" in ours               # and what was there is


def test_refusals(tmp_path):
    """Every refusal of --contam and its flags: exit 1, its own 'Error:' sentence, nothing on stdout, no GPU work (devices are
    hidden), the store -- bytes and mtime -- as it was, and no --samples-out file left behind."""
    rng = np.random.default_rng(5)
    db = rng.integers(0, 30, size=(3, 40, 2)).astype(np.uint32)
    write_store(tmp_path / "S", db, rng)
    write_store(tmp_path / "empty", db[:0], rng)
    good = open(str(tmp_path / "S"), "rb").read()
    open(str(tmp_path / "trunc"), "wb").write(good[:-1])
    open(str(tmp_path / "magic"), "wb").write(b"NTSMCOH2" + good[8:])
    open(str(tmp_path / "q.txt"), "w").write("#@TK\t5\n#@KS\t19\nrs1\t1\t2\t1\t2\t1\t1\n")
    open(str(tmp_path / "rot.tsv"), "w").write("x\n")
    open(str(tmp_path / "norm.txt"), "w").write("0\n")
    os.mkdir(str(tmp_path / "dir"))
    own = b"--contam checks one store for cross-sample contamination and is a run of its own"
    flags = b"belong to --contam: give them with --contam STORE"
    cases = [
        (["--contam", "S", "--pack", "S", "q.txt"], "S", own),                               # with any other store run
        (["--contam", "S", "--against", "S", "q.txt"], "S", own),
        (["--contam", "S", "--index", "S", "-p", "rot.tsv", "-n", "norm.txt"], "S", own),
        (["--contam", "S", "--near", "S", "q.txt"], "S", own),
        (["--contam", "S", "--within", "S"], "S", own),
        (["--contam", "S", "--within-near", "S"], "S", own),
        (["--contam", "S", "--between", "S", "S"], "S", own),
        (["--between-near", "S", "--contam", "S", "S"], "S", own),
        (["--qc", "S", "--contam", "S"], "S", own),
        (["--contam-depth", "4", "--within", "S"], "S", flags),                              # its flags without it
        (["--contam-min", "0.1", "--qc", "S"], "S", flags),
        (["--contam-explained", "0.1", "q.txt"], "S", flags),
        (["--contam-rows", "2", "--within", "S"], "S", flags),
        (["--samples-out", "samples.tsv", "--qc", "S"], "S", b"--samples-out is the per-sample table of --contam"),
        (["--samples-out", "samples.tsv", "q.txt"], "S", b"--samples-out is the per-sample table of --contam"),
        (["--contam", "S", "q.txt"], "S", b"--contam takes no input files"),
        (["--contam", "S", "-p", "rot.tsv", "-n", "norm.txt"], "S", b"--contam reads allele counts, not projections, and takes no -p and no -n"),
        (["--contam", "S", "-p", "rot.tsv"], "S", b"takes no -p and no -n"),
        (["--contam", "S", "-n", "norm.txt"], "S", b"takes no -p and no -n"),
        (["--contam", "S", "-b", "truth.tsv"], "S", b"-b with --contam is not part of this build"),
        (["--contam", "S", "-e", "merged.txt"], "S", b"merging (-e, -o) with --contam is not part of this build"),
        (["--contam", "S", "-o"], "S", b"merging (-e, -o) with --contam is not part of this build"),
        (["--contam", "trunc"], "trunc", b"its header describes"),                           # an invalid store
        (["--contam", "magic"], "magic", b"not a cohort store"),
        (["--contam", "nowhere"], "S", b"cannot open store nowhere"),
        (["--contam", "empty"], "empty", b"empty holds no samples"),
        (["--contam", "S", "--contam-explained", "half"], "S", b"--contam-explained takes a number, not half"),
        (["--contam", "S", "--contam-explained", "0.5x"], "S", b"--contam-explained takes a number, not 0.5x"),
        (["--contam", "S", "--contam-min", "1e"], "S", b"--contam-min takes a number, not 1e"),
        (["--contam", "S", "--contam-min", ""], "S", b"--contam-min takes a number, not "),
        (["--contam", "S", "--contam-depth", "-1"], "S", b"--contam-depth takes a number of reads, not -1"),
        (["--contam", "S", "--contam-rows", "two"], "S", b"--contam-rows takes a number of samples, not two"),
        (["--contam", "S", "--samples-out", "dir"], "S", b"cannot write dir"),               # cannot be opened for writing
        (["--contam", "S", "--samples-out", "no/such/dir/samples.tsv"], "S", b"cannot write no/such/dir/samples.tsv"),
        (["--contam", "S", "--sites-out", "sites.tsv"], "S", b"--sites-out is the per-site table of --qc"),
        (["--contam", "S", "--within-rows", "3"], "S", b"--within-rows sets the bands of --within"),
        (["--contam", "S", "--between-rows", "3"], "S", b"--between-rows sets the bands of --between"),
    ]
    for args, touched, sentence in cases:
        extra = ["--samples-out", "samples.tsv"] if "--contam" in args and "--samples-out" not in args else []
        path = str(tmp_path / touched)
        before = snapshot(path)
        p = run(args + extra, tmp_path, env=HIDDEN)
        assert p.returncode == 1 and p.stdout == b"", (args, p.returncode, p.stdout[:100], p.stderr[-300:])
        errors = [line for line in p.stderr.split(b"\n") if line.startswith(b"Error: ")]
        assert len(errors) == 1 and sentence in errors[0], (args, p.stderr)
        assert unchanged(path, before), args
        for left in ("samples.tsv", "sites.tsv", "merged.txt", touched + ".pcaidx", touched + ".tmp"):
            assert not os.path.exists(str(tmp_path / left)), (args, left)
    # the sentences the other runs always had
    p = run(["--qc", "S", "--within", "S"], tmp_path, env=HIDDEN)
    assert p.returncode == 1 and b"--qc prints the QC tables of one store and is a run of its own" in p.stderr
    p = run(["--within", "S", "--pack", "S"], tmp_path, env=HIDDEN)
    assert p.returncode == 1 and b"are seven runs: give one of them" in p.stderr


def test_contam_without_a_device_fails_and_prints_nothing(tmp_path):
    """A valid --contam where no device can be opened: the GPU failure message, exit 3, no header on stdout, the store as it
    was, no --samples-out file made -- and one that was there keeps its bytes."""
    rng = np.random.default_rng(6)
    write_store(tmp_path / "S", rng.integers(0, 30, size=(3, 40, 2)).astype(np.uint32), rng)
    before = snapshot(str(tmp_path / "S"))
    open(str(tmp_path / "old.tsv"), "w").write("kept\n")
    for args in ([], ["-a", "-c", "0", "--contam-depth", "0", "--contam-min", "-1", "--contam-explained", "1e-3", "--contam-rows", "2", "-v", "-v"],
                 ["--samples-out", "samples.tsv"], ["--samples-out", "old.tsv"]):
        p = run(["--contam", "S"] + args, tmp_path, env=HIDDEN)
        assert p.returncode == 3 and p.stdout == b"", (args, p.returncode, p.stdout[:100], p.stderr[-300:])
        assert b"on the GPU failed" in p.stderr and b"there is no CPU path" in p.stderr, (args, p.stderr)
        assert unchanged(str(tmp_path / "S"), before) and not os.path.exists(str(tmp_path / "samples.tsv"))
        assert open(str(tmp_path / "old.tsv")).read() == "kept\n"


def test_bad_arguments_and_empty_shapes_need_no_device():
    """-1 before any HIP call: a stride below 8 * n_sites, one that is no multiple of 4, counts NULL, the handle's place NULL; a
    range past n_db, no rows, out NULL, the handle NULL.  A store without sites gives zeroed outputs and one without samples
    has no range to take -- neither touches a device."""
    import ntsm_amd.eval as ev
    opn, rows, close = ev.lib.ntsm_eval_contam_open, ev.lib.ntsm_eval_contam_rows, ev.lib.ntsm_eval_contam_close
    m, n = 5, 3
    db = np.ones((n, m, 2), dtype=np.uint32)
    h = ctypes.c_void_p(1)
    assert opn(0, db.ctypes.data, 8 * m - 8, n, m, 1, 8, 0, ctypes.byref(h)) == -1 and h.value is None
    assert opn(0, db.ctypes.data, 8 * m - 4, n, m, 1, 8, 0, ctypes.byref(h)) == -1
    assert opn(0, db.ctypes.data, 8 * m + 2, n, m, 1, 8, 0, ctypes.byref(h)) == -1
    assert opn(0, None, 8 * m, n, m, 1, 8, 0, ctypes.byref(h)) == -1
    assert opn(0, db.ctypes.data, 8 * m, n, m, 1, 8, 0, None) == -1
    tally = np.full((n, 3), 7, np.uint64)
    out = np.frombuffer(b"\x07" * (64 * n * n), dtype=RECORD).copy().reshape(n, n)
    assert rows(None, 0, 1, out.ctypes.data, tally.ctypes.data, None) == -1
    assert opn(0, db.ctypes.data, 0, n, 0, 1, 8, 0, ctypes.byref(h)) == 0 and h.value                # no site: a session without device work
    times = ev.CrossTimes(1.0, 1.0, 1.0, 1.0, 9)
    assert rows(h, 0, 0, out.ctypes.data, tally.ctypes.data, None) == -1
    assert rows(h, 1, n, out.ctypes.data, tally.ctypes.data, None) == -1
    assert rows(h, n, 1, out.ctypes.data, tally.ctypes.data, None) == -1
    assert rows(h, 0, n, None, tally.ctypes.data, None) == -1
    assert out.tobytes() == b"\x07" * (64 * n * n) and (tally == 7).all()
    assert rows(h, 1, 2, out.ctypes.data, tally.ctypes.data, ctypes.byref(times)) == 0
    assert out[:2].tobytes() == bytes(64 * n * 2) and out[2].tobytes() == b"\x07" * (64 * n)
    assert (tally[:2] == 0).all() and (tally[2] == 7).all() and times.chunks == 0 and times.upload_ms == 0
    assert rows(h, 0, n, out.ctypes.data, None, None) == 0 and out.tobytes() == bytes(64 * n * n)
    close(h)
    assert opn(0, None, 8 * m, 0, m, 1, 8, 0, ctypes.byref(h)) == 0 and h.value                      # no sample
    assert rows(h, 0, 0, out.ctypes.data, None, None) == -1 and rows(h, 0, 1, out.ctypes.data, None, None) == -1
    close(h)
    close(None)


def test_the_model_is_the_contract_site_by_site():
    """model() (vectorised, what the GPU tests compare with) against scalar_model() (the header's text, one pair and one site
    at a time) on edge cells: 9 samples x 70 sites at three (min_cov, min_depth); every record field and tally."""
    rng = np.random.default_rng(70)
    for c, depth in ((0, 0), (1, 8), (5, 1)):
        db = edge_cells(rng, 9, 70, c, depth)
        rec, tally = model(db, c, depth)
        want_rec, want_tally = scalar_model(db.tolist(), c, depth)
        assert tally.tolist() == want_tally
        got = [[[rec["minor"][q, d].tolist(), rec["depth"][q, d].tolist(), rec["sites"][q, d].tolist()] for d in range(9)] for q in range(9)]
        assert got == want_rec
        assert int(rec["sites"].sum()) > 200 and (rec["sites"].sum(axis=(0, 1)) > 0).all()   # every class occurs
        assert int(rec["depth"].max()) > 2**32


def test_row_and_sample_text_against_the_model():
    """eval_contam.hpp's two tables (through libntsm_host.so) against rows_text / samples_text on given integers: depth 0 in
    each class (NA, and NA in what is formed from it), a target without informative sites, rateAll == 0, sums past 2^53, thirds
    (digits that round), a row exactly at excess == X and one exactly at explained == Y (printed), rows just below either (not
    printed), a negative excess; under -a and under the filter; as one band and as a later band of a longer store."""
    import ntsm_amd.eval as ev
    big = 2**53 + 1

    def rec(minor, depth, sites=(1, 2, 3)):
        r = np.zeros((), dtype=RECORD)
        for k in range(3):
            r["minor"][k], r["depth"][k], r["sites"][k] = np.uint64(minor[k]), np.uint64(depth[k]), sites[k]
        return r
    cases = [                                                                                # (record, the target's tally)
        (rec((0, 0, 0), (0, 0, 0), (0, 0, 0)), (0, 0, 0)),                                   # nothing at all: every field NA
        (rec((1, 2, 3), (0, 10, 10)), (5, 6, 20)),                                           # no lack site
        (rec((1, 2, 3), (10, 0, 10)), (5, 6, 20)),                                           # no het site
        (rec((1, 2, 3), (10, 10, 0)), (5, 6, 20)),                                           # no opp site
        (rec((0, 0, 0), (10, 10, 10)), (5, 0, 30)),                                          # rateAll == 0
        (rec((1, 2, 3), (10, 10, 10)), (0, 0, 0)),                                           # a target without informative sites (not the device's, but the text's case)
        (rec((big, 2 * big, 3 * big), (3 * big, 3 * big, 4 * big + 3)), (7, 2**63, 2**64 - 1)),   # past 2^53
        (rec((1, 1, 2), (3, 3, 3)), (9, 4, 9)),                                              # thirds
        (rec((0, 5, 1), (100, 100, 100)), (9, 6, 300)),                                      # excess == 0.01 exactly, explained == 1
        (rec((0, 5, 1), (100, 100, 101)), (9, 6, 300)),                                      # excess just below X
        (rec((1, 5, 1), (100, 100, 10)), (9, 2, 100)),                                       # explained == 0.5 exactly: 1 - 0.01 / 0.02
        (rec((1, 5, 1), (100, 100, 10)), (9, 2, 101)),                                       # explained just below Y
        (rec((9, 5, 1), (100, 100, 100)), (9, 15, 300)),                                     # a negative excess
        (rec((1, 5, 30), (100, 100, 100)), (9, 36, 300)),                                    # a plain contaminated pair
    ]
    assert fields(cases[8][0], cases[8][1])[1:] == (0.01, 1.0) and fields(cases[10][0], cases[10][1])[2] == 0.5
    assert fields(cases[9][0], cases[9][1])[1] < 0.01 and fields(cases[11][0], cases[11][1])[2] < 0.5
    n = len(cases) + 1                                                                       # one target per case, each against source 0 ... n - 1
    names = ["cohort/run%02d.txt" % i for i in range(n)]
    table = np.zeros((n - 1, n), dtype=RECORD)
    tally = np.zeros((n - 1, 3), dtype=np.uint64)
    for r, (record, t) in enumerate(cases):
        table[r, :] = record
        tally[r] = [np.uint64(v) for v in t]
    for all_rows in (False, True):
        got = ev.contam_rows_text(names, 0, table, tally, all_rows, X, Y)
        assert got == rows_text(names, table, tally, 0, all_rows), all_rows
        lines = got.decode().split("\n")[:-1]
        assert len(lines) == ((n - 1) * (n - 1) if all_rows else 4 * (n - 1))                # no het site, at X, at Y and the plain one; the diagonal is skipped
        assert ev.contam_rows_text(names, 1, table[1:], tally[1:], all_rows, X, Y) == rows_text(names, table[1:], tally[1:], 1, all_rows)
    text = ev.contam_rows_text(names, 0, table, tally, True, X, Y).decode().split("\n")
    assert text[0] == "cohort/run00.txt\tcohort/run01.txt\t0\t0\t0\tNA\tNA\tNA\tNA\tNA"
    assert text[7 * (n - 1)] == "cohort/run07.txt\tcohort/run00.txt\t1\t2\t3\t0.333333\t0.333333\t0.666667\t0.333333\t0.250000"
    kept = ev.contam_rows_text(names, 0, table, tally, False, X, Y).decode()
    assert "cohort/run08.txt\tcohort/run00.txt\t1\t2\t3\t0.000000\t0.050000\t0.010000\t0.010000\t1.000000\n" in kept
    assert "cohort/run10.txt\tcohort/run00.txt\t1\t2\t3\t0.010000\t0.050000\t0.100000\t0.090000\t0.500000\n" in kept
    assert {line[:16] for line in kept.split("\n")[:-1]} == {"cohort/run%02d.txt" % r for r in (2, 8, 10, 13)}
    assert ev.contam_rows_text(names, 0, table, tally, False, -1.0, -1e9).count(b"\n") == 9 * (n - 1)   # other cuts: every row whose two fields are numbers
    assert ev.contam_rows_text(names, 0, table[:0], tally[:0], True, X, Y) == b""
    assert ev.contam_sample_table_text(names[:-1], tally) == samples_text(names[:-1], tally.tolist())
    lines = ev.contam_sample_table_text(names[:-1], tally).decode().split("\n")
    assert lines[0] + "\n" == SAMPLE_HEADER and lines[1] == "cohort/run00.txt\t0\t0\t0\tNA" and lines[8] == "cohort/run07.txt\t9\t4\t9\t0.444444"
    assert lines[7] == "cohort/run06.txt\t7\t9223372036854775808\t18446744073709551615\t0.500000"
    assert ev.contam_sample_table_text([], np.zeros((0, 3))) == SAMPLE_HEADER.encode()


def test_band_rule():
    """As many targets as fit in the limit of records, at least one, never past the end; the default limit is 1 GiB of 64-byte
    records."""
    import ntsm_amd.eval as ev
    assert ev.contam_band_rows(0, 10, 35) == 3 and ev.contam_band_rows(9, 10, 35) == 1 and ev.contam_band_rows(8, 10, 35) == 2
    assert ev.contam_band_rows(0, 10, 9) == 1 and ev.contam_band_rows(0, 10, 0) == 1 and ev.contam_band_rows(0, 10, 100) == 10
    assert ev.contam_band_rows(0, 4096) == 4096 and ev.contam_band_rows(0, 8192) == 2048 and ev.contam_band_rows(7000, 8192) == 1192
    assert ev.contam_band_rows(0, FULL, 2**24) == 1 and ev.contam_band_rows(0, 0) == 0 and ev.contam_band_rows(10, 10) == 0
    for n, limit in ((1, 1), (7, 20), (130, 1000)):
        first, bands = 0, 0
        while first < n:
            rows = ev.contam_band_rows(first, n, limit)
            assert 1 <= rows <= n - first and (rows * n <= limit or rows == 1)
            first, bands = first + rows, bands + 1
        assert bands == -(-n // max(1, limit // n))


def test_band_rule_and_text_under_the_host_sanitizers():
    """`make contam_check`: tools/eval_contam_check.cpp -- eval_contam.hpp's band rule against a scan and both tables' text on
    their cases -- built with -fsanitize=address,undefined as a program of its own, run once by the target and once here for its
    lines."""
    subprocess.run(["make", "-s", "contam_check"], cwd=ROOT, check=True, stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(ROOT, "build", "eval_contam_check")], capture_output=True)
    assert p.returncode == 0 and p.stdout.endswith(b"ok\n") and b"FAILED" not in p.stdout and p.stderr == b"", (p.stdout[-600:], p.stderr[-600:])
    for part in (b"band rule: ", b"row text: ", b"sample text: "):
        assert part in p.stdout


def test_mixture_premise_on_the_model_alone():
    """A condition on the input, checked without the code under test: in the simulated cohort (default_rng(7); 8 samples x 2,000
    sites, 30x, 0.2 % error, sample 0 = 90 % its own reads + 10 % sample 3's) the model under the defaults prints exactly one
    row, (sample 0, source 3), so no row for a clean target; at a 2 % share the true source still leads in both fields."""
    names = ["cohort/run%04d.txt" % r for r in range(8)]
    rec, tally = model(mixture_cohort(), 1, DEPTH)
    text = rows_text(names, rec, tally).decode()
    assert text.count("\n") == 1 and text.startswith(names[0] + "\t" + names[3] + "\t")
    _, excess, explained = fields(rec[0, 3], tally[0])
    assert excess > 0.05 and explained > 0.8
    others = [fields(rec[0, d], tally[0]) for d in (1, 2, 4, 5, 6, 7)]
    assert all(e[2] < 0.4 for e in others)
    rec, tally = model(mixture_cohort(share=0.02), 1, DEPTH)
    lead = fields(rec[0, 3], tally[0])
    assert all(lead[1] > fields(rec[0, d], tally[0])[1] and lead[2] > fields(rec[0, d], tally[0])[2] for d in (1, 2, 4, 5, 6, 7))


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gpu(built):
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    import ntsm_amd.eval as ev
    return ev


def same(got, want, what):
    for name in ("minor", "depth", "sites", "pad"):
        assert np.array_equal(got[0][name], want[0][name]), (what, name, np.argwhere(got[0][name] != want[0][name])[:5].tolist())
    assert got[1].dtype == np.uint64 and np.array_equal(got[1], want[1]), (what, "tally", np.argwhere(got[1] != want[1])[:5].tolist())


def whole(ev, db, c, depth, chunk=0, head=0):
    with ev.Contam(ev.Records.of(db, head), c, depth, chunk) as s:
        return s.rows(0, s.n)


SETTINGS = [(c, depth) for c in (0, 1, 5) for depth in (0, 1, 8)]


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 63, 64, 65, 130])
def test_rows_equal_the_model_on_every_field(gpu, m):
    """ntsm_eval_contam_rows against model(): every field of every record and tally, as integers.  Sites 1, 63, 64, 65 and 130
    stand either side of the transpose's 64-site tile; samples 1, 2, 63, 64, 65, 130 and 257 either side of one wave of sources
    (257: five one-wave workgroups, the last with one live lane) and of the target groups; min_cov 0, 1, 5 and min_depth 0, 1, 8
    over edge_cells; the pitch dense and a store's (a 1,056-byte head).  65 x 65 and 257 x 130 take all nine settings at both
    pitches; every other shape takes three settings that between them hold every value, the pitch alternating."""
    rng = np.random.default_rng([m, 71])
    for i, n in enumerate((1, 2, 63, 64, 65, 130, 257)):
        full = (n, m) in ((65, 65), (257, 130))
        for j, (c, depth) in enumerate(SETTINGS if full else ((0, 8), (1, 0), (5, 1))):
            db = edge_cells(rng, n, m, c, depth)
            want = model(db, c, depth)
            for head in ((0, RECORD_HEAD) if full else ((0, RECORD_HEAD)[(i + j) % 2],)):
                got = whole(gpu, db, c, depth, 0, head)
                same(got, want, (n, m, c, depth, head))
                assert got[2].chunks == 0


@pytest.fixture(scope="module")
def edge130(gpu):
    """130 samples x 65 sites at min_cov 1, min_depth 8 in a store's pitch: (records, model) once for the tests that share it"""
    db = edge_cells(np.random.default_rng(72), 130, 65, 1, 8)
    return db, gpu.Records.of(db, RECORD_HEAD), model(db, 1, 8)


@pytest.mark.gpu
def test_bands_concatenate_to_the_one_call_result(gpu, edge130):
    """The whole store in one call; the band (0, 1); a middle band; a band that ends at n_db: each equals its rows of the model,
    and all bands concatenated equal the one call as bytes -- resident, and streamed in chunks of 64."""
    db, rec, want = edge130
    for chunk in (0, 64):
        with gpu.Contam(rec, 1, 8, chunk) as s:
            one = s.rows(0, 130)
            same(one, want, chunk)
            assert one[2].chunks == (3 if chunk else 0)
            parts = [s.rows(first, rows) for first, rows in ((0, 1), (1, 39), (40, 60), (100, 30))]
        for (first, rows), part in zip(((0, 1), (1, 39), (40, 60), (100, 30)), parts):
            same(part, (want[0][first:first + rows], want[1][first:first + rows]), (chunk, first))
        assert b"".join(p[0].tobytes() for p in parts) == one[0].tobytes() and b"".join(p[1].tobytes() for p in parts) == one[1].tobytes()


@pytest.mark.gpu
def test_resident_and_streamed_give_identical_bytes(gpu, edge130):
    """20 samples as one chunk, as a chunk of exactly 20 (still resident) and as 7 of 20; 130 samples resident and as 64 of 130:
    records and tallies byte for byte, and chunks counts the column chunks uploaded."""
    rng = np.random.default_rng(73)
    db = edge_cells(rng, 20, 65, 1, 8)
    want = model(db, 1, 8)
    runs = [whole(gpu, db, 1, 8, chunk, RECORD_HEAD) for chunk in (0, 20, 7)]
    same(runs[0], want, 20)
    assert [r[2].chunks for r in runs] == [0, 0, 3]
    assert all(r[0].tobytes() == runs[0][0].tobytes() and r[1].tobytes() == runs[0][1].tobytes() for r in runs[1:])
    db, rec, want = edge130
    with gpu.Contam(rec, 1, 8, 0) as a, gpu.Contam(rec, 1, 8, 64) as b:
        ra, rb = a.rows(0, 130), b.rows(0, 130)
    assert (ra[2].chunks, rb[2].chunks) == (0, 3)
    assert ra[0].tobytes() == rb[0].tobytes() == want[0].tobytes() and ra[1].tobytes() == rb[1].tobytes() == want[1].tobytes()


@pytest.mark.gpu
def test_every_forced_launch_gives_identical_bytes(gpu, edge130):
    """Every (width, target group) through ntsm_eval_contam_tune on 130 samples x 65 sites: the bytes of the library's rule."""
    db, rec, want = edge130
    try:
        with gpu.Contam(rec, 1, 8) as s:
            for width in (0, 64, 256):
                for group in (0, 1, 2, 4):
                    gpu.contam_tune(width, group)
                    got = s.rows(0, 130)
                    assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (width, group)
                    band = s.rows(127, 3)                                                   # three targets: a group of 2 and of 4 run past the band
                    assert band[0].tobytes() == want[0][127:].tobytes(), (width, group)
    finally:
        gpu.contam_tune(0, 0)


@pytest.mark.gpu
def test_optional_tally_two_calls_and_the_diagonal(gpu, edge130):
    """tally NULL leaves the records as they are; two calls give identical bytes; the diagonal (q, q) is the model's diagonal --
    a pair like any other -- and pad is 0 everywhere; resident and streamed."""
    db, rec, want = edge130
    diag = np.arange(130)
    for chunk in (0, 64):
        with gpu.Contam(rec, 1, 8, chunk) as s:
            first, second, bare = s.rows(0, 130), s.rows(0, 130), s.rows(0, 130, tally=False)
        assert first[0].tobytes() == second[0].tobytes() and first[1].tobytes() == second[1].tobytes()
        assert bare[1] is None and bare[0].tobytes() == first[0].tobytes()
        assert first[0][diag, diag].tobytes() == want[0][diag, diag].tobytes() and int(first[0]["sites"][diag, diag].sum()) > 0
        assert not first[0]["pad"].any()


def contam(args, d):
    p = run(["--contam"] + args, d)
    assert p.returncode == 0, p.stderr[-400:]
    return p


@pytest.mark.gpu
def test_cli_on_the_mixture_cohort(gpu, tmp_path):
    """The simulated cohort written as a store: under the defaults stdout is the header and the one row (sample 0, source 3);
    under -a all 56 rows; --samples-out writes the per-sample table, replacing a longer file; each byte for byte the model's
    text.  -vv reports the shape of the run on one stderr line."""
    db = mixture_cohort()
    _, names = write_store(tmp_path / "M", db, np.random.default_rng(74))
    rec, tally = model(db, 1, DEPTH)
    p = contam(["M", "-v", "-v"], tmp_path)
    assert p.stdout == HEADER.encode() + rows_text(names, rec, tally) and p.stdout.count(b"\n") == 2
    assert p.stdout.split(b"\n")[1].startswith((names[0] + "\t" + names[3] + "\t").encode())
    report = [l for l in p.stderr.split(b"\n") if l.startswith(b"store contam: ")]
    assert len(report) == 1 and b"resident, 1 bands, 0 chunks" in report[0] and b"rectangle kernel" in report[0] and b"upload" in report[0]
    open(str(tmp_path / "samples.tsv"), "w").write("x" * 100000)
    p = contam(["M", "-a", "--samples-out", "samples.tsv"], tmp_path)
    assert p.stdout == HEADER.encode() + rows_text(names, rec, tally, 0, True) and p.stdout.count(b"\n") == 57
    assert open(str(tmp_path / "samples.tsv"), "rb").read() == samples_text(names, tally.tolist())
    p = contam(["M", "--contam-min", "0.02", "--contam-explained", "0.1", "--contam-depth", "20", "-c", "2"], tmp_path)
    rec, tally = model(db, 2, 20)
    assert p.stdout == HEADER.encode() + rows_text(names, rec, tally, 0, False, 0.02, 0.1)


@pytest.mark.gpu
def test_cli_on_an_edge_store_in_bands(gpu, tmp_path):
    """70 x 65 edge cells, one sample empty, at -c 2 --contam-depth 3 -a --contam-rows 9: eight bands, the last of 7 rows, printed
    one after the other, equal the model's text; so does the one band of the band rule."""
    rng = np.random.default_rng(75)
    db = edge_cells(rng, 70, 65, 2, 3)
    db[7] = 0                                                                               # an empty sample: NA in its row and in its column
    _, names = write_store(tmp_path / "W", db, rng)
    rec, tally = model(db, 2, 3)
    want = HEADER.encode() + rows_text(names, rec, tally, 0, True)
    p = contam(["W", "-c", "2", "--contam-depth", "3", "-a", "--contam-rows", "9", "-v", "-v", "--samples-out", "w.tsv"], tmp_path)
    assert p.stdout == want and want.count(b"\n") == 1 + 70 * 69
    assert b"8 bands" in [l for l in p.stderr.split(b"\n") if l.startswith(b"store contam: ")][0]
    assert open(str(tmp_path / "w.tsv"), "rb").read() == samples_text(names, tally.tolist())
    assert contam(["W", "-c", "2", "--contam-depth", "3", "-a"], tmp_path).stdout == want
    assert (names[7] + "\t" + names[8] + "\t0\t0\t0\tNA\tNA\tNA\tNA\tNA\n").encode() in want


def stored(path):
    s = read_store(str(path))
    return [r["name"] for r in s["samples"]], np.stack([r["counts"] for r in s["samples"]]).reshape(s["n"], s["m"], 2)


@pytest.mark.gpu
def test_cli_on_a_packed_and_appended_store(gpu, tmp_path):
    """A store packed by --pack from six counts files (one with counts beyond 2^31, one empty) and the same files packed in two
    runs: the same stdout, the model's text over the counts and names the store holds."""
    _, files = qc_cohort(tmp_path)
    assert run(["--pack", "S2"] + files[:4], tmp_path).returncode == 0
    assert run(["--pack", "S2"] + files[4:], tmp_path).returncode == 0
    names, db = stored(tmp_path / "S2")
    assert names == files and db.shape == (6, 130, 2)
    rec, tally = model(db, 1, DEPTH)
    a, b = contam(["S2", "-a", "--samples-out", "s2.tsv"], tmp_path), contam(["S", "-a"], tmp_path)
    assert a.stdout == b.stdout == HEADER.encode() + rows_text(names, rec, tally, 0, True)
    assert open(str(tmp_path / "s2.tsv"), "rb").read() == samples_text(names, tally.tolist())
    assert contam(["S2"], tmp_path).stdout == HEADER.encode() + rows_text(names, rec, tally)


@pytest.mark.gpu
def test_cli_on_a_store_written_by_the_cohort_counter(gpu, tmp_path):
    """`ntsmCount --cohort --store` over two tiny samples: --contam of its store equals the model's text over what it holds."""
    import ntsm_amd
    d = tmp_path
    s = ntsm_amd.SynthShort(sites_seed=20261020, n_sites=200, read_seed=7, sites_path=str(d / "sites.fa"))
    s.write_fastq(str(d / "one.fq"), 0, 4000)
    s.write_fastq(str(d / "two.fq"), 4000, 5000)
    open(str(d / "m.tsv"), "w").write("one.txt\tone.fq\ntwo.txt\ttwo.fq\n")
    p = subprocess.run([COUNT, "-s", "sites.fa", "--cohort", "m.tsv", "--store", "CS"], cwd=str(d), capture_output=True)
    assert p.returncode == 0, p.stderr[-400:]
    names, db = stored(d / "CS")
    assert names == ["one.txt", "two.txt"] and int(db.sum()) > 0
    for c, depth in ((1, DEPTH), (0, 2)):
        rec, tally = model(db, c, depth)
        q = contam(["CS", "-a", "-c", c, "--contam-depth", depth, "--samples-out", "cs.tsv"], d)
        assert q.stdout == HEADER.encode() + rows_text(names, rec, tally, 0, True) and q.stdout.count(b"\n") == 3
        assert open(str(d / "cs.tsv"), "rb").read() == samples_text(names, tally.tolist())
