"""ntsmEval's PCA-guided pair search (-p / -n): ntsm_amd/csrc/xprec.h, the session calls of include/ntsm_eval_hip.h
(ntsm_eval_project, ntsm_eval_candidates, ntsm_eval_score_pairs) and build/ntsmEval -p.

PARITY WITH THE REFERENCE is pinned in tests/test_eval_reference.py, as for the all-pairs path: expected_text below and
build/ntsmEval -p against projectPCs + computeScorePCA of the unmodified CompareCounts.hpp (oracle/_ref/ref_ntsmEval) and
its recordings, byte for byte.  What the tests of this file pin is (CPU) the integer x87 add against the x87 itself, and the
CLI's refusals and flag errors; (GPU) the projection and the candidate list against tests/eval_pca_restatement.cpp, an
independent restatement written from the reference text and compiled here with real long double, the listed-pair scoring
against ntsm_eval_pairs, and the CLI's stdout against text assembled from the restatement and the all-pairs oracle
(oracle/ntsm_eval_oracle.c)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle_binding import EvalOracle, ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_eval import FIELDS, files_for, py_pair, random_samples, same_bits, write_counts  # noqa: E402

EVAL = os.path.join(ROOT, "build", "ntsmEval")
DBL_MAX = 1.7976931348623157e308
HEADER = ("sample1\tsample2\tscore\tsame\tdist\trelate\tibs0\tibs2\thomConcord\thet1\thet2\tsharedHet\thom1\thom2\tsharedHom\tn"
          "\tcov1\tcov2\terrorRate1\terrorRate2\tmiss1\tmiss2\tallHom1\tallHom2\tallHet1\tallHet2")


def gxx(tmp, src, name):
    exe = str(tmp / name)
    subprocess.run(["g++", "-O2", "-std=c++11", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", src)], check=True)
    return exe


@pytest.fixture(scope="module")
def restatement(tmp_path_factory):
    return gxx(tmp_path_factory.mktemp("rs"), "eval_pca_restatement.cpp", "eval_pca_restatement")


def digits19(rng, count):
    a, b = rng.integers(10 ** 9, 10 ** 10, size=count), rng.integers(0, 10 ** 9, size=count)
    return ["%d%09d" % (x, y) for x, y in zip(a.tolist(), b.tolist())]


def write_pca(tmp, m, comp, rng, extra=0, bad_line=False, exp=(2, 3)):
    """A centre file (one value per line, 19 significant digits) and a rotation file (header 'rsID PC1 ... PCcomp', then
    'rsID v1 ... vcomp' with 20 significant digits) for m sites plus `extra` rows the projection does not use."""
    rows = m + extra
    norm, rot = str(tmp / "norm.txt"), str(tmp / "rot.tsv")
    nd = digits19(rng, rows)
    with open(norm, "w") as f:
        for j in range(rows):
            f.write("x\n" if bad_line and j == 1 else "0.%s\n" % nd[j])           # a line that does not parse reads as 0
    lead = rng.integers(1, 10, size=(rows, comp)).tolist()
    dg = digits19(rng, rows * comp)
    sg = rng.integers(0, 2, size=rows * comp).tolist()
    ex = rng.choice(exp, size=rows * comp).tolist()
    with open(rot, "w") as f:
        f.write("rsID\t" + "\t".join("PC%d" % (d + 1) for d in range(comp)) + "\n")
        for j in range(rows):
            vals = ["%s%d.%se-%d" % ("-" if sg[j * comp + d] else "", lead[j][d], dg[j * comp + d], ex[j * comp + d]) for d in range(comp)]
            f.write("rs%d\t%s\n" % (j, "\t".join(vals)))
    return norm, rot


def rs_project(exe, tmp, counts, min_cov, norm, rot, dim):
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    n, m = counts.shape[0], counts.shape[1]
    cin, cout, nout, rout = (str(tmp / x) for x in ("c.bin", "cloud.bin", "norm.bin", "rot.bin"))
    counts.tofile(cin)
    subprocess.run([exe, "project", cin, str(n), str(m), str(min_cov), norm, rot, str(dim), cout, nout, rout], check=True)
    return (np.fromfile(cout, dtype=np.float64).reshape(n, dim), np.fromfile(nout, dtype=np.longdouble),
            np.fromfile(rout, dtype=np.longdouble).reshape(dim, m))


def rs_candidates(exe, tmp, cloud, radius):
    cin, rin, out = str(tmp / "cl.bin"), str(tmp / "rad.bin"), str(tmp / "cand.txt")
    np.ascontiguousarray(cloud, dtype=np.float64).tofile(cin)
    np.ascontiguousarray(radius, dtype=np.float64).tofile(rin)
    subprocess.run([exe, "candidates", cin, str(cloud.shape[0]), str(cloud.shape[1]), rin, out], check=True)
    rows = [line.split("\t") for line in open(out).read().splitlines()]
    return [(int(i), int(k), float.fromhex(d)) for i, k, d in rows]


def same_list(got, want):
    """Pairs in order; rows with equal (i, distance) compared as sets."""
    def groups(lst):
        out = []
        for i, k, d in lst:
            key = (i, np.float64(d).tobytes())
            if out and out[-1][0] == key:
                out[-1][1].add(k)
            else:
                out.append((key, {k}))
        return out
    return len(got) == len(want) and groups(got) == groups(want)


def cfmt(x):
    """std::to_string(double): "%f", with the x86 0.0 / 0.0 printing as -nan."""
    if isinstance(x, float) and math.isnan(x):
        return "-nan"
    return "%f" % x


def cdiv(a, b):
    if b == 0:
        return float("nan") if a == 0 else math.copysign(float("inf"), a)
    return a / b


SWAP = {"sum_single1": "sum_single2", "sum_single2": "sum_single1", "hets1": "hets2", "hets2": "hets1", "homs1": "homs2", "homs2": "homs1"}


def swap12(r):
    """An all-pairs record (min, max) seen from the other side: sample 1 <-> sample 2."""
    return {f: getattr(r, SWAP.get(f, f)) for f in FIELDS}


def expected_text(exe, tmp, files, dim, norm, rot, min_cov=1, thresh=0.5, all_=False, skew=0.2, genome=6200000000,
                  S=2.0, L=15.0, r=0.01, m1=0.01, m2=0.3):
    """computeScorePCA's stdout assembled from the restatement (cloud, pairs, calcDistance) and the oracle (genotype
    summaries, error rates, pair records, score)."""
    o = EvalOracle(files)
    n, m = o.n, o.m
    counts = o.counts()
    cloud, _, _ = rs_project(exe, tmp, counts, min_cov, norm, rot, dim)
    g = []
    for i in range(n):
        hets, homs, miss = o.genotype(i, min_cov)
        err = o.L.ntsm_eval_oracle_error_rate(o.h, i, genome)
        cov = o.L.ntsm_eval_oracle_total(o.h, i) / m
        pm = miss / m
        rad = S * S if (err < r and pm < m1) else (L * L if pm < m2 else DBL_MAX)
        g.append(dict(hets=hets, homs=homs, miss=miss, err=err, cov=cov, radius=rad))
    pairs = rs_candidates(exe, tmp, cloud, np.array([x["radius"] for x in g]))
    from oracle_binding import EvalPair
    out = [HEADER + "\n"]
    for i, k, dist in pairs:
        rec = o.pair(min(i, k), max(i, k), min_cov)
        d = swap12(rec) if i > k else {f: getattr(rec, f) for f in FIELDS}
        rr = EvalPair(**d)
        score = o.L.ntsm_eval_oracle_score(rr, g[i]["cov"], g[k]["cov"], skew)
        if not (all_ or score < thresh):
            continue
        relate = cdiv(float(d["shared_hets"]) - 2.0 * float(d["ibs0"]), float(min(d["hets1"], d["hets2"])))
        hc = cdiv(float(d["shared_homs"]) - 2.0 * float(d["ibs0"]), float(min(d["homs1"], d["homs2"])))
        same = ("1" if score < thresh else "0") if all_ else "1"
        cols = [files[i], files[k], cfmt(score), same, cfmt(dist), cfmt(relate), str(d["ibs0"]), str(d["ibs2"]), cfmt(hc),
                str(d["hets1"]), str(d["hets2"]), str(d["shared_hets"]), str(d["homs1"]), str(d["homs2"]), str(d["shared_homs"]),
                str(d["n_valid"]), cfmt(g[i]["cov"]), cfmt(g[k]["cov"]), cfmt(g[i]["err"]), cfmt(g[k]["err"]), str(g[i]["miss"]),
                str(g[k]["miss"]), str(g[i]["homs"]), str(g[k]["homs"]), str(g[i]["hets"]), str(g[k]["hets"])]
        out.append("\t".join(cols) + "\n")
    o.close()
    return "".join(out).encode(), cloud, g


def cohort(rng, n, m, missing=(0.0, 0.03, 0.2, 0.6)):
    """Related samples (random_samples) with a duplicate, an empty sample and a spread of missing-site fractions, so that
    the radii mix small, large and search-all."""
    s = random_samples(rng, n, m, depth=20.0)
    for i in range(n):
        f = missing[i % len(missing)]
        if f:
            s[i, rng.random(m) < f] = 0
    s[n - 1] = s[0]
    if n > 4:
        s[3] = 0
    return s


# ---------------------------------------------------------------------------------------------------- CPU
def test_x87_add_helper_matches_the_x87(tmp_path):
    """ntsm_x87_acc(acc, p) = RN53(RN64(acc + p)), bit for bit against g++'s long double on x86-64: 10^7 random operands
    plus constructed cases (ties at bit 64 and at bit 53 after RN64, exact cancellation, exponent gaps -130 ... +130, signed
    zeros, subnormal results, overflow) -- tests/xprec_check.cpp."""
    exe = gxx(tmp_path, "xprec_check.cpp", "xprec_check")
    p = subprocess.run([exe, "10000000", "7"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout[-2000:]
    assert int(p.stdout.split()[1]) > 10000000


def test_pca_cli_refusals_and_flag_errors(tmp_path):
    """The refusals exit 1 before any GPU work: -p without a readable -n file (the reference prints 'Error: Need
    normalization file' and then dies in an assert), -b with -p, fewer rotation rows / centre values than sites; -d beyond
    the rotation file's components and rows != centre values abort like the reference's asserts; a value that does not
    parse prints 'Error - Invalid parameter X' and returns 0; the help dialog lists the PCA flags."""
    rng = np.random.default_rng(5)
    files = files_for(tmp_path, random_samples(rng, 3, 40))
    norm, rot = write_pca(tmp_path, 40, 4, rng)
    run = lambda *a: subprocess.run([EVAL] + list(a), capture_output=True)   # noqa: E731
    p = run("-p", rot, *files)
    assert p.returncode == 1 and b"Error: Need normalization file" in p.stderr and b"not part of this build" in p.stderr and p.stdout == b""
    p = run("-p", rot, "-n", str(tmp_path / "none.txt"), files[0])
    assert p.returncode == 1 and b"Error: Need normalization file" in p.stderr
    p = run("-p", rot, "-n", norm, "-b", "truth.txt", *files)
    assert p.returncode == 1 and b"(-b) is not part of this build" in p.stderr and p.stdout == b""
    short = tmp_path / "short"
    short.mkdir()
    sn, sr = write_pca(short, 39, 4, rng)
    p = run("-p", sr, "-n", sn, "-d", "4", *files)
    assert p.returncode == 1 and b"fewer values than sites is not part of this build" in p.stderr and p.stdout == b""
    p = run("-p", rot, "-n", norm, "-d", "5", *files)                        # 4 components
    assert p.returncode in (-6, 134) and p.stdout == b""
    p = run("-p", rot, "-n", sn, "-d", "4", *files)                          # 40 rows, 39 values
    assert p.returncode in (-6, 134) and p.stdout == b""
    for flag in ("-d", "-r", "-1", "-2", "-S", "-l"):
        p = run(flag, "abc", "-p", rot, "-n", norm, *files)
        assert p.returncode == 0 and (b"Error - Invalid parameter %s: abc" % flag[1:].encode()) in p.stderr and p.stdout == b"", flag
    h = run("-h")
    assert h.returncode == 0
    for s in (b"-p, --pca = STR", b"-n, --norm = STR", b"-d, --dim = INT", b"[20]", b"-S, --small = FLOAT", b"[2.000000]", b"[15.000000]",
              b"-r, --error_rate", b"[0.300000]"):
        assert s in h.stderr, s
    p = run("-p", rot, "-n", norm, "-e", str(tmp_path / "m.txt"), "-o", *files)   # -o: merge only, no PCA (as the reference)
    assert p.returncode == 0 and p.stdout == b"" and os.path.exists(str(tmp_path / "m.txt"))


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
def test_projection_equals_restatement_bits(tmp_path, restatement):
    """m_cloud from ntsm_eval_project against the restatement's long double projection, compared by bits: N 2 / 65 / 300
    and 1,030 (five workgroups per component, the last with six live lanes), up to 96,287 sites, D 1 / 3 / 4 / 5 / 20,
    min_cov 0 / 1 / 3, samples without coverage, duplicated samples, centre and rotation values with 19-20 significant
    digits, a centre file longer than the site list and a line that does not parse."""
    import ntsm_amd.eval as ev
    rng = np.random.default_rng(21)
    for n, m, dim, c, extra, bad in ((2, 7, 1, 1, 0, False), (65, 1000, 3, 0, 5, True), (300, 2000, 20, 3, 0, False),
                                      (65, 3000, 5, 1, 0, False), (300, 500, 4, 1, 2, False), (65, 96287, 20, 1, 0, False),
                                      (1030, 60, 3, 1, 0, False)):
        d = tmp_path / ("p%d_%d_%d" % (n, m, dim))
        d.mkdir()
        s = cohort(rng, n, m)
        norm, rot = write_pca(d, m, dim + 1, rng, extra=extra, bad_line=bad)
        want, nv, rv = rs_project(restatement, d, s, c, norm, rot, dim)
        if bad:
            assert nv[1] == 0
        got, ms = ev.project(s, nv, rv, min_cov=c)
        assert got.shape == want.shape
        bad_idx = np.argwhere(got.view(np.uint64) != want.view(np.uint64))
        assert bad_idx.size == 0, (n, m, dim, c, bad_idx[:5].tolist(), got[tuple(bad_idx[0])], want[tuple(bad_idx[0])])
        if n > 4:
            assert np.array_equal(got[0].view(np.uint64), got[n - 1].view(np.uint64))
        assert ms >= 0


@pytest.mark.gpu
def test_candidates_equal_restatement(tmp_path, restatement):
    """ntsm_eval_candidates against the restatement's brute-force evalMetric selection: order, k and calcDistance bits,
    for radii that mix small, large and search-all samples (several radius scales and seeds); a buffer that is too small
    gets NTSM_EVAL_E_CAPACITY with the size needed.  N = 1,030: every row takes five passes of 256 partners, the last
    with six live lanes."""
    import ntsm_amd.eval as ev
    rng = np.random.default_rng(22)
    for n, m, dim in ((2, 50, 1), (65, 800, 5), (300, 1500, 20), (257, 400, 4), (120, 600, 3), (1030, 60, 3)):
        d = tmp_path / ("c%d" % n)
        d.mkdir()
        s = cohort(rng, n, m)
        norm, rot = write_pca(d, m, dim, rng)
        cloud, nv, rv = rs_project(restatement, d, s, 1, norm, rot, dim)
        diff = cloud[:, None, :] - cloud[None, :, :]
        dd = np.sqrt((diff * diff).sum(-1))[np.triu_indices(n, 1)]
        sess = ev.Session(s, 1)
        for q1, q2 in ((10, 40), (1, 5), (30, 90)):
            S, L = float(np.percentile(dd, q1)), float(np.percentile(dd, q2))
            radius = np.array([(S * S, L * L, DBL_MAX, L * L, S * S)[(i * 7 + q1) % 5] for i in range(n)])
            want = rs_candidates(restatement, d, cloud, radius)
            pi, pk, dist, ms = sess.candidates(cloud, radius)
            got = list(zip(pi.tolist(), pk.tolist(), dist.tolist()))
            assert same_list(got, want), (n, m, dim, q1, len(got), len(want))
            assert np.array_equal(np.array([w[2] for w in want]).view(np.uint64), dist.view(np.uint64))
            if len(want) > 1:
                with pytest.raises(ValueError) as e:
                    sess.candidates(cloud, radius, capacity=len(want) - 1)
                assert e.value.args[1] == len(want)
        sess.close()


@pytest.mark.gpu
def test_score_pairs_equal_all_pairs_records(tmp_path):
    """ntsm_eval_score_pairs on every pair in both orientations and on a random list with repeats: each record bit-equal
    to ntsm_eval_pairs' record of (min, max), with the 1 / 2 fields swapped when the first sample is the larger.  At
    N = 1,025 ntsm_eval_pairs runs its 256-thread tiles: the gather kernel (one lane per listed pair) and the tile kernel
    are two independent paths to the same record."""
    import ntsm_amd.eval as ev
    rng = np.random.default_rng(23)
    for n, m, c in ((2, 5, 1), (65, 3000, 1), (150, 1000, 3), (40, 96287, 0), (1025, 24, 1)):
        s = cohort(rng, n, m)
        rec, _ = ev.pairs(s, min_cov=c)
        sess = ev.Session(s, c)
        ii, kk = np.triu_indices(n, 1)
        rnd_i = rng.integers(0, n, size=3000)
        rnd_k = (rnd_i + rng.integers(1, n, size=3000)) % n
        for pi, pk in ((ii, kk), (kk, ii), (rnd_i, rnd_k)):
            got, _ = sess.score_pairs(pi, pk)
            lo, hi = np.minimum(pi, pk).astype(np.int64), np.maximum(pi, pk).astype(np.int64)
            w = rec[ev.pair_index(lo, hi, n)]
            assert len(got) == len(pi)
            for f in FIELDS:
                want = np.where(pi > pk, w[SWAP.get(f, f)], w[f])
                bits = np.uint64 if f.startswith("sum") else want.dtype
                ne = np.flatnonzero(np.ascontiguousarray(got[f]).view(bits) != want.view(bits))
                assert ne.size == 0, (n, c, f, [(int(pi[p]), int(pk[p]), got[f][p], want[p]) for p in ne[:5]])
        sess.close()


NO_DEVICE = 1 << 20                              # a device ordinal that no machine has: hipSetDevice refuses it (an API error)


def zero_records(count):
    import ntsm_amd.eval as ev
    return np.zeros(count, dtype=ev.RECORD).tobytes()


@pytest.mark.gpu
def test_eval_entry_points_return_early_on_degenerate_shapes():
    """Every entry point of include/ntsm_eval_hip.h on the shapes it answers without a kernel: one sample (no pair), no
    site (all-zero records, a +0.0 cloud), an empty pair list; a listed pair that names a sample twice or a sample that
    does not exist is refused with -1 and the session goes on scoring, bit-equal to ntsm_eval_pairs."""
    import ctypes as C
    import ntsm_amd.eval as ev
    rec, _ = ev.pairs(np.zeros((1, 5, 2), dtype=np.uint32))
    assert len(rec) == 0
    rec, _ = ev.pairs(np.zeros((3, 0, 2), dtype=np.uint32))
    assert len(rec) == 3 and rec.tobytes() == zero_records(3)

    sess = ev.Session(np.full((1, 5, 2), 7, dtype=np.uint32))
    pi, pk, dist, _ = sess.candidates(np.zeros((1, 2)), np.array([DBL_MAX]))
    assert len(pi) == 0 and len(pk) == 0 and len(dist) == 0
    got, _ = sess.score_pairs([], [])
    assert len(got) == 0
    sess.close()

    sess = ev.Session(np.zeros((3, 0, 2), dtype=np.uint32))
    cloud = np.full((3, 2), np.nan)
    norm, rot = np.zeros(1, dtype=np.longdouble), np.zeros(2, dtype=np.longdouble)      # no site: neither is read
    assert ev.lib.ntsm_eval_project(sess.h, ev._ld_ptr(norm), ev._ld_ptr(rot), 2, cloud.ctypes.data, C.byref(C.c_double())) == 0
    assert cloud.tobytes() == np.zeros((3, 2)).tobytes()                                # +0.0, by the bits
    got, _ = sess.score_pairs([0, 2], [1, 0])
    assert len(got) == 2 and got.tobytes() == zero_records(2)
    sess.close()

    s = cohort(np.random.default_rng(24), 3, 4)
    want, _ = ev.pairs(s)
    sess = ev.Session(s)
    for pi, pk in (([1], [1]), ([0], [3])):
        with pytest.raises(RuntimeError, match=r"failed: -1$"):
            sess.score_pairs(pi, pk)
        got, _ = sess.score_pairs([0], [1])
        assert got.tobytes() == want[:1].tobytes()
    sess.close()


@pytest.mark.gpu
def test_eval_reports_a_refused_device_and_works_afterwards():
    """ntsm_eval_pairs and ntsm_eval_open on a device ordinal that does not exist return -2 (hipSetDevice's error, no
    device fault), and the next calls on device 0 give the record of py_pair for 2 samples x 3 sites."""
    import ntsm_amd.eval as ev
    s = np.array([[[9, 0], [4, 5], [0, 0]], [[0, 8], [6, 3], [7, 7]]], dtype=np.uint32)
    with pytest.raises(RuntimeError, match=r"ntsm_eval_pairs failed: -2$"):
        ev.pairs(s, device=NO_DEVICE)
    with pytest.raises(RuntimeError, match=r"ntsm_eval_open failed: -2$"):
        ev.Session(s, device=NO_DEVICE)
    want = py_pair(s[0], s[1], 1)
    assert want["n_valid"] == 2 and want["ibs0"] == 1 and want["shared_hets"] == 1
    rec, _ = ev.pairs(s)
    sess = ev.Session(s)
    got, _ = sess.score_pairs([0], [1])
    sess.close()
    for r in (rec, got):
        assert len(r) == 1
        for f in FIELDS:
            assert same_bits(r[f][0], want[f]) if f.startswith("sum") else int(r[f][0]) == want[f], (f, r[f][0], want[f])


@pytest.mark.gpu
def test_cli_pca_equals_expected_bytes(tmp_path, restatement):
    """build/ntsmEval -p ROT -n NORM: stdout byte-equal to the text assembled from the restatement and the oracle, with
    and without -a, -d 5, other -S / -l / -r / -1 / -2 / -s / -c / -w; one file with -p prints the QC table with its PC
    columns; all-pairs output is unchanged (dist -1)."""
    rng = np.random.default_rng(24)
    n, m = 40, 3000
    s = cohort(rng, n, m)
    files = files_for(tmp_path, s)
    norm, rot = write_pca(tmp_path, m, 22, rng)
    cloud, _, _ = rs_project(restatement, tmp_path, s, 1, norm, rot, 20)
    diff = cloud[:, None, :] - cloud[None, :, :]
    dd = np.sqrt((diff * diff).sum(-1))[np.triu_indices(n, 1)]
    S, L = repr(float(np.percentile(dd, 15))), repr(float(np.percentile(dd, 60)))
    cases = [dict(args=[], kw={}), dict(args=["-a"], kw=dict(all_=True)),
             dict(args=["-a", "-d", "5"], kw=dict(all_=True, dim=5)),
             dict(args=["-S", S, "-l", L, "-r", "1", "-1", "0.05", "-2", "0.5"], kw=dict(S=float(S), L=float(L), r=1.0, m1=0.05, m2=0.5)),
             dict(args=["-a", "-S", S, "-l", L, "-r", "1", "-1", "0.1", "-2", "0.7", "-s", "0.3", "-w", "0", "-c", "2", "-t", "4"],
                  kw=dict(all_=True, S=float(S), L=float(L), r=1.0, m1=0.1, m2=0.7, thresh=0.3, skew=0.0, min_cov=2))]
    for case in cases:
        kw = dict(case["kw"])
        dim = kw.pop("dim", 20)
        want, _, g = expected_text(restatement, tmp_path, files, dim, norm, rot, **kw)
        p = subprocess.run([EVAL, "-p", rot, "-n", norm] + case["args"] + files, capture_output=True)
        assert p.returncode == 0, (case["args"], p.stderr[-500:])
        assert p.stdout == want, (case["args"], p.stdout[:300], want[:300])
        assert want.count(b"\n") >= 2, case["args"]
    assert len({x["radius"] for x in g}) == 3                                # the last case mixes all three radii
    # one file: the QC table with PC1 ... PC20
    o = EvalOracle(files[:1])
    one = subprocess.run([EVAL, "-p", rot, "-n", norm, files[0]], capture_output=True)
    hets, homs, miss = o.genotype(0, 1)
    row = [files[0], cfmt(o.L.ntsm_eval_oracle_total(o.h, 0) / m), cfmt(o.L.ntsm_eval_oracle_error_rate(o.h, 0, 6200000000)),
           str(miss), str(homs), str(hets)] + [cfmt(v) for v in cloud[0]]
    head = "sample\tcov\terrorRate\tmiss\thom\thet" + "".join("\tPC%d" % d for d in range(1, 21))
    assert one.returncode == 0 and one.stdout == (head + "\n" + "\t".join(row)).encode()
    o.close()
    plain = subprocess.run([EVAL, "-a"] + files, capture_output=True).stdout    # all-pairs: dist stays -1
    assert plain.count(b"\n") == 1 + n * (n - 1) // 2 and all(l.split(b"\t")[4] == b"-1" for l in plain.splitlines()[1:])


@pytest.mark.gpu
def test_cli_pca_tool_chain(tmp_path, restatement):
    """The whole chain: counts files printed by build/ntsmCount for related and unrelated 'individuals', then
    ntsmEval -a -p ROT -n NORM, byte-equal to the expected text."""
    import ntsm_amd as nt
    rng = np.random.default_rng(25)
    sp = str(tmp_path / "sites.fa")
    nt.SynthShort(sites_seed=5, n_sites=2000, read_seed=1, p_embed=0.9, sites_path=sp)
    outs = []
    for i, (seed, emb) in enumerate(((1, 0.9), (2, 0.9), (3, 0.5), (4, 0.9))):
        fq, out = str(tmp_path / ("r%d.fq" % i)), str(tmp_path / ("c%d.txt" % i))
        nt.SynthShort(sites_seed=5, n_sites=2000, read_seed=seed, p_embed=emb).write_fastq(fq, 0, 60000)
        with open(out, "wb") as fh:
            subprocess.run([os.path.join(ROOT, "build", "ntsmCount"), "-s", sp, fq], stdout=fh, stderr=subprocess.DEVNULL, check=True)
        outs.append(out)
    m = EvalOracle(outs[:1]).m
    norm, rot = write_pca(tmp_path, m, 20, rng)
    for args, kw in (([], dict(all_=True)), (["-d", "5", "-S", "0.01", "-l", "0.05"], dict(all_=True, dim=5, S=0.01, L=0.05))):
        kw = dict(kw)
        dim = kw.pop("dim", 20)
        want, _, _ = expected_text(restatement, tmp_path, outs, dim, norm, rot, **kw)
        p = subprocess.run([EVAL, "-a", "-p", rot, "-n", norm] + args + outs, capture_output=True)
        assert p.returncode == 0 and p.stdout == want and want.count(b"\n") >= 1, (args, p.stderr[-300:])
