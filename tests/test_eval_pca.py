"""ntsmEval's PCA-guided pair search (-p / -n): ntsm_amd/csrc/xprec.h, the session calls of include/ntsm_eval_hip.h
(ntsm_eval_project, ntsm_eval_candidates, ntsm_eval_score_pairs) and build/ntsmEval -p.

PARITY WITH THE REFERENCE is pinned in tests/test_eval_reference.py, as for the all-pairs path: expected_text below and
build/ntsmEval -p against projectPCs + computeScorePCA of the unmodified CompareCounts.hpp (oracle/_ref/ref_ntsmEval) and
its recordings, byte for byte.  What the tests of this file pin is (CPU) the integer x87 add against the x87 itself, and the
CLI's refusals and flag errors; (GPU) the projection and the candidate list against tests/eval_pca_restatement.cpp, an
independent restatement written from the reference text and compiled here with real long double, the listed-pair scoring
against ntsm_eval_pairs, and the CLI's stdout against text assembled from the restatement and the all-pairs oracle
(oracle/ntsm_eval_oracle.c).  The rotation files of write_pca keep the x87 add in a narrow regime (small exponent gaps, no
cancellation, carry, underflow or overflow), so the device build of the add also gets the operand classes of
tests/xprec_check.cpp as table entries, against real x87 arithmetic, and the candidate search gets hand-made clouds at the
edges of the double range."""
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


# ---------------------------------------------------------------------------------------------------- the x87 add's operand classes
# tests/xprec_check.cpp writes its cases; the GPU test feeds them to ntsm_eval_project, whose lane (sample i, component d)
# computes ntsm_x87_acc over the sites that sample i covers: with norm = 0 and a site called 1.0 the table entry is rot[d][j]
# itself, so the sites (lead-in, acc, p) give ntsm_x87_acc(ntsm_x87_acc(lead-in result, acc), p).
X87_RECORD = np.dtype([("acc", "<f8"), ("p", np.longdouble), ("want", "<f8")])
X87_PER_CLASS = 2000
X87_NOT_DUMPED = "nan_acc"                       # no finite table entry leads to a NaN accumulator: the host check alone has that class
X87_BRANCHES = {"p_zero", "acc_zero", "swap", "subtraction", "gap_ge_64", "gap_ge_128", "exact_cancellation", "shift_ge_64", "shift_gt_64", "rn64_tie",
                "rn64_carry_out", "rn53_tie_after_rn64", "subnormal_result", "underflow_to_zero", "overflow", "nonfinite_acc"}
COVERED, HALF, MISSING_SITE = (5, 0), (5, 5), (0, 0)        # counts that min_cov = 1 calls 1.0, 0.5 and missing


def parse_x87_report(text):
    """The "class NAME COUNT" and "branch NAME COUNT" lines of xprec_check as two dicts (classes in the file's order)."""
    classes, branches = {}, {}
    for line in text.splitlines():
        w = line.split()
        if len(w) == 3 and w[0] in ("class", "branch"):
            (classes if w[0] == "class" else branches)[w[1]] = int(w[2])
    return classes, branches


@pytest.fixture(scope="module")
def x87_cases(tmp_path_factory):
    """(records, class of each record, classes, branches) of `xprec_check dump FILE X87_PER_CLASS 7`, built and run once."""
    d = tmp_path_factory.mktemp("x87")
    exe = gxx(d, "xprec_check.cpp", "xprec_check")
    p = subprocess.run([exe, "dump", str(d / "cases.bin"), str(X87_PER_CLASS), "7"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout[-2000:]
    print(p.stdout)
    classes, branches = parse_x87_report(p.stdout)
    rec = np.fromfile(str(d / "cases.bin"), dtype=X87_RECORD)
    return rec, np.repeat(np.arange(len(classes)), list(classes.values())), classes, branches


def assert_x87_is_numpy_longdouble():
    """numpy's long double is the x87 format and its sums round twice: to 64 bits, then to the double."""
    assert X87_RECORD.itemsize == 32 and np.finfo(np.longdouble).nmant == 63
    witness = np.float64(np.longdouble(1.0) + (np.longdouble(2.0) ** -53 + np.longdouble(2.0) ** -64))
    assert witness.view(np.uint64) == np.float64(1.0).view(np.uint64)
    assert np.float64(1.0) + np.float64(2.0 ** -53 + 2.0 ** -64) == np.float64(1.0000000000000002)


def x87_fold(v, rot):
    """The reference's projection in real x87 arithmetic: v double [n][m] (call - norm, or +0.0 for a missing site), rot long
    double [dim][m]; acc = double(acc + (long double) v[j] * rot[d][j]) in site order, a store to double after every add."""
    acc = np.zeros((v.shape[0], rot.shape[0]), dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(v.shape[1]):
            prod = v[:, j, None].astype(np.longdouble) * rot[None, :, j]
            acc = (acc.astype(np.longdouble) + prod).astype(np.float64)
    return acc


def x87_chain(*entries):
    """x87_fold of one lane over sites called 1.0 with norm = 0: the table entries are rot's values themselves."""
    acc = np.zeros(entries[0].shape, dtype=np.float64)
    with np.errstate(all="ignore"):
        for e in entries:
            acc = (acc.astype(np.longdouble) + e).astype(np.float64)
    return acc


def x87_sites(cases):
    """The three table entries (lead-in, acc, p) whose chain from +0.0 is the case, as long doubles shaped like `cases`: a
    lead-in of +0 leaves +0; acc = -0.0 needs the lead-in -2^-1100, which rounds to -0.0 where (+0) + (-0) would give +0; an
    infinite acc is reached as the overflow of 1.7e308 + 1.7e308 of its sign."""
    acc = cases["acc"]
    lead = np.zeros(acc.shape, dtype=np.longdouble)
    site = acc.astype(np.longdouble)
    lead[(acc == 0) & np.signbit(acc)] = -np.longdouble(2.0) ** -1100
    big = np.copysign(1.7e308, acc[np.isinf(acc)]).astype(np.longdouble)
    lead[np.isinf(acc)], site[np.isinf(acc)] = big, big
    assert np.isfinite(lead).all() and np.isfinite(site).all() and np.isfinite(cases["p"]).all()
    return lead, site, cases["p"]


def x87_block_layout(cases, n, dim):
    """Sample i is covered at its own sites 3 i ... 3 i + 2 alone, and lane (i, d) runs case i * dim + d there; every other
    site is missing for it, a product of +-0 with the sign of rot.  Returns (counts, rot, expected, cases): expected is the
    fold of the lane's own three sites, and where that is a zero, of the zeros that follow: -0 survives only -0 products;
    cases [n][dim] are the records as the lanes got them (the input repeated where it is shorter than n * dim)."""
    cases = np.resize(cases, n * dim).reshape(n, dim)
    counts = np.zeros((n, 3 * n, 2), dtype=np.uint32)
    for s in range(3):
        counts[np.arange(n), 3 * np.arange(n) + s] = COVERED
    sites = x87_sites(cases)
    rot = np.ascontiguousarray(np.stack(sites, axis=-1).transpose(1, 0, 2).reshape(dim, 3 * n))
    own = x87_chain(*sites)
    neg_tail = np.ones((dim, 3 * n + 3), dtype=bool)                          # neg_tail[d][j]: every site from j on has a negative rot
    neg_tail[:, :3 * n] = np.logical_and.accumulate(np.signbit(rot)[:, ::-1], axis=1)[:, ::-1]
    stays_negative = np.signbit(own) & neg_tail[:, 3 * np.arange(1, n + 1)].T
    expected = np.where(own == 0, np.where(stays_negative, -0.0, 0.0), own)
    return counts, rot, expected, cases


def x87_wave_layout(cases, n, rng):
    """Every sample is covered at the same three sites, called 1.0 or 0.5 (sample 0: 1.0 throughout), and component d is case
    d: all lanes of a wave run the full add at once, on operands that differ by factors of two.  expected is each lane's own
    fold."""
    call = rng.integers(1, 3, size=(n, 3))
    call[0] = 2
    counts = np.where((call == 2)[:, :, None], np.array(COVERED, dtype=np.uint32), np.array(HALF, dtype=np.uint32)).astype(np.uint32)
    rot = np.ascontiguousarray(np.stack(x87_sites(cases), axis=-1))
    return counts, rot, x87_fold(call * 0.5, rot)


def same_double_bits(got, want):
    """Bit for bit; a NaN only has to be a NaN."""
    both_nan = np.isnan(got) & np.isnan(want)
    return (got.view(np.uint64) == want.view(np.uint64)) | both_nan


# ---------------------------------------------------------------------------------------------------- CPU
def test_x87_add_helper_matches_the_x87(tmp_path):
    """ntsm_x87_acc(acc, p) = RN53(RN64(acc + p)), bit for bit against g++'s long double on x86-64: 10^7 random operands
    plus constructed cases (ties at bit 64 and at bit 53 after RN64, exact cancellation, exponent gaps -130 ... +130, signed
    zeros, subnormal results, overflow, a carry out of the RN64 increment, an accumulator that is already infinite or NaN) --
    tests/xprec_check.cpp.  The program counts the branches of ntsm_x87_acc that its cases take and fails on one that none
    takes."""
    exe = gxx(tmp_path, "xprec_check.cpp", "xprec_check")
    p = subprocess.run([exe, "10000000", "7"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout[-2000:]
    assert int(p.stdout.split()[1]) > 12000000
    classes, branches = parse_x87_report(p.stdout)
    assert X87_BRANCHES <= set(branches) and all(v > 0 for v in branches.values()), branches
    assert len(classes) == 13 and all(v >= 200 for v in classes.values()), classes


def test_x87_add_helper_under_the_host_sanitizers():
    """tests/xprec_check.cpp as `make xprec_check` builds it, a program of its own under -fsanitize=address,undefined: every
    constructed class and 10^6 random operands, run once."""
    subprocess.run(["make", "-s", "build/xprec_check"], cwd=ROOT, check=True, stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(ROOT, "build", "xprec_check"), "1000000", "7"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok ") and p.stderr == "", (p.stdout[-600:], p.stderr[-600:])
    assert int(p.stdout.split()[1]) > 3000000


def test_x87_dumped_cases_cover_every_class_and_branch(x87_cases):
    """The conditions on the input of test_projection_runs_the_x87_add_on_every_operand_class, without a device: every class
    but NaN gives at least 1,000 cases, the written cases alone take every branch, numpy's long double folds every case's
    three sites to the x87's own result, and the block layout's expected values are the fold of the whole site sequence."""
    rec, cls, classes, branches = x87_cases
    assert_x87_is_numpy_longdouble()
    dumped = {k: v for k, v in classes.items() if k != X87_NOT_DUMPED}
    assert classes[X87_NOT_DUMPED] == 0 and len(dumped) == 12 and min(dumped.values()) >= 1000, classes
    assert len(rec) == sum(dumped.values()) == len(cls)
    assert X87_BRANCHES <= set(branches) and all(v > 0 for v in branches.values()), branches
    assert not np.isnan(rec["acc"]).any() and np.isinf(rec["acc"]).sum() >= 1000
    chain = x87_chain(*x87_sites(rec))
    bad = np.flatnonzero(chain.view(np.uint64) != rec["want"].view(np.uint64))
    assert bad.size == 0, (bad[:5].tolist(), rec[bad[:5]], chain[bad[:5]])
    zeros, spread = np.flatnonzero(rec["want"] == 0)[:150], np.arange(0, len(rec), 97)
    for n, dim in ((37, 11), (5, 60)):                                       # zero results with a tail, and in the last sample without
        counts, rot, expected, cases = x87_block_layout(rec[np.concatenate([spread[:n * dim - 150], zeros])], n, dim)
        v = np.where(counts[:, :, 0] > 0, 1.0, 0.0)
        assert np.array_equal(x87_fold(v, rot).view(np.uint64), expected.view(np.uint64))
        assert np.array_equal(expected[-1].view(np.uint64), cases["want"][-1].view(np.uint64))     # the last sample has no tail
        nz = cases["want"] != 0
        assert np.array_equal(expected[nz].view(np.uint64), cases["want"][nz].view(np.uint64))
        assert (np.signbit(expected) & (expected == 0)).any() and ((expected == 0) & np.signbit(cases["want"]) & ~np.signbit(expected)).any()


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
def test_projection_runs_the_x87_add_on_every_operand_class(x87_cases):
    """The device build of ntsm_x87_acc on the operand classes that no rotation file of the other tests reaches: the cases
    that tests/xprec_check.cpp dumps (12 classes of 2,000: signed zeros, cancellation, exponent gaps to +-130, ties at bit 64
    and at bit 53 after RN64, subnormal results, overflow, the carry out of the RN64 increment, an infinite accumulator,
    four random kinds; every branch of the function taken) through ntsm_eval_project, compared by bits with real x87
    arithmetic -- the dumped result, which is g++'s long double, and numpy's long double fold of each lane's sites.
    Block layout: lane (i, d) meets its case at sample i's own three sites and +-0 products elsewhere, so the lanes of a
    wave take different branches at one step; n = 256, 300 (a second workgroup of 44 lanes) and 65.  Wave layout: all
    samples covered at the same three sites with calls 1.0 or 0.5, so every lane of a wave runs the full add at once; n = 70
    (a wave of six live lanes) and 257."""
    import ntsm_amd.eval as ev
    rec, cls, classes, branches = x87_cases
    assert_x87_is_numpy_longdouble()
    names = list(classes)
    print({k: v for k, v in branches.items()})
    assert classes[X87_NOT_DUMPED] == 0 and all(v >= 1000 for k, v in classes.items() if k != X87_NOT_DUMPED), classes
    assert X87_BRANCHES <= set(branches) and all(v > 0 for v in branches.values()), branches
    compared, first = 0, 0
    plan = [(256, 64), (300, 24), (65, 8)]
    while first < len(rec):
        n, dim = plan[0]
        plan = plan[1:] + plan[:1]
        idx = np.resize(np.arange(first, min(first + n * dim, len(rec))), n * dim).reshape(n, dim)
        counts, rot, expected, cases = x87_block_layout(rec[idx.ravel()], n, dim)
        got, _ = ev.project(counts, np.zeros(3 * n, dtype=np.longdouble), rot, min_cov=1)
        bad = np.argwhere(~same_double_bits(got, expected))
        assert bad.size == 0, ("block", n, dim, [(names[cls[idx[i, d]]], cases[i, d], got[i, d], expected[i, d]) for i, d in bad[:5]])
        last_or_nonzero = (cases["want"] != 0) | (np.arange(n) == n - 1)[:, None]          # no tail of zeros changes these
        assert np.array_equal(got[last_or_nonzero].view(np.uint64), cases["want"][last_or_nonzero].view(np.uint64))
        compared += min(n * dim, len(rec) - first)
        first += n * dim
    assert compared == len(rec)
    rng = np.random.default_rng(26)
    for n, pick in ((70, np.arange(len(rec))), (257, np.arange(0, len(rec), 5))):
        counts, rot, expected = x87_wave_layout(rec[pick], n, rng)
        got, _ = ev.project(counts, np.zeros(3, dtype=np.longdouble), rot, min_cov=1)
        assert got.shape == expected.shape == (n, len(pick))
        bad = np.argwhere(~same_double_bits(got, expected))
        assert bad.size == 0, ("wave", n, [(names[cls[pick[d]]], rec[pick[d]], counts[i, :, 1].tolist(), got[i, d], expected[i, d]) for i, d in bad[:5]])
        assert np.array_equal(got[0].view(np.uint64), rec["want"][pick].view(np.uint64))    # sample 0 is the case itself


def edge_cloud(rng, n, dim, families):
    """A finite cloud at the edges of the double range, one family per row: 0 coordinates near +-1e200 (their squares
    overflow), 1 +-DBL_MAX (the subtraction itself overflows), 2 near +-1e-200 with some near 1e-160 (squares that underflow
    to zero or to a subnormal), 3 signed zeros, 4 ordinary values, 5 a coordinate of each kind."""
    def coords(f, size):
        sign = rng.choice([-1.0, 1.0], size=size)
        return {0: sign * rng.integers(1, 10, size=size) * 1e200,
                1: sign * DBL_MAX,
                2: sign * rng.integers(1, 4, size=size) * np.where(rng.random(size) < 0.2, 1e-160, 1e-200),
                3: sign * 0.0,
                4: rng.integers(-3, 4, size=size) * 0.5}[f]
    cloud = np.empty((n, dim))
    for i in range(n):
        f = families[i % len(families)]
        cloud[i] = coords(f, dim) if f < 5 else [coords(int(g), 1)[0] for g in rng.integers(0, 5, size=dim)]
    assert np.isfinite(cloud).all()
    return cloud


@pytest.mark.gpu
def test_candidates_at_the_edges_of_the_double_range(tmp_path, restatement):
    """eval_metric, calc_distance and the selection on hand-made finite clouds against the restatement, order, k and the bits
    of dist: squares and differences that overflow (metric +inf: a radius row takes nothing, a search-all row everything with
    dist inf), squares that underflow (exact ties at metric 0, ordered by k, and subnormal metrics), +0.0 against -0.0, and
    ordinary values among them; dim 1 / 3 / 4 / 5 / 8 (the four-wide loop and its tail), n 2 / 65 / 257, radii that mix
    finite values down to 1e-300 with DBL_MAX."""
    import ntsm_amd.eval as ev
    rng = np.random.default_rng(27)
    seen_inf = seen_zero = seen_subnormal = 0
    for n in (2, 65, 257):
        sess = ev.Session(np.full((n, 1, 2), 7, dtype=np.uint32), 1)
        for dim in (1, 3, 4, 5, 8):
            for families in ([(0,), (1,), (2,), (3,), (0, 1), (2, 3), (4, 0)] if n == 2 else [(0, 1, 2, 3, 4, 5, 2, 3, 2)]):
                cloud = edge_cloud(rng, n, dim, families)
                if families == (1,):
                    cloud[1] = -cloud[0]                                     # DBL_MAX against -DBL_MAX in every coordinate
                if families == (3,):
                    cloud[1] = -cloud[0]                                     # +0.0 against -0.0
                for radii in ((DBL_MAX, 1.0, 1e-300, 4.0, 1e300, 1e-300, DBL_MAX), (1e-300, 1e300), (DBL_MAX,)):
                    radius = np.array([radii[(i * 5 + dim) % len(radii)] for i in range(n)])
                    want = rs_candidates(restatement, tmp_path, cloud, radius)
                    pi, pk, dist, _ = sess.candidates(cloud, radius)
                    got = list(zip(pi.tolist(), pk.tolist(), dist.tolist()))
                    assert same_list(got, want), (n, dim, families, radii, len(got), len(want), got[:5], want[:5])
                    assert np.array_equal(np.array([w[2] for w in want], dtype=np.float64).view(np.uint64), dist.view(np.uint64))
                    seen_inf += int(np.isinf(dist).sum())
                    seen_zero += int((dist == 0).sum())
                    seen_subnormal += int(((dist > 0) & (dist < 2.2250738585072014e-308)).sum())
        sess.close()
    assert seen_inf > 1000 and seen_zero > 1000 and seen_subnormal > 100, (seen_inf, seen_zero, seen_subnormal)


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
