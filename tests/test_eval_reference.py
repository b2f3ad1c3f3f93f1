"""ntsmEval held to the reference's own scoring class: oracle/_ref/ref_ntsmEval is the UNMODIFIED src/CompareCounts.hpp,
#included where it lies by oracle/ref_eval_driver.cpp (the empty oracle/ref_config/config.h resolves the one include of
vendor/kfunc.c that kept it from compiling), replaying the calls of src/ntSeqMatchEval.cpp:276-341.  Its stdout at -t 1 is the
yardstick; with more threads the reference prints the same lines in another order.

CPU: the driver restates nothing of the class; the oracle CLI (oracle/ntsm_eval_oracle.c) and the PCA text assembled from
tests/eval_pca_restatement.cpp (test_eval_pca.expected_text) against the reference binary, byte for byte; both against the
recordings of tests/golden/eval/ (tests/golden/make_eval.py), which also hold where the binary is absent.
GPU: build/ntsmEval against the reference binary (it travels prebuilt; nothing here reads the reference tree) and against
the recordings, byte for byte, all pairs and -p / -n.

No comparison has a tolerance.  The one relaxation: on the cohort with a planted duplicate, rows of one sample1 that print the
same distance are compared as a set (exact distance ties come out of the reference in kd-tree order, out of the product by k).
"""
import contextlib
import gzip
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle_binding import EvalOracle, ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_eval  # noqa: E402
from test_eval import random_samples, write_counts  # noqa: E402
from test_eval_pca import cfmt, cohort, expected_text, gxx, rs_project, write_pca  # noqa: E402

EVAL = os.path.join(ROOT, "build", "ntsmEval")
ORACLE_CLI = os.path.join(ROOT, "oracle", "ntsm_eval_oracle")
REF_EVAL = os.path.join(ROOT, "oracle", "_ref", "ref_ntsmEval")
DRIVER = os.path.join(ROOT, "oracle", "ref_eval_driver.cpp")
GOLD = os.path.join(ROOT, "tests", "golden", "eval")
RECORDED = json.load(open(os.path.join(GOLD, "cases.json")))["cases"]
HAVE_REF_TREE = os.path.isdir("/root/reference/src")
need_ref = pytest.mark.skipif(not os.path.isfile(REF_EVAL), reason="oracle/_ref/ref_ntsmEval not built (no reference tree here)")
PCA = ["-p", "rot.tsv", "-n", "norm.txt"]


def stdout_of(exe, args, names, d):
    p = subprocess.run([exe] + list(args) + list(names), cwd=str(d), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, (os.path.basename(exe), args, p.returncode, p.stderr[-500:])
    return p.stdout


def reference(args, names, d):
    return stdout_of(REF_EVAL, ["-t", "1"] + list(args), names, d)


@contextlib.contextmanager
def inside(d):
    """expected_text and EvalOracle open the files by the names that get printed: relative ones, from the data directory"""
    here = os.getcwd()
    os.chdir(str(d))
    try:
        yield
    finally:
        os.chdir(here)


# ---------------------------------------------------------------------------------------------------- cohorts
def write_loader_cohort(d):
    """Four files over 50 loci that the reference's reader treats differently: the first fixes the loci; the second lists
    them in another order; the third lacks a locus (it stays 0) and has no column-header line; the fourth has neither order
    nor header and lacks three.  #@KS is 19 in all of them and no file names a locus the first does not have (the reference
    asserts on both)."""
    rng = np.random.default_rng(15)
    s = random_samples(rng, 4, 50)
    loci = ["rs%d" % (7 * j + 3) for j in range(50)]
    names = []
    for i, (keep, header) in enumerate(((np.arange(50), True), (rng.permutation(50), True), (np.delete(np.arange(50), 17), False),
                                        (rng.permutation(50)[3:], False))):
        names.append("l%d.txt" % i)
        write_counts(os.path.join(str(d), names[-1]), s[i][keep], loci=[loci[j] for j in keep], header=header, tk=1000 + i)
    return names


def wrapped_samples(rng, n, m):
    """make_eval.spread with one sample whose counts sit at and beyond 2^31 in both columns: in projectPCs
    (src/CompareCounts.hpp:179-198) `unsigned denom = countAT + countCG` wraps -- to 0 at (2^31, 2^31), which makes the site
    missing, and to a small number elsewhere, which makes the frequency huge and the call 1.0 -- and in the pair score the
    joint counts wrap likewise."""
    s = make_eval.spread(rng, n, m)
    big = 1 << 31
    s[2, 0:10] = [big, big]
    s[2, 10:20] = [big + 5, big + 7]
    s[2, 20:30] = [3000000000, 2000000000]
    s[2, 30:40] = [big - 1, big + 1]
    s[2, 40:50] = [big + 9, 4]
    return s


class Cohorts:
    """Each cohort is written once per module into its own directory; names are relative to it."""

    def __init__(self, factory):
        self.factory, self.made = factory, {}

    def get(self, key):
        if key not in self.made:
            d = self.factory.mktemp(key)
            self.made[key] = (d,) + getattr(self, "make_" + key.split(":")[0])(d, *key.split(":")[1:])
        return self.made[key]

    def make_random(self, d, seed, n, m, depth="8"):
        s = random_samples(np.random.default_rng(int(seed)), int(n), int(m), depth=float(depth))
        return make_eval.write_cohort(str(d), s), s

    def make_edge(self, d):
        s = make_eval.edge_samples()
        return make_eval.write_cohort(str(d), s), s

    def make_loader(self, d):
        return write_loader_cohort(d), None

    def make_spread(self, d, seed, n, m, components):
        """a tie-free PCA cohort: (samples, names) + norm.txt / rot.tsv"""
        s, names = make_eval.materialise(dict(kind="pca", seed=int(seed), n=int(n), m=int(m), components=int(components)), str(d))
        return names, s

    def make_duplicate(self, d):
        """the cohort of test_eval_pca.test_cli_pca_equals_expected_bytes: s[n - 1] = s[0], 40 x 3,000, 22 components"""
        rng = np.random.default_rng(24)
        s = cohort(rng, 40, 3000)
        names = make_eval.write_cohort(str(d), s)
        write_pca(d, 3000, 22, rng)
        return names, s

    def make_wrapped(self, d):
        rng = np.random.default_rng(34)
        s = wrapped_samples(rng, 20, 120)
        names = make_eval.write_cohort(str(d), s)
        write_pca(d, 120, 4, rng)
        return names, s


@pytest.fixture(scope="module")
def cohorts(tmp_path_factory):
    return Cohorts(tmp_path_factory)


@pytest.fixture(scope="module")
def restatement(tmp_path_factory):
    return gxx(tmp_path_factory.mktemp("rs"), "eval_pca_restatement.cpp", "eval_pca_restatement")


R12, R65, R257, WIDE = "random:12:12:3000", "random:65:65:1000", "random:257:257:200", "random:13:1030:30:30"
R12_SETS = [[], ["-a"], ["-a", "-s", "0.1", "-w", "0", "-c", "2"], ["-s", "5", "-g", "3100000000", "-w", "0.5"], ["-a", "-c", "0"],
            ["-a", "-c", "3", "-w", "1"]]
EDGE_SETS = [["-a", "-c", "0"], ["-a", "-c", "5"], ["-a", "-w", "-0.5"], ["-a", "-w", "2"], ["-s", "-1"], ["-a", "-s", "-1"],
             ["-a", "-g", "1000"], ["-g", "1000", "-s", "3"]]
CPU_PAIRS = ([(R12, a) for a in R12_SETS] + [("edge", a) for a in EDGE_SETS] + [(R65, ["-a"]), (R65, ["-s", "1.5"]),
             ("loader", ["-a"]), ("loader", ["-a", "-c", "0"])])
GPU_PAIRS = ([(R12, a) for a in R12_SETS[:4]] + [(R65, ["-a"]), (R257, ["-a", "-c", "3"])] + [("edge", a) for a in EDGE_SETS])
# (seed, n, m, components, dim) of the PCA cohorts without exact distance ties
TIE_FREE = [(31, 70, 1500, 20, 20), (32, 130, 700, 7, 7), (33, 33, 96, 3, 2)]
BIG_PCA = (35, 1030, 64, 3, 3)


def case_id(case):
    return (case[0].split(":")[0] + "_" + "x".join(case[0].split(":")[2:4]) + "".join(case[1])).replace("-", "_")


# ---------------------------------------------------------------------------------------------------- PCA helpers
def pca_kw(args):
    """the flags of a -p run as expected_text's arguments: (dim, kw)"""
    names = {"-s": ("thresh", float), "-w": ("skew", float), "-c": ("min_cov", int), "-g": ("genome", int), "-S": ("S", float),
             "-l": ("L", float), "-r": ("r", float), "-1": ("m1", float), "-2": ("m2", float)}
    dim, kw, i = 20, {}, 0
    while i < len(args):
        a = args[i]
        if a == "-a":
            kw["all_"] = True
        else:
            if a == "-d":
                dim = int(args[i + 1])
            elif a not in ("-p", "-n", "-t"):
                kw[names[a][0]] = names[a][1](args[i + 1])
            i += 1
        i += 1
    return dim, kw


def pca_expected(restatement, d, names, args):
    dim, kw = pca_kw(args)
    with inside(d):
        return expected_text(restatement, Path(str(d)), names, dim, "norm.txt", "rot.tsv", **kw)


def radii_flags(restatement, d, samples, dim, q_small, q_large, rest=("-r", "1", "-1", "0.05", "-2", "0.5")):
    """-S / -l at two percentiles of the restatement's pair distances (as test_cli_pca_equals_expected_bytes chooses them),
    so that the small and the large radius both cut through the cohort"""
    with inside(d):
        cloud, _, _ = rs_project(restatement, Path(str(d)), samples, 1, "norm.txt", "rot.tsv", dim)
    n = cloud.shape[0]
    dd = []
    for i in range(0, n, 128):                                                # row blocks: n = 1,030 without an n x n x dim array
        diff = cloud[i:i + 128, None, :] - cloud[None, :, :]
        block = np.sqrt((diff * diff).sum(-1))
        dd.append(block[np.arange(i, min(i + 128, n))[:, None] < np.arange(n)[None, :]])
    dd = np.concatenate(dd)
    return ["-d", str(dim), "-S", repr(float(np.percentile(dd, q_small))), "-l", repr(float(np.percentile(dd, q_large)))] + list(rest)


def tie_free_args(restatement, cohorts, spec):
    seed, n, m, comp, dim = spec
    d, names, s = cohorts.get("spread:%d:%d:%d:%d" % (seed, n, m, comp))
    if spec == BIG_PCA:
        # one sample in five below 5 % missing (small radius), the empty sample 3 alone at or above 99 % (search all: 1,029
        # rows), the rest large; 0.2 % and 1 % of 530,000 pairs: a few thousand rows
        args = ["-a"] + radii_flags(restatement, d, s, dim, 0.2, 1.0, rest=("-r", "1", "-1", "0.05", "-2", "0.99"))
    else:
        args = ["-a"] + radii_flags(restatement, d, s, dim, 15, 60)
    return d, names, s, PCA + args


def grouped(text):
    """The rows of a -p run as the header and a list of (sample1, printed distance, sorted rows): consecutive rows of one
    sample1 with the same printed distance form one group."""
    lines = text.split(b"\n")
    assert lines[-1] == b""
    out = []
    for line in lines[1:-1]:
        cols = line.split(b"\t")
        key = (cols[0], cols[4])
        if out and out[-1][0] == key:
            out[-1][1].append(line)
        else:
            out.append((key, [line]))
    return lines[0], [(k, sorted(rows)) for k, rows in out]


def same_up_to_tie_order(got, want):
    return sorted(got.split(b"\n")) == sorted(want.split(b"\n")) and grouped(got) == grouped(want)


DUPLICATE_CASES = [[], ["-a"], ["-a", "-d", "5"], ["-S", "{S}", "-l", "{L}", "-r", "1", "-1", "0.05", "-2", "0.5"],
                   ["-a", "-S", "{S}", "-l", "{L}", "-r", "1", "-1", "0.1", "-2", "0.7", "-s", "0.3", "-w", "0", "-c", "2"]]


def duplicate_cases(restatement, cohorts):
    d, names, s = cohorts.get("duplicate")
    flags = radii_flags(restatement, d, s, 20, 15, 60)
    S, L = flags[3], flags[5]
    return d, names, [PCA + [a.format(S=S, L=L) for a in c] for c in DUPLICATE_CASES]


def single_pca_text(d, name, cloud_row, min_cov=1, genome=6200000000):
    """computeScoreSingle's stdout with -p (src/CompareCounts.hpp:541-585) from the oracle's summaries and a cloud row"""
    with inside(d):
        o = EvalOracle([name])
        hets, homs, miss = o.genotype(0, min_cov)
        row = [name, cfmt(o.L.ntsm_eval_oracle_total(o.h, 0) / o.m), cfmt(o.L.ntsm_eval_oracle_error_rate(o.h, 0, genome)), str(miss),
               str(homs), str(hets)] + [cfmt(float(v)) for v in cloud_row]
        o.close()
    head = "sample\tcov\terrorRate\tmiss\thom\thet" + "".join("\tPC%d" % k for k in range(1, len(cloud_row) + 1))
    return (head + "\n" + "\t".join(row)).encode()


def restated_cloud(restatement, d, samples, dim, min_cov=1):
    with inside(d):
        return rs_project(restatement, Path(str(d)), samples, min_cov, "norm.txt", "rot.tsv", dim)[0]


# ---------------------------------------------------------------------------------------------------- CPU
def test_eval_driver_includes_the_class_and_restates_nothing(built):
    """oracle/ref_eval_driver.cpp takes the scoring class from the #include and carries no copy of it or of vendor/kfunc.c;
    oracle/ref_config/config.h defines nothing; what the recipe builds stays out of the history."""
    src = open(DRIVER).read()
    assert '#include "src/CompareCounts.hpp"' in src and '#include "src/Options.h"' in src
    for text in ("class CompareCounts", "computeLogLikelihood", "computeSumLogP", "gatherValidEntries", "calcRelatedness", "calcHomHetMiss",
                 "calcDistance", "computeErrorRate", "resultsStr", "loadPair", "radiusSearch", "inner_product", "kf_lgamma", "kf_betai",
                 "kt_fisher_exact", "void computeScore", "void projectPCs", "void mergeCounts"):
        assert text not in src, text
    for call in ("comp.computeScoreSingle()", "comp.computeScore()", "comp.projectPCs()", "comp.computeScorePCA()", "comp.mergeCounts()",
                 "omp_set_num_threads(opt::threads)"):
        assert call in src, call
    assert "#define" not in open(os.path.join(ROOT, "oracle", "ref_config", "config.h")).read()
    recipe = open(os.path.join(ROOT, "oracle", "Makefile")).read()
    line = [l for l in recipe.split("$(CXX)") if "ref_eval_driver.cpp -o _ref/ref_ntsmEval" in l][-1]
    assert line.split()[:5] == ["-O3", "-std=c++11", "-fopenmp", "-w", "-Iref_config"]
    assert "fast-math" not in line and "-march" not in line and "-ffp-contract" not in line
    tracked = subprocess.run(["git", "ls-files", "oracle"], cwd=ROOT, stdout=subprocess.PIPE).stdout.decode().split()
    assert not any(t.startswith("oracle/_ref/") for t in tracked)
    if HAVE_REF_TREE:
        assert os.path.isfile(REF_EVAL) and os.path.getmtime(REF_EVAL) >= os.path.getmtime(DRIVER)


@need_ref
@pytest.mark.parametrize("case", CPU_PAIRS, ids=case_id)
def test_oracle_cli_equals_reference_bytes(cohorts, case):
    """All pairs: the oracle's printer against the reference class, stdout byte for byte -- default threshold, -a, -s / -w /
    -c / -g at and beyond their usual ranges; 12 x 3,000, 65 x 1,000, the edge cohort (empty, duplicate, depth 0.5, counts to
    3e9) and files that differ in locus order, lack loci and lack the column-header line."""
    d, names, _ = cohorts.get(case[0])
    got, want = stdout_of(ORACLE_CLI, case[1], names, d), reference(case[1], names, d)
    assert got == want
    assert want.count(b"\n") == 1 + len(names) * (len(names) - 1) // 2 if "-a" in case[1] else want.count(b"\n") >= 1


@need_ref
def test_oracle_cli_single_table_and_merge_equal_reference_bytes(cohorts):
    """One file: the QC table (no trailing newline); -e FILE -o and -e FILE after the analysis: the merged counts file."""
    d, names, _ = cohorts.get(R12)
    for args in ([], ["-c", "2", "-g", "3100000000"], ["-c", "0"]):
        want = reference(args, names[3:4], d)
        assert stdout_of(ORACLE_CLI, args, names[3:4], d) == want and want.startswith(b"sample\tcov\t") and not want.endswith(b"\n")
    e, names, _ = cohorts.get("edge")                                         # column sums past 2^32 wrap in the merge
    l, lnames, _ = cohorts.get("loader")
    for where, files, args in ((d, names[:1], []), (e, names, ["-o"]), (e, names, ["-a"]), (l, lnames, ["-o"])):
        a = stdout_of(ORACLE_CLI, ["-e", "merged_oracle.txt"] + args, files, where)
        b = reference(["-e", "merged_ref.txt"] + args, files, where)
        assert a == b
        if len(files) > 1:
            assert open(os.path.join(str(where), "merged_oracle.txt"), "rb").read() == open(os.path.join(str(where), "merged_ref.txt"), "rb").read()
        else:
            assert not os.path.exists(os.path.join(str(where), "merged_ref.txt"))    # one file: no merge (ntSeqMatchEval.cpp:305-341)


@need_ref
def test_oracle_cli_wide_cohort_equals_reference(cohorts):
    """1,030 samples x 30 sites under -a (530,000 rows): length, line count and SHA-256."""
    d, names, _ = cohorts.get(WIDE)
    seen = [(len(x), x.count(b"\n"), hashlib.sha256(x).hexdigest()) for x in (stdout_of(ORACLE_CLI, ["-a"], names, d), reference(["-a"], names, d))]
    assert seen[0] == seen[1] and seen[0][1] == 1 + 1030 * 1029 // 2


@need_ref
@pytest.mark.parametrize("spec", TIE_FREE + [BIG_PCA], ids=lambda s: "n%d_m%d_d%d" % (s[1], s[2], s[4]))
def test_pca_expected_text_equals_reference_bytes(cohorts, restatement, spec):
    """-p / -n on cohorts without exact distance ties: the text assembled from the restatement (x87 projection, candidate
    selection, calcDistance) and the oracle against the reference's projectPCs + computeScorePCA, byte for byte; all three
    radii occur.  n = 1,030 is the cohort of the GPU test past the 256-wide tile."""
    d, names, s, args = tie_free_args(restatement, cohorts, spec)
    want = reference(args, names, d)
    got, _, g = pca_expected(restatement, d, names, args)
    assert len({x["radius"] for x in g}) == 3
    assert got == want and want.count(b"\n") > len(names)
    if spec == BIG_PCA:
        assert 2000 < want.count(b"\n") < 9000


@need_ref
def test_pca_expected_text_equals_reference_up_to_tie_order(cohorts, restatement):
    """The cohort with the planted duplicate s[n - 1] = s[0]: same multiset of rows, and the same order once the rows of one
    sample1 that print one distance count as a set (the documented deviation: ties ordered by k)."""
    d, names, cases = duplicate_cases(restatement, cohorts)
    for args in cases:
        want = reference(args, names, d)
        got, _, _ = pca_expected(restatement, d, names, args)
        assert same_up_to_tie_order(got, want), args
        assert want.count(b"\n") >= 2


@need_ref
def test_pca_single_file_columns_equal_reference_bytes(cohorts, restatement):
    """-p -n FILE on one file prints the projection itself: the restatement's cloud (long double compiled here) against the
    reference's own long double inner_product, as printed -- 20 and 7 components, and the sample with wrapped counts."""
    for key, dim, pick in (("spread:31:70:1500:20", 20, (0, 2, 3, 69)), ("spread:32:130:700:7", 7, (1, 127)), ("wrapped", 3, (2, 5))):
        d, names, s = cohorts.get(key)
        cloud = restated_cloud(restatement, d, s, dim)
        for i in pick:
            assert single_pca_text(d, names[i], cloud[i]) == reference(PCA + ["-d", str(dim)], names[i:i + 1], d), (key, i)
    d, names, s = cohorts.get("wrapped")
    cloud = restated_cloud(restatement, d, s, 4, min_cov=0)
    assert single_pca_text(d, names[2], cloud[2], min_cov=0) == reference(PCA + ["-d", "4", "-c", "0"], names[2:3], d)


WRAPPED_SETS = [["-a", "-d", "3"], ["-a", "-d", "4", "-c", "0", "-S", "0.3", "-l", "0.6", "-r", "1", "-1", "0.05", "-2", "0.5"]]


@need_ref
def test_pca_wrapped_counts_equal_reference_bytes(cohorts, restatement):
    """A sample with counts at and beyond 2^31 in both columns: countAT + countCG wraps as `unsigned` in projectPCs and in the
    joint counts of the score.  The restatement and the oracle against the reference, byte for byte."""
    d, names, s = cohorts.get("wrapped")
    assert int(s[2, 0, 0]) + int(s[2, 0, 1]) == 1 << 32 and int(s[2, 10, 0]) + int(s[2, 10, 1]) > 1 << 32
    for args in WRAPPED_SETS:
        want = reference(PCA + args, names, d)
        got, _, _ = pca_expected(restatement, d, names, PCA + args)
        assert got == want and want.count(b"\n") > 20, args
    assert stdout_of(ORACLE_CLI, ["-a"], names, d) == reference(["-a"], names, d)


# ---------------------------------------------------------------------------------------------------- recordings
def recorded(case, d):
    """(names, recorded stdout, recorded merge file or None) with the inputs rebuilt in d"""
    _, names = make_eval.materialise(case["input"], str(d))
    if case["files"] is not None:
        names = [names[i] for i in case["files"]]
    out = gzip.open(os.path.join(GOLD, case["stdout"])).read()
    assert out.count(b"\n") == case["lines"]
    return names, out, gzip.open(os.path.join(GOLD, case["merge_out"])).read() if case.get("merge_out") else None


def check_recording(exe, case, d, extra=()):
    names, out, merged = recorded(case, d)
    assert stdout_of(exe, list(extra) + case["args"], names, d) == out
    if merged is not None:
        assert open(os.path.join(str(d), case["merge"]), "rb").read() == merged


@pytest.mark.parametrize("case", RECORDED, ids=[c["name"] for c in RECORDED])
def test_recordings_equal_oracle_and_restatement(tmp_path, restatement, case):
    """What the reference class printed (tests/golden/eval/, inputs rebuilt from the seeds of cases.json) against the oracle
    CLI, and for -p against expected_text / the restatement's cloud: byte for byte, with or without the reference binary."""
    if "-p" not in case["args"]:
        return check_recording(ORACLE_CLI, case, tmp_path)
    names, out, _ = recorded(case, tmp_path)
    dim, kw = pca_kw(case["args"])
    if len(names) == 1:
        s, _ = make_eval.materialise(case["input"], str(tmp_path))
        cloud = restated_cloud(restatement, tmp_path, s, dim, min_cov=kw.get("min_cov", 1))
        assert single_pca_text(tmp_path, names[0], cloud[case["files"][0]], min_cov=kw.get("min_cov", 1)) == out
    else:
        assert pca_expected(restatement, tmp_path, names, case["args"])[0] == out


def test_recordings_cover_what_they_should():
    by = {c["name"]: c for c in RECORDED}
    assert {"pairs_all", "pairs_all_c0", "pairs_all_c3_w1", "pairs_default", "single", "merge", "pca_all", "pca_radii", "pca_single", "pca_range_0",
            "pca_range_3", "pca_range_4"} <= set(by)
    # rotation values to e+308: an accumulator that overflows to inf and then meets -1.7e+308, one at -inf, one huge and finite
    pcs = [gzip.open(os.path.join(GOLD, by[k]["stdout"])).read().split(b"\n")[1].split(b"\t")[6:] for k in ("pca_range_0", "pca_range_3", "pca_range_4")]
    assert pcs[0][:2] == [b"inf", b"-inf"] and pcs[1][1] == b"inf" and pcs[2][0] == b"inf"
    assert all(len(p) == 3 and len(p[2]) > 300 and b"inf" not in p[2] for p in pcs) and len(pcs[1][0]) > 300 and len(pcs[2][1]) > 300
    assert by["pairs_all"]["lines"] == 1 + 12 * 11 // 2 and by["pairs_default"]["lines"] >= 2 and by["pca_radii"]["lines"] > 5
    files = set(os.listdir(GOLD))
    assert files == {"cases.json"} | {c["stdout"] for c in RECORDED} | {c["merge_out"] for c in RECORDED if c.get("merge_out")}
    assert sum(os.path.getsize(os.path.join(GOLD, f)) for f in files) < 100 * 1024


@need_ref
@pytest.mark.parametrize("case", RECORDED, ids=[c["name"] for c in RECORDED])
def test_recordings_equal_a_fresh_reference_run(tmp_path, case):
    check_recording(REF_EVAL, case, tmp_path, extra=["-t", "1"])


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gpu_ref(built):
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    assert os.path.isfile(REF_EVAL), "oracle/_ref/ref_ntsmEval must travel to the GPU box prebuilt (it needs /root/reference to build)"
    return REF_EVAL


@pytest.mark.gpu
@pytest.mark.parametrize("case", GPU_PAIRS, ids=case_id)
def test_cli_equals_reference_bytes(gpu_ref, cohorts, case):
    """build/ntsmEval, all pairs, against the reference class at -t 1: stdout byte for byte at -t 1 and at -t 4.  65 samples
    cross one 64-lane tile edge, 257 four; the edge cohort has an empty sample, a duplicate, depth 0.5 and counts to 3e9."""
    d, names, _ = cohorts.get(case[0])
    want = reference(case[1], names, d)
    assert want.count(b"\n") == 1 + len(names) * (len(names) - 1) // 2 if "-a" in case[1] else want.count(b"\n") >= 1
    for t in ("1", "4"):
        assert stdout_of(EVAL, ["-t", t] + case[1], names, d) == want, t


@pytest.fixture(scope="module")
def wide_reference(gpu_ref, cohorts):
    d, names, _ = cohorts.get(WIDE)
    x = reference(["-a"], names, d)
    return len(x), x.count(b"\n"), hashlib.sha256(x).hexdigest()


@pytest.mark.gpu
@pytest.mark.parametrize("t", ["1", "4"])
def test_cli_wide_cohort_equals_reference(wide_reference, cohorts, t):
    """1,030 x 30 under -a (256-thread workgroups, five tiles of j): length, line count and SHA-256 of stdout."""
    d, names, _ = cohorts.get(WIDE)
    x = stdout_of(EVAL, ["-t", t, "-a"], names, d)
    assert (len(x), x.count(b"\n"), hashlib.sha256(x).hexdigest()) == wide_reference
    assert wide_reference[1] == 1 + 1030 * 1029 // 2


@pytest.mark.gpu
@pytest.mark.parametrize("spec", TIE_FREE + [BIG_PCA], ids=lambda s: "n%d_m%d_d%d" % (s[1], s[2], s[4]))
def test_cli_pca_equals_reference_bytes(gpu_ref, cohorts, restatement, spec):
    """build/ntsmEval -p -n against projectPCs + computeScorePCA of the reference class, byte for byte, on the tie-free
    cohorts; n = 1,030 x 64 sites, dim 3 is past the 256-wide tile of the pair kernel, four loop trips of the count / fill
    kernels, -S / -l at 0.2 % and 1 % of the restatement's distances: all three radii, a few thousand rows."""
    d, names, s, args = tie_free_args(restatement, cohorts, spec)
    want = reference(args, names, d)
    assert want.count(b"\n") > len(names)
    if spec == BIG_PCA:
        assert 2000 < want.count(b"\n") < 9000
    for t in ("1", "4"):
        assert stdout_of(EVAL, ["-t", t] + args, names, d) == want, t


@pytest.mark.gpu
def test_cli_pca_equals_reference_up_to_tie_order(gpu_ref, cohorts, restatement):
    """The planted-duplicate cohort under the five flag sets of test_cli_pca_equals_expected_bytes: the same rows, in the
    same order once rows of one sample1 with one printed distance count as a set."""
    d, names, cases = duplicate_cases(restatement, cohorts)
    for args in cases:
        want = reference(args, names, d)
        assert same_up_to_tie_order(stdout_of(EVAL, args, names, d), want) and want.count(b"\n") >= 2, args


@pytest.mark.gpu
def test_cli_pca_single_file_and_wrapped_counts_equal_reference_bytes(gpu_ref, cohorts):
    """The one-file PC table (the device's integer x87 chain against the reference's long double, as printed) and the cohort
    whose sample 2 has counts at and beyond 2^31 in both columns, byte for byte."""
    for key, dim, pick in (("spread:31:70:1500:20", 20, (0, 2, 3, 69)), ("spread:32:130:700:7", 7, (1, 127)), ("wrapped", 3, (2, 5))):
        d, names, _ = cohorts.get(key)
        for i in pick:
            args = PCA + ["-d", str(dim)]
            assert stdout_of(EVAL, args, names[i:i + 1], d) == reference(args, names[i:i + 1], d), (key, i)
    d, names, _ = cohorts.get("wrapped")
    for args in [PCA + a for a in WRAPPED_SETS] + [["-a"]]:
        want = reference(args, names, d)
        assert stdout_of(EVAL, args, names, d) == want and want.count(b"\n") > 20, args
    args = PCA + ["-d", "4", "-c", "0"]
    assert stdout_of(EVAL, args, names[2:3], d) == reference(args, names[2:3], d)


@pytest.mark.gpu
@pytest.mark.parametrize("case", RECORDED, ids=[c["name"] for c in RECORDED])
def test_cli_equals_recordings(built, tmp_path, case):
    """build/ntsmEval against what the reference class printed (tests/golden/eval/): needs nothing from oracle/_ref/."""
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    check_recording(EVAL, case, tmp_path)
