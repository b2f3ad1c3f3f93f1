#!/usr/bin/env python3
"""Generate the ntsmEval fixtures under tests/golden/eval/ by running the UNMODIFIED reference scoring class.

Runs only where oracle/_ref/ref_ntsmEval exists (oracle/Makefile compiles it from /root/reference: the reference's
CompareCounts class behind oracle/ref_eval_driver.cpp).  Every case is: inputs regenerated from a seed (counts files, and
for the PCA route a centre and a rotation file), the flags, and what the reference wrote at -t 1 -- stdout, and for -e the
merged counts file.  Only tests/golden/eval/cases.json and the recorded outputs (gzip'd) are committed; materialise()
rebuilds the inputs, for this script and for tests/test_eval_reference.py alike.  The reference runs with relative file
names from the data directory, so the recorded bytes do not depend on where the tree lies.

Usage: python tests/golden/make_eval.py          (rewrites tests/golden/eval/)
"""
import gzip
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "eval")
REF_EVAL = os.path.join(ROOT, "oracle", "_ref", "ref_ntsmEval")
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_eval import random_samples, write_counts  # noqa: E402  (the generators; importing them changes nothing there)
from test_eval_pca import write_pca  # noqa: E402

MISSING = (0.0, 0.03, 0.2, 0.6)                  # the missing-site fractions of test_eval_pca.cohort


def spread(rng, n, m):
    """test_eval_pca.cohort without its planted duplicate: related samples at depth 20, a spread of missing-site fractions,
    sample 3 empty.  Without the duplicate no two candidate distances of a sample tie, so the order of the rows is fixed."""
    s = random_samples(rng, n, m, depth=20.0)
    for i in range(n):
        if MISSING[i % len(MISSING)]:
            s[i, rng.random(m) < MISSING[i % len(MISSING)]] = 0
    if n > 4:
        s[3] = 0
    return s


def edge_samples():
    """An empty sample, a duplicate, a sample at depth 0.5 and one whose counts reach 3e9: the sum of a
    site's two counts wraps as `unsigned` in the sample's total (src/CompareCounts.hpp:104-106, which moves cov and the score),
    and so do the joint counts of a pair."""
    rng = np.random.default_rng(14)
    s = random_samples(rng, 6, 400)
    s[1] = 0
    s[2] = s[0]
    s[3] = random_samples(rng, 1, 400, depth=0.5)[0]
    s[4] = rng.integers(0, 3000000001, size=(400, 2)).astype(np.uint32)
    s[4, :3] = [[3000000000, 0], [0, 3000000000], [3000000000, 3000000000]]
    return s


def write_pca_range(d, rng):
    """norm.txt and rot.tsv for 12 sites and 4 components (the runs use three) whose values span the long double exponents
    that a file can name and a double cannot hold.  Sites 0-3 have centres of -1.25 ... -2, so every call there gives
    v >= 1.25.  PC1 starts with rotation values of 1.5e+308 -- the first covered site's product already overflows the double
    accumulator to inf -- and goes on with -1.7e+308, which the inf has to survive; PC2 runs to -inf at sites 2-5 and then
    meets +1.7e+308; PC3 sums products of a few e+306, huge but finite throughout; the last sites carry values near e-300."""
    def digits(k):
        return "".join(str(x) for x in rng.integers(0, 10, size=k).tolist())
    norm = ["-1.5", "-1.25", "-1.75", "-2"] + ["0.%s" % digits(19) for _ in range(4)]
    norm += ["2.5%se-300" % digits(12), "1.25e-5", "0.%s" % digits(19), "7.%se-301" % digits(15)]
    rows = []
    for j in range(12):
        small = "%s%d.%se-300" % ("-" if j % 2 else "", 1 + j % 9, digits(18))
        pc1 = "1.5%se+308" % digits(16) if j < 4 else "-1.7%se+308" % digits(16) if j < 8 else small
        pc2 = small if j < 2 else "-1.6%se+308" % digits(16) if j < 6 else "1.7%se+308" % digits(16) if j < 10 else "3.%se+150" % digits(18)
        pc3 = small if j == 8 else "%s%d.%se+306" % ("-" if j % 3 == 1 else "", 1 + j % 4, digits(18))
        rows.append("rs%d\t%s\t%s\t%s\t%s.%se-2" % (j, pc1, pc2, pc3, 1 + j % 9, digits(19)))
    with open(os.path.join(d, "norm.txt"), "w") as f:
        f.write("".join(x + "\n" for x in norm))
    with open(os.path.join(d, "rot.tsv"), "w") as f:
        f.write("rsID\tPC1\tPC2\tPC3\tPC4\n" + "".join(r + "\n" for r in rows))


def range_samples(rng):
    """Six samples over 12 sites at depth 20; sample 3 lacks the first four sites (PC1 meets -1.7e+308 from +0.0), sample 4
    lacks sites 2-5 (PC2 meets +1.7e+308 first), sample 5 lacks every site."""
    s = random_samples(rng, 6, 12, depth=20.0)
    s[3, :4] = 0
    s[4, 2:6] = 0
    s[5] = 0
    return s


def write_cohort(d, samples):
    names = []
    for i in range(samples.shape[0]):
        names.append("s%03d.txt" % i)
        write_counts(os.path.join(d, names[-1]), samples[i])
    return names


def materialise(spec, d):
    """The input files of one cases.json "input" entry, written into directory d.  Returns (samples, file names relative to
    d); a "pca" input also leaves norm.txt and rot.tsv there."""
    from pathlib import Path
    rng = np.random.default_rng(spec["seed"])
    if spec["kind"] == "random":
        s = random_samples(rng, spec["n"], spec["m"])
    elif spec["kind"] == "edge":
        s = edge_samples()
    elif spec["kind"] == "pca_range":
        s = range_samples(rng)
    else:
        assert spec["kind"] == "pca", spec
        s = spread(rng, spec["n"], spec["m"])
    names = write_cohort(d, s)
    if spec["kind"] == "pca":
        write_pca(Path(d), spec["m"], spec["components"], rng)
    if spec["kind"] == "pca_range":
        write_pca_range(d, rng)
    return s, names


def run_reference(args, names, d):
    p = subprocess.run([REF_EVAL, "-t", "1"] + args + names, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, (args, p.stderr[-500:])
    return p.stdout


PAIRS = dict(kind="random", seed=46, n=12, m=300)   # one pair scores under the default threshold, a dozen under 1.5
EDGE = dict(kind="edge", seed=14)
PCA = dict(kind="pca", seed=33, n=33, m=96, components=3)
PCA_ARGS = ["-p", "rot.tsv", "-n", "norm.txt", "-d", "2"]
# single-file mode only: the QC row with its PC columns is the projection as printed, and no tree is built over an infinite cloud
RANGE = dict(kind="pca_range", seed=36)
RANGE_ARGS = ["-p", "rot.tsv", "-n", "norm.txt", "-d", "3"]
# -S / -l: about the 15th and 60th percentile of the pair distances of the PCA cohort (make() checks that the three radii occur)
# -s 3: without -a the default threshold leaves one row of this small cohort
RADII = ["-S", "0.13", "-l", "0.31", "-r", "1", "-1", "0.05", "-2", "0.5", "-s", "3"]
CASES = [
    dict(name="pairs_all", input=PAIRS, files=None, args=["-a"]),
    dict(name="pairs_all_c0", input=PAIRS, files=None, args=["-a", "-c", "0"]),
    dict(name="pairs_all_c3_w1", input=PAIRS, files=None, args=["-a", "-c", "3", "-w", "1"]),
    dict(name="pairs_default", input=PAIRS, files=None, args=[]),
    dict(name="pairs_s1_5", input=PAIRS, files=None, args=["-s", "1.5"]),
    dict(name="edge_all", input=EDGE, files=None, args=["-a"]),
    dict(name="edge_merge", input=EDGE, files=None, args=["-s", "3", "-e", "merged.txt"], merge="merged.txt"),
    dict(name="edge_single", input=EDGE, files=[4], args=[]),
    dict(name="single", input=PAIRS, files=[5], args=["-c", "2", "-g", "3100000000"]),
    dict(name="merge", input=PAIRS, files=[2, 7, 4], args=["-e", "merged.txt", "-o"], merge="merged.txt"),
    dict(name="pca_all", input=PCA, files=None, args=PCA_ARGS + ["-a"]),
    dict(name="pca_radii", input=PCA, files=None, args=PCA_ARGS + RADII),
    dict(name="pca_single", input=PCA, files=[6], args=PCA_ARGS + ["-a"]),
    dict(name="pca_range_0", input=RANGE, files=[0], args=RANGE_ARGS),
    dict(name="pca_range_3", input=RANGE, files=[3], args=RANGE_ARGS + ["-c", "2"]),
    dict(name="pca_range_4", input=RANGE, files=[4], args=RANGE_ARGS),
]


def radii_of(d, names, args):
    """The distinct search radii the reference's rule gives the samples, from the restatement and the oracle."""
    from pathlib import Path
    from test_eval_pca import expected_text, gxx
    exe = gxx(Path(d), "eval_pca_restatement.cpp", "eval_pca_restatement")
    kw = dict(zip(("S", "L", "r", "m1", "m2"), (float(args[args.index(f) + 1]) for f in ("-S", "-l", "-r", "-1", "-2"))))
    here = os.getcwd()
    os.chdir(d)
    try:
        _, _, g = expected_text(exe, Path(d), names, 2, "norm.txt", "rot.tsv", **kw)
    finally:
        os.chdir(here)
    return {x["radius"] for x in g}


def make():
    assert os.path.isfile(REF_EVAL), "oracle/_ref/ref_ntsmEval is built only where /root/reference exists"
    os.makedirs(OUT, exist_ok=True)
    for f in os.listdir(OUT):
        os.remove(os.path.join(OUT, f))
    doc, range_pcs = [], []
    for case in CASES:
        with tempfile.TemporaryDirectory() as d:
            _, names = materialise(case["input"], d)
            if case["files"] is not None:
                names = [names[i] for i in case["files"]]
            out = run_reference(case["args"], names, d)
            if case["name"] == "pca_radii":
                assert len(radii_of(d, names, case["args"])) == 3 and out.count(b"\n") > 5
            if case["name"].startswith("pca_range"):
                pcs = out.split(b"\n")[1].split(b"\t")[6:]
                assert len(pcs) == 3 and len(pcs[2]) > 300 and b"inf" not in pcs[2], pcs      # PC3: huge and finite
                range_pcs.append(pcs[:2])
            rec = dict(case, stdout=case["name"] + ".out.gz", lines=out.count(b"\n"))
            with open(os.path.join(OUT, rec["stdout"]), "wb") as fh:
                fh.write(gzip.compress(out, mtime=0))
            if case.get("merge"):
                rec["merge_out"] = case["name"] + ".merged.gz"
                with open(os.path.join(OUT, rec["merge_out"]), "wb") as fh:
                    fh.write(gzip.compress(open(os.path.join(d, case["merge"]), "rb").read(), mtime=0))
            doc.append(rec)
            print("%-16s %6d bytes %4d lines" % (case["name"], len(out), rec["lines"]))
    assert [b"inf", b"-inf"] in range_pcs and len({tuple(p) for p in range_pcs}) == len(range_pcs), range_pcs
    with open(os.path.join(OUT, "cases.json"), "w") as fh:
        json.dump(dict(recorded_with="oracle/_ref/ref_ntsmEval -t 1 (oracle/ref_eval_driver.cpp around the unmodified "
                                     "src/CompareCounts.hpp), relative file names, cwd = the data directory",
                       cases=doc), fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    make()
