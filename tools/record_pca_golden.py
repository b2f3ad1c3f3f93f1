#!/usr/bin/env python3
"""Records the fixtures of tests/test_pca.py under tests/golden/pca (see the README there).

For every case: the matrix (committed ones are written here from their seed, the largest is only generated), then the
rotation and the components that pandas + scikit-learn's exact solver give on it -- tests/test_pca.py::sklearn_recipe,
the same function the test re-derives them with.  Also prints, per case, the gate of the GPU test beside what a float64
and a float32-Gram numpy model of the method reach, so the gate can be judged without a device.

Needs pandas and scikit-learn; no GPU.      python tools/record_pca_golden.py
"""
import gzip
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "pca")

CASES = [
    dict(name="vcf_plain", matrix="vcf/plain/expected_matrix.tsv", d=3),
    dict(name="vcf_cohort_19_digits", matrix="pca/vcf_cohort_19_digits/matrix.tsv.gz", d=5, vcf=dict(seed=40300, n=40, snps=300, multi=3)),
    dict(name="cohort_96x1500", matrix="pca/cohort_96x1500/matrix.tsv.gz", d=4, generate=dict(seed=9601500, n=96, p=1500, pops=6)),
    dict(name="cohort_48x700", matrix="pca/cohort_48x700/matrix.tsv.gz", d=2, generate=dict(seed=480700, n=48, p=700, pops=3, thirds=0.04)),
    dict(name="cohort_300x6000", matrix=None, d=20, generate=dict(seed=3006000, n=300, p=6000, pops=5)),
]


def vcf_matrix(case, path):
    """A matrix as ntsmVCF itself prints it: the seeded VCF cohort of tests/test_vcf.py through tests/vcf_restatement.cpp
    (the CPU restatement that ntsmVCF is tested against byte for byte); -m 3 gives cells at 19 digits."""
    import pathlib
    import subprocess
    import tempfile
    import test_vcf
    v = case["vcf"]
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "vcf_restatement")
        subprocess.run(["g++", "-O2", "-std=c++11", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "vcf_restatement.cpp")], check=True)
        genome, sites, vcf = test_vcf.cohort(pathlib.Path(d), np.random.default_rng(v["seed"]), v["n"], v["snps"])
        subprocess.run([exe, "-s", sites, "-r", genome, "-d", "-m", str(v["multi"]), "-p", os.path.join(d, "out"), vcf], capture_output=True, check=True)
        with open(path, "wb") as f:
            f.write(gzip.compress(open(os.path.join(d, "out_matrix.tsv"), "rb").read(), 9, mtime=0))


def main():
    os.makedirs(GOLD, exist_ok=True)
    with open(os.path.join(GOLD, "cases.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in CASES) + "\n]\n")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import tempfile
    import test_pca as tp
    scratch = tempfile.mkdtemp()
    for case in CASES:
        out = os.path.join(GOLD, case["name"])
        os.makedirs(out, exist_ok=True)
        g = case.get("generate")
        if case.get("vcf"):
            vcf_matrix(case, os.path.join(ROOT, "tests", "golden", case["matrix"]))
        if g and case["matrix"]:
            os.makedirs(os.path.dirname(os.path.join(ROOT, "tests", "golden", case["matrix"])), exist_ok=True)
            a = tp.structured_cohort(g["seed"], g["n"], g["p"], g["pops"], g.get("thirds", 0.0))
            tp.write_matrix(os.path.join(ROOT, "tests", "golden", case["matrix"]), a, gz=case["matrix"].endswith(".gz"))
        matrix = tp.case_matrix(case, scratch)
        rot, comp = tp.sklearn_recipe(matrix, case["d"])
        for frame, name in ((rot, "rotation.f8.gz"), (comp, "components.f8.gz")):
            with open(os.path.join(out, name), "wb") as f:
                f.write(gzip.compress(np.ascontiguousarray(frame.values, dtype="<f8").tobytes(), 9, mtime=0))
        _, a, _ = tp.read_table(matrix)
        bound, l = tp.golden_bounds(a, case["d"])
        g_rot, _ = tp.case_golden(case)
        e64 = np.abs(tp.numpy_model(a, case["d"])[1] - g_rot).max(axis=0)
        e32 = np.abs(tp.numpy_model(a, case["d"], np.float32)[1] - g_rot).max(axis=0)
        worst = int(np.argmax(bound))
        print("%-22s %4d x %5d d=%2d  largest gate %.2g (component %d)  float64 model %.2g  float32-Gram model %.2g  "
              "[min over components of float32 error / gate: %.2g]" %
              (case["name"], a.shape[1], a.shape[0], case["d"], bound[worst], worst, e64.max(), e32.max(), (e32 / bound).min()))
        if g and not case["matrix"]:
            os.remove(matrix)
    os.rmdir(scratch)


if __name__ == "__main__":
    main()
