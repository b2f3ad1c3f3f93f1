"""What `ntsmEval`'s command line does, held to recordings ("The run table"): the first refusal of every
combination of run flags, own flags, reference flags and positionals, and the bytes of every store run at tiny shapes.

CPU, devices hidden (tests/golden/eval_cli_args.json.gz): a fixed product of argument vectors over two stores S and T of
4 samples x 40 sites (test_eval_qc.write_store), one counts file, a rotation, a centre and a pedigree; no index exists.  Abbreviated
long options are among them: getopt names the possibilities of an ambiguous one in the order of the program's option table.  Exit
status, stdout and stderr of each vector equal the recording, with the program path that getopt prints replaced by a token
and the `Time:` line dropped.  Every file is put back before each vector, so no vector sees what another left.
GPU (tests/golden/eval_cli_runs.json.gz): each run that uses the device at 7 x 130 (A) and 5 x 130 (B, and Bm lacking nine
of A's loci in another order), with search-all samples (two runs of dense rows in A) and finite-radius samples on either side, the band overrides at three bands
and the band rules, B's projections from its index and projected in the run: stdout and the side files byte for byte, the
`-v -v` stderr with every number before " ms" or " s" masked.
A vector without a recording fails.  `python tests/test_eval_cli_args.py cpu|gpu FILE` writes a recording; the committed ones
were made by the binary built from the last commit before the run table (dd1c984)."""
import base64
import gzip
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle_binding import ROOT
from test_eval import random_samples, write_counts
from test_eval_pca import write_pca
from test_eval_qc import EVAL, HIDDEN, write_store

GOLDEN = os.path.join(ROOT, "tests", "golden")
ARGS_RECORDING, RUNS_RECORDING = os.path.join(GOLDEN, "eval_cli_args.json.gz"), os.path.join(GOLDEN, "eval_cli_runs.json.gz")
PCA = ["-p", "rot.tsv", "-n", "norm.txt"]

# name: (the run's flag, what a valid call of it has besides)
RUNS = {
    "files": ([], ["q.txt"]), "pack": (["--pack", "S"], ["q.txt"]), "against": (["--against", "S"], ["q.txt"]),
    "index": (["--index", "S"], PCA), "near": (["--near", "S"], ["q.txt"]), "within": (["--within", "S"], []),
    "within-near": (["--within-near", "S"], []), "between": (["--between", "S"], ["T"]), "between-near": (["--between-near", "S"], ["T"]),
    "qc": (["--qc", "S"], []), "contam": (["--contam", "S"], []), "trios": (["--trios", "S"], []), "ld": (["--ld", "S"], []),
}
VALUE_FLAGS = {
    "--within-rows": "3", "--between-rows": "2", "--contam-depth": "5", "--contam-min": "0.1", "--contam-explained": "0.2", "--contam-rows": "3",
    "--trio-depth": "5", "--trio-called": "7", "--trio-max": "0.1", "--trio-duo": "0.2", "--ld-depth": "5", "--ld-called": "3", "--ld-min": "0.3",
}
OWN_FLAGS = dict({f: [f, v] for f, v in VALUE_FLAGS.items()}, **{
    "--trio-exhaustive": ["--trio-exhaustive"], "--ped": ["--ped", "ped.txt"], "--sites-out": ["--sites-out", "out.tsv"],
    "--samples-out": ["--samples-out", "out.tsv"], "--ld-prune": ["--ld-prune", "out.txt"]})
RUN_OF_FLAG = {"--within-rows": "within", "--between-rows": "between", "--ped": "trios", "--sites-out": "qc", "--samples-out": "contam"}
BAD_VALUES = ["x", "", "1x", "-1", "0", "nan", "inf", "4294967296"]
REFERENCE_FLAGS = [["-p", "rot.tsv"], ["-n", "norm.txt"], PCA, ["-b", "truth.tsv"], ["-e", "merged.txt"], ["-o"]]


def run_of(flag):
    return RUN_OF_FLAG.get(flag) or {"--con": "contam", "--tri": "trios", "--ld-": "ld"}[flag[:5]]


def vectors():
    """group id -> its argument vectors, in a fixed order"""
    g = {}
    flags = [r[0] for r in RUNS.values() if r[0]]
    for a in flags:                                                                     # every ordered pair, and each flag twice
        g["pair" + a[0]] = [a + b for b in flags]
    for f, own in OWN_FLAGS.items():                                                    # each own flag with each run, bare and valid
        g["own" + f] = [flag + own + rest for flag, valid in RUNS.values() for rest in ([], valid)]
    g["reference_flags"] = [flag + ([] if valid is PCA else valid) + x for flag, valid in RUNS.values() for x in REFERENCE_FLAGS]
    g["positionals"] = [flag + pos for name, (flag, valid) in RUNS.items()
                        for pos in ([], ["T"] if "between" in name else ["q.txt"], ["T", "T"] if "between" in name else ["q.txt", "q.txt"])]
    g["positionals"] += [["--index", "S"] + PCA + pos for pos in (["q.txt"], ["q.txt", "q.txt"])]
    g["unknown"] = [flag + valid + ["--bogus"] for flag, valid in RUNS.values()]
    for f in VALUE_FLAGS:                                                               # each value flag's reader, with its own run
        flag, valid = RUNS[run_of(f)]
        g["value" + f] = [flag + valid + [f, v] for v in BAD_VALUES]
    g["threads"] = [["-t", "x"], ["-t", "x", "q.txt"]]
    # abbreviated long options: getopt names the possibilities of an ambiguous one in the order of its table
    g["abbreviations"] = [["--with", "S"], ["--withi", "S"], ["--within-", "S"], ["--b", "S", "T"], ["--between-", "S", "T"], ["--l", "S"], ["--ld-", "3", "--ld", "S"],
                          ["--p", "S", "q.txt"], ["--pe", "ped.txt", "--trios", "S"], ["--t", "S"], ["--trio", "S"], ["--trio-", "3", "--trios", "S"],
                          ["--c", "S"], ["--contam-", "3", "--contam", "S"], ["--s", "out.tsv", "--qc", "S"], ["--a", "S", "q.txt"], ["--n", "S", "q.txt"],
                          ["--i", "S"], ["--q", "S"], ["--trio-e", "--trios", "S"], ["--between-r", "2", "--between", "S", "T"]]
    seen = set()                                                                        # a vector that two rules give is run once, where it first stands
    for name in g:
        g[name] = [v for v in g[name] if not (json.dumps(v) in seen or seen.add(json.dumps(v)))]
    return g


VECTORS = vectors()


def write_inputs(d):
    """S, T, q.txt over the stores' loci, rot.tsv, norm.txt and ped.txt in the empty directory d; name -> bytes"""
    rng = np.random.default_rng(20)
    for store in ("S", "T"):
        loci, names = write_store(os.path.join(d, store), rng.integers(0, 30, size=(4, 40, 2)).astype(np.uint32), rng)
    write_counts(os.path.join(d, "q.txt"), rng.integers(0, 30, size=(40, 2)).astype(np.uint32), loci=loci)
    from pathlib import Path
    write_pca(Path(d), 40, 3, rng)
    with open(os.path.join(d, "ped.txt"), "w") as f:
        f.write("fam\trun0002\trun0000\trun0001\t0\t0\n")
    return {name: open(os.path.join(d, name), "rb").read() for name in sorted(os.listdir(d))}


def put_back(d, pristine):
    for name in os.listdir(d):
        path = os.path.join(d, name)
        if name not in pristine:
            shutil.rmtree(path) if os.path.isdir(path) else os.unlink(path)
        elif open(path, "rb").read() != pristine[name]:
            open(path, "wb").write(pristine[name])


def observe(argv, d, pristine):
    put_back(d, pristine)
    p = subprocess.run([EVAL] + argv, capture_output=True, cwd=d, env=HIDDEN)
    err = b"".join(l for l in p.stderr.replace(EVAL.encode(), b"<ntsmEval>").splitlines(True) if not l.startswith(b"Time:"))
    return [p.returncode, p.stdout.decode("latin-1"), err.decode("latin-1")]


def load(path):
    with gzip.open(path, "rb") as f:
        return json.loads(f.read().decode())


def save(path, recording):
    with open(path, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", mtime=0, filename="") as f:
        f.write(json.dumps(recording, indent=0, sort_keys=True).encode())


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("cli_args"))
    return d, write_inputs(d)


@pytest.fixture(scope="module")
def args_recording():
    return load(ARGS_RECORDING)


def test_the_product_is_the_recorded_one(args_recording):
    """no vector twice under one key, every recorded vector generated and every generated one recorded"""
    keys = [json.dumps(v) for group in VECTORS.values() for v in group]
    assert len(keys) == len(set(keys)) and set(keys) == set(args_recording) and len(keys) >= 700


@pytest.mark.parametrize("group", list(VECTORS))
def test_first_refusal_equals_the_recording(inputs, args_recording, group):
    d, pristine = inputs
    for argv in VECTORS[group]:
        key = json.dumps(argv)
        assert key in args_recording, "no recording of %s" % key
        assert observe(argv, d, pristine) == args_recording[key], argv


# ---------------------------------------------------------------------------------------------------- GPU: the runs
V = ["-a", "-v", "-v"]
TRIO, LD = ["--trio-called", "5", "--trio-duo", "1", "--trio-depth", "2"], ["--ld-called", "3", "--ld-depth", "2", "--ld-min", "0.2"]
# id: (arguments, side files, environment)
CASES = {
    "pairs": (V + ["a0.txt", "a1.txt", "a2.txt", "b0.txt"], [], {}),
    "pca": (V + PCA + ["-d", "3", "a0.txt", "a1.txt", "a2.txt", "b0.txt", "b2.txt"], [], {}),
    "single_pca": (V + PCA + ["-d", "3", "a1.txt"], [], {}),
    "against": (V + ["--against", "A", "b0.txt", "b2.txt"], [], {}),
    "index": (V + ["--index", "I"] + PCA + ["-d", "3"], ["I.pcaidx"], {}),
    "near": (V + ["--near", "A", "b0.txt", "b2.txt"], [], {}),
    "within": (V + ["--within", "A"], [], {}),
    "within_rows3": (V + ["--within", "A", "--within-rows", "3"], [], {}),
    "within_near": (V + ["--within-near", "A"], [], {}),
    "between": (V + ["--between", "A", "Bm"], [], {}),
    "between_rows2": (V + ["--between", "A", "Bm", "--between-rows", "2"], [], {}),
    "between_near_from_index": (V + ["--between-near", "A", "B"], [], {}),
    "between_near_projected": (V + ["--between-near", "A", "Bm"], [], {}),
    "qc": (V + ["--qc", "A"], [], {}),
    "qc_pca_sites": (V + ["--qc", "A"] + PCA + ["-d", "3", "--sites-out", "sites.tsv"], ["sites.tsv"], {}),
    "contam": (V + ["--contam", "A", "--contam-depth", "4", "--samples-out", "samples.tsv"], ["samples.tsv"], {}),
    "contam_rows3": (V + ["--contam", "A", "--contam-depth", "4", "--contam-rows", "3", "--samples-out", "samples.tsv"], ["samples.tsv"], {}),
    "trios": (V + ["--trios", "A"] + TRIO, [], {}),
    "trios_ped": (["-v", "-v", "--trios", "A", "--ped", "ped.txt"] + TRIO, [], {}),
    "ld": (V + ["--ld", "A", "--ld-prune", "kept.txt"] + LD, ["kept.txt"], {}),
    "ld_small_budget": (V + ["--ld", "A", "--ld-prune", "kept.txt"] + LD, ["kept.txt"], {"NTSM_LD_PAIR_BUDGET": "1"}),
}


def write_cohort(d):
    """a0 ... a6 and b0 ... b4 over 130 sites, a2, a5 and b2 empty (they search all; a2 and a5 are two runs of dense rows of A),
    m0 ... m4 = b0 ... b4 without nine of the loci and in another order; the stores A, I = A, B, Bm; the indexes of A and B at
    -d 3 (on the GPU); a pedigree over A"""
    rng = np.random.default_rng(2024)
    s = random_samples(rng, 12, 130)
    s[2] = 0
    s[5] = 0
    s[9] = 0
    lacking = np.concatenate([[0, 129], rng.choice(np.arange(1, 129), size=7, replace=False)])
    order = rng.permutation(np.setdiff1d(np.arange(130), lacking))
    fa, fb, fm = ["a%d.txt" % i for i in range(7)], ["b%d.txt" % i for i in range(5)], ["m%d.txt" % i for i in range(5)]
    for i in range(7):
        write_counts(os.path.join(d, fa[i]), s[i])
    for i in range(5):
        write_counts(os.path.join(d, fb[i]), s[7 + i])
        write_counts(os.path.join(d, fm[i]), s[7 + i][order], loci=["rs%d" % x for x in order])
    from pathlib import Path
    write_pca(Path(d), 130, 4, rng)
    with open(os.path.join(d, "ped.txt"), "w") as f:
        f.write("# a comment\nfam\ta3\ta0\ta1\t0\t0\nfam\ta0\t0\t0\t0\t0\nfam\ta6\ta4\ta5\t0\t0\n")
    for store, files in (("A", fa), ("I", fa), ("B", fb), ("Bm", fm)):
        assert subprocess.run([EVAL, "--pack", store] + files, cwd=d, capture_output=True).returncode == 0
    for store in ("A", "B"):
        p = subprocess.run([EVAL, "--index", store] + PCA + ["-d", "3"], cwd=d, capture_output=True)
        assert p.returncode == 0, p.stderr


def observe_run(case, d):
    argv, side, env = CASES[case]
    for name in side:
        if os.path.exists(os.path.join(d, name)):
            os.unlink(os.path.join(d, name))
    p = subprocess.run([EVAL] + argv, capture_output=True, cwd=d, env=dict(os.environ, **env))
    err = re.sub(r"[-+0-9.e]+(?= (?:ms|s)\b)", "#", p.stderr.decode("latin-1"))
    files = {name: base64.b64encode(open(os.path.join(d, name), "rb").read()).decode() for name in side}
    return {"status": p.returncode, "stdout": p.stdout.decode("latin-1"), "stderr": err, "files": files}


@pytest.fixture(scope="module")
def cohort(tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    d = str(tmp_path_factory.mktemp("cli_runs"))
    write_cohort(d)
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
def test_run_equals_the_recording(cohort, case):
    recording = load(RUNS_RECORDING)
    assert case in recording, "no recording of %s" % case
    got = observe_run(case, cohort)
    assert got["status"] == 0 and got == recording[case], case


if __name__ == "__main__":                                                              # python tests/test_eval_cli_args.py cpu|gpu FILE
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        if sys.argv[1] == "cpu":
            pristine = write_inputs(tmp)
            save(sys.argv[2], {json.dumps(v): observe(v, tmp, pristine) for group in VECTORS.values() for v in group})
        else:
            write_cohort(tmp)
            save(sys.argv[2], {case: observe_run(case, tmp) for case in CASES})
