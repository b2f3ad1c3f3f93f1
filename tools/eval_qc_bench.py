#!/usr/bin/env python3
"""ntsmEval --qc on the store of tools/eval_store_bench.py: N samples x 96,287 sites of the structured
cohort of tools/eval_pca_bench.py, written from the documented layout.  Whole-process wall times and the -vv split of

  * `build/ntsmEval -vv --qc STORE`, once with the store out of the page cache and once with it in;
  * the same with `-p ROT -n NORM` (20 components) and with `--sites-out FILE`;

and, for comparison, what the same table costs without the feature: one `build/ntsmEval FILE` per sample over K text counts
files (with and without -p), given per file and scaled to N.

    python tools/eval_qc_bench.py [--n 4096] [--files 16] [--dir DIR] [--json OUT]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import eval_pca_bench as pb  # noqa: E402
import eval_store_bench as sb  # noqa: E402

M, D = pb.M, pb.D


def write_pca(d, rng):
    norm = 0.5 + rng.random(M) * 1e-3
    rot = rng.standard_normal((M, D)) * (pb.SCALE / np.sqrt(M))
    with open(os.path.join(d, "norm.txt"), "w") as f:
        f.write("".join("%.17g\n" % v for v in norm.tolist()))
    with open(os.path.join(d, "rot.tsv"), "w") as f:
        f.write("rsID\t" + "\t".join("PC%d" % (k + 1) for k in range(D)) + "\n")
        f.write("".join("rs%d\t%s\n" % (s, "\t".join("%.17g" % v for v in row)) for s, row in enumerate(rot.tolist())))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--files", type=int, default=16, help="samples that also exist as text counts files, for the one-run-per-file route")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n, k = a.n, min(a.files, a.n)
    res = {"n": n, "sites": M, "files": k}
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        rng = np.random.default_rng(7)
        t0 = time.perf_counter()
        cohort = pb.cohort(rng, n)
        names = ["s%05d.txt" % i for i in range(n)]
        prefix = np.char.add(np.char.add("rs", np.arange(M).astype(str)), "\t")
        for i in range(k):
            sb.write_text(os.path.join(d, names[i]), cohort[i], prefix)
        store = os.path.join(d, "cohort.store")
        sb.write_store(store, names, cohort)
        write_pca(d, rng)
        del cohort
        res["store_bytes"] = os.path.getsize(store)
        print("store of %d samples x %d sites (%.3f GB), %d counts files and a %d-component rotation written in %.1f s"
              % (n, M, res["store_bytes"] / 1e9, k, D, time.perf_counter() - t0), flush=True)

        pca = ["-p", "rot.tsv", "-n", "norm.txt"]
        runs = [("qc_cold", [], True), ("qc_warm", [], False), ("qc_warm_again", [], False), ("qc_sites_out", ["--sites-out", "sites.tsv"], False),
                ("qc_pca", pca, False), ("qc_pca_sites_out", pca + ["--sites-out", "sites.tsv"], False)]
        for tag, extra, cold in runs:
            if cold:
                sb.drop_cache(store)
            wall, _, lines = sb.timed_eval(["-v", "-v", "--qc", "cohort.store"] + extra, d)
            split = [x for x in lines if x.startswith("store qc:")][0]
            res[tag] = {"wall_s": wall, "split": split}
            print("--qc %s: wall %.2f s; %s" % (" ".join(extra) or "(plain)", wall, split), flush=True)
        res["sites_out_bytes"] = os.path.getsize(os.path.join(d, "sites.tsv"))

        for tag, extra, count in (("single_file", [], k), ("single_file_pca", pca, min(k, 4))):
            t0 = time.perf_counter()
            for i in range(count):
                sb.timed_eval(extra + [names[i]], d)
            per = (time.perf_counter() - t0) / count
            res[tag] = {"files": count, "s_per_file": per, "s_for_n": per * n}
            print("one `ntsmEval %sFILE` per sample: %.3f s per file over %d files = %.0f s for %d samples"
                  % (" ".join(extra) + " " if extra else "", per, count, per * n, n), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
