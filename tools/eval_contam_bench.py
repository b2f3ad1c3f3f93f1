#!/usr/bin/env python3
"""ntsmEval --contam on the store of tools/eval_store_bench.py: N samples x 96,287 sites of the
structured cohort of tools/eval_pca_bench.py, written from the documented layout.

  cli       `build/ntsmEval -vv --contam STORE`, once with the store out of the page cache and twice with it in, and once
            under -a (every row printed): whole-process wall time and the -vv split (map, upload, prepare, rectangle kernel,
            download, print)
  library   ntsm_eval_contam_rows over the mapped store, the whole rectangle in one band: resident, three runs; streamed in
            chunks of N / 4, one run (its records must be the resident run's bytes); and, for context only -- the two do
            different arithmetic -- the pair kernel of --within over the same store's triangle, two runs

Each part runs in a process of its own under a time limit.  There is no figure of an earlier version to compare with: before
--contam nothing printed this table.

    python tools/eval_contam_bench.py [--n 4096] [--dir DIR] [--json OUT]"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import eval_pca_bench as pb  # noqa: E402
import eval_store_bench as sb  # noqa: E402

M = pb.M


def mapped(store, n):
    import ntsm_amd.eval as ev
    buf = np.memmap(store, dtype=np.uint8, mode="r")
    loci = sum(len(b"rs%d\0" % s) for s in range(M))
    first = (64 + loci + 7) // 8 * 8 + 8 * M
    return ev, ev.Records(buf, first + 32 + sb.NAME, 32 + sb.NAME + 8 * M, n, M)


def step_cli(d, n, res):
    store = os.path.join(d, "cohort.store")
    for tag, extra, cold in (("cold", [], True), ("warm", [], False), ("warm_again", [], False), ("warm_all_rows", ["-a"], False),
                             ("warm_samples_out", ["--samples-out", "samples.tsv"], False)):
        if cold:
            sb.drop_cache(store)
        wall, _, lines = sb.timed_eval(["-v", "-v", "--contam", "cohort.store"] + extra, d)
        split = [x for x in lines if x.startswith("store contam:")][0]
        res["cli_" + tag] = {"wall_s": wall, "split": split}
        print("--contam %s(%s): wall %.2f s; %s" % (" ".join(extra) + " " if extra else "", tag, wall, split), flush=True)


def step_library(d, n, res):
    ev, rec = mapped(os.path.join(d, "cohort.store"), n)
    times = lambda t: dict(upload_ms=t.upload_ms, prepare_ms=t.prepare_kernel_ms, kernel_ms=t.cross_kernel_ms, download_ms=t.download_ms, chunks=t.chunks)  # noqa: E731
    runs, first = [], None
    with ev.Contam(rec, 1, 8) as s:
        for run in range(3):
            t0 = time.perf_counter()
            out, tally, t = s.rows(0, n)
            runs.append(dict(times(t), call_s=time.perf_counter() - t0))
            print("resident run %d: rectangle kernel %8.1f ms (upload %.1f, prepare %.1f, download %.1f ms), call %.2f s"
                  % (run, t.cross_kernel_ms, t.upload_ms, t.prepare_kernel_ms, t.download_ms, runs[-1]["call_s"]), flush=True)
            first = out if first is None else first
            assert out.tobytes() == first.tobytes()
    pairs = n * n
    res["resident"] = dict(runs=runs, kernel_median_ms=float(np.median([r["kernel_ms"] for r in runs])), pairs=pairs,
                           informative_sites_per_target=float(tally[:, 0].mean()))
    print("resident: median %.1f ms for %d ordered pairs x %d sites = %.1f G pair-sites/s; %.0f informative sites per target"
          % (res["resident"]["kernel_median_ms"], pairs, M, pairs * M / res["resident"]["kernel_median_ms"] / 1e6, tally[:, 0].mean()), flush=True)
    with ev.Contam(rec, 1, 8, n // 4) as s:
        t0 = time.perf_counter()
        out, _, t = s.rows(0, n)
        res["streamed"] = dict(times(t), call_s=time.perf_counter() - t0, same_bytes=bool(out.tobytes() == first.tobytes()))
        print("streamed in chunks of %d: rectangle kernel %8.1f ms (upload %.1f, prepare %.1f, download %.1f ms, %d chunks), call %.2f s, same bytes: %s"
              % (n // 4, t.cross_kernel_ms, t.upload_ms, t.prepare_kernel_ms, t.download_ms, t.chunks, res["streamed"]["call_s"], res["streamed"]["same_bytes"]), flush=True)
    del out, first
    within = []
    with ev.Within(rec, 1) as w:
        for run in range(2):
            _, _, t = w.rows(0, n)
            within.append(t.cross_kernel_ms)
            print("--within's pair kernel, run %d: %8.1f ms for the %d pairs of the triangle" % (run, t.cross_kernel_ms, n * (n - 1) // 2), flush=True)
    res["within_pair_kernel_ms"] = within


STEPS = {"cli": (step_cli, 600), "library": (step_library, 600)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:                                                                  # one part, in this process, over the store in --dir
        res = {}
        STEPS[a.step][0](a.dir, a.n, res)
        print("RESULT " + json.dumps(res), flush=True)
        return
    res = {"n": a.n, "sites": M}
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        t0 = time.perf_counter()
        cohort = pb.cohort(np.random.default_rng(7), a.n)
        store = os.path.join(d, "cohort.store")
        sb.write_store(store, ["s%05d.txt" % i for i in range(a.n)], cohort)
        del cohort
        res["store_bytes"] = os.path.getsize(store)
        print("store of %d samples x %d sites (%.3f GB) written in %.1f s" % (a.n, M, res["store_bytes"] / 1e9, time.perf_counter() - t0), flush=True)
        for step, (_, limit) in STEPS.items():                                  # a part that fails or runs out of time ends the run
            p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--dir", d, "--n", str(a.n)],
                               stdout=subprocess.PIPE, text=True)
            sys.stdout.write("".join(line + "\n" for line in p.stdout.split("\n")[:-1] if not line.startswith("RESULT ")))
            sys.stdout.flush()
            if p.returncode:
                print("step %s ended with status %d: stopping" % (step, p.returncode), flush=True)
                sys.exit(1)
            res.update(json.loads([line for line in p.stdout.split("\n") if line.startswith("RESULT ")][-1][7:]))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
