#!/usr/bin/env python3
"""ntsmEval --trios on the store of tools/eval_store_bench.py: N samples x 96,287 sites of the
structured cohort of tools/eval_pca_bench.py, written from the documented layout.  The cohort has replicate pairs and
populations, no families: under the defaults every sample has one candidate (its replicate) and nothing is scored, so the
default run times the planes and the duo rectangle; --trio-duo 0.06 lets a sample's population in and gives lists of about 66.

  cli       `build/ntsmEval -vv --trios STORE`, once with the store out of the page cache and twice with it in, and once with
            --trio-duo 0.06: whole-process wall time and the -vv line
  planes    ntsm_eval_trio_open over the mapped store, three sessions: upload and plane-kernel ms
  duos      the whole duo rectangle in one call, three runs: kernel ms and pair-words per second; for context only -- the two
            do different arithmetic -- the pair kernel of --within over the same store's triangle, two runs
  score     ntsm_eval_trio_score on the exhaustive lists of the first 256 samples among themselves (256 x 32,385 triples),
            three runs: kernel ms and triple-words per second; and on N entries of length 3, three runs; both again under the
            other tile (ntsm_eval_trio_tune) for the launch rule

Each part runs in a process of its own under a time limit, and the first that fails ends the run.  There is no figure of an
earlier version to compare with: before --trios nothing printed this table.

    python tools/eval_trio_bench.py [--n 4096] [--dir DIR] [--json OUT]"""
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
W = (M + 63) // 64


def mapped(store, n):
    import ntsm_amd.eval as ev
    buf = np.memmap(store, dtype=np.uint8, mode="r")
    loci = sum(len(b"rs%d\0" % s) for s in range(M))
    first = (64 + loci + 7) // 8 * 8 + 8 * M
    return ev, ev.Records(buf, first + 32 + sb.NAME, 32 + sb.NAME + 8 * M, n, M)


def step_cli(d, n, res):
    store = os.path.join(d, "cohort.store")
    for tag, extra, cold in (("cold", [], True), ("warm", [], False), ("warm_again", [], False), ("warm_duo_0.06", ["--trio-duo", "0.06"], False)):
        if cold:
            sb.drop_cache(store)
        wall, _, lines = sb.timed_eval(["-v", "-v", "--trios", "cohort.store"] + extra, d)
        split = [x for x in lines if x.startswith("store trios:")][0]
        res["cli_" + tag] = {"wall_s": wall, "split": split}
        print("--trios %s(%s): wall %.2f s; %s" % (" ".join(extra) + " " if extra else "", tag, wall, split), flush=True)


def step_planes(d, n, res):
    ev, rec = mapped(os.path.join(d, "cohort.store"), n)
    runs = []
    for run in range(3):
        t0 = time.perf_counter()
        with ev.Trio(rec, 1, 8) as s:
            t = s.times
            runs.append(dict(upload_ms=t.upload_ms, kernel_ms=t.prepare_kernel_ms, download_ms=t.download_ms, chunks=t.chunks, call_s=time.perf_counter() - t0))
            geno = s.geno.copy()
        print("open %d: upload %.1f ms, plane and geno kernels %.2f ms, %d chunks, call %.2f s" % (run, t.upload_ms, t.prepare_kernel_ms, t.chunks, runs[-1]["call_s"]), flush=True)
    res["planes"] = dict(runs=runs, kernel_median_ms=float(np.median([r["kernel_ms"] for r in runs])), bytes=3 * W * 8 * n,
                         mean_geno=[float(v) for v in geno.mean(0)])
    print("planes: %d bytes; median %.2f ms for %.3f GB of counts read = %.0f GB/s; mean homAT / het / homCG / miss per sample %s"
          % (3 * W * 8 * n, res["planes"]["kernel_median_ms"], n * M * 8 / 1e9, n * M * 8 / res["planes"]["kernel_median_ms"] / 1e6,
             " / ".join("%.0f" % v for v in geno.mean(0))), flush=True)


def step_duos(d, n, res):
    ev, rec = mapped(os.path.join(d, "cohort.store"), n)
    runs, first = [], None
    with ev.Trio(rec, 1, 8, geno=False) as s:
        for run in range(3):
            t0 = time.perf_counter()
            out, ms = s.duos(0, n)
            runs.append(dict(kernel_ms=ms, call_s=time.perf_counter() - t0))
            print("duo rectangle %d: kernel %8.2f ms, call %.2f s" % (run, ms, runs[-1]["call_s"]), flush=True)
            first = out if first is None else first
            assert out.tobytes() == first.tobytes()
    med = float(np.median([r["kernel_ms"] for r in runs]))
    res["duos"] = dict(runs=runs, kernel_median_ms=med, pairs=n * n, pair_words_per_s=n * n * W / med * 1e3)
    print("duos: median %.2f ms for %d ordered pairs x %d words = %.1f G pair-words/s" % (med, n * n, W, n * n * W / med / 1e6), flush=True)
    del out, first
    within = []
    with ev.Within(rec, 1) as w:
        for run in range(2):
            _, _, t = w.rows(0, n)
            within.append(t.cross_kernel_ms)
            print("--within's pair kernel, run %d: %8.1f ms for the %d pairs of the triangle" % (run, t.cross_kernel_ms, n * (n - 1) // 2), flush=True)
    res["within_pair_kernel_ms"] = within


def step_score(d, n, res):
    ev, rec = mapped(os.path.join(d, "cohort.store"), n)
    first = min(256, n)
    dense = (list(range(first)), [[p for p in range(first) if p != k] for k in range(first)])
    rng = np.random.default_rng(11)
    short = (list(range(n)), [[int(v) for v in (k + 1 + rng.choice(n - 1, 3, replace=False)) % n] for k in range(n)])
    res["score"] = {}
    try:
        with ev.Trio(rec, 1, 8, geno=False) as s:
            for tag, (children, lists) in (("dense", dense), ("short", short)):
                triples = sum(len(l) * (len(l) - 1) // 2 for l in lists)
                want = None
                for width in (0, 64, 256):
                    ev.trio_tune(width)
                    runs = []
                    for run in range(3):
                        t0 = time.perf_counter()
                        out, ms = s.score(children, lists)
                        runs.append(dict(kernel_ms=ms, call_s=time.perf_counter() - t0))
                        want = out.tobytes() if want is None else want
                        assert out.tobytes() == want
                    med = float(np.median([r["kernel_ms"] for r in runs]))
                    res["score"]["%s_width_%d" % (tag, width)] = dict(runs=runs, kernel_median_ms=med, triples=triples, triple_words_per_s=triples * W / med * 1e3)
                    print("score %s, %d entries, %d triples, width %d: kernel median %.2f ms (%s), %.1f G triple-words/s, call %.3f s"
                          % (tag, len(children), triples, width, med, ", ".join("%.2f" % r["kernel_ms"] for r in runs), triples * W / med / 1e6, runs[-1]["call_s"]), flush=True)
    finally:
        ev.trio_tune(0)


STEPS = {"cli": (step_cli, 600), "planes": (step_planes, 300), "duos": (step_duos, 600), "score": (step_score, 600)}


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
    res = {"n": a.n, "sites": M, "words": W}
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
