#!/usr/bin/env python3
"""ntsmEval --ld on the store of tools/eval_store_bench.py: N samples x 96,287 sites of the structured
cohort of tools/eval_pca_bench.py, written from the documented layout.  The cohort's sites are drawn independently: what LD it has
comes from its populations and replicate pairs, so the default run selects few pairs and times the planes and the triangle.

  cli        `build/ntsmEval -vv --ld STORE --ld-prune FILE`, once with the store out of the page cache and twice with it in:
             whole-process wall time, the -vv line, and the SHA-256 of stdout and of the kept list, which must not differ
  planes     ntsm_eval_ld_open over the mapped store, three sessions: upload and plane-kernel ms, TB/s of counts read
  select     ntsm_eval_ld_select over all rows (the triangle's tiles), three runs under the library's register block and under
             each forced one: kernel ms and pair-words per second, the pairs counted being those of the tiles evaluated
  rows       ntsm_eval_ld_rows on a band of 256 rows (the dense instance of the same kernel body), three runs

Each part runs in a process of its own under a time limit, and the first that fails ends the run.  There is no figure of an
earlier version to compare with: before --ld nothing printed this table.

    python tools/eval_ld_bench.py [--n 4096] [--dir DIR] [--json OUT]"""
import argparse
import hashlib
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
BLOCKS = ((0, 0), (2, 2), (4, 2), (2, 4))


def mapped(store, n):
    import ntsm_amd.eval as ev
    buf = np.memmap(store, dtype=np.uint8, mode="r")
    loci = sum(len(b"rs%d\0" % s) for s in range(M))
    first = (64 + loci + 7) // 8 * 8 + 8 * M
    return ev, ev.Records(buf, first + 32 + sb.NAME, 32 + sb.NAME + 8 * M, n, M)


def sha(path):
    h = hashlib.sha256()
    with open(path, "rb") as f:
        for part in iter(lambda: f.read(1 << 20), b""):
            h.update(part)
    return h.hexdigest()


def step_cli(d, n, res):
    store = os.path.join(d, "cohort.store")
    seen = set()
    for tag, cold in (("cold", True), ("warm", False), ("warm_again", False)):
        if cold:
            sb.drop_cache(store)
        t0 = time.perf_counter()
        with open(os.path.join(d, "ld.tsv"), "wb") as out:
            p = subprocess.run([sb.EVAL, "-v", "-v", "--ld", "cohort.store", "--ld-prune", "kept.txt"], cwd=d, stdout=out, stderr=subprocess.PIPE, text=True)
        wall = time.perf_counter() - t0
        if p.returncode:
            raise RuntimeError("ntsmEval --ld failed (%d): %s" % (p.returncode, p.stderr[-400:]))
        split = [x for x in p.stderr.split("\n") if x.startswith("store ld:")][0]
        digest = (sha(os.path.join(d, "ld.tsv")), sha(os.path.join(d, "kept.txt")))
        seen.add(digest)
        res["cli_" + tag] = {"wall_s": wall, "split": split, "stdout_sha256": digest[0], "kept_sha256": digest[1]}
        print("--ld (%s): wall %.2f s; %s" % (tag, wall, split), flush=True)
    assert len(seen) == 1, "the three runs differ"
    print("three runs: identical stdout (%s...) and kept list (%s...)" % (digest[0][:12], digest[1][:12]), flush=True)


def step_planes(d, n, res):
    ev, rec = mapped(os.path.join(d, "cohort.store"), n)
    runs = []
    for run in range(3):
        t0 = time.perf_counter()
        with ev.Ld(rec, 1, 8) as s:
            t = s.times
            runs.append(dict(upload_ms=t.upload_ms, kernel_ms=t.prepare_kernel_ms, download_ms=t.download_ms, chunks=t.chunks, call_s=time.perf_counter() - t0))
            geno = s.site_geno.copy()
        print("open %d: upload %.1f ms, plane and geno kernels %.2f ms, %d chunks, call %.2f s" % (run, t.upload_ms, t.prepare_kernel_ms, t.chunks, runs[-1]["call_s"]), flush=True)
    runs2 = []
    for run in range(3):                                                        # the plane kernel alone
        with ev.Ld(rec, 1, 8, site_geno=False) as s:
            runs2.append(s.times.prepare_kernel_ms)
    med = float(np.median(runs2))
    res["planes"] = dict(runs=runs, plane_kernel_ms=runs2, plane_kernel_median_ms=med, bytes=3 * ((n + 63) // 64) * 8 * M, counts_tb_per_s=n * M * 8 / med / 1e9,
                         mean_site_geno=[float(v) for v in geno.mean(0)])
    print("planes: %d bytes; plane kernel alone %s ms, median %.2f ms for %.3f GB of counts read = %.2f TB/s; mean het / homCG / called / homAT per site %s"
          % (res["planes"]["bytes"], ", ".join("%.2f" % v for v in runs2), med, n * M * 8 / 1e9, n * M * 8 / med / 1e9, " / ".join("%.0f" % v for v in geno.mean(0))), flush=True)


def tile_pairs(rows, cols):
    """the pairs of the tiles a _select call over all rows evaluates: tiles of rows x cols sites that hold a pair a < b"""
    tr, tc = 16 * rows, 16 * cols
    col_tiles = (M + tc - 1) // tc
    # column tile c holds a b > r0 exactly when c >= (r0 + 1) // tc
    return sum((col_tiles - (r0 + 1) // tc) * tr * tc for r0 in range(0, M, tr))


def step_select(d, n, res):
    ev, rec = mapped(os.path.join(d, "cohort.store"), n)
    w = (n + 63) // 64
    res["select"] = {}
    want = None
    try:
        with ev.Ld(rec, 1, 8, site_geno=False) as s:
            for block in BLOCKS:
                ev.ld_tune(*block)
                rr, rc = block if block[0] else (2, 2)
                pairs = tile_pairs(rr, rc)
                runs = []
                for run in range(3):
                    t0 = time.perf_counter()
                    code, got, found, ms = s.select(0, M, 20, 0.5, cap=1 << 22)
                    runs.append(dict(kernel_ms=ms, call_s=time.perf_counter() - t0, found=found))
                    assert code == 0
                    want = got.tobytes() if want is None else want
                    assert got.tobytes() == want
                med = float(np.median([r["kernel_ms"] for r in runs]))
                res["select"]["block_%dx%d" % block] = dict(runs=runs, kernel_median_ms=med, tile_pairs=pairs, pair_words_per_s=pairs * w / med * 1e3)
                print("select, block %d x %d: kernel median %.2f ms (%s), %d pairs found, %d pairs in the tiles x %d words = %.1f G pair-words/s, call %.2f s"
                      % (block + (med, ", ".join("%.2f" % r["kernel_ms"] for r in runs), found, pairs, w, pairs * w / med / 1e6, runs[-1]["call_s"])), flush=True)
    finally:
        ev.ld_tune(0, 0)


def step_rows(d, n, res):
    ev, rec = mapped(os.path.join(d, "cohort.store"), n)
    w, band = (n + 63) // 64, 256
    runs, first = [], None
    with ev.Ld(rec, 1, 8, site_geno=False) as s:
        for run in range(3):
            t0 = time.perf_counter()
            out, ms = s.rows(1000, band)
            runs.append(dict(kernel_ms=ms, call_s=time.perf_counter() - t0))
            first = out.tobytes() if first is None else first
            assert out.tobytes() == first
    med = float(np.median([r["kernel_ms"] for r in runs]))
    res["rows"] = dict(runs=runs, kernel_median_ms=med, pairs=band * M, pair_words_per_s=band * M * w / med * 1e3)
    print("rows, %d x %d: kernel median %.2f ms (%s) = %.1f G pair-words/s, call %.2f s"
          % (band, M, med, ", ".join("%.2f" % r["kernel_ms"] for r in runs), band * M * w / med / 1e6, runs[-1]["call_s"]), flush=True)


STEPS = {"cli": (step_cli, 600), "planes": (step_planes, 300), "select": (step_select, 600), "rows": (step_rows, 300)}


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
    res = {"n": a.n, "sites": M, "words": (a.n + 63) // 64}
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
