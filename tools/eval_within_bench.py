#!/usr/bin/env python3
"""ntsmEval inside a cohort store (--within / --within-near) on the structured cohort of
tools/eval_pca_bench.py: N samples x 96,287 sites written as a store from the documented layout (tools/eval_store_bench.py),
the first K of them also as text counts files.

Without --step this program touches no GPU: it runs the steps below as child processes, each under a time limit of its own,
and stops at the first that fails.

  prepare   the cohort, the store, the K text files, rotation and centre            (no GPU)
  parity    THE GATE.  The resident within kernel over the whole triangle in one band, at the workgroup width ntsm_eval_pairs'
            rule gives this N, against ntsm_eval_pairs' kernel_ms on the same counts, in one process, alternating, three runs
            each.  The two kernels then do the same arithmetic on the same tiles; the new one adds two pitch multiplies per
            site, so its median may exceed the old median by the old runs' own max - min spread plus 3 %, and no more.  The
            records are compared as bytes as well.  Exit 1 if it fails.
  widths    the same launch at forced widths 64 and 256 (ntsm_eval_within_tune), three runs each: the library's rule (64 at
            every size since this measurement) moves only if the other width wins outside the spread
  streamed  the same store with db_chunk = 1,024, as one band and as four
  cli       --index, then --within and --within-near, store cold and warm: wall time and the -vv split
  text      the text route on the K files that exist (all pairs, and -p): wall, loading, kernels; the N-file figure is an
            extrapolation of the per-file loading time and is printed as one

    python tools/eval_within_bench.py [--n 4096] [--files 128] [--dir DIR] [--json OUT]"""
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

import eval_near_bench as nb  # noqa: E402
import eval_pca_bench as pb  # noqa: E402
import eval_store_bench as sb  # noqa: E402

M, D = pb.M, pb.D
PCA_FLAGS = ["-r", "1", "-1", "0.05", "-S", repr(pb.S)]
STEPS = [("prepare", 900), ("parity", 300), ("widths", 300), ("streamed", 300), ("cli", 300), ("text", 600)]


def names_of(n):
    return ["s%05d.txt" % i for i in range(n)]


def mapped(d, n):
    """the store's samples as Records over a read-only mapping (kept alive by the Records)"""
    import ntsm_amd.eval as ev
    mm = np.memmap(os.path.join(d, "cohort.store"), dtype=np.uint8, mode="r")
    first = int(np.frombuffer(mm[24:32], dtype="<u8")[0])
    stride = int(np.frombuffer(mm[32:40], dtype="<u8")[0])
    return ev.Records(mm, first + 32 + sb.NAME, stride, n, M)


def dense(rec):
    rows = np.lib.stride_tricks.as_strided(rec.buf[rec.offset:], shape=(rec.n, 8 * rec.m), strides=(rec.stride, 1))
    return np.ascontiguousarray(rows).view(np.uint32).reshape(rec.n, rec.m, 2)


def prepare(d, n, k, res):
    rng = np.random.default_rng(7)
    t0 = time.perf_counter()
    cohort = pb.cohort(rng, n)
    print("cohort of %d samples x %d sites generated in %.1f s" % (n, M, time.perf_counter() - t0), flush=True)
    names = names_of(n)
    sb.write_store(os.path.join(d, "cohort.store"), names, cohort)
    res["store_bytes"] = os.path.getsize(os.path.join(d, "cohort.store"))
    print("store of %d samples: %.3f GB" % (n, res["store_bytes"] / 1e9), flush=True)
    prefix = np.char.add(np.char.add("rs", np.arange(M).astype(str)), "\t")
    t0 = time.perf_counter()
    for i in range(k):
        sb.write_text(os.path.join(d, names[i]), cohort[i], prefix)
    print("%d counts files written in %.1f s" % (k, time.perf_counter() - t0), flush=True)
    nb.write_matrices(d, rng)


def band_times(w, bands):
    """one pass over the given bands: (summed CrossTimes fields, wall s); the records are dropped"""
    tot = dict(upload_ms=0.0, prepare_ms=0.0, kernel_ms=0.0, download_ms=0.0, chunks=0)
    t0 = time.perf_counter()
    for first, rows in bands:
        _, _, tm = w.rows(first, rows)
        tot["upload_ms"] += tm.upload_ms
        tot["prepare_ms"] += tm.prepare_kernel_ms
        tot["kernel_ms"] += tm.cross_kernel_ms
        tot["download_ms"] += tm.download_ms
        tot["chunks"] += tm.chunks
    tot["wall_s"] = time.perf_counter() - t0
    return tot


def parity(d, n, k, res):
    import ntsm_amd.eval as ev
    rec = mapped(d, n)
    counts = dense(rec)
    old, new, same = [], [], True
    width = 64 if n <= 1024 else 256                                       # ntsm_eval_pairs' rule: the same tiles on both sides
    ev.within_tune(width)
    with ev.Within(rec, min_cov=1) as w:
        for run in range(3):
            want, ms = ev.pairs(counts, min_cov=1)
            old.append(ms)
            got, _, tm = w.rows(0, n)
            assert tm.chunks == 0, "the store is not resident on this device"
            new.append(tm.cross_kernel_ms)
            same = same and got.tobytes() == want.tobytes()
            print("run %d: ntsm_eval_pairs kernel %8.1f ms, within kernel %8.1f ms, records %s" % (run, ms, tm.cross_kernel_ms,
                  "equal as bytes" if same else "DIFFER"), flush=True)
    spread = max(old) - min(old)
    bound = float(np.median(old)) + spread + 0.03 * float(np.median(old))
    ok = same and float(np.median(new)) <= bound
    res["parity"] = dict(pairs_ms=old, within_ms=new, pairs_median=float(np.median(old)), within_median=float(np.median(new)), spread_ms=spread,
                         bound_ms=bound, width=width, records_equal=bool(same), passed=bool(ok))
    ev.within_tune(0)
    print("parity gate at width %d: within median %.1f ms against pairs median %.1f ms + spread %.1f ms + 3 %% = %.1f ms: %s"
          % (width, np.median(new), np.median(old), spread, bound, "PASSED" if ok else "FAILED"), flush=True)
    return 0 if ok else 1


def widths(d, n, k, res):
    import ntsm_amd.eval as ev
    rec = mapped(d, n)
    res["widths"] = {}
    with ev.Within(rec, min_cov=1) as w:
        w.rows(0, 1)                                                       # the first call reports open's upload; keep it out of the runs
        for run in range(3):
            for width in (64, 256):
                ev.within_tune(width)
                try:
                    tot = band_times(w, [(0, n)])
                finally:
                    ev.within_tune(0)
                res["widths"].setdefault(str(width), []).append(tot["kernel_ms"])
                print("width %3d, %d columns, run %d: within kernel %8.1f ms" % (width, n, run, tot["kernel_ms"]), flush=True)
    a, b = res["widths"]["64"], res["widths"]["256"]
    print("width 64: median %.1f ms (spread %.1f); width 256: median %.1f ms (spread %.1f); %d columns; the library's rule is 64"
          % (np.median(a), max(a) - min(a), np.median(b), max(b) - min(b), n), flush=True)


def streamed(d, n, k, res):
    import ntsm_amd.eval as ev
    rec = mapped(d, n)
    res["streamed"] = []
    quarter = -(-n // 4)
    four = [(f, min(quarter, n - f)) for f in range(0, n, quarter)]
    for chunk, bands, what in ((0, [(0, n)], "resident, one band"), (1024, [(0, n)], "db_chunk 1,024, one band"), (1024, four, "db_chunk 1,024, four bands")):
        t0 = time.perf_counter()
        with ev.Within(rec, min_cov=1, db_chunk=chunk) as w:
            tot = band_times(w, bands)
        tot.update(what=what, open_and_rows_s=time.perf_counter() - t0)
        res["streamed"].append(tot)
        print("%-28s: %2d column chunks, upload %7.1f ms, prepare %6.1f ms, pair kernel %8.1f ms, download %6.1f ms, open + rows %.2f s"
              % (what, tot["chunks"], tot["upload_ms"], tot["prepare_ms"], tot["kernel_ms"], tot["download_ms"], tot["open_and_rows_s"]), flush=True)


def cli(d, n, k, res):
    store = os.path.join(d, "cohort.store")
    wall, _, lines = sb.timed_eval(["-v", "-v", "--index", "cohort.store", "-p", "rot.tsv", "-n", "norm.txt", "-d", str(D)], d)
    print("--index, N = %d: wall %.2f s; %s" % (n, wall, [x for x in lines if x.startswith("store index:")][0]), flush=True)
    for mode, flags, tag in (("--within", [], "store within:"), ("--within-near", PCA_FLAGS, "store search:")):
        for state in ("cold", "warm"):
            if state == "cold":
                sb.drop_cache(store)
                if mode == "--within-near":
                    sb.drop_cache(store + ".pcaidx")
            wall, _, lines = sb.timed_eval(flags + ["-v", "-v", mode, "cohort.store"], d)
            split = [x for x in lines if x.startswith(tag)][0]
            res["%s_%s" % (mode[2:], state)] = {"wall_s": wall, "split": split}
            print("%s, N = %d, store %s: wall %.2f s; %s" % (mode, n, state, wall, split), flush=True)


def text(d, n, k, res):
    names = names_of(n)[:k]
    mark = "Finished loading files"
    wall, seen, lines = sb.timed_eval(["-v", "-v", "-t", "1"] + names, d, marks=(mark,))
    kern = [x for x in lines if x.startswith("pair kernel:")][0]
    res["text_all_pairs"] = {"files": k, "wall_s": wall, "load_s": seen[mark], "kernel": kern}
    print("text route, all pairs over the %d files that exist: wall %.2f s, of which loading %.2f s = %.4f s per file; %s"
          % (k, wall, seen[mark], seen[mark] / k, kern), flush=True)
    print("  extrapolated, not measured: loading %d files at that rate = %.0f s" % (n, seen[mark] / k * n), flush=True)
    wall, seen, lines = sb.timed_eval(["-v", "-v", "-t", "1", "-p", "rot.tsv", "-n", "norm.txt", "-d", str(D)] + PCA_FLAGS + names, d, marks=(mark,))
    kern = [x for x in lines if x.startswith("search kernels:")][0]
    res["text_pca"] = {"files": k, "wall_s": wall, "load_s": seen.get(mark), "kernels": kern}
    print("text route, -p over the %d files: wall %.2f s; %s" % (k, wall, kern), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--files", type=int, default=128, help="samples that also exist as text counts files")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    k = min(a.files, a.n)
    if a.step:                                                              # one step, in this process
        res = {}
        rc = globals()[a.step](a.dir, a.n, k, res) or 0
        with open(os.path.join(a.dir, a.step + ".json"), "w") as f:
            json.dump(res, f)
        sys.exit(rc)
    res = {"n": a.n, "sites": M, "files": k}
    rc = 0
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        for step, limit in STEPS:                                           # each under its own limit; nothing starts after a failure
            p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--dir", d, "--n", str(a.n),
                                "--files", str(k)])
            if os.path.exists(os.path.join(d, step + ".json")):
                res.update(json.load(open(os.path.join(d, step + ".json"))))
            if p.returncode:
                print("step %s ended with status %d: stopping" % (step, p.returncode), flush=True)
                rc = p.returncode
                break
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)
    sys.exit(rc)


if __name__ == "__main__":
    main()
