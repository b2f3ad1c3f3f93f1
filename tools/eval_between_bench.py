#!/usr/bin/env python3
"""ntsmEval --between (one cohort store against another) on the structured cohort of
tools/eval_pca_bench.py: NA + NB samples x 96,287 sites.  Store A takes one replicate of each of the first NA individuals,
store B the other replicate and every further sample, so each sample of A has its match in B.  Both stores are written from
the documented layout (tools/eval_store_bench.py); the first K samples of A also exist as text counts files.

Without --step this program touches no GPU: it runs the steps below as child processes, each under a time limit of its own,
and stops at the first that fails.

  prepare   the cohort, A.store, B.store, the K text files                                              (no GPU)
  widths    the rectangle kernel over all of A against a resident B at forced widths 64 and 256 (ntsm_eval_between_tune),
            alternating, three runs each: the library's default moves only if the other width wins outside the spread
  holdings  B resident against B forced to 4 chunks: the split of open + one band, and the wall time of both
  staging   a window of B staged by ntsm_eval_chunk.h's kernels (site_map = NULL) and by the mapped kernels under the identity
            given as a map, under A's order with 1 % of the loci absent, and under a random permutation: upload and prepare ms
            and the bytes the kernels move
  cli       --between A.store B.store with the stores cold and warm: wall time and the -vv split
  text      the route the parent commit has: --against B.store with the K text files of A as queries: wall, loading, kernel;
            the NA-file figure is an extrapolation of the per-file loading time and is printed as one

    python tools/eval_between_bench.py [--na 1024] [--nb 4096] [--files 128] [--dir DIR] [--json OUT]"""
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
LACKS = 0xFFFFFFFF
STEPS = [("prepare", 900), ("widths", 300), ("holdings", 300), ("staging", 300), ("cli", 300), ("text", 600)]


def names_of(prefix, n):
    return ["%s%05d.txt" % (prefix, i) for i in range(n)]


def mapped(d, store, n):
    """a store's samples as Records over a read-only mapping (kept alive by the Records)"""
    import ntsm_amd.eval as ev
    mm = np.memmap(os.path.join(d, store), dtype=np.uint8, mode="r")
    first = int(np.frombuffer(mm[24:32], dtype="<u8")[0])
    stride = int(np.frombuffer(mm[32:40], dtype="<u8")[0])
    return ev.Records(mm, first + 32 + sb.NAME, stride, n, M)


def prepare(d, na, nb, k, res):
    rng = np.random.default_rng(7)
    t0 = time.perf_counter()
    cohort = pb.cohort(rng, na + nb)
    print("cohort of %d samples x %d sites generated in %.1f s" % (na + nb, M, time.perf_counter() - t0), flush=True)
    in_a = np.zeros(na + nb, dtype=bool)
    in_a[0:2 * na:2] = True                                                # one replicate of each of the first NA individuals
    sb.write_store(os.path.join(d, "A.store"), names_of("a", na), cohort[in_a])
    sb.write_store(os.path.join(d, "B.store"), names_of("b", nb), cohort[~in_a])
    res["store_bytes"] = [os.path.getsize(os.path.join(d, s)) for s in ("A.store", "B.store")]
    print("A.store of %d samples: %.3f GB; B.store of %d samples: %.3f GB" % (na, res["store_bytes"][0] / 1e9, nb, res["store_bytes"][1] / 1e9), flush=True)
    prefix = np.char.add(np.char.add("rs", np.arange(M).astype(str)), "\t")
    t0 = time.perf_counter()
    for i, name in enumerate(names_of("a", na)[:k]):
        sb.write_text(os.path.join(d, name), cohort[2 * i], prefix)
    print("%d counts files written in %.1f s" % (k, time.perf_counter() - t0), flush=True)


def split_of(tm):
    return dict(upload_ms=tm.upload_ms, prepare_ms=tm.prepare_kernel_ms, kernel_ms=tm.cross_kernel_ms, download_ms=tm.download_ms, chunks=tm.chunks)


def widths(d, na, nb, k, res):
    import ntsm_amd.eval as ev
    res["widths"] = {}
    with ev.Between(mapped(d, "A.store", na), mapped(d, "B.store", nb), min_cov=1) as s:
        tm = s.rows(0, 1)[3]                                               # the first call reports open's upload; keep it out of the runs
        assert tm.chunks == 0, "B is not resident on this device"
        for run in range(3):
            for width in (64, 256):
                ev.between_tune(width)
                try:
                    rec, _, _, tm = s.rows(0, na)
                finally:
                    ev.between_tune(0)
                assert int(rec["n_valid"].min()) > 0
                res["widths"].setdefault(str(width), []).append(tm.cross_kernel_ms)
                print("width %3d, %d x %d, run %d: rectangle kernel %8.1f ms" % (width, na, nb, run, tm.cross_kernel_ms), flush=True)
    a, b = res["widths"]["64"], res["widths"]["256"]
    print("width 64: median %.1f ms (spread %.1f); width 256: median %.1f ms (spread %.1f)" % (np.median(a), max(a) - min(a), np.median(b), max(b) - min(b)),
          flush=True)


def holdings(d, na, nb, k, res):
    import ntsm_amd.eval as ev
    res["holdings"] = []
    for chunk, what in ((0, "B resident"), (-(-nb // 4), "B in 4 chunks")):
        t0 = time.perf_counter()
        with ev.Between(mapped(d, "A.store", na), mapped(d, "B.store", nb), min_cov=1, b_chunk=chunk) as s:
            tot = split_of(s.rows(0, na)[3])
        tot.update(what=what, open_and_rows_s=time.perf_counter() - t0)
        res["holdings"].append(tot)
        print("%-14s: %d chunks of B, upload %7.1f ms, prepare %6.1f ms, rectangle kernel %8.1f ms, download %6.1f ms, open + one band %.2f s"
              % (what, tot["chunks"], tot["upload_ms"], tot["prepare_ms"], tot["kernel_ms"], tot["download_ms"], tot["open_and_rows_s"]), flush=True)


def staging(d, na, nb, k, res):
    import ntsm_amd.eval as ev
    window = min(1024, nb)
    rng = np.random.default_rng(11)
    a, b = mapped(d, "A.store", 1), mapped(d, "B.store", window)
    b_dense = np.ascontiguousarray(np.lib.stride_tricks.as_strided(b.buf[b.offset:], shape=(window, 8 * M), strides=(b.stride, 1))).view(np.uint32).reshape(window, M, 2)
    kept = np.sort(rng.choice(M, size=M - M // 100, replace=False))
    fewer = np.full(M, LACKS, dtype=np.uint32)
    fewer[kept] = np.arange(len(kept), dtype=np.uint32)                     # A's order, 1 % of the loci absent: monotone
    cases = (("ntsm_eval_chunk.h (no map)", None, b), ("mapped, identity", np.arange(M, dtype=np.uint32), b),
             ("mapped, 1 % absent", fewer, ev.Records.of(b_dense[:, kept])), ("mapped, random order", rng.permutation(M).astype(np.uint32), b))
    res["staging"] = []
    for what, site_map, records in cases:
        runs = []
        for run in range(3):
            with ev.Between(a, records, site_map=site_map, min_cov=1) as s:
                tm = s.rows(0, 1)[3]                                       # open's upload and preparation, plus one row of A
            assert tm.chunks == 0
            runs.append((tm.upload_ms, tm.prepare_kernel_ms))
        mb = window * records.m * 8                                        # the dense window: read once by the transpose, once by the tallies
        moved = 2 * mb + window * M * 16 + (0 if site_map is None else 2 * 4 * M * -(-window // 64))
        res["staging"].append(dict(what=what, window=window, sites_b=records.m, upload_ms=[r[0] for r in runs], prepare_ms=[r[1] for r in runs], kernel_bytes=moved))
        print("%-28s: window of %d samples x %d sites of B: upload %s ms, prepare (transpose + tallies, + one row of A) %s ms, %.2f GB moved by the kernels"
              % (what, window, records.m, " / ".join("%.1f" % r[0] for r in runs), " / ".join("%.2f" % r[1] for r in runs), moved / 1e9), flush=True)


def cli(d, na, nb, k, res):
    for state in ("cold", "warm"):
        if state == "cold":
            for s in ("A.store", "B.store"):
                sb.drop_cache(os.path.join(d, s))
        wall, _, lines = sb.timed_eval(["-v", "-v", "--between", "A.store", "B.store"], d)
        split = [x for x in lines if x.startswith("store between:")][0]
        res["between_%s" % state] = {"wall_s": wall, "split": split}
        print("--between, %d x %d, stores %s: wall %.2f s; %s" % (na, nb, state, wall, split), flush=True)


def text(d, na, nb, k, res):
    names = names_of("a", na)[:k]
    mark = "Finished loading files"
    wall, seen, lines = sb.timed_eval(["-v", "-v", "-t", "1", "--against", "B.store"] + names, d, marks=(mark,))
    split = [x for x in lines if x.startswith("store query:")][0]
    res["text_against"] = {"files": k, "wall_s": wall, "load_s": seen[mark], "split": split}
    print("text route, --against B.store with the %d files of A that exist: wall %.2f s, of which map + loading %.2f s = %.4f s per file; %s"
          % (k, wall, seen[mark], seen[mark] / k, split), flush=True)
    print("  extrapolated, not measured: loading %d files at that rate = %.0f s" % (na, seen[mark] / k * na), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--na", type=int, default=1024)
    ap.add_argument("--nb", type=int, default=4096)
    ap.add_argument("--files", type=int, default=128, help="samples of A that also exist as text counts files")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    k = min(a.files, a.na)
    if a.step:                                                              # one step, in this process
        res = {}
        rc = globals()[a.step](a.dir, a.na, a.nb, k, res) or 0
        with open(os.path.join(a.dir, a.step + ".json"), "w") as f:
            json.dump(res, f)
        sys.exit(rc)
    res = {"na": a.na, "nb": a.nb, "sites": M, "files": k}
    rc = 0
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        for step, limit in STEPS:                                           # each under its own limit; nothing starts after a failure
            p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--dir", d, "--na", str(a.na),
                                "--nb", str(a.nb), "--files", str(k)])
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
