#!/usr/bin/env python3
"""ntsmEval's PCA-guided search against a cohort store (--index / --near) on the structured cohort of
tools/eval_store_bench.py: N samples x 96,287 sites written as a store from the documented layout, Q = 1 and 8 queries that
are each the second replicate of an individual whose first is in the store, D = 20 components of a random rotation, every
sample at the small radius (-r 1 -1 0.05, S = 2).

  * the index build: `build/ntsmEval -vv --index STORE -p ROT -n NORM` (wall and split), and, in this process on the same
    samples, ntsm_eval_project_store on the mapped store (one pass, and passes of 1,024) against ntsm_eval_project on the
    dense samples, clouds compared bit for bit (profiles/r21_eval_near/projection_gate.txt is this step with the transposed
    projection kernel that was measured and not kept);
  * `build/ntsmEval -a -vv --near STORE QUERIES` for Q = 1 and 8, store cold and warm: wall time and its split (map + query
    load, projection of the queries, search, gather + score, print);
  * `build/ntsmEval -a -vv --against STORE QUERIES` on the same store, for comparison.

    python tools/eval_near_bench.py [--n 4096] [--dir DIR] [--json OUT]"""
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
FLAGS = ["-a", "-r", "1", "-1", "0.05", "-S", repr(pb.S)]


def write_matrices(d, rng):
    """norm.txt and rot.tsv as doubles printed with 17 digits (read back exactly); returns them as loadPCA reads them"""
    norm = 0.5 + rng.random(M) * 1e-3
    rot = rng.standard_normal((D, M)) * (pb.SCALE / np.sqrt(M))
    with open(os.path.join(d, "norm.txt"), "w") as f:
        f.write("".join("%.17g\n" % v for v in norm))
    with open(os.path.join(d, "rot.tsv"), "w") as f:
        f.write("rsID\t" + "\t".join("PC%d" % (k + 1) for k in range(D)) + "\n")
        for j in range(M):
            f.write("rs%d\t%s\n" % (j, "\t".join("%.17g" % v for v in rot[:, j])))
    return norm.astype(np.longdouble), rot.astype(np.longdouble)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n = a.n
    res = {"n": n, "sites": M, "dim": D}
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        rng = np.random.default_rng(7)
        t0 = time.perf_counter()
        both = pb.cohort(rng, n + 8)                                         # samples 2i, 2i + 1: one individual sequenced twice
        tail = both[n - 8:]                                                 # the last 8 individuals: one replicate each way
        cohort, queries = np.concatenate([both[:n - 8], tail[0::2]]), np.ascontiguousarray(tail[1::2])
        print("cohort of %d + 8 samples x %d sites generated in %.1f s" % (n, M, time.perf_counter() - t0), flush=True)
        prefix = np.char.add(np.char.add("rs", np.arange(M).astype(str)), "\t")
        names = ["s%05d.txt" % i for i in range(n)]
        qnames = ["q%d.txt" % i for i in range(8)]
        for i in range(8):
            sb.write_text(os.path.join(d, qnames[i]), queries[i], prefix)
        norm, rot = write_matrices(d, rng)
        store = os.path.join(d, "cohort.store")
        first, stride = sb.write_store(store, names, cohort)
        res["store_bytes"] = os.path.getsize(store)
        print("store of %d samples: %.3f GB" % (n, res["store_bytes"] / 1e9), flush=True)

        # the index build
        P = ["-p", "rot.tsv", "-n", "norm.txt", "-d", str(D)]
        wall, _, lines = sb.timed_eval(["-v", "-v", "--index", "cohort.store"] + P, d)
        split = [x for x in lines if x.startswith("store index:")][0]
        res["index"] = {"wall_s": wall, "split": split, "bytes": os.path.getsize(store + ".pcaidx")}
        print("--index, N = %d: wall %.2f s, index of %.2f MB; %s" % (n, wall, res["index"]["bytes"] / 1e6, split), flush=True)

        # the two projection kernels on the same samples, in one process
        import ntsm_amd.eval as ev
        mm = np.memmap(store, dtype=np.uint8, mode="r")
        rec = ev.Records(mm, first + 32 + sb.NAME, stride, n, M)
        res["projection"] = []
        for chunk in (0, 1024):
            cloud, geno, tm = ev.project_store(rec, norm, rot, min_cov=1, db_chunk=chunk)
            row = dict(kernel="store", chunk=chunk, chunks=tm.chunks, upload_ms=tm.upload_ms, prepare_ms=tm.prepare_kernel_ms,
                       project_ms=tm.cross_kernel_ms, download_ms=tm.download_ms)
            res["projection"].append(row)
            print("ntsm_eval_project_store, chunk %4d (%d passes): upload %7.1f ms, prepare %6.1f ms, projection kernel %7.1f ms, download %5.1f ms"
                  % (chunk, tm.chunks, tm.upload_ms, tm.prepare_kernel_ms, tm.cross_kernel_ms, tm.download_ms), flush=True)
        s = ev.Session(cohort, 1)
        for rep in range(2):
            want, ms = s.project(norm, rot)
            res["projection"].append(dict(kernel="session", project_ms=ms))
            print("ntsm_eval_project on the dense samples, run %d: projection kernel %7.1f ms" % (rep, ms), flush=True)
        s.close()
        res["projection_bits_equal"] = bool(want.tobytes() == cloud.tobytes())
        print("clouds %s bit for bit" % ("equal" if res["projection_bits_equal"] else "DIFFER"), flush=True)
        del mm, rec

        # --near and --against
        for mode, tag in (("--near", "store search:"), ("--against", "store query:")):
            flags = FLAGS if mode == "--near" else ["-a"]
            for q in (1, 8):
                for state in ("cold", "warm"):
                    if state == "cold":
                        sb.drop_cache(store)
                    wall, _, lines = sb.timed_eval(flags + ["-v", "-v", mode, "cohort.store"] + qnames[:q], d)
                    split = [x for x in lines if x.startswith(tag)][0]
                    res["%s_q%d_%s" % (mode[2:], q, state)] = {"wall_s": wall, "split": split}
                    print("%s, Q = %d, N = %d, store %s: wall %.2f s; %s" % (mode, q, n, state, wall, split), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
