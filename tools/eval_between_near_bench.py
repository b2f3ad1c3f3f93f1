#!/usr/bin/env python3
"""ntsmEval --between-near (the PCA-guided search between two cohort stores) on the structured cohort of
tools/eval_between_bench.py: NA + NB samples x 96,287 sites, store A one replicate of each of the first NA individuals, store
B the other replicate and every further sample, every sample at the small radius (-r 1 -1 0.05, S = 2).  Bmap.store holds B's
samples over a locus table of its own: A's loci in a random order, 1 % of them absent.  All stores are written from the
documented layout.

Without --step this program touches no GPU: it runs the steps below as child processes, each under a time limit of its own,
and stops at the first that fails.

  prepare   the cohort, A.store, B.store, Bmap.store, rotation and centre                                  (no GPU)
  index     --index A.store and --index B.store: wall and split
  runs      three command lines alternating, three rounds (the first with the stores dropped from the page cache), wall and the
            -vv split of each: --between-near A.store B.store (B's projections from its index); --between-near A.store Bmap.store
            (B projected in the run through the map); --between A.store B.store, the route without the search -- with
            --between-exe at another build's ntsmEval (the parent commit's, whose only route this is), else at this build's
  remap     a window of B through ntsm_eval_project_store (no map) and ntsm_eval_project_store_mapped under the identity given
            as a map and under a random permutation, no components: upload ms and prepare ms (the tallies, with the remap in
            front of them where there is a map), three runs each

    python tools/eval_between_near_bench.py [--na 1024] [--nb 4096] [--dir DIR] [--json OUT] [--between-exe PATH]"""
import argparse
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import eval_between_bench as bb  # noqa: E402
import eval_near_bench as nb_  # noqa: E402
import eval_pca_bench as pb  # noqa: E402
import eval_store_bench as sb  # noqa: E402

M, D = pb.M, pb.D
PCA_FLAGS = ["-r", "1", "-1", "0.05", "-S", repr(pb.S)]
STEPS = [("prepare", 900), ("index", 300), ("runs", 600), ("remap", 300)]


def write_store_over(path, names, cohort, order):
    """sb.write_store with a locus table of its own: the store's site t is locus rs<order[t]>"""
    m = len(order)
    loci = b"".join(b"rs%d\0" % s for s in order)
    pad = (64 + len(loci) + 7) // 8 * 8
    first, stride = pad + 8 * m, 32 + sb.NAME + 8 * m
    with open(path, "wb") as f:
        f.write(b"NTSMCOH1" + struct.pack("<IIQQQ", 1, m, len(names), first, stride) + bytes(24))
        f.write(loci + bytes(pad - 64 - len(loci)))
        f.write(np.full((m, 2), 13, dtype="<u4").tobytes())
        for name, c in zip(names, cohort):
            c = c[order]
            total = int((c[:, 0] + c[:, 1]).astype(np.uint64).sum())
            f.write(struct.pack("<QQQII", int(c.sum()) * 40, total, total, 19, 0) + name.encode().ljust(sb.NAME, b"\0"))
            f.write(np.ascontiguousarray(c, dtype="<u4").tobytes())


def prepare(d, na, nb, res, exe):
    rng = np.random.default_rng(7)
    t0 = time.perf_counter()
    cohort = pb.cohort(rng, na + nb)
    print("cohort of %d samples x %d sites generated in %.1f s" % (na + nb, M, time.perf_counter() - t0), flush=True)
    in_a = np.zeros(na + nb, dtype=bool)
    in_a[0:2 * na:2] = True                                                # one replicate of each of the first NA individuals
    sb.write_store(os.path.join(d, "A.store"), bb.names_of("a", na), cohort[in_a])
    sb.write_store(os.path.join(d, "B.store"), bb.names_of("b", nb), cohort[~in_a])
    order = rng.permutation(M)[:M - M // 100]
    write_store_over(os.path.join(d, "Bmap.store"), bb.names_of("b", nb), cohort[~in_a], order)
    res["store_bytes"] = [os.path.getsize(os.path.join(d, s)) for s in ("A.store", "B.store", "Bmap.store")]
    print("A.store %.3f GB, B.store %.3f GB, Bmap.store (%d of %d loci, random order) %.3f GB" % (res["store_bytes"][0] / 1e9, res["store_bytes"][1] / 1e9,
          len(order), M, res["store_bytes"][2] / 1e9), flush=True)
    nb_.write_matrices(d, rng)


def index(d, na, nb, res, exe):
    for store in ("A.store", "B.store"):
        wall, _, lines = sb.timed_eval(["-v", "-v", "--index", store, "-p", "rot.tsv", "-n", "norm.txt", "-d", str(D)], d)
        split = [x for x in lines if x.startswith("store index:")][0]
        res["index_" + store[0]] = {"wall_s": wall, "split": split}
        print("--index %s: wall %.2f s; %s" % (store, wall, split), flush=True)


def runs(d, na, nb, res, exe):
    """the three command lines alternating, three rounds, the first with the stores dropped from the page cache"""
    lines_of = (("between_near_index", "--between-near, B from its index", PCA_FLAGS + ["-v", "-v", "--between-near", "A.store", "B.store"], "store between-near:", None),
                ("between_near_mapped", "--between-near, B projected through a mapped table", PCA_FLAGS + ["-v", "-v", "--between-near", "A.store", "Bmap.store"],
                 "store between-near:", None),
                ("between", "--between" + (" (%s)" % a_name(exe) if exe else ""), ["-v", "-v", "--between", "A.store", "B.store"], "store between:", exe))
    for key, _, _, _, _ in lines_of:
        res[key] = {"wall_s": [], "splits": []}
    for run in range(3):
        if run == 0:
            for s in ("A.store", "B.store", "Bmap.store", "A.store.pcaidx", "B.store.pcaidx"):
                sb.drop_cache(os.path.join(d, s))
        for key, what, args, tag, other in lines_of:
            if other:
                t0 = time.perf_counter()
                p = subprocess.run([other] + args, cwd=d, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
                wall, lines = time.perf_counter() - t0, p.stderr.split("\n")
                if p.returncode:
                    raise RuntimeError("%s failed (%d): %s" % (other, p.returncode, lines[-3:]))
            else:
                wall, _, lines = sb.timed_eval(args, d)
            split = [x for x in lines if x.startswith(tag)][0]
            res[key]["wall_s"].append(wall)
            res[key]["splits"].append(split)
            print("%s, %d x %d, run %d (%s): wall %.2f s; %s" % (what, na, nb, run, "cold" if run == 0 else "warm", wall, split), flush=True)
    for key, what, _, _, _ in lines_of:
        w = res[key]["wall_s"]
        res[key].update(median_s=float(np.median(w)), spread_s=max(w) - min(w))
        print("%s: %s s, median %.2f, spread %.2f" % (what, " / ".join("%.2f" % x for x in w), np.median(w), max(w) - min(w)), flush=True)


def a_name(exe):
    """the other build's ntsmEval as the report names it: its last three path components"""
    return os.sep.join(exe.split(os.sep)[-3:])


def remap(d, na, nb, res, exe):
    import ntsm_amd.eval as ev
    window = min(1024, nb)
    rng = np.random.default_rng(11)
    b = bb.mapped(d, "B.store", window)
    norm, rot = np.full(M, 0.5, dtype=np.longdouble), np.zeros((0, M), dtype=np.longdouble)
    cases = (("ntsm_eval_project_store (no map)", "none"), ("remap, identity", np.arange(M, dtype=np.uint32)), ("remap, random order", rng.permutation(M).astype(np.uint32)))
    res["remap"] = []
    for what, site_map in cases:
        runs = []
        for run in range(3):
            if isinstance(site_map, str):
                tm = ev.project_store(b, norm, rot, min_cov=1)[2]
            else:
                tm = ev.project_store_mapped(b, M, site_map, norm, rot, min_cov=1)[2]
            assert tm.chunks == 1
            runs.append((tm.upload_ms, tm.prepare_kernel_ms))
        res["remap"].append(dict(what=what, window=window, upload_ms=[r[0] for r in runs], prepare_ms=[r[1] for r in runs]))
        print("%-34s: window of %d samples x %d sites of B (%.2f GB dense): upload %s ms, prepare (%stallies) %s ms"
              % (what, window, M, window * M * 8 / 1e9, " / ".join("%.1f" % r[0] for r in runs), "" if isinstance(site_map, str) else "remap + ",
                 " / ".join("%.2f" % r[1] for r in runs)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--na", type=int, default=1024)
    ap.add_argument("--nb", type=int, default=4096)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--between-exe", default=None, help="the ntsmEval of another build for the --between step")
    ap.add_argument("--step", default=None, choices=[s for s, _ in STEPS])
    a = ap.parse_args()
    exe = os.path.abspath(a.between_exe) if a.between_exe else None
    if a.step:                                                              # one step, in this process
        res = {}
        rc = globals()[a.step](a.dir, a.na, a.nb, res, exe) or 0
        with open(os.path.join(a.dir, a.step + ".json"), "w") as f:
            json.dump(res, f)
        sys.exit(rc)
    res = {"na": a.na, "nb": a.nb, "sites": M, "dim": D}
    rc = 0
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        for step, limit in STEPS:                                           # each under its own limit; nothing starts after a failure
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step, "--dir", d, "--na", str(a.na), "--nb", str(a.nb)]
            p = subprocess.run(cmd + (["--between-exe", exe] if exe else []))
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
