#!/usr/bin/env python3
"""ntsmEval's cohort store and query mode (--pack / --against) on the structured cohort of
tools/eval_pca_bench.py: N samples x 96,287 sites, Q = 1 and 8 queries drawn as further replicates.

Text counts files are slow to write and to read (that is the point of the store), so only K of the N samples exist as
files: `--pack` and the all-pairs run are timed on those K (+ Q) files, both read one file after the other on one thread,
and their figures are given per file.  The store of all N samples is written here from the documented layout; its first K
records are compared with the bytes `--pack` wrote for the K files.  Then:

  * `build/ntsmEval -a -vv --against STORE QUERIES` for Q = 1 and 8: wall time and its split (map + query load, upload, prepare,
    cross kernel, download, print), once cold and once with the store in the page cache;
  * the all-pairs `build/ntsmEval -vv` on the K + Q files: wall time, the time until the files are loaded (the stderr line
    "Finished loading files"), the pair kernel;
  * ntsm_eval_cross on the mapped store for every workgroup width and query group (ntsm_eval_cross_tune) and two chunk sizes:
    what the launch rule of ntsm_amd/csrc/ntsm_eval_cross.hip rests on.

    python tools/eval_store_bench.py [--n 4096] [--files 128] [--dir DIR] [--json OUT]"""
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

import eval_pca_bench as pb  # noqa: E402

EVAL = os.path.join(ROOT, "build", "ntsmEval")
M = pb.M
NAME = 1024


def write_text(path, counts, prefix):
    """one counts file as ntsmCount prints it; sums = counts, distinct 13 / 13"""
    a, b = counts[:, 0].astype(str), counts[:, 1].astype(str)
    tab = np.char.add
    lines = tab(tab(tab(tab(tab(tab(tab(prefix, a), "\t"), b), "\t"), a), "\t"), tab(b, "\t13\t13\n"))
    with open(path, "w") as f:
        f.write("#@TK\t%d\n#@KS\t19\n#locusID\tcountAT\tcountCG\tsumAT\tsumCG\tdistinctAT\tdistinctCG\n" % (int(counts.sum()) * 40))
        f.write("".join(lines.tolist()))


def write_store(path, names, cohort):
    """the layout of ntsm_amd/csrc/host/eval_store.hpp, written independently of it"""
    loci = b"".join(b"rs%d\0" % s for s in range(M))
    pad = (64 + len(loci) + 7) // 8 * 8
    first, stride = pad + 8 * M, 32 + NAME + 8 * M
    with open(path, "wb") as f:
        f.write(b"NTSMCOH1" + struct.pack("<IIQQQ", 1, M, len(names), first, stride) + bytes(24))
        f.write(loci + bytes(pad - 64 - len(loci)))
        f.write(np.full((M, 2), 13, dtype="<u4").tobytes())
        for name, c in zip(names, cohort):
            total = int((c[:, 0] + c[:, 1]).astype(np.uint64).sum())
            f.write(struct.pack("<QQQII", int(c.sum()) * 40, total, total, 19, 0) + name.encode().ljust(NAME, b"\0"))
            f.write(np.ascontiguousarray(c, dtype="<u4").tobytes())
    return first, stride


def timed_eval(args, cwd, marks=()):
    """run build/ntsmEval, stdout discarded; returns (wall s, {mark: s since start when a stderr line contains it}, stderr lines)"""
    t0 = time.perf_counter()
    p = subprocess.Popen([EVAL] + args, cwd=cwd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
    seen, lines = {}, []
    for line in p.stderr:
        lines.append(line.rstrip("\n"))
        for m in marks:
            if m in line and m not in seen:
                seen[m] = time.perf_counter() - t0
    rc = p.wait()
    wall = time.perf_counter() - t0
    if rc:
        raise RuntimeError("ntsmEval %s failed (%d): %s" % (" ".join(args[:4]), rc, lines[-3:]))
    return wall, seen, lines


def drop_cache(path):
    fd = os.open(path, os.O_RDONLY)
    try:
        os.fsync(fd)
        os.posix_fadvise(fd, 0, 0, os.POSIX_FADV_DONTNEED)
    finally:
        os.close(fd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--files", type=int, default=128, help="samples that also exist as text counts files")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    n, k = a.n, min(a.files, a.n)
    res = {"n": n, "sites": M, "files": k}
    with tempfile.TemporaryDirectory(dir=a.dir) as d:
        rng = np.random.default_rng(7)
        t0 = time.perf_counter()
        both = pb.cohort(rng, n + 8)
        cohort, queries = both[:n], both[n:]
        print("cohort of %d + 8 samples x %d sites generated in %.1f s" % (n, M, time.perf_counter() - t0), flush=True)
        prefix = np.char.add(np.char.add("rs", np.arange(M).astype(str)), "\t")
        names = ["s%05d.txt" % i for i in range(n)]
        qnames = ["q%d.txt" % i for i in range(8)]
        t0 = time.perf_counter()
        for i in range(k):
            write_text(os.path.join(d, names[i]), cohort[i], prefix)
        for i in range(8):
            write_text(os.path.join(d, qnames[i]), queries[i], prefix)
        text_bytes = os.path.getsize(os.path.join(d, names[0]))
        print("%d + 8 counts files of %.2f MB written in %.1f s" % (k, text_bytes / 1e6, time.perf_counter() - t0), flush=True)

        # --pack on the K files
        wall, _, _ = timed_eval(["--pack", "k.store"] + names[:k], d)
        res["pack_s_per_file"] = wall / k
        first, stride = write_store(os.path.join(d, "cohort.store"), names, cohort)
        size = os.path.getsize(os.path.join(d, "cohort.store"))
        packed = open(os.path.join(d, "k.store"), "rb").read()
        with open(os.path.join(d, "cohort.store"), "rb") as f:
            mine = f.read(first + k * stride)
        same = packed[:16] == mine[:16] and packed[24:] == mine[24:] and struct.unpack_from("<Q", packed, 16)[0] == k
        res.update(store_bytes=size, pack_equals_layout=bool(same))
        print("--pack: %.2f s for %d files = %.3f s per file (%.0f s for %d); store of %d samples: %.3f GB (text: %.2f GB); "
              "--pack's bytes %s the layout's" % (wall, k, wall / k, wall / k * n, n, n, size / 1e9, text_bytes * n / 1e9,
                                                   "equal" if same else "DIFFER FROM"), flush=True)
        os.remove(os.path.join(d, "k.store"))

        # --against
        for q in (1, 8):
            for state in ("cold", "warm"):
                if state == "cold":
                    drop_cache(os.path.join(d, "cohort.store"))
                wall, _, lines = timed_eval(["-a", "-v", "-v", "--against", "cohort.store"] + qnames[:q], d)
                split = [x for x in lines if x.startswith("store query:")][0]
                res["against_q%d_%s" % (q, state)] = {"wall_s": wall, "split": split}
                print("--against, Q = %d, N = %d, store %s: wall %.2f s; %s" % (q, n, state, wall, split), flush=True)

        # the all-pairs run on K + Q files
        for q in (1, 8):
            mark = "Finished loading files"
            wall, seen, lines = timed_eval(["-v", "-v", "-t", "1"] + qnames[:q] + names[:k], d, marks=(mark,))
            kern = [x for x in lines if x.startswith("pair kernel:")][0]
            res["all_pairs_q%d" % q] = {"files": k + q, "wall_s": wall, "load_s": seen[mark], "kernel": kern}
            print("all pairs over %d files: wall %.2f s, of which loading %.2f s = %.3f s per file (%.0f s for %d files); %s"
                  % (k + q, wall, seen[mark], seen[mark] / (k + q), seen[mark] / (k + q) * (n + q), n + q, kern), flush=True)

        # the launch shapes of the cross kernel, on the mapped store
        import ntsm_amd.eval as ev
        import ctypes as C
        mm = np.memmap(os.path.join(d, "cohort.store"), dtype=np.uint8, mode="r")
        base = mm.ctypes.data + first + 32 + NAME
        res["shapes"] = []
        for q in (1, 8):
            qc = np.ascontiguousarray(queries[:q])
            for chunk in (0, 1024):
                for width in (64, 256):
                    for group in ((1,) if q == 1 else (1, 2, 4)):
                        assert ev.lib.ntsm_eval_cross_tune(width, group) == 0
                        out = np.zeros((q, n), dtype=ev.RECORD)
                        geno = np.zeros((n, 3), dtype=np.uint32)
                        tm = ev.CrossTimes()
                        t0 = time.perf_counter()
                        rc = ev.lib.ntsm_eval_cross(0, qc.ctypes.data, q, base, stride, n, M, 1, chunk, out.ctypes.data, geno.ctypes.data, C.byref(tm))
                        wall = time.perf_counter() - t0
                        assert rc == 0 and int(out["n_valid"].min()) > 0
                        row = dict(q=q, chunk=chunk, width=width, group=group, chunks=tm.chunks, wall_s=wall, upload_ms=tm.upload_ms,
                                   prepare_ms=tm.prepare_kernel_ms, cross_ms=tm.cross_kernel_ms, download_ms=tm.download_ms)
                        res["shapes"].append(row)
                        print("cross Q = %d, chunk %4d (%d passes), width %3d, query group %d: upload %7.1f ms, prepare %6.1f ms, "
                              "cross kernel %7.1f ms, download %5.1f ms, call %.2f s"
                              % (q, chunk, tm.chunks, width, group, tm.upload_ms, tm.prepare_kernel_ms, tm.cross_kernel_ms, tm.download_ms, wall), flush=True)
        ev.lib.ntsm_eval_cross_tune(0, 0)
        del mm
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
