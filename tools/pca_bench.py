#!/usr/bin/env python3
"""ntsmPCA at full size: the matrix of the tools/vcf_bench.py cohort (96,287 sites x 3,202 samples, written by
build/ntsmVCF -d -p), then `build/ntsmPCA -v` runs on it.

Prints one JSON line: the program's wall time by stage (read, parse, device, write) and its device steps (upload,
centre, Gram, eigen, projection, download), the Gram step's float64 FLOP/s counting n (n + 1) p operations (the
triangle) and its share of --peak-tflops (the vendor's float64 matrix figure, a data-sheet number), and yardsticks that
are not gates: in this process ntsm_amd.pca.gram on a random matrix of the same shape (device events, best and median
of --reps) beside torch.mm(A^T, A) in float64 on that shape (which computes the full square: twice the triangle's
operations), and where scikit-learn is importable the CPU time of PCA(svd_solver="full") on --sk-sites x --sk-samples.
--rocprof runs the program under `rocprofv3 --kernel-trace --stats` instead, with its output in --rocprof-out.

  python3 tools/pca_bench.py [--sites 96287] [--samples 3202] [--threads 16] [--components 20] [--dir DIR]
                             [--reps 5] [--split-sweep 3,6,12,23] [--no-torch] [--rocprof --rocprof-out DIR]
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
PCA = os.path.join(ROOT, "build", "ntsmPCA")
VCF = os.path.join(ROOT, "build", "ntsmVCF")


def make_matrix(d, n_sites, n_samples, seed, threads):
    """cohort.vcf of tools/vcf_bench.py through ntsmVCF -d -p: DIR/cohort_matrix.tsv"""
    import vcf_bench
    if not os.path.exists(os.path.join(d, "cohort.vcf")):
        vcf_bench.generate(d, n_sites, n_samples, seed)
    subprocess.run([VCF, "-d", "-t", str(threads), "-s", os.path.join(d, "sites.fa"), "-r", os.path.join(d, "genome.fa"),
                    "-p", os.path.join(d, "cohort"), os.path.join(d, "cohort.vcf")], check=True, stderr=subprocess.DEVNULL)
    os.remove(os.path.join(d, "cohort.vcf"))
    return os.path.join(d, "cohort_matrix.tsv")


def run_program(matrix, a, prefix, rocprof_out=None):
    cmd = [PCA, "-m", matrix, "-n", str(a.components), "-t", str(a.threads), "-p", prefix, "-v"]
    if rocprof_out:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", rocprof_out, "-o", "pca", "--"] + cmd
    t0 = time.time()
    p = subprocess.run(cmd, capture_output=True)
    wall = time.time() - t0
    err = p.stderr.decode(errors="replace")
    if p.returncode != 0:
        sys.stderr.write(err[-3000:])
        sys.exit(p.returncode)
    stages = {m.group(1): float(m.group(2)) for m in re.finditer(r"^\[pca\] (\w+): ([0-9.]+) s$", err, re.M)}
    dev = re.search(r"upload ([0-9.]+) ms, centre ([0-9.]+) ms, gram ([0-9.]+) ms \((\d+) tiles x (\d+) pieces, ([0-9.]+) TFLOP/s\), "
                    r"eigen ([0-9.]+) ms, projection ([0-9.]+) ms, download ([0-9.]+) ms", err)
    res = dict(wall_s=round(wall, 3), stages_s=stages)
    if dev:
        g = dev.groups()
        res["device_ms"] = dict(upload=float(g[0]), centre=float(g[1]), gram=float(g[2]), eigen=float(g[6]), projection=float(g[7]),
                                download=float(g[8]))
        res.update(gram_tiles=int(g[3]), gram_pieces=int(g[4]), gram_tflops=float(g[5]))
    return res


def in_process(a, res):
    """the library's Gram step and torch.mm on one random matrix of the same shape, in this process"""
    import torch
    import ntsm_amd.pca as pca
    rng = np.random.default_rng(a.seed)
    host = rng.random((a.sites, a.samples))
    ms = []
    for _ in range(a.reps + 1):                                                  # the first call warms the code object up
        _, _, t = pca.gram(host, centre=True)
        ms.append(t.gram_ms)
    ms = sorted(ms[1:])
    flops = t.gram_flops
    res["gram_in_process"] = dict(reps=a.reps, best_ms=round(ms[0], 3), median_ms=round(ms[len(ms) // 2], 3), flops=flops,
                                  best_tflops=round(flops / ms[0] * 1e-9, 2), median_tflops=round(flops / ms[len(ms) // 2] * 1e-9, 2),
                                  kernel_bytes=t.gram_bytes, centre_ms=round(t.centre_ms, 3), upload_ms=round(t.upload_ms, 1))
    if a.split_sweep:                                                            # how the auto split was chosen
        sweep = {}
        for split in (int(v) for v in a.split_sweep.split(",")):
            best = min(pca.gram(host, centre=True, split=split)[2].gram_ms for _ in range(3))
            sweep[split] = round(best, 3)
        res["gram_ms_by_split"] = sweep
    if a.no_torch:
        return
    x = torch.from_numpy(host).to("cuda")
    del host
    xt = x.t()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * (a.reps + 2))]
    tm = []
    for r in range(a.reps + 2):                                                  # two warm-ups: the library picks its kernel
        ev[2 * r].record()
        g = torch.mm(xt, x)
        ev[2 * r + 1].record()
        torch.cuda.synchronize()
        tm.append(ev[2 * r].elapsed_time(ev[2 * r + 1]))
        del g
    tm = sorted(tm[2:])
    full = 2 * a.samples * a.samples * a.sites
    res["torch_mm_f64"] = dict(reps=a.reps, best_ms=round(tm[0], 3), median_ms=round(tm[len(tm) // 2], 3), flops_full_square=full,
                               best_tflops=round(full / tm[0] * 1e-9, 2), torch=torch.__version__)


def sklearn_cpu(a, res):
    try:
        from sklearn.decomposition import PCA as SkPCA
    except ImportError:
        return
    x = np.random.default_rng(a.seed).random((a.sk_samples, a.sk_sites))
    t0 = time.time()
    SkPCA(n_components=a.components, svd_solver="full").fit_transform(x)
    res["sklearn_full_cpu"] = dict(samples=a.sk_samples, sites=a.sk_sites, seconds=round(time.time() - t0, 2))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sites", type=int, default=96287)
    ap.add_argument("--samples", type=int, default=3202)
    ap.add_argument("--components", type=int, default=20)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--peak-tflops", type=float, default=78.6)
    ap.add_argument("--sk-samples", type=int, default=600)
    ap.add_argument("--sk-sites", type=int, default=20000)
    ap.add_argument("--dir", default=None, help="keep the generated matrix here (reused when present)")
    ap.add_argument("--split-sweep", default=None, help="comma-separated piece counts: best Gram time of 3 calls for each")
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--rocprof-out", default=None)
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="pca_bench_")
    d = a.dir or tmp
    os.makedirs(d, exist_ok=True)
    try:
        t0 = time.time()
        matrix = os.path.join(d, "cohort_matrix.tsv")
        if not os.path.exists(matrix):
            make_matrix(d, a.sites, a.samples, a.seed, a.threads)
        res = dict(sites=a.sites, samples=a.samples, components=a.components, threads=a.threads, generate_s=round(time.time() - t0, 2),
                   matrix_bytes=os.path.getsize(matrix), rocprof=a.rocprof)
        prefix = os.path.join(tmp, "out")
        if a.rocprof:
            res.update(run_program(matrix, a, prefix, a.rocprof_out or os.path.join(tmp, "rocprof")))
        else:
            res["first_run"] = run_program(matrix, a, prefix)                    # loads the code objects, rocSOLVER and rocBLAS
            res.update(run_program(matrix, a, prefix))
            res["rotation_bytes"] = os.path.getsize(prefix + "_rotationalMatrix.tsv")
            in_process(a, res)
            sklearn_cpu(a, res)
        if "gram_tflops" in res:
            res["gram_share_of_peak"] = round(res["gram_tflops"] / a.peak_tflops, 3)
        print(json.dumps(res))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
