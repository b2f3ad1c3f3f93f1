#!/usr/bin/env python3
"""PCA-guided pair search of ntsmEval (-p / -n; include/ntsm_eval_hip.h session calls) on a synthetic structured cohort:
K founder populations, individuals that differ from their population at a fraction of sites, and replicate pairs (the same
individual sequenced twice), 96,287 sites, D = 20 components of a random rotation, every sample at the small radius
(S = 2, the reference's default).  Prints, per N, the projection, search and scoring kernel times (HIP events), the number
of candidate pairs and the wall time of the whole PCA path; at N = 4,096 also the all-pairs kernel (ntsm_eval_pairs) on
the same counts for comparison.

    python tools/eval_pca_bench.py [N,N,...]        (default 4096,16384)"""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import ntsm_amd.eval as ev  # noqa: E402

M, D, K = 96287, 20, 64
FLIP, DEPTH, SCALE, S = 0.1, 10, 4.0, 2.0


def cohort(rng, n):
    """uint32 [n][M][2]: n // 2 individuals, each sequenced twice (replicates differ only in count noise)."""
    pops = rng.integers(0, 3, size=(K, M), dtype=np.int8)                 # 0 hom AT, 1 het, 2 hom CG
    out = np.empty((n, M, 2), dtype=np.uint32)
    g = None
    for i in range(n):
        if i % 2 == 0:
            g = pops[rng.integers(0, K)].copy()
            flip = rng.random(M) < FLIP
            g[flip] = rng.integers(0, 3, size=int(flip.sum()), dtype=np.int8)
        noise = rng.integers(0, 3, size=(M, 2), dtype=np.uint32)
        out[i, :, 0] = np.where(g == 0, DEPTH, np.where(g == 1, DEPTH // 2, 0)) + noise[:, 0]
        out[i, :, 1] = np.where(g == 2, DEPTH, np.where(g == 1, DEPTH // 2, 0)) + noise[:, 1] // 2
    return out


def main():
    sizes = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "4096,16384").split(",")]
    rng = np.random.default_rng(7)
    norm = np.full(M, 0.5, dtype=np.longdouble) + rng.random(M).astype(np.longdouble) * np.longdouble(1e-3)
    rot = (rng.standard_normal((D, M)) * (SCALE / np.sqrt(M))).astype(np.longdouble)
    print("sites %d, D %d, K %d founder populations, %.0f %% private sites, replicate pairs, radius S = %g (squared %g)"
          % (M, D, K, FLIP * 100, S, S * S), flush=True)
    for n in sizes:
        t0 = time.perf_counter()
        c = cohort(rng, n)
        gen = time.perf_counter() - t0
        t0 = time.perf_counter()
        s = ev.Session(c, 1)
        t_open = time.perf_counter() - t0
        t0 = time.perf_counter()
        cloud, ms_p = s.project(norm, rot)
        radius = np.full(n, S * S)
        pi, pk, dist, ms_c = s.candidates(cloud, radius)
        rec, ms_s = s.score_pairs(pi, pk)
        wall = time.perf_counter() - t0
        s.close()
        reps = int(np.sum((pi // 2 == pk // 2)))
        print("N=%d: projection %.1f ms, search %.2f ms, scoring %.1f ms (%d pairs, %d of them replicate pairs, %.3g per sample); "
              "PCA path kernels %.1f ms, wall %.2f s (session open incl. upload %.2f s; cohort generation %.1f s)"
              % (n, ms_p, ms_c, ms_s, len(pi), reps, len(pi) / n, ms_p + ms_c + ms_s, wall, t_open, gen), flush=True)
        if n == 4096:
            t0 = time.perf_counter()
            _, ms_a = ev.pairs(c, 1)
            print("N=%d: all-pairs kernel %.1f ms for %d pairs (whole call %.2f s)" % (n, ms_a, n * (n - 1) // 2, time.perf_counter() - t0),
                  flush=True)
        del c


if __name__ == "__main__":
    main()
