#!/usr/bin/env python3
"""The expansion kernel of the PCA library (ntsm_pca_expand: 16-bit cells -> the padded float64 matrix) at the size of
the tools/vcf_bench.py cohort, beside a hipMemset of the same padded buffer in the same process: both from HIP events.
The kernel reads 2 bytes and writes 8 per cell, the memset only writes, so the memset is the floor.  One JSON line.

  python3 tools/pca_expand_bench.py [--sites 96287] [--samples 3202] [--repeat 5]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def memset_ms(nbytes, repeat):
    hip = C.CDLL("libamdhip64.so")
    buf, e0, e1, ms = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_float()

    def chk(rc, what):
        if rc:
            raise RuntimeError("%s failed: %d" % (what, rc))
    chk(hip.hipMalloc(C.byref(buf), C.c_size_t(nbytes)), "hipMalloc")
    chk(hip.hipEventCreate(C.byref(e0)), "hipEventCreate")
    chk(hip.hipEventCreate(C.byref(e1)), "hipEventCreate")
    out = []
    for _ in range(repeat):
        chk(hip.hipEventRecord(e0, None), "hipEventRecord")
        chk(hip.hipMemsetAsync(buf, 0, C.c_size_t(nbytes), None), "hipMemsetAsync")
        chk(hip.hipEventRecord(e1, None), "hipEventRecord")
        chk(hip.hipEventSynchronize(e1), "hipEventSynchronize")
        chk(hip.hipEventElapsedTime(C.byref(ms), e0, e1), "hipEventElapsedTime")
        out.append(round(ms.value, 4))
    hip.hipEventDestroy(e0)
    hip.hipEventDestroy(e1)
    hip.hipFree(buf)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sites", type=int, default=96287)
    ap.add_argument("--samples", type=int, default=3202)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    import ntsm_amd.pca as pca
    rng = np.random.default_rng(1)
    codes = np.array([r | v << 8 for r in (0, 20, 40) for v in (0, 20, 40) if r + v], dtype=np.uint16)
    cells = codes[rng.integers(0, len(codes), size=(a.sites, a.samples))]
    cells[rng.random((a.sites, a.samples)) < 0.03] = 0
    value, fill = rng.random((2, 65536)), rng.random(a.sites)
    expand = []
    for _ in range(a.repeat):
        m, ms = pca.expand_cells(cells, value, fill, cells.size // 50)
        expand.append(round(ms, 4))
    del m
    p_pad, ld = (a.sites + 15) // 16 * 16, (a.samples + 127) // 128 * 128
    nbytes = p_pad * ld * 8
    ms = memset_ms(nbytes, a.repeat)
    best_e, best_m = min(expand), min(ms)
    print(json.dumps(dict(sites=a.sites, samples=a.samples, buffer_bytes=nbytes, cell_bytes=int(cells.nbytes), expand_ms=expand, hipMemset_ms=ms,
                          expand_write_gbps=round(nbytes / best_e / 1e6, 1), expand_total_gbps=round((nbytes + cells.nbytes) / best_e / 1e6, 1),
                          hipMemset_gbps=round(nbytes / best_m / 1e6, 1), expand_over_memset=round(best_e / best_m, 3))))


if __name__ == "__main__":
    main()
