#!/usr/bin/env python3
"""ntsmPCA --store on the cohort of tools/eval_pca_bench.py (96,287 sites, N = 4,096 samples by default):

  genotype   ntsm_pca_store_genotype's HIP-event time per chunk (ntsm_amd.pca.store_cells at --chunk samples and unchunked, three
             calls each, the first one warms up), as bytes per second for the 10 B per cell it moves (8 in, 2 out); beside it the
             staging of the same chunk that ntsmEval's store paths run -- prepare_kernel (8 B in, 16 B out per cell) and the
             tally kernel, ntsm_eval_cross with one query: times.prepare_kernel_ms per chunk -- and the tally kernel alone
             (ntsm_eval_project_store with one component: its prepare_kernel_ms)
  end to end `build/ntsmPCA --store cohort.store -p st -v`, its -v lines kept, beside `build/ntsmPCA -m M.tsv -p mt -v` on the
             matrix text of the same genotypes; the two runs' rotation and components are compared byte for byte

    python tools/pca_store_bench.py [--samples 4096] [--chunk 1024] [--threads 16] [--out DIR] [--no-text]"""
import argparse
import json
import os
import re
import struct
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

import ntsm_amd.eval as ev  # noqa: E402
import ntsm_amd.pca as pca  # noqa: E402
from eval_pca_bench import M, cohort  # noqa: E402

PCA = os.path.join(ROOT, "build", "ntsmPCA")
RECORD_HEAD = 1056


def say(*a):
    print(*a, flush=True)


def write_store(path, counts, loci, names):
    """DESIGN.md section 9.1, record by record"""
    n, m = counts.shape[0], counts.shape[1]
    section = b"".join(l.encode() + b"\0" for l in loci)
    section += bytes(-(64 + len(section)) % 8) + np.ones((m, 2), dtype="<u4").tobytes()
    with open(path, "wb") as f:
        f.write(b"NTSMCOH1" + struct.pack("<IIQQQ", 1, m, n, 64 + len(section), RECORD_HEAD + 8 * m) + bytes(24) + section)
        for r in range(n):
            total = int((counts[r, :, 0] + counts[r, :, 1]).astype(np.uint64).sum())
            f.write(struct.pack("<QQQII", 0, total, total, 19, 0) + names[r].encode().ljust(1024, b"\0") + counts[r].tobytes())


def write_matrix_text(path, cells, tallies, loci, names):
    """NAME_matrix.tsv of the store's genotypes: 0 / 0.5 / 1, a missing cell as its site's centre (%.19Lg of the quotient)"""
    with open(path, "wb") as f:
        f.write(("alleleID\t" + "\t".join(names) + "\n").encode())
        for s in range(cells.shape[0]):
            h, o, c = (int(x) for x in tallies[s])
            centre = b"0"
            if c and (cells[s] == 0).any():
                assert (o + 0.5 * h) / c >= 1e-4                                        # below that %.19Lg switches to exponent form
                q = np.format_float_positional(np.longdouble(o + 0.5 * h) / np.longdouble(c), precision=19, unique=False, fractional=False, trim="-")
                centre = q.encode()
            words = np.array([centre, b"0", b"0.5", b"1"], dtype=object)
            f.write(loci[s].encode() + b"\t" + b"\t".join(words[cells[s]].tolist()) + b"\n")


def cli(args, cwd):
    t0 = time.perf_counter()
    p = subprocess.run([PCA] + args, cwd=cwd, capture_output=True, timeout=1500)
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        raise SystemExit("ntsmPCA %s failed: %s" % (" ".join(args), p.stderr.decode()[-600:]))
    return wall, p.stderr.decode()


def numbers(err):
    """the -v lines as {name: value}: "[pca] what: x s" laps and the "name x ms" pairs of the device lines"""
    out = {}
    for what, x in re.findall(r"\[pca\] ([a-z ]+): ([0-9.]+) s", err):
        out[what.strip() + "_s"] = float(x)
    for what, x in re.findall(r"([a-z]+(?: and [a-z]+)?) ([0-9.]+) ms", err):
        out[what.replace(" ", "_") + "_ms"] = float(x)
    m = re.search(r"store: (\d+) chunks of (\d+) samples", err)
    if m:
        out["chunks"], out["chunk"] = int(m.group(1)), int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=1024)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=".", help="directory of pca_store_bench.json")
    ap.add_argument("--no-text", action="store_true", help="skip the matrix-text route")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    n, res = a.samples, {"sites": M, "samples": a.samples, "chunk": a.chunk}
    t0 = time.perf_counter()
    counts = cohort(np.random.default_rng(7), n)
    say("cohort: %d sites x %d samples (tools/eval_pca_bench.py), generated in %.1f s" % (M, n, time.perf_counter() - t0))

    # ---- the genotype kernel per chunk, beside the staging kernels of ntsmEval's store paths on the same chunk
    for chunk in (a.chunk, 0):
        per = []
        for _ in range(3):
            cells, tallies, st = pca.store_cells(counts, min_cov=1, db_chunk=chunk)
            per.append(st.genotype_ms / st.chunks)
        width = st.chunk
        gbs = 10.0 * M * width / (min(per) * 1e-3) / 1e9
        res["genotype_chunk%d" % chunk] = {"samples_per_chunk": width, "chunks": st.chunks, "ms_per_chunk": per, "upload_ms": st.upload_ms,
                                          "GBps_10B_per_cell": gbs}
        say("genotype kernel, %d chunk(s) of %d samples: %s ms per chunk -> %.0f GB/s at 10 B per cell (upload of the last call %.0f ms)"
            % (st.chunks, width, " / ".join("%.3f" % x for x in per), gbs, st.upload_ms))
    assert int(cells.min()) >= 0 and int(cells.max()) <= 3 and int(tallies[:, 2].max()) <= n
    norm = np.full(M, 0.5, dtype=np.longdouble)
    rot = np.zeros((1, M), dtype=np.longdouble)
    per_cross, per_tally = [], []
    for _ in range(3):
        _, _, tc = ev.cross(counts[:1], counts, min_cov=1, db_chunk=a.chunk)
        per_cross.append(tc.prepare_kernel_ms / tc.chunks)
        _, _, tp = ev.project_store(counts, norm, rot, min_cov=1, db_chunk=a.chunk)
        per_tally.append(tp.prepare_kernel_ms / tp.chunks)
    res["eval_staging"] = {"samples_per_chunk": a.chunk, "prepare_plus_tally_ms_per_chunk": per_cross, "tally_ms_per_chunk": per_tally}
    say("ntsmEval's staging of the same chunk: transpose (prepare_kernel, 24 B per cell) + tallies %s ms per chunk (ntsm_eval_cross, one query: "
        "its row's transpose is in the first chunk's share); tallies alone %s ms (ntsm_eval_project_store)"
        % (" / ".join("%.3f" % x for x in per_cross), " / ".join("%.3f" % x for x in per_tally)))

    # ---- end to end
    with tempfile.TemporaryDirectory(dir=os.environ.get("TMPDIR", "/tmp")) as tmp:
        loci = ["rs%d" % s for s in range(M)]
        names = ["run%05d" % r for r in range(n)]
        t0 = time.perf_counter()
        write_store(os.path.join(tmp, "cohort.store"), counts, loci, names)
        say("store written in %.1f s (%.2f GB)" % (time.perf_counter() - t0, os.path.getsize(os.path.join(tmp, "cohort.store")) / 1e9))
        del counts
        for k in range(2):                                                              # the second run reads the store from the page cache
            wall, err = cli(["--store", "cohort.store", "-p", "st", "-t", str(a.threads), "-v"], tmp)
            res["cli_store_run%d" % k] = dict(numbers(err), wall_s=wall)
            say("ntsmPCA --store, run %d: wall %.2f s\n%s" % (k, wall, err.rstrip()))
        if not a.no_text:
            t0 = time.perf_counter()
            write_matrix_text(os.path.join(tmp, "M.tsv"), cells, tallies, loci, names)
            say("matrix text written in %.1f s (%.2f GB)" % (time.perf_counter() - t0, os.path.getsize(os.path.join(tmp, "M.tsv")) / 1e9))
            wall, err = cli(["-m", "M.tsv", "-p", "mt", "-t", str(a.threads), "-v"], tmp)
            res["cli_matrix"] = dict(numbers(err), wall_s=wall)
            say("ntsmPCA -m M.tsv: wall %.2f s\n%s" % (wall, err.rstrip()))
            same = all(open(os.path.join(tmp, "st" + s), "rb").read() == open(os.path.join(tmp, "mt" + s), "rb").read()
                       for s in ("_rotationalMatrix.tsv", "_components.tsv"))
            res["same_bytes_as_matrix_route"] = same
            say("rotation and components of the two routes: %s" % ("the same bytes" if same else "DIFFERENT"))
    with open(os.path.join(a.out, "pca_store_bench.json"), "w") as f:
        json.dump(res, f, indent=1)
    say("wrote " + os.path.join(a.out, "pca_store_bench.json"))


if __name__ == "__main__":
    main()
