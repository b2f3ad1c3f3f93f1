#!/usr/bin/env python3
"""ntsmVCF at full size: a seeded cohort of 96,287 sites x 3,202 samples (the site count of human_sites_n10, a
1000 Genomes-sized panel) generated on this machine, then one `build/ntsmVCF -d -p` run with NTSM_VCF_PROF=1.

Prints one JSON line with the phase split: sites, genome, parse, events (CSR), upload, state kernel, sum kernel (HIP
events), download, format + write, wall time, and the state kernel's bytes over its time.  The inputs (about 1.2 GB of
VCF text) and the matrix (1-7 GB of text, depending on where the first undefined cell falls) live in a temporary
directory that is removed afterwards, unless --dir names one to keep the inputs in (the matrix is removed anyway).
--rocprof runs the same command under `rocprofv3 --kernel-trace --stats` instead, with its output in --rocprof-out.
--rotation measures the three routes from the VCF to the rotation on the same inputs instead and prints one JSON line
per leg: `ntsmVCF -p`, then `ntsmPCA` on its matrix; `ntsmVCF -R`; `ntsmVCF -R -M` -- wall time of every program and its
lap lines (--raw-out DIR keeps every program's stderr laps as text).
--store measures the route from the VCF to a cohort store instead and prints one JSON line per leg: `ntsmVCF --store`
(lap lines, the records kernel's bytes over its time), then, for scale, the two-step route `ntsmVCF --counts DIR` and
`ntsmEval --pack` of DIR's files (--no-two-step leaves that leg out: at full size it writes about 10 GB of text).

  python3 tools/vcf_bench.py [--sites 96287] [--samples 3202] [--threads 16] [--seed 1] [--dir DIR]
                             [--rocprof --rocprof-out DIR] [--rotation [--dims 20] [--raw-out DIR]]
                             [--store [--no-two-step] [--raw-out DIR]]
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
VCF = os.path.join(ROOT, "build", "ntsmVCF")
PCA = os.path.join(ROOT, "build", "ntsmPCA")
EVAL = os.path.join(ROOT, "build", "ntsmEval")
ALT = {65: 71, 67: 84, 71: 65, 84: 67}


def generate(d, n_sites, n_samples, seed, k=19):
    """Chromosomes of random bases with one SNP every 30-50 bases; 2 % of the sites are not in the VCF, 0.02 % of
    the lines are duplicated with other genotypes (conflicting inserts), genotypes mostly phased, a few unparsed."""
    rng = np.random.default_rng(seed)
    n_chrom = 8
    per = (n_sites + n_chrom - 1) // n_chrom
    sites = open(os.path.join(d, "sites.fa"), "wb")
    genome = open(os.path.join(d, "genome.fa"), "wb")
    vcf = open(os.path.join(d, "cohort.vcf"), "wb")
    vcf.write(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" +
              "\t".join("HG%05d" % i for i in range(n_samples)).encode() + b"\n")
    table = np.frombuffer(b"0|0\t0|1\t1|0\t1|1\t./.\t0/1\t", dtype=np.uint8).reshape(6, 4)
    weights = np.array([0.45, 0.15, 0.15, 0.2, 0.03, 0.02])
    done = 0
    for c in range(n_chrom):
        m = min(per, n_sites - done)
        if m <= 0:
            break
        gaps = rng.integers(30, 51, size=m)
        pos = 60 + np.cumsum(gaps)                                              # 1-based SNP positions
        seq = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=int(pos[-1]) + 60)
        genome.write(b">chr%d\n" % c + seq.tobytes() + b"\n")
        absent = rng.random(m) < 0.02
        dup = rng.random(m) < 0.0002
        for start in range(0, m, 2048):
            idx = np.arange(start, min(m, start + 2048))
            reps = 1 + dup[idx]
            codes = rng.choice(6, size=(int(reps.sum()), n_samples), p=weights)
            rows = table[codes]
            rows[:, -1, 3] = 10
            r = 0
            for i, nrep in zip(idx, reps):
                p = int(pos[i])
                b = int(seq[p - 1])
                name = b"rs%d_%d" % (c, p)
                w = seq[p - k:p + k - 1].copy()
                sites.write(b">" + name + b"\n" + w.tobytes() + b"\n")
                w[k - 1] = ALT[b]
                sites.write(b">" + name + b"_v\n" + w.tobytes() + b"\n")
                for _ in range(nrep):
                    if not absent[i]:
                        vcf.write(b"chr%d\t%d\t%s\t%c\t%c\t.\tPASS\t.\tGT\t" % (c, p, name, b, ALT[b]) + rows[r].tobytes())
                    r += 1
        done += m
    for f in (sites, genome, vcf):
        f.close()


def laps(err):
    """The lap lines of a program's stderr: {"[vcf] parse": seconds, ...} and the device lines as text"""
    phases = {m.group(1) + " " + m.group(2): float(m.group(3)) for m in re.finditer(r"^(\[(?:vcf|pca)\]) ([^:\n]+): ([0-9.]+) s$", err, re.M)}
    device = [l for l in err.splitlines() if l.startswith(("[vcf] device:", "[pca] device:"))]
    return phases, device


def rotation_legs(a, d, tmp):
    """Three routes to NAME_center.txt + NAME_rotationalMatrix.tsv + NAME_components.tsv, in one session"""
    env = dict(os.environ, NTSM_VCF_PROF="1")
    common = [VCF, "-d", "-t", str(a.threads), "-s", os.path.join(d, "sites.fa"), "-r", os.path.join(d, "genome.fa")]
    vcf = os.path.join(d, "cohort.vcf")
    two, fused, nomat = os.path.join(tmp, "two"), os.path.join(tmp, "fused"), os.path.join(tmp, "nomat")
    legs = [("two_programs", [common + ["-p", two, vcf],
                              [PCA, "-v", "-t", str(a.threads), "-n", str(a.dims), "-m", two + "_matrix.tsv", "-p", two]]),
            ("rotation", [common + ["-R", "-n", str(a.dims), "-p", fused, vcf]]),
            ("rotation_no_matrix", [common + ["-R", "-M", "-n", str(a.dims), "-p", nomat, vcf]])]
    raw = []
    for name, cmds in legs:
        res = dict(leg=name, sites=a.sites, samples=a.samples, threads=a.threads, dims=a.dims, programs=[])
        total = 0.0
        for cmd in cmds:
            t0 = time.time()
            p = subprocess.run(cmd, env=env, capture_output=True)
            wall = time.time() - t0
            err = p.stderr.decode(errors="replace")
            if p.returncode != 0:
                sys.stderr.write(err[-3000:])
                sys.exit(p.returncode)
            phases, device = laps(err)
            total += wall
            res["programs"].append(dict(program=os.path.basename(cmd[0]), wall_s=round(wall, 3), laps_s=phases, device=device))
            raw.append("== %s: %s\n" % (name, " ".join(os.path.basename(c) if os.sep in c else c for c in cmd)) +
                       "".join(l + "\n" for l in err.splitlines() if l.startswith(("[vcf]", "[pca]", "Time:", "Matrix:"))))
        res["wall_s"] = round(total, 3)
        print(json.dumps(res), flush=True)
    same = all(open(two + s, "rb").read() == open(fused + s, "rb").read() for s in ("_center.txt", "_rotationalMatrix.tsv", "_components.tsv"))
    same = same and all(open(fused + s, "rb").read() == open(nomat + s, "rb").read() for s in ("_center.txt", "_rotationalMatrix.tsv", "_components.tsv"))
    print(json.dumps(dict(leg="check", same_bytes_on_every_route=same, matrix_bytes=os.path.getsize(fused + "_matrix.tsv"))), flush=True)
    if a.raw_out:
        os.makedirs(a.raw_out, exist_ok=True)
        with open(os.path.join(a.raw_out, "laps.txt"), "w") as f:
            f.write("".join(raw))


def store_legs(a, d, tmp):
    """The VCF to a cohort store: in one run, and through counts files and ntsmEval --pack"""
    env = dict(os.environ, NTSM_VCF_PROF="1")
    common = [VCF, "-d", "-t", str(a.threads), "-s", os.path.join(d, "sites.fa"), "-r", os.path.join(d, "genome.fa")]
    vcf = os.path.join(d, "cohort.vcf")
    one, two, cdir = os.path.join(tmp, "one.store"), os.path.join(tmp, "two.store"), os.path.join(tmp, "counts")
    os.makedirs(cdir)
    files = [os.path.join(cdir, "HG%05d.counts.txt" % i) for i in range(a.samples)]
    legs = [("store", [common + ["--store", one, vcf]])]
    if not a.no_two_step:
        legs.append(("counts_then_pack", [common + ["--counts", cdir, vcf], [EVAL, "--pack", two] + files]))
    raw = []
    for name, cmds in legs:
        res = dict(leg=name, sites=a.sites, samples=a.samples, threads=a.threads, programs=[])
        total = 0.0
        for cmd in cmds:
            t0 = time.time()
            p = subprocess.run(cmd, env=env, capture_output=True)
            wall = time.time() - t0
            err = p.stderr.decode(errors="replace")
            if p.returncode != 0:
                sys.stderr.write(err[-3000:])
                sys.exit(p.returncode)
            phases, device = laps(err)
            rec = re.search(r"^\[vcf\] records device: windows (\d+) of (\d+) samples, upload ([0-9.]+) s, kernel ([0-9.]+) s, "
                            r"download ([0-9.]+) s, kernel bytes (\d+)$", err, re.M)
            prog = dict(program=os.path.basename(cmd[0]), wall_s=round(wall, 3), laps_s=phases, device=device)
            if rec:
                w, ws, up, ks, down, nb = (float(x) for x in rec.groups())
                prog.update(records_windows=int(w), records_window_samples=int(ws), records_upload_s=up, records_kernel_s=ks,
                            records_download_s=down, records_kernel_bytes=int(nb), records_kernel_gbps=round(nb / ks / 1e9, 1) if ks > 0 else None)
            total += wall
            res["programs"].append(prog)
            raw.append("== %s: %s\n" % (name, " ".join(os.path.basename(c) if os.sep in c else c for c in cmd[:12])) +
                       "".join(l + "\n" for l in err.splitlines() if l.startswith(("[vcf]", "Time:"))))
        res["wall_s"] = round(total, 3)
        res["store_bytes"] = os.path.getsize(one if name == "store" else two)
        if name != "store":
            res["counts_text_bytes"] = sum(os.path.getsize(f) for f in files)
        print(json.dumps(res), flush=True)
    if a.raw_out:
        os.makedirs(a.raw_out, exist_ok=True)
        with open(os.path.join(a.raw_out, "laps.txt"), "w") as f:
            f.write("".join(raw))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--sites", type=int, default=96287)
    ap.add_argument("--samples", type=int, default=3202)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir", default=None, help="keep the generated inputs here (reused when present)")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--rocprof-out", default=None)
    ap.add_argument("--rotation", action="store_true", help="measure the routes to the rotation instead (three legs)")
    ap.add_argument("--dims", type=int, default=20)
    ap.add_argument("--raw-out", default=None)
    ap.add_argument("--store", action="store_true", help="measure the routes to a cohort store instead (two legs)")
    ap.add_argument("--no-two-step", action="store_true", help="with --store: leave the --counts + --pack leg out")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="vcf_bench_")
    d = a.dir or tmp
    os.makedirs(d, exist_ok=True)
    try:
        t0 = time.time()
        if not os.path.exists(os.path.join(d, "cohort.vcf")):
            generate(d, a.sites, a.samples, a.seed)
        gen_s = time.time() - t0
        if a.rotation:
            rotation_legs(a, d, tmp)
            return
        if a.store:
            store_legs(a, d, tmp)
            return
        prefix = os.path.join(tmp, "out")
        cmd = [VCF, "-d", "-t", str(a.threads), "-s", os.path.join(d, "sites.fa"), "-r", os.path.join(d, "genome.fa"), "-p", prefix,
               os.path.join(d, "cohort.vcf")]
        if a.rocprof:
            out = a.rocprof_out or os.path.join(tmp, "rocprof")
            cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "vcf", "--"] + cmd
        env = dict(os.environ, NTSM_VCF_PROF="1")
        t0 = time.time()
        p = subprocess.run(cmd, env=env, capture_output=True)
        wall = time.time() - t0
        if p.returncode != 0:
            sys.stderr.write(p.stderr.decode(errors="replace")[-3000:])
            sys.exit(p.returncode)
        err = p.stderr.decode(errors="replace")
        phases = {m.group(1): float(m.group(2)) for m in re.finditer(r"^\[vcf\] ([^:\n]+): ([0-9.]+) s$", err, re.M)}
        dev = re.search(r"^\[vcf\] device: upload ([0-9.]+) s, state kernel ([0-9.]+) s, sum kernel ([0-9.]+) s, download ([0-9.]+) s, "
                        r"kernel bytes (\d+), state launches (\d+)$", err, re.M)
        res = dict(sites=a.sites, samples=a.samples, threads=a.threads, generate_s=round(gen_s, 2), wall_s=round(wall, 3),
                   vcf_bytes=os.path.getsize(os.path.join(d, "cohort.vcf")),
                   matrix_bytes=os.path.getsize(prefix + "_matrix.tsv"), phases_s=phases,
                   warnings=err.count("Inconsistent k-mer counts"), rocprof=a.rocprof)
        if dev:
            up, ks, ss, down, nb, nl = (float(x) for x in dev.groups())
            res.update(upload_s=up, state_kernel_s=ks, sum_kernel_s=ss, download_s=down, state_kernel_bytes=int(nb), state_launches=int(nl),
                       state_kernel_gbps=round(nb / ks / 1e9, 1) if ks > 0 else None)
        print(json.dumps(res))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
