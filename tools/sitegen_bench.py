#!/usr/bin/env python3
"""ntsmSiteGen at full size: a seeded genome with repeat families and a VCF of SNPs generated on this machine, one
`build/ntsmSiteGen -V` run, two yardsticks taken in the same session, and two checks of the result.

  python3 tools/sitegen_bench.py [--bases 1073741824] [--snps 1000000] [--seed 1] [--dir DIR] [--out OUT.json]
                                 [--sample 10000] [--no-yardsticks] [--gaps]

Genome: 8 records of random bases; 24 repeat families of 300 bases, planted 200 .. 50,000 times each with 3 % of the bases
substituted per copy (about 5 % of the genome); the first reference 19-mer of one SNP's window planted 1,000 more times
(saturation: its count must come out as 255); one N per 200 kb.  VCF: SNPs at sorted random positions, REF from the
genome, ALT on the other side of A/T | C/G except for 2 % (dropped by step 1) and 1 % with a REF that does not match.

Prints one JSON line (and writes it to --out): wall time by stage from the program's own -V lines (genome read, step 1,
table build, table upload, staging, genome upload, scan kernel from HIP events, the candidate files, step 3 with its files), windows/s and probes/s
of the scan kernel, the spread of the kernel's full launches, the yardsticks (build/gather_bench's random-gather rate at its largest
table; the exact-match count kernel's bases/s on the same genome fed as reads against the sites file this run wrote),
and the checks (--sample candidates against tests/sitegen_restatement.cpp's "halves" brute force on the CPU; the planted
family's count).  --gaps runs the program a second time with -g on the same genome in the same session and adds, under
"gaps": the same -V figures of that run, its scan kernel over the substitution-only one, the share of candidates whose
keep / drop verdict (count <= 1) -g changes, and the size and sites of NAME_n10.fa both ways.  Needs a GPU; there is no
fallback."""
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
EXE = os.path.join(ROOT, "build", "ntsmSiteGen")
K, W = 19, 31


def generate(d, n_bases, n_snps, seed):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    n_rec = 8
    per = n_bases // n_rec
    per_snps = n_snps // n_rec
    families = [letters[rng.integers(0, 4, size=300)] for _ in range(24)]
    copies = np.maximum(np.geomspace(200, 50000, num=24) * n_bases / (1 << 30), 2 * n_rec).astype(np.int64)
    planted_name, sat_pos = None, -1
    with open(os.path.join(d, "genome.fa"), "wb") as fa, open(os.path.join(d, "snps.vcf"), "wb") as vcf:
        vcf.write(b"##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
        for r in range(n_rec):
            seq = letters[rng.integers(0, 4, size=per, dtype=np.uint8)]
            for fam, n_copies in zip(families, copies):
                m = max(1, int(n_copies) // n_rec)
                at = rng.integers(0, per - 300, size=m)
                idx = at[:, None] + np.arange(300)[None, :]
                body = np.broadcast_to(fam, (m, 300)).copy()
                mut = rng.random((m, 300)) < 0.03
                body[mut] = letters[rng.integers(0, 4, size=int(mut.sum()))]
                seq[idx.ravel()] = body.ravel()
            pos = np.sort(rng.choice(np.arange(100, per - 100, 25), size=per_snps, replace=False)) + rng.integers(0, 12, size=per_snps)
            if r == 0:                                     # the saturation family: SNP 10's first reference 19-mer, 1,000 copies
                p0 = int(pos[10]) - 1 - W // 2
                fam19 = seq[p0:p0 + K].copy()
                for at in rng.integers(per // 2, per - 100, size=1000):
                    if np.min(np.abs(pos - at)) > 100:
                        seq[at:at + K] = fam19
                sat_pos = int(pos[10])
                planted_name = b"c0p%d|0|" % sat_pos
            n_at = np.sort(rng.integers(0, per, size=max(1, per // 200000)))
            seq[n_at] = ord("N")
            # a window with N makes step 1 refuse the whole input (the script raises there): no SNP within w of an N
            nearest = np.searchsorted(n_at, pos - 1 - W)
            ok = (nearest == len(n_at)) | (n_at[np.minimum(nearest, len(n_at) - 1)] > pos - 1 + W)
            pos = pos[ok]
            ref = seq[pos - 1].copy()
            other = {65: b"CG", 84: b"CG", 67: b"AT", 71: b"AT"}
            same = {65: 84, 84: 65, 67: 71, 71: 67}
            pick = rng.integers(0, 2, size=len(pos))
            kind = rng.random(len(pos))
            lines = []
            for i in range(len(pos)):
                b = int(ref[i])
                alt = other[b][pick[i]]
                keep = r == 0 and pos[i] == sat_pos
                if 0.02 <= kind[i] < 0.04 and not keep:
                    alt = same[b]
                if kind[i] < 0.01 and not keep:
                    b = same[b]
                lines.append(b"chr%d\t%d\tc%dp%d\t%c\t%c\t.\tPASS\t.\n" % (r, pos[i], r, pos[i], b, alt))
            vcf.write(b"".join(lines))
            fa.write(b">chr%d\n" % r + seq.tobytes() + b"\n")
    return planted_name


def parse_v(err):
    out = {}
    m = re.search(r"Device: table build ([\d.]+) ms, table upload ([\d.]+) ms \(([\d.]+) MB\), stage ([\d.]+) ms, upload ([\d.]+) ms, "
                  r"scan kernel ([\d.]+) ms in (\d+) launches \((\d+) full: ([\d.]+) \.\. ([\d.]+) ms each\); (\d+) windows"
                  r"(?: \((\d+) of k \+ 1 bases, (\d+) of k - 1\))?, (\d+) bitmap tests, (\d+) probes", err)
    keys = ["table_build_ms", "table_upload_ms", "table_mb", "stage_ms", "genome_upload_ms", "scan_kernel_ms", "launches", "full_launches",
            "full_launch_ms_min", "full_launch_ms_max", "windows", "windows_long", "windows_short", "bitmap_tests", "probes"]
    out.update({k: float(v) for k, v in zip(keys, m.groups()) if v is not None})
    m = re.search(r"Time: genome ([\d.]+) ms, step 1 ([\d.]+) ms, step 2 ([\d.]+) ms, candidate files ([\d.]+) ms, step 3 ([\d.]+) ms; (\d+) SNPs, (\d+) candidates", err)
    out.update({k: float(v) for k, v in zip(["genome_read_ms", "step1_ms", "step2_ms", "candidate_files_ms", "step3_ms", "snps", "candidates"], m.groups())})
    return out


def yardsticks(d, n_bases):
    import ntsm_amd
    res = {}
    p = subprocess.run([os.path.join(ROOT, "build", "gather_bench")], capture_output=True, timeout=300, check=True)
    rows = [l.split() for l in p.stdout.decode().splitlines() if l.startswith("gather4_all")]
    res["gather4_all_largest_table_kib"] = int(rows[-1][2])
    res["gather4_all_largest_table_g_per_s"] = float(rows[-1][4])
    # the exact-match count kernel on the same genome, fed as reads of 100 kb, against this run's sites file
    sites = ntsm_amd.Sites(os.path.join(d, "run_n%d.fa" % (W - K)))
    ctx = ntsm_amd.Context(sites.keys, k=K, device=0)
    ctx.set_timing(1)
    piece = 256 << 20
    total_ms, total_bases = 0.0, 0
    with open(os.path.join(d, "genome.fa"), "rb") as f:
        for rep in range(2):                                # the first piece twice: the first pass is the warm-up
            f.seek(0)
            done = 0
            while done < (piece if rep == 0 else n_bases):
                buf = np.frombuffer(f.read(piece), dtype=np.uint8).copy()
                if not len(buf):
                    break
                # include/ntsm_hip.h's layout: every read is followed by one separator byte, read_end = its offset
                ends = np.unique(np.append(np.arange(99999, len(buf), 100000, dtype=np.uint64), np.uint64(len(buf) - 1)))
                buf[ends.astype(np.int64)] = ord("N")
                ctx.reset()
                n0, ms0 = ctx.get_timing()
                ctx.submit(buf, ends)
                ctx.sync()
                n1, ms1 = ctx.get_timing()
                if rep:
                    total_ms += ms1 - ms0
                    total_bases += len(buf)
                done += len(buf)
    ctx.close()
    res["count_kernel_bases"] = total_bases
    res["count_kernel_ms"] = total_ms
    res["count_kernel_gbases_per_s"] = total_bases / total_ms / 1e6 if total_ms else None
    res["count_kernel_keys"] = int(len(sites.keys))
    return res


def checks(d, res, planted, sample):
    """the result in figures, and the two checks of it"""
    # the result: hit histogram, sites per file
    tsv = os.path.join(d, "run_subKmerHits.tsv")
    hist = subprocess.run(["awk", "-F\t", "{h[$2]++} END {for (v in h) print v, h[v]}", tsv], capture_output=True, check=True).stdout.decode()
    hist = {int(l.split()[0]): int(l.split()[1]) for l in hist.splitlines()}
    res["hits_histogram"] = {"0": hist.get(0, 0), "1": hist.get(1, 0), "2": hist.get(2, 0), "3..254": sum(v for h, v in hist.items() if 2 < h < 255),
                             "255": hist.get(255, 0)}
    res["sites_per_file"] = [int(subprocess.run(["grep", "-c", " ref$", os.path.join(d, "run_n%d.fa" % i)], capture_output=True).stdout or 0)
                             for i in range(W - K + 1)]
    # check 1: the planted family saturates
    fam = subprocess.run(["grep", "-m", "2", "-F", planted.decode(), tsv], capture_output=True).stdout.decode().splitlines()
    res["planted_family_rows"] = fam
    res["planted_family_ok"] = any(l.endswith("\t255") for l in fam)
    # check 2: a sample of candidates against the CPU brute force ("halves", streamed over the whole genome)
    n_cand = int(res["candidates"])
    stride = max(1, n_cand // sample)
    rows = subprocess.run(["awk", "-v", "s=%d" % stride, "NR % s == 1 || s == 1", tsv], capture_output=True, check=True).stdout.decode().splitlines()
    seqs = subprocess.run(["awk", "-v", "s=%d" % stride, "NR % 2 == 0 && ((NR / 2) % s == 1 || s == 1)", os.path.join(d, "run_subKmers.fa")],
                          capture_output=True, check=True).stdout.decode().splitlines()
    assert len(rows) == len(seqs), (len(rows), len(seqs))
    open(os.path.join(d, "sample.txt"), "w").write("".join(s + "\n" for s in seqs))
    rs = os.path.join(d, "sitegen_restatement")
    subprocess.run(["g++", "-O2", "-std=c++11", "-o", rs, os.path.join(ROOT, "tests", "sitegen_restatement.cpp")], check=True)
    t0 = time.time()
    want = subprocess.run([rs, "hits", os.path.join(d, "genome.fa"), os.path.join(d, "sample.txt"), str(K), "1", "halves"], capture_output=True,
                          check=True, timeout=3000).stdout.decode().split()
    res["sample_brute_force_s"] = round(time.time() - t0, 1)
    got = [r.split("\t")[1] for r in rows]
    res["sample_checked"] = len(got)
    res["sample_mismatches"] = sum(1 for g, w_ in zip(got, want) if g != w_)
    res["sample_above_one"] = sum(1 for w_ in want if int(w_) > 1)


def gaps_run(d, res):
    """the same genome and VCF with -g: the figures of that run beside the first one's"""
    t0 = time.time()
    p = subprocess.run([EXE, "-r", os.path.join(d, "genome.fa"), "-v", os.path.join(d, "snps.vcf"), "-p", os.path.join(d, "gap"), "-g", "-V"],
                       capture_output=True, timeout=3000)
    if p.returncode:
        raise SystemExit("ntsmSiteGen -g failed (%d): %s" % (p.returncode, p.stderr.decode()[-500:]))
    g = parse_v(p.stderr.decode())
    g["program_wall_s"] = round(time.time() - t0, 1)
    g["e"] = 5
    g["scan_kernel_over_substitutions_only"] = g["scan_kernel_ms"] / res["scan_kernel_ms"]
    g["windows_per_s"] = g["windows"] / g["scan_kernel_ms"] * 1e3
    g["table_reads_per_s"] = (g["bitmap_tests"] + g["probes"]) / g["scan_kernel_ms"] * 1e3
    both = subprocess.run("paste %s %s | awk -F'\t' '{a = $2 <= 1; b = $4 <= 1; if (a != b) n++; if (a && !b) lost++; if ($4 < $2) less++} "
                          "END {print NR, n + 0, lost + 0, less + 0}'" % (os.path.join(d, "run_subKmerHits.tsv"), os.path.join(d, "gap_subKmerHits.tsv")),
                          shell=True, capture_output=True, check=True).stdout.decode().split()
    g["candidates"], g["verdict_changed"], g["kept_to_dropped"], g["count_below_substitutions_only"] = (int(x) for x in both)
    g["verdict_changed_share"] = g["verdict_changed"] / max(g["candidates"], 1)
    for tag in ("run", "gap"):
        path = os.path.join(d, "%s_n10.fa" % tag)
        g["n10_bytes_" + ("with_gaps" if tag == "gap" else "without")] = os.path.getsize(path)
        g["n10_sites_" + ("with_gaps" if tag == "gap" else "without")] = int(subprocess.run(["grep", "-c", " ref$", path], capture_output=True).stdout or 0)
    for f in os.listdir(d):
        if f.startswith("gap_"):
            os.remove(os.path.join(d, f))
    res["gaps"] = g


def say(what):
    print("[sitegen_bench %s] %s" % (time.strftime("%H:%M:%S"), what), file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=1 << 30)
    ap.add_argument("--snps", type=int, default=1000000)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--dir")
    ap.add_argument("--out")
    ap.add_argument("--sample", type=int, default=10000)
    ap.add_argument("--no-yardsticks", action="store_true")
    ap.add_argument("--gaps", action="store_true")
    a = ap.parse_args()
    d = a.dir or tempfile.mkdtemp(prefix="sitegen_bench_")
    os.makedirs(d, exist_ok=True)
    res = {"bases": a.bases, "snps_asked": a.snps, "seed": a.seed, "k": K, "w": W, "x": 1}
    try:
        t0 = time.time()
        planted = generate(d, a.bases, a.snps, a.seed)
        res["generate_s"] = round(time.time() - t0, 1)
        say("generated in %.1f s; running ntsmSiteGen" % res["generate_s"])
        t0 = time.time()
        p = subprocess.run([EXE, "-r", os.path.join(d, "genome.fa"), "-v", os.path.join(d, "snps.vcf"), "-p", os.path.join(d, "run"), "-V"],
                           capture_output=True, timeout=3000)
        res["program_wall_s"] = round(time.time() - t0, 1)
        err = p.stderr.decode()
        if p.returncode:
            raise SystemExit("ntsmSiteGen failed (%d): %s" % (p.returncode, err[-500:]))
        res.update(parse_v(err))
        res["script_lines"] = [l for l in err.splitlines() if l.startswith(("Processed", "Filtered"))]
        res["does_not_match"] = err.count("Wildtype allele does not match")
        res["windows_per_s"] = res["windows"] / res["scan_kernel_ms"] * 1e3
        res["probes_per_s"] = res["probes"] / res["scan_kernel_ms"] * 1e3
        res["table_reads_per_s"] = (res["bitmap_tests"] + res["probes"]) / res["scan_kernel_ms"] * 1e3
        say("program done in %.1f s; checking" % res["program_wall_s"])
        checks(d, res, planted, a.sample)
        say("checked: %d sampled, %d mismatches; yardsticks" % (res["sample_checked"], res["sample_mismatches"]))
        if a.gaps:
            gaps_run(d, res)
            say("-g run done in %.1f s: scan kernel %.1f ms against %.1f ms" % (res["gaps"]["program_wall_s"], res["gaps"]["scan_kernel_ms"], res["scan_kernel_ms"]))
        for f in os.listdir(d):                               # the large outputs are not needed by the yardsticks
            if f.startswith("run_") and f != "run_n%d.fa" % (W - K):
                os.remove(os.path.join(d, f))
        say("so far: " + json.dumps(res))
        if not a.no_yardsticks:
            res.update(yardsticks(d, a.bases))
            res["scan_table_reads_over_gather_rate"] = res["table_reads_per_s"] / (res["gather4_all_largest_table_g_per_s"] * 1e9)
            res["count_kernel_over_scan"] = res["count_kernel_gbases_per_s"] * 1e9 / res["windows_per_s"] if res["count_kernel_gbases_per_s"] else None
    finally:
        if not a.dir:
            shutil.rmtree(d, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(line + "\n")
    return 0 if res["planted_family_ok"] and res["sample_mismatches"] == 0 else 1


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.exit(main())
