#!/usr/bin/env python3
"""Building a cohort store from reads, two routes on the same inputs: S synthetic samples (SynthShort
with the site geometry of hs_n10_like: 96,287 sites, 1.54 M k-mers) as FASTQ files, then

  (a) the route without `--cohort`: S `build/ntsmCount` processes, each printing its counts text, plus one
      `build/ntsmEval --pack` over the S texts;
  (b) `build/ntsmCount --cohort MANIFEST --store STORE`: one process, one set of contexts, no text.

Every GPU step is a child process of its own under its own time limit, and the script stops at the first one that fails.
Each route runs --runs times (default 3), alternating, so that (a)'s own run-to-run spread is known; for both it reports wall
time, time per sample, bytes written and `cmp` of the two stores; for (b) also the split per sample that
NTSM_PHASE_TIMES prints: counting, the wait for the device, reduce + download (and the reduce kernel alone by HIP events), store
write.

    python tools/cohort_count_bench.py [--samples 16] [--reads 400000] [--threads 16] [--runs 3] [--dir DIR] [--json OUT]"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COUNT = os.path.join(ROOT, "build", "ntsmCount")
EVAL = os.path.join(ROOT, "build", "ntsmEval")
SITES_SEED, N_SITES = 20241218, 96287                      # hs_n10_like


def child(cmd, limit, **kw):
    """one step as a child process under its own time limit; the first failure ends the script"""
    t0 = time.perf_counter()
    try:
        p = subprocess.run(cmd, timeout=limit, stderr=subprocess.PIPE, **kw)
    except subprocess.TimeoutExpired:
        sys.exit("cohort_count_bench: %s ran into its limit of %d s; stopping" % (" ".join(cmd[:3]), limit))
    if p.returncode != 0:
        sys.exit("cohort_count_bench: %s ended with status %d; stopping\n%s" % (" ".join(cmd[:3]), p.returncode, p.stderr[-800:].decode(errors="replace")))
    return time.perf_counter() - t0, p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=16)
    ap.add_argument("--reads", type=int, default=400000, help="reads of 150 bases per sample")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--limit", type=int, default=120, help="time limit of one child process in seconds")
    ap.add_argument("--dir", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import ntsm_amd as nt
    work = a.dir or tempfile.mkdtemp(prefix="cohort_bench_")
    os.makedirs(work, exist_ok=True)
    at = lambda n: os.path.join(work, n)                                   # noqa: E731
    s = nt.SynthShort(sites_seed=SITES_SEED, n_sites=N_SITES, read_seed=31, sites_path=at("sites.fa"))
    names = ["sample%04d.txt" % i for i in range(a.samples)]
    for i in range(a.samples):
        s.write_fastq(at("reads%04d.fq" % i), i * a.reads, a.reads, threads=min(16, a.threads))
    with open(at("manifest.tsv"), "w") as f:
        f.write("".join("%s\treads%04d.fq\n" % (n, i) for i, n in enumerate(names)))
    fastq_bytes = sum(os.path.getsize(at("reads%04d.fq" % i)) for i in range(a.samples))
    flags = ["-s", "sites.fa", "-t", str(a.threads)]
    runs_a, runs_b = [], []
    same = True
    for r in range(a.runs):
        # (a) S processes + --pack
        for p in ["packed"] + names:
            if os.path.exists(at(p)):
                os.unlink(at(p))
        t0 = time.perf_counter()
        per_process = []
        for i, n in enumerate(names):
            with open(at(n), "wb") as out:
                dt, _ = child([COUNT] + flags + ["reads%04d.fq" % i], a.limit, cwd=work, stdout=out)
            per_process.append(dt)
        t_count = time.perf_counter() - t0
        t_pack, _ = child([EVAL, "--pack", "packed"] + names, a.limit + 2 * a.samples, cwd=work, stdout=subprocess.DEVNULL)
        wall_a = time.perf_counter() - t0
        text_bytes = sum(os.path.getsize(at(n)) for n in names)
        runs_a.append(dict(wall_s=wall_a, count_s=t_count, pack_s=t_pack, per_process_s=per_process, bytes_written=text_bytes + os.path.getsize(at("packed"))))
        # (b) one process
        if os.path.exists(at("cohort")):
            os.unlink(at("cohort"))
        wall_b, p = child([COUNT] + flags + ["--cohort", "manifest.tsv", "--store", "cohort"], a.limit + 10 * a.samples, cwd=work,
                          stdout=subprocess.PIPE, env=dict(os.environ, NTSM_PHASE_TIMES="1"))
        err = p.stderr.decode(errors="replace")
        split = [dict(zip(("reset_s", "count_s", "wait_s", "reduce_download_s", "kernel_ms", "text_s", "store_s"), map(float, m.groups())))
                 for m in re.finditer(r"\[phase\] cohort sample \S+: reset (\S+) s, count (\S+) s, wait (\S+) s, reduce\+download (\S+) s \(kernel (\S+) ms\), counts text (\S+) s, store (\S+) s", err)]
        start = re.search(r"\[phase\] cohort: start-up .* (\S+) s", err)
        assert len(split) == a.samples and p.stdout.count(b"\n") == a.samples, err[-800:]
        runs_b.append(dict(wall_s=wall_b, startup_s=float(start.group(1)) if start else None, per_sample=split, bytes_written=os.path.getsize(at("cohort"))))
        same = same and subprocess.run(["cmp", at("cohort"), at("packed")]).returncode == 0

    def med(xs):
        return statistics.median(xs)

    wa, wb = [r["wall_s"] for r in runs_a], [r["wall_s"] for r in runs_b]
    keys = ("reset_s", "count_s", "wait_s", "reduce_download_s", "kernel_ms", "text_s", "store_s")
    later = [x for r in runs_b for x in r["per_sample"][1:]] or [x for r in runs_b for x in r["per_sample"]]
    result = dict(
        samples=a.samples, reads_per_sample=a.reads, bases_per_sample=a.reads * 150, threads=a.threads, runs=a.runs, n_sites=N_SITES, n_kmers=s.n_kmers,
        fastq_bytes=fastq_bytes, stores_equal=same,
        route_a=dict(wall_s=wa, wall_median_s=med(wa), spread_s=max(wa) - min(wa), per_sample_s=med(wa) / a.samples,
                     count_median_s=med([r["count_s"] for r in runs_a]), pack_median_s=med([r["pack_s"] for r in runs_a]),
                     process_median_s=med([x for r in runs_a for x in r["per_process_s"]]), bytes_written=runs_a[-1]["bytes_written"]),
        route_b=dict(wall_s=wb, wall_median_s=med(wb), spread_s=max(wb) - min(wb), per_sample_s=med(wb) / a.samples,
                     startup_median_s=med([r["startup_s"] for r in runs_b if r["startup_s"] is not None] or [0]),
                     first_sample_median=dict((k, med([r["per_sample"][0][k] for r in runs_b])) for k in keys),
                     later_samples_median=dict((k, med([x[k] for x in later])) for k in keys), bytes_written=runs_b[-1]["bytes_written"]),
        raw=dict(route_a=runs_a, route_b=runs_b))
    result["b_over_a"] = result["route_b"]["wall_median_s"] / result["route_a"]["wall_median_s"]
    result["b_not_slower_than_a_by_more_than_its_spread"] = result["route_b"]["wall_median_s"] <= result["route_a"]["wall_median_s"] + result["route_a"]["spread_s"]
    line = json.dumps(result)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(line + "\n")
    brief = dict((k, v) for k, v in result.items() if k != "raw")
    print(json.dumps(brief, indent=1))
    if not same:
        sys.exit("cohort_count_bench: the two stores differ")


if __name__ == "__main__":
    main()
