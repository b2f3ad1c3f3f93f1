#!/usr/bin/env python3
"""Recipe of tests/golden/sitegen/ (README.md beside this file).

    python3 tests/golden/sitegen/make_fixtures.py UPSTREAM_SCRIPTS_DIR

UPSTREAM_SCRIPTS_DIR holds upstream's extractSNPsfromVCF.py and filterRepetiveSNP.pl; both are run unmodified and neither
is copied.  Step 1's expected output is the Python script's own stdout / stderr (with standin/pyfaidx.py on PYTHONPATH);
step 3's is the Perl script's files on a SAM-shaped text that tests/sitegen_restatement.cpp writes from its brute-force
hit counts.  Inputs are generated here from fixed seeds."""
import gzip
import json
import os
import random
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
TO_CG = {"A": "CG", "T": "CG", "C": "AT", "G": "AT"}


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


def rand_seq(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def other(rng, base):
    return rng.choice([b for b in "ACGT" if b != base])


def subst(rng, s, offsets):
    s = list(s)
    for o in offsets:
        s[o] = other(rng, s[o])
    return "".join(s)


def build(seed, len1, len2, n_snps, k, w, repeat_family):
    """Two long records carrying SNPs and a third that holds the planted copies.  Returns (records, vcf lines)."""
    rng = random.Random(seed)
    half = w // 2
    a, b = k // 3, 2 * (k // 3)                       # part boundaries of the device step's A | B | C cut
    chroms = {"chr1": list(rand_seq(rng, len1)), "chr2": list(rand_seq(rng, len2))}
    # SNP positions (1-based), most of them far apart, every tenth within k of its predecessor (shared sub-k-mers)
    snps = []
    for name, seq in chroms.items():
        pos = 200
        share = 0
        while pos < len(seq) - 200 and len([s for s in snps if s[0] == name]) < n_snps // 2:
            snps.append((name, pos))
            share += 1
            pos += rng.randrange(5, k - 2) if share % 10 == 0 else rng.randrange(w + k, 3 * w + 60)
    plants = []                                        # pieces of the third record, joined by random spacers

    def spacer():
        return rand_seq(rng, rng.randrange(3, 9))

    boundary = None
    for n, (name, pos) in enumerate(snps):
        seq = chroms[name]
        c = pos - 1
        win = "".join(seq[c - half:c - half + w])
        r = rng.random()
        if r >= 0.55:
            continue
        p = rng.randrange(0, w - k + 1)
        kmer = win[p:p + k]
        kind = n % 16
        if kind < 5:                                   # exact copies of k .. w bases: 1 .. w-k+1 sub-k-mers repeated
            length = rng.randrange(k, w + 1)
            start = rng.randrange(0, w - length + 1)
            plants.append(win[start:start + length])
        elif kind == 5:
            plants.append(subst(rng, kmer, [0]))
        elif kind == 6:
            plants.append(subst(rng, kmer, [k - 1]))
        elif kind == 7:
            plants.append(subst(rng, kmer, [k // 2]))
        elif kind == 8:                                # one substitution on either side of each part boundary
            plants.append(subst(rng, kmer, [rng.choice([a - 1, a, b - 1, b])]))
        elif kind == 9:                                # two substitutions: must not count
            plants.append(subst(rng, kmer, rng.sample(range(k), 2)))
        elif kind == 10:                               # reverse strand, exact or with one substitution
            plants.append(rc(kmer) if n % 32 < 16 else subst(rng, rc(kmer), [rng.randrange(k)]))
        elif kind == 11:                               # interrupted by N: must not count
            plants.append(kmer[:k // 2] + "N" + kmer[k // 2 + 1:])
            plants.append(kmer[:k // 2] + "N" + kmer[k // 2:])
        elif kind == 12:                               # lower-case exact copy: counts
            plants.append(kmer.lower())
        elif kind == 13 and boundary is None:          # straddles the end of chr1 / start of chr2: must not count
            boundary = kmer
        else:
            plants.append(subst(rng, win, [rng.randrange(w)]))
    if boundary:
        chroms["chr1"][-(k // 2):] = list(boundary[:k // 2])
        chroms["chr2"][:k - k // 2] = list(boundary[k // 2:])
    # lower-case stretches over SNP neighbourhoods
    for name, pos in snps[3::17]:
        seq = chroms[name]
        for i in range(pos - 25, pos + 5):
            seq[i] = seq[i].lower()
    # a repeat family: one SNP's first reference sub-k-mer planted 300 times (saturates at 255)
    if repeat_family:
        name, pos = snps[1]
        c = pos - 1
        fam = "".join(chroms[name][c - half:c - half + k]).upper()
        for i in range(300):
            plants.append(fam if i % 3 else rc(fam))
    rng.shuffle(plants)
    chr3 = spacer()
    for piece in plants:
        chr3 += piece + spacer()
    records = [("chr1", "".join(chroms["chr1"])), ("chr2 the second record, with a description", "".join(chroms["chr2"])), ("chr3", chr3)]
    # the VCF
    lines = ["##fileformat=VCFv4.2", "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO"]
    for n, (name, pos) in enumerate(snps):
        ref = chroms[name][pos - 1].upper()
        alt = rng.choice(TO_CG[ref])
        rs = "rs%d" % (1000 + 7 * n)
        if n % 23 == 5:
            rs = "."
        if n % 29 == 11:
            alt = COMP[ref]                            # A <-> T or C <-> G: dropped unless -i
        if n % 37 == 13:
            ref = other(rng, ref)                      # does not match
        if n % 41 == 17:
            ref = ref + chroms[name][pos].upper()      # multi-base REF: does not match
        if chroms[name][pos - 1].islower() and n % 2:
            ref = ref.lower()                          # lower-case REF: does not match
        lines.append("\t".join([name, str(pos), rs, ref, alt, ".", "PASS", "."]))
    # duplicate IDs: a later line replaces the values and keeps the first line's place; a literal ID that collides with
    # the running counter of "."
    name, pos = snps[7]
    ref = chroms[name][pos - 1].upper()
    lines.append("\t".join([snps[2][0], str(snps[2][1]), "rs%d" % (1000 + 7 * 9), chroms[snps[2][0]][snps[2][1] - 1].upper(),
                            TO_CG[chroms[snps[2][0]][snps[2][1] - 1].upper()][0], ".", "PASS", "."]))
    lines.append("\t".join([name, str(pos), "1", ref, TO_CG[ref][1], ".", ".", "."]))
    return records, lines


def write_inputs(stem, records, lines):
    fa, vcf = os.path.join(HERE, "inputs", stem + ".fa"), os.path.join(HERE, "inputs", stem + ".vcf")
    with open(fa, "w") as f:
        for name, seq in records:
            f.write(">%s\n" % name)
            for i in range(0, len(seq), 70):
                f.write(seq[i:i + 70] + "\n")
    with open(vcf, "w") as f:
        f.write("\n".join(lines) + "\n")
    return fa, vcf


def gz_write(path, data):
    with open(path, "wb") as raw:
        with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
            f.write(data)


def record(case, scripts, restatement, tmp):
    fa, vcf = [os.path.join(HERE, "inputs", case[x]) for x in ("genome", "vcf")]
    k, w, x, keep = case["k"], case["w"], case["x"], case["keep_all"]
    out = os.path.join(HERE, "expected", case["name"])
    os.makedirs(out, exist_ok=True)
    env = dict(os.environ, PYTHONPATH=os.path.join(HERE, "standin"))
    p = subprocess.run([sys.executable, os.path.join(scripts, "extractSNPsfromVCF.py"), "-v", vcf, "-f", fa, "-s", str(k), "-k", str(w)]
                       + (["-i"] if keep else []), env=env, capture_output=True, check=True)
    work = os.path.join(tmp, case["name"])
    os.makedirs(work)
    subprocess.run([restatement, "all", fa, vcf, os.path.join(work, "r"), str(k), str(w), str(x), str(int(keep))], check=True,
                   capture_output=True)
    assert open(os.path.join(work, "r_subKmers.fa"), "rb").read() == p.stdout, "the restatement's candidates differ from the script's"
    subprocess.run(["perl", os.path.join(scripts, "filterRepetiveSNP.pl"), os.path.join(work, "r_sam.txt"), os.path.join(work, "u"), str(w), str(k)],
                   check=True, capture_output=True)
    gz_write(os.path.join(out, "subKmers.fa.gz"), p.stdout)
    open(os.path.join(out, "stderr.txt"), "wb").write(p.stderr)
    gz_write(os.path.join(out, "subKmerHits.tsv.gz"), open(os.path.join(work, "r_subKmerHits.tsv"), "rb").read())
    files = []
    for i in range(w - k + 1):
        files.append(open(os.path.join(work, "u_n%d.fa" % i), "rb").read())
        gz_write(os.path.join(out, "n%d.fa.gz" % i), files[-1])
    hits = [int(l.split(b"\t")[1]) for l in open(os.path.join(work, "r_subKmerHits.tsv"), "rb")]
    n_sites = [f.count(b" ref\n") for f in files]
    processed = int(p.stderr.split(b"Processed ")[1].split()[0])
    stats = {"candidates": len(hits), "dropped_by_step2": sum(h > 1 for h in hits), "zero_hits": sum(h == 0 for h in hits),
             "saturated": sum(h == 255 for h in hits), "snps_processed": processed, "sites_per_file": n_sites}
    print(case["name"], json.dumps(stats))
    return stats


def main():
    scripts = sys.argv[1]
    for d in ("inputs", "expected"):
        shutil.rmtree(os.path.join(HERE, d), ignore_errors=True)
        os.makedirs(os.path.join(HERE, d))
    write_inputs("main", *build(20261, 52000, 48000, 320, 19, 31, True))
    write_inputs("small", *build(77, 9000, 8000, 60, 19, 31, False))
    cases = [{"name": "main", "genome": "main.fa", "vcf": "main.vcf", "k": 19, "w": 31, "x": 1, "keep_all": False},
             {"name": "main_x0", "genome": "main.fa", "vcf": "main.vcf", "k": 19, "w": 31, "x": 0, "keep_all": False},
             {"name": "small_keep_all", "genome": "small.fa", "vcf": "small.vcf", "k": 19, "w": 31, "x": 1, "keep_all": True},
             {"name": "small_k15_w25", "genome": "small.fa", "vcf": "small.vcf", "k": 15, "w": 25, "x": 1, "keep_all": False},
             {"name": "small_k25_w31", "genome": "small.fa", "vcf": "small.vcf", "k": 25, "w": 31, "x": 1, "keep_all": False},
             {"name": "small_k31_w31", "genome": "small.fa", "vcf": "small.vcf", "k": 31, "w": 31, "x": 1, "keep_all": False},
             {"name": "small_k11_w30", "genome": "small.fa", "vcf": "small.vcf", "k": 11, "w": 30, "x": 1, "keep_all": False}]
    with tempfile.TemporaryDirectory() as tmp:
        restatement = os.path.join(tmp, "sitegen_restatement")
        subprocess.run(["g++", "-O2", "-std=c++11", "-o", restatement, os.path.join(ROOT, "tests", "sitegen_restatement.cpp")], check=True)
        for case in cases:
            case["stats"] = record(case, scripts, restatement, tmp)
    # a fixture where the filter never fires, or where nothing survives, tests nothing
    st = cases[0]["stats"]
    n = st["sites_per_file"]
    assert n[0] * 3 >= st["snps_processed"], "fewer than a third of the SNPs reach _n0"
    assert sum(1 for i in range(1, len(n)) if n[i] > n[i - 1]) >= 3, "SNPs enter at fewer than three different _n{i}"
    assert st["dropped_by_step2"] * 20 >= st["candidates"], "step 2 drops fewer than a twentieth of the candidates"
    assert st["saturated"] >= 1 and cases[1]["stats"]["zero_hits"] >= 1
    json.dump(cases, open(os.path.join(HERE, "cases.json"), "w"), indent=1)


if __name__ == "__main__":
    main()
