"""ntsmVCF: build/ntsmVCF (ntsm_amd/csrc/host/ntsm_vcf_main.cpp) and its device step (include/ntsm_vcf_hip.h,
ntsm_amd/csrc/ntsm_vcf.hip, ntsm_amd/vcf.py).

The contract is one thread of the reference with the sample x k-mer matrix sized for the header's samples.  The
fixtures under tests/golden/vcf/ were recorded from the reference classes with only that change (README there);
tests/vcf_restatement.cpp is an independent restatement written from the reference text.  CPU: the restatement
reproduces every fixture, the CLI's refusals and flag errors, and the whole program -- ntsm_vcf_main.cpp built against
tests/vcf_step_standin.cpp, a plain C++ ntsm_vcf_run, under ASan + UBSan -- against the fixtures and the restatement.  GPU: the CLI against the fixtures and against the
restatement on seeded cohorts, -t 1 against -t 16, gzip / BGZF input, the device step against a numpy model (also on
cohorts past 1,024 and 4,096 samples, where the state kernel widens its workgroup and then loops a lane over chunks),
and the chain into ntsmEval -p / -n."""
import gzip
import json
import os
import re
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_binding import ROOT  # noqa: E402

VCF = os.path.join(ROOT, "build", "ntsmVCF")
EVAL = os.path.join(ROOT, "build", "ntsmEval")
GOLD = os.path.join(ROOT, "tests", "golden", "vcf")
CASES = json.load(open(os.path.join(GOLD, "cases.json")))
ALT = {"A": "G", "C": "T", "G": "A", "T": "C"}


@pytest.fixture(scope="module")
def restatement(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vrs") / "vcf_restatement")
    subprocess.run(["g++", "-O2", "-std=c++11", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "vcf_restatement.cpp")],
                   check=True)
    return exe


def strip_time(err):
    return b"".join(l for l in err.splitlines(True) if not l.startswith(b"Time: "))


def run(exe, args, cwd, prefix):
    """(exit status, matrix bytes or None, centre bytes or None, stderr without the Time line)"""
    p = subprocess.run([exe] + args, cwd=cwd, capture_output=True, timeout=600)
    out = []
    for suffix in ("_matrix.tsv", "_center.txt"):
        f = prefix + suffix
        out.append(open(f, "rb").read() if os.path.exists(f) else None)
    return p.returncode, out[0], out[1], strip_time(p.stderr)


# ---------------------------------------------------------------------------------------------------- inputs
def write_case(tmp, genome, sites, samples, lines, tail="\n"):
    """genome: [(name, seq)]; sites: [(id, ref, var)]; lines: lists of VCF fields or raw strings"""
    g, s, v = str(tmp / "genome.fa"), str(tmp / "sites.fa"), str(tmp / "in.vcf")
    with open(g, "w") as f:
        for name, seq in genome:
            f.write(">%s\n%s\n" % (name, seq))
    with open(s, "w") as f:
        for rs, ref, var in sites:
            f.write(">%s\n%s\n>%s_v\n%s\n" % (rs, ref, rs, var))
    body = "##fileformat=VCFv4.2\n" + "\t".join(["#CHROM", "POS", "ID", "REF", "ALT", "QUAL", "FILTER", "INFO", "FORMAT"] + samples) + "\n"
    body += "\n".join(l if isinstance(l, str) else "\t".join(l) for l in lines) + tail
    with open(v, "w", newline="") as f:
        f.write(body)
    return g, s, v


def site_of(seq, pos, k=19, rs="rs"):
    c = pos - 1
    ref = seq[max(0, c - k + 1):c + k].upper()
    o = c - max(0, c - k + 1)
    return (rs, ref, ref[:o] + ALT[ref[o]] + ref[o + 1:])


def cohort(tmp, rng, n_samples, n_snps, dense=True, n_chrom=3):
    """A seeded cohort: random chromosomes, SNPs of which many lie within k of each other (shared k-mers), some lines
    duplicated with other genotypes (conflicting inserts), some sites absent from the VCF, some unparsed genotypes."""
    chrom_len = max(2000, n_snps * 40 // n_chrom)
    genome = [("c%d" % i, "".join(rng.choice(list("ACGT"), size=chrom_len))) for i in range(n_chrom)]
    gd = dict(genome)
    snps = set()
    if not dense:                                                               # at least 2k apart: no shared k-mers
        snps = {(i % n_chrom, 60 + 45 * (i // n_chrom) + int(rng.integers(0, 5))) for i in range(n_snps)}
        chrom_len = max(chrom_len, 60 + 45 * (n_snps // n_chrom + 1) + 60)
        genome = [("c%d" % i, "".join(rng.choice(list("ACGT"), size=chrom_len))) for i in range(n_chrom)]
        gd = dict(genome)
    while len(snps) < n_snps:
        c = int(rng.integers(0, n_chrom))
        p = int(rng.integers(40, chrom_len - 40))
        snps.add((c, p))
        if dense and rng.random() < 0.4 and len(snps) < n_snps:
            snps.add((c, min(chrom_len - 40, p + int(rng.integers(1, 18)))))
    snps = sorted(snps)
    sites = [site_of(gd["c%d" % c], p, rs="rs%d_%d" % (c, p)) for c, p in snps]
    samples = ["S%d" % i for i in range(n_samples)]
    pool = np.array(["0|0", "0|1", "1|0", "1|1", "0|0", "1|1", "./.", "0/1"])
    lines = []
    for c, p in snps:
        if rng.random() < 0.05:
            continue                                                            # site absent from the VCF
        b = gd["c%d" % c][p - 1]
        for _ in range(2 if rng.random() < 0.15 else 1):                        # a duplicated line: conflicts
            g = pool[rng.integers(0, 6 if rng.random() < 0.8 else 8, size=n_samples)]
            lines.append("\t".join(["c%d" % c, str(p), "rs%d_%d" % (c, p), b, ALT[b], ".", "PASS", ".", "GT"]) + "\t" + "\t".join(g))
    return write_case(tmp, genome, sites, samples, lines)


def bgzf(data):
    """BGZF (SAM spec 4.1): gzip members of at most 64 KiB with the BC extra field, then the empty EOF member"""
    out = bytearray()
    for i in range(0, len(data), 60000):
        c = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = c.compress(data[i:i + 60000]) + c.flush()
        out += struct.pack("<BBBBIBBHBBHH", 31, 139, 8, 4, 0, 0, 255, 6, 66, 67, 2, len(body) + 25)
        out += body + struct.pack("<II", zlib.crc32(data[i:i + 60000]) & 0xFFFFFFFF, len(data[i:i + 60000]))
    out += bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
    return bytes(out)


# ---------------------------------------------------------------------------------------------------- CPU
def test_restatement_reproduces_every_fixture(restatement, tmp_path):
    """tests/vcf_restatement.cpp gives the recorded matrix, centre file and stderr of every fixture."""
    for case in CASES:
        d = os.path.join(GOLD, case["name"])
        prefix = str(tmp_path / case["name"])
        p = subprocess.run([restatement, "-s", "sites.fa", "-r", "genome.fa"] + case["args"] + ["-p", prefix, "in.vcf"], cwd=d,
                           capture_output=True, check=True)
        assert open(prefix + "_matrix.tsv", "rb").read() == open(os.path.join(d, "expected_matrix.tsv"), "rb").read(), case
        assert open(prefix + "_center.txt", "rb").read() == open(os.path.join(d, "expected_center.txt"), "rb").read(), case
        assert p.stderr == open(os.path.join(d, "expected_stderr.txt"), "rb").read(), case


def refusal_inputs(tmp, rng):
    chrom = "".join(rng.choice(list("ACGT"), size=300))
    genome = [("chr1", chrom)]
    sites = [site_of(chrom, 100, rs="rsA"), site_of(chrom, 200, rs="rsB")]
    gt = ["0|1", "1|1"]

    def line(pos="100", chrom_name="chr1"):
        return [chrom_name, pos, "rsA", chrom[int(pos) - 1] if pos.isdigit() and int(pos) <= 300 else "A", "T", ".", "PASS", ".", "GT"] + gt
    return genome, sites, line


REFUSALS = [
    # (name, what to change, message fragment)
    ("unknown_chromosome", "chrom", "unknown chromosome"),
    ("pos_not_past_half_window", "pos15", "not greater than half the window"),
    ("window_past_end", "pos_end", "starts past the end"),
    ("field_count", "fields", "genotype fields, the header has"),
    ("empty_line", "empty", "empty line"),
    ("bad_pos", "pos_text", "is not an int"),
    ("k32", "k32", "-k 32 is not supported"),
    ("odd_sites", "odd", "odd number of records"),
    ("shared_without_d", "shared", "-p needs -d"),
    ("two_vcfs", "two", "takes one VCF file"),
    ("missing_vcf", "missing", "does not exist"),
]


@pytest.mark.parametrize("name,what,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(built, tmp_path, name, what, msg):
    """Inputs where the reference throws, asserts or has undefined behaviour: 'Error: ...', exit status 1, nothing
    written.  All are found before any device work."""
    rng = np.random.default_rng(3)
    genome, sites, line = refusal_inputs(tmp_path, rng)
    lines = [line("100"), line("200")]
    args = []
    if what == "chrom":
        lines.append(line("150", "chrX"))
    elif what == "pos15":
        lines.append(line("15"))
    elif what == "pos_end":
        lines.append(line("400"))
    elif what == "fields":
        lines.append(line("120")[:-1])
    elif what == "empty":
        lines.append("")
    elif what == "pos_text":
        lines.append(["chr1", "abc"] + line("120")[2:])
    elif what == "k32":
        args = ["-k", "32"]
    elif what == "shared":
        sites = sites + [site_of(genome[0][1], 105, rs="rsC")]          # shares k-mers with rsA
    g, s, v = write_case(tmp_path, genome, sites, ["S0", "S1"], lines)
    if what == "odd":
        with open(s, "a") as f:
            f.write(">rsZ\nACGTACGTACGTACGTACGTACGT\n")
    vcfs = [v]
    if what == "two":
        vcfs = [v, v]
    elif what == "missing":
        vcfs = [str(tmp_path / "nope.vcf")]
    prefix = str(tmp_path / "out")
    rc, mat, cen, err = run(VCF, ["-s", s, "-r", g, "-p", prefix] + args + vcfs, str(tmp_path), prefix)
    assert rc == 1, (name, err)
    assert err.splitlines()[-1].startswith(b"Error: ") and msg.encode() in err, (name, err)
    assert mat is None and cen is None, name


def test_flag_errors(built, tmp_path):
    """src/ntSeqMatchVCF.cpp:90-194: an unparsable value prints 'Error - Invalid parameter X: V' and exits 0; a missing
    VCF, a missing reference and k > 32 print the reference's messages, then "Try '--help'", exit 1."""
    g, s, v = write_case(tmp_path, [("chr1", "ACGT" * 50)], [], ["S0"], [])
    for flag in ("k", "w", "m", "t", "G"):
        p = subprocess.run([VCF, "-" + flag, "x1", "-s", s, "-r", g, v], capture_output=True)
        assert p.returncode == 0 and p.stderr == ("Error - Invalid parameter %s: x1\n" % flag).encode(), flag
    p = subprocess.run([VCF, "-s", s, "-r", g], capture_output=True)
    assert p.returncode == 1 and p.stderr == b"Error: Need Input File\nTry '--help' for more information.\n"
    p = subprocess.run([VCF, "-s", s, "-r", str(tmp_path / "none.fa"), v], capture_output=True)
    assert p.returncode == 1 and p.stderr == b"Error: Unable to load reference file\nTry '--help' for more information.\n"
    p = subprocess.run([VCF, "-k", "33", "-s", s, "-r", g, v], capture_output=True)
    assert p.returncode == 1 and p.stderr == b"k cannot be greater than 32\nTry '--help' for more information.\n"
    p = subprocess.run([VCF, "-s", str(tmp_path / "none.fa"), "-r", g, v], capture_output=True)
    assert p.returncode == 1 and p.stderr == ("file %s cannot be opened\n" % (tmp_path / "none.fa")).encode()
    p = subprocess.run([VCF, "-h"], capture_output=True)
    assert p.returncode == 0 and p.stderr.startswith(b"Usage: ntsmVCF -s [FASTA] -r [FASTA] [VCF]\n")


# ------------------------------------------------------------------------------ the whole program on the CPU
@pytest.fixture(scope="module")
def cpu_program(tmp_path_factory):
    """ntsm_vcf_main.cpp + the Makefile's $(VCFSRC) + tests/vcf_step_standin.cpp (ntsm_vcf_run in plain C++, written from
    include/ntsm_vcf_hip.h) as a program of its own under ASan + UBSan: it is run directly, nothing is preloaded."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    vcfsrc = re.search(r"^VCFSRC := ((?:.*\\\n)*.*)$", mk, re.M).group(1).replace("\\\n", " ").split()
    host = os.path.join(ROOT, "ntsm_amd", "csrc", "host")
    src = [os.path.join(host, "ntsm_vcf_main.cpp")] + [f.replace("$(HOST)", host) for f in vcfsrc]
    assert len(src) > 5 and all(os.path.exists(f) for f in src), src
    exe = str(tmp_path_factory.mktemp("vcpu") / "ntsmVCF_cpu")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off",
                    "-o", exe] + src + [os.path.join(ROOT, "tests", "vcf_step_standin.cpp"), "-lz", "-pthread"], check=True)
    return exe


def run_cpu(exe, args, cwd, prefix):
    """run(), and no sanitizer report on stderr"""
    out = run(exe, args, cwd, prefix)
    assert b"Sanitizer" not in out[3] and b"runtime error" not in out[3], out[3][-3000:].decode(errors="replace")
    return out


def test_cpu_program_gives_the_fixtures(cpu_program, tmp_path):
    for case in CASES:
        d = os.path.join(GOLD, case["name"])
        prefix = str(tmp_path / case["name"])
        rc, mat, cen, err = run_cpu(cpu_program, ["-s", "sites.fa", "-r", "genome.fa"] + case["args"] + ["-p", prefix, "in.vcf"], d, prefix)
        assert rc == 0, (case, err)
        assert mat == open(os.path.join(d, "expected_matrix.tsv"), "rb").read(), case
        assert cen == open(os.path.join(d, "expected_center.txt"), "rb").read(), case
        assert err == open(os.path.join(d, "expected_stderr.txt"), "rb").read(), case


@pytest.mark.parametrize("n_samples,n_snps,seed", [(7, 60, 46), (33, 120, 32)], ids=["7x60", "33x120"])
def test_cpu_program_matches_restatement_for_every_t(cpu_program, restatement, tmp_path, n_samples, n_snps, seed):
    """Dense seeded cohorts (33 samples cross the 16- and 32-byte genotype stride) under -t 1, -t 5 and -t 64 -- more
    threads than the first cohort has body lines: matrix, centre file and stderr byte for byte against the restatement."""
    g, s, v = cohort(tmp_path, np.random.default_rng(seed), n_samples, n_snps)
    b = str(tmp_path / "rs")
    p = subprocess.run([restatement, "-s", s, "-r", g, "-d", "-p", b, v], capture_output=True, check=True)
    want = (0, open(b + "_matrix.tsv", "rb").read(), open(b + "_center.txt", "rb").read(), p.stderr)
    assert b"Inconsistent k-mer counts" in p.stderr and want[1].count(b"\n") == n_snps + 1
    if n_snps == 60:
        assert open(v, "rb").read().count(b"\n") - 2 < 64                         # this seed: 58 body lines
    for t in ("1", "5", "64"):
        a = str(tmp_path / ("t" + t))
        assert run_cpu(cpu_program, ["-s", s, "-r", g, "-d", "-t", t, "-p", a, v], str(tmp_path), a) == want, t


def test_cpu_program_threads_give_identical_verbose_stderr(cpu_program, tmp_path):
    """-v -v -v interleaves "Processing site" with the warnings of its line: the same stderr for -t 1 and -t 5"""
    g, s, v = cohort(tmp_path, np.random.default_rng(33), 7, 60)
    outs = []
    for t in ("1", "5"):
        prefix = str(tmp_path / ("t" + t))
        outs.append(run_cpu(cpu_program, ["-s", s, "-r", g, "-d", "-t", t, "-p", prefix, "-v", "-v", "-v", v], str(tmp_path), prefix))
    assert outs[0][0] == 0 and outs[0] == outs[1]
    assert b"Processing site: " in outs[0][3] and b"Inconsistent k-mer counts" in outs[0][3]


def test_cpu_program_calls_again_when_the_warnings_need_more_room(cpu_program, monkeypatch, tmp_path):
    """The stand-in's first call has room for 3 warnings (NTSM_STANDIN_FIRST_CAP): the program takes NTSM_VCF_E_CAPACITY,
    makes the room the call asked for and calls again; files and stderr are those of the run with room from the start."""
    g, s, v = cohort(tmp_path, np.random.default_rng(33), 7, 60)
    a, b = str(tmp_path / "plain"), str(tmp_path / "again")
    want = run_cpu(cpu_program, ["-s", s, "-r", g, "-d", "-t", "5", "-p", a, v], str(tmp_path), a)
    assert want[0] == 0 and want[3].count(b"Inconsistent k-mer counts") > 3
    monkeypatch.setenv("NTSM_STANDIN_FIRST_CAP", "3")
    assert run_cpu(cpu_program, ["-s", s, "-r", g, "-d", "-t", "5", "-p", b, v], str(tmp_path), b) == want


def test_cpu_program_names_the_line_of_a_refusal_for_every_t(cpu_program, tmp_path):
    """A bad POS in the last body line: the message names that line of the file, under -t 1 and -t 5"""
    g, s, v = cohort(tmp_path, np.random.default_rng(34), 7, 60)
    with open(v, "a") as f:
        f.write("c0\tabc\trsX\tA\tC\t.\tPASS\t.\tGT" + "\t0|1" * 7 + "\n")
    n_lines = open(v, "rb").read().count(b"\n")
    for t in ("1", "5"):
        prefix = str(tmp_path / ("t" + t))
        rc, mat, cen, err = run_cpu(cpu_program, ["-s", s, "-r", g, "-d", "-t", t, "-p", prefix, v], str(tmp_path), prefix)
        assert rc == 1 and mat is None and cen is None
        assert err.splitlines()[-1] == ("Error: line %d of the VCF: POS 'abc' is not an int" % n_lines).encode(), (t, err)


def test_cpu_program_prints_19_digits_only_after_the_first_undefined_cell(cpu_program, restatement, tmp_path):
    """Three sites, two samples; the site in the middle has no VCF line, so its row is undefined.  Sample 2 of the sites
    around it is hom2 in one line and het in a second one (REF m, VAR 2m: 1/3).  The cell right before the first
    undefined cell is printed with the stream's 6 digits, the same value after it with 19 -- for -t 1 and -t 5."""
    chrom = "".join(np.random.default_rng(36).choice(list("ACGT"), size=400))
    sites = [site_of(chrom, pos, rs="rs%d" % pos) for pos in (100, 200, 300)]
    lines = [["chr1", str(pos), "rs%d" % pos, chrom[pos - 1], ALT[chrom[pos - 1]], ".", "PASS", ".", "GT", "0|0", gt]
             for pos in (100, 300) for gt in ("1|1", "0|1")]
    g, s, v = write_case(tmp_path, [("chr1", chrom)], sites, ["S0", "S1"], lines)
    b = str(tmp_path / "rs")
    p = subprocess.run([restatement, "-s", s, "-r", g, "-p", b, v], capture_output=True, check=True)
    want = (0, open(b + "_matrix.tsv", "rb").read(), open(b + "_center.txt", "rb").read(), p.stderr)
    rows = want[1].split(b"\n")
    assert rows[1] == b"rs100\t1\t0.333333" and rows[3] == b"rs300\t1\t0.3333333333333333148" and rows[2].startswith(b"rs200\t")
    for t in ("1", "5"):
        a = str(tmp_path / ("t" + t))
        assert run_cpu(cpu_program, ["-s", s, "-r", g, "-t", t, "-p", a, v], str(tmp_path), a) == want, t


def test_cpu_program_reads_a_directory_as_an_empty_vcf(cpu_program, tmp_path):
    """A directory given as the VCF: the exit status and the bytes of the same command on an empty file"""
    g, s, _ = cohort(tmp_path, np.random.default_rng(35), 7, 60)
    empty, folder = str(tmp_path / "empty.vcf"), str(tmp_path / "folder.vcf")
    open(empty, "wb").close()
    os.mkdir(folder)
    outs = []
    for name, v in (("e", empty), ("f", folder)):
        prefix = str(tmp_path / name)
        outs.append(run_cpu(cpu_program, ["-s", s, "-r", g, "-d", "-t", "5", "-p", prefix, v], str(tmp_path), prefix))
    assert outs[0] == outs[1] and outs[0][0] == 0 and outs[0][1].startswith(b"alleleID\n")


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cli_gives_the_fixtures(built, tmp_path, case):
    d = os.path.join(GOLD, case["name"])
    prefix = str(tmp_path / "out")
    rc, mat, cen, err = run(VCF, ["-s", "sites.fa", "-r", "genome.fa"] + case["args"] + ["-p", prefix, "in.vcf"], d, prefix)
    assert rc == 0, err
    assert mat == open(os.path.join(d, "expected_matrix.tsv"), "rb").read()
    assert cen == open(os.path.join(d, "expected_center.txt"), "rb").read()
    assert err == open(os.path.join(d, "expected_stderr.txt"), "rb").read()


@pytest.mark.gpu
@pytest.mark.parametrize("n_samples,n_snps,args,seed", [
    (7, 300, ["-d"], 1), (100, 800, ["-d", "-m", "128"], 2), (33, 500, ["-d", "-m", "200", "-k", "11", "-w", "41"], 3),
    (61, 400, [], 4), (3202, 2500, ["-d"], 5)], ids=["small", "m128", "m200_k11", "no_dupes_sparse", "3202x2500"])
def test_cli_matches_restatement_on_cohorts(built, restatement, tmp_path, n_samples, n_snps, args, seed):
    """Seeded cohorts with dense overlaps (shared k-mers, conflicting inserts): matrix, centre file and stderr byte for
    byte against the restatement."""
    rng = np.random.default_rng(seed)
    g, s, v = cohort(tmp_path, rng, n_samples, n_snps, dense="-d" in args)
    a, b = str(tmp_path / "port"), str(tmp_path / "rs")
    rc, mat, cen, err = run(VCF, ["-s", s, "-r", g, "-p", a, "-t", "8"] + args + [v], str(tmp_path), a)
    assert rc == 0, err[-500:]
    p = subprocess.run([restatement, "-s", s, "-r", g, "-p", b] + args + [v], capture_output=True, check=True)
    assert mat == open(b + "_matrix.tsv", "rb").read()
    assert cen == open(b + "_center.txt", "rb").read()
    assert err == p.stderr
    if "-d" in args:
        assert b"Inconsistent k-mer counts" in err and b"collision" in err


@pytest.mark.gpu
def test_threads_give_identical_bytes(built, tmp_path):
    rng = np.random.default_rng(11)
    g, s, v = cohort(tmp_path, rng, 300, 1500)
    outs = []
    for t in ("1", "16"):
        prefix = str(tmp_path / ("t" + t))
        outs.append(run(VCF, ["-s", s, "-r", g, "-d", "-t", t, "-p", prefix, "-v", "-v", "-v", v], str(tmp_path), prefix))
    assert outs[0][0] == 0 and outs[0] == outs[1]
    assert b"Processing site: " in outs[0][3]


@pytest.mark.gpu
def test_gzip_and_bgzf_vcf_give_the_plain_bytes(built, tmp_path):
    rng = np.random.default_rng(12)
    g, s, v = cohort(tmp_path, rng, 200, 1200)
    data = open(v, "rb").read()
    open(v + ".gz", "wb").write(gzip.compress(data))
    open(v + ".bgz", "wb").write(bgzf(data))
    outs = []
    for f in (v, v + ".gz", v + ".bgz"):
        prefix = str(tmp_path / os.path.basename(f).replace(".", "_"))
        outs.append(run(VCF, ["-s", s, "-r", g, "-d", "-t", "4", "-p", prefix, f], str(tmp_path), prefix))
    assert outs[0][0] == 0 and outs[0][1].count(b"\n") > 100
    assert outs[1] == outs[0] and outs[2] == outs[0]


def numpy_model(geno, multi, key_events, site_ref, site_var):
    n = geno.shape[1]
    v1, v2 = np.uint64(multi), np.uint64((2 * multi) & 0xFFFFFFFF)
    state, warns = [], []
    for evs in key_events:
        st = np.zeros(n, dtype=np.uint64)
        for ordv, line, side in evs:
            code = geno[line]
            full = 2 if side else 0
            ins = (code == full) | (code == 1)
            val = np.where(code == full, v2, v1)
            busy = ins & (st != 0)
            for j in np.nonzero(busy & (st != val))[0]:
                warns.append((ordv, int(j), int(st[j]), int(val[j])))
            fresh = ins & (st == 0)
            st[fresh] = val[fresh] & np.uint64(255)
        state.append(st)
    m = len(site_ref)
    cells = np.zeros((m, n), dtype=np.uint16)
    sums = np.zeros(m)
    first = np.full(m, n, dtype=np.uint32)
    for i in range(m):
        r = np.max([state[q] for q in site_ref[i]], axis=0) if site_ref[i] else np.zeros(n, dtype=np.uint64)
        w = np.max([state[q] for q in site_var[i]], axis=0) if site_var[i] else np.zeros(n, dtype=np.uint64)
        cells[i] = (r | (w << np.uint64(8))).astype(np.uint16)
        acc = 0.0
        for j in range(n):
            d = int(r[j]) + int(w[j])
            if d == 0:
                first[i] = min(first[i], j)
            else:
                acc += float(r[j]) / float(d)
        sums[i] = acc
    return cells, sums, first, sorted(warns)


@pytest.mark.gpu
@pytest.mark.parametrize("multi", [20, 127, 128, 200])
def test_device_step_matches_numpy_model(built, multi):
    """ntsm_vcf_run on adversarial event lists: many events per key, both sides on one key, genotypes that conflict,
    keys without events, sites without keys, sample counts that are not a multiple of 16."""
    import ntsm_amd.vcf as V
    rng = np.random.default_rng(multi)
    n, n_lines, n_keys, m = 37, 60, 90, 25
    geno = rng.integers(0, 4, size=(n_lines, n)).astype(np.uint8)             # 3: no insert on either side
    n_ev = 700
    ords = np.arange(n_ev)
    keys = rng.integers(0, n_keys - 5, size=n_ev)                                # the last keys get no events
    lines = np.sort(rng.integers(0, n_lines, size=n_ev))
    sides = rng.integers(0, 2, size=n_ev)
    key_events = [[(int(o), int(l), int(sd)) for o, k, l, sd in zip(ords, keys, lines, sides) if k == q] for q in range(n_keys)]
    perm = rng.permutation(n_keys)                                              # every key in exactly one list, some lists empty
    cut = [0] + sorted(int(x) for x in rng.integers(0, n_keys + 1, size=2 * m - 1)) + [n_keys]
    site_ref = [[int(x) for x in perm[cut[2 * i]:cut[2 * i + 1]]] for i in range(m)]
    site_var = [[int(x) for x in perm[cut[2 * i + 1]:cut[2 * i + 2]]] for i in range(m)]
    cells, sums, first, warn, _ = V.run(geno, multi, key_events, site_ref, site_var, warn_cap=4)   # the caller's E_CAPACITY round trip
    ec, es, ef, ew = numpy_model(geno, multi, key_events, site_ref, site_var)
    assert np.array_equal(cells, ec)
    assert np.array_equal(sums.view(np.uint64), es.view(np.uint64))
    assert np.array_equal(first, ef)
    assert [tuple(int(x) for x in w) for w in warn] == ew
    assert len(ew) > 4


def wide_lists(rng, n, n_lines, n_sites, events_on_key0):
    """Small lists for a wide cohort (numpy_model walks warnings and sums in Python): key 0 takes events_on_key0 events
    of both sides, the other events spread over the next keys, the last key of the plain layout has no event and its
    last site no key.  n_sites > 5: one key per site (the sum kernel then needs a second block of 256 sites)."""
    geno = rng.integers(0, 3 if events_on_key0 > 10 else 4, size=(n_lines, n)).astype(np.uint8)
    if n_sites > 5:
        n_keys, n_ev = n_sites, 300
        keys = np.sort(rng.integers(0, n_keys, size=n_ev))
        site_ref = [[q] if q % 2 == 0 else [] for q in range(n_keys)]
        site_var = [[q] if q % 2 == 1 else [] for q in range(n_keys)]
    else:
        n_keys, n_ev = 12, 40
        keys = np.sort(np.concatenate([np.zeros(events_on_key0, dtype=np.int64), rng.integers(1, n_keys - 1, size=n_ev - events_on_key0)]))
        site_ref = [[0, 1, 2], [5], [7, 8], [11], []]                           # key 11: no events; site 4: no keys
        site_var = [[3, 4], [6], [], [9, 10], []]
    lines = rng.integers(0, n_lines, size=n_ev)
    sides = rng.integers(0, 2, size=n_ev)
    sides[:2] = (0, 1)                                                          # both sides on key 0
    key_events = [[(int(o), int(lines[o]), int(sides[o])) for o in np.flatnonzero(keys == q)] for q in range(n_keys)]
    return geno, key_events, site_ref, site_var


WIDE_STEPS = [(1024, 20, 5, 4), (1025, 20, 5, 4), (3073, 20, 5, 4), (4096, 20, 5, 4), (4097, 20, 5, 4), (4113, 128, 5, 4), (8200, 20, 5, 30),
              (1025, 20, 257, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,multi,n_sites,on_key0", WIDE_STEPS, ids=["n%d_m%d_sites%d" % w[:3] for w in WIDE_STEPS])
def test_device_step_matches_numpy_model_on_wide_cohorts(built, n, multi, n_sites, on_key0):
    """ntsm_vcf_run where the state kernel changes its launch: a lane holds 16 samples and a workgroup 64 to 256 lanes.
    1,024 samples: 64 lanes, all full; 1,025: 128 lanes, the last chunk one live sample and 15 padding bytes; 3,073: 256
    lanes; 4,096: every lane one chunk; 4,097: lane 0 alone loops to a second chunk of one live sample; 4,113: a second
    pass with a ragged chunk (multi 128: 2 * multi truncates to 0); 8,200: three passes, and more than 65,536 warnings,
    so the buffer regrow runs together with the lane loop; 257 sites: the sum kernel's second block.  Cells, sums by
    their bits, first_undef and the sorted warnings against numpy_model."""
    import ntsm_amd.vcf as V
    rng = np.random.default_rng(n + multi + n_sites)
    geno, key_events, site_ref, site_var = wide_lists(rng, n, 10, n_sites, on_key0)
    ec, es, ef, ew = numpy_model(geno, multi, key_events, site_ref, site_var)
    assert any(len(e) == 0 for e in key_events) and len(ew) > n // 4
    if n == 8200:
        assert len(ew) > 65536
    cells, sums, first, warn, times = V.run(geno, multi, key_events, site_ref, site_var, warn_cap=1 << 18)
    assert times.state_launches == (2 if len(ew) > 65536 else 1)
    bad = np.argwhere(cells != ec)
    assert bad.size == 0, (n, bad[:10].tolist())                                # (site, sample): chunk = sample // 16, lane = chunk % block
    assert np.array_equal(sums.view(np.uint64), es.view(np.uint64))
    assert np.array_equal(first, ef)
    assert len(warn) == len(ew)
    assert np.array_equal(np.stack([warn[f] for f in ("event", "sample", "old", "value")], axis=1).astype(np.int64),
                          np.array(ew, dtype=np.int64).reshape(-1, 4))


@pytest.mark.gpu
def test_device_step_regrows_its_warning_buffer(built):
    """More warnings than the device buffer starts with (65,536): the buffer is grown and both kernels run again; the
    result of that second launch is what comes back, and it equals the model.  One key: line 0 makes every sample's byte
    2m (hom1), then 300 events of line 1 (het) each conflict with it for all 301 samples: 90,300 warnings."""
    import ntsm_amd.vcf as V
    n, multi = 301, 20
    geno = np.array([[V.HOM1] * n, [V.HET] * n], dtype=np.uint8)
    key_events = [[(0, 0, 0)] + [(o, 1, 0) for o in range(1, 301)], [(301, 1, 1)]]
    site_ref, site_var = [[0], []], [[], [1]]
    cells, sums, first, warn, times = V.run(geno, multi, key_events, site_ref, site_var, warn_cap=1 << 17)
    assert times.state_launches == 2
    ec, es, ef, ew = numpy_model(geno, multi, key_events, site_ref, site_var)
    assert len(ew) == 300 * n
    assert np.array_equal(cells, ec) and np.array_equal(sums.view(np.uint64), es.view(np.uint64)) and np.array_equal(first, ef)
    assert np.array_equal(warn["event"], [w[0] for w in ew]) and np.array_equal(warn["sample"], [w[1] for w in ew])
    assert set(warn["old"].tolist()) == {40} and set(warn["value"].tolist()) == {20}
    # below the initial size: one launch
    _, _, _, warn2, times2 = V.run(geno[:, :100], multi, [[(0, 0, 0)] + [(o, 1, 0) for o in range(1, 301)]], [[0]], [[]],
                                   warn_cap=1 << 17)
    assert times2.state_launches == 1 and len(warn2) == 300 * 100


@pytest.mark.gpu
def test_device_step_reports_a_refused_device_and_works_afterwards(built):
    """ntsm_vcf_run on a device ordinal that does not exist returns -2 (hipSetDevice's error, no device fault), and the
    next call on device 0 gives the model's answer for one site with one key."""
    import ntsm_amd.vcf as V
    geno = np.array([[V.HOM1, V.HET, V.HOM2]], dtype=np.uint8)
    key_events, site_ref, site_var = [[(0, 0, 0)]], [[0]], [[]]
    with pytest.raises(RuntimeError, match=r"ntsm_vcf_run failed: -2$"):
        V.run(geno, 20, key_events, site_ref, site_var, device=1 << 20)
    cells, sums, first, warn, times = V.run(geno, 20, key_events, site_ref, site_var)
    ec, es, ef, ew = numpy_model(geno, 20, key_events, site_ref, site_var)
    assert ec.tolist() == [[40, 20, 0]] and es.tolist() == [2.0] and ef.tolist() == [2] and ew == []
    assert np.array_equal(cells, ec) and np.array_equal(sums.view(np.uint64), es.view(np.uint64)) and np.array_equal(first, ef)
    assert len(warn) == 0 and times.state_launches == 1


@pytest.mark.gpu
def test_chain_centre_file_into_ntsmEval(built, tmp_path):
    """ntsmVCF -p's centre file and a synthetic rotation through ntsmEval -p ROT -n CENTRE give the stdout that the
    restatements (tests/vcf_restatement.cpp for the centres, tests/eval_pca_restatement.cpp for the search) expect."""
    from test_eval import files_for, random_samples
    from test_eval_pca import expected_text, gxx
    rng = np.random.default_rng(21)
    vrs = gxx(tmp_path, "vcf_restatement.cpp", "vcf_restatement")
    ers = gxx(tmp_path, "eval_pca_restatement.cpp", "eval_pca_restatement")
    g, s, v = cohort(tmp_path, rng, 150, 600)
    a, b = str(tmp_path / "port"), str(tmp_path / "rs")
    rc, _, cen, err = run(VCF, ["-s", s, "-r", g, "-d", "-p", a, v], str(tmp_path), a)
    assert rc == 0, err[-500:]
    subprocess.run([vrs, "-s", s, "-r", g, "-d", "-p", b, v], capture_output=True, check=True)
    assert cen == open(b + "_center.txt", "rb").read()
    m = cen.count(b"\n")
    rot = str(tmp_path / "rot.tsv")
    with open(rot, "w") as f:
        f.write("rsID\t" + "\t".join("PC%d" % (d + 1) for d in range(20)) + "\n")
        for j in range(m):
            f.write("rs%d\t%s\n" % (j, "\t".join("%.17g" % x for x in rng.normal(0, 0.05, size=20))))
    files = files_for(tmp_path, random_samples(rng, 24, m, depth=20.0))
    want, _, _ = expected_text(ers, tmp_path, files, 20, b + "_center.txt", rot, all_=True)
    p = subprocess.run([EVAL, "-a", "-p", rot, "-n", a + "_center.txt"] + files, capture_output=True)
    assert p.returncode == 0 and p.stdout == want and want.count(b"\n") >= 2, p.stderr[-300:]
