"""ntsmSiteGen: build/ntsmSiteGen (ntsm_amd/csrc/host/ntsm_sitegen_main.cpp) and its device step
(include/ntsm_sitegen_hip.h, ntsm_amd/csrc/ntsm_sitegen.hip, ntsm_amd/sitegen.py).

The contract of steps 1 and 3 is upstream's two scripts; the fixtures under tests/golden/sitegen/ are the outputs of the
unmodified scripts (README there).  The contract of step 2 is the definition of H in the header;
tests/sitegen_restatement.cpp states it as a brute force.  CPU: the program with -H and the restatement both reproduce
every fixture, every refusal, the flags.  GPU: the C ABI against the brute force value for value (k = 11 .. 31, x = 0 / 1,
one piece and many chunks, duplicates, an empty set, a dense set, a genome longer than one staging buffer), the program
without -H against the fixtures, and the chain into ntsmCount and ntsmVCF."""
import gzip
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_binding import ROOT  # noqa: E402

EXE = os.path.join(ROOT, "build", "ntsmSiteGen")
GOLD = os.path.join(ROOT, "tests", "golden", "sitegen")
CASES = json.load(open(os.path.join(GOLD, "cases.json")))
IDS = [c["name"] for c in CASES]
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


@pytest.fixture(scope="module")
def restatement(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("srs") / "sitegen_restatement")
    subprocess.run(["g++", "-O2", "-std=c++11", "-o", exe, os.path.join(ROOT, "tests", "sitegen_restatement.cpp")], check=True)
    return exe


def gold(case, name):
    path = os.path.join(GOLD, "expected", case["name"], name)
    return gzip.open(path + ".gz", "rb").read() if os.path.exists(path + ".gz") else open(path, "rb").read()


def inputs(case):
    return os.path.join(GOLD, "inputs", case["genome"]), os.path.join(GOLD, "inputs", case["vcf"])


def flags(case):
    return ["-k", str(case["k"]), "-w", str(case["w"]), "-x", str(case["x"])] + (["-i"] if case["keep_all"] else [])


def outputs(prefix, case, suffixes=None):
    names = suffixes or ["_subKmers.fa"] + ["_n%d.fa" % i for i in range(case["w"] - case["k"] + 1)]
    return {n: open(prefix + n, "rb").read() for n in names}


def expected(case):
    out = {"_subKmers.fa": gold(case, "subKmers.fa")}
    for i in range(case["w"] - case["k"] + 1):
        out["_n%d.fa" % i] = gold(case, "n%d.fa" % i)
    return out


def hits_file(tmp_path, case):
    path = str(tmp_path / (case["name"] + "_hits.tsv"))
    open(path, "wb").write(gold(case, "subKmerHits.tsv"))
    return path


def run(args, **kw):
    return subprocess.run([EXE] + args, capture_output=True, timeout=900, **kw)


def no_time(err):
    return b"".join(l for l in err.splitlines(True) if not l.startswith((b"Time: ", b"Device: ")))


# ------------------------------------------------------------------------------------------------ CPU: steps 1 and 3
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_hits_file_run_gives_the_recordings(built, tmp_path, case):
    """-H: candidates, stderr and every _n{i}.fa byte-identical to what the unmodified upstream scripts wrote"""
    g, v = inputs(case)
    p = str(tmp_path / "out")
    r = run(["-r", g, "-v", v, "-p", p, "-H", hits_file(tmp_path, case)] + flags(case))
    assert r.returncode == 0, r.stderr[-500:]
    assert r.stderr == gold(case, "stderr.txt")
    assert outputs(p, case) == expected(case)
    assert not os.path.exists(p + "_subKmerHits.tsv")          # -H: the counts were given, none are written


def test_upstream_spelling_threads_and_gzip_give_the_same_bytes(built, tmp_path):
    case = CASES[0]
    g, v = inputs(case)
    want = expected(case)
    h = hits_file(tmp_path, case)
    variants = [["-r", g, "-v", v, "-H", h, "-t", "1", "-p"], ["-r", g, "-v", v, "-H", h, "-t", "3", "-p"],
                ["-t", "16", "-H", h, "-k", "19", "-w", "31", "-v", v, "-r", g, "-p"]]
    for n, args in enumerate(variants):
        p = str(tmp_path / ("t%d" % n))
        r = run(args + [p])
        assert r.returncode == 0 and r.stderr == gold(case, "stderr.txt") and outputs(p, case) == want, args
    # upstream's spelling; hits= is this program's own addition to it (-H)
    for n, args in enumerate((["ref=" + g, "vcf=" + v, "hits=" + h], ["t=2", "k=19", "hits=" + h, "vcf=" + v, "w=31", "ref=" + g])):
        p = str(tmp_path / ("u%d" % n))
        r = run(["generate-sites", "name=" + p] + args)
        assert r.returncode == 0 and r.stderr == gold(case, "stderr.txt") and outputs(p, case) == want, args
    gz = str(tmp_path / "genome.fa.gz")
    with gzip.open(gz, "wb") as f:
        f.write(open(g, "rb").read())
    p = str(tmp_path / "gz")
    r = run(["-r", gz, "-v", v, "-p", p, "-H", h])
    assert r.returncode == 0 and r.stderr == gold(case, "stderr.txt") and outputs(p, case) == want


def test_upstream_spelling_maps_onto_the_flags(built, tmp_path):
    """generate-sites name= ref= vcf= k= w= t=: the same parameter checks and refusals as the flag form (its full run needs
    the device: test_program_on_the_device); generate-pca-rot-mat names the two programs that replace it"""
    case = CASES[0]
    g, v = inputs(case)
    r = run(["generate-pca-rot-mat", "name=x", "sites=12", "multivcf=m.vcf"])
    assert r.returncode == 1 and b"ntsmVCF" in r.stderr and b"ntsmPCA" in r.stderr and r.stderr.startswith(b"Error: ")
    r = run(["generate-sites", "ref=" + g, "vcf=" + v])
    assert r.returncode == 1 and b"missing required param 'name'" in r.stderr
    r = run(["generate-sites", "name=" + str(tmp_path / "o"), "vcf=" + v])
    assert r.returncode == 1 and b"missing required param 'ref'" in r.stderr
    r = run(["generate-sites", "name=" + str(tmp_path / "o"), "ref=" + g])
    assert r.returncode == 1 and b"missing required param 'vcf'" in r.stderr
    r = run(["generate-sites", "name=" + str(tmp_path / "o"), "ref=" + g, "vcf=" + v, "k=32"])
    assert r.returncode == 1 and r.stderr.startswith(b"Error: k must be")
    r = run(["generate-sites", "name=" + str(tmp_path / "o"), "ref=" + g, "vcf=" + v, "k=19", "w=18", "t=2"])
    assert r.returncode == 1 and r.stderr.startswith(b"Error: w must be")
    r = run(["generate-sites", "name=" + str(tmp_path / "o"), "ref=" + g, "vcf=" + v, "dims=20"])
    assert r.returncode == 1 and r.stderr.startswith(b"Error: ")
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_reproduces_the_recordings(restatement, tmp_path, case):
    """so the brute-force H that wrote the SAM-shaped text of the recipe is the H the device is checked against"""
    g, v = inputs(case)
    p = str(tmp_path / "rs")
    r = subprocess.run([restatement, "all", g, v, p, str(case["k"]), str(case["w"]), str(case["x"]), str(int(case["keep_all"]))],
                       capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr[-300:]
    assert r.stderr == gold(case, "stderr.txt")
    assert outputs(p, case) == expected(case)
    assert open(p + "_subKmerHits.tsv", "rb").read() == gold(case, "subKmerHits.tsv")


def planted_genome(rng, n, k, n_cands):
    """a genome of about n bases in three records with copies of its own k-mers planted (exact, one and two substitutions,
    reverse strand, lower case, N inside), and candidates drawn from it: (records, candidates)"""
    base = "".join(rng.choice(list("ACGT"), size=n))
    cands, extra = [], []
    for i in range(n_cands):
        at = int(rng.integers(0, n - k))
        q = list(base[at:at + k])
        kind = i % 8
        if kind in (1, 2, 3):
            for o in rng.choice(k, size=kind if kind < 3 else 1, replace=False):
                q[o] = rng.choice([b for b in "ACGT" if b != q[o]])
        q = "".join(q)
        if kind == 4:
            q = "".join(COMP[c] for c in reversed(q))
        cands.append(q)
        m = list(base[at:at + k])
        o = [0, k - 1, k // 3 - 1, k // 3, 2 * (k // 3) - 1, 2 * (k // 3)][i % 6]
        m[o] = rng.choice([b for b in "ACGT" if b != m[o]])
        piece = "".join(m)
        if kind == 5:
            piece = piece.lower()
        if kind == 6:
            piece = piece[:k // 2] + "N" + piece[k // 2 + 1:]
        if kind == 7:
            piece = "".join(COMP[c] for c in reversed(piece))
        extra.append(piece + "".join(rng.choice(list("ACGT"), size=int(rng.integers(0, 5)))))
    third = "".join(extra)
    cut = n // 2 + 3
    return [base[:cut], base[cut:], third, "ACGT"], cands      # the last record is shorter than any k


def write_fasta(path, records):
    with open(path, "w") as f:
        for i, seq in enumerate(records):
            f.write(">r%d\n%s\n" % (i, seq))


def brute(restatement, tmp_path, records, cands, k, x, method="naive", tag="b"):
    fa, km = str(tmp_path / (tag + ".fa")), str(tmp_path / (tag + ".txt"))
    write_fasta(fa, records)
    open(km, "w").write("".join(c + "\n" for c in cands))
    r = subprocess.run([restatement, "hits", fa, km, str(k), str(x), method], capture_output=True, check=True, timeout=1800)
    return np.array(r.stdout.split(), dtype=np.int64) if cands else np.zeros(0, dtype=np.int64)


@pytest.mark.parametrize("k,x", [(11, 1), (19, 0), (19, 1), (31, 1)])
def test_the_faster_brute_forces_agree_with_the_definition(restatement, tmp_path, k, x):
    """"neighbours" (the dense GPU test) and "halves" (the full-size check of tools/sitegen_bench.py), used where
    every-candidate-against-every-window is too slow, give the definition's counts"""
    rng = np.random.default_rng(100 + k + x)
    records, cands = planted_genome(rng, 6000, k, 240)
    records.append(cands[0] * 1 + ("G" + cands[0]) * 299)        # saturates
    cands += cands[:5]                                            # duplicates
    a = brute(restatement, tmp_path, records, cands, k, x, "naive")
    b = brute(restatement, tmp_path, records, cands, k, x, "neighbours")
    c = brute(restatement, tmp_path, records, cands, k, x, "halves")
    assert np.array_equal(a, b) and np.array_equal(a, c) and a.max() == 255 and (a == 0).any() and (a == 1).any() and (a[a < 255] > 1).any()


# ------------------------------------------------------------------------------------------------ CPU: refusals
def small_inputs(tmp_path, lines, genome=None):
    g, v = str(tmp_path / "g.fa"), str(tmp_path / "s.vcf")
    rng = np.random.default_rng(5)
    seq = "".join(rng.choice(list("ACGT"), size=400))
    seq = seq[:99] + "A" + seq[100:199] + "N" + seq[200:]      # base 100 is A, base 200 is N
    open(g, "w").write(genome if genome is not None else ">c1 first\n%s\n>c2\n%s\n" % (seq, seq[::-1]))
    open(v, "w").write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n" + "".join(l + "\n" for l in lines))
    return g, v


GOOD = "c1\t100\trs1\tA\tC"
REFUSALS = [
    ("multi_alt", [GOOD, "c1\t150\trs2\tA\tC,G"], [], b"Error: Multiple alternate alleles found in VCF\n"),
    ("long_alt", ["c1\t150\trs2\tA\tCG"], [], b"Error: Multiple alternate alleles found in VCF\n"),
    ("four_fields", [GOOD, "c1\t150\trs2\tA"], [], b"fewer than five fields"),
    ("alt_only_blank", ["c1\t150\trs2\tA\t"], [], b"fewer than five fields"),
    ("empty_line", [GOOD, "", GOOD], [], b"fewer than five fields"),
    ("pos_not_int", ["c1\t1e2\trs2\tA\tC"], [], b"POS is not an integer"),
    ("pos_empty", ["c1\t\trs2\tA\tC"], [], b"POS is not an integer"),
    ("unknown_chromosome", ["c9\t100\trs2\tA\tC"], [], b"is not in the genome"),
    ("description_is_not_the_name", ["first\t100\trs2\tA\tC"], [], b"is not in the genome"),
    ("window_before_start", ["c1\t15\trs2\tA\tC"], [], b"does not lie inside"),
    ("window_past_end", ["c1\t386\trs2\tA\tC"], [], b"does not lie inside"),
    ("negative_pos", ["c1\t-5\trs2\tA\tC"], [], b"does not lie inside"),
    ("n_in_window", ["c1\t100\trs1\tA\tC", "c1\t190\trs2\t%s\tC"], [], b"outside ACGT"),
    ("alt_lower_case", ["c1\t100\trs1\tA\tc"], [], b"not one of ACGT"),
    ("alt_n", ["c1\t100\trs1\tA\tN"], [], b"not one of ACGT"),
    ("k_zero", [GOOD], ["-k", "0"], b"Error: k must be"),
    ("k_32", [GOOD], ["-k", "32", "-w", "40"], b"Error: k must be"),
    ("w_below_k", [GOOD], ["-k", "19", "-w", "18"], b"Error: w must be"),
    ("x_2", [GOOD], ["-x", "2"], b"Error: x must be"),
]


@pytest.mark.parametrize("name,lines,extra,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(built, tmp_path, name, lines, extra, msg):
    """message on stderr, exit 1, no file written"""
    work = tmp_path / "in"
    work.mkdir()
    g, v = small_inputs(work, lines)
    if name == "n_in_window":                                   # REF must match for the window to reach the encoder
        seq = open(g).read().split("\n")[1]
        ref = seq[189]
        alt = "C" if ref in "AT" else "A"
        g, v = small_inputs(work, [lines[0], "c1\t190\trs2\t%s\t%s" % (ref, alt)])
    out = tmp_path / "out"
    out.mkdir()
    hits = str(work / "none.tsv")
    open(hits, "w").close()
    r = run(["-r", g, "-v", v, "-p", str(out / "p"), "-H", hits] + extra)
    assert r.returncode == 1 and msg in r.stderr and b"Error: " in r.stderr, r.stderr[-300:]
    assert os.listdir(str(out)) == []


def test_skips_that_are_not_refusals(built, restatement, tmp_path):
    """a window with N, a multi-base REF, a lower-case REF whose wild type does not match are skipped with the five lines,
    as the script does; an A <-> T SNP over an N window is dropped by the rule before the encoder sees it"""
    seq = open(small_inputs(tmp_path, [])[0]).read().split("\n")[1]
    t_or_a = {"A": "T", "T": "A", "C": "G", "G": "C"}
    lines = [GOOD, "c1\t190\trs2\t%s\tC" % ("G" if seq[189] != "G" else "T"), "c1\t100\trs3\tAC\tG", "c1\t100\trs4\ta\tG",
             "c1\t195\trs5\t%s\t%s" % (seq[194], t_or_a[seq[194]]), "c2\t120\t.\t%s\tA" % seq[::-1][119], "c1\t 100 \trs6\tA\tG"]
    g, v = small_inputs(tmp_path, lines)
    p, q = str(tmp_path / "p"), str(tmp_path / "q")
    r = subprocess.run([restatement, "all", g, v, q, "19", "31", "1", "0"], capture_output=True)
    assert r.returncode == 0, r.stderr
    r2 = run(["-r", g, "-v", v, "-p", p, "-H", q + "_subKmerHits.tsv"])
    assert r2.returncode == 0 and r2.stderr == r.stderr and r.stderr.count(b"Wildtype allele does not match") == 3
    assert outputs(p, CASES[0]) == outputs(q, CASES[0])


def test_hits_file_must_name_the_computed_candidates(built, tmp_path):
    case = CASES[2]
    g, v = inputs(case)
    good = gold(case, "subKmerHits.tsv").splitlines(True)
    for n, bad in enumerate((good[:-1], good + good[:1], good[:3] + [good[3].replace(b"|AT\t", b"|XX\t").replace(b"|CG\t", b"|AT\t").replace(b"|XX\t", b"|CG\t")] + good[4:],
                             good[:5] + [good[5].split(b"\t")[0] + b"\tx\n"] + good[6:])):
        out = tmp_path / ("o%d" % n)
        out.mkdir()
        h = str(tmp_path / ("h%d.tsv" % n))
        open(h, "wb").write(b"".join(bad))
        r = run(["-r", g, "-v", v, "-p", str(out / "p"), "-H", h] + flags(case))
        assert r.returncode == 1 and r.stderr.count(b"Error: ") == 1 and os.listdir(str(out)) == [], (n, r.stderr[-300:])


# ------------------------------------------------------------------------------------------------ CPU: the build
SCALAR_MEMORY = re.compile(r"\bs_(?:buffer|scratch|dcache|atomic|load|store)\w*", re.I)
SCALAR_LOAD = re.compile(r"^s_(?:buffer_)?load_", re.I)


def test_library_builds_clean_and_its_scalar_memory_instructions_are_loads(built, tmp_path):
    """the project's flags with -Werror; in the gfx950 assembly every scalar memory instruction is a load, and neither
    source names any other"""
    src = os.path.join(ROOT, "ntsm_amd", "csrc", "ntsm_sitegen.hip")
    flags_ = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Werror", "-fvisibility=hidden"]
    asm = str(tmp_path / "sitegen.s")
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + flags_ + ["-c", "-o", str(tmp_path / "both.o"), src], capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + flags_ + ["-Wno-unused-command-line-argument", "--cuda-device-only", "-S", "-o", asm, src],
                       capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
    text = open(asm).read()
    assert "scan_kernel" in text and "v_" in text
    found = set(m.group(0).lower() for m in SCALAR_MEMORY.finditer(text))
    assert found and all(SCALAR_LOAD.match(m) for m in found), sorted(found)
    for path in (src, os.path.join(ROOT, "ntsm_amd", "csrc", "host", "ntsm_sitegen_main.cpp"), os.path.join(ROOT, "include", "ntsm_sitegen_hip.h"),
                 os.path.join(ROOT, "ntsm_amd", "sitegen.py")):
        assert not [m.group(0) for m in SCALAR_MEMORY.finditer(open(path).read()) if not SCALAR_LOAD.match(m.group(0))], path
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "ntsm_amd", "libntsm_sitegen_hip.so")], capture_output=True, check=True)
    names = set(l.split()[-1] for l in syms.stdout.decode().splitlines() if l.split()[-2] in "TtDdBb")
    assert set(n for n in names if not n.startswith("__hip_")) == {"ntsm_sitegen_open", "ntsm_sitegen_submit", "ntsm_sitegen_hits",
                                                                     "ntsm_sitegen_times_get", "ntsm_sitegen_close"}


def test_staging_state_machine_under_sanitizers(tmp_path):
    """tests/sitegen_stage_check.cpp, a program of its own under ASan + UBSan: the staging layer that both device libraries
    share (ntsm_amd/csrc/ntsm_sitegen_stage.h) with buffers of 64 and 256 bytes, k = 11, 19, 31, both seam settings, whole
    and in chunks around k and around the buffer size: launch shapes, every window counted once, refused ends stage nothing"""
    exe = str(tmp_path / "sitegen_stage_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "sitegen_stage_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, timeout=120)
    assert p.returncode == 0 and p.stdout.startswith(b"stage check ok: 96 cases"), (p.stdout + p.stderr).decode()[-2000:]


# ------------------------------------------------------------------------------------------------ GPU: the C ABI
def fasta_records(path):
    recs = []
    for line in open(path):
        if line.startswith(">"):
            recs.append([])
        else:
            recs[-1].append(line.strip())
    return ["".join(r) for r in recs]


def device_hits(cands, k, x, records, chunk=None):
    import ntsm_amd.sitegen as S
    with S.Session(cands, k, x) as s:
        s.submit_records(records, chunk)
        return s.hits().astype(np.int64), s.times()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_counts_on_the_fixtures(built, case):
    """min(H, 255) of every fixture's candidates equal to the recorded brute force, in one piece and in chunks of 1000 and
    of 37 bytes (seams inside the planted copies), twice"""
    if case["k"] < 11:
        pytest.fail("fixtures of the device step need k >= 11")
    rows = gold(case, "subKmerHits.tsv").decode().splitlines()
    want = np.array([int(r.split("\t")[1]) for r in rows], dtype=np.int64)
    cands = gold(case, "subKmers.fa").decode().splitlines()[1::2]
    records = fasta_records(inputs(case)[0])
    got, t = device_hits(cands, case["k"], case["x"], records)
    print("%s: %d candidates, %d windows, %d probes, kernel %.3f ms" % (case["name"], len(cands), t.windows, t.probes, t.kernel_ms))
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert t.windows == sum(len(w) - case["k"] + 1 for r in records for w in re.split("[^ACGTacgt]+", r) if len(w) >= case["k"])
    for chunk in (1000, 37):
        again, _ = device_hits(cands, case["k"], case["x"], records, chunk)
        assert np.array_equal(again, want), chunk


@pytest.mark.gpu
@pytest.mark.parametrize("k", [11, 13, 19, 25, 31])
@pytest.mark.parametrize("x", [0, 1])
def test_device_counts_on_generated_genomes(built, restatement, tmp_path, k, x):
    rng = np.random.default_rng(1000 * x + k)
    records, cands = planted_genome(rng, 30000, k, 600)
    records.append(cands[1] + ("T" + cands[1]) * 299)            # saturates at 255
    cands += cands[:7]                                            # duplicate candidates: each its own count
    want = brute(restatement, tmp_path, records, cands, k, x)
    got, t = device_hits(cands, k, x, records)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert want.max() == 255 and (want == 0).any() and np.array_equal(got[:7], got[-7:])
    assert t.bitmap_tests == t.windows * (3 if x else 1)
    for chunk in (k - 1, 4096):
        again, _ = device_hits(cands, k, x, records, chunk)
        assert np.array_equal(again, want), chunk


@pytest.mark.gpu
def test_device_empty_candidate_list_and_bad_arguments(built):
    import ctypes as C
    import ntsm_amd.sitegen as S
    got, t = device_hits([], 19, 1, ["ACGT" * 100])
    assert len(got) == 0 and t.windows == 400 - 18 and t.probes == 0
    h = C.c_void_p()
    one = np.array([5], dtype=np.uint64)
    for k, x in ((10, 1), (32, 1), (19, 2)):
        assert S.lib.ntsm_sitegen_open(0, k, x, 1, one.ctypes.data, C.byref(h)) == -1
    assert S.lib.ntsm_sitegen_open(0, 11, 1, 1, np.array([1 << 22], dtype=np.uint64).ctypes.data, C.byref(h)) == -1
    assert S.lib.ntsm_sitegen_open(0, 19, 1, 1, None, C.byref(h)) == -1
    with S.Session(["A" * 19], 19, 1) as s:
        ends = np.array([5, 3], dtype=np.uint64)
        assert S.lib.ntsm_sitegen_submit(s._h, b"ACGTACGT", 8, ends.ctypes.data, 2) == -1
        ends = np.array([9], dtype=np.uint64)
        assert S.lib.ntsm_sitegen_submit(s._h, b"ACGTACGT", 8, ends.ctypes.data, 1) == -1


@pytest.mark.gpu
def test_device_counts_on_a_dense_candidate_set(built, restatement, tmp_path):
    """2 * 10^5 candidates drawn from a 1 Mb genome: most windows find their bucket occupied, buckets hold several entries"""
    rng = np.random.default_rng(77)
    k, n = 19, 1000000
    codes = rng.integers(0, 4, size=n)
    # a repeat family so that some counts exceed 1 by more than planted noise
    fam = codes[5000:5300].copy()
    for at in rng.integers(10000, n - 400, size=200):
        codes[at:at + 300] = np.where(rng.random(300) < 0.03, rng.integers(0, 4, size=300), fam)
    base = np.array(list("ACGT"))[codes]
    base[rng.integers(0, n, size=50)] = "N"
    genome = "".join(base)
    starts = rng.integers(0, n - k, size=200000)
    cands = []
    for i, at in enumerate(starts):
        q = genome[at:at + k].replace("N", "A")
        if i % 4 == 1:
            o = int(rng.integers(0, k))
            q = q[:o] + "ACGT"[("ACGT".index(q[o]) + 1 + i % 3) % 4] + q[o + 1:]
        if i % 4 == 2:
            q = "".join(COMP[c] for c in reversed(q))
        if i % 16 == 3:
            q = "".join(rng.choice(list("ACGT"), size=k))
        cands.append(q)
    records = [genome[:400000], genome[400000:]]
    want = brute(restatement, tmp_path, records, cands, k, 1, "neighbours", tag="dense")
    got, t = device_hits(cands, k, 1, records)
    print("dense: %d windows, %d probes (%.2f per window), kernel %.3f ms" % (t.windows, t.probes, t.probes / t.windows, t.kernel_ms))
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
    assert t.probes > t.windows and (want > 1).sum() > 1000 and (want == 0).sum() > 1000
    again, _ = device_hits(cands, k, 1, records, 65536)
    assert np.array_equal(again, want)


STAGE = 1 << 27                                                # kStageCap of ntsm_sitegen.hip: bytes per full launch
SEAMS = ["straddles", "ends_at", "in_the_carry", "starts_at", "two_records"]


def mutate(rng, q, subs):
    q = list(q)
    for o in rng.choice(len(q), size=subs, replace=False):
        q[o] = rng.choice([b for b in "ACGT" if b != q[o]])
    return "".join(q)


def seam_case(rng, k, seam):
    """(record text as uint8, record ends, islands, candidates, number of candidates cut from the islands): a text of 'N'
    a little longer than STAGE with islands of random ACGT near offset 0, at the tail and at the seam.  Offsets are those
    of the text; for "two_records" the first record is text[:STAGE - 1], so that its separator is byte STAGE - 1 of the
    staged stream and the second record starts at byte STAGE of it."""
    total = STAGE + 5000
    at_seam = {"straddles": [(STAGE - 150, STAGE + 150)], "ends_at": [(STAGE - 300, STAGE), (STAGE + 1, STAGE + 200)],
               "in_the_carry": [(STAGE - (k - 1), STAGE + 280)], "starts_at": [(STAGE - 250, STAGE - 1), (STAGE, STAGE + 300)],
               "two_records": [(STAGE - 151, STAGE - 1), (STAGE - 1, STAGE + 149)]}[seam]
    spans = [(5, 305)] + at_seam + [(total - 400, total)]
    islands = ["".join(rng.choice(list("ACGT"), size=b - a)) for a, b in spans]
    text = np.full(total, ord("N"), dtype=np.uint8)
    for (a, b), isl in zip(spans, islands):
        text[a:b] = np.frombuffer(isl.encode(), dtype=np.uint8)
    cands = []
    for n_isl, isl in enumerate(islands):
        for at in range(0, len(isl) - k + 1, 1 if 0 < n_isl < len(islands) - 1 else 7):
            q, kind = isl[at:at + k], len(cands) % 4            # exact, one substitution, two, reverse strand
            q = mutate(rng, q, kind) if kind in (1, 2) else q
            cands.append("".join(COMP[c] for c in reversed(q)) if kind == 3 else q)
    cut = len(cands)
    if seam == "two_records":                                   # the window that a scan without the separator would see
        cands.append(islands[1][-(k // 2):] + islands[2][:k - k // 2])
    return text, [STAGE - 1, total] if seam == "two_records" else [total], islands, cands, cut


@pytest.mark.gpu
@pytest.mark.parametrize("k", [19, 31])
@pytest.mark.parametrize("seam", SEAMS)
def test_device_counts_across_a_full_staging_buffer(built, restatement, tmp_path, k, seam):
    """More than one staging buffer (2^27 bytes) through a single submit call: the first launch is full, has no 'N'
    padding behind it, and hands its last k - 1 bytes to the second.  The genome is 'N' except for islands of random
    ACGT: near offset 0, at the tail, and at the seam -- straddling byte 2^27; ending exactly at 2^27 (its last window
    ends on the last byte of the full launch); starting at 2^27 - (k - 1) (its part before the seam is exactly the
    carry: every window ends in the second launch and must be counted once); starting exactly at 2^27; or one island
    cut at 2^27 - 1 into two records, so that the separator is the last byte of the full launch and no window may bridge
    it.  No window crosses an 'N', so the expected counts are the brute force's on a small FASTA of the islands alone.
    Candidates are every window of the seam islands and some of the others: exact, one and two substitutions, reverse
    strand.  full_launches == 1 and launches == 2: if the buffer size ever changes, this fails instead of silently
    missing the seam."""
    import ntsm_amd.sitegen as S
    rng = np.random.default_rng(k * 10 + SEAMS.index(seam))
    text, ends, islands, cands, cut = seam_case(rng, k, seam)
    want = brute(restatement, tmp_path, islands, cands, k, 1)
    assert (want[0:cut:4] >= 1).all() and (want[1:cut:4] >= 1).all() and (want[3:cut:4] >= 1).all() and (want[cut:] == 0).all()
    with S.Session(cands, k, 1) as sess:
        sess.submit(text, ends)
        got, t = sess.hits().astype(np.int64), sess.times()
    assert (t.full_launches, t.launches) == (1, 2)
    assert t.windows == sum(len(isl) - k + 1 for isl in islands)
    assert np.array_equal(got, want), [(int(c), cands[c], int(got[c]), int(want[c])) for c in np.flatnonzero(got != want)[:10]]


# ------------------------------------------------------------------------------------------------ GPU: the program
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_program_on_the_device(built, tmp_path, case):
    """without -H: every output byte-identical to the recordings; its _subKmerHits.tsv fed back through -H gives the same files"""
    g, v = inputs(case)
    p, q = str(tmp_path / "dev"), str(tmp_path / "fed")
    r = run(["-r", g, "-v", v, "-p", p, "-V"] + flags(case))
    assert r.returncode == 0, r.stderr[-500:]
    assert no_time(r.stderr) == gold(case, "stderr.txt") and b"Device: " in r.stderr
    assert outputs(p, case) == expected(case)
    assert open(p + "_subKmerHits.tsv", "rb").read() == gold(case, "subKmerHits.tsv")
    r = run(["-r", g, "-v", v, "-p", q, "-H", p + "_subKmerHits.tsv"] + flags(case))
    assert r.returncode == 0 and outputs(q, case) == expected(case)


@pytest.mark.gpu
def test_program_upstream_spelling_on_the_device(built, tmp_path):
    case = CASES[0]
    g, v = inputs(case)
    p = str(tmp_path / "up")
    r = run(["generate-sites", "name=" + p, "ref=" + g, "vcf=" + v, "t=2"])
    assert r.returncode == 0 and r.stderr == gold(case, "stderr.txt") and outputs(p, case) == expected(case)
    p2 = str(tmp_path / "up2")
    r = run(["generate-sites", "vcf=" + v, "k=19", "name=" + p2, "w=31", "ref=" + g])
    assert r.returncode == 0 and outputs(p2, case) == expected(case)


@pytest.mark.gpu
def test_chain_into_ntsmCount_and_ntsmVCF(built, tmp_path):
    """the most permissive sites file of the main fixture loads in ntsmCount; reads tiled over the fixture genome give
    non-zero counts on the AT side of the sites whose reference base is A / T; ntsmVCF -s accepts the same file"""
    case = CASES[0]
    g, v = inputs(case)
    sites = str(tmp_path / "sites.fa")
    open(sites, "wb").write(gold(case, "n%d.fa" % (case["w"] - case["k"])))
    records = fasta_records(g)
    reads = str(tmp_path / "reads.fa")
    with open(reads, "w") as f:
        n = 0
        for seq in records[:2]:
            for at in range(0, len(seq) - 100 + 1, 10):
                f.write(">r%d\n%s\n" % (n, seq[at:at + 100]))
                n += 1
    r = subprocess.run([os.path.join(ROOT, "build", "ntsmCount"), "-s", sites, reads], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-500:]
    rows = {l.split("\t")[0]: [int(x) for x in l.split("\t")[1:]] for l in r.stdout.decode().splitlines() if not l.startswith("#")}
    in_file = set(l[1:].split()[0] for l in open(sites) if l.startswith(">"))
    assert set(rows) == in_file and len(rows) > 200
    # the last line for an ID decides; "." IDs are numbered
    last, counter = {}, 0
    for l in open(v):
        if l.startswith("#"):
            continue
        c, pos, rs, ref, alt = l.rstrip("\n").split("\t")[:5]
        if rs == ".":
            rs, counter = str(counter), counter + 1
        last[rs] = ref
    checked = 0
    for rs, row in rows.items():
        count_at, count_cg, sum_at, sum_cg = row[:4]
        if last[rs] in ("A", "T"):
            assert sum_at > 0 and count_at > 0, (rs, row)
            checked += 1
        else:
            assert sum_cg > 0 and count_cg > 0, (rs, row)
    assert checked > 50
    # ntsmVCF: a two-sample VCF over the first SNPs of the fixture
    multi = str(tmp_path / "multi.vcf")
    with open(multi, "w") as f:
        f.write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\ts1\ts2\n")
        done = 0
        for l in open(v):
            c = l.rstrip("\n").split("\t")
            if l.startswith("#") or c[2] not in rows or done >= 40:
                continue
            f.write("\t".join(c[:5] + [".", "PASS", ".", "GT", "0|1" if done % 2 else "1|1", "0|0"]) + "\n")
            done += 1
    r = subprocess.run([os.path.join(ROOT, "build", "ntsmVCF"), "-s", sites, "-r", g, "-p", str(tmp_path / "pca"), multi], capture_output=True,
                       timeout=600, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-500:]
    assert os.path.getsize(str(tmp_path / "pca_matrix.tsv")) > 0
