"""ntsmSiteGen -g: one-base gapped places counted beside the substitutions (include/ntsm_sitegen_gap_hip.h,
ntsm_amd/csrc/ntsm_sitegen_gap.hip, ntsm_amd/sitegen.py's GapSession, -g / -e of build/ntsmSiteGen).

The contract is the definition of G in the header; tests/sitegen_gap_restatement.cpp states it as a brute force on
strings ("naive") and in a faster form for dense sets ("neighbours").  CPU: answers that can be derived by hand pin the
restatement, the two forms agree, the program with -g -H reproduces the restatement's files, the refusals, the build.
GPU: the C ABI against the brute force value for value (k = 11 .. 31, three end margins, one piece and chunks around
k, a dense set, a genome longer than one staging buffer), and the program without -H."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_binding import ROOT  # noqa: E402

EXE = os.path.join(ROOT, "build", "ntsmSiteGen")
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
GAP_SYMBOLS = {"ntsm_sitegap_open", "ntsm_sitegap_submit", "ntsm_sitegap_hits", "ntsm_sitegap_stats", "ntsm_sitegap_close"}


def rc(s):
    return "".join(COMP[c] for c in reversed(s))


def compile_cpp(tmp_path_factory, name):
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-O2", "-std=c++11", "-o", exe, os.path.join(ROOT, "tests", name + ".cpp")], check=True)
    return exe


@pytest.fixture(scope="module")
def restatement(tmp_path_factory):
    return compile_cpp(tmp_path_factory, "sitegen_gap_restatement")


@pytest.fixture(scope="module")
def parent_restatement(tmp_path_factory):
    return compile_cpp(tmp_path_factory, "sitegen_restatement")


def write_fasta(path, records):
    with open(path, "w") as f:
        for i, seq in enumerate(records):
            f.write(">r%d\n%s\n" % (i, seq))


def brute(restatement, tmp_path, records, cands, k, e, method="naive", tag="b"):
    """(H, G) of the restatement, both clamped at 255"""
    fa, km = str(tmp_path / (tag + ".fa")), str(tmp_path / (tag + ".txt"))
    write_fasta(fa, records)
    open(km, "w").write("".join(c + "\n" for c in cands))
    r = subprocess.run([restatement, "hits", fa, km, str(k), str(e), method], capture_output=True, check=True, timeout=1800)
    both = np.array(r.stdout.split(), dtype=np.int64).reshape(-1, 2)
    return both[:, 0], both[:, 1]


def random_bases(rng, n):
    return "".join(rng.choice(list("ACGT"), size=n))


def inserted(rng, q, p):
    """q with one base put in before position p (0 .. k) that differs from both its neighbours: p is the only reading"""
    near = q[max(p - 1, 0):p + 1]
    return q[:p] + str(rng.choice([b for b in "ACGT" if b not in near])) + q[p:]


def removed(q, p):
    return q[:p] + q[p + 1:]


def no_two_alike(rng, k):
    """k random bases over ACG, no base equal to the one before it: removing base p is the only reading of the result, and
    a T put in is the only reading of that"""
    q = [str(rng.choice(list("ACG")))]
    while len(q) < k:
        q.append(str(rng.choice([b for b in "ACG" if b != q[-1]])))
    return "".join(q)


# ------------------------------------------------------------------------------------------------ CPU: the restatement
HAND_Q = no_two_alike(np.random.default_rng(19), 19)


@pytest.mark.parametrize("method", ["naive", "neighbours"])
@pytest.mark.parametrize("e", [1, 5, 9])
def test_answers_derived_by_hand(restatement, tmp_path, method, e):
    """k = 19.  A genome that is q with one base inserted before position p is a gapped place exactly for e <= p <= k - e, one
    that is q without base p exactly for e <= p <= k - 1 - e (5 .. 14 and 5 .. 13 at the default margin); the same on the
    reverse strand and in lower case; none with an N inside.  q has no T and no base twice in a row and the base put in is
    a T, so no other p and no shorter window of the genome can stand for the same place."""
    k, q = 19, HAND_Q
    for variant in ("forward", "reverse", "lower", "n_inside"):
        for kind, last in (("ins", k), ("del", k - 1)):
            records = []
            for p in range(last + 1):
                g = q[:p] + "T" + q[p:] if kind == "ins" else removed(q, p)
                if variant == "reverse":
                    g = rc(g)
                if variant == "lower":
                    g = g.lower()
                if variant == "n_inside":
                    g = g[:7] + "N" + g[8:]
                records.append(g)
            got = [int(brute(restatement, tmp_path, [g], [q], k, e, method)[1][0]) for g in records]
            hi = k - e if kind == "ins" else k - 1 - e
            want = [int(variant != "n_inside" and e <= p <= hi) for p in range(last + 1)]
            assert got == want, (variant, kind, got)


@pytest.mark.parametrize("method", ["naive", "neighbours"])
def test_a_gap_in_a_run_is_one_place(restatement, tmp_path, method):
    """q = X AAAA Y with the run across the A | B boundary (6 | 6 | 7 at k = 19) against X AAAAA Y: four positions
    qualify, the window counts once; the same for the run one base shorter"""
    k = 19
    x, y = "CGTCG", "CTGACTGTCA"
    q = x + "AAAA" + y
    assert len(q) == k and q[4] != "A" and q[9] != "A"
    for g in (x + "AAAAA" + y, x + "AAA" + y):
        h, gap = brute(restatement, tmp_path, [g], [q], k, 5, method)
        assert (int(h[0]), int(gap[0])) == (0, 1)
    # the stated consequence: a homopolymer suffix of e + 1 bases makes the k-mer's own place a gapped one as well
    tail = "GTCAGTCTGACGT" + "AAAAAA"
    h, gap = brute(restatement, tmp_path, ["C" + tail + "C"], [tail], k, 5, method)
    assert (int(h[0]), int(gap[0])) == (1, 1)


def planted(rng, n, k, e, n_cands):
    """(records, candidates): about n random bases in two records, a third record of gapped copies of the candidates, a
    record shorter than any window.  Copy i has one base put in or taken out at a position around the end margins and the
    part boundaries (a = b = k // 3), as it stands, on the reverse strand, in lower case, with an N inside, as a copy of
    the reverse complement, or as a run that is one base longer or shorter across a part boundary."""
    a = k // 3
    ps = sorted(set(p for p in (e - 1, e, a - 1, a, a + 1, 2 * a - 1, 2 * a, 2 * a + 1, k - e - 1, k - e, k - e + 1) if 0 <= p <= k))
    base = random_bases(rng, n)
    cands, extra = [], []
    for i in range(n_cands):
        p, ins, kind = ps[i % len(ps)], (i // len(ps)) % 2 == 0, (i // (2 * len(ps))) % 7
        at = int(rng.integers(0, n - k))
        q = base[at:at + k]
        if kind == 5:                                           # a run of four across A | B or B | C
            edge = a if i % 2 == 0 else 2 * a
            run = str(rng.choice(list("ACGT")))
            q = q[:edge - 2] + run * 4 + q[edge + 2:]
            piece = q[:edge - 2] + run * (5 if ins else 3) + q[edge + 2:]
        else:
            piece = inserted(rng, q, p) if ins else removed(q, min(p, k - 1))
        if kind == 1:
            piece = rc(piece)
        if kind == 2:
            piece = piece.lower()
        if kind == 3:
            piece = piece[:k // 2] + "N" + piece[k // 2 + 1:]
        if kind == 4:
            q = rc(q)
        if kind == 6:                                           # a substitution as well: neither H nor G
            o = int(rng.integers(0, len(piece)))
            piece = piece[:o] + str(rng.choice([b for b in "ACGT" if b != piece[o]])) + piece[o + 1:]
        cands.append(q)
        extra.append(piece + random_bases(rng, int(rng.integers(0, 5))))
        if kind == 0 and i % 3 == 0:                            # a second copy: G = 2
            extra.append(piece + "T")
    cut = n // 2 + 3
    return [base[:cut], base[cut:], "".join(extra), "ACGT"], cands


def saturating(rng, q):
    """300 gapped copies of q, a base between them"""
    return "T".join(inserted(rng, q, len(q) // 2) for _ in range(300))


@pytest.mark.parametrize("k,e", [(11, 5), (19, 1), (19, 5), (31, 5)])
def test_the_two_brute_forces_agree(restatement, tmp_path, k, e):
    rng = np.random.default_rng(200 + k + e)
    records, cands = planted(rng, 6000, k, e, 240)
    records.append(saturating(rng, cands[0]))
    cands += cands[:5]
    h1, g1 = brute(restatement, tmp_path, records, cands, k, e, "naive")
    h2, g2 = brute(restatement, tmp_path, records, cands, k, e, "neighbours")
    assert np.array_equal(h1, h2) and np.array_equal(g1, g2)
    assert g1.max() == 255 and (g1 == 0).any() and (g1 == 1).any() and (g1[g1 < 255] > 1).any()


# ------------------------------------------------------------------------------------------------ CPU: the program
K, W = 19, 31


def program_case(work):
    """a genome of 20 kb in chr1, 40 SNPs on it (REF on one side of A/T | C/G, ALT on the other), and in a second record,
    between stretches of N, a gapped copy of one reference sub-k-mer of every third SNP: (genome, vcf, planted ids)"""
    rng = np.random.default_rng(41)
    seq = random_bases(rng, 20000)
    lines, copies, planted_ids = [], [], []
    for i in range(40):
        while True:                                             # no run of four in either window: by the definition's stated
            pos = 300 + 480 * i + int(rng.integers(0, 300))    # consequence a k-mer that ends in a run loses itself (1-based)
            ref = seq[pos - 1]
            alt = str(rng.choice(list("CG" if ref in "AT" else "AT")))
            window = seq[pos - 1 - W // 2:pos + W // 2]
            if not re.search(r"(.)\1{3}", window) and not re.search(r"(.)\1{3}", window[:W // 2] + alt + window[W // 2 + 1:]):
                break
        lines.append("chr1\t%d\tsnp%02d\t%s\t%s" % (pos, i, ref, alt))
        if i % 3 == 0:
            start = pos - 1 - W // 2 + int(rng.integers(0, W - K + 1))
            sub = seq[start:start + K]
            p = int(rng.integers(5, K - 5))
            copies.append(inserted(rng, sub, p) if i % 2 else removed(sub, p))
            planted_ids.append("snp%02d" % i)
    g, v = os.path.join(work, "g.fa"), os.path.join(work, "s.vcf")
    open(g, "w").write(">chr1\n%s\n>copies\n%s\n" % (seq, "NNNN".join(copies)))
    open(v, "w").write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n" + "".join(l + "\n" for l in lines))
    return g, v, planted_ids


def run(args):
    return subprocess.run([EXE] + args, capture_output=True, timeout=900)


def outputs(prefix):
    return {n: open(prefix + n, "rb").read() for n in ["_subKmers.fa"] + ["_n%d.fa" % i for i in range(W - K + 1)]}


def ids_of(fa):
    return set(l[1:].split()[0] for l in fa.decode().splitlines() if l.startswith(">"))


@pytest.fixture(scope="module")
def program_inputs(restatement, parent_restatement, tmp_path_factory):
    """the case, and what the two restatements make of it: (genome, vcf, planted ids, prefix with gaps, prefix without)"""
    work = str(tmp_path_factory.mktemp("gapcase"))
    g, v, planted_ids = program_case(work)
    with_gaps, without = os.path.join(work, "rs_gap"), os.path.join(work, "rs_sub")
    r = subprocess.run([restatement, "all", g, v, with_gaps, str(K), str(W), "5", "0"], capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr[-300:]
    r2 = subprocess.run([parent_restatement, "all", g, v, without, str(K), str(W), "1", "0"], capture_output=True, timeout=900)
    assert r2.returncode == 0 and r2.stderr == r.stderr, r2.stderr[-300:]
    return g, v, planted_ids, with_gaps, without, r.stderr


def test_the_case_is_what_it_claims(program_inputs):
    """by the restatements alone: without gaps every SNP is in _n0.fa; with them exactly the planted ones are gone"""
    g, v, planted_ids, with_gaps, without, _ = program_inputs
    all_ids = set("snp%02d" % i for i in range(40))
    assert ids_of(outputs(without)["_n0.fa"]) == all_ids
    assert all_ids - ids_of(outputs(with_gaps)["_n0.fa"]) == set(planted_ids) and len(planted_ids) == 14
    assert outputs(with_gaps)["_subKmers.fa"] == outputs(without)["_subKmers.fa"]
    assert any(outputs(with_gaps)["_n%d.fa" % i] != outputs(without)["_n%d.fa" % i] for i in range(W - K + 1))


def test_program_with_gaps_and_a_hits_file(built, program_inputs, tmp_path):
    """-g -H with the restatement's counts (H + G): every file equal to the restatement's, in both spellings; without -g
    and with the substitution counts, the files the program wrote before it knew -g"""
    g, v, planted_ids, with_gaps, without, err = program_inputs
    want = outputs(with_gaps)
    p = str(tmp_path / "flags")
    r = run(["-r", g, "-v", v, "-p", p, "-g", "-H", with_gaps + "_subKmerHits.tsv"])
    assert r.returncode == 0 and r.stderr == err, r.stderr[-500:]
    assert outputs(p) == want and not os.path.exists(p + "_subKmerHits.tsv")
    p = str(tmp_path / "flags_e")
    r = run(["-g", "-e", "5", "-k", "19", "-w", "31", "-r", g, "-v", v, "-p", p, "-H", with_gaps + "_subKmerHits.tsv"])
    assert r.returncode == 0 and outputs(p) == want
    p = str(tmp_path / "upstream")
    r = run(["generate-sites", "name=" + p, "ref=" + g, "vcf=" + v, "gaps=1", "gapskip=5", "hits=" + with_gaps + "_subKmerHits.tsv"])
    assert r.returncode == 0 and r.stderr == err and outputs(p) == want, r.stderr[-500:]
    p = str(tmp_path / "plain")
    r = run(["-r", g, "-v", v, "-p", p, "-H", without + "_subKmerHits.tsv"])
    assert r.returncode == 0 and r.stderr == err and outputs(p) == outputs(without)
    assert all_lost(outputs(p), want) == set(planted_ids)
    p = str(tmp_path / "gaps0")
    r = run(["generate-sites", "name=" + p, "ref=" + g, "vcf=" + v, "gaps=0", "hits=" + without + "_subKmerHits.tsv"])
    assert r.returncode == 0 and outputs(p) == outputs(without)


def all_lost(before, after):
    return ids_of(before["_n0.fa"]) - ids_of(after["_n0.fa"])


REFUSALS = [
    ("gaps_without_substitutions", ["-g", "-x", "0"], b"Error: -g needs -x 1"),
    ("margin_without_gaps", ["-e", "3"], b"Error: -e needs -g"),
    ("margin_zero", ["-g", "-e", "0"], b"Error: e must be"),
    ("margin_too_wide", ["-g", "-e", "10", "-k", "19"], b"Error: e must be"),
    ("upstream_margin_without_gaps", None, b"Error: -e needs -g"),
    ("upstream_margin_too_wide", None, b"Error: e must be"),
]


@pytest.mark.parametrize("name,extra,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(built, program_inputs, tmp_path, name, extra, msg):
    """message on stderr, exit 1, no file written"""
    g, v, _, with_gaps, _, _ = program_inputs
    out = tmp_path / "out"
    out.mkdir()
    hits = with_gaps + "_subKmerHits.tsv"
    if extra is not None:
        r = run(["-r", g, "-v", v, "-p", str(out / "p"), "-H", hits] + extra)
    else:
        more = ["gapskip=3"] if name == "upstream_margin_without_gaps" else ["gaps=1", "gapskip=10"]
        r = run(["generate-sites", "name=" + str(out / "p"), "ref=" + g, "vcf=" + v, "hits=" + hits] + more)
    assert r.returncode == 1 and r.stderr.startswith(msg) and r.stderr.count(b"Error: ") == 1, r.stderr[-300:]
    assert os.listdir(str(out)) == []


def test_usage_names_the_new_flags(built):
    r = run(["-h"])
    assert r.returncode == 0 and all(s in r.stderr for s in (b"-g ", b"-e ", b"gaps=1", b"gapskip="))


# ------------------------------------------------------------------------------------------------ CPU: the build
def exported(lib):
    syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "ntsm_amd", lib)], capture_output=True, check=True)
    names = set(l.split()[-1] for l in syms.stdout.decode().splitlines() if l.split()[-2] in "TtDdBb")
    return set(n for n in names if not n.startswith("__hip_"))


def test_gap_library_builds_clean_and_exports_its_five_names(built, tmp_path):
    src = os.path.join(ROOT, "ntsm_amd", "csrc", "ntsm_sitegen_gap.hip")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Werror", "-fvisibility=hidden"]
    r = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-c", "-o", str(tmp_path / "both.o"), src], capture_output=True)
    assert r.returncode == 0 and r.stderr == b"", r.stderr[-2000:]
    assert exported("libntsm_sitegen_gap_hip.so") == GAP_SYMBOLS
    assert exported("libntsm_sitegen_hip.so") == {"ntsm_sitegen_open", "ntsm_sitegen_submit", "ntsm_sitegen_hits", "ntsm_sitegen_times_get",
                                                  "ntsm_sitegen_close"}


def test_python_module_loads_the_gap_library_on_first_use(built):
    """import ntsm_amd.sitegen must go on working where only the first library has been built"""
    code = ("import sys, ctypes; sys.path.insert(0, %r); import ntsm_amd.sitegen as S; "
            "assert S._gap is None and hasattr(S, 'GapSession'); "
            "lib = S.gap_lib(); assert S._gap is lib and isinstance(lib, ctypes.CDLL) and lib.ntsm_sitegap_open" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True)
    assert r.returncode == 0, r.stderr[-500:]


# ------------------------------------------------------------------------------------------------ GPU: the C ABI
def window_counts(records, k):
    runs = [len(w) for r in records for w in re.split("[^ACGTacgt]+", r)]
    return tuple(sum(n - m + 1 for n in runs if n >= m) for m in (k, k + 1, k - 1))


def gap_hits(cands, k, e, records, chunk=None):
    import ntsm_amd.sitegen as S
    with S.GapSession(cands, k, e) as s:
        s.submit_records(records, chunk)
        sub, gap = s.hits()
        return sub.astype(np.int64), gap.astype(np.int64), s.stats()


@pytest.mark.gpu
@pytest.mark.parametrize("k,e", [(11, 5), (13, 5), (19, 5), (25, 5), (31, 5), (19, 1), (19, 9)])
def test_device_counts_on_generated_genomes(built, restatement, tmp_path, k, e):
    """G equal to the definition's brute force and H to the first library's x = 1 count, in one piece and in chunks just
    below, at and above k, of 37 and of 4096 bytes; the three window counts as a split of the records gives them"""
    import ntsm_amd.sitegen as S
    rng = np.random.default_rng(3000 + 10 * k + e)
    records, cands = planted(rng, 30000, k, e, 600)
    records.append(saturating(rng, cands[1]))
    cands += cands[:7]                                            # duplicate candidates: each its own count
    want_sub, want_gap = brute(restatement, tmp_path, records, cands, k, e)
    with S.Session(cands, k, 1) as first:
        first.submit_records(records)
        first_sub = first.hits().astype(np.int64)
    assert np.array_equal(first_sub, want_sub)
    assert want_gap.max() == 255 and (want_gap == 0).any() and (want_gap == 1).any() and (want_gap[want_gap < 255] > 1).any()
    for chunk in (None, k - 2, k - 1, k, k + 1, 37, 4096):
        sub, gap, st = gap_hits(cands, k, e, records, chunk)
        assert np.array_equal(gap, want_gap), (chunk, [(int(c), cands[c], int(gap[c]), int(want_gap[c])) for c in np.flatnonzero(gap != want_gap)[:10]])
        assert np.array_equal(sub, first_sub), (chunk, np.flatnonzero(sub != first_sub)[:10])
        assert (st.windows, st.windows_long, st.windows_short) == window_counts(records, k), chunk
        assert st.probes > 0
        assert np.array_equal(gap[:7], gap[-7:])


@pytest.mark.gpu
def test_device_counts_on_a_dense_candidate_set(built, restatement, tmp_path):
    """2 * 10^5 candidates from a 1 Mb genome with a repeat family; a quarter of them are a genome window of k + 1 bases
    less an interior base, or one of k - 1 bases with a base put in"""
    rng = np.random.default_rng(78)
    k, e, n = 19, 5, 1000000
    codes = rng.integers(0, 4, size=n)
    fam = codes[5000:5300].copy()
    for at in rng.integers(10000, n - 400, size=200):
        codes[at:at + 300] = np.where(rng.random(300) < 0.03, rng.integers(0, 4, size=300), fam)
    base = np.array(list("ACGT"))[codes]
    base[rng.integers(0, n, size=50)] = "N"
    genome = "".join(base)
    starts = rng.integers(0, n - k - 1, size=200000)
    cands = []
    for i, at in enumerate(starts):
        p = int(rng.integers(1, k - 1))
        if i % 8 == 1:
            q = removed(genome[at:at + k + 1].replace("N", "A"), p)
        elif i % 8 == 5:
            q = genome[at:at + k - 1].replace("N", "A")
            q = q[:p] + "ACGT"[i % 4] + q[p:]
        else:
            q = genome[at:at + k].replace("N", "A")
        if i % 4 == 2:
            q = rc(q)
        if i % 16 == 3:
            q = random_bases(rng, k)
        cands.append(q)
    records = [genome[:400000], genome[400000:]]
    want_sub, want_gap = brute(restatement, tmp_path, records, cands, k, e, "neighbours", tag="dense")
    assert (want_gap > 0).sum() > 1000 and (want_gap == 0).sum() > 1000
    sub, gap, st = gap_hits(cands, k, e, records)
    print("dense: %d windows, %d probes, kernel %.3f ms" % (st.windows, st.probes, st.kernel_ms))
    assert np.array_equal(gap, want_gap), np.flatnonzero(gap != want_gap)[:10]
    assert np.array_equal(sub, want_sub), np.flatnonzero(sub != want_sub)[:10]
    sub, gap, _ = gap_hits(cands, k, e, records, 65536)
    assert np.array_equal(gap, want_gap) and np.array_equal(sub, want_sub)


STAGE = 1 << 27                                                # kStageCap of ntsm_sitegen_gap.hip: bytes per full launch


@pytest.mark.gpu
def test_device_counts_across_a_full_staging_buffer(built, restatement, tmp_path):
    """2^27 + 5000 bytes of N with islands of random bases through one submit call: the first launch is full and hands its
    last k bytes to the second.  One island holds a gapped copy of its own start that straddles byte 2^27; one starts at
    2^27 - k, so that its part before the seam is exactly the carry and its first windows of k and k - 1 bases lie wholly
    inside it; one is cut into two records at 2^27 - 1, and the long window that would bridge the separator is a gapped
    place of a candidate that must read 0.  Expected: the brute force on the islands alone (no window crosses an N)."""
    import ntsm_amd.sitegen as S
    k, e = 19, 5
    rng = np.random.default_rng(2027)
    total = STAGE + 5000

    def run_case(spans, islands, ends, extra_cands):
        text = np.full(total, ord("N"), dtype=np.uint8)
        for (a, b), isl in zip(spans, islands):
            assert b - a == len(isl)
            text[a:b] = np.frombuffer(isl.encode(), dtype=np.uint8)
        cands = [isl[at:at + k] for isl in islands[1:-1] for at in range(len(isl) - k + 1)] + extra_cands
        want_sub, want_gap = brute(restatement, tmp_path, islands, cands, k, e)
        with S.GapSession(cands, k, e) as sess:
            sess.submit(text, ends)
            sub, gap = sess.hits()
            st = sess.stats()
        assert (st.full_launches, st.launches) == (1, 2)
        assert (st.windows, st.windows_long, st.windows_short) == window_counts(islands, k)
        assert np.array_equal(gap.astype(np.int64), want_gap), [(int(c), cands[c], int(gap[c]), int(want_gap[c])) for c in np.flatnonzero(gap != want_gap)[:10]]
        assert np.array_equal(sub.astype(np.int64), want_sub)
        return want_gap, len(cands) - len(extra_cands)

    head, tail = random_bases(rng, 300), random_bases(rng, 400)
    # 1: a gapped copy across the seam, and the island whose run-up is the carry
    src = random_bases(rng, 120)
    copy = src[:k]
    straddle = src + "".join(inserted(rng, copy, p) + removed(copy, p) for p in (5, 9, 13))
    straddle = straddle + random_bases(rng, 10)
    a0 = STAGE - 120 - 27                                       # the second gapped copy lies across byte 2^27
    in_carry = random_bases(rng, 300)
    spans = [(5, 305), (a0, a0 + len(straddle)), (total - 400, total)]
    want_gap, _ = run_case(spans, [head, straddle, tail], [total], [])
    assert want_gap[0] >= 6
    spans = [(5, 305), (STAGE - k, STAGE - k + 300), (total - 400, total)]
    run_case(spans, [head, in_carry, tail], [total], [])
    # 2: one island cut into two records at 2^27 - 1: its two sides are islands of their own for the brute force
    left, right = random_bases(rng, 150), random_bases(rng, 150)
    bridge = left[-9:] + right[:k + 1 - 9]                      # the long window a scan without the separator would see
    bridged = [removed(bridge, 9), rc(removed(bridge, 9))]
    spans = [(5, 305), (STAGE - 151, STAGE - 1), (STAGE - 1, STAGE + 149), (total - 400, total)]
    want_gap, cut = run_case(spans, [head, left, right, tail], [STAGE - 1, total], bridged)
    assert (want_gap[cut:] == 0).all()


@pytest.mark.gpu
def test_device_empty_candidate_list_and_bad_arguments(built):
    import ctypes as C
    import ntsm_amd.sitegen as S
    sub, gap, st = gap_hits([], 19, 5, ["ACGT" * 100])
    assert len(sub) == 0 and len(gap) == 0 and (st.windows, st.windows_long, st.windows_short, st.probes) == (382, 381, 383, 0)
    lib = S.gap_lib()
    h = C.c_void_p()
    one = np.array([5], dtype=np.uint64)
    for k, e in ((10, 3), (32, 5), (19, 0), (19, 10), (11, 6)):
        assert lib.ntsm_sitegap_open(0, k, e, 1, one.ctypes.data, C.byref(h)) == -1, (k, e)
    assert lib.ntsm_sitegap_open(0, 11, 5, 1, np.array([1 << 22], dtype=np.uint64).ctypes.data, C.byref(h)) == -1
    assert lib.ntsm_sitegap_open(0, 19, 5, 1, None, C.byref(h)) == -1
    with S.GapSession(["A" * 19], 19, 5) as s:
        ends = np.array([5, 3], dtype=np.uint64)
        assert lib.ntsm_sitegap_submit(s._h, b"ACGTACGT", 8, ends.ctypes.data, 2) == -1
        ends = np.array([9], dtype=np.uint64)
        assert lib.ntsm_sitegap_submit(s._h, b"ACGTACGT", 8, ends.ctypes.data, 1) == -1


# ------------------------------------------------------------------------------------------------ GPU: the program
@pytest.mark.gpu
def test_program_on_the_device(built, program_inputs, tmp_path):
    """-g without -H: every file equal to the restatement's; its hits file fed back through -H gives the same files; the
    most permissive sites file loads in ntsmCount"""
    g, v, planted_ids, with_gaps, without, err = program_inputs
    p, q = str(tmp_path / "dev"), str(tmp_path / "fed")
    r = run(["-r", g, "-v", v, "-p", p, "-g", "-V"])
    assert r.returncode == 0, r.stderr[-500:]
    kept = b"".join(l for l in r.stderr.splitlines(True) if not l.startswith((b"Time: ", b"Device: ")))
    assert kept == err and b"Device: " in r.stderr and b"of k + 1 bases" in r.stderr
    assert outputs(p) == outputs(with_gaps)
    assert open(p + "_subKmerHits.tsv", "rb").read() == open(with_gaps + "_subKmerHits.tsv", "rb").read()
    r = run(["-r", g, "-v", v, "-p", q, "-g", "-H", p + "_subKmerHits.tsv"])
    assert r.returncode == 0 and outputs(q) == outputs(with_gaps)
    p2 = str(tmp_path / "up")
    r = run(["generate-sites", "name=" + p2, "ref=" + g, "vcf=" + v, "gaps=1", "gapskip=5"])
    assert r.returncode == 0 and outputs(p2) == outputs(with_gaps)
    p3 = str(tmp_path / "sub")
    r = run(["-r", g, "-v", v, "-p", p3])
    assert r.returncode == 0 and outputs(p3) == outputs(without)
    sites = p + "_n%d.fa" % (W - K)
    reads = str(tmp_path / "reads.fa")
    seq = open(g).read().split("\n")[1]
    with open(reads, "w") as f:
        for n, at in enumerate(range(0, len(seq) - 100 + 1, 10)):
            f.write(">r%d\n%s\n" % (n, seq[at:at + 100]))
    r = subprocess.run([os.path.join(ROOT, "build", "ntsmCount"), "-s", sites, reads], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-500:]
    rows = set(l.split("\t")[0] for l in r.stdout.decode().splitlines() if not l.startswith("#"))
    assert rows == ids_of(open(sites, "rb").read()) and len(rows) == 40
