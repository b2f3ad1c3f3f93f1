"""ntsmVCF --counts DIR / --store STORE (ntsm_amd/csrc/host/ntsm_vcf_main.cpp) and their device step ntsm_vcf_records
(include/ntsm_vcf_hip.h, ntsm_amd/csrc/ntsm_vcf.hip, ntsm_amd/vcf.py: records).

The contract is the reference's VCFConvert::outputCounts (src/VCFConvert.hpp:176-187, MultiCount::printCountsMax,
src/MultiCount.hpp:93-138) after count(): tests/golden/vcf_counts/ holds its recordings for the cases of
tests/golden/vcf/ (README there), and counts_model below restates count + printCountsMax from the reference text, with
canonical k-mer strings in place of hashes.  CPU: the model reproduces every recording; the whole program --
ntsm_vcf_main.cpp built against tests/vcf_step_standin.cpp and tests/vcf_records_standin.cpp under ASan + UBSan, run
directly -- gives the recordings, equals the model on seeded cohorts for every -t and window size, writes the store that
ntsmEval --pack makes of its counts files, and refuses what it must.  GPU: ntsm_vcf_records against a numpy model at every
launch edge, the CLI against the recordings and against --pack, and the chain into ntsmEval --against."""
import os
import re
import subprocess
import urllib.parse

import numpy as np
import pytest

from oracle_binding import ROOT
from test_vcf import CASES, EVAL, GOLD, VCF, cohort, numpy_model, refusal_inputs, site_of, strip_time, write_case

RECORDED = os.path.join(ROOT, "tests", "golden", "vcf_counts")
HEADER = b"\n#locusID\tcountAT\tcountCG\tsumAT\tsumCG\tdistinctAT\tdistinctCG\n"
WITH_SAMPLES = [c for c in CASES if c["name"] != "zero_samples"]


def recorded_name(sample):
    """the file of tests/golden/vcf_counts/<case>/ that holds SAMPLE.counts.txt (README there: percent-encoded)"""
    return urllib.parse.quote_from_bytes(sample + b".counts.txt", safe="")


# ------------------------------------------------------------------------------------------ the restatement
def read_fasta(path):
    """name = header up to the first white space, sequence = the lines up to the next '>' (kseq)"""
    out = []
    for line in open(path, "rb").read().split(b"\n"):
        if line[:1] == b">":
            out.append([line[1:].split()[0] if line[1:].split() else b"", b""])
        elif out:
            out[-1][1] += line.rstrip(b"\r")
    return [(n.decode("latin-1"), s.decode("latin-1")) for n, s in out]


COMP = str.maketrans("ACGT", "TGCA")


def kmers(s, k):
    """vendor/KseqHashIterator.hpp: the k-mers of s in position order, ACGT in either case (U as T), anything else
    restarts; a k-mer is the smaller of its forward and reverse-complement spelling"""
    s = s.upper().replace("U", "T")
    out = []
    for i in range(len(s) - k + 1):
        w = s[i:i + k]
        if all(c in "ACGT" for c in w):
            out.append(min(w, w.translate(COMP)[::-1]))
    return out


def counts_model(sites_fa, genome_fa, vcf, k=19, window=31, multi=20, dupes=False):
    """VCFConvert::count (one thread) and MultiCount::printCountsMax per sample.  Returns ([sample name bytes], [the
    bytes of SAMPLE.counts.txt]).  Raises KeyError where the reference throws (a shared k-mer without -d)."""
    column, shared, ids, ref_list, var_list = {}, set(), [], [], []
    for r, (name, seq) in enumerate(read_fasta(sites_fa)):              # MultiCount::initCountsHash
        lst = []
        (ref_list if r % 2 == 0 else var_list).append(lst)
        for km in kmers(seq, k):
            if km in column:
                shared.add(km)
            else:
                lst.append(km)
                column[km] = len(column)
        if r % 2 == 0:
            ids.append(name)
    if not dupes:
        for km in shared:
            del column[km]
    genome = dict(read_fasta(genome_fa))                                # a later record of a name wins
    lines = open(vcf, "rb").read().split(b"\n")
    complete, at, samples = lines[:-1], 0, []                           # a last line without '\n' is not read
    for at, line in enumerate(complete):
        f = line.split(b"\t")
        if f[0] == b"#CHROM":
            samples = f[9:]
            if samples and samples[-1] == b"":                          # getline reads no empty last field
                samples.pop()
            break
    n = len(samples)
    state = {km: np.zeros(n, dtype=np.uint8) for km in column}
    m1, m2 = multi & 0xFFFFFFFF, (2 * multi) & 0xFFFFFFFF
    for line in complete[at + 1:]:
        f = line.decode("latin-1").split("\t")
        field = lambda i: f[min(i, len(f) - 1)]                         # noqa: E731  (a used-up stream keeps its last item)
        pos = int(field(1))
        if field(3) == "." or len(field(4)) != 1:
            continue
        chrom = genome[field(0)]
        ref_win = chrom[pos - window // 2 - 1:][:window]                # cut at the chromosome's end
        var_win = ref_win[:window // 2] + field(4) + ref_win[window // 2 + 1:] if len(ref_win) >= window // 2 else ref_win
        g = np.array([1 if x in ("0|1", "1|0") else 2 if x == "1|1" else 0 for x in (f[9:9 + n] + [""] * n)[:n]], dtype=np.int64)
        for win, full in ((ref_win, 0), (var_win, 2)):
            for km in kmers(win, k):
                if km not in column:
                    continue                                            # insertCount: not a key, nothing happens
                st = state[km]
                fresh = ((g == full) | (g == 1)) & (st == 0)            # a non-zero byte is kept
                st[fresh] = (np.where(g == full, m2, m1)[fresh] & 255).astype(np.uint8)
    texts = []
    for j in range(n):                                                  # printCountsMax(j, out)
        out = [HEADER]
        for i, rs in enumerate(ids):
            a = [int(state[km][j]) for km in ref_list[i]]               # KeyError: m_kmerToHash.at throws
            b = [int(state[km][j]) for km in var_list[i]]
            out.append(("%s\t%d\t%d\t%d\t%d\t%d\t%d\n" % (rs, max(a, default=0), max(b, default=0), sum(a), sum(b), len(a), len(b))).encode("latin-1"))
        texts.append(b"".join(out))
    return samples, texts


def case_flags(args):
    kw, it = {}, iter(args)
    for a in it:
        if a == "-d":
            kw["dupes"] = True
        else:
            kw[{"-k": "k", "-w": "window", "-m": "multi"}[a]] = int(next(it))
    return kw


def recordings(case):
    d = os.path.join(RECORDED, case["name"])
    return {f: open(os.path.join(d, f), "rb").read() for f in sorted(os.listdir(d))}


def test_restatement_reproduces_every_recording():
    """counts_model gives, for every sample of the 13 cases with samples, the bytes the reference recorded; the
    zero-sample case has no recording and the model writes none."""
    assert len(WITH_SAMPLES) == 13 and not os.path.exists(os.path.join(RECORDED, "zero_samples"))
    for case in CASES:
        d = os.path.join(GOLD, case["name"])
        samples, texts = counts_model(os.path.join(d, "sites.fa"), os.path.join(d, "genome.fa"), os.path.join(d, "in.vcf"), **case_flags(case["args"]))
        if case["name"] == "zero_samples":
            assert samples == [] and texts == []
            continue
        assert {recorded_name(s): t for s, t in zip(samples, texts)} == recordings(case), case


# ------------------------------------------------------------------------------ the whole program on the CPU
@pytest.fixture(scope="module")
def cpu_programs(tmp_path_factory):
    """ntsm_vcf_main.cpp + the Makefile's $(VCFSRC) + tests/vcf_step_standin.cpp under ASan + UBSan, linked twice: with
    tests/vcf_records_standin.cpp (ntsm_vcf_records in plain C++) and without it (the weak reference stays null).  Both
    are programs of their own: run directly, nothing preloaded."""
    mk = open(os.path.join(ROOT, "Makefile")).read()
    vcfsrc = re.search(r"^VCFSRC := ((?:.*\\\n)*.*)$", mk, re.M).group(1).replace("\\\n", " ").split()
    host = os.path.join(ROOT, "ntsm_amd", "csrc", "host")
    src = [os.path.join(host, "ntsm_vcf_main.cpp")] + [f.replace("$(HOST)", host) for f in vcfsrc]
    src += [os.path.join(ROOT, "tests", "vcf_step_standin.cpp"), os.path.join(ROOT, "tests", "vcf_records_standin.cpp")]
    d = tmp_path_factory.mktemp("vccpu")
    flags = ["-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-ffp-contract=off"]
    objs = [str(d / (os.path.basename(f) + ".o")) for f in src]
    jobs = [subprocess.Popen(["g++"] + flags + ["-c", f, "-o", o]) for f, o in zip(src, objs)]
    assert all(j.wait() == 0 for j in jobs)
    with_step, without = str(d / "ntsmVCF_cpu"), str(d / "ntsmVCF_cpu_no_records")
    subprocess.run(["g++"] + flags + ["-o", with_step] + objs + ["-lz", "-pthread"], check=True)
    subprocess.run(["g++"] + flags + ["-o", without] + objs[:-1] + ["-lz", "-pthread"], check=True)
    return with_step, without


def run_cpu(exe, args, cwd, env=None):
    """(exit status, stderr without the Time line); no sanitizer report"""
    p = subprocess.run([exe] + args, cwd=str(cwd), capture_output=True, timeout=600, env=dict(os.environ, **(env or {})))
    assert b"Sanitizer" not in p.stderr and b"runtime error" not in p.stderr, p.stderr[-3000:].decode(errors="replace")
    return p.returncode, strip_time(p.stderr)


def dir_bytes(d):
    return {f: open(os.path.join(str(d), f), "rb").read() for f in sorted(os.listdir(str(d)))}


def check_recordings(exe, tmp_path, run):
    for case in WITH_SAMPLES:
        d = os.path.join(GOLD, case["name"])
        out = tmp_path / case["name"]
        out.mkdir()
        rc, err = run(exe, ["-s", "sites.fa", "-r", "genome.fa"] + case["args"] + ["--counts", str(out), "in.vcf"], d)
        assert rc == 0, (case, err)
        assert {urllib.parse.quote(f, safe=""): b for f, b in dir_bytes(out).items()} == recordings(case), case
        assert err == open(os.path.join(d, "expected_stderr.txt"), "rb").read(), case      # stderr is -p's


def test_cpu_program_gives_the_recordings(cpu_programs, tmp_path):
    check_recordings(cpu_programs[0], tmp_path, run_cpu)


@pytest.fixture(scope="module")
def seeded(tmp_path_factory):
    """the two dense cohorts of tests/test_vcf.py and what counts_model says of them"""
    out = {}
    for n_samples, n_snps, seed in ((7, 60, 46), (33, 120, 32)):
        d = tmp_path_factory.mktemp("c%d" % n_samples)
        g, s, v = cohort(d, np.random.default_rng(seed), n_samples, n_snps)
        samples, texts = counts_model(s, g, v, dupes=True)
        assert len(samples) == n_samples and all(t.count(b"\n") == n_snps + 2 for t in texts)
        out[n_samples] = (d, g, s, v, {sm.decode() + ".counts.txt": t for sm, t in zip(samples, texts)})
    return out


@pytest.mark.parametrize("n_samples", [7, 33])
def test_cpu_program_matches_restatement_for_every_t_and_window(cpu_programs, seeded, tmp_path, n_samples):
    """--counts on the dense seeded cohorts under -t 1, -t 5 and -t 64, with the default window and with
    NTSM_VCF_STORE_WINDOW=16 (33 samples: windows of 16, 16 and 1): the model's bytes every time."""
    d, g, s, v, want = seeded[n_samples]
    for t in ("1", "5", "64"):
        for window in (None, "16"):
            out = tmp_path / ("t%s_w%s" % (t, window))
            out.mkdir()
            rc, err = run_cpu(cpu_programs[0], ["-s", s, "-r", g, "-d", "-t", t, "--counts", str(out), v], d,
                              env={"NTSM_VCF_STORE_WINDOW": window} if window else None)
            assert rc == 0, err[-500:]
            assert dir_bytes(out) == want, (t, window)


def pack(store, files, cwd):
    p = subprocess.run([EVAL, "--pack", store] + files, cwd=str(cwd), capture_output=True)
    assert p.returncode == 0, p.stderr[-500:]
    return open(os.path.join(str(cwd), store), "rb").read()


def records_of(store_bytes):
    """(head of the file, [(scalars, name field, counts bytes)]) by the layout of eval_store.hpp"""
    m, n, first, stride = np.frombuffer(store_bytes, dtype="<u4", count=1, offset=12)[0], *np.frombuffer(store_bytes, dtype="<u8", count=3, offset=16)
    assert stride == 1056 + 8 * m and len(store_bytes) == first + n * stride
    recs = [store_bytes[int(first + r * stride):int(first + (r + 1) * stride)] for r in range(int(n))]
    return store_bytes[:int(first)], [(r[:32], r[32:1056], r[1056:]) for r in recs]


def renamed_samples(vcf, out, prefix):
    """the same VCF with the samples S<i> of its header called <prefix><i>"""
    lines = open(vcf).read().split("\n")
    i = next(i for i, l in enumerate(lines) if l.startswith("#CHROM"))
    lines[i] = re.sub(r"\tS(\d+)", lambda mo: "\t%s%s" % (prefix, mo.group(1)), lines[i])
    open(out, "w", newline="").write("\n".join(lines))
    return out


def check_store_against_pack(exe, run, built, seeded, tmp_path):
    """--counts DIR --store S in three windows = ntsmEval --pack of DIR's files in header order, byte for byte; --store
    alone differs only in the name fields, which hold the sample IDs; a second VCF's samples appended = --pack of both"""
    d, g, s, v, want = seeded[33]
    env = {"NTSM_VCF_STORE_WINDOW": "16"}
    os.mkdir(str(tmp_path / "DIR"))
    rc, err = run(exe, ["-s", s, "-r", g, "-d", "-t", "3", "--counts", "DIR", "--store", "both.store", v], tmp_path, env=env)
    assert rc == 0 and dir_bytes(tmp_path / "DIR") == want and not os.path.exists(str(tmp_path / "both.store.tmp")), err[-500:]
    files = ["DIR/S%d.counts.txt" % i for i in range(33)]
    both = open(str(tmp_path / "both.store"), "rb").read()
    assert both == pack("pack.store", files, tmp_path)
    rc, err = run(exe, ["-s", s, "-r", g, "-d", "--store", "alone.store", v], tmp_path)      # the default window: one call
    assert rc == 0, err[-500:]
    head_a, recs_a = records_of(open(str(tmp_path / "alone.store"), "rb").read())
    head_b, recs_b = records_of(both)
    assert head_a == head_b and len(recs_a) == 33
    for i, (a, b) in enumerate(zip(recs_a, recs_b)):
        assert a[0] == b[0] and a[2] == b[2] and a[1] == b"S%d" % i + bytes(1024 - len(b"S%d" % i)), i
        assert b[1].rstrip(b"\0") == files[i].encode()
    v2 = renamed_samples(v, str(tmp_path / "second.vcf"), "T")
    rc, err = run(exe, ["-s", s, "-r", g, "-d", "--counts", "DIR", "--store", "both.store", v2], tmp_path, env=env)
    assert rc == 0, err[-500:]
    assert open(str(tmp_path / "both.store"), "rb").read() == pack("pack.store", ["DIR/T%d.counts.txt" % i for i in range(33)], tmp_path)
    assert len(open(str(tmp_path / "both.store"), "rb").read()) == len(both) + 33 * (1056 + 8 * 120)


def test_cpu_program_store_equals_pack(cpu_programs, built, seeded, tmp_path):
    check_store_against_pack(cpu_programs[0], run_cpu, built, seeded, tmp_path)


def test_cpu_program_with_p_still_writes_the_fixtures(cpu_programs, tmp_path):
    """-p together with --counts and --store: matrix, centre file and stderr are the fixtures' bytes, the counts the
    recordings"""
    case = next(c for c in CASES if c["name"] == "overlap_dupes")
    d = os.path.join(GOLD, case["name"])
    out = tmp_path / "DIR"
    out.mkdir()
    prefix = str(tmp_path / "m")
    rc, err = run_cpu(cpu_programs[0], ["-s", "sites.fa", "-r", "genome.fa"] + case["args"] +
                      ["-p", prefix, "--counts", str(out), "--store", str(tmp_path / "s.store"), "in.vcf"], d)
    assert rc == 0 and err == open(os.path.join(d, "expected_stderr.txt"), "rb").read()
    assert open(prefix + "_matrix.tsv", "rb").read() == open(os.path.join(d, "expected_matrix.tsv"), "rb").read()
    assert open(prefix + "_center.txt", "rb").read() == open(os.path.join(d, "expected_center.txt"), "rb").read()
    assert dir_bytes(out) == recordings(case) and os.path.getsize(str(tmp_path / "s.store")) > 6 * 1056


REFUSALS = [
    # (name, flags beside -s -r VCF, message fragment)
    ("shared_without_d", ["--counts", "DIR"], "--counts / --store need -d"),
    ("shared_without_d_p", ["-p", "m", "--store", "S"], "-p needs -d"),
    ("zero_samples", ["--counts", "DIR", "--store", "S"], "has no samples"),
    ("slash_in_sample", ["--counts", "DIR"], "cannot name a counts file"),
    ("empty_sample", ["--counts", "DIR"], "cannot name a counts file"),
    ("long_name", ["--store", "S"], "a store holds names of at most 1023"),
    ("long_path", ["--counts", "DIR"], "a store holds names of at most 1023"),
    ("same_sample_twice", ["--store", "S"], "two samples are named S1"),
    ("name_in_store", ["--store", "S"], "the name S0 is already in the store"),
    ("path_in_store", ["--counts", "DIR", "--store", "S"], "the name DIR/S0.counts.txt is already in the store"),
    ("locus_twice", ["--store", "S"], "the locus ID rsA twice"),
    ("other_loci", ["--store", "S"], "(IDs and distinct columns) are not those of"),
    ("other_distinct", ["--store", "S", "-k", "17", "-d"], "(IDs and distinct columns) are not those of"),
    ("no_dir", ["--counts", "NODIR", "--store", "S"], "NODIR is not a directory"),
    ("file_is_directory", ["--counts", "DIR", "--store", "S"], "cannot write DIR/S1.counts.txt"),
    ("not_a_store", ["--store", "S"], "is not a cohort store"),
]


@pytest.mark.parametrize("name,flags,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(cpu_programs, tmp_path, name, flags, msg):
    """'Error: ...' as the last line, exit status 1, no file written (DIR stays empty, no new store, no STORE.tmp, no -p
    file) and a store that was there keeps its bytes."""
    rng = np.random.default_rng(3)
    genome, sites, line = refusal_inputs(tmp_path, rng)
    samples, lines = ["S0", "S1"], [line("100"), line("200")]
    os.mkdir(str(tmp_path / "DIR"))
    store = str(tmp_path / "S")
    if name in ("name_in_store", "path_in_store", "other_loci", "other_distinct", "file_is_directory", "no_dir"):    # a store to keep
        g, s, v = write_case(tmp_path, genome, sites, ["A0", "S0"] if name == "name_in_store" else ["A0", "A1"], lines)
        assert run_cpu(cpu_programs[0], ["-s", s, "-r", g, "--store", store, v], tmp_path)[0] == 0
    if name == "path_in_store":
        g, s, v = write_case(tmp_path, genome, sites, ["S0"], [l[:-1] for l in lines])
        assert run_cpu(cpu_programs[0], ["-s", s, "-r", g, "--counts", "DIR", "--store", store, v], tmp_path)[0] == 0
    if name == "not_a_store":
        open(store, "wb").write(b"NTSMCOH0" + bytes(100))
    if name.startswith("shared_without_d"):
        sites = sites + [site_of(genome[0][1], 105, rs="rsC")]
    elif name == "zero_samples":
        samples, lines = [], [l[:-2] for l in lines]
    elif name == "slash_in_sample":
        samples = ["S0", "a/b"]
    elif name == "empty_sample":
        samples, lines = ["S0", "", "S2"], [l + ["0|0"] for l in lines]
    elif name == "long_name":
        samples = ["S0", "L" * 1024]
    elif name == "long_path":
        samples = ["S0", "L" * (1024 - len("DIR/.counts.txt"))]
    elif name == "same_sample_twice":
        samples, lines = ["S0", "S1", "S1"], [l + ["0|0"] for l in lines]
    elif name == "locus_twice":
        sites = sites + [site_of(genome[0][1], 250, rs="rsA")]
    elif name == "other_loci":
        sites = [sites[0], site_of(genome[0][1], 200, rs="rsZ")]
    elif name == "file_is_directory":
        os.mkdir(str(tmp_path / "DIR" / "S1.counts.txt"))
    before = {f: (open(os.path.join(str(tmp_path), f), "rb").read() if os.path.isfile(os.path.join(str(tmp_path), f)) else None)
              for f in os.listdir(str(tmp_path))}
    in_dir = sorted(os.listdir(str(tmp_path / "DIR")))
    g, s, v = write_case(tmp_path, genome, sites, samples, lines)
    rc, err = run_cpu(cpu_programs[0], ["-s", s, "-r", g] + flags + [v], tmp_path)
    assert rc == 1, (name, err)
    assert err.splitlines()[-1].startswith(b"Error: ") and msg.encode() in err.splitlines()[-1], (name, err)
    after = {f: (open(os.path.join(str(tmp_path), f), "rb").read() if os.path.isfile(os.path.join(str(tmp_path), f)) else None)
             for f in os.listdir(str(tmp_path)) if f not in ("genome.fa", "sites.fa", "in.vcf")}
    assert after == {f: b for f, b in before.items() if f not in ("genome.fa", "sites.fa", "in.vcf")}, name
    assert sorted(os.listdir(str(tmp_path / "DIR"))) == in_dir, name


def test_program_without_the_records_step_refuses(cpu_programs, tmp_path):
    """ntsm_vcf_main.cpp references ntsm_vcf_records weakly: linked without a definition, the program still runs -p as
    before and refuses --counts and --store, each with a message that says what this build lacks."""
    genome, sites, line = refusal_inputs(tmp_path, np.random.default_rng(3))
    g, s, v = write_case(tmp_path, genome, sites, ["S0", "S1"], [line("100"), line("200")])
    os.mkdir(str(tmp_path / "DIR"))
    for flags in (["--counts", "DIR"], ["--store", "S"], ["-p", "m", "--counts", "DIR", "--store", "S"]):
        rc, err = run_cpu(cpu_programs[1], ["-s", s, "-r", g] + flags + [v], tmp_path)
        assert rc == 1 and err.splitlines()[-1].startswith(b"Error: ") and b"the device library of this build lacks the records step" in err
        assert os.listdir(str(tmp_path / "DIR")) == [] and sorted(os.listdir(str(tmp_path))) == ["DIR", "genome.fa", "in.vcf", "sites.fa"]
    assert run_cpu(cpu_programs[1], ["-s", s, "-r", g, "-p", "m", v], tmp_path)[0] == 0
    assert os.path.exists(str(tmp_path / "m_matrix.tsv"))


# ---------------------------------------------------------------------------------------------------- GPU
TILE_SITES = 32                                  # kTileSites of ntsm_amd/csrc/ntsm_vcf.hip


def adversarial(rng, n, m, n_lines=60, n_keys=90, n_ev=700):
    """the lists of test_device_step_matches_numpy_model for n samples and m sites: many events per key, both sides on
    one key, conflicting genotypes, the last five keys without events, every key in exactly one list, some lists empty;
    site 0 (when there are others) has both lists empty"""
    geno = rng.integers(0, 4, size=(n_lines, n)).astype(np.uint8)
    keys = rng.integers(0, n_keys - 5, size=n_ev)
    lines = np.sort(rng.integers(0, n_lines, size=n_ev))
    sides = rng.integers(0, 2, size=n_ev)
    key_events = [[(int(o), int(lines[o]), int(sides[o])) for o in np.flatnonzero(keys == q)] for q in range(n_keys)]
    perm = rng.permutation(n_keys)
    cut = sorted(int(x) for x in rng.integers(0, n_keys + 1, size=2 * m - 1)) + [n_keys]
    cut = ([0, 0, 0] + cut[2:]) if m > 1 else [0] + cut
    site_ref = [[int(x) for x in perm[cut[2 * i]:cut[2 * i + 1]]] for i in range(m)]
    site_var = [[int(x) for x in perm[cut[2 * i + 1]:cut[2 * i + 2]]] for i in range(m)]
    return geno, key_events, site_ref, site_var


def records_model(geno, multi, key_events, site_ref, site_var):
    """numpy_model's state walk kept per key, then printCountsMax's maxima and 32-bit sums per (sample, site) and the two
    totals of a store record.  counts is checked against numpy_model's own cells."""
    n = geno.shape[1]
    v1, v2 = np.uint64(multi), np.uint64((2 * multi) & 0xFFFFFFFF)
    state = []
    for evs in key_events:
        st = np.zeros(n, dtype=np.uint64)
        for _, line, side in evs:
            code = geno[line]
            full = 2 if side else 0
            fresh = ((code == full) | (code == 1)) & (st == 0)
            st[fresh] = np.where(code == full, v2, v1)[fresh] & np.uint64(255)
        state.append(st)
    m = len(site_ref)
    counts = np.zeros((n, m, 2), dtype=np.uint32)
    sums = np.zeros((n, m, 2), dtype=np.uint32)
    for i in range(m):
        for c, lst in enumerate((site_ref[i], site_var[i])):
            if lst:
                counts[:, i, c] = np.max([state[q] for q in lst], axis=0)
                sums[:, i, c] = np.sum([state[q] for q in lst], axis=0)
    cells = numpy_model(geno, multi, key_events, site_ref, site_var)[0]
    assert np.array_equal(counts[:, :, 0] | counts[:, :, 1] << 8, cells.T)
    total = (counts[:, :, 0] + counts[:, :, 1]).astype(np.uint64).sum(axis=1)
    sum_of_sums = (sums[:, :, 0] + sums[:, :, 1]).astype(np.uint64).sum(axis=1)
    return counts, sums, total, sum_of_sums


def check_records(V, lists, multi, model, s_begin=0, s_count=None, pitch=None, want_sums=True):
    geno, key_events, site_ref, site_var = lists
    counts, sums, total, sos = model
    n, m = geno.shape[1], len(site_ref)
    hi = n if s_count is None else s_begin + s_count
    r = V.records(geno, multi, key_events, site_ref, site_var, s_begin=s_begin, s_count=s_count, pitch=pitch, want_sums=want_sums)
    bad = np.argwhere(r.counts != counts[s_begin:hi])
    assert bad.size == 0, bad[:10].tolist()                                       # (sample in the window, site, column)
    assert np.array_equal(r.total, total[s_begin:hi]) and np.array_equal(r.sum_of_sums, sos[s_begin:hi])
    if want_sums:
        assert np.array_equal(r.sums, sums[s_begin:hi])
    else:
        assert r.sums is None and r.raw_sums is None
    for raw in (r.raw_counts, r.raw_sums):                                        # nothing past a row's 8 * m bytes is written
        if raw is not None:
            assert raw.shape == (hi - s_begin, pitch or 8 * m) and np.all(raw[:, 8 * m:] == V.FILL)
    return r


SHAPES = [(1, 1, 20), (15, TILE_SITES - 1, 128), (16, TILE_SITES, 200), (17, TILE_SITES + 1, 20), (33, 1, 128), (33, TILE_SITES + 1, 200),
          (1025, TILE_SITES - 1, 20), (1025, TILE_SITES, 128), (4097, TILE_SITES + 1, 200), (4097, 1, 20)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,multi", SHAPES, ids=["n%d_sites%d_m%d" % s for s in SHAPES])
def test_records_match_numpy_model(built, n, m, multi):
    """ntsm_vcf_records on the adversarial lists: 1 to 4,097 samples (a 16-sample chunk that is ragged, full, one past
    full; 128-sample tiles: 1, 9 and 33 of them, the last with one live sample) x 1, T - 1, T and T + 1 sites for the
    tile's T = 32, multi 20 / 128 (2m truncates to 0) / 200.  counts, sums, both totals against records_model -- whose
    counts are numpy_model's cells -- with and without sums, and counts against the unpacked cells of V.run."""
    import ntsm_amd.vcf as V
    rng = np.random.default_rng(1000 * n + 10 * m + multi)
    lists = adversarial(rng, n, m)
    assert any(len(e) == 0 for e in lists[1]) and (m == 1 or (lists[2][0] == [] and lists[3][0] == []))
    model = records_model(lists[0], multi, *lists[1:])
    r = check_records(V, lists, multi, model)
    check_records(V, lists, multi, model, want_sums=False)
    cells = V.run(lists[0], multi, *lists[1:], warn_cap=1 << 20)[0]
    assert np.array_equal(r.counts[:, :, 0], (cells & 255).T) and np.array_equal(r.counts[:, :, 1], (cells >> 8).T)
    assert r.times.kernel_bytes > 0 and r.times.download_bytes == n * m * 16 + 16 * n


@pytest.mark.gpu
def test_records_window_and_pitch(built):
    """40 samples, 33 sites: the window [16, 33) -- its last chunk holds one sample of the window and 7 of the cohort that
    are not -- and rows at a store record's pitch, 1056 + 8 * n_sites: the bytes between the rows keep their fill.  Also
    the windows [0, 16) and [32, 40), and a refused window (s_begin not a multiple of 16, past the end): -1."""
    import ntsm_amd.vcf as V
    rng = np.random.default_rng(40)
    lists = adversarial(rng, 40, TILE_SITES + 1)
    model = records_model(lists[0], 20, *lists[1:])
    pitch = 1056 + 8 * (TILE_SITES + 1)
    check_records(V, lists, 20, model, s_begin=16, s_count=17, pitch=pitch)
    check_records(V, lists, 20, model, s_begin=16, s_count=17, pitch=pitch, want_sums=False)
    check_records(V, lists, 20, model, s_begin=0, s_count=16)
    check_records(V, lists, 20, model, s_begin=32, s_count=8, pitch=pitch)
    for s_begin, s_count, p in ((8, 8, None), (16, 25, None), (0, 0, None), (0, 40, 8 * TILE_SITES), (0, 40, 8 * TILE_SITES + 12)):
        with pytest.raises(RuntimeError, match=r"ntsm_vcf_records failed: -1$"):
            V.records(lists[0], 20, *lists[1:], s_begin=s_begin, s_count=s_count, pitch=p)


@pytest.mark.gpu
def test_records_sum_needs_more_than_16_bits(built):
    """One REF list of 300 keys, multi 255, every sample het: each final byte is 255, the sum 76,500; the VAR list of
    the site is empty, a second site has no keys, and two keys at the end have no events."""
    import ntsm_amd.vcf as V
    n = 33
    geno = np.full((1, n), V.HET, dtype=np.uint8)
    key_events = [[(q, 0, 0)] for q in range(300)] + [[], []]
    site_ref, site_var = [list(range(300)), []], [[], [300, 301]]
    r = V.records(geno, 255, key_events, site_ref, site_var)
    assert np.array_equal(r.counts, np.tile(np.array([[255, 0], [0, 0]], dtype=np.uint32), (n, 1, 1)))
    assert np.array_equal(r.sums, np.tile(np.array([[76500, 0], [0, 0]], dtype=np.uint32), (n, 1, 1)))
    assert r.total.tolist() == [255] * n and r.sum_of_sums.tolist() == [76500] * n
    model = records_model(geno, 255, key_events, site_ref, site_var)
    check_records(V, (geno, key_events, site_ref, site_var), 255, model, want_sums=False)


def run_gpu(exe, args, cwd, env=None):
    p = subprocess.run([exe] + args, cwd=str(cwd), capture_output=True, timeout=120, env=dict(os.environ, **(env or {})))
    return p.returncode, strip_time(p.stderr)


@pytest.mark.gpu
def test_cli_gives_the_recordings(built, tmp_path):
    """build/ntsmVCF --counts on the 13 cases with samples: the reference's recordings; the zero-sample case is refused"""
    check_recordings(VCF, tmp_path, run_gpu)
    d = os.path.join(GOLD, "zero_samples")
    rc, err = run_gpu(VCF, ["-s", "sites.fa", "-r", "genome.fa", "--counts", str(tmp_path), "in.vcf"], d)
    assert rc == 1 and b"has no samples" in err.splitlines()[-1]


@pytest.mark.gpu
def test_cli_store_equals_pack(built, seeded, tmp_path):
    """build/ntsmVCF --counts --store on the 33 x 120 cohort in windows of 16 against build/ntsmEval --pack, byte for
    byte; --store alone; the append of a second VCF"""
    check_store_against_pack(VCF, run_gpu, built, seeded, tmp_path)


@pytest.mark.gpu
def test_cli_threads_give_identical_bytes(built, seeded, tmp_path):
    """-t 1 against -t 16: the same counts files (the model's) and the same records"""
    d, g, s, v, want = seeded[33]
    for t in ("1", "16"):
        out = tmp_path / ("t" + t)
        out.mkdir()
        rc, err = run_gpu(VCF, ["-s", s, "-r", g, "-d", "-t", t, "--counts", str(out), "--store", str(tmp_path / ("s" + t)), v], tmp_path)
        assert rc == 0 and dir_bytes(out) == want, err[-500:]
    # the two stores differ only in their name fields (the counts files' paths hold t1 / t16)
    a, b = records_of(open(str(tmp_path / "s1"), "rb").read()), records_of(open(str(tmp_path / "s16"), "rb").read())
    assert a[0] == b[0] and [(r[0], r[2]) for r in a[1]] == [(r[0], r[2]) for r in b[1]]


@pytest.mark.gpu
def test_chain_store_into_ntsmEval_against(built, tmp_path):
    """One sample's --counts text as the query: ntsmEval -a --against STORE prints the same stdout for the store that
    ntsmVCF wrote and for the one ntsmEval --pack made of DIR's files, and without -a the query's row with its own record
    passes the default score threshold."""
    g, s, v = cohort(tmp_path, np.random.default_rng(51), 20, 400, dense=False)
    os.mkdir(str(tmp_path / "DIR"))
    rc, err = run_gpu(VCF, ["-s", s, "-r", g, "-t", "4", "--counts", "DIR", "--store", "vcf.store", v], tmp_path)
    assert rc == 0, err[-500:]
    files = ["DIR/S%d.counts.txt" % i for i in range(20)]
    assert open(str(tmp_path / "vcf.store"), "rb").read() == pack("pack.store", files, tmp_path)
    open(str(tmp_path / "query.txt"), "wb").write(open(str(tmp_path / files[3]), "rb").read())
    outs = []
    for store in ("vcf.store", "pack.store"):
        p = subprocess.run([EVAL, "-a", "--against", store, "query.txt"], cwd=str(tmp_path), capture_output=True, timeout=120)
        assert p.returncode == 0, p.stderr[-500:]
        outs.append(p.stdout)
    assert outs[0] == outs[1] and outs[0].count(b"\n") == 21, outs[0][:600]
    p = subprocess.run([EVAL, "--against", "vcf.store", "query.txt"], cwd=str(tmp_path), capture_output=True, timeout=120)
    assert p.returncode == 0, p.stderr[-500:]
    own = [l for l in p.stdout.splitlines() if l.split(b"\t")[:2] in ([b"query.txt", files[3].encode()], [files[3].encode(), b"query.txt"])]
    assert len(own) == 1, p.stdout[:600]
    assert own[0] in outs[0].splitlines()
