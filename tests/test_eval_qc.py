"""`ntsmEval --qc STORE [-p ROT -n NORM] [--sites-out FILE]`: the QC table of the reference's
single-file run (computeScoreSingle, src/CompareCounts.hpp:541-585) with one row per sample of a cohort store, and per-site
tallies under the same rule (calcHomHetMiss, :742-767).  Device side: ntsm_eval_store_profile
(ntsm_amd/csrc/ntsm_eval_profile.hip); host side: ntsm_amd/csrc/host/eval_qc.hpp.

CPU, devices hidden: the surface, every refusal, the failure without a device, the bad-argument returns, and the site table's
text against a Python model of its expressions.
GPU: the entry point against an exact numpy model at the shapes where its kernel can go wrong, against
ntsm_eval_project_store's tallies, twice for determinism; the CLI's rows byte for byte against oracle/_ref/ref_ntsmEval run on
each sample's counts file; an appended store; a store written by `ntsmCount --cohort`; the site table against the model.
No comparison has a tolerance."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle_binding import ROOT
from test_eval_pca import write_pca
from test_eval_reference import gpu_ref, reference, wrapped_samples  # noqa: F401
from test_eval_store import snapshot, unchanged

import make_eval  # noqa: E402  (tests/golden, on the path since test_eval_reference)

EVAL = os.path.join(ROOT, "build", "ntsmEval")
COUNT = os.path.join(ROOT, "build", "ntsmCount")
HEAD, NAME = 64, 1024
RECORD_HEAD = 32 + NAME
HIDDEN = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
SITE_HEADER = "#locusID\tcalled\tmiss\thomAT\thomCG\thet\tfreqAT\thetObs\thetExp\tmeanCov\n"
LARGE = 3000000000


def run(args, cwd, env=None):
    return subprocess.run([EVAL] + [str(a) for a in args], capture_output=True, cwd=str(cwd), env=env)


# ---------------------------------------------------------------------------------------------------- the store and the models
def store_bytes(counts, loci, names, raw_total, sum_of_sums, kmer_size, distinct):
    """A cohort store as DESIGN.md section 9.1 lays it out, with the scalars a counted sample has: `total` is the sum of the
    sites' uint32 line sums, widened"""
    counts = np.ascontiguousarray(counts, dtype="<u4")
    n, m = counts.shape[0], counts.shape[1]
    section = b"".join(l.encode() + b"\0" for l in loci)
    section += bytes(-(HEAD + len(section)) % 8) + np.ascontiguousarray(distinct, dtype="<u4").tobytes()
    first, stride = HEAD + len(section), RECORD_HEAD + 8 * m
    out = [b"NTSMCOH1" + struct.pack("<IIQQQ", 1, m, n, first, stride) + bytes(24), section]
    for r in range(n):
        total = int((counts[r, :, 0] + counts[r, :, 1]).astype(np.uint64).sum())
        name = names[r].encode()
        out.append(struct.pack("<QQQII", int(raw_total[r]), total, int(sum_of_sums[r]), int(kmer_size[r]), 0) + name + bytes(NAME - len(name))
                   + counts[r].tobytes())
    return b"".join(out)


def write_store(path, counts, rng):
    n, m = counts.shape[0], counts.shape[1]
    loci = ["rs%d" % (3 * s + 1) for s in range(m)]
    names = ["cohort/run%04d.txt" % r for r in range(n)]
    total = counts.astype(np.uint64).sum(axis=(1, 2))
    with open(str(path), "wb") as f:
        f.write(store_bytes(counts, loci, names, total * 7 + 1000, total * 3, np.full(n, 19), rng.integers(1, 30, size=(m, 2))))
    return loci, names


def model(db, c):
    """ntsm_eval_store_profile as include/ntsm_eval_hip.h states it, in numpy: (geno [n][3], tally [m][4], cov [m])"""
    db = np.asarray(db, dtype=np.uint32)
    a, b = db[:, :, 0] > c, db[:, :, 1] > c
    het, hom, miss = a & b, a ^ b, ~a & ~b
    geno = np.stack([het.sum(1), hom.sum(1), miss.sum(1)], axis=1).astype(np.uint32)
    tally = np.stack([(a & ~b).sum(0), (~a & b).sum(0), het.sum(0), miss.sum(0)], axis=1).astype(np.uint32)
    cov = db.astype(np.uint64).sum(axis=(0, 2), dtype=np.uint64)
    return geno.reshape(-1, 3), tally.reshape(-1, 4), cov


def site_text(loci, tally, cov, n):
    """The --sites-out bytes from the integers: the double expressions of eval_qc.hpp, each printed as std::to_string prints
    (%f).  Python floats are IEEE doubles and int -> float rounds to nearest, as the C++ conversions do."""
    out = [SITE_HEADER]
    for locus, (hom_at, hom_cg, het, miss), sc in zip(loci, np.asarray(tally).tolist(), np.asarray(cov).tolist()):
        called = hom_at + hom_cg + het
        if called == 0:
            mid = "NA\tNA\tNA"
        else:
            p = float(2 * hom_at + het) / float(2 * called)
            het_obs = float(het) / float(called)
            het_exp = 2 * p * (1 - p)
            mid = "%f\t%f\t%f" % (p, het_obs, het_exp)
        out.append("%s\t%d\t%d\t%d\t%d\t%d\t%s\t%f\n" % (locus, called, miss, hom_at, hom_cg, het, mid, float(sc) / float(n)))
    return "".join(out).encode()


def edge_cells(rng, n, m, c):
    """[n][m][2] with every cell drawn from {0, c, c + 1, large}; at the first and last site and both sides of every 64-site
    tile edge the first four samples (as many as there are) are a het, a hom of either allele and a miss whose counts sit at
    c + 1 and c: both sides of the strict comparison"""
    db = rng.choice(np.array([0, c, c + 1, LARGE], dtype=np.uint32), size=(n, m, 2))
    planted = [(c + 1, c + 1), (c + 1, c), (c, c + 1), (c, c)]
    for s in sorted({0, m - 1} | {e for k in range(64, m + 1, 64) for e in (k - 2, k - 1, k, k + 1) if 0 <= e < m}):
        for r in range(min(n, 4)):
            db[(r + s) % n if n >= 4 else r, s] = planted[r]
    return db


def qc_cohort(d, seed=41):
    """six samples x 130 sites as counts files over one sites set, one with wrapped line totals and one empty, + norm.txt and
    rot.tsv of 4 components; packed into S"""
    rng = np.random.default_rng(seed)
    s = wrapped_samples(rng, 6, 130)
    names = make_eval.write_cohort(str(d), s)
    write_pca(d, 130, 4, rng)
    p = run(["--pack", "S"] + names, d)
    assert p.returncode == 0, p.stderr
    return s, names


# ---------------------------------------------------------------------------------------------------- CPU
def test_surface():
    """The entry point is exported and declared, the Python binding exists, the help text names both flags under its "This
    build only" part and says how the rows differ from the single-file run's."""
    lib = ctypes.CDLL(os.path.join(ROOT, "ntsm_amd", "libntsm_eval_hip.so"))
    hdr = open(os.path.join(ROOT, "include", "ntsm_eval_hip.h")).read()
    assert hasattr(lib, "ntsm_eval_store_profile")
    assert "int ntsm_eval_store_profile(int device, const void *db_counts, uint64_t db_stride_bytes, uint32_t n_db, uint32_t n_sites," in hdr
    import ntsm_amd.eval as ev
    assert callable(ev.store_profile) and callable(ev.site_table_text)
    p = subprocess.run([EVAL, "--help"], capture_output=True, env=HIDDEN)
    assert p.returncode == 0 and p.stdout == b""
    ours = p.stderr.split(b"This build only")[1]
    assert b"--qc = STORE" in ours and b"--sites-out = FILE" in ours and b"newline" in ours
    assert b"--within = STORE" in ours and b"--between-near = STORE_A STORE_B" in ours               # and what was there is
    assert b"Not in this build: -b (debug mode of the PCA search); the PCA-guided search (-p)\nagainst a store" in p.stderr


def test_refusals(tmp_path):
    """Every refusal of --qc and --sites-out: exit 1, its own 'Error:' sentence, nothing on stdout, no GPU work (devices are
    hidden), the store -- bytes and mtime -- as it was, no --sites-out file and no index left behind."""
    rng = np.random.default_rng(5)
    db = rng.integers(0, 30, size=(3, 40, 2)).astype(np.uint32)
    write_store(tmp_path / "S", db, rng)
    write_store(tmp_path / "empty", db[:0], rng)
    good = open(str(tmp_path / "S"), "rb").read()
    open(str(tmp_path / "trunc"), "wb").write(good[:-1])
    open(str(tmp_path / "magic"), "wb").write(b"NTSMCOH2" + good[8:])
    write_pca(tmp_path, 40, 3, rng)
    open(str(tmp_path / "q.txt"), "w").write("#@TK\t5\n#@KS\t19\nrs1\t1\t2\t1\t2\t1\t1\n")
    os.mkdir(str(tmp_path / "dir"))
    P = ["-p", "rot.tsv", "-n", "norm.txt", "-d", "2"]
    own = b"--qc prints the QC tables of one store and is a run of its own"
    cases = [
        (["--qc", "S", "--pack", "S", "q.txt"], "S", own),                                   # with any other store run
        (["--qc", "S", "--against", "S", "q.txt"], "S", own),
        (["--qc", "S", "--index", "S"] + P, "S", own),
        (["--qc", "S", "--near", "S", "q.txt"], "S", own),
        (["--qc", "S", "--within", "S"], "S", own),
        (["--qc", "S", "--within-near", "S"], "S", own),
        (["--qc", "S", "--between", "S", "S"], "S", own),
        (["--between-near", "S", "--qc", "S", "S"], "S", own),
        (["--sites-out", "sites.tsv", "--within", "S"], "S", b"--sites-out is the per-site table of --qc"),
        (["--sites-out", "sites.tsv", "q.txt"], "S", b"--sites-out is the per-site table of --qc"),
        (["--qc", "S", "q.txt"], "S", b"--qc takes no input files"),
        (["--qc", "S", "-b", "truth.tsv"], "S", b"-b with --qc is not part of this build"),
        (["--qc", "S", "-e", "merged.txt"], "S", b"merging (-e, -o) with --qc is not part of this build"),
        (["--qc", "S", "-o"], "S", b"merging (-e, -o) with --qc is not part of this build"),
        (["--qc", "S", "-p", "rot.tsv"], "S", b"--qc -p needs a readable normalization file (-n)"),
        (["--qc", "S", "-p", "rot.tsv", "-n", "nowhere.txt"], "S", b"--qc -p needs a readable normalization file (-n)"),
        (["--qc", "S", "-n", "norm.txt"], "S", b"--qc takes -n only with -p"),
        (["--qc", "S", "-p", "nowhere.tsv", "-n", "norm.txt"], "S", b"--qc -p needs a readable rotation file"),
        (["--qc", "S", "-p", "rot.tsv", "-n", "norm.txt", "-d", "0"], "S", b"a PCA search with -d 0 is not part of this build"),
        (["--qc", "trunc"], "trunc", b"its header describes"),                               # an invalid store
        (["--qc", "magic"], "magic", b"not a cohort store"),
        (["--qc", "nowhere"], "S", b"cannot open store nowhere"),
        (["--qc", "empty"], "empty", b"empty holds no samples"),
        (["--qc", "S", "--sites-out", "dir"], "S", b"cannot write dir"),                     # cannot be opened for writing
        (["--qc", "S", "--sites-out", "no/such/dir/sites.tsv"], "S", b"cannot write no/such/dir/sites.tsv"),
        (["--qc", "S", "--within-rows", "3"], "S", b"--within-rows sets the bands of --within"),
        (["--qc", "S", "--between-rows", "3"], "S", b"--between-rows sets the bands of --between"),
    ]
    for args, touched, sentence in cases:
        extra = [] if "--sites-out" in args else ["--sites-out", "sites.tsv"]
        if "--qc" not in args:
            extra = []
        path = str(tmp_path / touched)
        before = snapshot(path)
        p = run(args + extra, tmp_path, env=HIDDEN)
        assert p.returncode == 1 and p.stdout == b"", (args, p.returncode, p.stdout[:100], p.stderr[-300:])
        assert any(line.startswith(b"Error: ") and sentence in line for line in p.stderr.split(b"\n")), (args, p.stderr)
        assert unchanged(path, before), args
        for left in ("sites.tsv", "merged.txt", touched + ".pcaidx", touched + ".tmp"):
            assert not os.path.exists(str(tmp_path / left)), (args, left)
    # the sentences the other runs always had
    p = run(["--within", "S", "--pack", "S"], tmp_path, env=HIDDEN)
    assert p.returncode == 1 and b"are seven runs: give one of them" in p.stderr
    p = run(["--between-near", "S", "--within", "S", "S"], tmp_path, env=HIDDEN)
    assert p.returncode == 1 and b"are eight runs: give one of them" in p.stderr


def test_qc_without_a_device_fails_and_prints_nothing(tmp_path):
    """A valid --qc where no device can be opened: the GPU failure message, exit 3, no header on stdout, the store as it was,
    no --sites-out file made -- and one that was there keeps its bytes.  -a, -s, -w and the radius flags are read."""
    rng = np.random.default_rng(6)
    write_store(tmp_path / "S", rng.integers(0, 30, size=(3, 40, 2)).astype(np.uint32), rng)
    write_pca(tmp_path, 40, 3, rng)
    before = snapshot(str(tmp_path / "S"))
    open(str(tmp_path / "old.tsv"), "w").write("kept\n")
    for args in ([], ["-a", "-s", "0.1", "-w", "0", "-S", "1", "-l", "3", "-r", "0.5", "-1", "0.1", "-2", "0.2"], ["--sites-out", "sites.tsv"],
                 ["--sites-out", "old.tsv"], ["-p", "rot.tsv", "-n", "norm.txt", "-d", "2", "-c", "0"]):
        p = run(["--qc", "S"] + args, tmp_path, env=HIDDEN)
        assert p.returncode == 3 and p.stdout == b"", (args, p.returncode, p.stdout[:100], p.stderr[-300:])
        assert b"on the GPU failed" in p.stderr and b"there is no CPU path" in p.stderr, (args, p.stderr)
        assert unchanged(str(tmp_path / "S"), before) and not os.path.exists(str(tmp_path / "sites.tsv"))
        assert open(str(tmp_path / "old.tsv")).read() == "kept\n"
    assert not os.path.exists(str(tmp_path / "S.pcaidx"))


def test_bad_arguments_need_no_device():
    """-1 before any HIP call: a stride below 8 * n_sites, a stride that is no multiple of 4, all three outputs NULL, counts
    NULL; and the empty shapes give zeroed outputs without a device."""
    import ntsm_amd.eval as ev
    f = ev.lib.ntsm_eval_store_profile
    m, n = 5, 3
    db = np.ones((n, m, 2), dtype=np.uint32)
    geno, tally, cov = np.full((n, 3), 7, np.uint32), np.full((m, 4), 7, np.uint32), np.full(m, 7, np.uint64)
    out = (geno.ctypes.data, tally.ctypes.data, cov.ctypes.data)
    assert f(0, db.ctypes.data, 8 * m - 8, n, m, 1, 0, *out, None) == -1
    assert f(0, db.ctypes.data, 8 * m - 4, n, m, 1, 0, *out, None) == -1
    assert f(0, db.ctypes.data, 8 * m + 2, n, m, 1, 0, *out, None) == -1
    assert f(0, db.ctypes.data, 8 * m, n, m, 1, 0, None, None, None, None) == -1
    assert f(0, None, 8 * m, n, m, 1, 0, *out, None) == -1
    assert (geno == 7).all() and (tally == 7).all() and (cov == 7).all()
    times = ev.CrossTimes()
    assert f(0, db.ctypes.data, 8 * m, 0, m, 1, 0, *out, ctypes.byref(times)) == 0               # no sample
    assert (tally == 0).all() and (cov == 0).all() and times.chunks == 0
    geno[:] = 7
    assert f(0, db.ctypes.data, 0, n, 0, 1, 0, *out, None) == 0                                   # no site
    assert (geno == 0).all()


def test_site_table_text_against_the_model():
    """eval_qc.hpp's table (through libntsm_host.so) against site_text on given integers: a site nobody calls (NA), one
    everybody calls, single classes, thirds (digits that round), counts near 2^32 and a coverage sum past 2^53."""
    import ntsm_amd.eval as ev
    tally = np.array([[0, 0, 0, 9], [9, 0, 0, 0], [0, 9, 0, 0], [0, 0, 9, 0], [1, 1, 1, 6], [2, 0, 1, 6], [0, 1, 2, 6], [1, 0, 0, 8],
                      [4294967295, 0, 0, 0], [1431655765, 1431655765, 1431655765, 0], [0, 0, 1, 4294967294], [3, 2, 1, 3]], dtype=np.uint32)
    cov = np.array([0, 1, 2, 3, 10, 100, 1000, 7, 2**64 - 1, 2**53 + 1, 3 * 2 * (2**32 - 1), 123456789], dtype=np.uint64)
    loci = ["rs%d" % i for i in range(len(tally))]
    for n in (9, 7, 4294967295):
        got = ev.site_table_text(loci, tally, cov, n)
        assert got == site_text(loci, tally, cov, n), n
    text = ev.site_table_text(loci, tally, cov, 9).decode()
    assert text.startswith(SITE_HEADER) and text.split("\n")[1] == "rs0\t0\t9\t0\t0\t0\tNA\tNA\tNA\t0.000000"
    assert text.split("\n")[5] == "rs4\t3\t6\t1\t1\t1\t0.500000\t0.333333\t0.500000\t1.111111"
    assert ev.site_table_text([], np.zeros((0, 4)), np.zeros(0), 3) == SITE_HEADER.encode()


# ---------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def gpu(built):
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    import ntsm_amd.eval as ev
    return ev


def check_profile(ev, db, c, chunk=0, head=0):
    got = ev.store_profile(ev.Records.of(db, head), c, chunk)
    want = model(db, c)
    for name, g, w in zip(("geno", "tally", "cov"), got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, db.shape, c, chunk, head, np.argwhere(g != w)[:5].tolist())
    n = db.shape[0]
    assert got[3].chunks == (0 if n == 0 else -(-n // (chunk or n)))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 63, 64, 65, 130])
def test_profile_equals_the_model_on_every_field(gpu, m):
    """ntsm_eval_store_profile against model(): geno, tally and cov, every value.  Sites 1, 63, 64, 65 and 130 stand either
    side of the kernel's 64-site tile; samples 1, 3, 4, 5 either side of its four waves, 65 past one wave's first pass and 257
    past one 256-sample strip (two workgroups add into every site); min_cov 0, 1, 5 over edge_cells, where a lane or row that
    padding let in would count as a miss; the pitch dense and a store's (a 1,056-byte head); one chunk, and chunks of 7 of 20."""
    rng = np.random.default_rng([m, 77])
    for n in (1, 3, 4, 5, 65, 257):
        for c in (0, 1, 5):
            db = edge_cells(rng, n, m, c)
            for head in (0, RECORD_HEAD):
                check_profile(gpu, db, c, 0, head)
    for c in (0, 1, 5):
        db = edge_cells(rng, 20, m, c)
        for head in (0, RECORD_HEAD):
            check_profile(gpu, db, c, 7, head)


@pytest.mark.gpu
def test_profile_coverage_does_not_wrap_and_outputs_are_optional(gpu):
    """Both alleles 0xFFFFFFFF in 3 of 5 samples: every site's coverage sum passes 2^33 (and the 32-bit line sum wraps, which
    the 64-bit one must not).  Then each output NULL in turn: the others are unchanged."""
    ev = gpu
    rng = np.random.default_rng(78)
    db = edge_cells(rng, 5, 130, 1)
    db[[0, 2, 4]] = 0xFFFFFFFF
    geno, tally, cov, _ = check_profile(ev, db, 1, 0, RECORD_HEAD)
    assert int(cov.min()) >= 3 * 2 * (2**32 - 1) > 2**33
    db = edge_cells(rng, 65, 130, 1)
    want = model(db, 1)
    for off in range(3):
        on = [k != off for k in range(3)]
        got = ev.store_profile(ev.Records.of(db, RECORD_HEAD), 1, 0, geno=on[0], tally=on[1], cov=on[2])
        assert got[off] is None
        assert all(np.array_equal(got[k], want[k]) for k in range(3) if on[k]), off


@pytest.mark.gpu
def test_profile_geno_is_project_stores_geno_and_two_calls_agree(gpu):
    """db_geno as raw bytes against ntsm_eval_project_store's on the same records (65 x 130 and 257 x 65, min_cov 0 and 2);
    two calls of the profile give the same bytes in every output."""
    ev = gpu
    rng = np.random.default_rng(79)
    for (n, m), c in (((65, 130), 0), ((257, 65), 2)):
        rec = ev.Records.of(edge_cells(rng, n, m, c), RECORD_HEAD)
        norm = rng.random(m).astype(np.longdouble)
        rot = rng.standard_normal((2, m)).astype(np.longdouble)
        first, second = ev.store_profile(rec, c), ev.store_profile(rec, c, 100)
        assert first[0].tobytes() == ev.project_store(rec, norm, rot, c)[1].tobytes()
        assert all(first[k].tobytes() == second[k].tobytes() for k in range(3))


@pytest.fixture(scope="module")
def packed(tmp_path_factory, gpu_ref):
    d = tmp_path_factory.mktemp("qc")
    s, names = qc_cohort(d)
    return d, s, names


def rows_of(stdout):
    assert stdout.endswith(b"\n")
    return stdout[:-1].split(b"\n")


QC_FLAGS = [[], ["-c", "0"], ["-c", "3", "-g", "1000000"], ["-p", "rot.tsv", "-n", "norm.txt", "-d", "3"],
            ["-p", "rot.tsv", "-n", "norm.txt", "-d", "3", "-c", "0"]]


@pytest.mark.gpu
@pytest.mark.parametrize("flags", QC_FLAGS, ids=["default", "c0", "c3_g", "pca_d3", "pca_d3_c0"])
def test_cli_qc_equals_the_reference_rows(packed, flags):
    """build/ntsmEval --qc S against the unmodified reference class run on each sample's counts file
    (oracle/_ref/ref_ntsmEval -t 1 [flags] FILE): the header and every data row byte for byte; --qc ends every row in a
    newline, the reference prints its one row without.  Six samples x 130 sites: sample 2 has line totals that wrap at 2^32,
    sample 3 is empty.  The equality holds when a file's loci and distinct columns are the store's -- any cohort counted with
    one sites file, which these inputs are: the store takes both from the first file packed, the reference from the file it
    is given.  Ignored flags (-a, -s, -w, the radii) change nothing."""
    d, _, names = packed
    p = run(["--qc", "S"] + flags, d)
    assert p.returncode == 0, p.stderr[-400:]
    lines = rows_of(p.stdout)
    assert len(lines) == 1 + len(names)
    for i, name in enumerate(names):
        head, row = reference(flags, [name], d).split(b"\n")
        assert lines[0] == head and lines[1 + i] == row, (name, lines[1 + i], row)
        assert row.startswith(name.encode() + b"\t")
    assert lines[0].count(b"\tPC") == (3 if "-p" in flags else 0)
    q = run(["--qc", "S", "-a", "-s", "0.1", "-w", "0", "-S", "1", "-l", "3", "-t", "4"] + flags, d)
    assert q.returncode == 0 and q.stdout == p.stdout
    assert not os.path.exists(str(d / "S.pcaidx"))


@pytest.mark.gpu
def test_cli_qc_appended_store_and_its_report(packed):
    """A store packed in two runs prints the rows of the store packed in one; -vv reports chunks and times on stderr."""
    d, _, names = packed
    assert run(["--pack", "S2"] + names[:4], d).returncode == 0
    assert run(["--pack", "S2"] + names[4:], d).returncode == 0
    flags = ["-p", "rot.tsv", "-n", "norm.txt", "-d", "2"]
    a, b = run(["--qc", "S2", "-v", "-v"] + flags, d), run(["--qc", "S"] + flags, d)
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout and a.stdout.count(b"\n") == 7
    report = [l for l in a.stderr.split(b"\n") if l.startswith(b"store qc: ")]
    assert len(report) == 1 and b"1 chunks" in report[0] and b"profile kernel" in report[0] and b"upload" in report[0]


@pytest.mark.gpu
def test_cli_qc_of_a_store_written_by_the_cohort_counter(gpu_ref, tmp_path):
    """`ntsmCount --cohort --store --counts` over three tiny samples: --qc of its store equals the reference on the counts
    files the same run wrote."""
    import ntsm_amd
    d = tmp_path
    s = ntsm_amd.SynthShort(sites_seed=20261020, n_sites=200, read_seed=7, sites_path=str(d / "sites.fa"))
    samples = [("one.txt", 0, 3000), ("two.txt", 3000, 5000), ("three.txt", 8000, 1000)]
    for name, first, count in samples:
        s.write_fastq(str(d / (name[:-4] + ".fq")), first, count)
    open(str(d / "m.tsv"), "w").write("".join("%s\t%s.fq\n" % (n, n[:-4]) for n, _, _ in samples))
    p = subprocess.run([COUNT, "-s", "sites.fa", "--cohort", "m.tsv", "--store", "CS", "--counts"], cwd=str(d), capture_output=True)
    assert p.returncode == 0, p.stderr[-400:]
    for flags in ([], ["-c", "0"]):
        q = run(["--qc", "CS"] + flags, d)
        assert q.returncode == 0, q.stderr[-400:]
        lines = rows_of(q.stdout)
        assert len(lines) == 4
        for i, (name, _, _) in enumerate(samples):
            head, row = reference(flags, [name], d).split(b"\n")
            assert lines[0] == head and lines[1 + i] == row, (name, lines[1 + i], row)


def check_site_table(d, store, db, loci, c, qc_rows):
    out = "sites_%s.tsv" % store
    p = run(["--qc", store, "-c", c, "--sites-out", out], d)
    assert p.returncode == 0 and p.stdout == qc_rows, p.stderr[-400:]
    n = db.shape[0]
    _, tally, cov = model(db, c)
    got = open(str(d / out), "rb").read()
    assert got == site_text(loci, tally, cov, n)
    rows = [l.split("\t") for l in got.decode().split("\n")[1:-1]]
    assert len(rows) == db.shape[1]
    assert all(int(r[1]) + int(r[2]) == n for r in rows)
    sample_hets = sum(int(l.split(b"\t")[5]) for l in rows_of(qc_rows)[1:])
    assert sum(int(r[5]) for r in rows) == sample_hets
    return got


@pytest.mark.gpu
def test_cli_site_table_equals_the_model(packed, gpu):
    """--sites-out on the packed 6 x 130 store (-c 1) and on a written 70 x 65 store with -c 2 (two passes of a wave, one site
    past a tile) against site_text over model(): byte for byte; called + miss is the number of samples on every line and the
    het column sums to the samples' het; stdout is what --qc prints without --sites-out; an existing file is replaced."""
    d, s, _ = packed
    plain = run(["--qc", "S"], d)
    assert plain.returncode == 0
    open(str(d / "sites_S.tsv"), "w").write("x" * 100000)                                   # longer than the table: it is cut
    text = check_site_table(d, "S", s, ["rs%d" % j for j in range(130)], 1, plain.stdout)
    assert b"\tNA\t" not in text.split(b"\n")[1]
    rng = np.random.default_rng(80)
    db = edge_cells(rng, 70, 65, 2)
    db[:, 40] = rng.integers(0, 3, size=(70, 2))                                            # a site nobody calls at -c 2
    loci, _ = write_store(d / "W", db, rng)
    plain = run(["--qc", "W", "-c", "2"], d)
    assert plain.returncode == 0
    text = check_site_table(d, "W", db, loci, 2, plain.stdout)
    assert text.split(b"\n")[41].split(b"\t")[6:9] == [b"NA", b"NA", b"NA"]
