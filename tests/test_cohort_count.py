"""`ntsmCount --cohort MANIFEST --store STORE [--counts] [--resume]`: every sample of a manifest counted
in one process on the same contexts, each appended to a cohort store as soon as it is finished.  Device side:
ntsm_sites_attach / ntsm_sites_reduce (include/ntsm_hip.h, ntsm_amd/csrc/kernels_sites.hip) turn a context's per-k-mer vector
into the per-site record; host side: ntsm_amd/csrc/host/cohort.hpp and FingerPrint::nextSample / siteRecord.

The contract: STORE is byte for byte what `ntsmCount [flags] READS... > NAME` per manifest line followed by
`ntsmEval --pack STORE NAME...` gives -- two paths this feature leaves as they were.

CPU: the surface, the refusals that need no context, every refusal of the command line (exit status 1, one sentence, STORE
untouched), and the host code under the sanitizers (`make cohort_check`).
GPU: ntsm_sites_reduce against a numpy statement of its contract on planted vectors (counts at and past 2^32 included) and
against the host's print_counts_max / sites_covered on a counted sample; the command line against the two-step route for the
default flags, -d, -m 5 (and a -m that stops every sample), -t 4 and -g 0,0; append and --resume; `ntsmEval --within` over both stores.  No comparison has a
tolerance."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT = os.path.join(ROOT, "build", "ntsmCount")
EVAL = os.path.join(ROOT, "build", "ntsmEval")
ERR_ARG = -1


def run(exe, args, cwd, **kw):
    return subprocess.run([exe] + [str(a) for a in args], cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, **kw)


# ------------------------------------------------------------------------------------------------------------------- CPU
def test_surface(built):
    """The two entry points are exported by the library and declared in the header with the reference lines they replace; the
    help text names the four options under its "This build only" part; the Python calls exist."""
    import ntsm_amd.capi as capi
    header = open(os.path.join(ROOT, "include", "ntsm_hip.h")).read()
    for name in ("ntsm_sites_attach", "ntsm_sites_reduce"):
        assert hasattr(capi.H, name) and "int %s(ntsm_ctx *ctx" % name in header
    assert "ntsm_site_totals" in header and "src/FingerPrint.hpp:270-311" in header and "src/FingerPrint.hpp:313-349" in header
    assert callable(capi.Context.sites_attach) and callable(capi.Context.sites_reduce)
    text = run(COUNT, ["--help"], ROOT).stderr
    own = text[text.index(b"This build only"):]
    for opt in (b"--cohort", b"--store", b"--counts", b"--resume"):
        assert opt in own
    assert b"-s, --snp = STR" in text and b"-g, --gpu" in text                  # and what was there is


def test_argument_refusals_without_a_device(built):
    """A NULL context is NTSM_ERR_ARG for both entry points whatever else is passed, and the check ntsm_sites_attach runs on
    its lists before any HIP call (ntsm_debug_sites_check) refuses NULL offsets, offsets that decrease and an index >= n_kmers
    -- all with no device in sight.  (A reduce without lists and NULL counts need a context, which cannot be made without a
    device: test_sites_reduce_refusals repeats the whole list on one.)"""
    import ntsm_amd.capi as capi
    off = np.zeros(3, dtype=np.uint32)
    ix = np.zeros(1, dtype=np.uint32)
    out = np.zeros(2, dtype=np.uint32)
    tot = capi.SiteTotals()
    u32p = capi.u32p
    assert capi.H.ntsm_sites_attach(None, off.ctypes.data_as(u32p), ix.ctypes.data_as(u32p), 1) == ERR_ARG
    assert capi.H.ntsm_sites_attach(None, None, None, 0) == ERR_ARG
    assert capi.H.ntsm_sites_reduce(None, out.ctypes.data_as(u32p), out.ctypes.data_as(u32p), ctypes.byref(tot)) == ERR_ARG
    assert capi.H.ntsm_sites_reduce(None, None, None, None) == ERR_ARG
    ms = ctypes.c_double()
    assert capi.H.ntsm_sites_kernel_ms(None, ctypes.byref(ms)) == ERR_ARG
    p = lambda a: np.asarray(a, dtype=np.uint32).ctypes.data_as(u32p)      # noqa: E731
    check = capi.H.ntsm_debug_sites_check
    assert check(100, p([0, 2, 3, 3, 4]), p([0, 99, 5, 7]), 2) == 0
    assert check(100, p([0]), None, 0) == 0 and check(100, p([0, 0, 0]), None, 1) == 0        # no site; a site with two empty lists
    assert check(100, None, p([0, 99, 5, 7]), 2) == ERR_ARG
    assert check(100, p([0, 2, 1, 3, 4]), p([0, 99, 5, 7]), 2) == ERR_ARG                        # offsets that decrease
    assert check(100, p([0, 2, 3, 3, 4]), p([0, 100, 5, 7]), 2) == ERR_ARG                       # an index >= n_kmers
    assert check(99, p([0, 2, 3, 3, 4]), p([0, 99, 5, 7]), 2) == ERR_ARG
    assert check(100, p([0, 2, 3, 3, 4]), None, 2) == ERR_ARG                                    # lists without indices
    assert check(100, p([0]), None, 0x80000000) == ERR_ARG                                       # 2 * n_sites no longer fits


# two loci; rs2's REF record holds two 19-mers joined by 'N'
RS2_REF = "TTGACCATGGCATTAGCAGNTGACCATGGCATTAGCAGG"
SITES_OK = ">rs1 ref\nGATTACAGGCTTAACCGTA\n>rs1 var\nGATTACAGGATTAACCGTA\n>rs2 ref\n" + RS2_REF + "\n>rs2 var\nTTGACCATGGAATTAGCAG\n"


def _cli_world(tmp_path):
    """a sites file of two loci, two read files, and a valid store over exactly those loci (written from counts text that
    is made here, with --pack: no GPU)"""
    (tmp_path / "sites.fa").write_text(SITES_OK)
    for n in ("a.fq", "b.fq"):
        (tmp_path / n).write_text("@r\nGATTACAGGCTTAACCGTAGC\n+\nIIIIIIIIIIIIIIIIIIIII\n")
    sites = _sites(str(tmp_path / "sites.fa"))
    off, _ = sites.lists()
    rows = "".join("rs%d\t1\t0\t2\t0\t%d\t%d\n" % (i + 1, off[2 * i + 1] - off[2 * i], off[2 * i + 2] - off[2 * i + 1]) for i in range(2))
    (tmp_path / "old.txt").write_text("#@TK\t10\n#@KS\t19\n#locusID\tcountAT\tcountCG\tsumAT\tsumCG\tdistinctAT\tdistinctCG\n" + rows)
    assert run(EVAL, ["--pack", "S", "old.txt"], tmp_path).returncode == 0
    return sites


def _sites(path, dupes=False):
    import ntsm_amd.capi as capi
    return capi.Sites(path, k=19, allow_dupes=dupes)


def test_cli_refusals(built, tmp_path):
    """Everything that can be known up front: exit status 1, one sentence on stderr, nothing on stdout, STORE's bytes and
    mtime as they were, no NAME written -- on a machine with or without a GPU, because no device is touched before."""
    _cli_world(tmp_path)
    at = lambda n: str(tmp_path / n)                                      # noqa: E731

    def manifest(text, name="m.tsv"):
        (tmp_path / name).write_text(text)
        return name

    def snapshot(p):
        return (open(p, "rb").read(), os.stat(p).st_mtime_ns)

    # stores a run must not append to
    (tmp_path / "other_sites.fa").write_text(SITES_OK.replace("rs2", "rs9"))
    (tmp_path / "fewer_sites.fa").write_text(SITES_OK[:SITES_OK.index(">rs2")])
    (tmp_path / "shorter_sites.fa").write_text(SITES_OK.replace(RS2_REF, RS2_REF[:19]))        # same loci, other distinct columns
    good = open(at("S"), "rb").read()
    open(at("cut"), "wb").write(good[:-8])
    open(at("magic"), "wb").write(b"NTSMCOHX" + good[8:])
    # site sets a cohort run refuses: a k-mer shared between two sites (erased without -d), a repeated locus
    (tmp_path / "shared_sites.fa").write_text(SITES_OK + ">rs3 ref\nGATTACAGGCTTAACCGTA\n>rs3 var\nCCGTACGTTCGAACGTAGC\n")
    (tmp_path / "twice_sites.fa").write_text(SITES_OK + ">rs1 ref\nAAGTCCTGATCGGATCAAT\n>rs1 var\nAAGTCCTGAACGGATCAAT\n")
    ok = manifest("x\ta.fq\n", "ok.tsv")
    long_name = "n" * 1024
    cases = [
        (["-s", "sites.fa", "--cohort", manifest("x\n", "m1"), "--store", "S"], b"is not NAME<TAB>READS"),            # manifest syntax
        (["-s", "sites.fa", "--cohort", manifest("x\ta.fq\t\tb.fq\n", "m2"), "--store", "S"], b"is not NAME<TAB>READS"),
        (["-s", "sites.fa", "--cohort", manifest("x a.fq\n", "m3"), "--store", "S"], b"is not NAME<TAB>READS"),
        (["-s", "sites.fa", "--cohort", manifest("# none\n\n", "m4"), "--store", "S"], b"lists no sample"),          # an empty manifest
        (["-s", "sites.fa", "--cohort", manifest("", "m5"), "--store", "S"], b"lists no sample"),
        (["-s", "sites.fa", "--cohort", "no_such_manifest", "--store", "S"], b"cannot be opened"),
        (["-s", "sites.fa", "--cohort", manifest("x\ta.fq\ny\tb.fq\nx\tb.fq\n", "m6"), "--store", "S"], b"listed twice"),
        (["-s", "sites.fa", "--cohort", manifest(long_name + "\ta.fq\n", "m7"), "--store", "S"], b"at most 1023"),
        (["-s", "sites.fa", "--cohort", manifest("x\ta.fq\tmissing.fq\n", "m8"), "--store", "S"], b"missing.fq of sample x does not exist"),
        (["-s", "sites.fa", "--cohort", ok, "--store", "cut"], b"its header describes"),                               # an invalid store
        (["-s", "sites.fa", "--cohort", ok, "--store", "magic"], b"not a cohort store"),
        (["-s", "other_sites.fa", "--cohort", ok, "--store", "S"], b"the sites file has rs9 there"),                   # a store that does not match
        (["-s", "fewer_sites.fa", "--cohort", ok, "--store", "S"], b"holds 2 loci, the sites file has 1"),
        (["-s", "shorter_sites.fa", "--cohort", ok, "--store", "S"], b"distinct columns"),
        (["-s", "sites.fa", "--cohort", manifest("old.txt\ta.fq\n", "m9"), "--store", "S"], b"already in the store"),  # without --resume
        (["-s", "shared_sites.fa", "--cohort", ok, "--store", "S"], b"shared between sites"),                          # an erased k-mer
        (["-s", "shared_sites.fa", "--cohort", ok, "--store", "new1"], b"shared between sites"),
        (["-s", "twice_sites.fa", "--cohort", ok, "--store", "new2"], b"is in the sites file twice"),            # a repeated locus
        (["-s", "sites.fa", "--cohort", ok], b"--cohort needs --store"),
        (["-s", "sites.fa", "--store", "S"], b"--store needs --cohort"),
        (["-s", "sites.fa", "--counts", "a.fq"], b"--counts needs --cohort"),
        (["-s", "sites.fa", "--resume", "a.fq"], b"--resume needs --cohort"),
        (["-s", "sites.fa", "--cohort", ok, "--store", "S", "a.fq"], b"come from the manifest"),                       # positional read files
        (["-s", "sites.fa", "--cohort", ok, "--store", "S", "--counts", "no_such_reads.fq"], b"come from the manifest"),
    ]
    before = {n: snapshot(at(n)) for n in ("S", "cut", "magic")}
    for args, want in cases:
        p = run(COUNT, args, tmp_path)
        lines = p.stderr.split(b"\n")
        assert p.returncode == 1 and p.stdout == b"", (args, p.returncode, p.stderr[-300:])
        assert len(lines) == 2 and lines[1] == b"" and lines[0].startswith(b"ntsmCount: ") and want in lines[0], (args, p.stderr[-400:])
        for n, was in before.items():
            assert snapshot(at(n)) == was, (args, n)
        assert not os.path.exists(at("x")) and not os.path.exists(at("new1")) and not os.path.exists(at("new2")) and not os.path.exists(at("S.tmp"))
    # without --cohort the tool is the one it was: the same complaint about missing input files, exit status 1
    p = run(COUNT, ["-s", "sites.fa"], tmp_path)
    assert p.returncode == 1 and b"Error: Need input files" in p.stderr


def test_host_code_under_the_sanitizers():
    """`make cohort_check`: tools/cohort_count_check.cpp -- the manifest parser, the site lists and the record builder against
    counts text + eval_store::pack, byte for byte, creation and append, totals that wrap at 2^32 -- built with
    -fsanitize=address,undefined as a program of its own, run once by the target."""
    p = subprocess.run(["make", "-s", "cohort_check"], cwd=ROOT, capture_output=True)
    assert p.returncode == 0 and p.stdout.endswith(b"ok\n") and b"FAILED" not in p.stdout and b"NOT refused" not in p.stdout, (p.stdout[-800:], p.stderr[-800:])
    assert b"runtime error" not in p.stderr and b"AddressSanitizer" not in p.stderr
    assert p.stdout.count(b"cohort store == packed store") == 3 and p.stdout.count(b"refused (") >= 16
    assert b"5 of 5 records hold a total that wrapped at 2^32" in p.stdout


# ------------------------------------------------------------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def nt(built):
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    import ntsm_amd
    return ntsm_amd


U32 = np.uint64(0xFFFFFFFF)


def model(vec, offsets, kmer_ix):
    """ntsm_sites_reduce as include/ntsm_hip.h states it, in numpy (uint64 vec)"""
    n = (len(offsets) - 1) // 2
    counts = np.zeros((n, 2), dtype=np.uint32)
    sums = np.zeros((n, 2), dtype=np.uint32)
    covered = 0
    for i in range(n):
        hit = False
        for a in range(2):
            v = vec[kmer_ix[offsets[2 * i + a]:offsets[2 * i + a + 1]]]
            f = v & U32
            counts[i, a] = f.max() if len(f) else 0
            sums[i, a] = int(f.sum()) & 0xFFFFFFFF
            hit = hit or bool((v != 0).any())
        covered += hit
    wrap = lambda x: int(((x[:, 0].astype(np.uint64) + x[:, 1].astype(np.uint64)) & U32).sum())   # noqa: E731
    return counts, sums, dict(total=wrap(counts), sum_of_sums=wrap(sums), sites_covered=covered)


def plant(nt, ctx, vec):
    """the context's dense vector := vec, through counts_device() + import_reduced() as tests/test_gpu_parity.py does"""
    import torch
    from ntsm_amd.dist import _DeviceVector
    ptr, words = ctx.counts_device()
    assert words == len(vec) + 4
    d = torch.as_tensor(_DeviceVector(ptr, words), device="cuda")
    d[:len(vec)] = torch.from_numpy(vec.view(np.int64)).to(d.device)
    torch.cuda.synchronize()
    ctx.import_reduced()


SPECIAL = np.array([0, 1, 0xFFFFFFFF, 1 << 32, (1 << 32) + 5, 0x80000000, 0x80000001, 0xFFFFFFF0, 0x20, (7 << 32) + 0xFFFFFFFF], dtype=np.uint64)


def lists_for(rng, n_sites, n_kmers):
    """list lengths from {0, 1, 13, 40}; site 0 (where there are two sites or more: site 1) has both lists empty"""
    lens = rng.choice(np.array([0, 1, 13, 40]), size=2 * n_sites)
    if n_sites >= 2:
        lens[2:4] = 0
        lens[0:2] = (13, 1)
    offsets = np.concatenate(([0], np.cumsum(lens))).astype(np.uint32)
    kmer_ix = rng.integers(0, n_kmers, size=int(offsets[-1]), dtype=np.uint32)
    return offsets, kmer_ix


@pytest.fixture(scope="module")
def planted(nt):
    """one context over 4,096 keys whose vector holds the special values and random ones"""
    rng = np.random.default_rng(1019)
    n_kmers = 4096
    keys = rng.choice(1 << 38, size=n_kmers, replace=False).astype(np.uint64)
    ctx = nt.Context(keys)
    vec = np.where(rng.random(n_kmers) < 0.3, 0, rng.integers(1, 300, size=n_kmers)).astype(np.uint64)
    where = rng.choice(n_kmers, size=1500, replace=False)
    vec[where] = SPECIAL[rng.integers(0, len(SPECIAL), size=len(where))]
    vec[where[:len(SPECIAL)]] = SPECIAL                                         # each of them at least once
    plant(nt, ctx, vec)
    yield ctx, vec, rng
    ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_sites", [1, 63, 64, 65, 257, 70000])
def test_sites_reduce_against_the_contract(nt, planted, n_sites):
    """counts, sums and the three totals for equality; one site, the workgroup's 128 sites and its waves' 32 from both sides,
    several workgroups, and 70,000 sites (547 workgroups: the totals through many atomics)."""
    ctx, vec, rng = planted
    offsets, kmer_ix = lists_for(rng, n_sites, len(vec))
    if n_sites >= 65:
        # pairs whose maxima and whose sums wrap when added: 2^32 - 1 beside 1 (to 0), 0x80000000 twice, 0xFFFFFFF0 + 0x20;
        # a site whose only count is exactly 2^32: covered, maximum 0
        fixed = {10: ([0xFFFFFFFF], [1]), 11: ([0x80000000], [0x80000001]), 12: ([0xFFFFFFF0, 1], [0x20, 0x20]), 13: ([1 << 32], []), 14: ([(1 << 32) + 5], [1 << 32])}
        pieces, lens = [], (offsets[1:] - offsets[:-1]).astype(np.int64)
        at = {int(v): int(np.flatnonzero(vec == np.uint64(v))[0]) for vals in fixed.values() for side in vals for v in side}
        starts = offsets[:-1].astype(np.int64)
        for t in range(2 * n_sites):
            site, a = divmod(t, 2)
            pieces.append(np.array([at[v] for v in fixed[site][a]], dtype=np.uint32) if site in fixed else kmer_ix[starts[t]:starts[t] + lens[t]])
        offsets = np.concatenate(([0], np.cumsum([len(p) for p in pieces]))).astype(np.uint32)
        kmer_ix = np.concatenate(pieces).astype(np.uint32)
    ctx.sites_attach(offsets, kmer_ix)
    counts, sums, tot = ctx.sites_reduce()
    want_counts, want_sums, want_tot = model(vec, offsets, kmer_ix)
    assert np.array_equal(counts, want_counts) and np.array_equal(sums, want_sums) and tot == want_tot, (tot, want_tot)
    if n_sites >= 65:
        assert list(counts[10]) == [0xFFFFFFFF, 1] and list(counts[13]) == [0, 0] and list(counts[14]) == [5, 0] and list(sums[12]) == [0xFFFFFFF1, 0x40]
        assert tot["total"] < int(counts.astype(np.uint64).sum())                    # the wrap of a pair's sum is in the total
    if n_sites >= 2:
        assert list(counts[1]) == [0, 0] and list(sums[1]) == [0, 0]                  # both lists empty
    counts_only, none, tot2 = ctx.sites_reduce(want_sums=False)
    assert none is None and np.array_equal(counts_only, counts) and tot2["total"] == tot["total"] and tot2["sites_covered"] == tot["sites_covered"]


@pytest.mark.gpu
def test_sites_reduce_attach_again_reset_and_no_site(nt):
    """A second attach replaces the first; after ntsm_reset the lists are still there and everything reads zero; n_sites = 0
    is legal and returns zeros."""
    rng = np.random.default_rng(7)
    n_kmers = 600
    keys = rng.choice(1 << 38, size=n_kmers, replace=False).astype(np.uint64)
    ctx = nt.Context(keys)
    vec = rng.integers(0, 50, size=n_kmers).astype(np.uint64)
    vec[5] = (1 << 32)
    plant(nt, ctx, vec)
    first = lists_for(rng, 130, n_kmers)
    second = lists_for(rng, 33, n_kmers)
    ctx.sites_attach(*first)
    a = ctx.sites_reduce()
    ctx.sites_attach(*second)
    b = ctx.sites_reduce()
    for got, lists in ((a, first), (b, second)):
        want = model(vec, *lists)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    assert b[0].shape == (33, 2)
    ctx.reset()
    counts, sums, tot = ctx.sites_reduce()
    assert counts.shape == (33, 2) and not counts.any() and not sums.any() and tot == dict(total=0, sum_of_sums=0, sites_covered=0)
    plant(nt, ctx, vec)
    ctx.sites_attach(np.zeros(1, dtype=np.uint32), np.zeros(0, dtype=np.uint32))
    counts, sums, tot = ctx.sites_reduce()
    assert counts.shape == (0, 2) and tot == dict(total=0, sum_of_sums=0, sites_covered=0)
    ctx.close()


@pytest.mark.gpu
def test_sites_reduce_refusals(nt):
    """NTSM_ERR_ARG for: a reduce without lists, NULL counts, offsets that decrease, an index >= n_kmers; the lists
    attached before stay in use after a refused attach."""
    capi = nt.capi
    u32p = capi.u32p
    keys = np.arange(1, 101, dtype=np.uint64) * np.uint64(977)
    ctx = nt.Context(keys)
    out = np.zeros(8, dtype=np.uint32)
    tot = capi.SiteTotals()
    p = lambda a: a.ctypes.data_as(u32p)                                   # noqa: E731
    assert capi.H.ntsm_sites_reduce(ctx._h, p(out), p(out), ctypes.byref(tot)) == ERR_ARG         # nothing attached
    good_off, good_ix = np.array([0, 2, 3, 3, 4], dtype=np.uint32), np.array([0, 99, 5, 7], dtype=np.uint32)
    assert capi.H.ntsm_sites_attach(ctx._h, p(good_off), p(good_ix), 2) == 0
    assert capi.H.ntsm_sites_reduce(ctx._h, None, p(out), ctypes.byref(tot)) == ERR_ARG           # NULL counts
    assert capi.H.ntsm_sites_attach(ctx._h, None, p(good_ix), 2) == ERR_ARG
    assert capi.H.ntsm_sites_attach(ctx._h, p(np.array([0, 2, 1, 3, 4], dtype=np.uint32)), p(good_ix), 2) == ERR_ARG
    assert capi.H.ntsm_sites_attach(ctx._h, p(good_off), p(np.array([0, 100, 5, 7], dtype=np.uint32)), 2) == ERR_ARG
    assert capi.H.ntsm_sites_reduce(ctx._h, p(out), None, ctypes.byref(tot)) == 0 and not out.any()   # still the good lists, nothing counted
    ctx.close()


N_SITES, N_READS = 2000, 60_000


@pytest.fixture(scope="module")
def world(nt, tmp_path_factory):
    """2,000 SynthShort sites and three samples of 60,000 reads each, the third in two read files"""
    d = tmp_path_factory.mktemp("cohort")
    s = nt.SynthShort(sites_seed=20261019, n_sites=N_SITES, read_seed=5, sites_path=str(d / "sites.fa"))
    s.write_fastq(str(d / "s1.fq"), 0, N_READS)
    s.write_fastq(str(d / "s2.fq"), N_READS, N_READS)
    s.write_fastq(str(d / "s3_1.fq"), 2 * N_READS, N_READS // 2)
    s.write_fastq(str(d / "s3_2.fq"), 2 * N_READS + N_READS // 2, N_READS // 2)
    samples = [("one.txt", ["s1.fq"]), ("two.txt", ["s2.fq"]), ("three.txt", ["s3_1.fq", "s3_2.fq"])]
    return s, d, samples


@pytest.mark.gpu
def test_sites_reduce_against_the_counting_path(nt, world):
    """One sample counted through the C ABI: the device's per-site record equals what the host computes from ntsm_counts --
    print_counts_max's rows (parsed back) and sites_covered."""
    s, d, _ = world
    sites = nt.Sites(str(d / "sites.fa"))
    ctx = nt.Context(sites.keys)
    offsets, kmer_ix = sites.lists()
    ctx.sites_attach(offsets, kmer_ix)
    ctx.submit(s.host_bytes(0, N_READS), s.read_end(N_READS))
    t = ctx.sync()
    counts, sums, tot = ctx.sites_reduce()
    vec = ctx.counts()
    rc, text = sites.format_counts(vec, t.total_kmers)
    rows = [l.split(b"\t") for l in text.split(b"\n") if l and not l.startswith(b"#")]
    assert rc == 0 and len(rows) == N_SITES
    host = np.array([[int(x) for x in r[1:7]] for r in rows], dtype=np.uint64)
    assert np.array_equal(counts, host[:, 0:2]) and np.array_equal(sums, host[:, 2:4])
    assert np.array_equal(host[:, 4], offsets[1::2] - offsets[0:-1:2]) and np.array_equal(host[:, 5], offsets[2::2] - offsets[1::2])
    _, covered = sites.format_summary(vec, t.total_bases, t.total_kmers, t.total_hits)
    assert tot["sites_covered"] == covered and 0 < covered <= N_SITES
    assert tot["total"] == int(host[:, 0:2].sum()) and tot["sum_of_sums"] == int(host[:, 2:4].sum()) and tot["total"] > 0
    want = model(vec, offsets, kmer_ix)
    assert tot == want[2]
    ctx.close()


def _summary_numbers(err):
    want = (b"Total Bases Considered: ", b"Total k-mers Considered: ", b"Total k-mers Recorded: ", b"Sites Covered by at least one k-mer: ")
    return [next(l[len(w):] for l in err.split(b"\n") if l.startswith(w)) for w in want]


def _two_step(d, samples, flags, tag):
    """the route the parent commit has: one ntsmCount per sample into its NAME, then ntsmEval --pack"""
    single = {}
    for name, reads in samples:
        p = run(COUNT, ["-s", "sites.fa"] + flags + reads, d)
        assert p.returncode == 0, p.stderr[-400:]
        open(os.path.join(str(d), name), "wb").write(p.stdout)
        single[name] = (p.stdout, _summary_numbers(p.stderr), p.stderr)
    store = "packed_" + tag
    assert run(EVAL, ["--pack", store] + [n for n, _ in samples], d).returncode == 0
    for name, _ in samples:
        os.unlink(os.path.join(str(d), name))
    return store, single


def _manifest(d, samples, name):
    open(os.path.join(str(d), name), "w").write("# cohort\n\n" + "".join("%s\t%s\n" % (n, "\t".join(r)) for n, r in samples))
    return name


# -m 5 arms the stop without tripping it on samples of this size (the threshold is 2.5 hits per site k-mer); -m 0.2 trips it
FLAG_SETS = {"default": [], "dupes": ["-d"], "m5": ["-m", "5"], "m_stop": ["-m", "0.2"], "t4": ["-t", "4"], "g00": ["-g", "0,0", "-t", "2"]}


@pytest.mark.gpu
@pytest.mark.parametrize("tag", list(FLAG_SETS))
def test_cli_identity(nt, world, tag):
    """--cohort --store --counts against the two-step route: the stores with cmp, each NAME against the single run's stdout,
    each stdout row against the single run's summary numbers; with -v the single run's summary block under `== NAME`."""
    s, d, samples = world
    flags = FLAG_SETS[tag]
    packed, single = _two_step(d, samples, flags, tag)
    store = "cohort_" + tag
    p = run(COUNT, ["-s", "sites.fa"] + flags + ["-v", "--cohort", _manifest(d, samples, "all.tsv"), "--store", store, "--counts"], d)
    assert p.returncode == 0, p.stderr[-600:]
    assert run("cmp", [store, packed], d).returncode == 0
    rows = [l.split(b"\t") for l in p.stdout.split(b"\n") if l]
    assert [r[0].decode() for r in rows] == [n for n, _ in samples]
    for (name, _), row in zip(samples, rows):
        text, numbers, err = single[name]
        assert open(os.path.join(str(d), name), "rb").read() == text, name
        assert row[1:] == numbers, (name, row, numbers)
        block = err[err.index(b"Total Bases Considered: "):err.index(b"Sites Covered")]
        assert b"== " + name.encode() + b"\n" + block in p.stderr, name
        os.unlink(os.path.join(str(d), name))
    reached = b"Reached desired (-m) threshold"
    assert p.stderr.count(reached) == sum(reached in single[n][2] for n, _ in samples)
    if tag == "m_stop":                                                      # every sample stops, each on its own reads
        assert p.stderr.count(reached) == len(samples) and all(int(r[1]) < N_READS * 150 for r in rows)


@pytest.mark.gpu
def test_append_resume_and_within(nt, world):
    """Samples 1-2 then 3 give the bytes of 1-3; --resume over the full manifest after the first two adds only the third;
    a name the store holds is refused without it; `ntsmEval --within` prints over the cohort store what it prints over the
    packed one."""
    s, d, samples = world
    packed, _ = _two_step(d, samples, [], "append")
    first, last, full = _manifest(d, samples[:2], "first.tsv"), _manifest(d, samples[2:], "last.tsv"), _manifest(d, samples, "full.tsv")
    assert run(COUNT, ["-s", "sites.fa", "--cohort", first, "--store", "two_runs"], d).returncode == 0
    p = run(COUNT, ["-s", "sites.fa", "--cohort", last, "--store", "two_runs"], d)
    assert p.returncode == 0 and p.stdout.startswith(b"three.txt\t") and p.stdout.count(b"\n") == 1
    assert run("cmp", ["two_runs", packed], d).returncode == 0
    assert run(COUNT, ["-s", "sites.fa", "--cohort", first, "--store", "resumed"], d).returncode == 0
    two = open(os.path.join(str(d), "resumed"), "rb").read()
    p = run(COUNT, ["-s", "sites.fa", "--cohort", full, "--store", "resumed"], d)                 # without --resume: refused, untouched
    assert p.returncode == 1 and b"already in the store" in p.stderr and open(os.path.join(str(d), "resumed"), "rb").read() == two
    p = run(COUNT, ["-s", "sites.fa", "--cohort", full, "--store", "resumed", "--resume"], d)
    assert p.returncode == 0 and p.stdout.startswith(b"three.txt\t") and p.stdout.count(b"\n") == 1
    assert run("cmp", ["resumed", packed], d).returncode == 0
    p = run(COUNT, ["-s", "sites.fa", "--cohort", full, "--store", "resumed", "--resume"], d)     # nothing left to do
    assert p.returncode == 0 and p.stdout == b"" and run("cmp", ["resumed", packed], d).returncode == 0
    assert not os.path.exists(os.path.join(str(d), "one.txt"))                                     # no --counts, no NAME
    a, b = run(EVAL, ["-a", "--within", "two_runs"], d), run(EVAL, ["-a", "--within", packed], d)
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout and a.stdout.count(b"\n") >= 4
