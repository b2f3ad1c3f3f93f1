"""ntsmVCF --rotation (-R / -n / -M): the panel VCF to centre file, rotation and components in one run, and the layers
under it -- the expansion kernel of ntsm_amd/csrc/ntsm_pca.hip (cells of ntsm_vcf_run -> the PCA's padded matrix) and the
*_cells entry points of include/ntsm_pca_hip.h (ntsm_amd.pca.expand_cells / gram_cells / run_cells).

The yardstick of the program is the two-program route it replaces: `ntsmVCF -p A`, then `ntsmPCA -m A_matrix.tsv`, byte
for byte (ntsmPCA itself is held to scikit-learn by tests/test_pca.py).  The yardstick of the kernel is a numpy model on
the bits of the doubles.

CPU: the flag errors, the refusals that need no device, the wrappers' argument checks, and the prediction -- from the
fixtures' own matrices -- of which golden cases pass ntsmPCA's rank test.  Everything else needs the device."""
import glob
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_binding import ROOT  # noqa: E402
from test_pca import CASES as PCA_CASES, case_golden, golden_bounds, read_table  # noqa: E402
from test_vcf import CASES as VCF_CASES, GOLD as VCF_GOLD, cohort, strip_time  # noqa: E402

VCF = os.path.join(ROOT, "build", "ntsmVCF")
PCA = os.path.join(ROOT, "build", "ntsmPCA")
EVAL = os.path.join(ROOT, "build", "ntsmEval")
SUFFIXES = ("_matrix.tsv", "_center.txt", "_rotationalMatrix.tsv", "_components.tsv")
NO_DEVICE = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")

# The golden VCF cases that take the "both programs exit 0" branch with D = min(3, samples, sites), predicted from their
# recorded matrices (test_golden_cases_predicted_to_pass_the_rank_test): 7, where the plan of this feature hoped for at
# least 8.  The six cases with 3 sites (undef_then_third, site_absent, multi128, multi200, k15_w21, k11_w41_shared) have a
# centred matrix of rank 2 -- their third eigenvalue is below 1e-15 of the first -- so ntsmPCA refuses component 2 and the
# fused run has to refuse in the same words; zero_samples is refused for its header.  The cases below MUST succeed on
# both routes; for the others the test only demands that the two routes agree.
MUST_SUCCEED = ("plain", "overlap_dupes", "genotypes_crlf", "chrom_end_lower_nonl", "ref_alt_rules", "trailing_tab_body",
                "trailing_tab_header_body")


def files(prefix):
    return [open(prefix + s, "rb").read() if os.path.exists(prefix + s) else None for s in SUFFIXES]


def call(exe, args, cwd, env=None):
    return subprocess.run([exe] + args, cwd=str(cwd), capture_output=True, timeout=600, env=env)


def error_line(err):
    lines = err.splitlines()
    return lines[-1] if lines else b""


# ---------------------------------------------------------------------------------------------------- CPU
def test_flag_errors(built, tmp_path):
    """-R needs -p, -n and -M need -R, -n 0 is ntsmPCA's refusal; an unparsable -n is an error too.  Exit status 1 and
    nothing written, with no device in sight."""
    d = os.path.join(VCF_GOLD, "plain")
    out = tmp_path / "out"
    out.mkdir()
    common = ["-s", "sites.fa", "-r", "genome.fa"]
    prefix = str(out / "o")
    for args, msg in ((["-R"], b"Error: -R needs -p\nTry '--help' for more information.\n"),
                      (["-n", "5", "-p", prefix], b"Error: -n needs -R\nTry '--help' for more information.\n"),
                      (["-M", "-p", prefix], b"Error: -M needs -R\nTry '--help' for more information.\n"),
                      (["-R", "-n", "0", "-p", prefix], b"Error: -n 0: the number of components must be at least 1\n"),
                      (["-R", "-n", "2x", "-p", prefix], b"Error - Invalid parameter n: 2x\nTry '--help' for more information.\n"),
                      (["--rotation", "--dims", "-1", "--no-matrix", "--pca", prefix],
                       b"Error: -n -1: the number of components must be at least 1\n")):
        p = call(VCF, common + args + ["in.vcf"], d, env=NO_DEVICE)
        assert p.returncode == 1 and p.stderr == msg and p.stdout == b"", (args, p.stderr)
        assert os.listdir(str(out)) == [], args
    p = call(VCF, ["-h"], d)
    assert p.returncode == 0 and b"--rotation" in p.stderr and b"--dims" in p.stderr and b"--no-matrix" in p.stderr


@pytest.mark.parametrize("case,args,text", [
    ("plain", ["-R", "-n", "7"], "-n 7 is more than min(samples, sites) = min(6, 6)"),
    ("zero_samples", ["-R"], "the header of %s_matrix.tsv names 0 sample(s); a PCA needs at least 2")],
    ids=["plain_n7", "zero_samples"])
def test_refusals_before_the_device(built, tmp_path, case, args, text):
    """What ntsmPCA refuses from the shape of the matrix, in its words (it names the matrix file: the one this run would
    have written), exit status 1, nothing written, and no device touched (none is visible)."""
    prefix = str(tmp_path / "o")
    p = call(VCF, ["-s", "sites.fa", "-r", "genome.fa", "-p", prefix] + args + ["in.vcf"], os.path.join(VCF_GOLD, case), env=NO_DEVICE)
    want = "Error: " + (text % prefix if "%s" in text else text) + "\n"
    assert p.returncode == 1 and p.stderr.decode() == want and p.stdout == b"", p.stderr
    assert os.listdir(str(tmp_path)) == []


def test_wrappers_refuse_bad_arguments(built):
    """ntsm_amd.pca.expand_cells / run_cells: the ABI's argument checks come before any device call"""
    import ntsm_amd.pca as pca
    cells = np.ones((4, 3), dtype=np.uint16)
    value = np.zeros((2, 65536))
    fill = np.zeros(4)
    for c, v, f in ((None, value, fill), (cells, None, fill), (cells, value, None)):         # null pointers
        with pytest.raises(RuntimeError, match="ntsm_pca_expand_cells failed: -1$"):
            pca.expand_cells(c, v, f, shape=(4, 3))
        with pytest.raises(RuntimeError, match="ntsm_pca_run_cells failed: -1$"):
            pca.run_cells(c, v, f, 2, shape=(4, 3))
    with pytest.raises(RuntimeError, match="ntsm_pca_run_cells failed: -1$"):               # n < 2
        pca.run_cells(np.ones((4, 1), dtype=np.uint16), value, fill, 1)
    for d in (0, 4, 5):                                                                     # d < 1, d > n
        with pytest.raises(RuntimeError, match="ntsm_pca_run_cells failed: -1$"):
            pca.run_cells(cells, value, fill, d)
    with pytest.raises(RuntimeError, match="ntsm_pca_run_cells failed: -1$"):               # d > p
        pca.run_cells(np.ones((2, 3), dtype=np.uint16), value, np.zeros(2), 3)
    with pytest.raises(ValueError):
        pca.expand_cells(np.ones(5, dtype=np.uint16), value, fill)
    with pytest.raises(ValueError):
        pca.expand_cells(cells, np.zeros((2, 256)), fill)
    with pytest.raises(ValueError):
        pca.run_cells(cells, value, np.zeros(3), 2)


def test_golden_cases_predicted_to_pass_the_rank_test():
    """MUST_SUCCEED, confirmed from the fixtures' recorded matrices with numpy: each of those cases has its D-th centred
    eigenvalue at least 1e-3 of the first (ntsmPCA's refusal threshold is n eps l_1, below 2e-15 l_1 here), every other case
    with 2 or more samples has it below 1e-12 of the first (zero but for the rounding of this LAPACK: nothing in between), and
    plain is among them.  The seeded cohort's own rank is
    pinned by tests/golden/pca (vcf_cohort_19_digits, d = 5)."""
    passing = []
    for case in VCF_CASES:
        names, a, _ = read_table(os.path.join(VCF_GOLD, case["name"], "expected_matrix.tsv"))
        if a.size == 0 or a.shape[1] < 2:
            continue
        p, n = a.shape
        d = min(3, n, p)
        ac = a - a.mean(axis=1, keepdims=True)
        l = np.sort(np.linalg.eigvalsh(ac.T @ ac))[::-1]
        if l[d - 1] > 1e-3 * l[0]:
            passing.append(case["name"])
        else:
            assert l[d - 1] < 1e-12 * l[0], (case["name"], l[:d])
    assert tuple(passing) == MUST_SUCCEED and "plain" in passing and len(passing) == 7


# ---------------------------------------------------------------------------------------------------- GPU: the kernel
SHAPES = [(1, 2), (3, 7), (15, 16), (16, 127), (17, 128), (33, 129), (5, 1031), (100, 4113), (2049, 3)]


def byte_codes(multi):
    """The non-zero cell codes maxREF | maxVAR << 8 that -m multi allows: bytes 0, (uint8) m, (uint8) 2m"""
    b = sorted({0, multi & 255, (2 * multi) & 255})
    return np.array([r | v << 8 for r in b for v in b if r + v], dtype=np.uint16)


def random_bits(rng, size):
    """Doubles as random bit patterns (infinities, NaNs and subnormals as they fall), every eighth a NaN with a random
    payload, quiet or signalling: the comparison is on the bits"""
    x = np.frombuffer(rng.bytes(8 * int(np.prod(size))), dtype=np.uint64).copy()
    x[::8] = np.uint64(0x7FF0000000000000) | (x[::8] & np.uint64(0x800FFFFFFFFFFFFF)) | np.uint64(1)
    return x.reshape(size)


def expand_model(cells, value_bits, fill_bits, first):
    """Table look-up by code; the long form strictly after first_undef_cell; row_fill where the code is 0 -- on uint64"""
    p, n = cells.shape
    lin = np.arange(p * n, dtype=np.uint64).reshape(p, n)
    form = np.zeros((p, n), dtype=np.intp) if first is None else (lin > np.uint64(first)).astype(np.intp)
    out = value_bits[form, cells.astype(np.intp)]
    return np.where(cells == 0, fill_bits[:, None], out)


def first_choices(p, n):
    """none; 0; the last cell; the last cell of a row; the first cell of a row; one index in the middle"""
    return [None, 0, p * n - 1, (p // 2 + 1) * n - 1, (p // 2) * n, (p * n) // 2 + (1 if n > 2 else 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("p,n", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_expand_kernel_value_for_value(built, p, n):
    """ntsm_pca_expand against the model, bit for bit: an odd row stride, a row shorter than one 16-byte store, both sides
    of the 128-sample and 16-site padding edges, several workgroups per row and several rows per workgroup; every kind of
    first_undef_cell; the codes of -m 20, 128 (2m & 255 == 0) and 200 with code 0 in 0 %, 5 % and all of the cells; table
    entries and fills random bit patterns, NaN payloads included, so a wrong index cannot give the right value."""
    import ntsm_amd.pca as pca
    rng = np.random.default_rng(100000 * p + n)
    for multi in (20, 128, 200):
        codes = byte_codes(multi)
        for share in (0.0, 0.05, 1.0):
            cells = codes[rng.integers(0, len(codes), size=(p, n))]
            cells[rng.random((p, n)) < share] = 0
            if share == 1.0:
                cells[:] = 0
            value_bits = random_bits(rng, (2, 65536))
            fill_bits = random_bits(rng, (p,))
            for first in first_choices(p, n):
                got, ms = pca.expand_cells(cells, value_bits.view(np.float64), fill_bits.view(np.float64), first)
                want = expand_model(cells, value_bits, fill_bits, first)
                bad = np.argwhere(got.view(np.uint64) != want)
                assert bad.size == 0, (multi, share, first, bad[:5].tolist())
                assert ms > 0


def finite_inputs(rng, p, n, multi=20, share=0.05):
    codes = byte_codes(multi)
    cells = codes[rng.integers(0, len(codes), size=(p, n))]
    cells[rng.random((p, n)) < share] = 0
    return cells, rng.random((2, 65536)), rng.random(p), (p * n) // 3


@pytest.mark.gpu
def test_expand_writes_zero_padding(built):
    """33 x 129: the padded buffer is [48][256], so 127 padding columns per row and 15 padding rows.  The Gram matrix and
    the means of the cell route (ntsm_pca_gram_cells: expansion, centre, Gram tiles on the device buffer) equal pca.gram
    on the expanded matrix (upload into a zeroed buffer) bit for bit, centred and not: a non-zero padding cell changes G.
    Through run_cells (centre implied) the eigenvalues, rotation and components equal pca.run's on the same matrix.  Before
    either, a call on a larger shape leaves non-zero bytes behind in the memory the allocator hands out again."""
    import ntsm_amd.pca as pca
    rng = np.random.default_rng(33129)
    pca.expand_cells(*finite_inputs(rng, 100, 300)[:3])
    cells, value, fill, first = finite_inputs(rng, 33, 129)
    a, _ = pca.expand_cells(cells, value, fill, first)
    for centre in (True, False):
        g, means, _ = pca.gram(a, centre=centre)
        g2, means2, _ = pca.gram_cells(cells, value, fill, first, centre=centre)
        assert g.tobytes() == g2.tobytes() and means.tobytes() == means2.tobytes(), centre
    l, v, t, _ = pca.run(a, 3)
    l2, v2, t2, _, _ = pca.run_cells(cells, value, fill, 3, first)
    assert (l.tobytes(), v.tobytes(), t.tobytes()) == (l2.tobytes(), v2.tobytes(), t2.tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("p,n,d", [(300, 40, 5), (17, 128, 3)], ids=["300x40_d5", "17x128_d3"])
def test_run_cells_equals_run(built, p, n, d):
    """The contract of include/ntsm_pca_hip.h: run_cells returns the bits of run on expand_cells' matrix (same split, same
    process), also with a forced split."""
    import ntsm_amd.pca as pca
    rng = np.random.default_rng(1000 * p + n)
    cells, value, fill, first = finite_inputs(rng, p, n)
    a, _ = pca.expand_cells(cells, value, fill, first)
    for split in (0, 2):
        l, v, t, tm = pca.run(a, d, split=split)
        l2, v2, t2, tm2, ms = pca.run_cells(cells, value, fill, d, first, split=split)
        assert (l.tobytes(), v.tobytes(), t.tobytes()) == (l2.tobytes(), v2.tobytes(), t2.tobytes()), split
        assert tm2.gram_split == tm.gram_split and tm2.gram_flops == tm.gram_flops and ms > 0 and tm2.upload_ms > 0


# ---------------------------------------------------------------------------------------------------- GPU: the program
def two_routes(common, vcf, d, cwd, tmp, threads=None):
    """`ntsmVCF -p A` then `ntsmPCA -m A_matrix.tsv -p A -n d`, and `ntsmVCF -R -n d -p B`.  Returns True where the first
    route ran through (then B's four files and stderr are A's), False where a step refused (then B refused alike)."""
    a, b = str(tmp / "A"), str(tmp / "B")
    t = ["-t", str(threads)] if threads else []
    pv = call(VCF, common + t + ["-p", a, vcf], cwd)
    pp = call(PCA, ["-m", a + "_matrix.tsv", "-p", a, "-n", str(d)] + t, cwd) if pv.returncode == 0 else None
    pf = call(VCF, common + t + ["-R", "-n", str(d), "-p", b, vcf], cwd)
    if pv.returncode == 0 and pp.returncode == 0:
        assert pf.returncode == 0, pf.stderr[-500:]
        want, got = files(a), files(b)
        assert None not in want
        for w, g, s in zip(want, got, SUFFIXES):
            assert g == w, s
        assert strip_time(pf.stderr) == strip_time(pv.stderr)
        assert pf.stderr.splitlines()[-1].startswith(b"Time: ")
        return True
    refused = pv if pv.returncode != 0 else pp
    want = error_line(refused.stderr).replace(a.encode(), b.encode())
    assert want.startswith(b"Error: ")
    assert pf.returncode == 1 and error_line(pf.stderr) == want, (pf.stderr[-500:], want)
    assert files(b) == [None] * 4
    return False


@pytest.mark.gpu
@pytest.mark.parametrize("case", VCF_CASES, ids=[c["name"] for c in VCF_CASES])
def test_program_equals_two_programs_on_the_fixtures(built, tmp_path, case):
    """Every case of tests/golden/vcf with D = min(3, samples, sites): the four files and stderr of the two-program route,
    or its refusal (the header of zero_samples; component 2 of the rank-2 cases).  The cases of MUST_SUCCEED run through."""
    d_case = os.path.join(VCF_GOLD, case["name"])
    n = len(open(os.path.join(d_case, "expected_matrix.tsv")).readline().rstrip("\r\n").split("\t")) - 1
    p = open(os.path.join(d_case, "expected_matrix.tsv")).read().count("\n") - 1
    through = two_routes(["-s", "sites.fa", "-r", "genome.fa"] + case["args"], "in.vcf", max(1, min(3, n, p)), d_case, tmp_path)
    assert through or case["name"] not in MUST_SUCCEED
    if case["name"] == "zero_samples":
        assert not through


def all_missing(vcf, which):
    """Rewrite the genotypes of every line of the which-th SNP of the VCF as ./. ; returns the SNP's id"""
    lines = open(vcf).read().split("\n")
    body = [i for i, l in enumerate(lines) if l and not l.startswith("#")]
    rs = lines[body[which]].split("\t")[2]
    for i in body:
        f = lines[i].split("\t")
        if f[2] == rs:
            lines[i] = "\t".join(f[:9] + ["./."] * (len(f) - 9))
    with open(vcf, "w", newline="") as f:
        f.write("\n".join(lines))
    return rs


COHORTS = [("seeded_19_digits", 40300, 40, 300, ["-d", "-m", "3"], 5, False), ("130_samples", 130, 130, 250, ["-d"], 3, False),
           ("undefined_row_m128", 4040, 40, 300, ["-m", "128"], 3, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,seed,n,snps,args,d,missing", COHORTS, ids=[c[0] for c in COHORTS])
def test_program_equals_two_programs_on_cohorts(built, tmp_path, name, seed, n, snps, args, d, missing):
    """Seeded cohorts: the one of tests/golden/pca (40 samples, 300 SNPs, -d -m 3, d = 5: thirds, so 19-digit cells after
    the first site the VCF lacks); 130 samples (a second 128-sample tile); and 40 samples under -m 128 with one SNP's
    genotypes all ./. (SNPs at least 2k apart, so no other line touches its k-mers) -- the reference reads ./. as hom1, and
    with 2m & 255 == 0 a hom1 or hom2 cell has both bytes 0, so that SNP's whole row is undefined and the other rows hold defined cells before an undefined one (short form), the
    undefined ones (the row's centre) and defined cells after (long form) side by side."""
    rng = np.random.default_rng(seed)
    g, s, v = cohort(tmp_path, rng, n, snps, dense=not missing)
    if missing:
        rs = all_missing(v, 7)
    assert two_routes(["-s", s, "-r", g] + args, v, d, tmp_path, tmp_path, threads=4)
    names, a, texts = read_table(str(tmp_path / "A_matrix.tsv"))
    assert a.shape[1] == n
    if name == "seeded_19_digits":
        assert any(len(x) >= 19 for x in texts)
    if missing:
        centre = open(str(tmp_path / "A_center.txt")).read().split("\n")
        k = names.index(rs)
        assert texts[k * n:(k + 1) * n] == [centre[k]] * n                               # the whole row is its centre
        mixed = [i for i in range(len(names)) if 0 < sum(x == centre[i] for x in texts[i * n:(i + 1) * n]) < n and i != k]
        assert mixed                                                                    # rows with defined and undefined cells


@pytest.fixture(scope="module")
def seeded(built, tmp_path_factory):
    """The seeded cohort and one fused run of it: (dir, common args, vcf, the four files of `-R -n 5 -t 3`)"""
    tmp = tmp_path_factory.mktemp("vcf_rotation")
    g, s, v = cohort(tmp, np.random.default_rng(40300), 40, 300)
    common = ["-s", s, "-r", g, "-d", "-m", "3", "-R", "-n", "5"]
    p = call(VCF, common + ["-t", "3", "-p", str(tmp / "t3"), v], tmp)
    assert p.returncode == 0, p.stderr[-500:]
    return tmp, common, v, files(str(tmp / "t3"))


@pytest.mark.gpu
def test_same_bytes_for_every_t_and_from_gzip(seeded):
    tmp, common, v, want = seeded
    assert None not in want
    with open(v + ".gz", "wb") as f:
        f.write(gzip.compress(open(v, "rb").read(), 6))
    for prefix, vcf, t in (("t1", v, "1"), ("t16", v, "16"), ("gz", v + ".gz", "5")):
        p = call(VCF, common + ["-t", t, "-p", str(tmp / prefix), vcf], tmp)
        assert p.returncode == 0, p.stderr[-500:]
        assert files(str(tmp / prefix)) == want, prefix


@pytest.mark.gpu
def test_no_matrix(seeded):
    """-M: no NAME_matrix.tsv; the other three files are those of the run that writes it.  -v adds the PCA's lines."""
    tmp, common, v, want = seeded
    p = call(VCF, common + ["-M", "-v", "-t", "3", "-p", str(tmp / "nomatrix"), v], tmp)
    assert p.returncode == 0, p.stderr[-500:]
    got = files(str(tmp / "nomatrix"))
    assert got[0] is None and got[1:] == want[1:]
    assert sorted(os.path.basename(f) for f in glob.glob(str(tmp / "nomatrix*"))) == ["nomatrix" + s for s in sorted(SUFFIXES[1:])]
    err = p.stderr.decode()
    assert "Matrix: " in err and "[pca] device: upload " in err and " expand " in err and err.splitlines()[-1].startswith("Time: ")


@pytest.mark.gpu
def test_rank_refusal_names_the_component(built, tmp_path):
    """After the eigen step: ntsmPCA's words, exit status 1, nothing written -- the matrix and the centre file neither.
    site_absent has 3 sites of which one is absent from the VCF: the centred matrix has rank 2."""
    prefix = str(tmp_path / "o")
    p = call(VCF, ["-s", "sites.fa", "-r", "genome.fa", "-R", "-n", "3", "-p", prefix, "in.vcf"], os.path.join(VCF_GOLD, "site_absent"))
    assert p.returncode == 1 and error_line(p.stderr).startswith(b"Error: component 2 of the 3 requested has no positive eigenvalue"), p.stderr
    assert os.listdir(str(tmp_path)) == []
    p = call(VCF, ["-s", "sites.fa", "-r", "genome.fa", "-R", "-n", "2", "-p", prefix, "in.vcf"], os.path.join(VCF_GOLD, "site_absent"))
    assert p.returncode == 0 and None not in files(prefix)


@pytest.mark.gpu
def test_against_scikit_learn(built, tmp_path):
    """The fused run's rotation and components on tests/golden/vcf/plain (d = 3) inside golden_bounds of
    tests/golden/pca/vcf_plain: the gate test_pca.py's test_cli_against_the_goldens applies to ntsmPCA."""
    case = next(c for c in PCA_CASES if c["name"] == "vcf_plain")
    d = case["d"]
    prefix = str(tmp_path / "o")
    p = call(VCF, ["-s", "sites.fa", "-r", "genome.fa", "-R", "-n", str(d), "-p", prefix, "in.vcf"], os.path.join(VCF_GOLD, "plain"))
    assert p.returncode == 0, p.stderr[-500:]
    sites, a, _ = read_table(prefix + "_matrix.tsv")
    rot_names, rot, _ = read_table(prefix + "_rotationalMatrix.tsv")
    comp_names, comp, _ = read_table(prefix + "_components.tsv")
    assert rot_names == sites and comp_names == open(prefix + "_matrix.tsv").readline().rstrip("\n").split("\t")[1:]
    g_rot, g_comp = case_golden(case)
    bound, l = golden_bounds(a, d)
    for i in range(d):
        err_v, err_t = np.abs(rot[:, i] - g_rot[:, i]).max(), np.abs(comp[:, i] - g_comp[:, i]).max()
        print("component %d: bound %.3g  rotation %.3g  components: bound %.3g  %.3g" % (i, bound[i], err_v, bound[i] * np.sqrt(l[i]), err_t))
        assert err_v <= bound[i]
        assert err_t <= bound[i] * np.sqrt(l[i])


@pytest.mark.gpu
def test_chain_into_ntsmEval(built, tmp_path):
    """ntsmVCF -R -> ntsmEval -p B_rotationalMatrix.tsv -n B_center.txt reports the pairs that the chain through ntsmPCA
    reports: the construction is test_pca.py's chain test itself, run here into tmp_path (it asserts that those are
    exactly the planted pairs); its inputs and counts files then serve the fused run."""
    from test_pca import test_chain_vcf_pca_eval_finds_planted_duplicates as through_ntsmpca
    through_ntsmpca(built, tmp_path)
    counts = sorted(glob.glob(str(tmp_path / "s[0-9][0-9][0-9].txt")))
    assert len(counts) == 24
    a, b = str(tmp_path / "port"), str(tmp_path / "fused")
    p = call(VCF, ["-s", str(tmp_path / "sites.fa"), "-r", str(tmp_path / "genome.fa"), "-R", "-t", "4", "-p", b, str(tmp_path / "in.vcf")], tmp_path)
    assert p.returncode == 0, p.stderr[-500:]
    assert files(b) == files(a)

    def pairs(prefix):
        q = call(EVAL, ["-p", prefix + "_rotationalMatrix.tsv", "-n", prefix + "_center.txt"] + counts, tmp_path)
        assert q.returncode == 0, q.stderr[-500:]
        return {tuple(sorted(l.split("\t")[:2])) for l in q.stdout.decode().splitlines()[1:]}

    got = pairs(b)
    assert got == pairs(a) and got == {tuple(sorted((counts[j], counts[16 + j]))) for j in range(8)}
