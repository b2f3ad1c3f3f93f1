"""ntsmPCA (build/ntsmPCA, ntsm_amd/pca.py): the exact PCA rotation of the matrix ntsmVCF writes.

CPU: the refusals, and the fixtures under tests/golden/pca re-derived from their recipe (pandas + scikit-learn's full
solver) where those are importable.  GPU: the Gram kernel bit for bit on integer matrices, the program against the
fixtures and against gap-free identities inside bounds derived from the rounding of a length-p dot product, determinism,
the text form, and the chain ntsmVCF -> ntsmPCA -> ntsmEval -p -n.
"""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle_binding import ROOT  # noqa: E402

PCA = os.path.join(ROOT, "build", "ntsmPCA")
VCF = os.path.join(ROOT, "build", "ntsmVCF")
EVAL = os.path.join(ROOT, "build", "ntsmEval")
GOLDEN = os.path.join(ROOT, "tests", "golden")
GOLD = os.path.join(GOLDEN, "pca")
CASES = json.load(open(os.path.join(GOLD, "cases.json")))
U = 2.0 ** -53                                                                   # unit roundoff of IEEE double


# ---------------------------------------------------------------------------------------------------- inputs
def cell_text(x):
    """A cell as ntsmVCF prints it: the short forms, anything else at 19 significant digits."""
    return "%.19g" % x


def write_matrix(path, a, gz=False, sites=None, samples=None):
    p, n = a.shape
    sites = sites or ["rs%d" % k for k in range(p)]
    samples = samples or ["HG%05d" % j for j in range(n)]
    text = "alleleID\t" + "\t".join(samples) + "\n"
    text += "".join("%s\t%s\n" % (sites[k], "\t".join(cell_text(x) for x in a[k])) for k in range(p))
    data = text.encode()
    with open(path, "wb") as f:
        f.write(gzip.compress(data, 6, mtime=0) if gz else data)
    return path


def structured_cohort(seed, n, p, pops, thirds=0.0):
    """[p sites][n samples] of REF fractions 0 / 0.5 / 1: `pops` populations whose allele frequencies drift from a common
    ancestral one, genotypes binomial; a share `thirds` of the cells replaced by 1/3 or 2/3 (19-digit cells)."""
    rng = np.random.default_rng(seed)
    anc = rng.uniform(0.05, 0.95, size=p)
    freq = np.clip(anc[:, None] + rng.normal(0.0, 0.12, size=(p, pops)), 0.01, 0.99)
    pop = np.arange(n) % pops
    a = rng.binomial(2, freq[:, pop]) / 2.0
    if thirds:
        mask = rng.random((p, n)) < thirds
        a[mask] = rng.integers(1, 3, size=int(mask.sum())) / 3.0
    return a


def case_matrix(case, tmp):
    """The matrix file of a fixture: committed, or generated from the case's seed into tmp."""
    if case.get("matrix"):
        return os.path.join(GOLDEN, case["matrix"])
    g = case["generate"]
    return write_matrix(os.path.join(str(tmp), case["name"] + "_matrix.tsv"), structured_cohort(g["seed"], g["n"], g["p"], g["pops"], g.get("thirds", 0.0)))


def read_table(path):
    """(row names, values float64 [rows][cols], the number texts) of a matrix / rotation / components file"""
    opener = gzip.open if open(path, "rb").read(2) == b"\x1f\x8b" else open
    with opener(path, "rt") as f:
        lines = f.read().split("\n")
    assert lines[-1] == ""
    rows = [l.split("\t") for l in lines[1:-1]]
    return [r[0] for r in rows], np.array([[float(x) for x in r[1:]] for r in rows], dtype=np.float64), [x for r in rows for x in r[1:]]


def case_golden(case):
    """(rotation [p][d], components [n][d]) of a fixture: gzip'd little-endian float64"""
    d = os.path.join(GOLD, case["name"])
    load = lambda name: np.frombuffer(gzip.decompress(open(os.path.join(d, name), "rb").read()), dtype="<f8").reshape(-1, case["d"])  # noqa: E731
    return load("rotation.f8.gz"), load("components.f8.gz")


def sklearn_recipe(matrix, d):
    """What the fixtures are: pandas reads the matrix (sites x samples), scikit-learn's exact solver is fitted on the
    samples.  Returns (rotation frame [site][d], components frame [sample][d])."""
    import pandas as pd
    from sklearn.decomposition import PCA as SkPCA
    frame = pd.read_csv(matrix, sep="\t", index_col=0, float_precision="round_trip")
    model = SkPCA(n_components=d, svd_solver="full")
    scores = model.fit_transform(frame.values.T)
    return pd.DataFrame(model.components_.T, index=frame.index), pd.DataFrame(scores, index=frame.columns)


def fix_signs(v, t):
    """The sign rule: the entry of each column of v with the largest magnitude (the first on a tie) is positive"""
    k = np.argmax(np.abs(v), axis=0)
    s = np.where(v[k, np.arange(v.shape[1])] < 0, -1.0, 1.0)
    return v * s, t * s


def numpy_model(a, d, gram_dtype=np.float64):
    """The method in numpy: Gram matrix of the centred matrix (in gram_dtype), eigh, projection.  (l, v, t)"""
    ac = a - a.mean(axis=1, keepdims=True)
    x = ac.astype(gram_dtype)
    g = (x.T @ x).astype(np.float64)
    l, u = np.linalg.eigh(g)
    l, u = l[::-1][:d], u[:, ::-1][:, :d]
    s = np.sqrt(l)
    v, t = fix_signs(ac @ u / s, u * s)
    return l, v, t


def golden_bounds(a, d):
    """Per component, p u trace(G) / gap_i: first-order perturbation of an eigenvector of G under the standard
    summation-error bound of the length-p dot products that make G (|dG| <= p u trace(G) in norm), gap_i the distance
    from l_i to its nearest other eigenvalue.  Everything from the input with numpy.  (bounds [d], eigenvalues [n])"""
    p = a.shape[0]
    ac = a - a.mean(axis=1, keepdims=True)
    g = ac.T @ ac
    l = np.sort(np.linalg.eigvalsh(g))[::-1]
    gap = np.array([np.min(np.abs(np.delete(l, i) - l[i])) for i in range(d)])
    return p * U * np.trace(g) / gap, l


def run_pca(args, cwd):
    return subprocess.run([PCA] + args, cwd=str(cwd), capture_output=True, timeout=900)


def outputs(cwd, prefix=""):
    return [os.path.join(str(cwd), prefix + s) for s in ("_rotationalMatrix.tsv", "_components.tsv")]


# ---------------------------------------------------------------------------------------------------- CPU
def refusal_inputs(tmp):
    w = lambda name, text: open(os.path.join(str(tmp), name), "w", newline="").write(text)  # noqa: E731
    w("ok.tsv", "alleleID\tA\tB\tC\nrs1\t0.5\t1\t0\nrs2\t0\t0.25\t1\n")
    w("empty.tsv", "")
    w("header_only.tsv", "alleleID\tA\tB\n")
    w("one_sample.tsv", "alleleID\tA\nrs1\t0.5\nrs2\t1\n")
    w("no_sample.tsv", "alleleID\nrs1\n")
    w("short_row.tsv", "alleleID\tA\tB\tC\nrs1\t0.5\t1\t0\nrs2\t0\t0.25\n")
    w("long_row.tsv", "alleleID\tA\tB\nrs1\t0.5\t1\nrs2\t0\t0.25\t1\n")
    w("blank_line.tsv", "alleleID\tA\tB\nrs1\t0.5\t1\n\nrs2\t0\t0.25\n")
    w("word.tsv", "alleleID\tA\tB\nrs1\t0.5\tx1\nrs2\t0\t0.25\n")
    w("empty_cell.tsv", "alleleID\tA\tB\nrs1\t0.5\t\nrs2\t0\t0.25\n")
    w("nan.tsv", "alleleID\tA\tB\nrs1\t0.5\tnan\nrs2\t0\t0.25\n")
    w("inf.tsv", "alleleID\tA\tB\nrs1\t0.5\t1\nrs2\t-inf\t0.25\n")
    w("overflow.tsv", "alleleID\tA\tB\nrs1\t0.5\t1e999\nrs2\t0\t0.25\n")
    w("trailing.tsv", "alleleID\tA\tB\nrs1\t0.5\t1 \nrs2\t0\t0.25\n")
    os.mkdir(os.path.join(str(tmp), "dir.tsv"))
    with open(os.path.join(str(tmp), "corrupt.tsv.gz"), "wb") as f:
        f.write(gzip.compress(b"alleleID\tA\tB\nrs1\t0.5\t1\nrs2\t0\t0.25\n" * 50)[:-12] + b"\0" * 12)


REFUSALS = [
    ("missing", ["-m", "nope.tsv"], "cannot read the matrix file nope.tsv"),
    ("directory", ["-m", "dir.tsv"], "cannot read the matrix file dir.tsv"),
    ("corrupt_gzip", ["-m", "corrupt.tsv.gz"], "cannot read the matrix file corrupt.tsv.gz"),
    ("empty", ["-m", "empty.tsv"], "the matrix file empty.tsv is empty"),
    ("header_only", ["-m", "header_only.tsv", "-n", "1"], "has no sites"),
    ("one_sample", ["-m", "one_sample.tsv", "-n", "1"], "names 1 sample(s); a PCA needs at least 2"),
    ("no_sample", ["-m", "no_sample.tsv", "-n", "1"], "names 0 sample(s); a PCA needs at least 2"),
    ("short_row", ["-m", "short_row.tsv", "-n", "1"], "line 3 of short_row.tsv (rs2): has 3 fields, the header has 4"),
    ("long_row", ["-m", "long_row.tsv", "-n", "1"], "line 3 of long_row.tsv (rs2): has 4 fields, the header has 3"),
    ("blank_line", ["-m", "blank_line.tsv", "-n", "1"], "line 3 of blank_line.tsv (): has 1 fields, the header has 3"),
    ("word", ["-m", "word.tsv", "-n", "1"], "line 2 of word.tsv (rs1): the cell of sample 2 is not a finite number: 'x1'"),
    ("empty_cell", ["-m", "empty_cell.tsv", "-n", "1"], "the cell of sample 2 is not a finite number: ''"),
    ("nan", ["-m", "nan.tsv", "-n", "1"], "the cell of sample 2 is not a finite number: 'nan'"),
    ("inf", ["-m", "inf.tsv", "-n", "1"], "line 3 of inf.tsv (rs2): the cell of sample 1 is not a finite number: '-inf'"),
    ("overflow", ["-m", "overflow.tsv", "-n", "1"], "the cell of sample 2 is not a finite number: '1e999'"),
    ("trailing_blank", ["-m", "trailing.tsv", "-n", "1"], "the cell of sample 2 is not a finite number: '1 '"),
    ("d_zero", ["-m", "ok.tsv", "-n", "0"], "-n 0: the number of components must be at least 1"),
    ("d_negative", ["-m", "ok.tsv", "-n", "-3"], "-n -3: the number of components must be at least 1"),
    ("d_above_sites", ["-m", "ok.tsv", "-n", "3"], "-n 3 is more than min(samples, sites) = min(3, 2)"),
    ("d_default_too_many", ["-m", "ok.tsv"], "-n 20 is more than min(samples, sites) = min(3, 2)"),
    ("first_bad_line_any_t", ["-m", "short_row.tsv", "-n", "1", "-t", "7"], "line 3 of short_row.tsv (rs2): has 3 fields"),
]


@pytest.mark.parametrize("name,args,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(built, tmp_path, name, args, msg):
    """Each refusal: "Error: ..." on stderr, exit status 1, nothing written -- all of them before the device is touched
    (HIP_VISIBLE_DEVICES hides every device: a program that reached the device step would report that instead)."""
    refusal_inputs(tmp_path)
    before = sorted(os.listdir(str(tmp_path)))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    p = subprocess.run([PCA] + args + ["-p", "out"], cwd=str(tmp_path), capture_output=True, env=env, timeout=120)
    err = p.stderr.decode()
    assert p.returncode == 1 and err.startswith("Error: ") and msg in err and err.count("\n") == 1, (p.returncode, err)
    assert p.stdout == b"" and sorted(os.listdir(str(tmp_path))) == before


def test_bad_cell_in_a_last_line_without_newline_names_its_line_for_every_t(built, tmp_path):
    """6 sites x 4 samples, no '\\n' after the last line, a bad cell in it: line 7, whether one thread reads the whole body or
    16 threads are cut more ranges than there are lines (the refusal comes before the device: every device is hidden)."""
    rows = ["rs%d\t0\t0.5\t1\t0.25" % k for k in range(5)] + ["rs5\t0\t0.5\tbad\t0.25"]
    with open(str(tmp_path / "m.tsv"), "w", newline="") as f:
        f.write("alleleID\tA\tB\tC\tD\n" + "\n".join(rows))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    for t in ("1", "16"):
        p = subprocess.run([PCA, "-m", "m.tsv", "-n", "2", "-t", t, "-p", "out"], cwd=str(tmp_path), capture_output=True, env=env, timeout=120)
        assert p.returncode == 1 and p.stdout == b"", t
        assert p.stderr == b"Error: line 7 of m.tsv (rs5): the cell of sample 3 is not a finite number: 'bad'\n", (t, p.stderr)
    assert sorted(os.listdir(str(tmp_path))) == ["m.tsv"]


def test_flag_errors(built, tmp_path):
    """Flag errors in ntsmVCF's style: the message, then "Try '--help' for more information.", exit status 1; --help and
    --version exit with 0; the long names are the upstream script's."""
    refusal_inputs(tmp_path)
    for args, msg in ((["-n", "2"], "Error: Need Input File (-m)"),
                      (["-m", "ok.tsv", "-n", "x"], "Error - Invalid parameter n: x"),
                      (["-m", "ok.tsv", "-n", "2x"], "Error - Invalid parameter n: 2x"),
                      (["-m", "ok.tsv", "-t", "many"], "Error - Invalid parameter t: many"),
                      (["-m", "ok.tsv", "-G", "z"], "Error - Invalid parameter G: z"),
                      (["-m", "ok.tsv", "-Q"], "invalid option -- 'Q'"),
                      (["-m", "ok.tsv", "stray"], "Error: Unexpected argument stray"),
                      (["-m"], "option requires an argument -- 'm'")):
        p = run_pca(args, tmp_path)
        err = p.stderr.decode()
        assert p.returncode == 1 and msg in err and err.endswith("Try '--help' for more information.\n"), (args, err)
        assert not any(f.endswith(("_rotationalMatrix.tsv", "_components.tsv")) for f in os.listdir(str(tmp_path)))
    for flag in ("-h", "--help", "--version"):
        p = run_pca([flag], tmp_path)
        assert p.returncode == 0 and b"ntsmPCA" in p.stderr
    # the long names parse: the refusal is the one of the value, not of the flag
    p = run_pca(["--matrix", "ok.tsv", "--numComp", "3", "--prefix", "x", "--threads", "2", "--gpu", "0"], tmp_path)
    assert p.returncode == 1 and b"-n 3 is more than min(samples, sites)" in p.stderr


def test_number_text_is_correctly_rounded_and_written_like_repr(built, tmp_path):
    """The program's two conversions (tests/pca_text_check.cpp around its own functions): a cell read with
    std::from_chars is Python's float() of the text, for short forms, 19-digit forms and repr forms; a value is written
    as Python's repr writes it, across the switch to exponent form below 1e-4 and at 1e16, subnormals and the largest
    double included."""
    exe = str(tmp_path / "pca_text_check")
    host = os.path.join(ROOT, "ntsm_amd", "csrc", "host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "pca_text_check.cpp")] +
                   [os.path.join(host, f) for f in ("inflate.cpp", "inflate_spec.cpp", "gz_stream.cpp", "gz_parallel.cpp", "crc32_fast.cpp")] +
                   ["-L" + os.path.join(ROOT, "ntsm_amd"), "-lntsm_pca_hip", "-lz", "-pthread", "-Wl,-rpath," + os.path.join(ROOT, "ntsm_amd"),
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    rng = np.random.default_rng(2)
    values = [0.0, -0.0, 1.0, 0.5, 1 / 3, 2 / 3, 1e16, 1.5e16, 9999999999999998.0, 1e15, 1e-4, 9.999e-5, 1e-5, 1.5e-5, 1e-100, 1e100,
              123456789.125, 5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, 0.1, -2.5e-7, 100.0, 123456789012345680.0]
    values += (rng.standard_normal(20000) * 10.0 ** rng.integers(-30, 30, 20000)).tolist()
    values += [v for v in np.frombuffer(rng.bytes(8 * 20000), dtype="<f8").tolist() if np.isfinite(v)]
    for form in (repr, lambda v: "%.19g" % v, lambda v: "%.18e" % v):
        texts = [form(v) for v in values]
        p = subprocess.run([exe], input="\n".join(texts) + "\n", capture_output=True, text=True, check=True)
        got = p.stdout.split("\n")[:-1]
        assert len(got) == len(values)
        bad = [(t, g, repr(float(t))) for t, g in zip(texts, got) if g != repr(float(t))]
        assert not bad, bad[:5]
    p = subprocess.run([exe], input="+1\n 1\n1 \n\nnan\ninf\n1e999\n0x10\n1,5\n", capture_output=True, text=True, check=True)
    assert p.stdout == "BAD\n" * 9


def test_wrapper_refuses_bad_arguments(built):
    """ntsm_amd.pca: the ABI's argument checks come before any device call"""
    import ntsm_amd.pca as pca
    a = np.zeros((4, 3))
    for d in (0, 4, 5):
        with pytest.raises(RuntimeError, match="-1"):
            pca.run(a, d)
    with pytest.raises(ValueError):
        pca.gram(np.zeros(5))
    import ctypes
    assert ctypes.sizeof(pca.Times) == 6 * 8 + 2 * 8 + 2 * 4                  # ntsm_pca_times of include/ntsm_pca_hip.h


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_goldens_follow_their_recipe(built, tmp_path, case):
    """The committed rotation and components are what pandas + scikit-learn's full solver give on the fixture's matrix
    today.  Another LAPACK build may round differently, so the comparison is the gate of the GPU test (golden_bounds),
    not byte equality; the float64 numpy model of the method passes the same gate and lies far inside it."""
    pytest.importorskip("sklearn")
    pytest.importorskip("pandas")
    assert os.path.exists(PCA)
    matrix = case_matrix(case, tmp_path)
    d = case["d"]
    rot, comp = sklearn_recipe(matrix, d)
    sites, a, _ = read_table(matrix)
    assert list(rot.index) == sites and rot.shape == (a.shape[0], d) and comp.shape == (a.shape[1], d)
    g_rot, g_comp = case_golden(case)
    bound, l = golden_bounds(a, d)
    _, v, t = numpy_model(a, d)
    for i in range(d):
        print(case["name"], i, "bound %.3g  recipe-golden %.3g  model-golden %.3g" %
              (bound[i], np.abs(rot.values[:, i] - g_rot[:, i]).max(), np.abs(v[:, i] - g_rot[:, i]).max()))
        assert np.abs(rot.values[:, i] - g_rot[:, i]).max() <= bound[i]
        assert np.abs(comp.values[:, i] - g_comp[:, i]).max() <= bound[i] * np.sqrt(l[i])
        assert np.abs(v[:, i] - g_rot[:, i]).max() <= bound[i]
        assert np.abs(t[:, i] - g_comp[:, i]).max() <= bound[i] * np.sqrt(l[i])
    for frame, name, label in ((rot, "rotationalMatrix.tsv", "AlleleID"), (comp, "components.tsv", "SampleID")):
        frame.to_csv(str(tmp_path / name), sep="\t", index_label=label)         # the header the program has to write
        assert open(str(tmp_path / name)).readline() == label + "".join("\t%d" % i for i in range(d)) + "\n"


# ---------------------------------------------------------------------------------------------------- GPU
def mirrored_integers(rng, p, n):
    """Cells in 0...8 whose row means are exactly 4: sample n - 1 - j holds 8 minus sample j's cell"""
    a = rng.integers(0, 9, size=(p, n))
    a[:, n - (n // 2):] = 8 - a[:, :n // 2][:, ::-1]
    if n % 2:
        a[:, n // 2] = 4
    return a


GRAM_SHAPES = [(5, 3, 0), (16, 128, 1), (33, 16, 0), (40, 127, 0), (40, 128, 0), (40, 129, 0), (1000, 300, 0), (1001, 200, 8),
               (333, 513, 3), (4099, 131, 0), (2, 2, 5), (48, 513, 0), (17, 640, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("p,n,split", GRAM_SHAPES, ids=["%dx%d_split%d" % s for s in GRAM_SHAPES])
def test_gram_is_exact_on_integers(built, p, n, split):
    """ntsm_pca_gram on integer matrices equals numpy's int64 product bit for bit, with the centring off (A^T A) and on
    (row means exactly 4): padding, one tile, a tile edge +/- 1, many tiles (the off-diagonal ones are not symmetric, so
    a transposed or wrongly mapped accumulator shows), a site split with a short last piece; 513 samples: a 5 x 5 tile
    grid (15 upper tiles) whose last tile has one live column; 640: five full tiles with p no multiple of 16 and a forced
    split."""
    import ntsm_amd.pca as pca
    rng = np.random.default_rng(1000 * p + n)
    a = mirrored_integers(rng, p, n)
    g, means, t = pca.gram(a.astype(np.float64), centre=False, split=split)
    assert np.array_equal(g, (a.T @ a).astype(np.float64))
    assert np.array_equal(means, np.full(p, 4.0))
    if split:
        chunks = (p + 15) // 16
        per = -(-chunks // min(split, chunks))
        assert t.gram_split == -(-chunks // per)
    assert t.gram_tiles == ((n + 127) // 128) * ((n + 127) // 128 + 1) // 2 and t.gram_flops == n * (n + 1) * p
    ac = a - 4
    g2, _, _ = pca.gram(a.astype(np.float64), centre=True, split=split)
    assert np.array_equal(g2, (ac.T @ ac).astype(np.float64))
    # any split gives the same sums here (they are exact), and the same bits on a second call
    g3, _, _ = pca.gram(a.astype(np.float64), centre=True, split=split)
    assert g3.tobytes() == g2.tobytes()


@pytest.mark.gpu
def test_gram_reports_a_refused_device_and_works_afterwards(built):
    """ntsm_pca_gram on a device ordinal that does not exist returns NTSM_PCA_E_HIP (hipSetDevice's error, no device
    fault), and the next call on device 0 gives the exact Gram matrix of a 2 x 2 matrix."""
    import ntsm_amd.pca as pca
    a = np.array([[1.0, 3.0], [6.0, 2.0]])
    with pytest.raises(RuntimeError, match=r"ntsm_pca_gram failed: %d$" % pca.E_HIP):
        pca.gram(a, device=1 << 20)
    g, means, _ = pca.gram(a, centre=False)
    assert g.tolist() == [[37.0, 15.0], [15.0, 13.0]] and means.tolist() == [2.0, 4.0]
    g, _, _ = pca.gram(a, centre=True)
    assert g.tolist() == [[5.0, -5.0], [-5.0, 5.0]]


@pytest.mark.gpu
def test_gram_of_real_cells_is_symmetric_and_repeatable(built):
    """Non-integer cells: G is symmetric bit for bit, two calls agree bit for bit, and it is the float64 product to the
    summation bound of the two products, 2 (p + 1) u |Ac|^T |Ac|."""
    import ntsm_amd.pca as pca
    a = structured_cohort(5, 203, 3001, 4, thirds=0.05)
    g, means, _ = pca.gram(a, centre=True)
    g2, _, _ = pca.gram(a, centre=True)
    assert g.tobytes() == g2.tobytes() and np.array_equal(g, g.T)
    assert np.abs(means - a.mean(axis=1)).max() <= 2 * (203 + 1) * U         # two sums of 203 cells <= 1, two divisions
    ac = a - means[:, None]                                                  # the device's own centred cells: one rounding each
    bound = 2 * (3001 + 1) * U * (np.abs(ac).T @ np.abs(ac))                # both products: gamma_p |Ac|^T |Ac| each
    assert (np.abs(g - ac.T @ ac) <= bound).all()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cli_against_the_goldens(built, tmp_path, case):
    """Per component, after the sign rule: max|v_i - v_i(golden)| <= p u trace(G) / gap_i, and the components inside the
    same bound times s_i; names and order of both files as the input has them."""
    matrix = case_matrix(case, tmp_path)
    d = case["d"]
    p = run_pca(["-m", matrix, "-n", str(d), "-p", "got", "-t", "4"], tmp_path)
    assert p.returncode == 0, p.stderr[-500:]
    sites, a, _ = read_table(matrix)
    samples = gzip.open(matrix, "rt").readline() if matrix.endswith(".gz") else open(matrix).readline()
    rot_names, rot, _ = read_table(outputs(tmp_path, "got")[0])
    comp_names, comp, _ = read_table(outputs(tmp_path, "got")[1])
    assert rot_names == sites and comp_names == samples.rstrip("\n").split("\t")[1:]
    for f, label in zip(outputs(tmp_path, "got"), ("AlleleID", "SampleID")):
        assert open(f).readline() == label + "".join("\t%d" % i for i in range(d)) + "\n"
    g_rot, g_comp = case_golden(case)
    bound, l = golden_bounds(a, d)
    _, v, _ = numpy_model(a, d)
    for i in range(d):
        err_v, err_t = np.abs(rot[:, i] - g_rot[:, i]).max(), np.abs(comp[:, i] - g_comp[:, i]).max()
        print("%s component %d: bound %.3g  device %.3g  numpy model %.3g  components: bound %.3g  device %.3g" %
              (case["name"], i, bound[i], err_v, np.abs(v[:, i] - g_rot[:, i]).max(), bound[i] * np.sqrt(l[i]), err_t))
        k = np.argmax(np.abs(rot[:, i]))
        assert rot[k, i] > 0
        assert err_v <= bound[i]
        assert err_t <= bound[i] * np.sqrt(l[i])


@pytest.fixture(scope="module")
def cohort_run(built, tmp_path_factory):
    """One run of the program on a generated cohort whose sizes are no multiples of 16: (dir, matrix path, a, d)"""
    tmp = tmp_path_factory.mktemp("pca_cohort")
    a = structured_cohort(77, 203, 3001, 5, thirds=0.03)
    matrix = write_matrix(str(tmp / "cohort_matrix.tsv"), a)
    p = run_pca(["-m", matrix, "-p", "run", "-t", "3"], tmp)
    assert p.returncode == 0, p.stderr[-500:]
    return tmp, matrix, a, 20


@pytest.mark.gpu
def test_gap_free_identities(cohort_run):
    """Orthonormality max|V^T V - I|, the residual max|Ac (Ac^T v_i) - l_i v_i| / l_1 and the components against the
    projection max|Ac^T v_i - t_i| / s_1, every reference quantity from the program's own input in float64 numpy, all
    inside p u sqrt(n) l_1 / l_D: the summation error of the length-p products times the amplification a Gram-matrix
    method has for a small eigenvalue."""
    tmp, matrix, a, d = cohort_run
    _, a_read, _ = read_table(matrix)
    assert np.array_equal(a_read, a)
    p, n = a.shape
    _, v, _ = read_table(outputs(tmp, "run")[0])
    _, t, _ = read_table(outputs(tmp, "run")[1])
    assert v.shape == (p, d) and t.shape == (n, d)
    ac = a - a.mean(axis=1, keepdims=True)
    l = np.sort(np.linalg.eigvalsh(ac.T @ ac))[::-1][:d]
    bound = p * U * np.sqrt(n) * l[0] / l[d - 1]
    orth = np.abs(v.T @ v - np.eye(d)).max()
    resid = np.abs(ac @ (ac.T @ v) - v * l).max() / l[0]
    proj = np.abs(ac.T @ v - t).max() / np.sqrt(l[0])
    print("gap-free: bound %.3g  orthonormality %.3g  residual %.3g  projection %.3g" % (bound, orth, resid, proj))
    assert orth <= bound and resid <= bound and proj <= bound


@pytest.mark.gpu
def test_text_form_is_pythons_repr(cohort_run):
    """Every number of both files is written as pandas writes it: repr(float(text)) == text; '\\n' line ends"""
    tmp, _, _, d = cohort_run
    for f in outputs(tmp, "run"):
        assert b"\r" not in open(f, "rb").read()
        _, values, texts = read_table(f)
        assert len(texts) == values.size and values.shape[1] == d
        bad = [x for x in texts if repr(float(x)) != x]
        assert not bad, bad[:5]


@pytest.mark.gpu
def test_same_bytes_every_run_every_t_and_from_gzip(cohort_run):
    """Two runs, -t 1 / -t 16 and a gzip'd matrix give the bytes of the module's -t 3 run"""
    tmp, matrix, _, _ = cohort_run
    want = [open(f, "rb").read() for f in outputs(tmp, "run")]
    gz = str(tmp / "cohort_matrix.tsv.gz")
    with open(gz, "wb") as f:
        f.write(gzip.compress(open(matrix, "rb").read(), 6))
    for prefix, args in (("again", ["-m", matrix, "-t", "3"]), ("t1", ["-m", matrix, "-t", "1"]), ("t16", ["-m", matrix, "-t", "16"]),
                         ("gz", ["-m", gz, "-t", "5"])):
        p = run_pca(args + ["-p", prefix], tmp)
        assert p.returncode == 0, p.stderr[-500:]
        assert [open(f, "rb").read() for f in outputs(tmp, prefix)] == want, prefix


@pytest.mark.gpu
def test_crlf_matrix_without_final_newline_gives_the_same_files_for_every_t(built, tmp_path):
    """6 sites x 4 samples, CRLF line ends, no line end after the last row: -n 2 writes the same two files under -t 1,
    -t 4 and -t 16 (more ranges than lines), and they hold 6 and 4 rows of 2 finite values"""
    a = structured_cohort(5, 4, 6, 2, thirds=0.3)
    data = open(write_matrix(str(tmp_path / "lf.tsv"), a), "rb").read()
    with open(str(tmp_path / "m.tsv"), "wb") as f:
        f.write(data[:-1].replace(b"\n", b"\r\n"))
    outs = []
    for t in ("1", "4", "16"):
        p = run_pca(["-m", "m.tsv", "-n", "2", "-t", t, "-p", "t" + t], tmp_path)
        assert p.returncode == 0, p.stderr[-500:]
        outs.append([open(f, "rb").read() for f in outputs(tmp_path, "t" + t)])
    assert outs[0] == outs[1] == outs[2]
    names, v, _ = read_table(outputs(tmp_path, "t1")[0])
    assert names == ["rs%d" % k for k in range(6)] and v.shape == (6, 2) and np.isfinite(v).all()
    names, c, _ = read_table(outputs(tmp_path, "t1")[1])
    assert len(names) == 4 and c.shape == (4, 2) and np.isfinite(c).all() and b"\r" not in outs[0][0] + outs[0][1]


@pytest.mark.gpu
def test_rank_refusal_names_the_component(built, tmp_path):
    """A component without a positive eigenvalue beyond rounding is refused by name and nothing is written: the centred
    matrix of n samples has rank n - 1 at most, and 3 distinct columns repeated have rank 2."""
    import ntsm_amd.pca as pca
    rng = np.random.default_rng(3)
    base = rng.integers(0, 3, size=(50, 3)) / 2.0
    a = base[:, np.arange(12) % 3]
    m = write_matrix(str(tmp_path / "rank2.tsv"), a)
    p = run_pca(["-m", m, "-n", "3", "-p", "out"], tmp_path)
    assert p.returncode == 1 and p.stderr.startswith(b"Error: component 2 of the 3 requested has no positive eigenvalue"), p.stderr
    assert not any(os.path.exists(f) for f in outputs(tmp_path, "out"))
    with pytest.raises(pca.RankError) as e:
        pca.run(a, 3)
    assert e.value.component == 2
    assert run_pca(["-m", m, "-n", "2", "-p", "out"], tmp_path).returncode == 0
    full = rng.random((40, 6))
    with pytest.raises(pca.RankError) as e:
        pca.run(full, 6)
    assert e.value.component == 5


@pytest.mark.gpu
def test_wrapper_run_agrees_with_the_cli(cohort_run):
    """ntsm_amd.pca.run on the parsed matrix: the same bits on a second call, and the program's numbers inside the gate
    of the fixtures (golden_bounds).  Not bit for bit: a Python process that has loaded PyTorch binds the rocSOLVER that
    PyTorch ships, the program the one of the ROCm installation, and the two round the eigenvectors differently."""
    import ntsm_amd.pca as pca
    tmp, _, a, d = cohort_run
    l, v, t, times = pca.run(a, d)
    l2, v2, t2, _ = pca.run(a, d)
    assert (l.tobytes(), v.tobytes(), t.tobytes()) == (l2.tobytes(), v2.tobytes(), t2.tobytes())
    bound, _ = golden_bounds(a, d)
    err_v = np.abs(v - read_table(outputs(tmp, "run")[0])[1]).max(axis=0)
    err_t = np.abs(t - read_table(outputs(tmp, "run")[1])[1]).max(axis=0)
    print("wrapper against the program: rotation %.3g, components %.3g" % (err_v.max(), err_t.max()))
    assert (err_v <= bound).all() and (err_t <= bound * np.sqrt(l)).all()
    assert (np.diff(l) < 0).all() and times.gram_flops == a.shape[1] * (a.shape[1] + 1) * a.shape[0] and times.gram_ms > 0


@pytest.mark.gpu
def test_chain_vcf_pca_eval_finds_planted_duplicates(built, tmp_path):
    """ntsmVCF -p -> ntsmPCA -> ntsmEval -p ROT -n CENTRE: a generated VCF cohort; counts files drawn from the matrix's
    columns as ntsmCount would print them, some individuals sequenced twice (the planted pairs).  ntsmEval reads the
    rotation unchanged and reports exactly the planted pairs; with the reference rotation of the same matrix
    (scikit-learn's full solver where importable, else its restatement: numpy's SVD of the centred matrix and the sign
    rule) it reports the same set."""
    from test_eval import files_for
    from test_vcf import cohort, run as run_vcf
    rng = np.random.default_rng(31)
    g, s, v = cohort(tmp_path, rng, 60, 900, dense=False)
    prefix = str(tmp_path / "port")
    rc, mat, cen, err = run_vcf(VCF, ["-s", s, "-r", g, "-p", prefix, "-t", "4", v], str(tmp_path), prefix)
    assert rc == 0 and mat and cen, err[-500:]
    p = run_pca(["-m", prefix + "_matrix.tsv", "-p", prefix, "-t", "4"], tmp_path)
    assert p.returncode == 0, p.stderr[-500:]
    sites, a, _ = read_table(prefix + "_matrix.tsv")
    m, n = a.shape
    assert open(prefix + "_rotationalMatrix.tsv").read().count("\n") == m + 1 == cen.count(b"\n") + 1
    # counts of 24 "sequencing runs": individuals 0...15 once, 0...7 a second time
    who = list(range(16)) + list(range(8))
    counts = np.zeros((len(who), m, 2), dtype=np.uint32)
    for r, j in enumerate(who):
        depth = 20.0 * (0.7 + 0.6 * rng.random())
        counts[r, :, 0] = rng.poisson(depth * a[:, j] + 0.02)
        counts[r, :, 1] = rng.poisson(depth * (1.0 - a[:, j]) + 0.02)
    files = files_for(tmp_path, counts, loci=sites)
    planted = {(files[j], files[16 + j]) for j in range(8)}

    def pairs(rot):
        q = subprocess.run([EVAL, "-p", rot, "-n", prefix + "_center.txt"] + files, capture_output=True, timeout=600)
        assert q.returncode == 0, q.stderr[-500:]
        lines = q.stdout.decode().splitlines()
        assert lines[0].startswith("sample1\tsample2\t")
        return {tuple(sorted(l.split("\t")[:2])) for l in lines[1:]}

    got = pairs(prefix + "_rotationalMatrix.tsv")
    assert got == {tuple(sorted(x)) for x in planted}
    ref = str(tmp_path / "reference_rotationalMatrix.tsv")
    try:
        rot, _ = sklearn_recipe(prefix + "_matrix.tsv", 20)
        rot.to_csv(ref, sep="\t", index_label="AlleleID")
    except ImportError:
        ac = a - a.mean(axis=1, keepdims=True)
        u, sv, vt = np.linalg.svd(ac.T, full_matrices=False)
        vv, _ = fix_signs(vt[:20].T, u[:, :20] * sv[:20])
        with open(ref, "w") as f:
            f.write("AlleleID" + "".join("\t%d" % i for i in range(20)) + "\n")
            f.writelines("%s\t%s\n" % (sites[k], "\t".join(repr(float(x)) for x in vv[k])) for k in range(m))
    assert pairs(ref) == got
