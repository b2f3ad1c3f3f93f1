"""ntsmPCA --store (build/ntsmPCA, ntsm_amd/pca.py: store_cells, run_store): centre and rotation trained on a cohort store's
own samples.  Stores are written here from the layout of DESIGN.md section 9.1.

CPU: every refusal, the surface, the wrapper's argument checks, and the centre's text (host/pca_text.hpp) against the model
of it that the GPU tests use.
GPU: the genotype step against a numpy restatement of the rule (exact), run_store against run_cells (bit for bit), the
program against `ntsmPCA -m` on the matrix text of the model (byte for byte), determinism, the chain
ntsmPCA --store -> ntsmEval --index -> ntsmEval --within-near, and the components against ntsmEval's own projection."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle_binding import ROOT
from test_pca import EVAL, PCA, U, outputs, read_table, run_pca, structured_cohort

HEAD, NAME = 64, 1024
RECORD_HEAD = 32 + NAME
HIDDEN = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")


# ---------------------------------------------------------------------------------------------------- the store and the model
def store_bytes(counts, loci, names):
    """A cohort store as DESIGN.md section 9.1 lays it out: header, locus section, one record per sample"""
    counts = np.ascontiguousarray(counts, dtype="<u4")
    n, m = counts.shape[0], counts.shape[1]
    section = b"".join(l.encode() + b"\0" for l in loci)
    section += bytes(-(HEAD + len(section)) % 8) + np.ones((m, 2), dtype="<u4").tobytes()
    first, stride = HEAD + len(section), RECORD_HEAD + 8 * m
    out = [b"NTSMCOH1" + struct.pack("<IIQQQ", 1, m, n, first, stride) + bytes(24), section]
    for r in range(n):
        total = int((counts[r, :, 0] + counts[r, :, 1]).astype(np.uint64).sum())       # uint32 sums that wrap, then widened
        name = names[r].encode()
        out.append(struct.pack("<QQQII", 0, total, total, 19, 0) + name + bytes(NAME - len(name)) + counts[r].tobytes())
    return b"".join(out)


def write_store(path, counts, loci=None, names=None):
    n, m = counts.shape[0], counts.shape[1]
    loci = loci or ["rs%d" % s for s in range(m)]
    names = names or ["run%04d" % r for r in range(n)]
    with open(str(path), "wb") as f:
        f.write(store_bytes(counts, loci, names))
    return loci, names


def model_codes(counts, c):
    """genotype_code of every cell of counts [samples][sites][2], restated: [sites][samples] of 0 / 1 / 2 (genotype 0 / 0.5 / 1)
    and 3 (missing); the denominator is a uint32 sum that wraps"""
    counts = np.asarray(counts, dtype=np.uint32)
    at = np.where(counts[:, :, 0] > c, counts[:, :, 0], 0).astype(np.uint32)
    cg = np.where(counts[:, :, 1] > c, counts[:, :, 1], 0).astype(np.uint32)
    den = at + cg
    assert den.dtype == np.uint32
    g = at.astype(np.float64) / np.where(den == 0, 1, den).astype(np.float64)
    code = np.where(g < 0.25, 0, np.where(g < 0.75, 1, 2))
    return np.where(den == 0, 3, code).astype(np.uint16).T.copy()


def model_tallies(codes):
    return np.stack([(codes == 1).sum(1), (codes == 2).sum(1), (codes != 3).sum(1)], axis=1).astype(np.uint32)


def g19(q):
    """printf("%.19Lg") of a long double q >= 0"""
    if q == 0:
        return "0"
    mant, exp = np.format_float_scientific(q, precision=18, unique=False, trim="k").split("e")
    digits, exp = mant.replace(".", ""), int(exp)
    assert len(digits) == 19
    if exp < -4 or exp >= 19:
        return "%se%s%02d" % ((digits[0] + "." + digits[1:]).rstrip("0").rstrip("."), "-" if exp < 0 else "+", abs(exp))
    whole, frac = (digits[:exp + 1], digits[exp + 1:]) if exp >= 0 else ("0", "0" * (-exp - 1) + digits)
    frac = frac.rstrip("0")
    return whole + ("." + frac if frac else "")


def centre_text(n_half, n_one, n_called):
    """A site's centre as DESIGN.md section 11.1 defines it: the long double quotient (n_one + n_half / 2) / n_called at 19 digits"""
    if n_called == 0:
        return "0"
    return g19(np.longdouble(float(n_one) + 0.5 * float(n_half)) / np.longdouble(int(n_called)))


def model_texts(tallies):
    return [centre_text(*(int(x) for x in t)) for t in tallies]


def model_matrix(codes, texts):
    """The training matrix [sites][samples]: 0 / 0.5 / 1, a missing cell at what its site's centre text reads back as"""
    fill = np.array([float(t) for t in texts])
    return np.where(codes == 3, fill[:, None], codes.astype(np.float64) / 2.0)


def random_counts(rng, n, m, depth=12.0):
    """[n][m][2] counts of a diploid-looking cohort with some sites not covered"""
    frac = rng.integers(0, 3, size=(n, m)) / 2.0
    counts = np.stack([rng.poisson(depth * frac + 0.3), rng.poisson(depth * (1.0 - frac) + 0.3)], axis=2).astype(np.uint32)
    counts[rng.random((n, m)) < 0.05] = 0
    return counts


def planted_cells(c):
    """(AT, CG, code) of the cells the genotype rule can get wrong, for min_cov = c"""
    k = c + 5
    return [(k, 3 * k, 1), (3 * k, k, 2),                                              # exactly 1:3 (0.25 -> 0.5) and 3:1 (0.75 -> 1)
            (k, 3 * k + 1, 0), (k, 3 * k - 1, 1), (3 * k, k + 1, 1), (3 * k, k - 1, 2),   # one count either side of each
            (0, 0, 3), (c, c, 3), (c, c + 7, 0), (c + 7, c, 2),                           # nothing; both, one at or below min_cov
            (2**31, 2**31, 3),                                                            # the denominator wraps to 0
            (3 * 10**9, 2 * 10**9, 2)]                                                    # it wraps to 705,032,704: 4.25 -> 1


def planted_counts(rng, n, m, c):
    """random_counts with planted_cells at random places (as many as fit) and, from 2 sites on, a last site nobody calls;
    (counts, [(sample, site, code)])"""
    counts = random_counts(rng, n, m)
    free = m - 1 if m > 1 else m
    cells = planted_cells(c)
    where = rng.permutation(n * free)[:len(cells)]
    placed = []
    for (at, cg, code), w in zip(cells, where):
        counts[w // free, w % free] = (at, cg)
        placed.append((w // free, w % free, code))
    if m > 1:
        counts[:, m - 1] = rng.integers(0, c + 1, size=(n, 2))
    return counts, placed


# ---------------------------------------------------------------------------------------------------- CPU
def refusal_inputs(tmp):
    rng = np.random.default_rng(3)
    counts = random_counts(rng, 3, 4)
    write_store(tmp / "good.store", counts)
    write_store(tmp / "one.store", counts[:1])
    write_store(tmp / "empty.store", counts[:0])
    good = open(str(tmp / "good.store"), "rb").read()
    open(str(tmp / "magic.store"), "wb").write(b"NTSMCOH2" + good[8:])
    open(str(tmp / "short.store"), "wb").write(good[:-8])
    open(str(tmp / "tiny.store"), "wb").write(good[:40])
    open(str(tmp / "m.tsv"), "w").write("alleleID\tA\tB\tC\nrs1\t0.5\t1\t0\nrs2\t0\t0.25\t1\n")
    os.mkdir(str(tmp / "dir.store"))


REFUSALS = [
    ("store_and_matrix", ["--store", "good.store", "-m", "m.tsv", "-p", "out"], "Error: --store and -m each name the matrix"),
    ("neither", ["-p", "out", "-n", "2"], "Error: Need Input File (-m) or a cohort store (--store)"),
    ("min_cov_without_store", ["-m", "m.tsv", "-c", "2", "-p", "out", "-n", "1"], "Error: -c belongs to --store"),
    ("train_without_store", ["-m", "m.tsv", "--train", "2", "-p", "out", "-n", "1"], "Error: --train belongs to --store"),
    ("min_cov_unparsable", ["--store", "good.store", "-c", "2x", "-p", "out"], "Error - Invalid parameter c: 2x"),
    ("min_cov_negative", ["--store", "good.store", "-c", "-1", "-p", "out"], "Error: -c -1 is not a count"),
    ("train_unparsable", ["--store", "good.store", "--train", "two", "-p", "out"], "Error - Invalid parameter train: two"),
    ("train_zero", ["--store", "good.store", "--train", "0", "-p", "out", "-n", "1"], "Error: --train 0: good.store holds 3 samples"),
    ("train_beyond", ["--store", "good.store", "--train", "4", "-p", "out", "-n", "1"], "Error: --train 4: good.store holds 3 samples"),
    ("train_one", ["--store", "good.store", "--train", "1", "-p", "out", "-n", "1"], "Error: a PCA needs at least 2 samples: 1 of good.store"),
    ("missing", ["--store", "nope.store", "-p", "out"], "Error: cannot open store nope.store"),
    ("directory", ["--store", "dir.store", "-p", "out"], "Error: dir.store is not a regular file"),
    ("magic", ["--store", "magic.store", "-p", "out"], "Error: magic.store is not a cohort store (magic)"),
    ("truncated", ["--store", "short.store", "-p", "out"], "its header describes 3 samples"),
    ("shorter_than_header", ["--store", "tiny.store", "-p", "out"], "Error: tiny.store is not a cohort store (shorter than its header)"),
    ("empty", ["--store", "empty.store", "-p", "out"], "Error: empty.store holds no samples"),
    ("one_sample", ["--store", "one.store", "-p", "out", "-n", "1"], "Error: a PCA needs at least 2 samples: 1 of one.store"),
    ("no_prefix", ["--store", "good.store", "-n", "2"], "Error: --store needs -p PREFIX"),
    ("d_zero", ["--store", "good.store", "-p", "out", "-n", "0"], "Error: -n 0: the number of components must be at least 1"),
    ("d_above_samples", ["--store", "good.store", "-p", "out", "-n", "4"], "Error: -n 4 is more than min(samples, sites) = min(3, 4)"),
    ("d_above_trained", ["--store", "good.store", "--train", "2", "-p", "out", "-n", "3"], "Error: -n 3 is more than min(samples, sites) = min(2, 4)"),
    ("d_default_too_many", ["--store", "good.store", "-p", "out"], "Error: -n 20 is more than min(samples, sites) = min(3, 4)"),
]


@pytest.mark.parametrize("name,args,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(built, tmp_path, name, args, msg):
    """Each refusal: its message first on stderr, exit status 1, nothing on stdout, nothing written -- all before the device is
    touched (every device is hidden: a program that reached the device step would report that instead)."""
    refusal_inputs(tmp_path)
    before = sorted(os.listdir(str(tmp_path)))
    p = subprocess.run([PCA] + args, cwd=str(tmp_path), capture_output=True, env=HIDDEN, timeout=120)
    err = p.stderr.decode()
    assert p.returncode == 1 and msg in err.split("\n")[0] and err.startswith("Error"), (p.returncode, err)
    assert err.count("\n") == 1 or err.endswith("Try '--help' for more information.\n"), err
    assert p.stdout == b"" and sorted(os.listdir(str(tmp_path))) == before


def test_surface(built):
    """The two entry points are exported and declared, the wrapper has both calls, the help names the mode"""
    import ctypes
    import ntsm_amd.pca as pca
    lib = ctypes.CDLL(os.path.join(ROOT, "ntsm_amd", "libntsm_pca_hip.so"))
    hdr = open(os.path.join(ROOT, "include", "ntsm_pca_hip.h")).read()
    for name in ("ntsm_pca_store_cells", "ntsm_pca_run_store"):
        assert hasattr(lib, name) and "int %s(int device, " % name in hdr, name
    assert callable(pca.store_cells) and callable(pca.run_store)
    assert ctypes.sizeof(pca.StoreTimes) == 4 * 8 + 2 * 4                               # ntsm_pca_store_times
    p = run_pca(["--help"], ".")
    assert p.returncode == 0 and b"--store" in p.stderr and b"--train" in p.stderr and b"--minCov" in p.stderr


def test_wrapper_refuses_bad_arguments(built):
    """The ABI's argument checks come before any device call: shapes, D, a stride below a record's counts"""
    import ntsm_amd.eval as ev
    import ntsm_amd.pca as pca
    db = np.zeros((3, 4, 2), dtype=np.uint32)
    for d in (0, 4, 5):
        with pytest.raises(RuntimeError, match="-1"):
            pca.run_store(db, d)
    with pytest.raises(RuntimeError, match="-1"):
        pca.run_store(db[:1], 1)                                                        # one sample
    with pytest.raises(RuntimeError, match="-1"):
        pca.store_cells(np.zeros((0, 4, 2), dtype=np.uint32))
    with pytest.raises(RuntimeError, match="-1"):
        pca.store_cells(np.zeros((3, 0, 2), dtype=np.uint32))
    rec = ev.Records.of(db, RECORD_HEAD)
    rec.stride = 8 * 4 - 4
    with pytest.raises(RuntimeError, match="-1"):
        pca.store_cells(rec)
    with pytest.raises(ValueError):
        pca.store_cells(db, n=4)
    with pytest.raises(ValueError):
        pca.store_cells(np.zeros((3, 4), dtype=np.uint32))


def test_centre_text_is_the_model(built, tmp_path):
    """store_centre_text / store_centre_value of host/pca_text.hpp (tests/pca_store_text_check.cpp around them) against the
    model the GPU tests use: the long double quotient at 19 digits, "0" for a site nobody calls, and the value Python's
    float() reads back -- for every tally of up to 40 samples, large cohorts, and quotients below 1e-4 (exponent form)."""
    exe = str(tmp_path / "pca_store_text_check")
    subprocess.run(["g++", "-O1", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "pca_store_text_check.cpp")], check=True)
    rng = np.random.default_rng(8)
    cases = [(h, o, c) for c in range(0, 41) for h in range(0, c + 1, 3) for o in range(0, c - h + 1, 2)]
    cases += [(0, 0, 0), (1, 0, 100000), (1, 0, 16777215), (3, 0, 99991), (1, 1, 3), (203, 0, 203), (0, 203, 203), (1, 0, 3)]
    for _ in range(2000):
        c = int(rng.integers(1, 100001))
        h = int(rng.integers(0, c + 1))
        cases.append((h, int(rng.integers(0, c - h + 1)), c))
    p = subprocess.run([exe], input="".join("%d %d %d\n" % x for x in cases), capture_output=True, text=True, check=True)
    got = [l.split("\t") for l in p.stdout.split("\n")[:-1]]
    assert len(got) == len(cases)
    bad = [(x, g, centre_text(*x)) for x, g in zip(cases, got) if g[0] != centre_text(*x) or float(g[1]) != float(g[0])]
    assert not bad, bad[:5]
    assert ("0", "0") in [tuple(g) for g in got] and any("e-" in g[0] for g in got)


def test_model_codes_of_the_planted_cells():
    """The numpy restatement gives the planted cells the codes that the rule gives them by hand, for the three min_cov of the GPU test"""
    for c in (0, 1, 3):
        cells = planted_cells(c)
        counts = np.array([[(at, cg) for at, cg, _ in cells]], dtype=np.uint32)
        assert model_codes(counts, c)[:, 0].tolist() == [code for _, _, code in cells], c


# ---------------------------------------------------------------------------------------------------- GPU: the device steps
GENOTYPE_SHAPES = [(1, 2, 0), (63, 65, 0), (64, 64, 64), (65, 129, 64), (300, 257, 100), (300, 257, 65), (30, 1030, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("c", [0, 1, 3])
@pytest.mark.parametrize("m,n,chunk", GENOTYPE_SHAPES, ids=["%dx%d_chunk%d" % s for s in GENOTYPE_SHAPES])
def test_genotype_step_equals_the_model(built, m, n, chunk, c):
    """store_cells on samples laid out at a store's stride (a record head in front of each): cells and tallies equal the
    numpy restatement exactly, the planted cells have their codes, the site nobody calls is all missing, the chunk count"""
    import ntsm_amd.eval as ev
    import ntsm_amd.pca as pca
    rng = np.random.default_rng([m, n, chunk, c])
    counts, placed = planted_counts(rng, n, m, c)
    codes = model_codes(counts, c)
    for sample, site, code in placed:
        assert codes[site, sample] == code
    rec = ev.Records.of(counts, RECORD_HEAD)
    assert rec.stride == RECORD_HEAD + 8 * m
    cells, tallies, times = pca.store_cells(rec, min_cov=c, db_chunk=chunk)
    assert cells.shape == (m, n) and tallies.shape == (m, 3)
    want = np.where(codes == 3, 0, codes + 1).astype(np.uint16)
    assert np.array_equal(cells, want), np.argwhere(cells != want)[:10]
    assert np.array_equal(tallies, model_tallies(codes)), np.argwhere(tallies != model_tallies(codes))[:10]
    if m > 1:
        assert not cells[m - 1].any() and not tallies[m - 1].any()
    assert times.chunks == (-(-n // chunk) if chunk else 1) and times.chunk == (min(chunk, n) if chunk else n)


@pytest.fixture(scope="module")
def cells_300x257(built):
    """(counts, Records, cells, value table, fills) of 257 samples x 300 sites, min_cov 1: the cells once, unchunked"""
    import ntsm_amd.eval as ev
    import ntsm_amd.pca as pca
    counts, _ = planted_counts(np.random.default_rng(300257), 257, 300, 1)
    rec = ev.Records.of(counts, RECORD_HEAD)
    cells, tallies, _ = pca.store_cells(rec, min_cov=1)
    fills = np.array([float(t) for t in model_texts(tallies)])
    return counts, rec, cells, tallies, pca.store_value_table(), fills


@pytest.mark.gpu
@pytest.mark.parametrize("split", [0, 3])
@pytest.mark.parametrize("chunk", [0, 64, 100])
def test_run_store_equals_run_cells_bits(cells_300x257, chunk, split):
    """run_store against run_cells on (store_cells' cells, the value table, the fills from the tallies): eigenvalues, rotation
    and components bit for bit, for every db_chunk and split; the tallies again"""
    import ntsm_amd.pca as pca
    _, rec, cells, tallies, value, fills = cells_300x257
    d = 12
    l, v, t, _, _ = pca.run_cells(cells, value, fills, d, split=split)
    l2, v2, t2, tallies2, times, store_times = pca.run_store(rec, d, min_cov=1, db_chunk=chunk, split=split)
    assert np.isfinite(v).all() and np.abs(t).max() > 0
    assert (l.tobytes(), v.tobytes(), t.tobytes()) == (l2.tobytes(), v2.tobytes(), t2.tobytes())
    assert np.array_equal(tallies2, tallies)
    assert store_times.chunks == (-(-257 // chunk) if chunk else 1) and store_times.genotype_ms > 0 and store_times.expand_ms > 0
    if split:
        assert times.gram_split == split


# ---------------------------------------------------------------------------------------------------- GPU: the program
def counts_of(rng, a, depth=20.0, missing=0.03):
    """[samples][sites][2] counts drawn from the REF fractions a [sites][samples] at about `depth`, a share of cells not covered"""
    a = a.T
    counts = np.stack([rng.poisson(depth * a + 0.02), rng.poisson(depth * (1.0 - a) + 0.02)], axis=2).astype(np.uint32)
    counts[rng.random(a.shape) < missing] = 0
    return counts


def cli(args, cwd, chunk=None):
    env = dict(os.environ) if chunk is None else dict(os.environ, NTSM_PCA_STORE_CHUNK=str(chunk))
    p = subprocess.run([PCA] + args, cwd=str(cwd), capture_output=True, env=env, timeout=600)
    assert p.returncode == 0 and p.stdout == b"", p.stderr[-500:]
    return p


def three_files(cwd, prefix):
    return [open(f, "rb").read() for f in outputs(cwd, prefix) + [os.path.join(str(cwd), prefix + "_center.txt")]]


@pytest.fixture(scope="module")
def cohort_run(built, tmp_path_factory):
    """203 samples x 3,001 sites at depth 20 with 3 % of the cells missing, packed into a store; the model's matrix text; one
    run of `ntsmPCA --store` at -t 3: (dir, counts, codes, texts, loci, names)"""
    tmp = tmp_path_factory.mktemp("pca_store")
    rng = np.random.default_rng(203)
    counts = counts_of(rng, structured_cohort(77, 203, 3001, 5))
    loci, names = write_store(tmp / "cohort.store", counts)
    codes = model_codes(counts, 1)
    texts = model_texts(model_tallies(codes))
    word = ("0", "0.5", "1")
    with open(str(tmp / "M.tsv"), "w") as f:
        f.write("alleleID\t" + "\t".join(names) + "\n")
        f.writelines("%s\t%s\n" % (loci[s], "\t".join(texts[s] if k == 3 else word[k] for k in codes[s])) for s in range(len(loci)))
    cli(["--store", "cohort.store", "-p", "st3", "-t", "3"], tmp)
    return tmp, counts, codes, texts, loci, names


@pytest.mark.gpu
def test_cli_equals_the_matrix_route(cohort_run):
    """`ntsmPCA --store` against `ntsmPCA -m M.tsv` with M.tsv written from the numpy model (0 / 0.5 / 1, a missing cell as its
    site's centre text): rotation and components byte for byte at -t 1 and -t 3, the centre file the model's texts, the rows
    named by the store's loci and samples"""
    tmp, _, codes, texts, loci, names = cohort_run
    assert (codes == 3).mean() > 0.02 and (codes == 3).all(axis=1).sum() == 0
    cli(["--store", "cohort.store", "-p", "st1", "-t", "1"], tmp)
    for t in ("1", "3"):
        cli(["-m", "M.tsv", "-p", "mt" + t, "-t", t], tmp)
        assert three_files(tmp, "st" + t)[:2] == [open(f, "rb").read() for f in outputs(tmp, "mt" + t)], t
        assert three_files(tmp, "st" + t)[2] == "".join(x + "\n" for x in texts).encode(), t
    rows, v, _ = read_table(outputs(tmp, "st1")[0])
    cols, c, _ = read_table(outputs(tmp, "st1")[1])
    assert rows == loci and cols == names and v.shape == (3001, 20) and c.shape == (203, 20)


@pytest.mark.gpu
def test_cli_train_takes_a_prefix(cohort_run):
    """--train 150 gives the three files of a store that holds only the first 150 records; -c is the genotype rule's min_cov"""
    tmp, counts, _, _, loci, names = cohort_run
    write_store(tmp / "first150.store", counts[:150], loci, names[:150])
    cli(["--store", "cohort.store", "--train", "150", "-p", "train", "-t", "3"], tmp)
    cli(["--store", "first150.store", "-p", "only", "-t", "3"], tmp)
    assert three_files(tmp, "train") == three_files(tmp, "only")
    assert three_files(tmp, "train")[2] == "".join(x + "\n" for x in model_texts(model_tallies(model_codes(counts[:150], 1)))).encode()
    assert three_files(tmp, "train") != three_files(tmp, "st3")
    cli(["--store", "cohort.store", "--train", "150", "-c", "4", "-p", "c4", "-t", "3"], tmp)
    assert three_files(tmp, "c4")[2] == "".join(x + "\n" for x in model_texts(model_tallies(model_codes(counts[:150], 4)))).encode()


@pytest.mark.gpu
def test_cli_same_bytes_every_run_and_every_chunk(cohort_run):
    """A second run, and runs that walk the store in chunks of 64 and of 77 samples (NTSM_PCA_STORE_CHUNK; the second starts
    chunks at odd columns), give the bytes of the unchunked run; -v names the chunk count"""
    tmp = cohort_run[0]
    want = three_files(tmp, "st3")
    cli(["--store", "cohort.store", "-p", "again", "-t", "3"], tmp)
    assert three_files(tmp, "again") == want
    for chunk, passes in ((64, 4), (77, 3)):
        p = cli(["--store", "cohort.store", "-p", "chunk%d" % chunk, "-t", "3", "-v"], tmp, chunk=chunk)
        assert three_files(tmp, "chunk%d" % chunk) == want, chunk
        assert b"[pca] store: %d chunks of %d samples" % (passes, chunk) in p.stderr, p.stderr[-800:]
        assert b"genotype" in p.stderr and b"expand" in p.stderr and b"gram" in p.stderr


@pytest.mark.gpu
def test_components_agree_with_ntsmEvals_projection(cohort_run):
    """The components file against ntsm_eval_project_store of the same store samples with the written centre and rotation
    (what `ntsmEval --index` keeps): max|cloud - t| / sqrt(l_1) inside p u sqrt(n) l_1 / l_D, the bound of
    test_pca.py::test_gap_free_identities, from the model matrix in numpy; the measured value is printed.  On the MI355X: 4.5e-16 inside a bound of 2.3e-11
    (DESIGN.md section 11.1)."""
    import ntsm_amd.eval as ev
    tmp, counts, codes, texts, _, _ = cohort_run
    a = model_matrix(codes, texts)
    p, n = a.shape
    d = 20
    ac = a - a.mean(axis=1, keepdims=True)
    l = np.sort(np.linalg.eigvalsh(ac.T @ ac))[::-1][:d]
    bound = p * U * np.sqrt(n) * l[0] / l[d - 1]
    norm = np.array([np.longdouble(x) for x in open(str(tmp / "st3_center.txt")).read().split("\n")[:p]], dtype=np.longdouble)
    rows = [line.split("\t")[1:] for line in open(outputs(tmp, "st3")[0]).read().split("\n")[1:p + 1]]
    rot = np.array([[np.longdouble(rows[s][k]) for s in range(p)] for k in range(d)], dtype=np.longdouble)
    cloud = ev.project_store(ev.Records.of(counts, RECORD_HEAD), norm, rot, min_cov=1)[0]
    _, t, _ = read_table(outputs(tmp, "st3")[1])
    err = np.abs(cloud - t).max() / np.sqrt(l[0])
    print("components against ntsmEval's projection: bound %.3g  measured %.3g" % (bound, err))
    assert cloud.shape == t.shape == (n, d) and err <= bound


@pytest.mark.gpu
def test_chain_store_pca_index_within_near_finds_planted_duplicates(built, tmp_path):
    """A store for which no VCF exists: 80 individuals of 5 populations over 900 sites, counts at depth 20 x (0.7 ... 1.3), 16 of
    them sequenced twice: 96 records.  ntsmPCA --store, ntsmEval --index with its two files, ntsmEval --within-near: exactly
    the 16 planted pairs, the set that ntsmEval --within (all pairs) reports."""
    rng = np.random.default_rng(31)
    a = structured_cohort(41, 80, 900, 5)
    who = list(range(80)) + list(range(16))
    counts = np.zeros((len(who), 900, 2), dtype=np.uint32)
    for r, j in enumerate(who):
        depth = 20.0 * (0.7 + 0.6 * rng.random())
        counts[r, :, 0] = rng.poisson(depth * a[:, j] + 0.02)
        counts[r, :, 1] = rng.poisson(depth * (1.0 - a[:, j]) + 0.02)
    _, names = write_store(tmp_path / "runs.store", counts)
    planted = {tuple(sorted((names[j], names[80 + j]))) for j in range(16)}
    cli(["--store", "runs.store", "-p", "runs", "-t", "4"], tmp_path)

    def pairs(args):
        q = subprocess.run([EVAL] + args, cwd=str(tmp_path), capture_output=True, timeout=600)
        assert q.returncode == 0, q.stderr[-500:]
        lines = q.stdout.decode().splitlines()
        assert lines[0].startswith("sample1\tsample2\t")
        return {tuple(sorted(l.split("\t")[:2])) for l in lines[1:]}

    q = subprocess.run([EVAL, "--index", "runs.store", "-p", "runs_rotationalMatrix.tsv", "-n", "runs_center.txt"], cwd=str(tmp_path), capture_output=True,
                       timeout=600)
    assert q.returncode == 0 and q.stdout == b"", q.stderr[-500:]
    near, every = pairs(["--within-near", "runs.store"]), pairs(["--within", "runs.store"])
    print("planted %d, --within-near %d, --within %d" % (len(planted), len(near), len(every)))
    assert near == planted and every == planted
