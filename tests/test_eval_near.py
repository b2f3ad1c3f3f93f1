"""ntsmEval's PCA-guided search of new samples against a cohort store: `--index STORE -p ROT -n NORM`
projects the store's samples into STORE.pcaidx (ntsm_amd/csrc/host/eval_index.hpp), `--near STORE FILES...` searches FILES
against the store through that index and prints the rows of the -p run over [FILES..., store samples...] that name one of
FILES.  Device side: ntsm_eval_project_store, ntsm_eval_cross_candidates, ntsm_eval_cross_score_pairs
(include/ntsm_eval_hip.h, ntsm_amd/csrc/ntsm_eval_near.hip).

CPU: the surface, every refusal that needs no index made on a GPU (indexes are written here from the documented layout), the
index writer and reader under the host sanitizers (`make index_check`).
GPU: each entry point bit for bit against the session call it mirrors on the concatenation or on the dense samples, and the
CLI's stdout byte for byte against `build/ntsmEval -p -n` over [queries, database files] -- a path this feature does not
touch and that tests/test_eval_reference.py holds to the reference class -- and, where it is built, against
oracle/_ref/ref_ntsmEval itself.  No comparison has a tolerance."""
import hashlib
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from oracle_binding import ROOT
from test_eval import EVAL, random_samples
from test_eval_pca import write_pca
from test_eval_reference import (BIG_PCA, PCA, REF_EVAL, TIE_FREE, cohorts, duplicate_cases, reference, restatement,  # noqa: F401
                                 stdout_of, tie_free_args, wrapped_samples)
from test_eval_store import read_store, run, seven_files, snapshot, unchanged

DBL_MAX = float(np.finfo(np.float64).max)
HEAD = 1056                                                                             # a store's record head: the stride is HEAD + 8 * sites


# ---------------------------------------------------------------------------------------------------- the index, as documented
def cells(values):
    """x87 numbers as the index holds them: 16-byte cells, the 6 padding bytes zero"""
    raw = np.ascontiguousarray(values, dtype=np.longdouble).reshape(-1).view(np.uint8).reshape(-1, 16).copy()
    raw[:, 10:] = 0
    return raw.tobytes()


def locus_crc(store_path):
    s = read_store(store_path)
    return zlib.crc32(open(store_path, "rb").read()[64:s["first"]]) & 0xFFFFFFFF


def index_bytes(store_path, n_samples, dim, min_cov, norm, rot, cloud=None, geno=None, crc=None):
    """An index of `store_path` written from the layout of eval_index.hpp, independently of it"""
    m = read_store(store_path)["m"]
    first, stride = 64 + 16 * m * (1 + dim), 8 * dim + 16
    head = b"NTSMPCX1" + struct.pack("<IIQIIIIQQ", 1, m, n_samples, dim, min_cov, locus_crc(store_path) if crc is None else crc, 0, first, stride) + bytes(8)
    assert len(head) == 64
    cloud = np.zeros((n_samples, dim)) if cloud is None else cloud
    geno = np.zeros((n_samples, 3), dtype=np.uint32) if geno is None else geno
    recs = b"".join(np.asarray(cloud[r], dtype="<f8").tobytes() + np.asarray(geno[r], dtype="<u4").tobytes() + bytes(4) for r in range(n_samples))
    return head + cells(norm) + cells(rot) + recs


def read_index(path):
    b = open(path, "rb").read()
    assert b[:8] == b"NTSMPCX1"
    version, m, n, dim, min_cov, crc, zero, first, stride = struct.unpack_from("<IIQIIIIQQ", b, 8)
    assert version == 1 and zero == 0 and b[56:64] == bytes(8)
    assert first == 64 + 16 * m * (1 + dim) and stride == 8 * dim + 16 and len(b) == first + n * stride
    mat = np.frombuffer(b, dtype=np.uint8, count=16 * m * (1 + dim), offset=64).reshape(-1, 16)
    assert not mat[:, 10:].any()                                                        # the padding of every cell is zero
    rec = np.frombuffer(b, dtype=np.uint8, count=n * stride, offset=first).reshape(n, stride)
    cloud = rec[:, :8 * dim].copy().view("<f8").reshape(n, dim)
    geno = rec[:, 8 * dim:].copy().view("<u4").reshape(n, 4)
    assert not geno[:, 3].any()
    return dict(m=m, n=n, dim=dim, min_cov=min_cov, crc=crc, matrices=mat.tobytes(), cloud=cloud, geno=geno[:, :3])


def loaded_pca(d, m, dim):
    """norm [m] and rot [dim][m] as loadPCA reads the files write_pca wrote: strtold of every field (numpy's parser of
    np.longdouble strings calls it)"""
    norm = [np.longdouble(x) for x in open(os.path.join(str(d), "norm.txt")).read().split("\n")[:m]]
    rows = [line.split("\t")[1:1 + dim] for line in open(os.path.join(str(d), "rot.tsv")).read().split("\n")[1:1 + m]]
    return np.array(norm, dtype=np.longdouble), np.array([[np.longdouble(rows[j][k]) for j in range(m)] for k in range(dim)], dtype=np.longdouble)


# ---------------------------------------------------------------------------------------------------- CPU
def test_surface():
    """The three entry points are exported and declared, the help text names both modes and still says that -p against a
    store is not how it is spelled."""
    import ctypes
    lib = ctypes.CDLL(os.path.join(ROOT, "ntsm_amd", "libntsm_eval_hip.so"))
    hdr = open(os.path.join(ROOT, "include", "ntsm_eval_hip.h")).read()
    for name in ("ntsm_eval_project_store", "ntsm_eval_cross_candidates", "ntsm_eval_cross_score_pairs"):
        assert hasattr(lib, name), name
        assert "int %s(int device, " % name in hdr, name
    p = subprocess.run([EVAL, "--help"], capture_output=True)
    assert p.returncode == 0 and p.stdout == b""
    assert b"--index" in p.stderr and b"--near" in p.stderr and b"against a store" in p.stderr


def test_refusals(tmp_path):
    """Every refusal of --index and --near that needs no index made on a GPU: exit 1, an 'Error:' line, nothing on stdout,
    the store and the index -- bytes and mtime -- as they were, no .tmp left.  The indexes are written here from the layout:
    a current one (S), a stale one (T: 3 of 4 samples), one with a broken magic (U), one for other loci (V), one a byte
    short (W)."""
    names = seven_files(tmp_path)[0]
    rng = np.random.default_rng(5)
    write_pca(tmp_path, 40, 3, rng)
    for s in "STUVW":
        assert run(["--pack", s] + names[:4], tmp_path).returncode == 0
    at = lambda x: str(tmp_path / x)  # noqa: E731
    norm, rot = loaded_pca(tmp_path, 40, 2)
    good = index_bytes(at("S"), 4, 2, 1, norm, rot)
    open(at("S.pcaidx"), "wb").write(good)
    open(at("T.pcaidx"), "wb").write(index_bytes(at("T"), 3, 2, 1, norm, rot))
    open(at("U.pcaidx"), "wb").write(b"NTSMPCX2" + good[8:])
    open(at("V.pcaidx"), "wb").write(index_bytes(at("V"), 4, 2, 1, norm, rot, crc=locus_crc(at("V")) ^ 1))
    open(at("W.pcaidx"), "wb").write(good[:-1])
    store = open(at("S"), "rb").read()
    layout = read_store(at("S"))
    with open(at("empty"), "wb") as f:                                                  # a valid store without samples
        f.write(store[:16] + struct.pack("<Q", 0) + store[24:layout["first"]])
    with open(at("trunc"), "wb") as f:
        f.write(store[:-1])
    assert run(["--pack", "bare"] + names[:2], tmp_path).returncode == 0               # a store without any index
    with open(at("alien.txt"), "w") as f:
        f.write("#@TK\t5\n#@KS\t19\nrs1\t3\t4\t3\t4\t1\t1\nrsUnknown\t3\t4\t3\t4\t1\t1\n")
    P = ["-p", "rot.tsv", "-n", "norm.txt", "-d", "2"]
    q = names[5]
    cases = [
        (["--index", "S"] + P + [q], "S"),                                              # FILES given
        (["--index", "S", "-n", "norm.txt", "-d", "2"], "S"),                           # no -p
        (["--index", "S", "-p", "rot.tsv", "-d", "2"], "S"),                            # no -n
        (["--index", "S", "-p", "nowhere.tsv", "-n", "norm.txt"], "S"),                 # -p unreadable
        (["--index", "S", "-p", "rot.tsv", "-n", "nowhere.txt"], "S"),                  # -n unreadable
        (["--index", "S", "-p", "rot.tsv", "-n", "norm.txt", "-d", "0"], "S"),
        (["--index", "S", "--pack", "S"] + P, "S"),
        (["--index", "S", "--against", "S"] + P, "S"),
        (["--index", "S", "--near", "S"] + P, "S"),
        (["--index", "S", "-b", "truth.tsv"] + P, "S"),
        (["--index", "S", "-e", "merged.txt"] + P, "S"),
        (["--index", "S", "-o"] + P, "S"),
        (["--index", "trunc"] + P, "trunc"),                                            # an invalid store
        (["--index", "empty"] + P, "empty"),                                            # an empty one
        (["--index", "S", "-p", "rot.tsv", "-n", "norm.txt", "-d", "3"], "S"),          # an index written with another -d
        (["--index", "S", "-c", "2"] + P, "S"),                                         # ... another -c
        (["--index", "U"] + P, "U"),                                                    # an index that is none: not overwritten
        (["--index", "V"] + P, "V"),
        (["--near", "bare", q], "bare"),                                                # the index is absent
        (["--near", "U", q], "U"),                                                      # invalid: magic
        (["--near", "V", q], "V"),                                                      # invalid: other loci
        (["--near", "W", q], "W"),                                                      # invalid: size
        (["--near", "T", q], "T"),                                                      # stale
        (["--near", "S", "-p", "rot.tsv", q], "S"),
        (["--near", "S", "-n", "norm.txt", q], "S"),
        (["--near", "S", "-b", "truth.tsv", q], "S"),
        (["--near", "S", "-e", "merged.txt", q], "S"),
        (["--near", "S", "-o", q], "S"),
        (["--near", "S", "--pack", "S", q], "S"),
        (["--near", "S", "--against", "S", q], "S"),
        (["--near", "S", "--index", "S", q], "S"),
        (["--near", "S", "-c", "2", q], "S"),                                           # the index says -c 1
        (["--near", "S", "-d", "3", q], "S"),                                           # the index says -d 2
        (["--near", "S"], "S"),                                                          # no FILES
        (["--near", "S", q, "alien.txt"], "S"),                                         # an unknown locus in a query
        (["--near", "trunc", q], "trunc"),
        (["--near", "empty", q], "empty"),
    ]
    for args, touched in cases:
        path, idx = at(touched), at(touched + ".pcaidx")
        before = snapshot(path), (snapshot(idx) if os.path.exists(idx) else None)
        p = run(args, tmp_path)
        assert p.returncode == 1 and p.stdout == b"", (args, p.returncode, p.stdout[:100], p.stderr[-300:])
        assert any(line.startswith(b"Error: ") for line in p.stderr.split(b"\n")), (args, p.stderr)
        assert unchanged(path, before[0]), args
        assert (unchanged(idx, before[1]) if before[1] else not os.path.exists(idx)), args
        assert not os.path.exists(idx + ".tmp") and not os.path.exists(path + ".tmp") and not os.path.exists(at("merged.txt")), args
    p = run(["--near", "T", q], tmp_path)
    assert b"--index" in p.stderr                                                       # the stale refusal says what to run
    p = run(["--index", "S", "-p", "rot.tsv", "-n", "norm.txt", "-d", "3"], tmp_path)
    assert b"delete" in p.stderr and b"S.pcaidx" in p.stderr                            # ... and this one which file to delete
    # the spelling that stays refused, with the sentence it always had
    p = run(["--against", "S", "-p", "rot.tsv", "-n", "norm.txt", q], tmp_path)
    assert p.returncode == 1 and b"against a store is not part of this build" in p.stderr
    p = run(["--pack", "S", "-p", "rot.tsv", q], tmp_path)
    assert p.returncode == 1 and b"with --pack is not part of this build" in p.stderr
    # an index that is current is left alone, without a GPU
    before = snapshot(at("S.pcaidx"))
    p = run(["--index", "S"] + P, tmp_path)
    assert p.returncode == 0 and p.stdout == b"" and b"up to date" in p.stderr and unchanged(at("S.pcaidx"), before)


def test_index_writer_and_reader_under_the_host_sanitizers(tmp_path):
    """`make index_check`: tools/eval_index_check.cpp -- writer, reader, append and every validity failure of eval_index.hpp
    on synthetic clouds -- built with -fsanitize=address,undefined as a program of its own, run once."""
    subprocess.run(["make", "-s", "index_check"], cwd=ROOT, check=True, stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(ROOT, "build", "eval_index_check"), str(tmp_path)], capture_output=True)
    assert p.returncode == 0 and p.stdout.endswith(b"ok\n") and b"NOT refused" not in p.stdout, (p.stdout[-600:], p.stderr[-600:])
    assert p.stdout.count(b"refused (") >= 14 and b"extended index == index written at once" in p.stdout


# ---------------------------------------------------------------------------------------------------- GPU: the projection
def synthetic_pca(rng, m, dim):
    """centre and rotation with full 64-bit significands"""
    wide = lambda shape: rng.random(shape).astype(np.longdouble) + rng.random(shape).astype(np.longdouble) * np.longdouble(2.0) ** -40  # noqa: E731
    return wide(m) * np.longdouble(0.9), (wide((dim, m)) - np.longdouble(0.5)) * np.longdouble(3.0)


# (n_db, sites, dim, min_cov, db_chunk): one lane, a wave less one, a full wave, one past it in two chunks, 257 samples in
# three ragged chunks, 1,025 samples (five workgroups, the last with one live lane)
PROJECT = [(1, 1, 1, 1, 0), (63, 7, 3, 0, 0), (64, 300, 4, 1, 0), (65, 300, 5, 1, 64), (257, 200, 20, 3, 100), (1025, 24, 2, 1, 0)]


def check_project_store(db, dim, c, chunk, rng):
    import ntsm_amd.eval as ev
    n, m = db.shape[0], db.shape[1]
    norm, rot = synthetic_pca(rng, m, dim)
    want = ev.project(db, norm, rot, min_cov=c)[0]
    rec = ev.Records.of(db, HEAD)
    assert rec.stride == HEAD + 8 * m > 8 * m
    cloud, geno, times = ev.project_store(rec, norm, rot, min_cov=c, db_chunk=chunk)
    assert cloud.shape == (n, dim) and cloud.tobytes() == want.tobytes()
    assert np.array_equal(geno, ev.cross(db[:1], db, min_cov=c)[1])
    a, b = db[:, :, 0] > c, db[:, :, 1] > c
    assert np.array_equal(geno, np.stack([(a & b).sum(1), (a ^ b).sum(1), (~a & ~b).sum(1)], axis=1))
    assert times.chunks == (-(-n // chunk) if chunk else 1)
    return cloud


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PROJECT, ids=["db%d_m%d_d%d_c%d_chunk%d" % s for s in PROJECT])
def test_project_store_equals_session_projection_bits(shape):
    """ntsm_eval_project_store on samples laid out at a store's stride (1,056 filler bytes in front of each) against
    ntsm_eval_project on the dense samples: the cloud as raw bytes; the tallies against ntsm_eval_cross's and a numpy count;
    the chunk count."""
    n, m, dim, c, chunk = shape
    rng = np.random.default_rng(list(shape))
    db = random_samples(rng, n, m, depth=8.0)
    if n > 4:
        db[0] = 0                                                                       # no coverage: every site missing
        db[2] = rng.integers(2**31, 2**32, size=(m, 2)).astype(np.uint32)
    cloud = check_project_store(db, dim, c, chunk, rng)
    if n > 4 and m > 1:
        assert np.abs(cloud[1:]).max() > 0                                              # a cloud never written cannot pass


@pytest.mark.gpu
def test_project_store_wrapped_counts():
    """wrapped_samples: counts at and beyond 2^31 in both columns, where `unsigned denom = countAT + countCG` wraps"""
    rng = np.random.default_rng(34)
    db = wrapped_samples(rng, 20, 120)
    for c, chunk in ((1, 0), (0, 7)):
        check_project_store(db, 4, c, chunk, rng)


def test_project_store_empty_sides_need_no_device():
    """no sample, or no site: zeroed outputs of the right shape, before any device call"""
    import ntsm_amd.eval as ev
    norm, rot = synthetic_pca(np.random.default_rng(1), 5, 2)
    cloud, geno, times = ev.project_store(np.zeros((0, 5, 2), dtype=np.uint32), norm, rot)
    assert cloud.shape == (0, 2) and geno.shape == (0, 3) and times.chunks == 0
    cloud, geno, times = ev.project_store(np.zeros((3, 0, 2), dtype=np.uint32), np.zeros(0, dtype=np.longdouble), np.zeros((2, 0), dtype=np.longdouble))
    assert cloud.tobytes() == bytes(3 * 2 * 8) and not geno.any() and times.chunks == 0


# ---------------------------------------------------------------------------------------------------- GPU: the search
def search_case(n_q, n_db, dim, seed=0, classes=None):
    """A synthetic cloud of n_q + n_db points and radii of the three classes on both sides (squared: small and large at the
    10th and 50th percentile of the pair metrics, DBL_MAX), queries and database each cycling through the classes from
    another start, so that each side owns pairs."""
    rng = np.random.default_rng([n_q, n_db, dim, seed])
    n = n_q + n_db
    cloud = rng.normal(size=(n, dim))
    diff = cloud[:min(n, 200), None, :] - cloud[None, :min(n, 200), :]
    dd = (diff * diff).sum(-1)[np.triu_indices(min(n, 200), 1)] if n > 1 else np.array([1.0])
    small, large = float(np.percentile(dd, 10)), float(np.percentile(dd, 50))
    if classes is None:
        kinds = [large, small, DBL_MAX]
        classes = [kinds[i % 3] for i in range(n_q)] + [kinds[(i + 1) % 3] for i in range(n_db)]
    return cloud, np.array(classes, dtype=np.float64)


def session_candidates(cloud, radius):
    import ntsm_amd.eval as ev
    return ev.candidates(np.zeros((len(radius), 1, 2), dtype=np.uint32), cloud, radius)[:3]


def check_candidates(cloud, radius, n_q):
    """cross_candidates against candidates on the concatenation, filtered to the pairs with a query: bytes"""
    import ntsm_amd.eval as ev
    pi, pk, dist = session_candidates(cloud, radius)
    keep = (pi < n_q) | (pk < n_q)
    gi, gk, gd, _ = ev.cross_candidates(cloud[:n_q], radius[:n_q], cloud[n_q:], radius[n_q:])
    assert (gi.tobytes(), gk.tobytes(), gd.tobytes()) == (pi[keep].tobytes(), pk[keep].tobytes(), dist[keep].tobytes())
    return gi, gk, gd


SEARCH = [(1, 1, 1), (1, 63, 3), (2, 64, 4), (3, 65, 5), (5, 257, 20), (2, 1025, 2), (9, 1030, 7)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_q,n_db,dim", SEARCH, ids=["q%d_db%d_d%d" % s for s in SEARCH])
def test_cross_candidates_equal_the_session_search_filtered(n_q, n_db, dim):
    """pi, pk and dist as bytes against ntsm_eval_candidates on the concatenation, filtered; radii of all three classes on
    both sides.  From 63 database samples on, both kinds of row must occur: a pair in a query's row and a pair in a database
    sample's row (the owner rule: the larger radius, the lower index on equal radii)."""
    cloud, radius = search_case(n_q, n_db, dim)
    gi, gk, _ = check_candidates(cloud, radius, n_q)
    if n_db >= 63:
        assert ((gi < n_q) & (gk >= n_q)).any() and (gi >= n_q).any(), (n_q, n_db, dim)
        assert len(gi) < n_q * (n_q + n_db)                                             # and the radii do cut


@pytest.mark.gpu
def test_cross_candidates_edge_cases():
    """All radii DBL_MAX (every pair, in the queries' rows); all equal and finite (every pair in the lower index's row); a
    radius that takes nothing; a database point equal to a query and two equal to each other (metric ties in one row come
    out by ascending k); capacity 0 returns the count and writes nothing; no query; no database."""
    import ntsm_amd.eval as ev
    n_q, n_db, dim = 3, 70, 4
    cloud, radius = search_case(n_q, n_db, dim, seed=1)
    n = n_q + n_db
    gi, gk, _ = check_candidates(cloud, np.full(n, DBL_MAX), n_q)
    assert len(gi) == n_q * (n_q - 1) // 2 + n_q * n_db and (gi < n_q).all()
    gi, gk, _ = check_candidates(cloud, np.full(n, radius[0]), n_q)
    assert len(gi) > 0 and (gi < n_q).all()                                             # equal radii: the lower index owns
    tiny = np.full(n, 1e-300)
    gi, gk, _ = check_candidates(cloud, tiny, n_q)
    assert len(gi) == 0
    mixed = radius.copy()
    mixed[1] = 1e-300                                                                   # one query whose radius takes nothing
    check_candidates(cloud, mixed, n_q)
    ties = cloud.copy()
    ties[n_q + 5] = ties[0]                                                             # a database point equal to query 0
    ties[n_q + 9] = ties[n_q + 40] = ties[n_q + 20]                                     # three equal to each other
    r = radius.copy()
    r[0] = r[n_q + 20] = float(np.percentile(radius[radius < DBL_MAX], 99))             # rows that see the ties
    gi, gk, gd = check_candidates(ties, r, n_q)
    row0 = gk[gi == 0]
    assert n_q + 5 in row0 and gd[(gi == 0) & (gk == n_q + 5)][0] == 0.0
    pos = [int(np.where(row0 == n_q + d)[0][0]) for d in (9, 20, 40) if n_q + d in row0]
    assert pos == sorted(pos)
    with pytest.raises(ValueError) as e:
        ev.cross_candidates(cloud[:n_q], radius[:n_q], cloud[n_q:], radius[n_q:], capacity=0)
    want = len(session_candidates(cloud, radius)[0])
    pi, pk, _ = session_candidates(cloud, radius)
    assert e.value.args[1] == int(((pi < n_q) | (pk < n_q)).sum()) <= want
    assert len(ev.cross_candidates(cloud[:0], radius[:0], cloud, radius)[0]) == 0       # no query: nothing has one
    gi, gk, _ = check_candidates(cloud[:5], radius[:5], 5)                              # no database: the session search itself
    assert len(gi) > 0


# ---------------------------------------------------------------------------------------------------- GPU: listed pairs
def check_score_pairs(q, db, pi, pk, c, chunk, passes=None):
    import ntsm_amd.eval as ev
    want = ev.score_pairs(np.concatenate([q, db]), pi, pk, min_cov=c)[0]
    got, times = ev.cross_score_pairs(q, ev.Records.of(db, HEAD), pi, pk, min_cov=c, db_chunk=chunk)
    assert got.tobytes() == want.tobytes()
    if passes is not None:
        assert times.chunks == passes
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 7, 300])
def test_cross_score_pairs_equal_session_records(m):
    """3 queries, 65 database samples of which 5 are named (one by several pairs, one a copy of a query, one without
    coverage, one with counts beyond 2^31), both orientations, a query-query pair; records as raw bytes against
    ntsm_eval_score_pairs on the concatenation, with db_chunk 1 (five passes), 2 (three) and 0 (one)."""
    rng = np.random.default_rng([7, m])
    n_q, n_db, c = 3, 65, 1
    s = random_samples(rng, n_q + n_db, m, depth=8.0)
    q, db = s[:n_q].copy(), s[n_q:].copy()
    db[0] = 0
    db[17] = q[1]
    db[64] = rng.integers(2**31, 2**32, size=(m, 2)).astype(np.uint32)
    D = lambda d: n_q + d  # noqa: E731
    pairs = [(0, D(17)), (D(17), 1), (2, D(17)), (D(64), 0), (1, D(0)), (0, 1), (2, 0), (D(33), 2), (1, D(40)), (D(40), 1), (0, D(64))]
    pi, pk = np.array([p[0] for p in pairs], dtype=np.uint32), np.array([p[1] for p in pairs], dtype=np.uint32)
    for chunk, passes in ((1, 5), (2, 3), (0, 1)):
        got = check_score_pairs(q, db, pi, pk, c, chunk, passes)
    if m > 1:
        assert got["n_valid"].max() > 0
    only_queries = check_score_pairs(q, db, pi[5:7], pk[5:7], c, 1, 1)                   # a list without any database sample
    assert only_queries.tobytes() == got[5:7].tobytes()


@pytest.mark.gpu
def test_cross_score_pairs_many_named_samples_in_passes():
    """9 queries against 1,030 x 24 sites: every database sample named once, in a shuffled order and alternating
    orientation, plus the query-query pairs; db_chunk 512 makes three passes whose records go back to list order."""
    rng = np.random.default_rng(77)
    n_q, n_db, m = 9, 1030, 24
    s = random_samples(rng, n_q + n_db, m, depth=30.0)
    q, db = s[:n_q].copy(), s[n_q:].copy()
    order = rng.permutation(n_db)
    pi = np.array([int(d) % n_q if x % 2 else n_q + int(d) for x, d in enumerate(order)] + [a for a in range(n_q) for b in range(a + 1, n_q)], dtype=np.uint32)
    pk = np.array([n_q + int(d) if x % 2 else int(d) % n_q for x, d in enumerate(order)] + [b for a in range(n_q) for b in range(a + 1, n_q)], dtype=np.uint32)
    got = check_score_pairs(q, db, pi, pk, 1, 512, 3)
    assert got["n_valid"].min() > 0                                                     # a record never written cannot pass


def test_cross_score_pairs_bad_lists_need_no_device():
    """-1 for an index out of range, for pi == pk and for a pair with no query in it; an empty list is no work"""
    import ntsm_amd.eval as ev
    q, db = np.ones((2, 5, 2), dtype=np.uint32), np.ones((4, 5, 2), dtype=np.uint32)
    for pi, pk in (([0], [6]), ([6], [0]), ([1], [1]), ([3], [4]), ([0, 2], [1, 3])):
        with pytest.raises(RuntimeError, match="failed: -1"):
            ev.cross_score_pairs(q, db, pi, pk)
    out, times = ev.cross_score_pairs(q, db, [], [])
    assert len(out) == 0 and times.chunks == 0


# ---------------------------------------------------------------------------------------------------- GPU: the CLI
def involving(text, queries):
    """header + the rows of a -p run in which sample 1 or sample 2 is a query, in order; and how many have a store sample as
    sample 1"""
    lines = text.split(b"\n")
    assert lines[-1] == b""
    q = set(x.encode() for x in queries)
    keep = [r for r in lines[1:-1] if r.split(b"\t", 2)[0] in q or r.split(b"\t", 2)[1] in q]
    owned_by_store = sum(1 for r in keep if r.split(b"\t", 1)[0] not in q)
    return b"".join(x + b"\n" for x in [lines[0]] + keep), owned_by_store


def without_pca(args):
    assert args[:4] == PCA
    return list(args[4:])


def index_args(args):
    """-p / -n and the flags the index fixes (-d, -c) of a -p run's arguments"""
    out = list(PCA)
    for flag in ("-d", "-c"):
        if flag in args:
            out += [flag, args[args.index(flag) + 1]]
    return out


def make_store(d, store, database, args):
    for f in (store, store + ".pcaidx"):
        if os.path.exists(os.path.join(str(d), f)):
            os.unlink(os.path.join(str(d), f))
    assert run(["--pack", store] + database, d).returncode == 0
    p = run(["--index", store] + index_args(args), d)
    assert p.returncode == 0 and p.stdout == b"", p.stderr[-300:]


def sig(x):
    return len(x), x.count(b"\n"), hashlib.sha256(x).hexdigest()


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"


@pytest.mark.gpu
@pytest.mark.parametrize("n_q", [1, 3])
@pytest.mark.parametrize("spec", TIE_FREE, ids=lambda s: "n%d_m%d_d%d" % (s[1], s[2], s[4]))
def test_cli_near_equals_the_pca_run_filtered(gpu, built, cohorts, restatement, spec, n_q):
    """--pack, --index, --near on the tie-free cohorts with the first 1 and the first 3 files as queries, -a, radii at the 15th
    and 60th percentile: stdout byte for byte, at -t 1 and -t 4, against the rows of `ntsmEval -p -n` over all files that
    name a query -- and against the reference class's where its binary is built.  Some of those rows must stand in a store
    sample's row, or the owner rule goes untested."""
    d, names, s, args = tie_free_args(restatement, cohorts, spec)
    queries, database = names[:n_q], names[n_q:]
    store = "near%d.store" % n_q
    make_store(d, store, database, args)
    want, owned_by_store = involving(stdout_of(EVAL, ["-t", "1"] + args, names, d), queries)
    assert owned_by_store >= 1 and want.count(b"\n") - 1 > owned_by_store
    for t in ("1", "4"):
        assert stdout_of(EVAL, ["-t", t] + without_pca(args) + ["--near", store], queries, d) == want, t
    if os.path.isfile(REF_EVAL):
        assert involving(reference(args, names, d), queries)[0] == want
    x = read_index(os.path.join(str(d), store + ".pcaidx"))
    assert (x["n"], x["m"], x["dim"], x["min_cov"]) == (len(database), spec[2], spec[4], 1)
    assert x["crc"] == locus_crc(os.path.join(str(d), store))
    a, b = s[n_q:, :, 0] > 1, s[n_q:, :, 1] > 1
    assert np.array_equal(x["geno"], np.stack([(a & b).sum(1), (a ^ b).sum(1), (~a & ~b).sum(1)], axis=1))


@pytest.mark.gpu
def test_cli_near_duplicate_cohort(gpu, built, cohorts, restatement):
    """The planted-duplicate cohort (40 x 3,000; sample 39 is a copy of sample 0, sample 3 is empty) with sample 0 as the
    query under the five flag sets of DUPLICATE_CASES (-d 5 and -c 2 among them: the index is rebuilt where they change).
    The query's copy sits in the store, so the default threshold prints a row.  Exact ties come out by k on both sides of the
    comparison, so it is byte for byte."""
    d, names, cases = duplicate_cases(restatement, cohorts)
    queries, database = names[:1], names[1:]
    owned = 0
    for args in cases:
        make_store(d, "dup.store", database, args)
        want, owned_by_store = involving(stdout_of(EVAL, ["-t", "1"] + args, names, d), queries)
        owned += owned_by_store
        assert want.count(b"\n") - 1 >= 1, args
        near = [a for a in without_pca(args)]
        assert stdout_of(EVAL, near + ["--near", "dup.store"], queries, d) == want, args
    assert owned >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("pick", ["two_queries", "empty_query"])
def test_cli_near_big_cohort(gpu, built, cohorts, restatement, pick):
    """1,030 x 64 sites, dim 3, by length, line count and SHA-256: with samples 0 and 1 as queries the empty sample 3 is a
    search-all row of the store that takes both; with the empty sample as the query its row is the whole store, which goes
    through ntsm_eval_cross."""
    d, names, s, args = tie_free_args(restatement, cohorts, BIG_PCA)
    if pick == "two_queries":
        queries, database = names[:2], names[2:]
    else:
        queries, database = names[3:4], names[:3] + names[4:]
    make_store(d, pick + ".store", database, args)
    want, owned_by_store = involving(stdout_of(EVAL, ["-t", "1"] + args, queries + database, d), queries)
    if pick == "two_queries":
        assert owned_by_store >= 2                                                      # at least the empty sample's row
    else:
        assert want.count(b"\n") - 1 == len(database) and owned_by_store == 0
    p = run(["-v", "-v"] + without_pca(args) + ["--near", pick + ".store"] + queries, d)
    assert p.returncode == 0 and sig(p.stdout) == sig(want), p.stderr[-300:]
    assert (b"1 dense rows" in p.stderr) == (pick == "empty_query")
    if os.path.isfile(REF_EVAL):
        assert sig(involving(reference(args, queries + database, d), queries)[0]) == sig(want)


@pytest.mark.gpu
def test_cli_index_append(gpu, built, cohorts, restatement):
    """Pack 8 samples and index them; pack 4 more: --near now refuses the stale index and names --index; --index again
    projects the tail only, and the index is byte for byte that of the 12-sample store indexed at once, --near's output the
    same, and equal to the -p run's rows."""
    d, names, s, args = tie_free_args(restatement, cohorts, TIE_FREE[2])
    queries, first, more = names[:1], names[1:9], names[9:13]
    make_store(d, "grow.store", first, args)
    make_store(d, "once.store", first + more, args)
    assert run(["--pack", "grow.store"] + more, d).returncode == 0
    before = snapshot(os.path.join(str(d), "grow.store.pcaidx"))
    p = run(without_pca(args) + ["--near", "grow.store"] + queries, d)
    assert p.returncode == 1 and p.stdout == b"" and b"Error: " in p.stderr and b"--index" in p.stderr
    assert unchanged(os.path.join(str(d), "grow.store.pcaidx"), before)
    p = run(["-v", "--index", "grow.store"] + index_args(args), d)
    assert p.returncode == 0 and b"Projected 4 samples" in p.stderr, p.stderr[-300:]
    grown, once = (open(os.path.join(str(d), x + ".store.pcaidx"), "rb").read() for x in ("grow", "once"))
    assert grown == once and read_index(os.path.join(str(d), "grow.store.pcaidx"))["n"] == 12
    want = involving(stdout_of(EVAL, ["-t", "1"] + args, queries + first + more, d), queries)[0]
    for store in ("grow.store", "once.store"):
        assert stdout_of(EVAL, without_pca(args) + ["--near", store], queries, d) == want, store
