"""The launches of the cohort-store tools that only a store of very many samples reaches ("Grids past
65,535"): a grid's second dimension ends at 65,535, and every device library of ntsmEval carries code that exists only because
of it -- launches cut into slices, a workgroup that strides over rows, a chunk capped at what one grid takes -- beside index
arithmetic that passes 2^32 late in a large triangle.  None of it runs below about 65,536 row groups, so the stores here have
2^16 to 2^24 samples over 1 to 3 sites: a few MB to 134 MB, a few seconds each.

The models.  rect_pairs and rect_contam are the per-pair models of tests/test_eval.py (vec_pairs) and tests/test_eval_contam.py
(model) over a rectangle rows x columns, vectorised over the pairs with a Python loop over the sites only; the doubles are
formed in site order with vec_pairs' operations, so their bits can be compared.  The CPU tests hold both against the models they
restate, field by field, doubles by their bits, and restate ntsm_eval_chunk.h's launch rule against the header itself.

The GPU tests compare every record with those models or with a numpy count; none has a tolerance.  Each prints its wall time."""
import math
import os
import subprocess
import time

import numpy as np
import pytest

from oracle_binding import ROOT
from test_eval import FIELDS, random_samples, vec_pairs
from test_eval_between import LACKS, remapped
from test_eval_contam import RECORD as CONTAM_RECORD
from test_eval_contam import edge_cells as contam_edge_cells
from test_eval_contam import model as contam_model
from test_eval_ld import Model as LdModel
from test_eval_near import synthetic_pca
from test_eval_qc import EVAL, HEAD, NAME, RECORD_HEAD, gpu  # noqa: F401
from test_eval_qc import model as profile_model

MAX_GRID_Y = 65535                                                                          # ntsm_eval_chunk::kMaxGridY
C, DEPTH = 1, 8                                                                             # min_cov and min_depth of every test here
INT_FIELDS = tuple(f for f in FIELDS if not f.startswith("sum"))


# ---------------------------------------------------------------------------------------------------- the models
def rect_pairs(rows, cols, c):
    """vec_pairs (tests/test_eval.py) over the rectangle rows [r][m][2] x cols [k][m][2]: {field: [r][k]}, the row's sample as
    sample 1.  The same operations in the same order over the sites: uint32 sums (they wrap as vec_pairs' do), elementwise
    float64 a / d, a * f + b * g, acc + x."""
    rows, cols = np.ascontiguousarray(rows, dtype=np.uint32), np.ascontiguousarray(cols, dtype=np.uint32)
    r, k, m = rows.shape[0], cols.shape[0], rows.shape[1]
    assert cols.shape[1] == m
    c = np.uint32(c)

    def term(x0, x1):
        d = (x0 + x1).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            f0 = np.where(x0 > c, x0.astype(np.float64) / d, 0.0)
            f1 = np.where(x1 > c, x1.astype(np.float64) / d, 0.0)
        return x0.astype(np.float64) * f0 + x1.astype(np.float64) * f1
    acc = {f: np.zeros((r, k), dtype=np.float64 if f.startswith("sum") else np.uint32) for f in FIELDS}
    for site in range(m):
        a0, a1, b0, b1 = rows[:, site, 0][:, None], rows[:, site, 1][:, None], cols[:, site, 0][None, :], cols[:, site, 1][None, :]
        valid = ((a0 > c) | (a1 > c)) & ((b0 > c) | (b1 > c))
        acc["sum_joint"] = np.where(valid, acc["sum_joint"] + term(a0 + b0, a1 + b1), acc["sum_joint"])
        acc["sum_single1"] = np.where(valid, acc["sum_single1"] + term(a0, a1), acc["sum_single1"])
        acc["sum_single2"] = np.where(valid, acc["sum_single2"] + term(b0, b1), acc["sum_single2"])
        h1, h2 = (a0 > c) & (a1 > c), (b0 > c) & (b1 > c)
        both_hom = valid & ~h1 & ~h2
        same_allele = (a0 > c) == (b0 > c)
        for f, x in (("n_valid", valid), ("hets1", valid & h1), ("homs1", valid & ~h1), ("hets2", valid & h2), ("homs2", valid & ~h2),
                     ("shared_hets", valid & h1 & h2), ("shared_homs", both_hom & same_allele), ("ibs0", both_hom & ~same_allele)):
            acc[f] += x
    acc["ibs2"] = acc["shared_hets"] + acc["shared_homs"]
    return acc


def rect_contam(rows, cols, c, depth):
    """model (tests/test_eval_contam.py) over the rectangle of targets rows [r][m][2] x sources cols [k][m][2]: (records [r][k],
    the targets' tallies [r][3]); integers throughout"""
    rows, cols = np.ascontiguousarray(rows, dtype=np.uint32), np.ascontiguousarray(cols, dtype=np.uint32)
    r, k, m = rows.shape[0], cols.shape[0], rows.shape[1]
    zero = np.uint64(0)
    rec = np.zeros((r, k), dtype=CONTAM_RECORD)
    tally = np.zeros((r, 3), dtype=np.uint64)
    minor, deep, sites = (np.zeros((3, r, k), dtype=t) for t in (np.uint64, np.uint64, np.uint32))
    for site in range(m):
        a, g = rows[:, site, 0].astype(np.uint64), rows[:, site, 1].astype(np.uint64)
        t, mn = a + g, np.minimum(a, g)
        informative, major_at = (t >= np.uint64(depth)) & (np.uint64(4) * mn < t), (a > g)[:, None]
        tally[:, 0] += informative
        tally[:, 1] += np.where(informative, mn, zero)
        tally[:, 2] += np.where(informative, t, zero)
        sa, sg = cols[:, site, 0][None, :], cols[:, site, 1][None, :]
        carries, has_major = np.where(major_at, sg, sa) > c, np.where(major_at, sa, sg) > c
        for x, cls in enumerate((~carries & has_major, carries & has_major, carries & ~has_major)):
            mask = cls & informative[:, None]
            sites[x] += mask
            minor[x] += np.where(mask, mn[:, None], zero)
            deep[x] += np.where(mask, t[:, None], zero)
    for x in range(3):
        rec["minor"][:, :, x], rec["depth"][:, :, x], rec["sites"][:, :, x] = minor[x], deep[x], sites[x]
    return rec, tally


def geno_of(db, c=C):
    """hets, homs, miss of every sample [n][3]: the numpy count of the tallies every store call returns"""
    a, b = db[:, :, 0] > c, db[:, :, 1] > c
    return np.stack([(a & b).sum(1), (a ^ b).sum(1), (~a & ~b).sum(1)], axis=1).astype(np.uint32)


def launch_shape(n_rows, n_cols):
    """ntsm_eval_chunk.h's launch_shape without forced values, restated: the row group 4, 2 or 1"""
    waves = (n_cols + 63) // 64
    for t in (4, 2):
        if t // 2 < n_rows and waves * ((n_rows + t - 1) // t) >= 1024:
            return t
    return 1


def pair_mismatches(rec, want):
    """(field, flat position) of the first fields of the library's records rec [...] that differ from the model's arrays of the same
    shape: doubles by their bits, integers by value"""
    out = []
    for f in FIELDS:
        g, w = np.ascontiguousarray(rec[f]), want[f]
        assert g.shape == w.shape, (f, g.shape, w.shape)
        ne = g.view(np.uint64) != w.view(np.uint64) if f.startswith("sum") else g != w.astype(g.dtype)
        out += [(f, int(p)) for p in np.flatnonzero(ne)[:5]]
    return out


def contam_mismatches(rec, want):
    return [(f, p.tolist()) for f in ("minor", "depth", "sites", "pad") for p in np.argwhere(rec[f] != want[f])[:5]]


# ---------------------------------------------------------------------------------------------------- the cells
# one cell of every kind at min_cov 1, min_depth 8: het, hom AT, hom CG below the depth, missing, both counts equal to min_cov,
# a hom with the other count equal to min_cov (either allele), a het just above min_cov, a count beyond 2^31, a het that is
# informative for --contam (minor 2 of 32), a deep hom CG, an informative hom AT (minor 1 of 13), both counts full
PALETTE = np.array([(5, 7), (9, 0), (0, 6), (0, 0), (1, 1), (1, 8), (8, 1), (2, 2), (3000000000, 7), (30, 2), (0, 12), (12, 1), (0xFFFFFFFF, 0xFFFFFFFF)],
                   dtype=np.uint32)
BEFORE = (0, 1, 10, 3, 4, 5)                            # the six samples before a boundary: het, hom AT, hom CG, missing, == min_cov, hom CG at min_cov
AFTER = (0, 6, 10)                                      # the three from it on: het, hom AT at min_cov, hom CG; then the empty sample and the copy


def draw(seed, n, m, boundaries=(), copy_of=None):
    """[n][m][2]: every cell drawn from PALETTE; around each boundary b (the first sample of the far side) the samples
    b - 8 ... b + 4, as far as they exist, are planted so that both sides hold a het, both homs, a missing cell and a count
    equal to min_cov, rotating from site to site: b - 8 a copy (of copy_of [m][2], else of sample b - 1), b - 7 empty, BEFORE,
    then AFTER, b + 3 empty, b + 4 a copy (of copy_of, else of sample b)"""
    rng = np.random.default_rng(seed)
    db = PALETTE[rng.integers(0, len(PALETTE), size=(n, m), dtype=np.uint8)]
    for b in boundaries:
        assert 8 <= b < n
        for k in range(len(BEFORE)):
            db[b - 6 + k] = PALETTE[[BEFORE[(k + s) % len(BEFORE)] for s in range(m)]]
        for k in range(len(AFTER)):
            if b + k < n:
                db[b + k] = PALETTE[[AFTER[(k + s) % len(AFTER)] for s in range(m)]]
        db[b - 7] = 0
        db[b - 8] = db[b - 1] if copy_of is None else copy_of
        if b + 3 < n:
            db[b + 3] = 0
        if b + 4 < n:
            db[b + 4] = db[b] if copy_of is None else copy_of
    return db


def classes(cells, c=C):
    """0 hom AT, 1 het, 2 hom CG, 3 missing of cells [...][2] under the scoring's rule"""
    a, g = cells[..., 0] > c, cells[..., 1] > c
    return np.where(a & g, 1, np.where(a, 0, np.where(g, 2, 3)))


def both_sides_differ(db, b):
    """the premise of a boundary test: on either side of b, as far as the store reaches, at least three genotype classes and a
    count equal to min_cov, and the samples b - 1 and b in different classes at every site"""
    lo, hi = db[b - 6:b], db[b:b + 3]
    assert len(set(classes(lo).ravel().tolist())) == 4 and (lo == C).any(), b
    assert len(set(classes(hi).ravel().tolist())) >= 3 and (hi == C).any(), b
    assert (classes(db[b - 1]) != classes(db[b])).all(), b


_cache = {}


def cached(key, make):
    """computed once per session, shared by the tests that need it and left unchanged"""
    if key not in _cache:
        value = make()
        for x in (value if isinstance(value, tuple) else (value,)):
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        _cache[key] = value
    return _cache[key]


def dense(ev, db):
    """a dense array as Records without the copy Records.of makes"""
    db = np.ascontiguousarray(db, dtype=np.uint32)
    return ev.Records(db.reshape(-1).view(np.uint8), 0, 8 * db.shape[1], db.shape[0], db.shape[1])


@pytest.fixture(autouse=True)
def wall_time(request):
    t = time.perf_counter()
    yield
    print("\n[many samples] %s: %.2f s" % (request.node.name, time.perf_counter() - t))


# ---------------------------------------------------------------------------------------------------- CPU
def small_cohort(seed, n, m):
    """the edge cells the per-pair tests plant: an empty sample, a copy, counts at and beyond 2^31, counts equal to min_cov"""
    rng = np.random.default_rng(seed)
    s = random_samples(rng, n, m, depth=8.0)
    s[1] = 0
    s[n - 2] = s[0]
    s[2] = rng.integers(2**31, 2**32, size=(m, 2)).astype(np.uint32)
    s[3] = rng.integers(0, 3, size=(m, 2)).astype(np.uint32)                                 # 0, min_cov and min_cov + 1
    s[n - 1, ::2] = C
    return s


def test_rect_pairs_equal_vec_pairs_bits():
    """rect_pairs against vec_pairs, the model it restates, on 13 samples x 40 sites with an empty sample, a copy, counts beyond
    2^31 and counts equal to min_cov, at min_cov 0, 1 and 3: the square of all samples against its upper triangle, and a 5 x 8
    rectangle cut across those samples, every field, the doubles by their bits"""
    n, m = 13, 40
    s = small_cohort(5, n, m)
    iu = np.triu_indices(n, 1)
    for c in (0, 1, 3):
        want = vec_pairs(s, c)
        square = rect_pairs(s, s, c)
        part = rect_pairs(s[:5], s[5:], c)
        where = np.full((n, n), -1)
        where[iu] = np.arange(len(iu[0]))
        for f in FIELDS:
            bits = (lambda x: np.ascontiguousarray(x).view(np.uint64)) if f.startswith("sum") else (lambda x: np.asarray(x).astype(np.int64))
            assert np.array_equal(bits(square[f][iu]), bits(want[f])), (f, c)
            assert np.array_equal(bits(part[f]), bits(want[f][where[:5, 5:]])), (f, c)
        assert want["n_valid"].max() > 0 and (want["n_valid"] == 0).any()
    assert square["sum_joint"].dtype == np.float64 and square["ibs2"].dtype == np.uint32


def test_rect_contam_equals_the_contam_model():
    """rect_contam against test_eval_contam.model on that file's edge cells (70 samples x 5 sites: t = D - 1 and D, t past 2^32,
    both counts full, sources at c and c + 1) and on the small cohort: whole square and a band of targets 3 ... 7, every field"""
    for db in (contam_edge_cells(np.random.default_rng(9), 70, 5, C, DEPTH), small_cohort(6, 13, 40)):
        want, want_tally = contam_model(db, C, DEPTH)
        for first, count in ((0, len(db)), (3, 5)):
            rec, tally = rect_contam(db[first:first + count], db, C, DEPTH)
            assert not contam_mismatches(rec, want[first:first + count]), (db.shape, first)
            assert tally.dtype == want_tally.dtype and np.array_equal(tally, want_tally[first:first + count])
        assert want["sites"].max() > 0


def test_launch_rule_picks_the_groups_these_tests_rely_on(tmp_path):
    """ntsm_eval_chunk.h's launch_shape restated in Python: 9 and 3 rows against 32,769 columns get groups 4 and 2 -- the
    premise of test_the_launch_rules_own_choice -- and one row or a narrow rectangle gets 1.  The header itself, compiled into a
    program that prints its choice (tests/eval_launch_shape_print.cpp), answers the same on those shapes and on a sweep around the
    rule's edges: if the rule moves, this test says so before the GPU test loses its subject."""
    assert [launch_shape(*s) for s in ((9, 32769), (3, 32769), (9, 32769), (3, 32769))] == [4, 2, 4, 2], "the rule moved: the premise is gone"
    assert launch_shape(1, 4194305) == 1 and launch_shape(262145, 2) == 4 and launch_shape(2, 32769) == 1 and launch_shape(2, 65473) == 2
    exe = str(tmp_path / "launch_shape_print")
    p = subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O1", "-std=c++17", "--offload-arch=gfx950", "-o", exe,
                        os.path.join(ROOT, "tests", "eval_launch_shape_print.cpp")], capture_output=True)
    assert p.returncode == 0, p.stderr[-2000:]
    shapes = [(r, k) for r in (1, 2, 3, 4, 5, 8, 9, 16, 17, 1023, 1024, 4096, 262145) for k in (1, 2, 64, 65, 16320, 16321, 21760, 21761, 32704, 32705, 32769, 65473, 4194305)]
    p = subprocess.run([exe] + [str(x) for s in shapes for x in s], capture_output=True, check=True)
    got = [tuple(int(x) for x in line.split()) for line in p.stdout.decode().splitlines()]
    assert got == [(64, launch_shape(r, k)) for r, k in shapes], [(s, g) for s, g in zip(shapes, got) if g != (64, launch_shape(*s))][:5]
    assert {g for _, g in got} == {1, 2, 4}


# ---------------------------------------------------------------------------------------------------- GPU: a. between, sliced
N_A, SLICE = 262145, 4 * MAX_GRID_Y                                                          # 262,140 rows of A fill one launch of ntsm_eval_between_kernel


def between_case():
    """A of 262,145 samples x 2 sites, B of 3 samples over the same sites (a het and a hom AT; a deep hom CG and a het beyond 2^31;
    a hom AT at min_cov and a het just above it; A's copies are copies of B's sample 0), and the model of the rectangle"""
    def make():
        b = PALETTE[[[0, 1], [10, 8], [6, 7]]]
        a = draw(32, N_A, 2, [SLICE], copy_of=b[0])
        both_sides_differ(a, SLICE)
        return a, b, rect_pairs(a, b, C)
    return cached("between", make)


def check_named_rows(rec, want, rows, what):
    """the rows named, one by one"""
    for r in rows:
        bad = pair_mismatches(rec[r], {f: v[r] for f, v in want.items()})
        assert not bad, "%s: row %d differs from the model: %s" % (what, r, bad)


@pytest.mark.gpu
def test_between_second_slice_of_a_band(gpu):
    """a.  Between(A, B).rows(0, 262,145): launch_between cuts the band after 262,140 rows, and the second launch reads the rows
    at rows.at + y0 and writes at d_out + y0 * out_pitch.  Every field of every record against rect_pairs, rows 262,136 ...
    262,144 by name, a_geno and b_geno against a numpy count; the bands (0, 262,140) and (262,140, 5) give the one call's bytes.
    Then B with 3 sites in another order, lacking A's site 1: the same against the model on B remapped by numpy."""
    ev = gpu
    a, b, want = between_case()
    with ev.Between(dense(ev, a), dense(ev, b), min_cov=C) as s:
        rec, a_geno, b_geno, times = s.rows(0, N_A)
        assert times.chunks == 0                                                            # B resident: one launch_between call for the band
        check_named_rows(rec, want, range(SLICE - 4, N_A), "identical tables")
        assert not pair_mismatches(rec, want)
        assert np.array_equal(a_geno, geno_of(a)) and np.array_equal(b_geno, geno_of(b))
        lo, hi = s.rows(0, SLICE), s.rows(SLICE, N_A - SLICE)
        assert lo[0].tobytes() + hi[0].tobytes() == rec.tobytes()
        assert np.array_equal(np.concatenate([lo[1], hi[1]]), a_geno) and np.array_equal(hi[2], b_geno)
    assert (want["n_valid"][SLICE:] > 0).any() and (want["n_valid"][SLICE:] == 0).any()      # written records, and the empty sample's
    site_map = np.array([2, LACKS], dtype=np.uint32)                                        # A's site 0 is B's site 2; B lacks A's site 1
    b3 = draw(33, 3, 3)
    b3[:, 2] = b[:, 0]
    over_a = remapped(b3, site_map)
    want = rect_pairs(a, over_a, C)
    with ev.Between(dense(ev, a), dense(ev, b3), site_map=site_map, min_cov=C) as s:
        rec, a_geno, b_geno, _ = s.rows(0, N_A)
    check_named_rows(rec, want, range(SLICE - 4, N_A), "mapped")
    assert not pair_mismatches(rec, want)
    assert np.array_equal(a_geno, geno_of(a)) and np.array_equal(b_geno, geno_of(over_a)) and b_geno[:, 2].min() >= 1


# ---------------------------------------------------------------------------------------------------- GPU: b. the same through the CLI
def write_big_store(path, counts, prefix, loci, rng):
    """tests/test_eval_qc.py's write_store for very many samples: the same layout and scalars, the records
    formed as one structured array.  Returns what the rows' text needs: (names, cov, error rate) per sample."""
    import struct
    counts = np.ascontiguousarray(counts, dtype="<u4")
    n, m = counts.shape[0], counts.shape[1]
    distinct = rng.integers(1, 30, size=(m, 2)).astype("<u4")
    section = b"".join(l.encode() + b"\0" for l in loci)
    section += bytes(-(HEAD + len(section)) % 8) + distinct.tobytes()
    first, stride = HEAD + len(section), RECORD_HEAD + 8 * m
    rec = np.zeros(n, dtype=np.dtype([("raw_total", "<u8"), ("total", "<u8"), ("sum_of_sums", "<u8"), ("ks", "<u4"), ("reserved", "<u4"), ("name", "S%d" % NAME),
                                      ("counts", "<u4", (m, 2))]))
    assert rec.dtype.itemsize == stride
    total = counts.astype(np.uint64).sum(axis=(1, 2))
    rec["raw_total"], rec["sum_of_sums"], rec["ks"] = total * 7 + 1000, total * 3, 19
    rec["total"] = (counts[:, :, 0] + counts[:, :, 1]).astype(np.uint64).sum(axis=1)        # the sites' uint32 line sums, widened
    names = ["%s%06d.txt" % (prefix, r) for r in range(n)]
    rec["name"], rec["counts"] = np.array(names, dtype="S%d" % NAME), counts
    with open(str(path), "wb") as f:
        f.write(b"NTSMCOH1" + struct.pack("<IIQQQ", 1, m, n, first, stride) + bytes(24) + section)
        rec.tofile(f)
    return names, rec, distinct


def store_summaries(rec, m, distinct_sum, genome=6200000000):
    """cov and errorRate of every sample of a store as appendStoreSamples (ntsm_eval_main.cpp) forms them: double(total) / double(m)
    and eval_store.hpp's error_rate, in Python floats (IEEE doubles; math.pow is the C library's pow)"""
    cov = [float(int(t)) / float(m) for t in rec["total"]]
    err = []
    for raw, ks, sos in zip(rec["raw_total"].tolist(), rec["ks"].tolist(), rec["sum_of_sums"].tolist()):
        if not (raw > 0 and ks > 0):
            err.append(-1.0)
            continue
        expected = float(raw) * float(distinct_sum) / float(genome)
        with np.errstate(all="ignore"):
            err.append(float(np.float64(1.0) - np.float64(math.pow(float(np.float64(sos) / np.float64(expected)), 1.0 / float(ks)))))
    return cov, err


def to_string(x):
    """std::to_string(double): printf's %f, which prints a NaN with its sign"""
    x = float(x)
    if math.isnan(x):
        return "-nan" if math.copysign(1.0, x) < 0 else "nan"
    return "%f" % x


def pair_row(name1, name2, r, s1, s2, g1, g2, skew=0.2, thresh=0.5):
    """printRow (eval_cli_rows.hpp) under -a for one record r (a dict of Python numbers): the expressions of pairScore and resultsStr
    in numpy doubles, so that a division by zero gives the infinity or the NaN, sign included, that the C++ expression gives"""
    f8 = np.float64
    with np.errstate(all="ignore"):
        score = f8(1.7976931348623157e308)
        if r["n_valid"] > 0:
            score = f8(-2.0) * (f8(r["sum_joint"]) - (f8(r["sum_single1"]) + f8(r["sum_single2"])))
            score = score / f8(math.pow(s1[0] * s2[0], skew))
            score = score / f8(float(r["n_valid"]))
        hom = (f8(float(r["shared_homs"])) - f8(2.0) * f8(float(r["ibs0"]))) / f8(float(min(r["homs1"], r["homs2"])))
        relate = (f8(float(r["shared_hets"])) - f8(2.0) * f8(float(r["ibs0"]))) / f8(float(min(r["hets1"], r["hets2"])))
    out = [name1, name2, to_string(score), "1" if score < thresh else "0", "-1", to_string(relate), "%d" % r["ibs0"], "%d" % r["ibs2"], to_string(hom)]
    out += ["%d" % r[f] for f in ("hets1", "hets2", "shared_hets", "homs1", "homs2", "shared_homs", "n_valid")]
    out += [to_string(s1[0]), to_string(s2[0]), to_string(s1[1]), to_string(s2[1])]
    out += ["%d" % v for v in (g1[2], g2[2], g1[1], g2[1], g1[0], g2[0])]
    return "\t".join(out) + "\n"


@pytest.mark.gpu
def test_cli_between_a_biobank_against_three_samples(gpu, tmp_path):
    """b.  `ntsmEval -a --between A B` on the stores of case a written to disk: B has at most 64 samples, so eval_between.hpp's band
    rule puts all 262,145 rows of A into one band -- the sliced launch, from the command line.  The run reports one band; stdout
    has a row for every pair, and the rows of A's samples 262,130 ... 262,144 are the text formed from the model's records."""
    a, b, want = between_case()
    rng = np.random.default_rng(34)
    loci = ["rs%d" % (3 * s + 1) for s in range(2)]
    names_a, rec_a, distinct = write_big_store(tmp_path / "A.store", a, "a/run", loci, rng)
    names_b, rec_b, _ = write_big_store(tmp_path / "B.store", b, "b/run", loci, rng)
    with open(str(tmp_path / "out.tsv"), "wb") as out:
        p = subprocess.run([EVAL, "-a", "-v", "-v", "--between", "A.store", "B.store"], stdout=out, stderr=subprocess.PIPE, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-500:]
    assert b"store between: loci identical (0 of 2 absent from B.store), B resident, 1 bands, 0 chunks" in p.stderr, p.stderr[-500:]
    lines = open(str(tmp_path / "out.tsv"), "rb").read().split(b"\n")
    assert lines[-1] == b"" and len(lines) == 1 + N_A * 3 + 1 and lines[0].startswith(b"sample1\tsample2\tscore\t")
    distinct_sum = int((distinct[:, 0] + distinct[:, 1]).astype(np.uint64).sum())
    first = 262130
    sum_a, sum_b = store_summaries(rec_a[first:], 2, distinct_sum), store_summaries(rec_b, 2, distinct_sum)
    geno_a, geno_b = geno_of(a[first:]).tolist(), geno_of(b).tolist()
    text = []
    for i in range(first, N_A):
        for j in range(3):
            r = {f: want[f][i, j].item() for f in FIELDS}
            k = i - first
            text.append(pair_row(names_a[i], names_b[j], r, (sum_a[0][k], sum_a[1][k]), (sum_b[0][j], sum_b[1][j]), geno_a[k], geno_b[j]))
    got = [l.decode() + "\n" for l in lines[1 + first * 3:-1]]
    assert got == text, [(g, w) for g, w in zip(got, text) if g != w][:2]
    assert any("\t1\t-1\t" in t for t in text) and any("\t0\t-1\t" in t for t in text)      # rows either side of the threshold


# ---------------------------------------------------------------------------------------------------- GPU: c. between-near remap
@pytest.mark.gpu
def test_remap_rows_past_one_grid(gpu):
    """c.  ntsm_eval_project_store_mapped on a B of 65,601 samples x 3 sites through a map onto 4 sites of A, in one chunk: the
    remap's grid has 65,535 rows, so its workgroups take a second trip for rows 65,535 ... 65,600.  The cloud is, bit for bit,
    ntsm_eval_project_store's on the cells remapped by numpy, and the tallies are numpy's count.  Then
    ntsm_eval_between_score_pairs on pairs that name B's samples 0, 65,534, 65,535, 65,536 and 65,600 against rect_pairs."""
    ev = gpu
    n_b = 65601
    b = draw(41, n_b, 3, [MAX_GRID_Y])
    both_sides_differ(b, MAX_GRID_Y)
    site_map = np.array([2, LACKS, 0, 1], dtype=np.uint32)
    over_a = remapped(b, site_map)
    norm, rot = synthetic_pca(np.random.default_rng(42), 4, 2)
    cloud, geno, times = ev.project_store_mapped(dense(ev, b), 4, site_map, norm, rot, min_cov=C)
    assert times.chunks == 1                                                                # one remap launch for all 65,601 rows
    want_cloud = ev.project_store(dense(ev, over_a), norm, rot, min_cov=C)[0]
    differ = np.flatnonzero((cloud.view(np.uint64) != want_cloud.view(np.uint64)).any(axis=1))
    assert differ.size == 0, differ[:5].tolist()
    assert np.array_equal(geno, geno_of(over_a))
    assert len(np.unique(cloud[MAX_GRID_Y - 6:MAX_GRID_Y + 3], axis=0)) > 3                  # different samples either side, not one value
    a = draw(43, 7, 4)
    a[5] = over_a[MAX_GRID_Y]                                                               # a copy of the first row of the second trip
    named = [0, 65534, 65535, 65536, 65600]
    pi = np.repeat(np.arange(7, dtype=np.uint32), len(named))
    pk = np.tile(np.array(named, dtype=np.uint32) + 7, 7)
    rec, _ = ev.between_score_pairs(dense(ev, a), dense(ev, b), pi, pk, site_map=site_map, min_cov=C)
    want = rect_pairs(a, over_a[named], C)
    assert not pair_mismatches(rec.reshape(7, len(named)), want)
    assert want["n_valid"].max() > 0


# ---------------------------------------------------------------------------------------------------- GPU: d. LD planes
@pytest.mark.gpu
def test_ld_planes_in_two_slices(gpu):
    """d.  4,194,305 samples x 2 sites in one chunk: 65,537 sample words, so ntsm_eval_ld_open launches the planes kernel twice,
    for the words 0 ... 65,534 and for 65,535 and 65,536.  site_geno and the records of rows(0, 2) against column counts in
    numpy (tests/test_eval_ld.py's Model); both sites have called samples in the words 65,535 and 65,536."""
    ev = gpu
    n = 64 * MAX_GRID_Y + 65
    db = draw(51, n, 2, [64 * MAX_GRID_Y])
    db[n - 1] = PALETTE[[0, 10]]                                                            # word 65,536 holds this sample alone: a het and a deep hom CG
    model = LdModel(db, C, DEPTH)
    for lo, hi in ((64 * MAX_GRID_Y, 64 * MAX_GRID_Y + 64), (n - 1, n)):
        assert model.C[lo:hi].any(axis=0).all() and model.H[lo:hi].any() and not model.C[lo - 64:hi].all()
    with ev.Ld(dense(ev, db), min_cov=C, min_depth=DEPTH) as s:
        assert s.times.chunks == 1                                                          # the slicing ran, not the chunking
        rec, _ = s.rows(0, 2)
        assert np.array_equal(s.site_geno, model.site_geno), (s.site_geno.tolist(), model.site_geno.tolist())
    assert rec.tobytes() == model.rec.tobytes(), (rec.tolist(), model.rec.tolist())


# ---------------------------------------------------------------------------------------------------- GPU: e. profile cap
@pytest.mark.gpu
def test_profile_chunk_capped_at_one_grid(gpu):
    """e.  16,777,217 samples x 1 site at db_chunk 0: memory would take them in one chunk, the grid takes 65,535 strips of 256,
    so a second chunk of 257 samples follows; its tallies land at d_geno + 3 * 16,776,960.  geno, site_tally and site_cov
    against numpy; the samples either side of the cut belong to different classes."""
    ev = gpu
    cut = 256 * MAX_GRID_Y
    n = cut + 257
    db = draw(61, n, 1, [cut])
    both_sides_differ(db, cut)
    geno, tally, cov, times = ev.store_profile(dense(ev, db), C, 0)
    assert times.chunks == 2
    want_geno, want_tally, want_cov = profile_model(db, C)
    for r in range(cut - 4, cut + 5):
        assert geno[r].tolist() == want_geno[r].tolist(), "sample %d" % r
    differ = np.flatnonzero((geno != want_geno).any(axis=1))
    assert differ.size == 0, differ[:5].tolist()
    assert np.array_equal(tally, want_tally) and np.array_equal(cov, want_cov), (tally.tolist(), want_tally.tolist(), cov.tolist(), want_cov.tolist())


# ---------------------------------------------------------------------------------------------------- GPU: f. the rule's own choice
def store_32769():
    def make():
        db = draw(71, 32769, 3, [32768])
        db[0] = PALETTE[[9, 11, 1]]                                                         # targets that are informative for --contam
        db[7] = PALETTE[[11, 9, 10]]
        return db
    return cached("32769", make)


@pytest.mark.gpu
def test_the_launch_rules_own_choice(gpu):
    """f.  Nothing forced: 9 and 3 queries against 32,769 samples x 3 sites, and the contamination bands (0, 9) and (7, 3) of a
    32,769-sample store, are the shapes at which ntsm_eval_chunk.h's launch rule picks a row group of 4 and of 2 by itself
    (test_launch_rule_picks_the_groups_these_tests_rely_on holds that premise).  Cross against rect_pairs, contam against
    rect_contam, every field."""
    ev = gpu
    db = store_32769()
    ev.lib.ntsm_eval_cross_tune(0, 0)                                                       # (0, 0) = the rule: the forcing is process-wide, and a test
    ev.lib.ntsm_eval_contam_tune(0, 0)                                                      # that ran earlier in this process may have left it on
    for n_q in (9, 3):
        q = draw(72 + n_q, n_q, 3)
        q[n_q - 1] = db[32768]
        rec, geno, times = ev.cross(q, db, min_cov=C)
        assert times.chunks == 1 and launch_shape(n_q, 32769) == (4 if n_q == 9 else 2)
        assert not pair_mismatches(rec, rect_pairs(q, db, C)), n_q
        assert np.array_equal(geno, geno_of(db))
    with ev.Contam(dense(ev, db), min_cov=C, min_depth=DEPTH) as s:
        for first, count in ((0, 9), (7, 3)):
            rec, tally, times = s.rows(first, count)
            assert times.chunks == 0 and launch_shape(count, 32769) == (4 if count == 9 else 2)
            want, want_tally = rect_contam(db[first:first + count], db, C, DEPTH)
            assert not contam_mismatches(rec, want), (first, count)
            assert np.array_equal(tally, want_tally) and want["sites"].max() > 0


# ---------------------------------------------------------------------------------------------------- GPU: g. within past 2^32
@pytest.mark.gpu
def test_within_band_past_two_to_the_32(gpu):
    """g.  100,001 samples x 1 site: from row 62,449 on (computed here) a band's base (eval_within.hpp's band_base) and every pair
    index in it lie past 2^32.  The 8 rows from the first such row against rect_pairs at pair_index, and as two bands of 3 and 5
    rows."""
    ev = gpu
    n = 100001
    base = lambda r: r * n - r * (r + 1) // 2  # noqa: E731
    first = next(r for r in range(n) if base(r) > 2**32)
    assert base(first - 1) <= 2**32 < base(first) and first + 8 < n and ev.pair_index(first, first + 1, n) == base(first)
    db = draw(81, n, 1, [first, first + 8, n - 5])
    with ev.Within(dense(ev, db), min_cov=C) as w:
        rec, geno, times = w.rows(first, 8)
        two = w.rows(first, 3)[0].tobytes() + w.rows(first + 3, 5)[0].tobytes()
    assert times.chunks == 0 and len(rec) == base(first + 8) - base(first)
    want = rect_pairs(db[first:first + 8], db, C)
    at = 0
    for k in range(8):
        i = first + k
        assert ev.pair_index(i, i + 1, n) - base(first) == at
        bad = pair_mismatches(rec[at:at + n - i - 1], {f: v[k, i + 1:] for f, v in want.items()})
        assert not bad, (i, bad)
        at += n - i - 1
    assert at == len(rec) and rec["n_valid"].max() > 0 and two == rec.tobytes()
    assert np.array_equal(geno[first:], geno_of(db)[first:])


# ---------------------------------------------------------------------------------------------------- GPU: h. launches that were not cut
N_WIDE = 64 * MAX_GRID_Y + 65                                                               # 4,194,305 samples: 65,537 tiles of the transposes


def wide_store():
    def make():
        db = draw(91, N_WIDE, 1, [64 * MAX_GRID_Y])
        db[0] = PALETTE[9]                                                                  # target 0 is informative: (30, 2)
        both_sides_differ(db, 64 * MAX_GRID_Y)
        return db
    return cached("wide", make)


@pytest.mark.gpu
def test_cross_one_query_against_four_million_samples(gpu):
    """h.  1 query against 4,194,305 samples x 1 site in one chunk: the transpose of the chunk has 65,537 tiles of 64 samples and
    goes out in two launches.  Every record against rect_pairs, the columns 4,194,236 ... 4,194,243 by name, the tallies against
    numpy."""
    ev = gpu
    db = wide_store()
    q = PALETTE[[0]].reshape(1, 1, 2)
    rec, geno, times = ev.cross(q, db, min_cov=C)
    assert times.chunks == 1
    want = rect_pairs(q, db, C)
    for d in range(64 * MAX_GRID_Y - 4, 64 * MAX_GRID_Y + 4):
        bad = pair_mismatches(rec[:, d], {f: v[:, d] for f, v in want.items()})
        assert not bad, "column %d differs from the model: %s" % (d, bad)
    assert not pair_mismatches(rec, want)
    assert np.array_equal(geno, geno_of(db))
    assert (want["n_valid"][0, 64 * MAX_GRID_Y:] > 0).any()


@pytest.mark.gpu
def test_contam_one_target_against_four_million_sources(gpu):
    """h.  Contam.rows(0, 1) on the same store, resident: ntsm_eval_contam.hip's own transpose has 65,537 tiles.  Every record
    against rect_contam, the columns either side of 4,194,240 by name, the target's tally."""
    ev = gpu
    db = wide_store()
    with ev.Contam(dense(ev, db), min_cov=C, min_depth=DEPTH) as s:
        rec, tally, times = s.rows(0, 1)
    assert times.chunks == 0
    want, want_tally = rect_contam(db[:1], db, C, DEPTH)
    for d in range(64 * MAX_GRID_Y - 4, 64 * MAX_GRID_Y + 4):
        bad = contam_mismatches(rec[:, d:d + 1], want[:, d:d + 1])
        assert not bad, "column %d differs from the model: %s" % (d, bad)
    assert not contam_mismatches(rec, want)
    assert np.array_equal(tally, want_tally) and len(set(want["sites"][0, 64 * MAX_GRID_Y:].ravel().tolist())) > 1


@pytest.mark.gpu
def test_between_mapped_staging_of_four_million_columns(gpu):
    """h.  ntsm_eval_between.hip's gathering transpose, the third copy of that launch: B is the same store seen through a map
    (A has 2 sites, B's one site is A's site 1), one row of A.  Records and b_geno against the model on B remapped by numpy."""
    ev = gpu
    b = wide_store()
    site_map = np.array([LACKS, 0], dtype=np.uint32)
    a = PALETTE[[1, 0]].reshape(1, 2, 2)
    over_a = remapped(b, site_map)
    with ev.Between(a, dense(ev, b), site_map=site_map, min_cov=C) as s:
        rec, a_geno, b_geno, times = s.rows(0, 1)
    assert times.chunks == 0
    want = rect_pairs(a, over_a, C)
    for d in range(64 * MAX_GRID_Y - 4, 64 * MAX_GRID_Y + 4):
        bad = pair_mismatches(rec[:, d], {f: v[:, d] for f, v in want.items()})
        assert not bad, "column %d differs from the model: %s" % (d, bad)
    assert not pair_mismatches(rec, want)
    assert np.array_equal(b_geno, geno_of(over_a)) and np.array_equal(a_geno, geno_of(a))


@pytest.mark.gpu
def test_cross_a_quarter_million_queries(gpu):
    """h.  262,145 queries against 2 samples x 2 sites: the rule gives a query group of 4, so the cross kernel's grid has 65,537
    rows of groups and goes out in two launches, the second from query 262,140 on.  Every record against rect_pairs, the queries
    262,136 ... 262,144 by name."""
    ev = gpu
    a, b, want = between_case()                                                             # A's samples as queries: the rectangle of case a
    assert launch_shape(N_A, 2) == 4
    ev.lib.ntsm_eval_cross_tune(0, 0)                                                       # the rule, whatever an earlier test forced
    rec, geno, times = ev.cross(a, b[:2], min_cov=C)
    assert times.chunks == 1
    part = {f: v[:, :2] for f, v in want.items()}
    check_named_rows(rec, part, range(SLICE - 4, N_A), "cross")
    assert not pair_mismatches(rec, part)
    assert np.array_equal(geno, geno_of(b[:2]))
