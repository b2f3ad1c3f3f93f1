"""ntsmEval --between-near STORE_A STORE_B: the PCA-guided search between two cohort stores through
A's index, B's loci matched to A's by ID.  Device side: ntsm_eval_project_store_mapped and ntsm_eval_between_score_pairs
(ntsm_amd/csrc/ntsm_eval_between_near.hip), ntsm_eval_between_candidates (ntsm_eval_near.hip); host side:
ntsm_amd/csrc/host/eval_between.hpp (b_index_usable, dense_runs).

CPU: the surface, every refusal (indexes are written here from the documented layout), the calls that need no device, and the
host decisions under the host sanitizers (`make between_near_check`).
GPU: each entry point as raw bytes against the session call it mirrors on the dense concatenation [A; B remapped to A's
sites], and the CLI's stdout byte for byte against `build/ntsmEval -p -n` over [A's files, B's files] filtered to the rows that
pair a file of one store with a file of the other -- a path this feature does not touch and that tests/test_eval_reference.py
holds to the reference class -- against the restatement and, where it is built, oracle/_ref/ref_ntsmEval itself.  No comparison
has a tolerance."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle_binding import ROOT
from test_eval import EVAL, random_samples, write_counts
from test_eval_between import LACKS, mapped_case, remapped
from test_eval_near import (DBL_MAX, HEAD, gpu, index_args, index_bytes, loaded_pca, locus_crc, make_store, search_case,  # noqa: F401
                            session_candidates, sig, synthetic_pca, without_pca)
from test_eval_pca import write_pca
from test_eval_reference import (BIG_PCA, REF_EVAL, TIE_FREE, cohorts, duplicate_cases, pca_expected, reference, restatement,  # noqa: F401
                                 same_up_to_tie_order, stdout_of, tie_free_args)
from test_eval_store import read_store, run, seven_files, snapshot, unchanged
from test_eval_within import greedy_passes

SYMBOLS = ("ntsm_eval_project_store_mapped", "ntsm_eval_between_candidates", "ntsm_eval_between_score_pairs")


# ---------------------------------------------------------------------------------------------------- CPU
def test_surface():
    """The three entry points are exported and declared; the help text names the run under "This build only" and says where
    STORE_B goes; eval_between.hpp states the rule for B's index."""
    import ntsm_amd.eval as ev
    hdr = open(os.path.join(ROOT, "include", "ntsm_eval_hip.h")).read()
    for name in SYMBOLS:
        assert hasattr(ev.lib, name), name
        assert "int %s(int device, " % name in hdr, name
    for name in ("project_store_mapped", "between_candidates", "between_score_pairs"):
        assert callable(getattr(ev, name)), name
    host = open(os.path.join(ROOT, "ntsm_amd", "csrc", "host", "eval_between.hpp")).read()
    assert "inline bool b_index_usable(" in host and "dense_runs(" in host
    p = subprocess.run([EVAL, "--help"], capture_output=True)
    assert p.returncode == 0 and p.stdout == b""
    ours = p.stderr.split(b"This build only")[1]
    assert b"--between-near = STORE_A STORE_B" in ours and b"positional" in ours.split(b"--between-near = ")[1]
    assert b"--between = STORE_A STORE_B" in ours and b"--within-near = STORE" in ours and b"--pack" in ours    # and what was there is


def test_refusals(tmp_path):
    """Every refusal of --between-near: its sentence, exit 1, one 'Error:' line, nothing on stdout, no GPU work (this test runs
    without one), every store and index -- bytes and mtime -- as they were.  Over the 40 loci of seven_files: S with a current
    index and T are good; `stale` holds 4 samples and an index of 3; `magic`, `loci` and `short` have an index with a broken
    magic, for other loci, a byte short; `bare` has none; `alien` lists a locus S lacks, `dup` lists one twice, `empty` holds no
    sample, `trunc` is a byte short."""
    names = seven_files(tmp_path)[0]
    write_pca(tmp_path, 40, 3, np.random.default_rng(5))
    at = lambda x: str(tmp_path / x)  # noqa: E731
    for s in ("S", "stale", "magic", "loci", "short", "bare"):
        assert run(["--pack", s] + names[:4], tmp_path).returncode == 0
    assert run(["--pack", "T"] + names[4:6], tmp_path).returncode == 0
    norm, rot = loaded_pca(tmp_path, 40, 2)
    good = index_bytes(at("S"), 4, 2, 1, norm, rot)
    open(at("S.pcaidx"), "wb").write(good)
    open(at("T.pcaidx"), "wb").write(index_bytes(at("T"), 2, 2, 1, norm, rot))
    open(at("stale.pcaidx"), "wb").write(index_bytes(at("stale"), 3, 2, 1, norm, rot))
    open(at("magic.pcaidx"), "wb").write(b"NTSMPCX2" + good[8:])
    open(at("loci.pcaidx"), "wb").write(index_bytes(at("loci"), 4, 2, 1, norm, rot, crc=locus_crc(at("loci")) ^ 1))
    open(at("short.pcaidx"), "wb").write(good[:-1])
    line = "rs%d\t3\t4\t3\t4\t1\t1\n"
    with open(at("alien.txt"), "w") as f:
        f.write("#@TK\t5\n#@KS\t19\n" + "".join(line % s for s in range(40)) + "rsUnknown\t3\t4\t3\t4\t1\t1\n")
    with open(at("dup.txt"), "w") as f:
        f.write("#@TK\t5\n#@KS\t19\n" + "".join(line % s for s in range(40)) + line % 17)
    assert run(["--pack", "alien", "alien.txt"], tmp_path).returncode == 0
    assert run(["--pack", "dup", "dup.txt"], tmp_path).returncode == 0
    store = open(at("S"), "rb").read()
    with open(at("empty"), "wb") as f:
        f.write(store[:16] + struct.pack("<Q", 0) + store[24:read_store(at("S"))["first"]])
    with open(at("trunc"), "wb") as f:
        f.write(store[:-1])
    P = ["-p", "rot.tsv", "-n", "norm.txt", "-d", "2"]
    q = names[6]
    N = ["--between-near", "S"]
    eight, build = b"--between and --between-near are eight runs: give one of them", b"is not part of this build"
    index = b"takes rotation and centre from the store's index: give no -p and no -n"
    cases = [
        (N + ["T", q], b"--between-near takes STORE_B and no input files"),             # FILES beyond STORE_B
        (N + ["T", q, names[5]], b"--between-near takes STORE_B and no input files"),
        (N, b"--between-near needs the second store"),                                  # STORE_B missing
        (N + ["T", "-p", "rot.tsv"], b"--between-near " + index),                       # -p / -n: the sentence of --within-near
        (N + ["T", "-n", "norm.txt"], b"--between-near " + index),
        (N + ["T"] + P, b"--between-near " + index),
        (N + ["T", "-b", "truth.tsv"], b"-b with --between-near " + build),
        (N + ["T", "-e", "merged.txt"], b"merging (-e, -o) with --between-near " + build),
        (N + ["T", "-o"], b"merging (-e, -o) with --between-near " + build),
        (["--between-near", "trunc", "T"], b"trunc"),                                   # either store invalid ...
        (N + ["trunc"], b"trunc"),
        (["--between-near", "nowhere", "T"], b"cannot open store nowhere"),
        (N + ["nowhere"], b"cannot open store nowhere"),
        (["--between-near", "empty", "T"], b"empty holds no samples"),                  # ... or empty
        (N + ["empty"], b"empty holds no samples"),
        (N + ["alien"], b"locus rsUnknown of alien is not in S"),                       # map_loci's two sentences
        (N + ["dup"], b"locus rs17 stands twice in dup"),
        (["--between-near", "dup", "T"], b"locus rs17 stands twice in dup"),
        (["--between-near", "bare", "T"], b"--index bare"),                             # A's index absent ...
        (["--between-near", "magic", "T"], b"--index magic"),                           # ... invalid: magic, other loci, size ...
        (["--between-near", "loci", "T"], b"--index loci"),
        (["--between-near", "short", "T"], b"--index short"),
        (["--between-near", "stale", "T"], b"--index stale"),                           # ... stale
        (N + ["T", "-c", "2"], b"-c 2, but S.pcaidx was written with -c 1"),            # a differing -c / -d
        (N + ["T", "-d", "3"], b"-d 3, but S.pcaidx was written with -d 2"),
        (N + ["T", "--between-rows", "3"], b"--between-rows sets the bands of --between"),
        (N + ["T", "--within-rows", "3"], b"--within-rows sets the bands of --within"),
        (N + ["--pack", "S", "T"], eight),                                              # together with any of the seven store runs
        (N + ["--against", "S", "T"], eight),
        (N + ["--index", "S", "T"] + P, eight),
        (N + ["--near", "S", "T"], eight),
        (N + ["--within", "S", "T"], eight),
        (N + ["--within-near", "S", "T"], eight),
        (N + ["--between", "S", "T"], eight),
        (["--between", "S", "--within", "S", "T"], b"are seven runs: give one of them"),  # the sentences the other runs always had
        (["--between", "S", "T"] + P, b"a PCA-guided search between two stores is not part of this build"),
        (["--between", "S", "T", "-p", "rot.tsv"], b"--between-near"),                  # ... which now goes on to name the run
    ]
    files = ["S", "T", "stale", "magic", "loci", "short", "bare", "alien", "dup", "empty", "trunc"] + [s + ".pcaidx" for s in ("S", "T", "stale", "magic", "loci", "short")]
    for args, sentence in cases:
        before = {s: snapshot(at(s)) for s in files}
        p = run(args, tmp_path)
        assert p.returncode == 1 and p.stdout == b"", (args, p.returncode, p.stdout[:100], p.stderr[-300:])
        errors = [x for x in p.stderr.split(b"\n") if x.startswith(b"Error: ")]
        assert len(errors) == 1 and sentence in errors[0], (args, p.stderr)
        assert all(unchanged(at(s), before[s]) for s in files), args
        assert not any(os.path.exists(at(x)) for x in ("merged.txt", "bare.pcaidx", "S.tmp", "T.tmp", "S.pcaidx.tmp", "T.pcaidx.tmp")), args
    p = run(["--index", "S", "--near", "S"] + P, tmp_path)
    assert p.returncode == 1 and b"are four runs" in p.stderr
    p = run(["--between-near", "stale", "T"], tmp_path)
    assert b"is stale" in p.stderr                                                      # the refusal still says what is wrong with the index


def test_host_decisions_under_the_host_sanitizers():
    """`make between_near_check`: tools/eval_between_near_check.cpp -- b_index_usable on every reason for "no", the grouping of
    dense rows into runs against a linear scan, and the pass cut over random two-store lists -- built with
    -fsanitize=address,undefined as a program of its own, run once by the target and once here for its lines."""
    subprocess.run(["make", "-s", "between_near_check"], cwd=ROOT, check=True, stdout=subprocess.DEVNULL)
    p = subprocess.run([os.path.join(ROOT, "build", "eval_between_near_check")], capture_output=True)
    assert p.returncode == 0 and p.stdout.endswith(b"ok\n") and b"FAILED" not in p.stdout and p.stderr == b"", (p.stdout[-600:], p.stderr[-600:])
    for part in (b"B's index: ", b"dense runs: ", b"pass cut: "):
        assert part in p.stdout


def test_empty_sides_need_no_device():
    """Zeroed outputs and no pairs where a side is empty, on a machine without a GPU"""
    import ntsm_amd.eval as ev
    norm, rot = synthetic_pca(np.random.default_rng(1), 5, 2)
    some = np.arange(5, dtype=np.uint32)[::-1].copy()
    cloud, geno, times = ev.project_store_mapped(np.zeros((0, 5, 2), dtype=np.uint32), 5, some, norm, rot)           # no sample of B
    assert cloud.shape == (0, 2) and geno.shape == (0, 3) and times.chunks == 0
    cloud, geno, times = ev.project_store_mapped(np.ones((3, 4, 2), dtype=np.uint32), 0, np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.longdouble),
                                                 np.zeros((2, 0), dtype=np.longdouble))                             # no site of A, four of B
    assert cloud.tobytes() == bytes(3 * 2 * 8) and not geno.any() and times.chunks == 0
    cloud, geno, times = ev.project_store_mapped(np.zeros((0, 5, 2), dtype=np.uint32), 5, None, norm, rot)           # ... and through the unmapped walk
    assert cloud.shape == (0, 2) and times.chunks == 0
    pts, radius = search_case(3, 4, 2)
    for n_a in (0, 7):                                                                  # no sample of A, none of B
        pi, pk, dist, _ = ev.between_candidates(pts[:n_a], radius[:n_a], pts[n_a:], radius[n_a:])
        assert len(pi) == len(pk) == len(dist) == 0
    ones = np.ones((3, 5, 2), dtype=np.uint32)
    out, times = ev.between_score_pairs(ones, ones, [], [])                             # an empty list
    assert len(out) == 0 and times.chunks == 0
    none = np.zeros((2, 0, 2), dtype=np.uint32)
    out, times = ev.between_score_pairs(none, none, [0, 3], [2, 1])                     # no site
    assert out.tobytes() == bytes(2 * 64) and times.chunks == 0
    out, times = ev.between_score_pairs(none, ones, [0], [4], site_map=np.zeros(0, dtype=np.uint32))
    assert out.tobytes() == bytes(64) and times.chunks == 0


def test_bad_arguments_need_no_device():
    """-1, before any HIP call, for each bad argument of the three entry points"""
    import ntsm_amd.eval as ev
    L = ev.lib
    a, b = np.ones((4, 5, 2), dtype=np.uint32), np.ones((3, 3, 2), dtype=np.uint32)
    good = np.array([0, LACKS, 1, LACKS, 2], dtype=np.uint32)
    norm, rot = synthetic_pca(np.random.default_rng(2), 5, 2)
    cloud, geno = np.zeros((3, 2)), np.zeros((3, 3), dtype=np.uint32)
    ld = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_longdouble))  # noqa: E731

    def projected(b_ptr=b.ctypes.data, stride=24, n_sites_b=3, site_map=good, norm_=ld(norm), rot_=ld(rot), cloud_=cloud.ctypes.data):
        return L.ntsm_eval_project_store_mapped(0, b_ptr, stride, 3, 5, n_sites_b, None if site_map is None else site_map.ctypes.data, 1, norm_, rot_, 2, 0,
                                                cloud_, geno.ctypes.data, None)
    for bad in (dict(b_ptr=None), dict(stride=20), dict(stride=26), dict(site_map=np.array([0, 3, 1, LACKS, 2], dtype=np.uint32)),
                dict(site_map=np.array([0, LACKS, 1, 0, 2], dtype=np.uint32)), dict(site_map=None), dict(site_map=None, n_sites_b=4, stride=32),
                dict(norm_=None), dict(rot_=None), dict(cloud_=None)):
        assert projected(**bad) == -1, bad

    pts, radius = search_case(2, 3, 2)
    ca, cb, ra, rb = pts[:2].copy(), pts[2:].copy(), radius[:2].copy(), radius[2:].copy()
    n = ctypes.c_uint64(77)
    pi = np.zeros(8, dtype=np.uint32)

    def searched(a_cloud=ca.ctypes.data, a_radius=ra.ctypes.data, b_cloud=cb.ctypes.data, b_radius=rb.ctypes.data, out=(None, None, None), cap=0, count=ctypes.byref(n)):
        return L.ntsm_eval_between_candidates(0, a_cloud, a_radius, 2, b_cloud, b_radius, 3, 2, out[0], out[1], out[2], cap, count, None)
    for bad in (dict(count=None), dict(a_cloud=None), dict(a_radius=None), dict(b_cloud=None), dict(b_radius=None), dict(cap=8),
                dict(cap=8, out=(pi.ctypes.data, pi.ctypes.data, None))):
        assert searched(**bad) == -1, bad

    out = np.zeros(4, dtype=ev.RECORD)

    def scored(pi_, pk_, a_ptr=a.ctypes.data, a_stride=40, b_ptr=b.ctypes.data, b_stride=24, site_map=good, n_sites_b=3, chunk=0, out_=out.ctypes.data):
        pi_, pk_ = np.array(pi_, dtype=np.uint32), np.array(pk_, dtype=np.uint32)
        return L.ntsm_eval_between_score_pairs(0, a_ptr, a_stride, 4, b_ptr, b_stride, 3, 5, n_sites_b, None if site_map is None else site_map.ctypes.data, 1,
                                               pi_.ctypes.data, pk_.ctypes.data, len(pi_), chunk, out_, None)
    for pi_, pk_ in (([0], [7]), ([7], [0]), ([0], [1]), ([4], [5]), ([2], [2]), ([5], [5]), ([0, 1], [4, 3])):     # out of range; two of A; two of B
        assert scored(pi_, pk_) == -1, (pi_, pk_)
    for bad in (dict(chunk=1), dict(a_ptr=None), dict(b_ptr=None), dict(a_stride=36), dict(a_stride=42), dict(b_stride=20), dict(b_stride=26), dict(out_=None),
                dict(site_map=np.array([0, 3, 1, LACKS, 2], dtype=np.uint32)), dict(site_map=np.array([0, LACKS, 1, 0, 2], dtype=np.uint32)),
                dict(site_map=None), dict(site_map=None, n_sites_b=4, b_stride=32)):
        assert scored([0], [4], **bad) == -1, bad
    assert L.ntsm_eval_between_score_pairs(0, a.ctypes.data, 40, 4, b.ctypes.data, 24, 3, 5, 3, good.ctypes.data, 1, None, None, 2, 0, out.ctypes.data, None) == -1
    with pytest.raises(RuntimeError, match="failed: -1"):
        ev.between_score_pairs(a, b, [0], [1], site_map=good)
    assert not out.view(np.uint8).any() and not cloud.any() and not geno.any()


# ---------------------------------------------------------------------------------------------------- GPU: the projection
def lacking_sites(m, count, seed=8):
    """`count` sites of A that B lacks, site 0 and the last among them"""
    if count == 0:
        return np.zeros(0, dtype=np.int64)
    return np.concatenate([[0, m - 1], np.random.default_rng(seed).choice(np.arange(1, m - 1), size=count - 2, replace=False)])


def check_projection(b, m, site_map, dim, c, chunk, rng):
    """cloud and tallies as raw bytes against ntsm_eval_project and ntsm_eval_cross on B remapped by numpy"""
    import ntsm_amd.eval as ev
    dense = remapped(b, site_map)
    norm, rot = synthetic_pca(rng, m, dim)
    want = ev.project(dense, norm, rot, min_cov=c)[0]
    want_geno = ev.cross(dense[:1], dense, min_cov=c)[1]
    cloud, geno, times = ev.project_store_mapped(ev.Records.of(b, HEAD), m, site_map, norm, rot, min_cov=c, b_chunk=chunk)
    assert cloud.shape == (len(b), dim) and cloud.tobytes() == want.tobytes(), (b.shape, dim, chunk)
    assert np.array_equal(geno, want_geno) and geno[:, 2].min() >= int((site_map == LACKS).sum())
    assert times.chunks == (-(-len(b) // chunk) if chunk else 1)
    return cloud, norm, rot


# (n_b, sites of A, sites B lacks, dim, min_cov, b_chunk): one lane; a wave less one in two ragged chunks; a full wave; one past
# it in two chunks; 257 in three ragged chunks; 1,025 (five workgroups of the projection, the last with one live lane) in four
PROJECT = [(1, 300, 17, 4, 1, 0), (63, 300, 17, 1, 0, 40), (64, 300, 17, 4, 1, 0), (65, 300, 17, 5, 1, 64), (257, 300, 17, 4, 3, 100),
           (1025, 40, 5, 5, 1, 300)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", PROJECT, ids=["b%d_m%d_lack%d_d%d_c%d_chunk%d" % s for s in PROJECT])
def test_project_store_mapped_equals_session_projection_bits(shape):
    """ntsm_eval_project_store_mapped on a B laid out at a store's stride whose sites are a random permutation of A's with some
    removed, site 0 and the last among them (more than 256 sites of A: two workgroups of the remap along the sites, the second
    ragged), one sample with counts beyond 2^31: the cloud against ntsm_eval_project and the tallies against ntsm_eval_cross on
    the remapped dense copy, raw bytes; the chunk count."""
    n_b, m, lack, dim, c, chunk = shape
    _, b, site_map = mapped_case(1, n_b, m, lacking_sites(m, lack), list(shape))
    assert (site_map == LACKS).sum() == lack and site_map[0] == LACKS and site_map[-1] == LACKS and b.shape == (n_b, m - lack, 2)
    assert (np.diff(site_map[site_map != LACKS].astype(np.int64)) < 0).any()            # not monotone: a real permutation
    if n_b > 2:
        assert b[2].min() >= 2**31
    cloud = check_projection(b, m, site_map, dim, c, chunk, np.random.default_rng(shape[0]))[0]
    if n_b > 2:
        assert np.abs(cloud).max() > 0                                                  # a cloud never written cannot pass


@pytest.mark.gpu
def test_project_store_mapped_one_site_and_the_identity():
    """A B of exactly one site, A's site 4 of 40.  Then the identity given as a map: the bytes of site_map = NULL and of
    ntsm_eval_project_store, chunked and not."""
    import ntsm_amd.eval as ev
    rng = np.random.default_rng(19)
    _, b1, map1 = mapped_case(1, 66, 40, np.setdiff1d(np.arange(40), [4]), 18)
    assert b1.shape[1] == 1 and map1[4] == 0 and (map1 == LACKS).sum() == 39
    for chunk in (0, 16):
        check_projection(b1, 40, map1, 4, 0, chunk, rng)
    m = 300
    b = random_samples(rng, 70, m, depth=8.0)
    b[2] = rng.integers(2**31, 2**32, size=(m, 2)).astype(np.uint32)
    identity = np.arange(m, dtype=np.uint32)
    out = []
    for chunk in (0, 16):
        cloud, norm, rot = check_projection(b, m, identity, 5, 1, chunk, np.random.default_rng(20))
        for given in (identity, None):
            got = ev.project_store_mapped(ev.Records.of(b, HEAD), m, given, norm, rot, min_cov=1, b_chunk=chunk)
            out.append(got[0].tobytes() + got[1].tobytes())
        got = ev.project_store(ev.Records.of(b, HEAD), norm, rot, min_cov=1, db_chunk=chunk)
        out.append(got[0].tobytes() + got[1].tobytes())
    assert len(set(out)) == 1 and out[0][:cloud.nbytes] == cloud.tobytes()


# ---------------------------------------------------------------------------------------------------- GPU: the search
def check_between_candidates(cloud, radius, n_a):
    """between_candidates against candidates on the concatenation, filtered to one index on each side: bytes"""
    import ntsm_amd.eval as ev
    pi, pk, dist = session_candidates(cloud, radius)
    keep = (pi < n_a) != (pk < n_a)
    gi, gk, gd, _ = ev.between_candidates(cloud[:n_a], radius[:n_a], cloud[n_a:], radius[n_a:])
    assert (gi.tobytes(), gk.tobytes(), gd.tobytes()) == (pi[keep].tobytes(), pk[keep].tobytes(), dist[keep].tobytes())
    return gi, gk, gd


# dim 1 / 3 / 4 / 5: evalMetric unrolls by four
SEARCH = [(1, 1, 1), (3, 63, 3), (5, 64, 4), (4, 65, 5), (9, 257, 4), (1030, 3, 3), (6, 1030, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_a,n_b,dim", SEARCH, ids=["a%d_b%d_d%d" % s for s in SEARCH])
def test_between_candidates_equal_the_session_search_filtered(n_a, n_b, dim):
    """pi, pk and dist as bytes against ntsm_eval_candidates on the concatenation, filtered to the pairs with one sample of each
    store; radii of all three classes on both sides.  Beyond one sample a side, both kinds of owner must occur: a pair in the
    row of a sample of A and a pair in the row of a sample of B."""
    cloud, radius = search_case(n_a, n_b, dim)
    gi, gk, _ = check_between_candidates(cloud, radius, n_a)
    assert ((gi < n_a) != (gk < n_a)).all()
    if n_a > 1:
        assert {DBL_MAX} < set(radius[:n_a]) and {DBL_MAX} < set(radius[n_a:]) and len(set(radius)) == 3
        assert (gi < n_a).any() and (gi >= n_a).any(), (n_a, n_b, dim)
        assert len(gi) < n_a * n_b                                                      # and the radii do cut


@pytest.mark.gpu
def test_between_candidates_edge_cases():
    """All radii DBL_MAX (the whole rectangle, in A's rows); all equal and finite (every pair in the lower index's row, a
    sample of A); a radius that takes nothing; a point of B equal to one of A and three of B equal to each other (metric ties
    in one row come out by ascending k); capacity 0 returns the count and writes nothing, the reported size then holds the
    list."""
    import ntsm_amd.eval as ev
    n_a, n_b, dim = 5, 70, 4
    cloud, radius = search_case(n_a, n_b, dim, seed=1)
    n = n_a + n_b
    gi, gk, _ = check_between_candidates(cloud, np.full(n, DBL_MAX), n_a)
    assert len(gi) == n_a * n_b and (gi < n_a).all() and (gk >= n_a).all()
    gi, gk, _ = check_between_candidates(cloud, np.full(n, float(np.max(radius[radius < DBL_MAX]))), n_a)
    assert len(gi) > 0 and (gi < n_a).all()                                             # equal radii: the lower index owns
    assert len(check_between_candidates(cloud, np.full(n, 1e-300), n_a)[0]) == 0
    mixed = radius.copy()
    mixed[1] = mixed[n_a + 2] = 1e-300                                                  # one sample of each store whose radius takes nothing
    check_between_candidates(cloud, mixed, n_a)
    ties = cloud.copy()
    ties[n_a + 5] = ties[0]                                                             # a point of B equal to sample 0 of A
    ties[n_a + 9] = ties[n_a + 21] = ties[n_a + 20]                                     # three of B equal to each other
    ties[3] = ties[4]                                                                   # two of A equal to each other
    r = radius.copy()
    assert max(r[3], r[4], r[n_a + 5], r[n_a + 9], r[n_a + 20], r[n_a + 21]) < DBL_MAX  # none of the tied points owns its rows
    r[0] = r[n_a + 11] = 1e6                                                            # rows of both stores that see the ties
    gi, gk, gd = check_between_candidates(ties, r, n_a)
    row0 = gk[gi == 0]
    assert n_a + 5 in row0 and gd[(gi == 0) & (gk == n_a + 5)][0] == 0.0
    pos = [int(np.where(row0 == n_a + d)[0][0]) for d in (9, 20, 21)]
    assert pos == sorted(pos) and pos[2] - pos[0] == 2                                  # the three tied points stand together, by k
    rowb = list(gk[gi == n_a + 11])
    assert 3 in rowb and rowb.index(4) == rowb.index(3) + 1
    with pytest.raises(ValueError) as e:
        ev.between_candidates(cloud[:n_a], radius[:n_a], cloud[n_a:], radius[n_a:], capacity=0)
    pi, pk, _ = session_candidates(cloud, radius)
    size = int(((pi < n_a) != (pk < n_a)).sum())
    assert e.value.args[1] == size > 0
    assert len(ev.between_candidates(cloud[:n_a], radius[:n_a], cloud[n_a:], radius[n_a:], capacity=size)[0]) == size
    with pytest.raises(ValueError):
        ev.between_candidates(cloud[:n_a], radius[:n_a], cloud[n_a:], radius[n_a:], capacity=size - 1)


# ---------------------------------------------------------------------------------------------------- GPU: listed pairs
def check_between_pairs(a, b, site_map, pi, pk, c, chunk, passes=None):
    """records as raw bytes against ntsm_eval_score_pairs on [A; B remapped]; the pass count against the greedy cut"""
    import ntsm_amd.eval as ev
    pi, pk = np.asarray(pi, dtype=np.uint32), np.asarray(pk, dtype=np.uint32)
    dense = b if site_map is None else remapped(b, site_map)
    want = ev.score_pairs(np.concatenate([a, dense]), pi, pk, min_cov=c)[0]
    got, times = ev.between_score_pairs(ev.Records.of(a, HEAD), ev.Records.of(b, HEAD), pi, pk, site_map=site_map, min_cov=c, chunk=chunk)
    assert got.tobytes() == want.tobytes(), (a.shape, b.shape, chunk)
    assert times.chunks == (greedy_passes(pi, pk, chunk) if passes is None else passes), chunk
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("mapped", [False, True], ids=["unmapped", "mapped"])
@pytest.mark.parametrize("m", [1, 7, 300])
def test_between_score_pairs_equal_session_records(m, mapped):
    """6 samples of A, 65 of B (one without coverage, one a sample of A seen through B's table, one with counts beyond 2^31), 16
    pairs in both orientations, sample 2 of A named by five of them and sample 17 of B by six: records as raw bytes against
    ntsm_eval_score_pairs on the dense concatenation with chunk 2 (a pass per pair), 3 (greedy passes of up to three samples)
    and 0 (one pass).  Mapped: B's sites a permutation of A's, lacking site 0 and the last of 7 and 17 of 300."""
    n_a, n_b, c = 6, 65, 1
    lack = {1: 0, 7: 2, 300: 17}[m] if mapped else 0
    a, b, site_map = mapped_case(n_a, n_b, m, lacking_sites(m, lack), [12, m, mapped])
    if mapped:
        assert len(site_map) == m and (site_map == LACKS).sum() == lack
    else:
        b, site_map = remapped(b, site_map), None                                       # B over A's own table
    b[0] = 0
    B = lambda x: n_a + x  # noqa: E731
    pairs = [(2, B(17)), (B(17), 0), (2, B(1)), (B(2), 2), (B(17), 5), (1, B(17)), (B(0), 2), (3, B(64)), (2, B(33)), (B(64), 3), (B(17), 4), (4, B(40)),
             (B(40), 5), (0, B(1)), (3, B(17)), (B(63), 1)]
    pi, pk = [p[0] for p in pairs], [p[1] for p in pairs]
    assert all(set(x) != set(y) for x, y in zip(pairs, pairs[1:])) and greedy_passes(pi, pk, 2) == len(pairs)
    for chunk, passes in ((2, len(pairs)), (3, None), (0, 1)):
        got = check_between_pairs(a, b, site_map, pi, pk, c, chunk, passes)
    assert 1 < greedy_passes(pi, pk, 3) < len(pairs)
    if m > 1:
        assert got["n_valid"].max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("mapped", [False, True], ids=["unmapped", "mapped"])
def test_between_score_pairs_many_samples_in_passes(mapped):
    """9 samples of A against 1,030 of B over 24 sites at chunk 64: every sample of B named, first as the whole row of a hub
    sample of A in store order (neighbouring samples of B: 2-D copies of many rows), then in a shuffled order and alternating
    orientation; then the row of a hub sample of B over all of A; dozens of passes whose records go back to list order; then
    the same list in one pass."""
    rng = np.random.default_rng(79)
    n_a, n_b, m = 9, 1030, 24
    a, b, site_map = mapped_case(n_a, n_b, m, lacking_sites(m, 4 if mapped else 0), 80)
    if not mapped:
        b, site_map = remapped(b, site_map), None
    order = rng.permutation(n_b)
    pi = [4] * n_b + [int(d) % n_a if x % 2 else n_a + int(d) for x, d in enumerate(order)] + [n_a + 500] * n_a
    pk = [n_a + d for d in range(n_b)] + [n_a + int(d) if x % 2 else int(d) % n_a for x, d in enumerate(order)] + list(range(n_a))
    assert greedy_passes(pi, pk, 64) > 20
    got = check_between_pairs(a, b, site_map, pi, pk, 1, 64)
    assert got["n_valid"].min() > 0                                                     # a record never written cannot pass
    assert check_between_pairs(a, b, site_map, pi, pk, 1, 0, 1).tobytes() == got.tobytes()


# ---------------------------------------------------------------------------------------------------- GPU: the CLI
def between(text, files_a, files_b):
    """header + the rows of a -p run over [A's files, B's files] that pair a file of one store with a file of the other, in
    order; and how many of them stand in the row of a file of B"""
    lines = text.split(b"\n")
    assert lines[-1] == b""
    sa, sb = set(f.encode() for f in files_a), set(f.encode() for f in files_b)
    assert not sa & sb
    keep, owned_by_b = [], 0
    for r in lines[1:-1]:
        one, two = r.split(b"\t", 2)[:2]
        if (one in sa and two in sb) or (one in sb and two in sa):
            keep.append(r)
            owned_by_b += one in sb
    return b"".join(x + b"\n" for x in [lines[0]] + keep), owned_by_b


def pack_only(d, store, files):
    for f in (store, store + ".pcaidx"):
        if os.path.exists(os.path.join(str(d), f)):
            os.unlink(os.path.join(str(d), f))
    assert run(["--pack", store] + files, d).returncode == 0


def between_near(args, store_a, store_b, d, extra=()):
    """(stdout, stderr) of --between-near with the flags of a -p run that the index does not fix"""
    p = run(list(extra) + ["-v", "-v"] + without_pca(args) + ["--between-near", store_a, store_b], d)
    assert p.returncode == 0, (args, p.stderr[-400:])
    return p.stdout, p.stderr.split(b"store between-near: ")[1]


@pytest.mark.gpu
@pytest.mark.parametrize("spec", TIE_FREE, ids=lambda s: "n%d_m%d_d%d" % (s[1], s[2], s[4]))
def test_cli_between_near_equals_the_pca_run_filtered(gpu, built, cohorts, restatement, spec):
    """The tie-free cohorts split in two (the first third is A), -a, radii at the 15th and 60th percentile: stdout byte for byte,
    at -t 1 and -t 4, against the rows of `ntsmEval -p -n` over all files that pair the two stores, against the restatement
    and, where it is built, the reference class.  B once without an index (projected in the run) and once with its own (from
    index): the same bytes.  Both kinds of owner occur.  Neither store nor index is touched."""
    d, names, s, args = tie_free_args(restatement, cohorts, spec)
    k = len(names) // 3
    fa, fb = names[:k], names[k:]
    make_store(d, "bnA.store", fa, args)
    pack_only(d, "bnB.store", fb)
    want, owned_by_b = between(stdout_of(EVAL, ["-t", "1"] + args, names, d), fa, fb)
    rows = want.count(b"\n") - 1
    assert owned_by_b >= 1 and rows > owned_by_b and rows < len(fa) * len(fb)
    assert between(pca_expected(restatement, d, names, args)[0], fa, fb)[0] == want
    if os.path.isfile(REF_EVAL):
        assert between(reference(args, names, d), fa, fb)[0] == want
    at = lambda x: os.path.join(str(d), x)  # noqa: E731
    before = [snapshot(at(x)) for x in ("bnA.store", "bnA.store.pcaidx", "bnB.store")]
    for t in ("1", "4"):
        out, report = between_near(args, "bnA.store", "bnB.store", d, ["-t", t])
        assert out == want, t
        assert b"loci identical (0 of %d absent from bnB.store), B's projections projected, %d candidates (" % (spec[2], rows) in report, report
    for part in (b" listed pairs", b" dense rows of A", b"map ", b"project ", b"search ", b"score ", b"print "):
        assert part in report, part
    assert all(unchanged(at(x), b) for x, b in zip(("bnA.store", "bnA.store.pcaidx", "bnB.store"), before)) and not os.path.exists(at("bnB.store.pcaidx"))
    make_store(d, "bnB.store", fb, args)                                                # B with an index of the same matrices
    before = snapshot(at("bnB.store.pcaidx"))
    out, report = between_near(args, "bnA.store", "bnB.store", d)
    assert out == want and b"B's projections from index" in report and unchanged(at("bnB.store.pcaidx"), before)
    if spec[4] > 2:                                                                     # ... and one written with another -d: projected again
        other = [x for x in args]
        other[other.index("-d") + 1] = str(spec[4] - 1)
        make_store(d, "bnB.store", fb, other)
        out, report = between_near(args, "bnA.store", "bnB.store", d)
        assert out == want and b"B's projections projected" in report


@pytest.mark.gpu
def test_cli_between_near_duplicate_cohort(gpu, built, cohorts, restatement):
    """The planted-duplicate cohort (40 x 3,000; sample 39 a copy of sample 0, sample 3 empty) split in the middle, so that the
    replicates stand on opposite sides, under the five flag sets of DUPLICATE_CASES (A's index is rebuilt where -d or -c
    change); B alternately indexed and not.  Byte for byte against this build's -p run filtered -- exact ties come out by k on
    both sides -- and the same rows up to the order among ties against the reference.  The default threshold prints the
    replicate pair."""
    d, names, cases = duplicate_cases(restatement, cohorts)
    fa, fb = names[:20], names[20:]
    for x, args in enumerate(cases):
        make_store(d, "dupA.store", fa, args)
        (make_store(d, "dupB.store", fb, args) if x % 2 else pack_only(d, "dupB.store", fb))
        want = between(stdout_of(EVAL, ["-t", "1"] + args, names, d), fa, fb)[0]
        assert want.count(b"\n") >= 2, args
        assert any(r.split(b"\t")[:2] == [names[0].encode(), names[39].encode()] for r in want.split(b"\n")), args
        got, report = between_near(args, "dupA.store", "dupB.store", d)
        assert got == want, args
        assert (b"from index" if x % 2 else b"projected") in report
        if os.path.isfile(REF_EVAL):
            assert same_up_to_tie_order(got, between(reference(args, names, d), fa, fb)[0]), args


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["search_all_in_A", "search_all_in_B"])
def test_cli_between_near_big_cohort(gpu, built, cohorts, restatement, side):
    """1,030 x 64 sites, dim 3, by length, line count and SHA-256.  The empty sample 3 searches all: with the first ten files as
    A its row of 1,020 pairs is a dense row through --between's session; with the first ten files as B, and so after the
    other 1,020 in the run, its pairs with every sample of A go through the list as (b, a)."""
    d, names, s, args = tie_free_args(restatement, cohorts, BIG_PCA)
    fa, fb = (names[:10], names[10:]) if side == "search_all_in_A" else (names[10:], names[:10])
    make_store(d, side + "A.store", fa, args)
    pack_only(d, side + "B.store", fb)
    text = stdout_of(EVAL, ["-t", "1"] + args, fa + fb, d)
    want, owned_by_b = between(text, fa, fb)
    own = [r for r in want.split(b"\n")[1:-1] if r.split(b"\t", 1)[0] == names[3].encode()]
    assert len(own) == (len(fb) if side == "search_all_in_A" else len(fa))              # the search-all row: the whole other store, under -a
    got, report = between_near(args, side + "A.store", side + "B.store", d)
    assert sig(got) == sig(want), report
    if side == "search_all_in_A":
        assert b" 1 dense rows of A in 1 runs" in report and b"(0 listed" not in report
    else:
        assert b" 0 dense rows of A in 0 runs" in report and owned_by_b >= len(fa)
    if os.path.isfile(REF_EVAL):
        assert sig(between(reference(args, fa + fb, d), fa, fb)[0]) == sig(want)


@pytest.mark.gpu
def test_cli_between_near_mapped_store(gpu, built, cohorts, restatement):
    """B packed from files written in another locus order and lacking 23 of A's 1,500 loci, the first and the last among them:
    stdout byte for byte against the -p run over [A's files, those files] filtered, and against the reference where built; -vv
    says "mapped", how many loci B lacks, and "projected".  An index of B's own -- over its own table, so with other matrices
    -- changes nothing: still "projected", the same bytes, the index untouched.  B as the first store is refused: it lacks
    loci of A."""
    d, names, s, args = tie_free_args(restatement, cohorts, TIE_FREE[0])
    m, k = s.shape[1], 25
    rng = np.random.default_rng(77)
    lacking = np.concatenate([[0, m - 1], rng.choice(np.arange(1, m - 1), size=21, replace=False)])
    order = rng.permutation(np.setdiff1d(np.arange(m), lacking))
    fa, fb = names[:k], []
    for j in range(k, len(names)):
        fb.append("m%03d.txt" % j)
        write_counts(os.path.join(str(d), fb[-1]), s[j][order], loci=["rs%d" % x for x in order])
    make_store(d, "mapA.store", fa, args)
    pack_only(d, "mapB.store", fb)
    assert read_store(os.path.join(str(d), "mapB.store"))["loci"] == ["rs%d" % x for x in order]
    want, owned_by_b = between(stdout_of(EVAL, ["-t", "1"] + args, fa + fb, d), fa, fb)
    assert owned_by_b >= 1 and want.count(b"\n") - 1 > owned_by_b
    if os.path.isfile(REF_EVAL):
        assert between(reference(args, fa + fb, d), fa, fb)[0] == want
    got, report = between_near(args, "mapA.store", "mapB.store", d)
    assert got == want and b"loci mapped (23 of 1500 absent from mapB.store), B's projections projected" in report, report
    p = run(["--index", "mapB.store"] + index_args(args), d)                             # B's own index: the first 1,477 rows of the matrices
    assert p.returncode == 0, p.stderr[-300:]
    before = snapshot(os.path.join(str(d), "mapB.store.pcaidx"))
    got, report = between_near(args, "mapA.store", "mapB.store", d)
    assert got == want and b"loci mapped" in report and b"B's projections projected" in report
    assert unchanged(os.path.join(str(d), "mapB.store.pcaidx"), before)
    p = run(without_pca(args) + ["--between-near", "mapB.store", "mapA.store"], d)
    assert p.returncode == 1 and p.stdout == b"" and b"of mapA.store is not in mapB.store" in p.stderr


@pytest.mark.gpu
def test_cli_between_near_after_an_append(gpu, built, cohorts, restatement):
    """A of 9 samples, B of 8 with its index; 4 more are packed into B: its index is stale, so B is projected in the run, and the
    output is that of the 21-file run; after --index on B the same bytes come "from index".  An append to A makes A's index
    stale: refused, naming --index A."""
    d, names, s, args = tie_free_args(restatement, cohorts, TIE_FREE[2])
    fa, first, more = names[:9], names[9:17], names[17:21]
    make_store(d, "growA.store", fa, args)
    make_store(d, "growB.store", first, args)
    got, report = between_near(args, "growA.store", "growB.store", d)
    assert got == between(stdout_of(EVAL, ["-t", "1"] + args, fa + first, d), fa, first)[0] and b"from index" in report
    assert run(["--pack", "growB.store"] + more, d).returncode == 0
    want = between(stdout_of(EVAL, ["-t", "1"] + args, fa + first + more, d), fa, first + more)[0]
    before = snapshot(os.path.join(str(d), "growB.store.pcaidx"))
    got, report = between_near(args, "growA.store", "growB.store", d)
    assert got == want and b"B's projections projected" in report and unchanged(os.path.join(str(d), "growB.store.pcaidx"), before)
    p = run(["-v", "--index", "growB.store"] + index_args(args), d)
    assert p.returncode == 0 and b"Projected 4 samples" in p.stderr, p.stderr[-300:]
    got, report = between_near(args, "growA.store", "growB.store", d)
    assert got == want and b"B's projections from index" in report
    assert run(["--pack", "growA.store"] + names[21:23], d).returncode == 0
    p = run(without_pca(args) + ["--between-near", "growA.store", "growB.store"], d)
    assert p.returncode == 1 and p.stdout == b"" and b"is stale" in p.stderr and b"--index growA.store" in p.stderr
