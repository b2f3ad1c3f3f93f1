"""ctypes plumbing for include/ntsm_eval_hip.h (all-pairs scoring of ntsmEval on the GPU, its PCA-guided search, queries and
that search against a cohort store, the pairs inside a store, one store against another, the search between two, the QC
tables of a store, the contamination check over one, the trios in one and the site-pair LD over one); used by tests and tools.
Loaded on demand: `import ntsm_amd.eval`.  Fails loudly when libntsm_eval_hip.so has not been built."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_path = os.path.join(_HERE, "libntsm_eval_hip.so")
if not os.path.exists(_path):
    raise ImportError("%s is missing: run `make` (there is no CPU fallback)" % _path)
lib = C.CDLL(_path)

RECORD = np.dtype([("sum_joint", "<f8"), ("sum_single1", "<f8"), ("sum_single2", "<f8"), ("n_valid", "<u8"),
                   ("hets1", "<u4"), ("homs1", "<u4"), ("hets2", "<u4"), ("homs2", "<u4"),
                   ("shared_hets", "<u4"), ("shared_homs", "<u4"), ("ibs0", "<u4"), ("ibs2", "<u4")])
assert RECORD.itemsize == 64

lib.ntsm_eval_pairs.restype = C.c_int
lib.ntsm_eval_pairs.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_double)]


def pair_index(i, j, n):
    """Position of pair (i < j) in the output (include/ntsm_eval_hip.h: ntsm_eval_pair_index)."""
    return i * n - i * (i + 1) // 2 + (j - i - 1)


def pairs(counts, min_cov=1, device=0):
    """counts: uint32 array [n_samples][n_sites][2].  Returns (records for every i < j in row order, kernel ms)."""
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    n, m = counts.shape[0], counts.shape[1]
    out = np.zeros(n * (n - 1) // 2, dtype=RECORD)
    ms = C.c_double()
    rc = lib.ntsm_eval_pairs(device, counts.ctypes.data, n, m, min_cov, out.ctypes.data, C.byref(ms))
    if rc:
        raise RuntimeError("ntsm_eval_pairs failed: %d" % rc)
    return out, ms.value


# ---- PCA-guided pair search (the reference's -p / -n mode; include/ntsm_eval_hip.h: ntsm_eval_open ... ntsm_eval_score_pairs)
E_CAPACITY = -3
lib.ntsm_eval_open.restype = C.c_int
lib.ntsm_eval_open.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
lib.ntsm_eval_close.restype = None
lib.ntsm_eval_close.argtypes = [C.c_void_p]
lib.ntsm_eval_project.restype = C.c_int
lib.ntsm_eval_project.argtypes = [C.c_void_p, C.POINTER(C.c_longdouble), C.POINTER(C.c_longdouble), C.c_uint32, C.c_void_p,
                                  C.POINTER(C.c_double)]
lib.ntsm_eval_candidates.restype = C.c_int
lib.ntsm_eval_candidates.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
lib.ntsm_eval_score_pairs.restype = C.c_int
lib.ntsm_eval_score_pairs.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_double)]
assert np.dtype(np.longdouble).itemsize == C.sizeof(C.c_longdouble)


def _ld_ptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_longdouble))


class _Handle:
    """A library session: `h` is its handle, `close=` in the class statement the name of the library function that frees it
    (a subclass of a session class that gives none keeps its parent's).  A context manager; closing twice, or what was never
    opened, does nothing."""
    h = None

    def __init_subclass__(cls, close=None, **kwargs):
        super().__init_subclass__(**kwargs)
        if close:
            cls._close = close

    def close(self):
        if self.h:
            getattr(lib, self._close)(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


def _tune(name, *args):
    """The library's tuning call `name` with args; a value it does not take is a ValueError"""
    rc = getattr(lib, name)(*args)
    if rc:
        raise ValueError("%s(%s) failed: %d" % (name, ", ".join("%r" % (a,) for a in args), rc))


class Session(_Handle, close="ntsm_eval_close"):
    """One run's counts on the device (ntsm_eval_open): uint32 [n_samples][n_sites][2], uploaded once."""

    def __init__(self, counts, min_cov=1, device=0):
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        self.n, self.m = counts.shape[0], counts.shape[1]
        self.h = C.c_void_p()
        rc = lib.ntsm_eval_open(device, counts.ctypes.data, self.n, self.m, min_cov, C.byref(self.h))
        if rc:
            raise RuntimeError("ntsm_eval_open failed: %d" % rc)

    def project(self, norm, rot):
        """norm: long double [n_sites]; rot: long double [dim][n_sites] (np.longdouble, the x87 format).  Returns
        (cloud double [n_samples][dim], kernel ms)."""
        norm = np.ascontiguousarray(norm, dtype=np.longdouble)
        rot = np.ascontiguousarray(rot, dtype=np.longdouble).reshape(-1, self.m)
        dim = rot.shape[0]
        cloud = np.zeros((self.n, dim), dtype=np.float64)
        ms = C.c_double()
        rc = lib.ntsm_eval_project(self.h, _ld_ptr(norm), _ld_ptr(rot), dim, cloud.ctypes.data, C.byref(ms))
        if rc:
            raise RuntimeError("ntsm_eval_project failed: %d" % rc)
        return cloud, ms.value

    def candidates(self, cloud, radius, capacity=None):
        """cloud: double [n_samples][dim]; radius: double [n_samples] (squared, DBL_MAX = search all).  Returns
        (pi, pk, calcDistance, kernel ms) in the reference's one-thread print order.  capacity: buffer size to offer
        (default: ask for the size first); too small raises ValueError carrying the size needed."""
        cloud = np.ascontiguousarray(cloud, dtype=np.float64)
        radius = np.ascontiguousarray(radius, dtype=np.float64)
        dim = cloud.shape[1] if cloud.ndim == 2 else 0
        ms, n = C.c_double(), C.c_uint64()
        if capacity is None:
            rc = lib.ntsm_eval_candidates(self.h, cloud.ctypes.data, dim, radius.ctypes.data, None, None, None, 0, C.byref(n), C.byref(ms))
            if rc not in (0, E_CAPACITY):
                raise RuntimeError("ntsm_eval_candidates failed: %d" % rc)
            capacity = n.value
        pi, pk = np.zeros(capacity, dtype=np.uint32), np.zeros(capacity, dtype=np.uint32)
        dist = np.zeros(capacity, dtype=np.float64)
        rc = lib.ntsm_eval_candidates(self.h, cloud.ctypes.data, dim, radius.ctypes.data, pi.ctypes.data, pk.ctypes.data, dist.ctypes.data,
                                      capacity, C.byref(n), C.byref(ms))
        if rc == E_CAPACITY:
            raise ValueError("capacity %d < %d candidate pairs" % (capacity, n.value), n.value)
        if rc:
            raise RuntimeError("ntsm_eval_candidates failed: %d" % rc)
        k = n.value
        return pi[:k], pk[:k], dist[:k], ms.value

    def score_pairs(self, pi, pk):
        """Records (RECORD) for the listed pairs, sample pi as sample 1; (records, kernel ms)."""
        pi = np.ascontiguousarray(pi, dtype=np.uint32)
        pk = np.ascontiguousarray(pk, dtype=np.uint32)
        out = np.zeros(len(pi), dtype=RECORD)
        ms = C.c_double()
        rc = lib.ntsm_eval_score_pairs(self.h, pi.ctypes.data, pk.ctypes.data, len(pi), out.ctypes.data, C.byref(ms))
        if rc:
            raise RuntimeError("ntsm_eval_score_pairs failed: %d" % rc)
        return out, ms.value


def project(counts, norm, rot, min_cov=1, device=0):
    """m_cloud of the reference's projectPCs: (cloud [n_samples][dim], kernel ms)."""
    s = Session(counts, min_cov, device)
    try:
        return s.project(norm, rot)
    finally:
        s.close()


def candidates(counts, cloud, radius, min_cov=1, device=0):
    """computeScorePCA's pairs: (pi, pk, calcDistance, kernel ms)."""
    s = Session(counts, min_cov, device)
    try:
        return s.candidates(cloud, radius)
    finally:
        s.close()


def score_pairs(counts, pi, pk, min_cov=1, device=0):
    """Records of arbitrary pairs (pi as sample 1): (records, kernel ms)."""
    s = Session(counts, min_cov, device)
    try:
        return s.score_pairs(pi, pk)
    finally:
        s.close()


# ---- queries against a cohort (ntsmEval --against; include/ntsm_eval_hip.h: ntsm_eval_cross)
class CrossTimes(C.Structure):
    _fields_ = [("upload_ms", C.c_double), ("prepare_kernel_ms", C.c_double), ("cross_kernel_ms", C.c_double), ("download_ms", C.c_double),
                ("chunks", C.c_uint32)]


lib.ntsm_eval_cross.restype = C.c_int
lib.ntsm_eval_cross.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                C.c_void_p, C.c_void_p, C.POINTER(CrossTimes)]
lib.ntsm_eval_cross_tune.restype = C.c_int
lib.ntsm_eval_cross_tune.argtypes = [C.c_uint32, C.c_uint32]


def cross(q, db, min_cov=1, db_chunk=0, device=0):
    """q: uint32 [n_q][n_sites][2], db: uint32 [n_db][n_sites][2].  Returns (records [n_q, n_db], the record of (q, d) being
    that of pair (q, n_q + d) of pairs(concatenate([q, db])); geno [n_db, 3] = hets, homs, miss of each database sample;
    times, a CrossTimes).  db_chunk: database samples per pass, 0 = the library's choice."""
    q = np.ascontiguousarray(q, dtype=np.uint32)
    db = np.ascontiguousarray(db, dtype=np.uint32)
    n_q, n_db, m = q.shape[0], db.shape[0], q.shape[1]
    if q.ndim != 3 or db.ndim != 3 or db.shape[1] != m or q.shape[2] != 2 or db.shape[2] != 2:
        raise ValueError("cross: q and db are [samples][sites][2] over the same sites")
    out = np.zeros((n_q, n_db), dtype=RECORD)
    geno = np.zeros((n_db, 3), dtype=np.uint32)
    times = CrossTimes()
    rc = lib.ntsm_eval_cross(device, q.ctypes.data, n_q, db.ctypes.data, 8 * m, n_db, m, min_cov, db_chunk, out.ctypes.data,
                             geno.ctypes.data, C.byref(times))
    if rc:
        raise RuntimeError("ntsm_eval_cross failed: %d" % rc)
    return out, geno, times


# ---- the PCA-guided search against a cohort store (ntsmEval --index / --near; include/ntsm_eval_hip.h:
# ntsm_eval_project_store, ntsm_eval_cross_candidates, ntsm_eval_cross_score_pairs).  Indices follow the concatenation
# [queries; database]: database sample d is sample n_q + d.
lib.ntsm_eval_project_store.restype = C.c_int
lib.ntsm_eval_project_store.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_longdouble),
                                        C.POINTER(C.c_longdouble), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(CrossTimes)]
lib.ntsm_eval_cross_candidates.restype = C.c_int
lib.ntsm_eval_cross_candidates.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
lib.ntsm_eval_cross_score_pairs.restype = C.c_int
lib.ntsm_eval_cross_score_pairs.argtypes = [C.c_int, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                            C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(CrossTimes)]


class Records:
    """Database samples as a cohort store holds them: the counts of sample d, [n_sites][2] uint32, at `address + d * stride`
    inside `buf`.  Records.of(db, head_bytes) lays a dense [n_db][n_sites][2] array out with head_bytes of filler in front
    of every sample's counts (a store's record head is 1,056 bytes)."""

    def __init__(self, buf, offset, stride, n, m):
        self.buf, self.offset, self.stride, self.n, self.m = buf, offset, stride, n, m

    @property
    def address(self):
        return self.buf.ctypes.data + self.offset

    @classmethod
    def of(cls, db, head_bytes=0):
        db = np.ascontiguousarray(db, dtype=np.uint32)
        if db.ndim != 3 or db.shape[2] != 2 or head_bytes % 4:
            raise ValueError("database samples are [samples][sites][2]; the head is a multiple of 4 bytes")
        n, m = db.shape[0], db.shape[1]
        stride = head_bytes + 8 * m
        buf = np.full(n * stride + 8, 0xAB, dtype=np.uint8)
        if n and m:
            rows = np.lib.stride_tricks.as_strided(buf[head_bytes:], shape=(n, 8 * m), strides=(stride, 1))
            rows[:] = db.reshape(n, 2 * m).view(np.uint8)
        return cls(buf, head_bytes, stride, n, m)


def _records(db):
    return db if isinstance(db, Records) else Records.of(db)


def project_store(db, norm, rot, min_cov=1, db_chunk=0, device=0):
    """db: uint32 [n_db][n_sites][2] or Records; norm, rot as Session.project.  Returns (cloud [n_db][dim] -- the bits of
    project() on the dense samples --, geno [n_db][3] as cross()'s, times)."""
    r = _records(db)
    norm = np.ascontiguousarray(norm, dtype=np.longdouble)
    rot = np.ascontiguousarray(rot, dtype=np.longdouble).reshape(-1, r.m) if r.m else np.zeros((np.shape(rot)[0], 0), dtype=np.longdouble)
    dim = rot.shape[0]
    cloud = np.zeros((r.n, dim), dtype=np.float64)
    geno = np.zeros((r.n, 3), dtype=np.uint32)
    times = CrossTimes()
    rc = lib.ntsm_eval_project_store(device, r.address, r.stride, r.n, r.m, min_cov, _ld_ptr(norm), _ld_ptr(rot), dim, db_chunk,
                                     cloud.ctypes.data, geno.ctypes.data, C.byref(times))
    if rc:
        raise RuntimeError("ntsm_eval_project_store failed: %d" % rc)
    return cloud, geno, times


def cross_candidates(q_cloud, q_radius, db_cloud, db_radius, capacity=None, device=0):
    """The pairs of candidates() on the concatenated clouds and radii that have a query in them, in its order:
    (pi, pk, calcDistance, kernel ms).  capacity as Session.candidates."""
    q_cloud = np.ascontiguousarray(q_cloud, dtype=np.float64)
    db_cloud = np.ascontiguousarray(db_cloud, dtype=np.float64)
    q_radius = np.ascontiguousarray(q_radius, dtype=np.float64)
    db_radius = np.ascontiguousarray(db_radius, dtype=np.float64)
    n_q, n_db = len(q_radius), len(db_radius)
    dim = q_cloud.shape[1] if q_cloud.ndim == 2 else 0
    if n_q and n_db and (db_cloud.ndim != 2 or db_cloud.shape[1] != dim):
        raise ValueError("cross_candidates: both clouds are [samples][dim]")
    ms, n = C.c_double(), C.c_uint64()

    def call(pi, pk, dist, cap):
        return lib.ntsm_eval_cross_candidates(device, q_cloud.ctypes.data, q_radius.ctypes.data, n_q, db_cloud.ctypes.data, db_radius.ctypes.data, n_db,
                                              dim, pi, pk, dist, cap, C.byref(n), C.byref(ms))
    if capacity is None:
        rc = call(None, None, None, 0)
        if rc not in (0, E_CAPACITY):
            raise RuntimeError("ntsm_eval_cross_candidates failed: %d" % rc)
        capacity = n.value
    pi, pk = np.zeros(capacity, dtype=np.uint32), np.zeros(capacity, dtype=np.uint32)
    dist = np.zeros(capacity, dtype=np.float64)
    rc = call(pi.ctypes.data, pk.ctypes.data, dist.ctypes.data, capacity)
    if rc == E_CAPACITY:
        raise ValueError("capacity %d < %d candidate pairs" % (capacity, n.value), n.value)
    if rc:
        raise RuntimeError("ntsm_eval_cross_candidates failed: %d" % rc)
    k = n.value
    return pi[:k], pk[:k], dist[:k], ms.value


def cross_score_pairs(q, db, pi, pk, min_cov=1, db_chunk=0, device=0):
    """q: uint32 [n_q][n_sites][2]; db: [n_db][n_sites][2] or Records; pi, pk in the concatenation's numbering, a query in
    every pair.  Returns (records, sample pi as sample 1 -- the bits of score_pairs on the concatenation --, times)."""
    q = np.ascontiguousarray(q, dtype=np.uint32)
    r = _records(db)
    if q.ndim != 3 or q.shape[2] != 2 or q.shape[1] != r.m:
        raise ValueError("cross_score_pairs: q and db are [samples][sites][2] over the same sites")
    pi = np.ascontiguousarray(pi, dtype=np.uint32)
    pk = np.ascontiguousarray(pk, dtype=np.uint32)
    out = np.zeros(len(pi), dtype=RECORD)
    times = CrossTimes()
    rc = lib.ntsm_eval_cross_score_pairs(device, q.ctypes.data, q.shape[0], r.address, r.stride, r.n, r.m, min_cov, pi.ctypes.data, pk.ctypes.data,
                                         len(pi), db_chunk, out.ctypes.data, C.byref(times))
    if rc:
        raise RuntimeError("ntsm_eval_cross_score_pairs failed: %d" % rc)
    return out, times


# ---- the pairs inside a cohort store (ntsmEval --within / --within-near; include/ntsm_eval_hip.h: ntsm_eval_within_open ...
# ntsm_eval_store_score_pairs).  Sample numbers are the store's.
lib.ntsm_eval_within_open.restype = C.c_int
lib.ntsm_eval_within_open.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
lib.ntsm_eval_within_rows.restype = C.c_int
lib.ntsm_eval_within_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(CrossTimes)]
lib.ntsm_eval_within_close.restype = None
lib.ntsm_eval_within_close.argtypes = [C.c_void_p]
lib.ntsm_eval_within_tune.restype = C.c_int
lib.ntsm_eval_within_tune.argtypes = [C.c_uint32]
lib.ntsm_eval_store_score_pairs.restype = C.c_int
lib.ntsm_eval_store_score_pairs.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64,
                                            C.c_uint32, C.c_void_p, C.POINTER(CrossTimes)]


def within_tune(width):
    """Force the workgroup width (64 or 256) of later Within.rows calls in this process; 0 = the library's rule."""
    _tune("ntsm_eval_within_tune", width)


class Within(_Handle, close="ntsm_eval_within_close"):
    """The pairs of a store's samples with each other (ntsm_eval_within_open): db is uint32 [n_db][n_sites][2] or Records,
    which the session keeps alive.  db_chunk: 0 = resident if the store fits the device, else streamed; a value below n_db
    streams the columns in chunks of it.  A context manager: `with Within(db) as w: rec, geno, times = w.rows(0, w.n)`."""

    def __init__(self, db, min_cov=1, db_chunk=0, device=0):
        self.records = _records(db)
        self.n, self.m = self.records.n, self.records.m
        self.h = C.c_void_p()
        rc = lib.ntsm_eval_within_open(device, self.records.address, self.records.stride, self.n, self.m, min_cov, db_chunk, C.byref(self.h))
        if rc:
            raise RuntimeError("ntsm_eval_within_open failed: %d" % rc)

    def rows(self, row_first, n_rows):
        """The records of the pairs (i, j), row_first <= i < row_first + n_rows, i < j < n, in pair_index order (the slice
        pairs()[pair_index(row_first, row_first + 1, n):pair_index(row_first + n_rows, ...)] of the dense samples); geno
        [n][3] with the entries from row_first on written; times, a CrossTimes (chunks == 0: the store is resident)."""
        base = lambda r: r * self.n - r * (r + 1) // 2  # noqa: E731
        count = base(row_first + n_rows) - base(row_first) if 0 <= row_first and 0 < n_rows and row_first + n_rows <= self.n else 0
        out = np.zeros(count, dtype=RECORD)
        geno = np.zeros((self.n, 3), dtype=np.uint32)
        times = CrossTimes()
        rc = lib.ntsm_eval_within_rows(self.h, row_first, n_rows, out.ctypes.data, geno.ctypes.data, C.byref(times))
        if rc:
            raise RuntimeError("ntsm_eval_within_rows failed: %d" % rc)
        return out, geno, times


def store_score_pairs(db, pi, pk, min_cov=1, db_chunk=0, device=0):
    """db: [n_db][n_sites][2] or Records; pi, pk: store sample numbers.  Returns (records, sample pi as sample 1 -- the bits
    of score_pairs on the dense samples --, times; times.chunks = the passes)."""
    r = _records(db)
    pi = np.ascontiguousarray(pi, dtype=np.uint32)
    pk = np.ascontiguousarray(pk, dtype=np.uint32)
    out = np.zeros(len(pi), dtype=RECORD)
    times = CrossTimes()
    rc = lib.ntsm_eval_store_score_pairs(device, r.address, r.stride, r.n, r.m, min_cov, pi.ctypes.data, pk.ctypes.data, len(pi), db_chunk,
                                         out.ctypes.data, C.byref(times))
    if rc:
        raise RuntimeError("ntsm_eval_store_score_pairs failed: %d" % rc)
    return out, times


# ---- one cohort store against another (ntsmEval --between; include/ntsm_eval_hip.h: ntsm_eval_between_open ... _tune).  Rows are
# samples of A, columns samples of B; B's sites are matched to A's by site_map.
LACKS = 0xFFFFFFFF
lib.ntsm_eval_between_open.restype = C.c_int
lib.ntsm_eval_between_open.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                       C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
lib.ntsm_eval_between_rows.restype = C.c_int
lib.ntsm_eval_between_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(CrossTimes)]
lib.ntsm_eval_between_close.restype = None
lib.ntsm_eval_between_close.argtypes = [C.c_void_p]
lib.ntsm_eval_between_tune.restype = C.c_int
lib.ntsm_eval_between_tune.argtypes = [C.c_uint32]


def between_tune(width):
    """Force the workgroup width (64 or 256) of later Between.rows calls in this process; 0 = the library's rule."""
    _tune("ntsm_eval_between_tune", width)


class Between(_Handle, close="ntsm_eval_between_close"):
    """The samples of store A against those of store B (ntsm_eval_between_open): a and b are uint32 [n][n_sites][2] or Records,
    which the session keeps alive.  site_map: uint32 [n_sites_a], the index among B's sites of each site of A, LACKS where B
    has none; None = identical tables.  b_chunk: 0 = B resident if it fits the device, else streamed; a value below n_b
    streams B in chunks of it.  A context manager: `with Between(a, b) as s: rec, a_geno, b_geno, times = s.rows(0, s.n_a)`."""

    def __init__(self, a, b, site_map=None, min_cov=1, b_chunk=0, device=0):
        self.a, self.b = _records(a), _records(b)
        self.n_a, self.n_b = self.a.n, self.b.n
        self.site_map = None if site_map is None else np.ascontiguousarray(site_map, dtype=np.uint32)
        self.h = C.c_void_p()
        rc = lib.ntsm_eval_between_open(device, self.a.address, self.a.stride, self.n_a, self.b.address, self.b.stride, self.n_b, self.a.m, self.b.m,
                                        None if self.site_map is None else self.site_map.ctypes.data, min_cov, b_chunk, C.byref(self.h))
        if rc:
            raise RuntimeError("ntsm_eval_between_open failed: %d" % rc)

    def rows(self, row_first, n_rows):
        """Rows row_first ... row_first + n_rows - 1 of A against every sample of B: (records [n_rows, n_b], the record of
        (a, b) being that of pair (a, n_a + b) of pairs(concatenate([A, B remapped to A's sites])); a_geno [n_rows, 3] and
        b_geno [n_b, 3] over A's sites; times, a CrossTimes (chunks == 0: B is resident))."""
        count = n_rows if 0 <= row_first and 0 <= n_rows and row_first + n_rows <= self.n_a else 0
        out = np.zeros((count, self.n_b), dtype=RECORD)
        a_geno = np.zeros((count, 3), dtype=np.uint32)
        b_geno = np.zeros((self.n_b, 3), dtype=np.uint32)
        times = CrossTimes()
        rc = lib.ntsm_eval_between_rows(self.h, row_first, n_rows, out.ctypes.data, a_geno.ctypes.data, b_geno.ctypes.data, C.byref(times))
        if rc:
            raise RuntimeError("ntsm_eval_between_rows failed: %d" % rc)
        return out, a_geno, b_geno, times


# ---- the PCA-guided search between two stores (ntsmEval --between-near; ntsm_eval_project_store_mapped, ntsm_eval_between_candidates,
# ntsm_eval_between_score_pairs).  Indices follow the concatenation [A; B]: sample b of B is sample n_a + b.
lib.ntsm_eval_project_store_mapped.restype = C.c_int
lib.ntsm_eval_project_store_mapped.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32,
                                               C.POINTER(C.c_longdouble), C.POINTER(C.c_longdouble), C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                               C.POINTER(CrossTimes)]
lib.ntsm_eval_between_candidates.restype = C.c_int
lib.ntsm_eval_between_candidates.argtypes = lib.ntsm_eval_cross_candidates.argtypes
lib.ntsm_eval_between_score_pairs.restype = C.c_int
lib.ntsm_eval_between_score_pairs.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(CrossTimes)]


def _site_map(site_map):
    return None if site_map is None else np.ascontiguousarray(site_map, dtype=np.uint32)


def project_store_mapped(b, n_sites_a, site_map, norm, rot, min_cov=1, b_chunk=0, device=0):
    """The PCA-guided search between two stores (ntsmEval --between-near): b is uint32 [n_b][n_sites_b][2] or Records; site_map
    as Between's (None = identical tables: project_store); norm [n_sites_a], rot [dim][n_sites_a].  Returns (cloud [n_b][dim]
    -- the bits of project() on B remapped to A's sites --, geno [n_b][3] as cross()'s on that copy, times)."""
    r = _records(b)
    site_map = _site_map(site_map)
    norm = np.ascontiguousarray(norm, dtype=np.longdouble)
    rot = np.ascontiguousarray(rot, dtype=np.longdouble).reshape(-1, n_sites_a) if n_sites_a else np.zeros((np.shape(rot)[0], 0), dtype=np.longdouble)
    dim = rot.shape[0]
    cloud = np.zeros((r.n, dim), dtype=np.float64)
    geno = np.zeros((r.n, 3), dtype=np.uint32)
    times = CrossTimes()
    rc = lib.ntsm_eval_project_store_mapped(device, r.address, r.stride, r.n, n_sites_a, r.m, None if site_map is None else site_map.ctypes.data, min_cov,
                                            _ld_ptr(norm), _ld_ptr(rot), dim, b_chunk, cloud.ctypes.data, geno.ctypes.data, C.byref(times))
    if rc:
        raise RuntimeError("ntsm_eval_project_store_mapped failed: %d" % rc)
    return cloud, geno, times


def between_candidates(a_cloud, a_radius, b_cloud, b_radius, capacity=None, device=0):
    """The pairs of candidates() on the concatenated clouds and radii [A; B] that name one sample of each store, in its order:
    (pi, pk, calcDistance, kernel ms).  capacity as Session.candidates."""
    a_cloud = np.ascontiguousarray(a_cloud, dtype=np.float64)
    b_cloud = np.ascontiguousarray(b_cloud, dtype=np.float64)
    a_radius = np.ascontiguousarray(a_radius, dtype=np.float64)
    b_radius = np.ascontiguousarray(b_radius, dtype=np.float64)
    n_a, n_b = len(a_radius), len(b_radius)
    dim = a_cloud.shape[1] if a_cloud.ndim == 2 else 0
    if n_a and n_b and (b_cloud.ndim != 2 or b_cloud.shape[1] != dim):
        raise ValueError("between_candidates: both clouds are [samples][dim]")
    ms, n = C.c_double(), C.c_uint64()

    def call(pi, pk, dist, cap):
        return lib.ntsm_eval_between_candidates(device, a_cloud.ctypes.data, a_radius.ctypes.data, n_a, b_cloud.ctypes.data, b_radius.ctypes.data, n_b,
                                                dim, pi, pk, dist, cap, C.byref(n), C.byref(ms))
    if capacity is None:
        rc = call(None, None, None, 0)
        if rc not in (0, E_CAPACITY):
            raise RuntimeError("ntsm_eval_between_candidates failed: %d" % rc)
        capacity = n.value
    pi, pk = np.zeros(capacity, dtype=np.uint32), np.zeros(capacity, dtype=np.uint32)
    dist = np.zeros(capacity, dtype=np.float64)
    rc = call(pi.ctypes.data, pk.ctypes.data, dist.ctypes.data, capacity)
    if rc == E_CAPACITY:
        raise ValueError("capacity %d < %d candidate pairs" % (capacity, n.value), n.value)
    if rc:
        raise RuntimeError("ntsm_eval_between_candidates failed: %d" % rc)
    k = n.value
    return pi[:k], pk[:k], dist[:k], ms.value


def between_score_pairs(a, b, pi, pk, site_map=None, min_cov=1, chunk=0, device=0):
    """a, b: [n][n_sites][2] or Records; pi, pk in the numbering of [A; B], one sample of each store in every pair; site_map as
    Between's.  Returns (records, sample pi as sample 1 -- the bits of score_pairs on [A; B remapped to A's sites] --, times;
    times.chunks = the passes)."""
    ra, rb = _records(a), _records(b)
    site_map = _site_map(site_map)
    pi = np.ascontiguousarray(pi, dtype=np.uint32)
    pk = np.ascontiguousarray(pk, dtype=np.uint32)
    out = np.zeros(len(pi), dtype=RECORD)
    times = CrossTimes()
    rc = lib.ntsm_eval_between_score_pairs(device, ra.address, ra.stride, ra.n, rb.address, rb.stride, rb.n, ra.m, rb.m,
                                           None if site_map is None else site_map.ctypes.data, min_cov, pi.ctypes.data, pk.ctypes.data, len(pi), chunk,
                                           out.ctypes.data, C.byref(times))
    if rc:
        raise RuntimeError("ntsm_eval_between_score_pairs failed: %d" % rc)
    return out, times


# ---- the QC tables of a cohort store (ntsmEval --qc; include/ntsm_eval_hip.h: ntsm_eval_store_profile)
lib.ntsm_eval_store_profile.restype = C.c_int
lib.ntsm_eval_store_profile.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.POINTER(CrossTimes)]


def store_profile(db, min_cov=1, db_chunk=0, device=0, geno=True, tally=True, cov=True):
    """db: uint32 [n_db][n_sites][2] or Records.  Returns (geno [n_db][3] = hets, homs, miss per sample as cross()'s; tally
    [n_sites][4] = homAT, homCG, het, miss per site; cov uint64 [n_sites] = the raw coverage sum per site; times).  An output
    switched off is passed as NULL and returned as None."""
    r = _records(db)
    g = np.zeros((r.n, 3), dtype=np.uint32) if geno else None
    t = np.zeros((r.m, 4), dtype=np.uint32) if tally else None
    c = np.zeros(r.m, dtype=np.uint64) if cov else None
    times = CrossTimes()
    rc = lib.ntsm_eval_store_profile(device, r.address, r.stride, r.n, r.m, min_cov, db_chunk, *[None if a is None else a.ctypes.data for a in (g, t, c)],
                                     C.byref(times))
    if rc:
        raise RuntimeError("ntsm_eval_store_profile failed: %d" % rc)
    return g, t, c, times


def site_table_text(locus, tally, cov, n_samples):
    """The bytes of `ntsmEval --qc --sites-out` for these integers (ntsm_amd/csrc/host/eval_qc.hpp through libntsm_host.so):
    locus: IDs; tally [n_sites][4]; cov [n_sites]."""
    from .capi import HO
    tally = np.ascontiguousarray(tally, dtype=np.uint32).reshape(-1, 4)
    cov = np.ascontiguousarray(cov, dtype=np.uint64)
    ids = (C.c_char_p * len(locus))(*[s.encode() for s in locus])
    out, ln = C.c_void_p(), C.c_size_t()
    rc = HO.ntsm_host_site_table(ids, len(locus), tally.ctypes.data_as(C.POINTER(C.c_uint32)), cov.ctypes.data_as(C.POINTER(C.c_uint64)), n_samples,
                                 C.byref(out), C.byref(ln))
    if rc:
        raise RuntimeError("ntsm_host_site_table failed: %d" % rc)
    data = C.string_at(out, ln.value)
    HO.ntsm_host_free(out)
    return data


# ---- the cross-sample contamination check over a cohort store (ntsmEval --contam; include/ntsm_eval_hip.h: ntsm_eval_contam_open ...
# _tune).  Rows are targets, columns sources, both the store's samples.
CONTAM_RECORD = np.dtype([("minor", "<u8", 3), ("depth", "<u8", 3), ("sites", "<u4", 3), ("pad", "<u4")])
assert CONTAM_RECORD.itemsize == 64
lib.ntsm_eval_contam_open.restype = C.c_int
lib.ntsm_eval_contam_open.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]
lib.ntsm_eval_contam_rows.restype = C.c_int
lib.ntsm_eval_contam_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(CrossTimes)]
lib.ntsm_eval_contam_close.restype = None
lib.ntsm_eval_contam_close.argtypes = [C.c_void_p]
lib.ntsm_eval_contam_tune.restype = C.c_int
lib.ntsm_eval_contam_tune.argtypes = [C.c_uint32, C.c_uint32]


def contam_tune(width, target_group):
    """Force the workgroup width (64 or 256) and target group (1, 2 or 4) of later Contam.rows calls in this process; 0 = the
    library's rule."""
    _tune("ntsm_eval_contam_tune", width, target_group)


class Contam(_Handle, close="ntsm_eval_contam_close"):
    """Every sample of a store as a target against every sample as a source (ntsm_eval_contam_open): db is uint32
    [n_db][n_sites][2] or Records, which the session keeps alive.  db_chunk: 0 = resident if the store fits the device, else
    streamed; a value below n_db streams the columns in chunks of it.  A context manager:
    `with Contam(db) as s: rec, tally, times = s.rows(0, s.n)`."""

    def __init__(self, db, min_cov=1, min_depth=8, db_chunk=0, device=0):
        self.records = _records(db)
        self.n, self.m = self.records.n, self.records.m
        self.h = C.c_void_p()
        rc = lib.ntsm_eval_contam_open(device, self.records.address, self.records.stride, self.n, self.m, min_cov, min_depth, db_chunk, C.byref(self.h))
        if rc:
            raise RuntimeError("ntsm_eval_contam_open failed: %d" % rc)

    def rows(self, row_first, n_rows, tally=True):
        """Targets row_first ... row_first + n_rows - 1 against every source: (records [n_rows, n] of CONTAM_RECORD; tally
        uint64 [n_rows, 3] = sites, minor reads, depth of each target, or None when switched off (passed as NULL); times, a
        CrossTimes (chunks == 0: the store is resident))."""
        count = n_rows if 0 <= row_first and 0 <= n_rows and row_first + n_rows <= self.n else 0
        out = np.zeros((count, self.n), dtype=CONTAM_RECORD)
        t = np.zeros((count, 3), dtype=np.uint64) if tally else None
        times = CrossTimes()
        rc = lib.ntsm_eval_contam_rows(self.h, row_first, n_rows, out.ctypes.data, None if t is None else t.ctypes.data, C.byref(times))
        if rc:
            raise RuntimeError("ntsm_eval_contam_rows failed: %d" % rc)
        return out, t, times


def _names(names):
    return (C.c_char_p * len(names))(*[s.encode() for s in names])


def _host_text(out, ln):
    from .capi import HO
    data = C.string_at(out, ln.value)
    HO.ntsm_host_free(out)
    return data


def contam_rows_text(names, row_first, rec, tally, all_rows=False, min_excess=0.01, min_explained=0.5):
    """The stdout lines of `ntsmEval --contam` for one band, without the header (ntsm_amd/csrc/host/eval_contam.hpp through
    libntsm_host.so): names of all n samples; rec [n_rows][n] of CONTAM_RECORD and tally [n_rows][3] as Contam.rows gives them."""
    from .capi import HO
    rec = np.ascontiguousarray(rec, dtype=CONTAM_RECORD).reshape(-1, len(names))
    tally = np.ascontiguousarray(tally, dtype=np.uint64).reshape(-1, 3)
    out, ln = C.c_void_p(), C.c_size_t()
    rc = HO.ntsm_host_contam_rows(_names(names), len(names), row_first, rec.shape[0], rec.ctypes.data, tally.ctypes.data_as(C.POINTER(C.c_uint64)),
                                  int(all_rows), min_excess, min_explained, C.byref(out), C.byref(ln))
    if rc:
        raise RuntimeError("ntsm_host_contam_rows failed: %d" % rc)
    return _host_text(out, ln)


def contam_sample_table_text(names, tally):
    """The bytes of `ntsmEval --contam --samples-out` for these tallies [n][3], header line included."""
    from .capi import HO
    tally = np.ascontiguousarray(tally, dtype=np.uint64).reshape(-1, 3)
    out, ln = C.c_void_p(), C.c_size_t()
    rc = HO.ntsm_host_contam_sample_table(_names(names), len(names), tally.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(out), C.byref(ln))
    if rc:
        raise RuntimeError("ntsm_host_contam_sample_table failed: %d" % rc)
    return _host_text(out, ln)


def contam_band_rows(row_first, n_db, limit=(1 << 30) // 64):
    """The band rule of --contam: the targets a band from row_first takes under `limit` records."""
    from .capi import HO
    return HO.ntsm_host_contam_band_rows(row_first, n_db, limit)


# ---- parent-parent-child trios in a cohort store (ntsmEval --trios; include/ntsm_eval_hip.h: ntsm_eval_trio_open ... _tune).
TRIO_DUO = np.dtype([("called", "<u4"), ("opp", "<u4")])
TRIO_RECORD = np.dtype([("called", "<u4"), ("err_hom", "<u4"), ("err_het", "<u4"), ("pad", "<u4")])
assert TRIO_DUO.itemsize == 8 and TRIO_RECORD.itemsize == 16
lib.ntsm_eval_trio_open.restype = C.c_int
lib.ntsm_eval_trio_open.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(CrossTimes),
                                    C.POINTER(C.c_void_p)]
lib.ntsm_eval_trio_duos.restype = C.c_int
lib.ntsm_eval_trio_duos.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_double)]
lib.ntsm_eval_trio_score.restype = C.c_int
lib.ntsm_eval_trio_score.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_double)]
lib.ntsm_eval_trio_close.restype = None
lib.ntsm_eval_trio_close.argtypes = [C.c_void_p]
lib.ntsm_eval_trio_tune.restype = C.c_int
lib.ntsm_eval_trio_tune.argtypes = [C.c_uint32]


def trio_tune(width):
    """Force the workgroup width (64 or 256) of later Trio.duos and Trio.score calls in this process; 0 = the library's rule."""
    _tune("ntsm_eval_trio_tune", width)


class Trio(_Handle, close="ntsm_eval_trio_close"):
    """The genotype bit-planes of a store on the device (ntsm_eval_trio_open): db is uint32 [n_db][n_sites][2] or Records, read
    once, here.  geno: uint32 [n_db, 4] = homAT, het, homCG, miss, or None when switched off (passed as NULL); times: the
    CrossTimes of open.  A context manager: `with Trio(db) as s: duo, ms = s.duos(0, s.n)`."""

    def __init__(self, db, min_cov=1, min_depth=8, db_chunk=0, device=0, geno=True):
        records = _records(db)
        self.n, self.m = records.n, records.m
        self.h = C.c_void_p()
        self.geno = np.zeros((self.n, 4), dtype=np.uint32) if geno else None
        self.times = CrossTimes()
        rc = lib.ntsm_eval_trio_open(device, records.address, records.stride, self.n, self.m, min_cov, min_depth, db_chunk,
                                     None if self.geno is None else self.geno.ctypes.data, C.byref(self.times), C.byref(self.h))
        if rc:
            raise RuntimeError("ntsm_eval_trio_open failed: %d" % rc)

    def duos(self, row_first, n_rows):
        """Rows row_first ... row_first + n_rows - 1 against every sample: (records [n_rows, n] of TRIO_DUO, kernel ms)."""
        count = n_rows if 0 <= row_first and 0 <= n_rows and row_first + n_rows <= self.n else 0
        out = np.zeros((count, self.n), dtype=TRIO_DUO)
        ms = C.c_double()
        rc = lib.ntsm_eval_trio_duos(self.h, row_first, n_rows, out.ctypes.data, C.byref(ms))
        if rc:
            raise RuntimeError("ntsm_eval_trio_duos failed: %d" % rc)
        return out, ms.value

    def score(self, children, lists):
        """The trios of every entry (children[i]; every pair of positions p < q of lists[i]), in CSR order: (records of
        TRIO_RECORD, kernel ms)."""
        child = np.ascontiguousarray(children, dtype=np.uint32)
        offset = np.zeros(len(lists) + 1, dtype=np.uint64)
        offset[1:] = np.cumsum([len(l) for l in lists], dtype=np.uint64)
        cand = np.ascontiguousarray(np.concatenate([np.asarray(l, dtype=np.uint32) for l in lists]) if len(lists) else [], dtype=np.uint32)
        out = np.zeros(sum(len(l) * (len(l) - 1) // 2 for l in lists), dtype=TRIO_RECORD)
        ms = C.c_double()
        rc = lib.ntsm_eval_trio_score(self.h, child.ctypes.data, offset.ctypes.data, cand.ctypes.data, len(lists), out.ctypes.data, C.byref(ms))
        if rc:
            raise RuntimeError("ntsm_eval_trio_score failed: %d" % rc)
        return out, ms.value


def _u32(a):
    a = np.ascontiguousarray(a, dtype=np.uint32)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint32))


def trio_rows_text(names, child, pa, pb, rec, da, db, ped=False, all_rows=False, min_called=200, max_rate=0.02):
    """The stdout lines of `ntsmEval --trios` for these evaluated triples, without the header (ntsm_amd/csrc/host/eval_trio.hpp
    through libntsm_host.so): child, pa, pb index names; rec of TRIO_RECORD; da, db of TRIO_DUO = (child, parentA), (child, parentB)."""
    from .capi import HO
    (child, cp), (pa, ap), (pb, bp) = _u32(child), _u32(pa), _u32(pb)
    rec = np.ascontiguousarray(rec, dtype=TRIO_RECORD)
    da, db = np.ascontiguousarray(da, dtype=TRIO_DUO), np.ascontiguousarray(db, dtype=TRIO_DUO)
    out, ln = C.c_void_p(), C.c_size_t()
    rc = HO.ntsm_host_trio_rows(_names(names), len(names), len(child), cp, ap, bp, rec.ctypes.data, da.ctypes.data, db.ctypes.data, int(ped), int(all_rows),
                                min_called, max_rate, C.byref(out), C.byref(ln))
    if rc:
        raise RuntimeError("ntsm_host_trio_rows failed: %d" % rc)
    return _host_text(out, ln)


def trio_ped_parse(text, names):
    """The complete trios of a pedigree file's bytes as samples of names: ([(child, father, mother), ...], comment lines skipped,
    lines with a 0 parent skipped); a refusal raises ValueError with its sentence."""
    from .capi import HO
    trios, n, err, err_len = C.c_void_p(), C.c_size_t(), C.c_void_p(), C.c_size_t()
    comments, founders = C.c_uint64(), C.c_uint64()
    rc = HO.ntsm_host_trio_ped_parse(text, len(text), _names(names), len(names), C.byref(trios), C.byref(n), C.byref(comments), C.byref(founders),
                                     C.byref(err), C.byref(err_len))
    if rc == 1:
        raise ValueError(_host_text(err, err_len).decode())
    if rc:
        raise RuntimeError("ntsm_host_trio_ped_parse failed: %d" % rc)
    flat = np.ctypeslib.as_array(C.cast(trios, C.POINTER(C.c_uint32)), shape=(max(n.value, 1) * 3,))[:n.value * 3].copy()
    HO.ntsm_host_free(trios)
    return [tuple(int(v) for v in flat[3 * i:3 * i + 3]) for i in range(n.value)], comments.value, founders.value


def trio_match(names, sample_id):
    """The sample an ID of a pedigree names: its index, -1 where none matches, -2 where the first matching level is ambiguous."""
    from .capi import HO
    return HO.ntsm_host_trio_match(_names(names), len(names), sample_id.encode())


def trio_candidates(row, child, min_called=200, max_duo=0.02):
    """The candidate parents of `child` out of its duo row (TRIO_DUO [n_db]), in store order."""
    from .capi import HO
    row = np.ascontiguousarray(row, dtype=TRIO_DUO)
    out = np.zeros(max(len(row), 1), dtype=np.uint32)
    n = HO.ntsm_host_trio_candidates(row.ctypes.data, len(row), child, min_called, max_duo, out.ctypes.data_as(C.POINTER(C.c_uint32)))
    return out[:n].tolist()


def trio_batches(lengths, limit=(1 << 30) // 16):
    """The batch cutter of --trios: (the ends of the batches, None), or (None, the position of a list that alone exceeds limit)."""
    from .capi import HO
    k, kp = _u32(lengths)
    ends = (C.c_size_t * max(len(k), 1))()
    n_ends = C.c_size_t()
    bad = HO.ntsm_host_trio_batches(kp, len(k), limit, ends, C.byref(n_ends))
    return (list(ends[:n_ends.value]), None) if bad == len(k) else (None, bad)


# ---- site-pair LD over a cohort store (ntsmEval --ld; include/ntsm_eval_hip.h: ntsm_eval_ld_open ... _tune).
LD_RECORD = np.dtype([(f, "<u4") for f in ("n", "hs", "gs", "ht", "gt", "hh", "hg", "gg")])
LD_PAIR = np.dtype([("a", "<u4"), ("b", "<u4"), ("rec", LD_RECORD)])
assert LD_RECORD.itemsize == 32 and LD_PAIR.itemsize == 40
lib.ntsm_eval_ld_open.restype = C.c_int
lib.ntsm_eval_ld_open.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(CrossTimes),
                                  C.POINTER(C.c_void_p)]
lib.ntsm_eval_ld_rows.restype = C.c_int
lib.ntsm_eval_ld_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(C.c_double)]
lib.ntsm_eval_ld_select.restype = C.c_int
lib.ntsm_eval_ld_select.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
lib.ntsm_eval_ld_close.restype = None
lib.ntsm_eval_ld_close.argtypes = [C.c_void_p]
lib.ntsm_eval_ld_tune.restype = C.c_int
lib.ntsm_eval_ld_tune.argtypes = [C.c_uint32, C.c_uint32]


def ld_tune(block_rows, block_cols):
    """Force the register block (2 x 2, 4 x 2 or 2 x 4 pairs per lane) of later Ld.rows and Ld.select calls in this process;
    (0, 0) = the library's rule."""
    _tune("ntsm_eval_ld_tune", block_rows, block_cols)


class Ld(_Handle, close="ntsm_eval_ld_close"):
    """The genotype bit-planes of a store on the device, samples along the bits (ntsm_eval_ld_open): db is uint32
    [n_db][n_sites][2] or Records, read once, here.  site_geno: uint32 [n_sites, 4] = het, homCG, called, homAT, or None when
    switched off (passed as NULL); times: the CrossTimes of open.  A context manager: `with Ld(db) as s: rec, ms = s.rows(0, s.m)`."""

    def __init__(self, db, min_cov=1, min_depth=8, db_chunk=0, device=0, site_geno=True):
        records = _records(db)
        self.n, self.m = records.n, records.m
        self.h = C.c_void_p()
        self.site_geno = np.zeros((self.m, 4), dtype=np.uint32) if site_geno else None
        self.times = CrossTimes()
        rc = lib.ntsm_eval_ld_open(device, records.address, records.stride, self.n, self.m, min_cov, min_depth, db_chunk,
                                   None if self.site_geno is None else self.site_geno.ctypes.data, C.byref(self.times), C.byref(self.h))
        if rc:
            raise RuntimeError("ntsm_eval_ld_open failed: %d" % rc)

    def rows(self, row_first, n_rows):
        """Sites row_first ... row_first + n_rows - 1 against every site: (records [n_rows, m] of LD_RECORD, kernel ms)."""
        count = n_rows if 0 <= row_first and 0 <= n_rows and row_first + n_rows <= self.m else 0
        out = np.zeros((count, self.m), dtype=LD_RECORD)
        ms = C.c_double()
        rc = lib.ntsm_eval_ld_rows(self.h, row_first, n_rows, out.ctypes.data, C.byref(ms))
        if rc:
            raise RuntimeError("ntsm_eval_ld_rows failed: %d" % rc)
        return out, ms.value

    def select(self, row_first, n_rows, min_called=20, r2_min=0.5, cap=None):
        """The selected pairs (a, b), a in the band, a < b, sorted: (return code 0 or 1, pairs of LD_PAIR -- empty on 1 --, the
        true number found, kernel ms).  cap None: as many as the band can hold."""
        if cap is None:
            cap = max(n_rows, 0) * self.m
        out = np.zeros(max(cap, 1), dtype=LD_PAIR)
        found, ms = C.c_uint64(), C.c_double()
        rc = lib.ntsm_eval_ld_select(self.h, row_first, n_rows, min_called, r2_min, cap, out.ctypes.data, C.byref(found), C.byref(ms))
        if rc not in (0, 1):
            raise RuntimeError("ntsm_eval_ld_select failed: %d" % rc)
        return rc, out[:0 if rc else found.value].copy(), found.value, ms.value


def ld_r2(rec, min_called=20):
    """The moments and r^2 of one LD_RECORD through libntsm_host.so: ((n, cov, vx, vy), r2 or None where it is undefined)."""
    from .capi import HO
    rec = np.ascontiguousarray(rec, dtype=LD_RECORD).reshape(1)
    mom, r2 = (C.c_int64 * 4)(), C.c_double()
    rc = HO.ntsm_host_ld_r2(rec.ctypes.data, min_called, mom, C.byref(r2))
    if rc < 0:
        raise RuntimeError("ntsm_host_ld_r2 failed: %d" % rc)
    return tuple(mom), (r2.value if rc else None)


def ld_rows_text(locus, pairs):
    """The stdout lines of `ntsmEval --ld` for these LD_PAIRs, in their order, without the header."""
    from .capi import HO
    pairs = np.ascontiguousarray(pairs, dtype=LD_PAIR)
    out, ln = C.c_void_p(), C.c_size_t()
    rc = HO.ntsm_host_ld_rows(_names(locus), len(locus), pairs.ctypes.data, len(pairs), C.byref(out), C.byref(ln))
    if rc:
        raise RuntimeError("ntsm_host_ld_rows failed: %d" % rc)
    return _host_text(out, ln)


def ld_prune(n_sites, pairs, min_called=20, r2_min=0.5):
    """The prune of --ld over LD_PAIRs in (a, b) order: a bool array [n_sites], True = kept."""
    from .capi import HO
    pairs = np.ascontiguousarray(pairs, dtype=LD_PAIR)
    kept = np.zeros(max(n_sites, 1), dtype=np.uint8)
    rc = HO.ntsm_host_ld_prune(n_sites, pairs.ctypes.data, len(pairs), min_called, r2_min, kept.ctypes.data)
    if rc:
        raise RuntimeError("ntsm_host_ld_prune failed: %d" % rc)
    return kept[:n_sites].astype(bool)


def ld_bands(row_pairs, budget=(1 << 30) // 40):
    """The band walk of --ld over a model device that selects row_pairs[a] pairs in row a: ([(first, rows, return), ...] of
    every call, (bands, re-runs, pairs))."""
    from .capi import HO
    rp = np.ascontiguousarray(row_pairs, dtype=np.uint64)
    room = 4 * len(rp) + 64
    calls = np.zeros((room, 3), dtype=np.uint32)
    stats = (C.c_uint64 * 3)()
    n = HO.ntsm_host_ld_bands(rp.ctypes.data_as(C.POINTER(C.c_uint64)), len(rp), budget, calls.ctypes.data_as(C.POINTER(C.c_uint32)), room, stats)
    if n < 0 or n > room:
        raise RuntimeError("ntsm_host_ld_bands failed: %d" % n)
    return [tuple(int(v) for v in c) for c in calls[:n]], tuple(stats)
