"""ctypes plumbing for include/ntsm_pca_hip.h (the device steps of ntsmPCA); used by tests and tools.
Loaded on demand: `import ntsm_amd.pca`.  Fails loudly when libntsm_pca_hip.so has not been built."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_path = os.path.join(_HERE, "libntsm_pca_hip.so")
if not os.path.exists(_path):
    raise ImportError("%s is missing: run `make` (there is no CPU fallback)" % _path)
lib = C.CDLL(_path)

E_ARG, E_HIP, E_SOLVER_MISSING, E_SOLVER, E_RANK = -1, -2, -3, -4, -5


class Times(C.Structure):
    _fields_ = [("upload_ms", C.c_double), ("centre_ms", C.c_double), ("gram_ms", C.c_double), ("eigen_ms", C.c_double),
                ("project_ms", C.c_double), ("download_ms", C.c_double), ("gram_flops", C.c_uint64),
                ("gram_bytes", C.c_uint64), ("gram_tiles", C.c_uint32), ("gram_split", C.c_uint32)]


class RankError(RuntimeError):
    """A requested component has no positive eigenvalue beyond rounding; .component says which."""

    def __init__(self, component):
        RuntimeError.__init__(self, "component %d has no positive eigenvalue beyond rounding" % component)
        self.component = component


lib.ntsm_pca_gram.restype = C.c_int
lib.ntsm_pca_gram.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p,
                              C.POINTER(Times)]
lib.ntsm_pca_run.restype = C.c_int
lib.ntsm_pca_run.argtypes = [C.c_int, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(Times)]
_CELLS = [C.c_int, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
lib.ntsm_pca_expand_cells.restype = C.c_int
lib.ntsm_pca_expand_cells.argtypes = _CELLS + [C.c_void_p, C.POINTER(C.c_double)]
lib.ntsm_pca_gram_cells.restype = C.c_int
lib.ntsm_pca_gram_cells.argtypes = _CELLS + [C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(Times), C.POINTER(C.c_double)]
lib.ntsm_pca_run_cells.restype = C.c_int
lib.ntsm_pca_run_cells.argtypes = _CELLS + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32),
                                            C.POINTER(Times), C.POINTER(C.c_double)]
NO_UNDEF = (1 << 64) - 1


def _matrix(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("the matrix must be 2-D [sites][samples] and not empty")
    return a


def gram(a, centre=True, split=0, device=0):
    """The Gram step on its own.  a: [p sites][n samples].  Returns (G float64 [n][n] = Ac^T Ac, or A^T A with
    centre=False; the row means float64 [p]; Times).  split: pieces of the site dimension, 0 = chosen by the library."""
    a = _matrix(a)
    p, n = a.shape
    g = np.empty((n, n), dtype=np.float64)
    means = np.empty(p, dtype=np.float64)
    times = Times()
    rc = lib.ntsm_pca_gram(device, p, n, a.ctypes.data, 1 if centre else 0, split, g.ctypes.data, means.ctypes.data,
                           C.byref(times))
    if rc:
        raise RuntimeError("ntsm_pca_gram failed: %d" % rc)
    return g, means, times


def run(a, d, split=0, device=0):
    """The whole PCA of a [p sites][n samples].  Returns (eigenvalues float64 [d] descending, rotation float64 [p][d],
    components float64 [n][d], Times), signs fixed as sklearn's full solver fixes them."""
    a = _matrix(a)
    p, n = a.shape
    eigval = np.empty(d, dtype=np.float64)
    rot = np.empty((p, d), dtype=np.float64)
    comp = np.empty((n, d), dtype=np.float64)
    bad = C.c_uint32()
    times = Times()
    rc = lib.ntsm_pca_run(device, p, n, a.ctypes.data, d, split, eigval.ctypes.data, rot.ctypes.data, comp.ctypes.data,
                          C.byref(bad), C.byref(times))
    if rc == E_RANK:
        raise RankError(bad.value)
    if rc == E_SOLVER_MISSING:
        raise RuntimeError("rocSOLVER cannot be loaded (librocsolver.so.0, librocsolver.so)")
    if rc:
        raise RuntimeError("ntsm_pca_run failed: %d" % rc)
    return eigval, rot, comp, times


def _cells(cells, value, row_fill, first_undef_cell):
    """The cell form of the matrix as the ABI takes it: (p, n, cells, value, row_fill, first_undef_cell).  None stays
    None (a NULL pointer, which the library refuses)."""
    if cells is not None:
        cells = np.ascontiguousarray(cells, dtype=np.uint16)
        if cells.ndim != 2 or cells.shape[0] < 1 or cells.shape[1] < 1:
            raise ValueError("the cells must be 2-D [sites][samples] and not empty")
    if value is not None:
        value = np.ascontiguousarray(value, dtype=np.float64)
        if value.shape != (2, 65536):
            raise ValueError("value must be [2][65536]: [long form][cell code]")
    if row_fill is not None:
        row_fill = np.ascontiguousarray(row_fill, dtype=np.float64)
        if cells is not None and row_fill.shape != (cells.shape[0],):
            raise ValueError("row_fill must hold one value per site")
    first = NO_UNDEF if first_undef_cell is None else int(first_undef_cell)
    return cells, value, row_fill, first


def _ptr(x):
    return None if x is None else x.ctypes.data


def expand_cells(cells, value, row_fill, first_undef_cell=None, device=0, shape=None):
    """The expansion step on its own.  cells: uint16 [p sites][n samples] of ntsm_amd.vcf.run; value: float64 [2][65536],
    [long form][code]; row_fill: float64 [p], the value of a cell of code 0; first_undef_cell: the linear index after
    which the long form holds, None for none.  Returns (the matrix float64 [p][n], the kernel's milliseconds).
    shape: (p, n) where cells is None (the argument checks)."""
    cells, value, row_fill, first = _cells(cells, value, row_fill, first_undef_cell)
    p, n = cells.shape if cells is not None else shape
    a = np.empty((p, n), dtype=np.float64)
    ms = C.c_double()
    rc = lib.ntsm_pca_expand_cells(device, p, n, _ptr(cells), _ptr(value), _ptr(row_fill), first, a.ctypes.data, C.byref(ms))
    if rc:
        raise RuntimeError("ntsm_pca_expand_cells failed: %d" % rc)
    return a, ms.value


def gram_cells(cells, value, row_fill, first_undef_cell=None, centre=True, split=0, device=0):
    """gram() on the cell form of the matrix: (G, the row means, Times)."""
    cells, value, row_fill, first = _cells(cells, value, row_fill, first_undef_cell)
    p, n = cells.shape
    g = np.empty((n, n), dtype=np.float64)
    means = np.empty(p, dtype=np.float64)
    times = Times()
    rc = lib.ntsm_pca_gram_cells(device, p, n, _ptr(cells), _ptr(value), _ptr(row_fill), first, 1 if centre else 0, split,
                                 g.ctypes.data, means.ctypes.data, C.byref(times), None)
    if rc:
        raise RuntimeError("ntsm_pca_gram_cells failed: %d" % rc)
    return g, means, times


def run_cells(cells, value, row_fill, d, first_undef_cell=None, split=0, device=0, shape=None):
    """run() on the cell form of the matrix: (eigenvalues, rotation, components, Times, the expansion's milliseconds) --
    the same bits as run(expand_cells(...)[0], d, split) in the same process."""
    cells, value, row_fill, first = _cells(cells, value, row_fill, first_undef_cell)
    p, n = cells.shape if cells is not None else shape
    eigval = np.empty(max(d, 1), dtype=np.float64)
    rot = np.empty((p, max(d, 1)), dtype=np.float64)
    comp = np.empty((n, max(d, 1)), dtype=np.float64)
    bad = C.c_uint32()
    times = Times()
    ms = C.c_double()
    rc = lib.ntsm_pca_run_cells(device, p, n, _ptr(cells), _ptr(value), _ptr(row_fill), first, d, split, eigval.ctypes.data,
                                rot.ctypes.data, comp.ctypes.data, C.byref(bad), C.byref(times), C.byref(ms))
    if rc == E_RANK:
        raise RankError(bad.value)
    if rc == E_SOLVER_MISSING:
        raise RuntimeError("rocSOLVER cannot be loaded (librocsolver.so.0, librocsolver.so)")
    if rc:
        raise RuntimeError("ntsm_pca_run_cells failed: %d" % rc)
    return eigval, rot, comp, times, ms.value


# ---- the matrix from a cohort store (ntsmPCA --store)
class StoreTimes(C.Structure):
    _fields_ = [("upload_ms", C.c_double), ("genotype_ms", C.c_double), ("fill_ms", C.c_double), ("expand_ms", C.c_double),
                ("chunks", C.c_uint32), ("chunk", C.c_uint32)]


_STORE = [C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint32, C.c_uint32]
lib.ntsm_pca_store_cells.restype = C.c_int
lib.ntsm_pca_store_cells.argtypes = _STORE + [C.c_void_p, C.c_void_p, C.POINTER(StoreTimes)]
lib.ntsm_pca_run_store.restype = C.c_int
lib.ntsm_pca_run_store.argtypes = _STORE + [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32),
                                            C.POINTER(Times), C.POINTER(StoreTimes)]


def store_value_table():
    """The value of the cell codes of store_cells: float64 [2][65536] with [0][1..3] = 0, 0.5, 1 (NaN elsewhere)."""
    value = np.full((2, 65536), np.nan, dtype=np.float64)
    value[0, 1:4] = (0.0, 0.5, 1.0)
    return value


def _store(db, n):
    """(address, stride, samples, sites, what keeps the memory alive) of db: uint32 [samples][sites][2], or anything with
    .address / .stride / .n / .m (ntsm_amd.eval.Records: samples at a store's pitch); n: the first n samples, None = all."""
    if not hasattr(db, "address"):
        db = np.ascontiguousarray(db, dtype=np.uint32)
        if db.ndim != 3 or db.shape[2] != 2:
            raise ValueError("the samples are uint32 [samples][sites][2]")
        address, stride, have, m = db.ctypes.data, 8 * db.shape[1], db.shape[0], db.shape[1]
    else:
        address, stride, have, m = db.address, db.stride, db.n, db.m
    n = have if n is None else int(n)
    if n > have:
        raise ValueError("%d samples asked for, %d given" % (n, have))
    return address, stride, n, m, db


def store_cells(db, min_cov=1, db_chunk=0, n=None, device=0):
    """The genotype step on its own.  Returns (cells uint16 [sites][n]: code + 1 = 1, 2, 3 for genotype 0, 0.5, 1 and
    0 where the sample does not call the site; tallies uint32 [sites][3] = n_half, n_one, n_called; StoreTimes)."""
    address, stride, n, m, keep = _store(db, n)
    cells = np.zeros((m, n), dtype=np.uint16)
    tallies = np.zeros((m, 3), dtype=np.uint32)
    times = StoreTimes()
    rc = lib.ntsm_pca_store_cells(device, address, stride, n, m, min_cov, db_chunk, cells.ctypes.data, tallies.ctypes.data, C.byref(times))
    if rc:
        raise RuntimeError("ntsm_pca_store_cells failed: %d" % rc)
    return cells, tallies, times


def run_store(db, d, min_cov=1, db_chunk=0, split=0, n=None, device=0):
    """The whole PCA of the first n samples of db: (eigenvalues, rotation [sites][d], components [n][d], tallies
    [sites][3], Times, StoreTimes) -- the same bits as run_cells on store_cells' cells with store_value_table() and the
    fills of the tallies, in the same process, for every db_chunk."""
    address, stride, n, m, keep = _store(db, n)
    eigval = np.empty(max(d, 1), dtype=np.float64)
    rot = np.empty((m, max(d, 1)), dtype=np.float64)
    comp = np.empty((n, max(d, 1)), dtype=np.float64)
    tallies = np.zeros((m, 3), dtype=np.uint32)
    bad = C.c_uint32()
    times, store_times = Times(), StoreTimes()
    rc = lib.ntsm_pca_run_store(device, address, stride, n, m, min_cov, db_chunk, d, split, eigval.ctypes.data, rot.ctypes.data,
                                comp.ctypes.data, tallies.ctypes.data, C.byref(bad), C.byref(times), C.byref(store_times))
    if rc == E_RANK:
        raise RankError(bad.value)
    if rc == E_SOLVER_MISSING:
        raise RuntimeError("rocSOLVER cannot be loaded (librocsolver.so.0, librocsolver.so)")
    if rc:
        raise RuntimeError("ntsm_pca_run_store failed: %d" % rc)
    return eigval, rot, comp, tallies, times, store_times
