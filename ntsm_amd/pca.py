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
