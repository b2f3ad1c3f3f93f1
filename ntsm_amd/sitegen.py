"""ctypes plumbing for include/ntsm_sitegen_hip.h (the device step of ntsmSiteGen) and include/ntsm_sitegen_gap_hip.h (the
device step of `ntsmSiteGen -g`); used by tests and tools.
Loaded on demand: `import ntsm_amd.sitegen`.  Fails loudly when libntsm_sitegen_hip.so has not been built; the second
library, libntsm_sitegen_gap_hip.so, is loaded by the first GapSession (or gap_lib()), and fails as loudly then."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_path = os.path.join(_HERE, "libntsm_sitegen_hip.so")
if not os.path.exists(_path):
    raise ImportError("%s is missing: run `make` (there is no CPU fallback)" % _path)


class Times(C.Structure):
    _fields_ = [("table_build_ms", C.c_double), ("table_upload_ms", C.c_double), ("stage_ms", C.c_double), ("upload_ms", C.c_double),
                ("kernel_ms", C.c_double), ("full_kernel_ms_min", C.c_double), ("full_kernel_ms_max", C.c_double),
                ("launches", C.c_uint64), ("full_launches", C.c_uint64), ("windows", C.c_uint64), ("bitmap_tests", C.c_uint64),
                ("probes", C.c_uint64), ("genome_bytes", C.c_uint64), ("table_bytes", C.c_uint64)]


class GapStats(C.Structure):
    _fields_ = [("table_build_ms", C.c_double), ("table_upload_ms", C.c_double), ("stage_ms", C.c_double), ("upload_ms", C.c_double),
                ("kernel_ms", C.c_double), ("full_kernel_ms_min", C.c_double), ("full_kernel_ms_max", C.c_double),
                ("launches", C.c_uint64), ("full_launches", C.c_uint64), ("windows", C.c_uint64), ("windows_long", C.c_uint64),
                ("windows_short", C.c_uint64), ("bitmap_tests", C.c_uint64), ("probes", C.c_uint64), ("genome_bytes", C.c_uint64),
                ("table_bytes", C.c_uint64)]


def _declare(l, session):
    """argument and result types of the five functions of the library behind a session class"""
    def f(name):
        return getattr(l, session._prefix + "_" + name)
    f("open").restype = C.c_int
    f("open").argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)]
    f("submit").restype = C.c_int
    f("submit").argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    f("hits").restype = C.c_int
    f("hits").argtypes = [C.c_void_p] + [C.c_void_p] * session._n_hits
    f(session._stats).restype = C.c_int
    f(session._stats).argtypes = [C.c_void_p, C.POINTER(session._stats_type)]
    f("close").restype = None
    f("close").argtypes = [C.c_void_p]
    return l


_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i


def pack(kmers, k):
    """k-mers (str or bytes over ACGT, each k long) -> uint64, base i in bits 2(k-1-i) .. 2(k-1-i)+1, A 0 C 1 G 2 T 3"""
    out = np.zeros(len(kmers), dtype=np.uint64)
    if not len(kmers):
        return out
    raw = np.frombuffer(b"".join(s.encode() if isinstance(s, str) else s for s in kmers), dtype=np.uint8)
    if raw.size != len(kmers) * k:
        raise ValueError("every candidate must be %d bases long" % k)
    codes = _CODE[raw].reshape(len(kmers), k)
    if (codes > 3).any():
        raise ValueError("candidates must be over ACGT")
    for i in range(k):
        out = (out << np.uint64(2)) | codes[:, i].astype(np.uint64)
    return out


class Session:
    """One candidate set on one device.  submit() takes genome text in pieces; hits() returns min(H, 255) per candidate."""
    _prefix, _n_hits, _stats, _stats_type = "ntsm_sitegen", 1, "times_get", Times

    @staticmethod
    def _library():
        return lib

    def __init__(self, kmers, k, x=1, device=0):
        """x: the substitutions allowed (GapSession: the end margin e, the fourth argument of its open as x is of this one)"""
        self._lib = self._library()
        self._h = C.c_void_p()
        packed = kmers if isinstance(kmers, np.ndarray) and kmers.dtype == np.uint64 else pack(kmers, k)
        packed = np.ascontiguousarray(packed)
        self.n = len(packed)
        try:
            self._call("open", device, k, x, self.n, packed.ctypes.data if self.n else None, C.byref(self._h))
        except RuntimeError:
            self._h = None
            raise

    def _call(self, name, *args):
        rc = getattr(self._lib, self._prefix + "_" + name)(*args)
        if rc:
            raise RuntimeError("%s_%s failed: %d" % (self._prefix, name, rc))

    def submit(self, bases, ends=()):
        """bases: bytes of record text; ends: the offsets (exclusive) at which a record ends inside `bases`"""
        if isinstance(bases, str):
            bases = bases.encode()
        e = np.asarray(ends, dtype=np.uint64)
        buf = np.frombuffer(bases, dtype=np.uint8)
        self._call("submit", self._h, buf.ctypes.data if len(buf) else None, len(buf), e.ctypes.data if len(e) else None, len(e))

    def submit_records(self, records, chunk=None):
        """records: sequences (str / bytes), each one whole record; chunk: submit in pieces of this many bytes"""
        for seq in records:
            if isinstance(seq, str):
                seq = seq.encode()
            if chunk is None:
                self.submit(seq, [len(seq)])
                continue
            for at in range(0, len(seq), chunk):
                piece = seq[at:at + chunk]
                self.submit(piece, [len(piece)] if at + chunk >= len(seq) else [])
            if not seq:
                self.submit(b"", [0])

    def _hit_arrays(self):
        out = [np.zeros(max(self.n, 1), dtype=np.uint8) for _ in range(self._n_hits)]
        self._call("hits", self._h, *[o.ctypes.data for o in out])
        return [o[:self.n] for o in out]

    def hits(self):
        return self._hit_arrays()[0]

    def times(self):
        t = self._stats_type()
        self._call(self._stats, self._h, C.byref(t))
        return t

    def close(self):
        if self._h:
            self._call("close", self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


lib = _declare(C.CDLL(_path), Session)
_gap = None


def gap_lib():
    """libntsm_sitegen_gap_hip.so, loaded on first use"""
    global _gap
    if _gap is None:
        path = os.path.join(_HERE, "libntsm_sitegen_gap_hip.so")
        if not os.path.exists(path):
            raise ImportError("%s is missing: run `make` (there is no CPU fallback)" % path)
        _gap = _declare(C.CDLL(path), GapSession)
    return _gap


class GapSession(Session):
    """One candidate set on one device, substitutions and one-base gaps in one pass (end margin e).  submit() and
    submit_records() as Session has them; hits() returns (min(H, 255), min(G, 255)) per candidate."""
    _prefix, _n_hits, _stats, _stats_type = "ntsm_sitegap", 2, "stats", GapStats
    _library = staticmethod(gap_lib)

    def __init__(self, kmers, k, e=5, device=0):
        super().__init__(kmers, k, e, device)

    def hits(self):
        return tuple(self._hit_arrays())

    def stats(self):
        return self.times()
