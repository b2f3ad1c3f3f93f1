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
lib = C.CDLL(_path)


class Times(C.Structure):
    _fields_ = [("table_build_ms", C.c_double), ("table_upload_ms", C.c_double), ("stage_ms", C.c_double), ("upload_ms", C.c_double),
                ("kernel_ms", C.c_double), ("full_kernel_ms_min", C.c_double), ("full_kernel_ms_max", C.c_double),
                ("launches", C.c_uint64), ("full_launches", C.c_uint64), ("windows", C.c_uint64), ("bitmap_tests", C.c_uint64),
                ("probes", C.c_uint64), ("genome_bytes", C.c_uint64), ("table_bytes", C.c_uint64)]


lib.ntsm_sitegen_open.restype = C.c_int
lib.ntsm_sitegen_open.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)]
lib.ntsm_sitegen_submit.restype = C.c_int
lib.ntsm_sitegen_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
lib.ntsm_sitegen_hits.restype = C.c_int
lib.ntsm_sitegen_hits.argtypes = [C.c_void_p, C.c_void_p]
lib.ntsm_sitegen_times_get.restype = C.c_int
lib.ntsm_sitegen_times_get.argtypes = [C.c_void_p, C.POINTER(Times)]
lib.ntsm_sitegen_close.restype = None
lib.ntsm_sitegen_close.argtypes = [C.c_void_p]

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

    def __init__(self, kmers, k, x=1, device=0):
        self._h = C.c_void_p()
        packed = kmers if isinstance(kmers, np.ndarray) and kmers.dtype == np.uint64 else pack(kmers, k)
        packed = np.ascontiguousarray(packed)
        self.n = len(packed)
        rc = lib.ntsm_sitegen_open(device, k, x, self.n, packed.ctypes.data if self.n else None, C.byref(self._h))
        if rc:
            self._h = None
            raise RuntimeError("ntsm_sitegen_open failed: %d" % rc)

    def submit(self, bases, ends=()):
        """bases: bytes of record text; ends: the offsets (exclusive) at which a record ends inside `bases`"""
        if isinstance(bases, str):
            bases = bases.encode()
        e = np.asarray(ends, dtype=np.uint64)
        buf = np.frombuffer(bases, dtype=np.uint8)
        rc = lib.ntsm_sitegen_submit(self._h, buf.ctypes.data if len(buf) else None, len(buf), e.ctypes.data if len(e) else None, len(e))
        if rc:
            raise RuntimeError("ntsm_sitegen_submit failed: %d" % rc)

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

    def hits(self):
        out = np.zeros(max(self.n, 1), dtype=np.uint8)
        rc = lib.ntsm_sitegen_hits(self._h, out.ctypes.data)
        if rc:
            raise RuntimeError("ntsm_sitegen_hits failed: %d" % rc)
        return out[:self.n]

    def times(self):
        t = Times()
        rc = lib.ntsm_sitegen_times_get(self._h, C.byref(t))
        if rc:
            raise RuntimeError("ntsm_sitegen_times_get failed: %d" % rc)
        return t

    def close(self):
        if self._h:
            lib.ntsm_sitegen_close(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class GapStats(C.Structure):
    _fields_ = [("table_build_ms", C.c_double), ("table_upload_ms", C.c_double), ("stage_ms", C.c_double), ("upload_ms", C.c_double),
                ("kernel_ms", C.c_double), ("full_kernel_ms_min", C.c_double), ("full_kernel_ms_max", C.c_double),
                ("launches", C.c_uint64), ("full_launches", C.c_uint64), ("windows", C.c_uint64), ("windows_long", C.c_uint64),
                ("windows_short", C.c_uint64), ("bitmap_tests", C.c_uint64), ("probes", C.c_uint64), ("genome_bytes", C.c_uint64),
                ("table_bytes", C.c_uint64)]


_gap = None


def gap_lib():
    """libntsm_sitegen_gap_hip.so, loaded on first use"""
    global _gap
    if _gap is None:
        path = os.path.join(_HERE, "libntsm_sitegen_gap_hip.so")
        if not os.path.exists(path):
            raise ImportError("%s is missing: run `make` (there is no CPU fallback)" % path)
        g = C.CDLL(path)
        g.ntsm_sitegap_open.restype = C.c_int
        g.ntsm_sitegap_open.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.POINTER(C.c_void_p)]
        g.ntsm_sitegap_submit.restype = C.c_int
        g.ntsm_sitegap_submit.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
        g.ntsm_sitegap_hits.restype = C.c_int
        g.ntsm_sitegap_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        g.ntsm_sitegap_stats.restype = C.c_int
        g.ntsm_sitegap_stats.argtypes = [C.c_void_p, C.POINTER(GapStats)]
        g.ntsm_sitegap_close.restype = None
        g.ntsm_sitegap_close.argtypes = [C.c_void_p]
        _gap = g
    return _gap


class GapSession(Session):
    """One candidate set on one device, substitutions and one-base gaps in one pass (end margin e).  submit() and
    submit_records() as Session has them; hits() returns (min(H, 255), min(G, 255)) per candidate."""

    def __init__(self, kmers, k, e=5, device=0):
        self._lib = gap_lib()
        self._h = C.c_void_p()
        packed = kmers if isinstance(kmers, np.ndarray) and kmers.dtype == np.uint64 else pack(kmers, k)
        packed = np.ascontiguousarray(packed)
        self.n = len(packed)
        rc = self._lib.ntsm_sitegap_open(device, k, e, self.n, packed.ctypes.data if self.n else None, C.byref(self._h))
        if rc:
            self._h = None
            raise RuntimeError("ntsm_sitegap_open failed: %d" % rc)

    def submit(self, bases, ends=()):
        if isinstance(bases, str):
            bases = bases.encode()
        e = np.asarray(ends, dtype=np.uint64)
        buf = np.frombuffer(bases, dtype=np.uint8)
        rc = self._lib.ntsm_sitegap_submit(self._h, buf.ctypes.data if len(buf) else None, len(buf), e.ctypes.data if len(e) else None, len(e))
        if rc:
            raise RuntimeError("ntsm_sitegap_submit failed: %d" % rc)

    def hits(self):
        sub, gap = np.zeros(max(self.n, 1), dtype=np.uint8), np.zeros(max(self.n, 1), dtype=np.uint8)
        rc = self._lib.ntsm_sitegap_hits(self._h, sub.ctypes.data, gap.ctypes.data)
        if rc:
            raise RuntimeError("ntsm_sitegap_hits failed: %d" % rc)
        return sub[:self.n], gap[:self.n]

    def stats(self):
        st = GapStats()
        rc = self._lib.ntsm_sitegap_stats(self._h, C.byref(st))
        if rc:
            raise RuntimeError("ntsm_sitegap_stats failed: %d" % rc)
        return st

    def times(self):
        return self.stats()

    def close(self):
        if self._h:
            self._lib.ntsm_sitegap_close(self._h)
            self._h = None
