"""ctypes plumbing for include/ntsm_vcf_hip.h (the device step of ntsmVCF); used by tests and tools.
Loaded on demand: `import ntsm_amd.vcf`.  Fails loudly when libntsm_vcf_hip.so has not been built."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_path = os.path.join(_HERE, "libntsm_vcf_hip.so")
if not os.path.exists(_path):
    raise ImportError("%s is missing: run `make` (there is no CPU fallback)" % _path)
lib = C.CDLL(_path)

HOM1, HET, HOM2, PAD = 0, 1, 2, 3
E_CAPACITY = -3
WARNING = np.dtype([("event", "<u4"), ("sample", "<u4"), ("old", "<u4"), ("value", "<u4")])


class Times(C.Structure):
    _fields_ = [("upload_ms", C.c_double), ("state_kernel_ms", C.c_double), ("sum_kernel_ms", C.c_double),
                ("download_ms", C.c_double), ("kernel_bytes", C.c_uint64), ("state_launches", C.c_uint64)]


lib.ntsm_vcf_run.restype = C.c_int
lib.ntsm_vcf_run.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32,
                             C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                             C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                             C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(Times)]


def run(geno, multi, key_events, site_ref, site_var, device=0, warn_cap=1 << 16):
    """The device step on its own.

    geno:       uint8 [n_lines][n_samples], codes HOM1 / HET / HOM2 (any other byte: no insert)
    key_events: per key, a list of events (ordinal, line, side) in ascending ordinal
    site_ref, site_var: per site, the list of its REF / VAR key indices
    Returns (cells uint16 [n_sites][n_samples] = maxREF | maxVAR << 8, sums float64 [n_sites], first_undef uint32
    [n_sites], warnings sorted by (event, sample), Times)."""
    geno = np.asarray(geno, dtype=np.uint8)
    n_lines, n = geno.shape
    stride = (n + 15) // 16 * 16
    g = np.full((max(n_lines, 1), max(stride, 16)), PAD, dtype=np.uint8)
    g[:n_lines, :n] = geno
    key_off = np.zeros(len(key_events) + 1, dtype=np.uint64)
    key_off[1:] = np.cumsum([len(e) for e in key_events])
    flat = [ev for evs in key_events for ev in evs]
    ev_ord = np.array([e[0] for e in flat], dtype=np.uint32)
    ev_ls = np.array([e[1] * 2 + e[2] for e in flat], dtype=np.uint32)
    site_off = np.zeros(2 * len(site_ref) + 1, dtype=np.uint64)
    keys = []
    for s in range(len(site_ref)):
        keys += list(site_ref[s])
        site_off[2 * s + 1] = len(keys)
        keys += list(site_var[s])
        site_off[2 * s + 2] = len(keys)
    site_keys = np.array(keys + [0], dtype=np.uint32)
    m = len(site_ref)
    cells = np.zeros((m, n), dtype=np.uint16)
    sums = np.zeros(m, dtype=np.float64)
    first = np.zeros(m, dtype=np.uint32)
    n_warn = C.c_uint64()
    times = Times()
    ev_ord_p = ev_ord.ctypes.data if len(flat) else None
    ev_ls_p = ev_ls.ctypes.data if len(flat) else None
    while True:
        warn = np.zeros(max(warn_cap, 1), dtype=WARNING)
        rc = lib.ntsm_vcf_run(device, n, multi, n_lines, g.ctypes.data, stride if n else 16, len(key_events), key_off.ctypes.data,
                              len(flat), ev_ord_p, ev_ls_p, m, site_off.ctypes.data, site_keys.ctypes.data,
                              cells.ctypes.data, sums.ctypes.data, first.ctypes.data, warn.ctypes.data, warn.shape[0],
                              C.byref(n_warn), C.byref(times))
        if rc == E_CAPACITY:
            warn_cap = n_warn.value
            continue
        if rc:
            raise RuntimeError("ntsm_vcf_run failed: %d" % rc)
        break
    warn = np.sort(warn[:n_warn.value], order=["event", "sample"])
    return cells, sums, first, warn, times


class RecordsTimes(C.Structure):
    _fields_ = [("upload_ms", C.c_double), ("kernel_ms", C.c_double), ("download_ms", C.c_double),
                ("kernel_bytes", C.c_uint64), ("upload_bytes", C.c_uint64), ("download_bytes", C.c_uint64)]


lib.ntsm_vcf_records.restype = C.c_int
lib.ntsm_vcf_records.argtypes = [C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32,
                                 C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                 C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32,
                                 C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(RecordsTimes)]

FILL = 0xA5   # records() fills its row buffers with this byte first: what the library does not write keeps it


def _lists(geno, key_events, site_ref, site_var):
    """The host arrays of include/ntsm_vcf_hip.h from Python lists (as run() builds them)."""
    geno = np.asarray(geno, dtype=np.uint8)
    n_lines, n = geno.shape
    stride = (n + 15) // 16 * 16
    g = np.full((max(n_lines, 1), max(stride, 16)), PAD, dtype=np.uint8)
    g[:n_lines, :n] = geno
    key_off = np.zeros(len(key_events) + 1, dtype=np.uint64)
    key_off[1:] = np.cumsum([len(e) for e in key_events])
    flat = [ev for evs in key_events for ev in evs]
    ev_ord = np.array([e[0] for e in flat] + [0], dtype=np.uint32)
    ev_ls = np.array([e[1] * 2 + e[2] for e in flat] + [0], dtype=np.uint32)
    site_off = np.zeros(2 * len(site_ref) + 1, dtype=np.uint64)
    keys = []
    for s in range(len(site_ref)):
        keys += list(site_ref[s])
        site_off[2 * s + 1] = len(keys)
        keys += list(site_var[s])
        site_off[2 * s + 2] = len(keys)
    site_keys = np.array(keys + [0], dtype=np.uint32)
    return g, max(stride, 16), key_off, len(flat), ev_ord, ev_ls, site_off, site_keys


class Records:
    """What records() returns.  counts / sums: uint32 [s_count][n_sites][2] views into raw_counts / raw_sums, the uint8
    [s_count][pitch] buffers the library wrote into (filled with FILL before the call); sums and raw_sums are None without
    want_sums.  total, sum_of_sums: uint64 [s_count].  times: RecordsTimes."""
    def __init__(self, counts, sums, total, sum_of_sums, times, raw_counts, raw_sums):
        self.counts, self.sums, self.total, self.sum_of_sums, self.times = counts, sums, total, sum_of_sums, times
        self.raw_counts, self.raw_sums = raw_counts, raw_sums


def records(geno, multi, key_events, site_ref, site_var, s_begin=0, s_count=None, pitch=None, want_sums=True, device=0):
    """The counts records of the samples [s_begin, s_begin + s_count) (ntsm_vcf_records); the lists as for run().
    s_count None: up to the last sample.  pitch: bytes between two samples' rows, for counts and sums alike (None:
    8 * n_sites, no gap)."""
    g, stride, key_off, n_ev, ev_ord, ev_ls, site_off, site_keys = _lists(geno, key_events, site_ref, site_var)
    n_lines, n = np.asarray(geno).shape
    m = len(site_ref)
    if s_count is None:
        s_count = n - s_begin
    if pitch is None:
        pitch = 8 * m
    rows = max(int(s_count), 0)
    raw_counts = np.full((rows, pitch), FILL, dtype=np.uint8)
    raw_sums = np.full((rows, pitch), FILL, dtype=np.uint8) if want_sums else None
    total = np.zeros(rows, dtype=np.uint64)
    sos = np.zeros(rows, dtype=np.uint64)
    times = RecordsTimes()
    rc = lib.ntsm_vcf_records(device, n, multi, n_lines, g.ctypes.data, stride, len(key_events), key_off.ctypes.data,
                              n_ev, ev_ord.ctypes.data, ev_ls.ctypes.data, m, site_off.ctypes.data, site_keys.ctypes.data,
                              s_begin, s_count, raw_counts.ctypes.data, pitch, raw_sums.ctypes.data if want_sums else None, pitch,
                              total.ctypes.data, sos.ctypes.data, C.byref(times))
    if rc:
        raise RuntimeError("ntsm_vcf_records failed: %d" % rc)

    def view(raw):
        return np.ascontiguousarray(raw[:, :8 * m]).view("<u4").reshape(rows, m, 2)
    return Records(view(raw_counts), view(raw_sums) if want_sums else None, total, sos, times, raw_counts, raw_sums)
