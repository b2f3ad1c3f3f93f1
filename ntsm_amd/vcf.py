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
