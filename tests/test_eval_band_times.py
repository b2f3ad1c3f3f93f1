"""What the band sessions of ntsmEval report in ntsm_eval_cross_times (include/ntsm_eval_hip.h: ntsm_eval_within_open,
ntsm_eval_between_open, ntsm_eval_contam_open and their _rows): which call of a session carries the upload and the preparation,
and what `chunks` counts.  The records themselves are test_eval_within.py's, test_eval_between.py's and test_eval_contam.py's.

One store of 130 samples x 65 sites, counts 0 ... 40.  Resident (chunk 0): the open's times arrive with the first _rows call and
with no later one, chunks stays 0.  Streamed (chunk 64): every call uploads, and chunks is the columns it walked over 64, rounded
up.  The open times are the session's: a session closed without a _rows call hands nothing to the next one.
No comparison of two wall-clock figures with each other: only zero against not zero."""
import numpy as np
import pytest

N, M, CHUNK = 130, 65, 64
BANDS = [(0, 64), (64, 66)]
KINDS = ["within", "between", "contam"]
_store = []


def store():
    if not _store:
        db = np.random.default_rng(130065).integers(0, 41, size=(N, M, 2)).astype(np.uint32)
        db.setflags(write=False)
        _store.append(db)
    return _store[0]


def session(kind, chunk):
    import ntsm_amd.eval as ev
    if kind == "within":
        return ev.Within(store(), db_chunk=chunk)
    if kind == "between":
        return ev.Between(store(), store(), b_chunk=chunk)
    return ev.Contam(store(), db_chunk=chunk)


def times_of(s, first, rows):
    return s.rows(first, rows)[-1]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_resident_first_call_reports_the_open(kind):
    with session(kind, 0) as s:
        t0 = times_of(s, *BANDS[0])
        t1 = times_of(s, *BANDS[1])
    print(kind, [(t.upload_ms, t.prepare_kernel_ms, t.cross_kernel_ms, t.download_ms, t.chunks) for t in (t0, t1)])
    assert t0.upload_ms > 0 and t0.chunks == 0, kind
    assert t1.chunks == 0, kind
    if kind != "between":                                                                   # between stages its band's rows in every call
        assert t1.upload_ms == 0 and t1.prepare_kernel_ms == 0, kind


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_streamed_every_call_uploads_and_counts_its_chunks(kind):
    with session(kind, CHUNK) as s:
        for first, rows in BANDS:
            t = times_of(s, first, rows)
            columns = N - first if kind == "within" else N
            print(kind, first, rows, t.upload_ms, t.prepare_kernel_ms, t.cross_kernel_ms, t.download_ms, t.chunks)
            assert t.upload_ms > 0, (kind, first)
            assert t.chunks == -(-columns // CHUNK), (kind, first, t.chunks)
    assert -(-N // CHUNK) == 3


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_open_times_belong_to_the_session(kind):
    """A session closed without a _rows call, one opened before it and one after it: each of the other two reports an open in its
    first call, and (within, contam) none in its second"""
    before = session(kind, 0)
    session(kind, 0).close()
    after = session(kind, 0)
    try:
        for s in (after, before):
            t0 = times_of(s, *BANDS[0])
            t1 = times_of(s, *BANDS[1])
            print(kind, t0.upload_ms, t0.prepare_kernel_ms, t1.upload_ms, t1.prepare_kernel_ms)
            assert t0.upload_ms > 0 and t0.prepare_kernel_ms > 0 and t0.chunks == 0, kind
            if kind != "between":
                assert t1.upload_ms == 0 and t1.prepare_kernel_ms == 0, kind
    finally:
        before.close()
        after.close()
