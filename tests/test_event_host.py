"""CPU: event search as tests/event_ref.py states it (hand cases), the mi_event_topk entry points
(exported, arguments validated before any HIP call, workspace size), the service's time-order
helper, and the precondition that makes the GPU test on the real rows (test_gpu_events.py) neither
vacuous nor flaky."""
import ctypes
import re

import numpy as np

from conftest import golden
from event_ref import event_ref, event_ref_arrays, real_case

NAN, INF = float("nan"), float("inf")


def _events(scores, tau, **kw):
    recs, total = event_ref(np.asarray(scores, np.float32), tau, **kw)
    assert total == len(recs)
    return [(float(s), pc, b, e, c) for s, pc, b, e, c in recs]


# ------------------------------------------------------------------ the reference, by hand
def test_ref_gap_of_exactly_max_gap_links():
    s = [1, 0, 0, 2, 0, 0, 0, 3]            # hot at 0, 3, 7: distances 3 and 4
    assert _events(s, 0.5, max_gap=3) == [(3.0, 7, 7, 7, 1), (2.0, 3, 0, 3, 2)]
    assert _events(s, 0.5, max_gap=4) == [(3.0, 7, 0, 7, 3)]
    assert _events(s, 0.5, max_gap=2) == [(3.0, 7, 7, 7, 1), (2.0, 3, 3, 3, 1), (1.0, 0, 0, 0, 1)]
    # the same through times: cold columns do not matter, only the hot columns' time distance
    t = [10, 11, 12, 13, 14, 15, 16, 17]
    assert _events(s, 0.5, max_gap=3, times=t) == _events(s, 0.5, max_gap=3)
    t = [0, 5, 5, 5, 9, 9, 9, 9]            # hot times 0, 5, 9
    assert _events(s, 0.5, max_gap=4, times=t) == [(3.0, 7, 3, 7, 2), (1.0, 0, 0, 0, 1)]
    assert _events(s, 0.5, max_gap=5, times=t) == [(3.0, 7, 0, 7, 3)]


def test_ref_null_times_gap_0_and_1():
    s = [1, 1, 0, 1]
    assert _events(s, 1, max_gap=0) == [(1.0, 0, 0, 0, 1), (1.0, 1, 1, 1, 1), (1.0, 3, 3, 3, 1)]
    assert _events(s, 1, max_gap=1) == [(1.0, 0, 0, 1, 2), (1.0, 3, 3, 3, 1)]


def test_ref_equal_times_link_at_gap_0():
    assert _events([1, 2, 3, 4], 0, max_gap=0, times=[7, 7, 7, 8]) == [(4.0, 3, 3, 3, 1), (3.0, 2, 0, 2, 3)]


def test_ref_nan_score_is_cold():
    s = [1, NAN, 1, 1]
    assert _events(s, 0.5, max_gap=1) == [(1.0, 0, 0, 0, 1), (1.0, 2, 2, 3, 2)]
    assert _events(s, 0.5, max_gap=2) == [(1.0, 0, 0, 3, 3)]       # the run goes on over it
    assert _events(s, -INF, max_gap=1) == _events(s, 0.5, max_gap=1)


def test_ref_infinite_and_nan_threshold():
    s = [-INF, 3, NAN, -5]
    assert _events(s, -INF, max_gap=1) == [(3.0, 1, 0, 1, 2), (-5.0, 3, 3, 3, 1)]
    assert _events(s, NAN, max_gap=1) == []
    assert _events(s, INF, max_gap=1) == []


def test_ref_min_count_and_total():
    s = [1, 1, 0, 0, 2, 0, 0, 1, 1, 1]
    assert _events(s, 1, max_gap=1) == [(2.0, 4, 4, 4, 1), (1.0, 0, 0, 1, 2), (1.0, 7, 7, 9, 3)]
    assert _events(s, 1, max_gap=1, min_count=2) == [(1.0, 0, 0, 1, 2), (1.0, 7, 7, 9, 3)]
    out = event_ref_arrays(np.asarray([s], np.float32), 1, k=1, max_gap=1, min_count=2, index_base=100)
    assert [a.tolist() for a in out] == [[[1.0]], [[100]], [[100]], [[101]], [[2]], [2]]   # total whatever k
    out = event_ref_arrays(np.asarray([s], np.float32), 1, k=3, max_gap=1, min_count=3)
    assert out[0].tolist() == [[1.0, -INF, -INF]] and out[2].tolist() == [[7, -1, -1]]
    assert out[4].tolist() == [[3, 0, 0]] and out[5].tolist() == [1]


def test_ref_peak_tie_takes_lowest_column_and_equal_peaks_order_by_begin():
    s = [1, 5, 5, 0, 0, 5, 2]
    assert _events(s, 1, max_gap=1) == [(5.0, 1, 0, 2, 3), (5.0, 5, 5, 6, 2)]


def test_ref_mask_and_range():
    s = [1, 1, 1, 1, 1, 1]
    m = np.array([1, 1, 0, 1, 1, 1], bool)
    assert _events(s, 1, max_gap=1, mask=m) == [(1.0, 0, 0, 1, 2), (1.0, 3, 3, 5, 3)]
    assert _events(s, 1, max_gap=2, mask=m) == [(1.0, 0, 0, 5, 5)]
    assert _events(s, 1, max_gap=1, rng=(-3, 2)) == [(1.0, 0, 0, 1, 2)]
    assert _events(s, 1, max_gap=1, rng=(4, 99)) == [(1.0, 4, 4, 5, 2)]
    assert _events(s, 1, max_gap=1, rng=(4, 4)) == []


# ------------------------------------------------------------------ the C entry points
def _lib():
    from miclip import _native
    return _native.lib()


def test_symbols_exported():
    from miclip import _native
    L = _lib()
    out = __import__("os").popen(f"nm -D --defined-only {_native.LIB_PATH}").read()
    for name in ("mi_event_topk", "mi_event_workspace_bytes"):
        assert name in _native.EXPORTS and hasattr(L, name)
        assert re.search(rf"\bT {name}$", out, re.M), f"{name} not exported"
    assert re.search(r"\bT mi_debug_event_block_cols$", out, re.M) and "mi_debug_event_block_cols" not in _native.EXPORTS
    assert L.mi_abi_version() == 7


ONE = ctypes.c_void_p(64)   # a non-null pointer that no argument check dereferences


def _call(L, scores=ONE, N=10, Q=2, thr=ONE, max_gap=0, min_count=1, k=10, outs=(ONE,) * 6, ws=None, nbytes=0):
    return L.mi_event_topk(scores, N, Q, thr, None, None, None, max_gap, min_count, k, 0, *outs, ws, nbytes, None)


def test_argument_errors_without_gpu():
    L = _lib()
    for k in (0, 65, -1):
        assert _call(L, k=k) == -1 and b"k must be in [1, 64]" in L.mi_last_error()
    assert _call(L, N=-1) == -1 and b"negative size" in L.mi_last_error()
    assert _call(L, Q=-1) == -1 and b"negative size" in L.mi_last_error()
    assert _call(L, max_gap=-1) == -1 and b"max_gap" in L.mi_last_error()
    for m in (0, -5):
        assert _call(L, min_count=m) == -1 and b"min_count" in L.mi_last_error()
    for kw in (dict(scores=None), dict(thr=None)) + tuple(
            dict(outs=tuple(None if j == i else ONE for j in range(6))) for i in range(6)):
        assert _call(L, **kw) == -1 and b"null pointer" in L.mi_last_error(), kw
    need = L.mi_event_workspace_bytes(10, 2, 10)
    assert need >= 128
    assert _call(L) == -1 and b"workspace too small" in L.mi_last_error()
    buf = ctypes.create_string_buffer(need)
    assert _call(L, ws=ctypes.cast(buf, ctypes.c_void_p), nbytes=need - 1) == -1 and \
        b"workspace too small" in L.mi_last_error()
    assert _call(L, Q=0) == 0 and _call(L, Q=0, N=0, scores=None) == 0           # nothing to do
    assert _call(L, N=1 << 31) == -3


def test_workspace_positive_and_monotone():
    f = _lib().mi_event_workspace_bytes
    assert f(10, 1, 0) == 0 and f(10, 1, 65) == 0 and f(-1, 1, 10) == 0 and f(10, -1, 10) == 0
    Ns = [0, 1, 255, 256, 257, 20_011, 262_144, 262_145, 300_000, 1_000_000, 5_000_000, 100_000_000]
    for Q in (1, 32):
        v = [f(n, Q, 10) for n in Ns]
        assert v[0] > 0 and all(a <= b for a, b in zip(v, v[1:])), v
    for n in Ns:
        v = [f(n, Q, 10) for Q in (0, 1, 2, 33, 1000)]
        assert v[0] > 0 and all(a <= b for a, b in zip(v, v[1:])), v
        assert f(n, 4, 64) >= f(n, 4, 1)


def test_block_cols_covers_the_columns_with_a_bounded_grid():
    f = _lib().mi_debug_event_block_cols
    for n in (1, 255, 256, 257, 20_011, 262_144, 262_145, 1_000_000, 100_000_000, (1 << 31) - 1):
        bc = f(n)
        assert bc >= 256 and bc % 256 == 0 and (n + bc - 1) // bc <= 1024, (n, bc)
    assert f(1_000_000) == 1024            # Q = 1 at 1M columns: 977 workgroups


# ------------------------------------------------------------------ the time-order helper
def test_frame_time_order():
    from miclip.service import frame_time_order
    names = sorted(["2214.jpg", "4599.jpg", "6704.jpg", "10152.jpg", "100.jpg"])     # string order
    assert names[0] == "100.jpg" and names[1] == "10152.jpg"
    times, order = frame_time_order(names)
    assert times.tolist() == [100, 10152, 2214, 4599, 6704] and order.tolist() == [0, 2, 3, 4, 1]
    times, order = frame_time_order(["frames/vid/0012.png", "frames/vid/0003.png"])  # paths, leading zeros
    assert times.tolist() == [12, 3] and order.tolist() == [1, 0]
    for bad in (["1.jpg", "broken.png", "3.jpg"], ["1.jpg", "-2.jpg"], ["1.5.jpg"], [" 7.jpg"]):
        times, order = frame_time_order(bad)
        assert times is None and order.tolist() == list(range(len(bad)))
    times, order = frame_time_order(["5.jpg", "3.jpg", "5.png", "3.png"])             # duplicates: stable
    assert times.tolist() == [5, 3, 5, 3] and order.tolist() == [1, 3, 0, 2]
    times, order = frame_time_order([])
    assert times.shape == (0,) and order.shape == (0,)


# ------------------------------------------------------------------ the real rows
def test_real_rows_thresholds_have_margin_and_few_events():
    """Every row of the fixture corpus as a query (the rows are consecutive keyframes of one
    video): the threshold sits in a score gap far wider than the kernels' score error (8e-6), so
    the GPU's hot set is the float64 one, and no query has more than 64 events at max_gap = 2."""
    rows = golden("rank_video_test_4.npz")["corpus"]
    assert rows.shape[0] == 387
    s, tau, half = real_case(rows)
    print(f"smallest half-gap {half.min():.3e}")
    assert half.min() >= 5e-4, half.min()
    hot = (s >= tau[:, None]).sum(axis=1)
    assert hot.min() >= 21 and hot.max() <= 60
    assert ((s.astype(np.float32) >= tau.astype(np.float32)[:, None]) == (s >= tau[:, None])).all()
    totals = [event_ref(s[i], tau[i], max_gap=2)[1] for i in range(len(s))]
    print(f"events per query {min(totals)} .. {max(totals)}")
    assert 2 <= min(totals) and max(totals) <= 64, (min(totals), max(totals))
