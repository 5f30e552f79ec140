"""GPU: mi_event_topk (csrc/rank_events.hip), the top-k temporal runs of matching frames, and the
layers on it (retrieval.event_topk / rank_events, FrameLibrary.search_events, the service), against
tests/event_ref.py (a serial NumPy loop).  On hand-fed scores the result is exact: every output
array and the total are compared with assert_array_equal, scores as bits.  Through a corpus the
reference runs on the GPU's own score matrix read back (exact again); on the real rows against
float64 scores, with the threshold margin tests/test_event_host.py asserts."""
import json

import numpy as np
import pytest

from conftest import golden
from event_ref import event_ref, event_ref_arrays, real_case
from test_gpu_service import Cache, Data, Paths, _tokens

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    """The six outputs of event_topk (device) against event_ref_arrays' (host)."""
    import torch
    s, p, b, e, c, t = got
    assert s.dtype == torch.float32 and p.dtype == b.dtype == e.dtype == torch.int64
    assert c.dtype == t.dtype == torch.int32
    got = [x.cpu().numpy() for x in got]
    for name, g, w in zip(("total", "begin", "end", "count", "peak"), [got[5], got[2], got[3], got[4], got[1]],
                          [want[5], want[2], want[3], want[4], want[1]]):
        np.testing.assert_array_equal(g, w, err_msg=name)
    np.testing.assert_array_equal(_bits(got[0]), _bits(want[0]), err_msg="score bits")


def _check(gpu, scores, tau, k, max_gap=0, min_count=1, times=None, mask=None, how="bool", rng=None, base=0):
    """event_topk on host float32 scores [Q, N] against the reference; how: the mask goes in as a
    bool tensor or as packed words."""
    import torch
    from miclip import retrieval
    scores = np.ascontiguousarray(scores, np.float32)
    row_mask = None
    if mask is not None:
        row_mask = torch.from_numpy(np.asarray(mask, bool)).to(gpu)
        if how == "packed":
            row_mask = retrieval.pack_row_mask(row_mask)
    got = retrieval.event_topk(torch.from_numpy(scores).to(gpu), tau, k, max_gap=max_gap, min_count=min_count,
                               row_time=None if times is None else np.asarray(times, np.int64), row_mask=row_mask,
                               query_range=rng if rng is None or isinstance(rng, tuple) else torch.from_numpy(rng),
                               index_base=base)
    want = event_ref_arrays(scores, tau, k, max_gap, min_count, times, mask, rng, base)
    _same(got, want)
    return want


def _block(n):
    from miclip import retrieval
    return retrieval.event_block_cols(n)


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("Q", [1, 33])
@pytest.mark.parametrize("N", [1, 31, 33, 64, 65, 4097, 20_011])
def test_shapes_densities_gaps(gpu, N, Q):
    """Seeded random scores at hot densities 0.01 / 0.5 / 0.99, NULL times at max_gap 0 / 1 / 3,
    k = 1 / 10 / 64 (the largest shape runs one k and gap per density: the reference is a loop)."""
    rng = np.random.default_rng(1000 * N + Q)
    scores = rng.random((Q, N), dtype=np.float32)
    combos = [(d, g) for d in (0.01, 0.5, 0.99) for g in (0, 1, 3)]
    if N * Q > 200_000:
        combos = [(0.01, 3), (0.5, 1), (0.99, 0)]
    for j, (density, gap) in enumerate(combos):
        k = (1, 10, 64)[(j + j // 3) % 3]
        want = _check(gpu, scores, np.float32(1.0 - density), k, max_gap=gap)
        if N >= 4097 and density == 0.5:
            assert want[5].min() > 64 or gap == 3      # more events than any k: the totals count them all


def test_empty_corpus_and_no_queries(gpu):
    import torch
    from miclip import retrieval
    _check(gpu, np.zeros((3, 0), np.float32), 0.5, 4)
    out = retrieval.event_topk(torch.zeros((0, 10), device=gpu), 0.5, 4)
    assert [tuple(o.shape) for o in out] == [(0, 4)] * 5 + [(0,)]


# ------------------------------------------------------------------ 2. several workgroups per query
def _multi_n():
    n = 4 * 256 + 37
    bc = _block(n)
    assert (n + bc - 1) // bc >= 4, (n, bc)          # at least four workgroups cover a query
    return n, bc


@pytest.mark.parametrize("density", [0.01, 0.5, 0.99])
def test_four_workgroups_random_times_with_duplicates(gpu, density):
    n, _ = _multi_n()
    rng = np.random.default_rng(int(density * 100))
    scores = rng.random((33, n), dtype=np.float32)
    times = np.cumsum(rng.integers(0, 4, n)) + 5_000_000_000     # steps 0 .. 3: duplicates; beyond int32
    for gap, k, min_count in ((0, 64, 1), (1, 10, 1), (2, 10, 3), (3, 1, 1), (1 << 62, 10, 1)):
        _check(gpu, scores, np.float32(1.0 - density), k, max_gap=gap, min_count=min_count, times=times)
    _check(gpu, scores, np.float32(1.0 - density), 10, max_gap=1)


def test_all_hot_none_hot_alternating(gpu):
    for n in (_multi_n()[0], 20_011):
        ones = np.ones((2, n), np.float32)
        ones[1, n // 3] = 2.0
        want = _check(gpu, ones, 1.0, 10, max_gap=1)
        assert want[5].tolist() == [1, 1] and want[4][:, 0].tolist() == [n, n]       # one event of N columns
        assert want[2][:, 0].tolist() == [0, 0] and want[3][:, 0].tolist() == [n - 1, n - 1]
        assert want[1][:, 0].tolist() == [0, n // 3]
        want = _check(gpu, ones, 3.0, 10, max_gap=1)
        assert want[5].tolist() == [0, 0] and (want[2] == -1).all() and np.isneginf(want[0]).all()
        alt = np.zeros((1, n), np.float32)
        alt[0, ::2] = 1.0 + np.arange((n + 1) // 2, dtype=np.float32) % 7
        want = _check(gpu, alt, 1.0, 64, max_gap=0)
        assert want[5].tolist() == [(n + 1) // 2]                                    # N/2 events
        _check(gpu, alt, 1.0, 64, max_gap=1)
        want = _check(gpu, alt, 1.0, 64, max_gap=2)
        assert want[5].tolist() == [1]


def test_events_on_workgroup_boundaries(gpu):
    n, bc = _multi_n()
    s = np.zeros((6, n), np.float32)
    s[0, bc - 1:bc + 1] = (2, 3)                     # begins on a workgroup's last column, ends on the next's first
    s[1, bc - 3:3 * bc + 6] = 1                      # covers two whole workgroups and more
    s[1, 2 * bc + 9] = 4                             # ... its peak two workgroups after its begin
    s[2, [5, bc - 1, bc, 2 * bc, n - 1]] = (1, 2, 3, 4, 5)
    s[3, bc - 2], s[3, 3 * bc + 1] = 7, 6            # one link over two cold workgroups
    s[4, :] = 1                                      # every workgroup inside one event
    s[4, n - 1] = 9
    s[5, 0], s[5, n - 1] = 1, 1
    want = _check(gpu, s, 0.5, 10, max_gap=1)
    assert (want[2][0, 0], want[3][0, 0], want[4][0, 0], want[1][0, 0]) == (bc - 1, bc, 2, bc)
    assert (want[2][1, 0], want[3][1, 0], want[4][1, 0], want[1][1, 0]) == (bc - 3, 3 * bc + 5, 2 * bc + 9, 2 * bc + 9)
    assert want[5].tolist() == [1, 1, 4, 2, 1, 2]
    assert (want[4][4, 0], want[1][4, 0]) == (n, n - 1)
    # a link across a workgroup boundary at exactly max_gap, no link at max_gap + 1
    gap = 2 * bc + 3
    want = _check(gpu, s[3:4], 0.5, 10, max_gap=gap)
    assert want[5].tolist() == [1] and (want[2][0, 0], want[3][0, 0], want[1][0, 0]) == (bc - 2, 3 * bc + 1, bc - 2)
    want = _check(gpu, s[3:4], 0.5, 10, max_gap=gap - 1)
    assert want[5].tolist() == [2]
    times = np.arange(n, dtype=np.int64) * 10
    times[bc:] += 7                                  # columns bc - 1 and bc are 17 apart
    for g, total in ((17, 1), (16, 2)):
        want = _check(gpu, s[0:1], 0.5, 10, max_gap=g, times=times)
        assert want[5].tolist() == [total]
    _check(gpu, s, 0.5, 10, max_gap=10, times=times)
    _check(gpu, s, 0.5, 3, max_gap=0, min_count=2)


# ------------------------------------------------------------------ 3. NaN, thresholds, mask, range, options
def test_nan_scores_and_per_query_thresholds(gpu):
    n, _ = _multi_n()
    rng = np.random.default_rng(7)
    scores = rng.standard_normal((6, n)).astype(np.float32)
    scores[:, rng.integers(0, n, 150)] = NAN
    scores[1, rng.integers(0, n, 40)] = -INF
    scores[2, rng.integers(0, n, 40)] = INF
    tau = np.array([0.3, -INF, INF, NAN, -0.5, 2.0], np.float32)
    for gap in (0, 1, 3):
        want = _check(gpu, scores, tau, 64, max_gap=gap)
        assert want[5][3] == 0 and want[5][1] > 0 and want[5][2] > 0
    want = _check(gpu, scores, tau, 64, max_gap=n)
    assert want[5].tolist() == [1, 1, 1, 0, 1, 1]
    assert want[4][1, 0] == int((~np.isnan(scores[1])).sum())                        # tau = -inf: every non-NaN column


@pytest.mark.parametrize("how", ["bool", "packed"])
def test_mask_and_range(gpu, how):
    n, bc = _multi_n()
    rng = np.random.default_rng(11)
    scores = rng.random((5, n), dtype=np.float32)
    mask = rng.random(n) < 0.7
    mask[bc - 40:bc + 40] = False                    # more than a word of invisible columns at a boundary
    ranges = np.array([[0, n], [-5, 300], [bc - 1, n + 100], [400, 400], [n - 1, n]], np.int64)
    for gap in (1, 3, 100):
        _check(gpu, scores, 0.5, 10, max_gap=gap, mask=mask, how=how)
        _check(gpu, scores, 0.5, 10, max_gap=gap, mask=mask, how=how, rng=ranges)
        _check(gpu, scores, 0.5, 10, max_gap=gap, rng=ranges)
        _check(gpu, scores, 0.5, 10, max_gap=gap, rng=(bc - 1, 2 * bc + 1))          # one pair for all queries
    want = _check(gpu, scores, 0.5, 10, max_gap=1, mask=np.zeros(n, bool), how=how)
    assert want[5].tolist() == [0] * 5
    want = _check(gpu, scores, 0.0, 10, max_gap=1, rng=ranges)
    assert want[5][3] == 0 and want[5][4] == 1


def test_index_base_min_count_short_lists_equal_peaks(gpu):
    n, _ = _multi_n()
    rng = np.random.default_rng(13)
    scores = (rng.integers(0, 4, (4, n)) * 0.25).astype(np.float32)                 # four score values: equal peaks
    for min_count in (1, 3):
        want = _check(gpu, scores, 0.5, 64, max_gap=1, min_count=min_count, base=1 << 33)
        assert want[2][0, 0] >= 1 << 33 and len(set(_bits(want[0][0, :20]).tolist())) <= 2
    sparse = np.zeros((2, n), np.float32)
    sparse[0, [3, 500, 501, 900]] = (1, 2, 2, 1)
    want = _check(gpu, sparse, 0.5, 64, max_gap=1, base=1 << 33)                     # k above the number of events
    assert want[5].tolist() == [3, 0] and (want[2][0, 3:] == -1).all() and (want[4][0, 3:] == 0).all()
    assert want[2][0, :3].tolist() == [(1 << 33) + 500, (1 << 33) + 3, (1 << 33) + 900]


def test_python_layer_checks(gpu):
    import torch
    from miclip import _native, retrieval
    s = torch.zeros((2, 10), device=gpu)
    for kw in (dict(k=0), dict(k=65), dict(max_gap=-1), dict(min_count=0), dict(row_time=[0, 2, 1, 3, 4, 5, 6, 7, 8, 9]),
               dict(row_time=[0, 1]), dict(threshold=[0.1, 0.2, 0.3])):
        args = dict(threshold=0.5, k=3)
        args.update(kw)
        with pytest.raises(_native.MiClipError):
            retrieval.event_topk(s, **args)
    with pytest.raises(_native.MiClipError):
        retrieval.event_topk(s.cpu(), 0.5, 3)


# ------------------------------------------------------------------ 4. through a corpus
@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("D", [32, 512])
def test_rank_events_equals_the_reference_on_its_own_scores(gpu, D, dtype):
    import torch
    from miclip import retrieval
    rng = np.random.default_rng(D)
    n, Q = 1500, 5
    centres = rng.standard_normal((12, D))
    rows = centres[np.repeat(rng.permutation(12), 125)] + 0.6 * rng.standard_normal((n, D))   # twelve scenes in time order
    rows[[17, 700]] = 0.0                                                               # NaN scores under "l2"
    corpus = torch.from_numpy(rows.astype(np.float32)).to(gpu).to(getattr(torch, dtype))
    queries = torch.from_numpy((centres[:Q] + 0.1 * rng.standard_normal((Q, D))).astype(np.float32)).to(gpu)
    scores = retrieval.score_matrix(corpus, queries, norm="l2")
    host = scores.cpu().numpy()
    tau = np.nanquantile(host, 0.9, axis=1).astype(np.float32)
    times = np.cumsum(rng.integers(1, 4, n))
    for kw in (dict(max_gap=1), dict(max_gap=4, min_count=2, row_time=times), dict(max_gap=2, index_base=77)):
        got = retrieval.rank_events(corpus, queries, 10, tau, norm="l2", **kw)
        want = event_ref_arrays(host, tau, 10, kw["max_gap"], kw.get("min_count", 1), kw.get("row_time"),
                                index_base=kw.get("index_base", 0))
        _same(got, want)
        assert want[5].min() >= 1 and (kw["max_gap"] != 1 or want[5].min() >= 2)


def test_real_rows_against_float64(gpu):
    """The 387 consecutive keyframes, each as a query, tau_i in its score gap (margin >= 5e-4,
    tests/test_event_host.py), max_gap = 2, k = 64 >= every query's events: the set of (begin,
    end, count) and the totals are the float64 ones exactly, each peak score within 8e-6, the
    peak column equal wherever the event's float64 runner-up is more than 2e-6 below its peak."""
    import torch
    from miclip import retrieval
    rows = golden("rank_video_test_4.npz")["corpus"]
    s64, tau, half = real_case(rows)
    assert half.min() >= 5e-4
    corpus = torch.from_numpy(rows).to(gpu)
    unit = rows.astype(np.float64) / np.linalg.norm(rows.astype(np.float64), axis=1, keepdims=True)
    queries = torch.from_numpy(unit.astype(np.float32)).to(gpu)
    got = retrieval.rank_events(corpus, queries, 64, tau.astype(np.float32), max_gap=2, norm="l2")
    score, peak, begin, end, count, total = (x.cpu().numpy() for x in got)
    compared = 0
    for q in range(rows.shape[0]):
        recs, want_total = event_ref(s64[q], tau[q], max_gap=2)
        assert total[q] == want_total <= 64
        mine = {(int(b), int(e), int(c)): (float(v), int(p)) for v, p, b, e, c in
                zip(score[q, :want_total], peak[q, :want_total], begin[q, :want_total], end[q, :want_total],
                    count[q, :want_total])}
        assert set(mine) == {(b, e, c) for _, _, b, e, c in recs}, q
        assert (begin[q, want_total:] == -1).all() and np.isneginf(score[q, want_total:]).all()
        assert (np.diff(score[q, :want_total]) <= 0).all()
        for _, _, b, e, c in recs:
            cols = np.arange(b, e + 1)
            cols = cols[s64[q, cols] >= tau[q]]
            v = np.sort(s64[q, cols])[::-1]
            got_v, got_p = mine[(b, e, c)]
            assert abs(got_v - v[0]) <= 8e-6, (q, b, got_v, v[0])
            if len(v) == 1 or v[0] - v[1] > 2e-6:
                assert got_p == cols[np.argmax(s64[q, cols])], (q, b)
                compared += 1
    assert compared >= 387 * 5


# ------------------------------------------------------------------ 5. FrameLibrary.search_events
def _library(gpu, with_times=True):
    """An f32 and a float16 video with shuffled times, and a second f32 video without times."""
    from miclip.library import FrameLibrary
    rng = np.random.default_rng(21)
    D = 64
    centres = rng.standard_normal((6, D))
    vids = {}
    for name, n, dt in (("a", 300, np.float32), ("h", 280, np.float16), ("b", 90, np.float32)):
        scene = np.repeat(rng.permutation(6), n // 6 + 1)[:n]                       # in time order
        rows = (centres[scene] + 0.5 * rng.standard_normal((n, D))).astype(dt)
        times = np.cumsum(rng.integers(1, 5, n)) if name != "b" else None
        order = rng.permutation(n) if name != "b" else np.arange(n)                 # stored row -> time rank
        vids[name] = (rows[order], None if times is None else times[order])
    lib = FrameLibrary(device=gpu)
    for name, (rows, times) in vids.items():
        lib.add(name, rows, times=times if with_times else None)
    queries = (centres[:4] + 0.05 * rng.standard_normal((4, D))).astype(np.float32)
    return lib, vids, queries


def _library_ref(lib, vids, queries, k, tau, max_gap, min_count=1, video=None, allow=None):
    """search_events by hand: per video the GPU's own scores (score_matrix on the library's
    resident rows) in time order through event_ref, the rows mapped back; all videos' events
    sorted by (peak descending, global begin column ascending: f32 videos first)."""
    import torch
    from miclip import retrieval
    Q = queries.shape[0]
    out = [[] for _ in range(Q)]
    col0 = 0
    for g in lib._groups:
        if not g.rows:
            continue
        scores = retrieval.score_matrix(g.corpus(), torch.from_numpy(queries).to(lib.device), norm=g.norm).cpu().numpy()
        for name, off, n in g.segments:
            times = vids[name][1]
            order = np.arange(n) if times is None else np.argsort(times, kind="stable")
            t = np.arange(n) if times is None else times[order]
            mask = None
            if allow is not None:
                mask = np.zeros(n, bool)
                if name in allow:
                    mask[np.asarray(allow[name])] = True
                mask = mask[order]
            for q in range(Q):
                want = video if video is None or isinstance(video, str) else video[q]
                if want is not None and want != name:
                    continue
                recs, _ = event_ref(scores[q, off:off + n][order], tau, max_gap, min_count, t, mask)
                out[q] += [(float(s), col0 + off + b, lib.names.index(name), int(order[pc]), int(order[b]),
                            int(order[e]), c, s) for s, pc, b, e, c in recs]
        col0 += g.rows
    res = []
    for q in range(Q):
        ev = sorted(out[q], key=lambda r: (-r[0], r[1]))
        res.append((ev[:k], len(ev)))
    return res


def _library_check(lib, vids, queries, k, tau, max_gap, **kw):
    got = lib.search_events(queries, k, tau, max_gap, **kw)
    s, vid, peak, begin, end, count, total = (x.cpu().numpy() for x in got)
    want = _library_ref(lib, vids, queries, k, tau, max_gap, **kw)
    for q, (ev, n) in enumerate(want):
        assert total[q] == n, (q, total[q], n)
        m = len(ev)
        assert [(int(a), int(b), int(c), int(d), int(e)) for a, b, c, d, e in
                zip(vid[q, :m], peak[q, :m], begin[q, :m], end[q, :m], count[q, :m])] == [r[2:7] for r in ev], q
        np.testing.assert_array_equal(_bits(s[q, :m]), _bits(np.array([r[7] for r in ev], np.float32)))
        assert (vid[q, m:] == -1).all() and (peak[q, m:] == -1).all() and (begin[q, m:] == -1).all()
        assert (end[q, m:] == -1).all() and (count[q, m:] == 0).all() and np.isneginf(s[q, m:]).all()
    return want


def test_library_events_shuffled_times_two_dtypes(gpu):
    lib, vids, queries = _library(gpu)
    for k, tau, gap, mc in ((10, 0.45, 4, 1), (64, 0.3, 2, 1), (5, 0.45, 8, 3), (3, -INF, 10, 1)):
        want = _library_check(lib, vids, queries, k, tau, gap, min_count=mc)
        assert all(n >= 2 for _, n in want)
    vid_of = {r[2] for ev, _ in _library_check(lib, vids, queries, 64, 0.3, 2) for r in ev}
    assert vid_of == {0, 1, 2}                         # events of the f32, the float16 and the untimed video


def test_library_events_allow_and_video(gpu):
    lib, vids, queries = _library(gpu)
    rng = np.random.default_rng(5)
    allow = {"a": np.flatnonzero(rng.random(300) < 0.6), "h": np.flatnonzero(rng.random(280) < 0.6)}
    _library_check(lib, vids, queries, 10, 0.4, 6, allow=allow)
    want = _library_check(lib, vids, queries, 10, 0.4, 6, video=["a", "h", None, "b"])
    assert {r[2] for r in want[0][0]} == {0} and {r[2] for r in want[1][0]} == {1} and {r[2] for r in want[3][0]} == {2}
    _library_check(lib, vids, queries, 10, 0.4, 6, video="h", allow=allow)


def test_library_events_never_cross_videos(gpu):
    from miclip import _native
    from miclip.library import FrameLibrary
    rows = np.ones((50, 32), np.float32)
    lib = FrameLibrary(device=gpu)
    lib.add("u", rows, times=np.arange(50)[::-1].copy())
    lib.add("v", rows[:30])
    s, vid, peak, begin, end, count, total = (x.cpu().numpy() for x in
                                              lib.search_events(rows[:1], 5, 0.5, (1 << 40) - 1))
    assert total.tolist() == [2] and count[0].tolist() == [50, 30, 0, 0, 0] and vid[0].tolist() == [0, 1, -1, -1, -1]
    assert (begin[0, 0], end[0, 0], begin[0, 1], end[0, 1]) == (49, 0, 0, 29)       # u's rows run backwards in time
    with pytest.raises(_native.MiClipError):
        lib.search_events(rows[:1], 5, 0.5, 1 << 40)
    for bad in (np.arange(49), np.arange(50) - 1, np.arange(50) + (1 << 40), np.arange(50) * 0.5):
        with pytest.raises(_native.MiClipError):
            lib.add("w", rows, times=bad)
    assert FrameLibrary(device=gpu).search_events(rows[:2], 3, 0.5, 1)[6].tolist() == [0, 0]


def test_library_search_unchanged_by_times(gpu):
    import torch
    (lib, _, queries), (plain, _, _) = _library(gpu), _library(gpu, with_times=False)
    for kw in (dict(), dict(video="h"), dict(distinct=0.9)):
        for a, b in zip(lib.search(queries, 10, **kw), plain.search(queries, 10, **kw)):
            assert torch.equal(a, b)


# ------------------------------------------------------------------ 6. the service
FRAME_NUMBERS = [2214, 4599, 6704, 10152, 10153, 10160, 12000, 12001, 12002, 15000, 99, 100, 101, 30000, 30001, 30002]


@pytest.fixture()
def service(gpu, tmp_path, monkeypatch):
    """Two videos whose frame lists are string-sorted numeric names, a third with a non-numeric
    name; rows planted so that the query (the service's own text features) matches known frames."""
    import torch
    from miclip import api, service as S
    root = tmp_path / "state"
    (root / "metadata").mkdir(parents=True)
    (root / "embedding").mkdir(parents=True)
    paths = Paths(str(root))
    svc = S.EmbeddingService(Cache(), paths, Data(paths, None), device="cuda", model_name="test-small")
    cfg = svc.original_model.cfg
    monkeypatch.setattr(api, "tokenize", lambda texts, *a, **k: torch.from_numpy(
        np.concatenate([_tokens(t, cfg) for t in texts])))
    text = np.asarray(svc.get_text_features("a person enters", None), np.float64).reshape(-1)
    rng = np.random.default_rng(3)
    noise = rng.standard_normal((3, len(FRAME_NUMBERS), text.shape[0]))
    noise -= np.outer(noise.reshape(-1, text.shape[0]) @ text, text).reshape(noise.shape) / (text @ text)
    noise /= np.linalg.norm(noise, axis=2, keepdims=True)
    videos = {}
    for v, (name, dt) in enumerate((("one", np.float32), ("two", np.float16), ("odd", np.float32))):
        frames = sorted(f"{t}.jpg" for t in FRAME_NUMBERS)
        if name == "odd":
            frames[4] = "cover.jpg"                  # in place of the string-sorted "10160.jpg"
        # cosine to the query by frame number: hot (>= 0.5) in runs, best frame in the middle run
        cos = {f: 0.1 for f in frames}
        for t, c in ((10152, 0.7), (10153, 0.9), (10160, 0.6), (12000, 0.65), (12001, 0.6), (99, 0.55), (101, 0.8),
                     (30002, 0.75)):
            if f"{t}.jpg" in cos:
                cos[f"{t}.jpg"] = c + 0.01 * v
        unit = text / np.linalg.norm(text)
        rows = np.stack([cos[f] * unit + np.sqrt(1 - cos[f] ** 2) * noise[v, i] for i, f in enumerate(frames)])
        np.save(paths.get_embeddings_path(name), rows.astype(dt))
        with open(paths.get_metadata_path(name), "w") as f:
            json.dump([{"frame": x} for x in frames], f)
        videos[name] = frames
    return svc, videos


def _records(out):
    return [(r["frame"], r["start"], r["end"], r["frames"]) for r in out]


def test_service_events_are_in_time_terms(service):
    svc, videos = service
    out, total = svc.search_events("a person enters", 10, "one", threshold=0.5, max_gap=10, with_total=True)
    assert total == 4 and _records(out) == [("10153.jpg", "10152.jpg", "10160.jpg", 3), ("101.jpg", "99.jpg", "101.jpg", 2),
                                            ("30002.jpg", "30002.jpg", "30002.jpg", 1),
                                            ("12000.jpg", "12000.jpg", "12001.jpg", 2)]
    assert [round(r["score"], 2) for r in out] == [0.9, 0.8, 0.75, 0.65]
    assert svc.search_events("a person enters", 10, "one", threshold=0.5, max_gap=10) == out
    assert _records(svc.search_events("a person enters", 10, "one", threshold=0.5, max_gap=1)) == [
        ("10153.jpg", "10152.jpg", "10153.jpg", 2), ("101.jpg", "101.jpg", "101.jpg", 1),
        ("30002.jpg", "30002.jpg", "30002.jpg", 1), ("12000.jpg", "12000.jpg", "12001.jpg", 2),
        ("10160.jpg", "10160.jpg", "10160.jpg", 1), ("99.jpg", "99.jpg", "99.jpg", 1)]
    assert _records(svc.search_events("a person enters", 2, "two", threshold=0.5, max_gap=10, min_frames=2)) == [
        ("10153.jpg", "10152.jpg", "10160.jpg", 3), ("101.jpg", "99.jpg", "101.jpg", 2)]
    # a non-numeric name: the row number is the time axis (rows 100 | 101 | 10152 | 10153 | cover | 12000 | 12001 ...)
    assert _records(svc.search_events("a person enters", 10, "odd", threshold=0.5, max_gap=1)) == [
        ("10153.jpg", "101.jpg", "10153.jpg", 3), ("30002.jpg", "30002.jpg", "30002.jpg", 1),
        ("12000.jpg", "12000.jpg", "12001.jpg", 2), ("99.jpg", "99.jpg", "99.jpg", 1)]


def test_service_events_all_videos(service):
    svc, videos = service
    out, total = svc.search_events_all("a person enters", 5, ["one", "two"], threshold=0.5, max_gap=10, with_total=True)
    assert total == 8 and [(v,) + rec for v, rec in zip([v for v, _ in out], _records([r for _, r in out]))] == [
        ("two", "10153.jpg", "10152.jpg", "10160.jpg", 3), ("one", "10153.jpg", "10152.jpg", "10160.jpg", 3),
        ("two", "101.jpg", "99.jpg", "101.jpg", 2), ("one", "101.jpg", "99.jpg", "101.jpg", 2),
        ("two", "30002.jpg", "30002.jpg", "30002.jpg", 1)]
    lib = svc._frame_library(["one", "two"])
    assert all(t is not None for g in lib._groups for t in g.times)
    only = svc.search_events_all("a person enters", 5, ["one", "two"], threshold=0.5, max_gap=10,
                                 allow_frames={"one": ["99.jpg", "10160.jpg", "12000.jpg"]})
    assert [(v,) + rec for v, rec in zip([v for v, _ in only], _records([r for _, r in only]))] == [
        ("one", "12000.jpg", "12000.jpg", "12000.jpg", 1), ("one", "10160.jpg", "10160.jpg", "10160.jpg", 1),
        ("one", "99.jpg", "99.jpg", "99.jpg", 1)]
    mixed = svc.search_events_all("a person enters", 64, ["one", "odd"], threshold=0.5, max_gap=10)
    lib = svc._frame_library(["one", "odd"])
    assert [t is None for t in lib._groups[0].times] == [False, True]
    # odd's hot rows 1, 2, 3, 5, 6, 12, 15 are at most 6 rows apart: one event on the row axis
    assert ("odd", ("10153.jpg", "101.jpg", "99.jpg", 7)) in [(v, _records([r])[0]) for v, r in mixed]


def test_service_event_cache_keys_and_swallowed_errors(service, capsys):
    svc, _ = service
    a = svc.search_events("a person enters", 10, "one", threshold=0.5, max_gap=10)
    keys = {k for k in svc.cache_service.d if k[0] == "s"}
    for kw in (dict(threshold=0.6, max_gap=10), dict(threshold=0.5, max_gap=1), dict(threshold=0.5, max_gap=10, min_frames=2),
               dict(threshold=0.5, max_gap=10, with_total=True)):
        before = len({k for k in svc.cache_service.d if k[0] == "s"})
        svc.search_events("a person enters", 10, "one", **kw)
        assert len({k for k in svc.cache_service.d if k[0] == "s"}) == before + 1, kw
    svc.search_events("a person enters", 9, "one", threshold=0.5, max_gap=10)
    svc.search_events("a person enters", 10, "two", threshold=0.5, max_gap=10)
    assert len({k for k in svc.cache_service.d if k[0] == "s"}) == len(keys) + 6
    svc.cache_service.d[next(iter(keys))] = ["cached"]
    assert svc.search_events("a person enters", 10, "one", threshold=0.5, max_gap=10) == ["cached"] != a
    # errors are swallowed, as in search_top_frames
    assert svc.search_events("a person enters", 10, "missing", threshold=0.5, max_gap=10) == []
    assert svc.search_events("a person enters", 10, "one", threshold=0.5, max_gap=-1) == []
    assert svc.search_events("a person enters", 10, "one", threshold=0.5, max_gap=-1, with_total=True) == ([], 0)
    assert svc.search_events_all("a person enters", 10, ["one", "missing"], threshold=0.5, max_gap=10) == []
    assert svc.search_events_all("a person enters", 10, ["one"], threshold=0.5, max_gap=1 << 41) == []
    assert svc.search_events("a person enters", 0, "one", threshold=0.5, max_gap=10) == []
    with pytest.raises(TypeError):
        svc.search_events("a person enters", 10, "one")                             # no default threshold / max_gap
    assert "Error in search_events" in capsys.readouterr().out
