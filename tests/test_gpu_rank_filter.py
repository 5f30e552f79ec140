"""Filtered top-k on the GPU (mi_rank_topk_filtered, csrc/rank_filter.hip), FrameLibrary and
EmbeddingService.search_top_frames_all.

Every comparison is bitwise (scores as int32 views, indices exactly).  The expected result
of a query is the existing product pass over the gathered visible rows,
``rank_topk(corpus[visible_rows], q, k, norm, nan_policy)``, its indices mapped back through
``visible_rows`` and padded with (-inf, -1): a row's score depends on the row and the query
only, so nothing is approximated."""
import json
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")


def _rows(gpu, n, d, dtype, seed):
    import torch
    g = torch.Generator(device=gpu).manual_seed(seed)
    return torch.randn(n, d, device=gpu, generator=g).to(dtype)


def _queries(gpu, q, d, seed):
    import torch
    g = torch.Generator(device=gpu).manual_seed(seed)
    return torch.nn.functional.normalize(torch.randn(q, d, device=gpu, generator=g), dim=1)


def _pad(s, i, k):
    import torch
    Q, kk = s.shape
    os_ = torch.full((Q, k), NEG_INF, dtype=torch.float32, device=s.device)
    oi = torch.full((Q, k), -1, dtype=torch.int64, device=s.device)
    os_[:, :kk] = s
    oi[:, :kk] = i
    return os_, oi


def _expected(corpus, q, k, mask=None, ranges=None, base=0, norm="l2", nan="first"):
    """rank_topk over each query's gathered visible rows (queries that share a range share a call)."""
    import torch
    from miclip import retrieval
    n, Q = corpus.shape[0], q.shape[0]
    es = torch.full((Q, k), NEG_INF, dtype=torch.float32, device=corpus.device)
    ei = torch.full((Q, k), -1, dtype=torch.int64, device=corpus.device)
    groups = {}
    for qi in range(Q):
        b, e = (0, n) if ranges is None else (max(int(ranges[qi][0]), 0), min(int(ranges[qi][1]), n))
        groups.setdefault((b, e), []).append(qi)
    for (b, e), qs in groups.items():
        if b >= e:
            continue
        vis = torch.arange(b, e, device=corpus.device)
        if mask is not None:
            vis = vis[mask[b:e]]
        if vis.numel() == 0:
            continue
        s, i = retrieval.rank_topk(corpus.index_select(0, vis), q[qs], k, norm=norm, nan_policy=nan)
        kk = s.shape[1]
        es[qs, :kk] = s
        ei[qs, :kk] = vis[i] + base
    return es, ei


def _same(got, want, what=""):
    import torch
    gs, gi = got
    ws, wi = want
    assert gs.shape == ws.shape and gi.shape == wi.shape, what
    assert torch.equal(gi, wi), (what, (gi != wi).nonzero()[:5].tolist())
    assert torch.equal(gs.contiguous().view(torch.int32), ws.contiguous().view(torch.int32)), what


def _filtered(corpus, q, k, mask=None, ranges=None, base=0, norm="l2", nan="first"):
    import torch
    from miclip import retrieval
    rng = ranges if ranges is None or isinstance(ranges, tuple) else torch.as_tensor(ranges, dtype=torch.int64)
    return retrieval.rank_topk_filtered(corpus, q, k, row_mask=mask, query_range=rng, index_base=base, norm=norm,
                                        nan_policy=nan)


# (N, D, dtype, k, norm, nan, index_base): every N, D, dtype, k, norm and NaN policy of the issue
# appears; D = 512 with k <= 16 is where rank_topk runs rank_reg
IDENTITY = [
    (1, 32, "float32", 1, "l2", "first", 0),
    (31, 512, "float32", 10, "l2", "first", 7),
    (32, 512, "bfloat16", 16, "l2_guard", "last", 0),
    (33, 768, "float16", 17, "none", "first", 1000),
    (383, 1024, "float32", 60, "l2", "last", 0),
    (384, 512, "float16", 64, "l2", "first", 5),
    (385, 32, "bfloat16", 10, "none", "last", 0),
    (385, 768, "float32", 64, "l2_guard", "first", 0),
    (100_003, 512, "float32", 10, "l2", "first", 3),
    (100_003, 768, "bfloat16", 16, "l2", "last", 0),
    (100_003, 512, "float32", 60, "l2_guard", "first", 0),
    (100_003, 1024, "float16", 1, "l2", "last", 1 << 33),
    (100_003, 32, "float32", 17, "none", "first", 11),
]


@pytest.mark.parametrize("N,D,dtype,k,norm,nan,base", IDENTITY)
def test_identity_with_rank_topk(gpu, N, D, dtype, k, norm, nan, base):
    """No mask and no range, and an all-ones mask with range [0, N): rank_topk bit for bit."""
    import torch
    from miclip import retrieval
    corpus = _rows(gpu, N, D, getattr(torch, dtype), seed=N + D)
    q = _queries(gpu, 5, D, seed=k)
    want = _pad(*retrieval.rank_topk(corpus, q, k, index_base=base, norm=norm, nan_policy=nan), k)
    _same(_filtered(corpus, q, k, base=base, norm=norm, nan=nan), want, "no filter")
    ones = torch.ones(N, dtype=torch.bool, device=gpu)
    _same(_filtered(corpus, q, k, mask=ones, ranges=[[0, N]] * 5, base=base, norm=norm, nan=nan), want, "all visible")
    packed = torch.full(((N + 31) // 32,), -1, dtype=torch.int32, device=gpu)   # bits at or beyond N set too
    _same(_filtered(corpus, q, k, mask=packed, ranges=(0, N), base=base, norm=norm, nan=nan), want, "packed words")


@pytest.fixture(scope="module")
def mid(gpu):
    """5000 x 64 f32 rows (14 workgroups), 33 queries (two query blocks)."""
    return _rows(gpu, 5000, 64, __import__("torch").float32, seed=1), _queries(gpu, 33, 64, seed=2)


def _mid_ranges(N):
    r = [[0, N]] * 33
    r[0] = [33, 95]              # starts and ends mid-tile
    r[1] = [700, 701]            # one row
    r[2] = [900, 900]            # begin == end
    r[3] = [1200, 1100]          # begin > end
    r[4] = [4990, N + 500]       # past N
    r[5] = [N, N + 10]           # wholly past N
    r[6] = [-50, 7]              # clipped at 0; fewer than k rows
    r[7] = [383, 385]            # across a workgroup edge
    r[8] = [2000, 2005]          # fewer than k rows
    for i in range(9, 32):       # differing ranges inside one 32-query block
        r[i] = [37 * i, 37 * i + 400 + 13 * i]
    r[32] = [4000, 4500]         # the second query block's union differs from the first's
    return r


@pytest.mark.parametrize("k", [10, 20])
def test_ranges(gpu, mid, k):
    corpus, q = mid
    N = corpus.shape[0]
    ranges = _mid_ranges(N)
    got = _filtered(corpus, q, k, ranges=ranges, base=100)
    _same(got, _expected(corpus, q, k, ranges=ranges, base=100), "ranges")
    gs, gi = got
    for qi in (2, 3, 5):
        assert (gi[qi] == -1).all() and (gs[qi] == NEG_INF).all()
    assert gi[1].tolist() == [800] + [-1] * (k - 1)
    assert (gi[8, :5] >= 0).all() and (gi[8, 5:] == -1).all() and (gs[8, 5:] == NEG_INF).all()
    # a block whose ranges are all empty: every workgroup exits at entry
    _same(_filtered(corpus, q[:4], k, ranges=[[5, 5], [9, 2], [N, N + 1], [-3, 0]]),
          _expected(corpus, q[:4], k, ranges=[[5, 5], [9, 2], [N, N + 1], [-3, 0]]), "all empty")


@pytest.mark.parametrize("k", [10, 20])
def test_masks(gpu, mid, k):
    import torch
    from miclip import retrieval
    corpus, q = mid
    corpus, q = corpus[:4987], q[:6]             # the last word is partial: 27 rows
    N = corpus.shape[0]
    words = (N + 31) // 32
    empty = (torch.full((6, k), NEG_INF, device=gpu), torch.full((6, k), -1, dtype=torch.int64, device=gpu))
    _same(_filtered(corpus, q, k, mask=torch.zeros(N, dtype=torch.bool, device=gpu)), empty, "all zero")
    beyond = torch.zeros(words, dtype=torch.int32, device=gpu)
    beyond[-1] = -1 << (N % 32)                  # only bits at or beyond N
    _same(_filtered(corpus, q, k, mask=beyond), empty, "bits beyond N")
    last = torch.zeros(N, dtype=torch.bool, device=gpu)
    last[words * 32 - 32:] = True                # only the last partial word
    _same(_filtered(corpus, q, k, mask=last), _expected(corpus, q, k, mask=last), "last word")
    lastw = torch.zeros(words, dtype=torch.int32, device=gpu)
    lastw[-1] = -1                               # the same, with the bits beyond N set as well
    _same(_filtered(corpus, q, k, mask=lastw), _expected(corpus, q, k, mask=last), "last word, packed")
    g = torch.Generator(device=gpu).manual_seed(5)
    sparse = torch.rand(N, device=gpu, generator=g) < 1 / 16
    _same(_filtered(corpus, q, k, mask=sparse), _expected(corpus, q, k, mask=sparse), "density 1/16")
    assert torch.equal(retrieval.pack_row_mask(sparse).cpu(),
                       torch.from_numpy(np.packbits(np.pad(sparse.cpu().numpy(), (0, -N % 32)),
                                                    bitorder="little").view("<i4").copy()))


@pytest.mark.parametrize("k", [10, 17])
def test_clustered_mask_several_workgroups(gpu, k):
    """N = 40 000 (105 workgroups): only words 5 and 900 set."""
    import torch
    corpus = _rows(gpu, 40_000, 32, torch.float32, seed=9)
    q = _queries(gpu, 3, 32, seed=10)
    m = torch.zeros(40_000, dtype=torch.bool, device=gpu)
    m[5 * 32:6 * 32] = True
    m[900 * 32:901 * 32] = True
    got = _filtered(corpus, q, k, mask=m)
    _same(got, _expected(corpus, q, k, mask=m), "clustered")
    assert ((got[1] // 32 == 5) | (got[1] // 32 == 900)).all()


@pytest.mark.parametrize("k", [10, 17])
def test_dead_and_live_tiles_inside_a_wave_stream(gpu, k):
    """600 000 rows: 1536 rows (48 tiles) per workgroup, so a wave streams 4 tiles (k <= 16, 12
    waves) or 12 (k > 16, 4 waves).  Tiles 12..35 of every workgroup live and the rest dead is
    'first and last tile of each wave's stream dead, the middle live' for both; then the reverse."""
    import torch
    N = 600_000
    corpus = _rows(gpu, N, 32, torch.bfloat16, seed=12)
    q = _queries(gpu, 3, 32, seed=13)
    g = torch.Generator(device=gpu).manual_seed(14)
    dense = torch.rand(N, device=gpu, generator=g) < 0.5
    tile = (torch.arange(N, device=gpu) // 32) % 48
    middle = (tile >= 12) & (tile < 36)
    for name, m in (("middle live", dense & middle), ("ends live", dense & ~middle)):
        _same(_filtered(corpus, q, k, mask=m, norm="l2"), _expected(corpus, q, k, mask=m, norm="l2"), name)
    # ... and a range hull that cuts every stream short of its last tiles
    _same(_filtered(corpus, q, k, mask=dense, ranges=[[1536 + 12 * 32, 3 * 1536 - 13 * 32]] * 3),
          _expected(corpus, q, k, mask=dense, ranges=[[1536 + 12 * 32, 3 * 1536 - 13 * 32]] * 3), "hull")


@pytest.mark.parametrize("k", [10, 20])
def test_mask_and_range_together(gpu, mid, k):
    import torch
    corpus, q = mid
    N = corpus.shape[0]
    m = torch.zeros(N, dtype=torch.bool, device=gpu)
    m[1000:1100] = True
    m[3000:3003] = True
    m[4999] = True
    ranges = _mid_ranges(N)              # some ranges meet the mask, some do not
    ranges[10] = [1050, 3001]
    ranges[11] = [1100, 3000]            # between the clusters: empty
    ranges[12] = [4999, 5000]
    got = _filtered(corpus, q, k, mask=m, ranges=ranges, nan="last")
    _same(got, _expected(corpus, q, k, mask=m, ranges=ranges, nan="last"), "mask and range")
    assert (got[1][11] == -1).all() and got[1][12].tolist() == [4999] + [-1] * (k - 1)
    assert (got[1][0] == -1).all() and (got[1][10] >= 0).sum() == min(k, 51)


@pytest.mark.parametrize("nan", ["first", "last"])
@pytest.mark.parametrize("k", [10, 20])
def test_nan_rows_visible_and_hidden(gpu, k, nan):
    """Zero rows score NaN under L2: visible ones rank by the policy, a hidden one never appears."""
    import torch
    corpus = _rows(gpu, 2000, 64, torch.float32, seed=20).clone()
    q = _queries(gpu, 4, 64, seed=21)
    zero = [3, 40, 700, 701, 1500, 1999]
    corpus[zero] = 0.0
    m = torch.ones(2000, dtype=torch.bool, device=gpu)
    m[[40, 701]] = False                               # hidden by the mask
    ranges = [[0, 2000], [0, 1999], [41, 1500], [600, 800]]   # 1999 / 3, 40, 1500, 1999 / ... hidden by range
    got = _filtered(corpus, q, k, mask=m, ranges=ranges, nan=nan)
    _same(got, _expected(corpus, q, k, mask=m, ranges=ranges, nan=nan), "nan rows")
    gi = got[1]
    assert not torch.isin(gi, torch.tensor([40, 701], device=gpu)).any()
    vis_nan = [[3, 700, 1500, 1999], [3, 700, 1500], [700], [700]]
    for qi, want in enumerate(vis_nan):
        if nan == "first":
            assert gi[qi, :len(want)].tolist() == want and torch.isnan(got[0][qi, :len(want)]).all()
            assert not torch.isnan(got[0][qi, len(want):]).any()
        else:
            assert not torch.isnan(got[0][qi]).any() and not torch.isin(gi[qi], torch.tensor(zero, device=gpu)).any()


@pytest.mark.parametrize("k", [10, 20])
def test_duplicate_rows_across_range_and_mask_edges(gpu, k):
    import torch
    corpus = _rows(gpu, 1000, 64, torch.float32, seed=30).clone()
    q = _queries(gpu, 2, 64, seed=31)
    corpus[100:112] = 50.0 * q[0]                      # 12 copies of the best row of query 0
    m = torch.ones(1000, dtype=torch.bool, device=gpu)
    m[[101, 107]] = False
    m[110:] = False
    m[500:] = True
    ranges = [[103, 1000], [0, 1000]]
    got = _filtered(corpus, q, k, mask=m, ranges=ranges)
    _same(got, _expected(corpus, q, k, mask=m, ranges=ranges), "duplicates")
    copies = [103, 104, 105, 106, 108, 109]            # the visible copies, index ascending
    assert got[1][0, :6].tolist() == copies
    assert len(set(got[0][0, :6].tolist())) == 1


@pytest.mark.parametrize("k", [16, 64])
def test_two_thousand_identical_visible_rows(gpu, k):
    import torch
    q = _queries(gpu, 2, 32, seed=41)
    corpus = q[1].repeat(3000, 1).contiguous()
    g = torch.Generator(device=gpu).manual_seed(42)
    m = torch.zeros(3000, dtype=torch.bool, device=gpu)
    m[torch.randperm(3000, device=gpu, generator=g)[:2000]] = True
    got = _filtered(corpus, q, k, mask=m)
    _same(got, _expected(corpus, q, k, mask=m), "identical rows")
    first = m.nonzero().flatten()[:k]
    assert torch.equal(got[1][0], first) and torch.equal(got[1][1], first)


# ------------------------------------------------------------------ against the NumPy oracle
# The bitwise tests above compare the filtered pass with rank_topk, which at D != 512 or k > 16
# runs the same pass body under the other row policy; this one compares it with float64 NumPy.
def _small_ranges(N):
    """_mid_ranges' pattern at N = 1000 (three 384-row workgroups)."""
    r = [[0, N]] * 33
    r[0] = [33, 95]              # starts and ends mid-tile
    r[1] = [700, 701]            # one row
    r[2] = [900, 900]            # begin == end
    r[3] = [240, 220]            # begin > end
    r[4] = [N - 10, N + 500]     # past N
    r[5] = [N, N + 10]           # wholly past N
    r[6] = [-50, 7]              # clipped at 0
    r[7] = [767, 769]            # across a workgroup edge
    r[8] = [800, 805]            # fewer than k rows
    for i in range(9, 32):       # differing ranges inside one 32-query block
        r[i] = [30 * i, 30 * i + 80 + 13 * i]
    r[32] = [800, 900]           # the second query block's hull: two workgroups without a live tile
    return r


ORACLE_ZERO_VISIBLE, ORACLE_ZERO_HIDDEN = 750, 100


@pytest.fixture(scope="module", params=[32, 96])
def oracle_case(gpu, request):
    """1000 x D f32 rows, 33 queries, a mask of rows 40-45 and 700-990, per-query ranges, a visible
    and a hidden zero row; per query the visible rows and their float64 scores (computed once)."""
    import torch
    from oracle import rank_ref
    D, N = request.param, 1000
    corpus = _rows(gpu, N, D, torch.float32, seed=50 + D).clone()
    corpus[[ORACLE_ZERO_VISIBLE, ORACLE_ZERO_HIDDEN]] = 0.0
    q = _queries(gpu, 33, D, seed=51)
    mask = torch.zeros(N, dtype=torch.bool, device=gpu)
    mask[40:46] = True
    mask[700:991] = True
    ranges = _small_ranges(N)
    c, qq, m = corpus.cpu().numpy(), q.cpu().numpy(), mask.cpu().numpy()
    ref = []
    for qi, (b, e) in enumerate(ranges):
        b, e = max(b, 0), min(e, N)
        vis = np.arange(b, e)[m[b:e]] if b < e else np.zeros(0, np.int64)
        with np.errstate(invalid="ignore", divide="ignore"):
            S = rank_ref.scores_ref(c[vis], qq[qi:qi + 1])[0] if len(vis) else np.zeros(0)
        ref.append((vis, S))
    return corpus, q, mask, ranges, ref


@pytest.mark.parametrize("nan", ["first", "last"])
@pytest.mark.parametrize("k", [10, 17])
def test_filtered_matches_oracle(oracle_case, k, nan):
    """rank_topk_filtered (k = 10: the stream kernel, k = 17: the tiles kernel; D = 32 / 96: 1 / 3
    chunks per tile) against NumPy over each query's gathered visible rows, indices mapped back."""
    from oracle import rank_ref
    corpus, q, mask, ranges, ref = oracle_case
    gs, gi = _filtered(corpus, q, k, mask=mask, ranges=ranges, nan=nan)
    gs, gi = gs.cpu().numpy(), gi.cpu().numpy()
    assert gs.shape == (33, k) and gi.shape == (33, k)
    empty = 0
    for qi, (vis, S) in enumerate(ref):
        kk = min(k, len(vis))
        assert (gi[qi, kk:] == -1).all() and (gs[qi, kk:] == NEG_INF).all(), qi
        empty += kk == 0
        if kk == 0:
            continue
        assert np.isin(gi[qi, :kk], vis).all(), (qi, gi[qi, :kk])            # only visible rows
        pos = np.searchsorted(vis, gi[qi, :kk])                              # global row -> gathered position
        rank_ref.assert_topk_equivalent(gs[qi, :kk], pos, S, k, nan_policy=nan)
    assert empty >= 4                                                        # r[2], r[3], r[5], r[6]
    assert ranges[20][0] <= ORACLE_ZERO_VISIBLE < ranges[20][1]             # [600, 940): more than k visible rows
    assert (ORACLE_ZERO_VISIBLE in gi[20]) == (nan == "first")
    assert not (gi == ORACLE_ZERO_HIDDEN).any()


# ------------------------------------------------------------------ library
@pytest.fixture(scope="module")
def library(gpu):
    import torch
    from conftest import golden
    from miclip import library as L, retrieval, weights
    g3, g4 = golden("rank_video_test_3.npz"), golden("rank_video_test_4.npz")
    videos = {"v3": np.asarray(g3["corpus"]), "v4": np.asarray(g4["corpus"], dtype=np.float32),
              "syn": weights.synthetic_corpus(500, 512, seed=77) * 3.0}
    lib = L.FrameLibrary(device=gpu)
    for name in ("v3", "v4", "syn"):
        lib.add(name, videos[name])
    # the per-video path of EmbeddingService._corpus_on_device / _rank
    dev = {}
    for name, rows in videos.items():
        t = torch.from_numpy(np.ascontiguousarray(rows)).to(gpu)
        dev[name] = (retrieval.normalize_rows_f16(t, out=t), "none") if t.dtype == torch.float16 else (t, "l2")
    q = torch.from_numpy(np.concatenate([np.asarray(g3["queries"])[:36], np.asarray(g4["queries"])[:4]])).to(gpu)
    return lib, dev, q


def _locate_expected(lib, name, s, i, k):
    """(scores, video_index, row) [Q, k] from a per-video ranking."""
    import torch
    s, i = _pad(s, i, k)
    vid = torch.where(i >= 0, torch.full_like(i, lib.names.index(name)), torch.full_like(i, -1)).to(torch.int32)
    return s, vid, i


def _same3(got, want, what=""):
    import torch
    assert got[1].dtype == torch.int32 and got[2].dtype == torch.int64
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), what
    assert torch.equal(got[0].contiguous().view(torch.int32), want[0].contiguous().view(torch.int32)), what


@pytest.mark.parametrize("k", [10, 60])
def test_library_one_video_equals_per_video_path(library, k):
    from miclip import retrieval
    lib, dev, q = library
    assert lib.names == ["v3", "v4", "syn"]
    assert [s[:3] for s in lib.segments()] == [("v4", 0, 387), ("syn", 387, 500), ("v3", 887, 360)]
    for name, (rows, norm) in dev.items():
        s, i = retrieval.rank_topk(rows, q[:8], k, norm=norm, nan_policy="first")
        _same3(lib.search(q[:8], k, video=name), _locate_expected(lib, name, s, i, k), name)


@pytest.mark.parametrize("k", [10, 60])
def test_library_all_videos_equals_merged_rankings(library, k):
    import torch
    from miclip import retrieval
    lib, dev, q = library
    cs, ci = [], []
    for name, off, rows, norm in lib.segments():
        s, i = retrieval.rank_topk(dev[name][0], q[:8], k, index_base=off, norm=dev[name][1])
        cs.append(s)
        ci.append(i)
    ms, mi = retrieval.merge_topk(torch.cat(cs, 1), torch.cat(ci, 1), k)
    vid, row = lib.locate(mi)
    _same3(lib.search(q[:8], k), (ms, vid, row), "all videos")


def test_library_per_query_videos(library):
    """Q = 40 > 32: the queries are sorted by range begin for the kernel and un-permuted after."""
    from miclip import retrieval
    lib, dev, q = library
    k = 10
    videos = [("syn", "v3", None, "v4")[(i * 7) % 4] for i in range(40)]
    got = lib.search(q, k, video=videos)
    allv = lib.search(q, k)
    for name in ("syn", "v3", "v4"):
        qs = [i for i, v in enumerate(videos) if v == name]
        s, i = retrieval.rank_topk(dev[name][0], q[qs], k, norm=dev[name][1])
        _same3(tuple(t[qs] for t in got), _locate_expected(lib, name, s, i, k), name)
    qs = [i for i, v in enumerate(videos) if v is None]
    _same3(tuple(t[qs] for t in got), tuple(t[qs] for t in allv), "None")


def test_library_allow_index_arrays(library):
    import torch
    from miclip import retrieval
    lib, dev, q = library
    k = 10
    rng = np.random.default_rng(3)
    allow = {"v3": rng.choice(360, 40, replace=False), "syn": np.array([499, 0, 31, 32]), "v4": True}
    got = lib.search(q[:8], k, video=["v3", "syn", "v4", None] * 2, allow=allow)
    for qi, name in enumerate(["v3", "syn", "v4", None] * 2):
        if name is None:
            continue
        rows = np.arange(387) if name == "v4" else np.sort(allow[name])
        vis = torch.from_numpy(rows).to(q.device)
        s, i = retrieval.rank_topk(dev[name][0].index_select(0, vis), q[qi:qi + 1], k, norm=dev[name][1])
        _same3(tuple(t[qi:qi + 1] for t in got), _locate_expected(lib, name, s, vis[i], k), (qi, name))
    assert (got[2][1, 4:] == -1).all() and (got[1][1, 4:] == -1).all()      # four allowed frames in "syn"
    none = lib.search(q[:2], k, allow={})                                   # every video excluded
    assert (none[1] == -1).all() and (none[2] == -1).all() and (none[0] == NEG_INF).all()


# ------------------------------------------------------------------ service
class Cache:
    def __init__(self):
        self.d = {}

    def get_text_features(self, key, video):
        return self.d.get(("t", key, video))

    def set_text_features(self, key, video, v):
        self.d[("t", key, video)] = v

    def get_embeddings(self, path):
        return self.d.get(("e", path))

    def set_embeddings(self, path, v):
        self.d[("e", path)] = v

    def get_frames_list(self, path):
        return self.d.get(("f", path))

    def set_frames_list(self, path, v):
        self.d[("f", path)] = v

    def get_search_results(self, key, video):
        return self.d.get(("s", key, video))

    def set_search_results(self, key, video, v):
        self.d[("s", key, video)] = v


class Paths:
    def __init__(self, root):
        self.root = root

    def get_embeddings_path(self, video):
        return os.path.join(self.root, "embedding", f"{video}_embeddings.npy")

    def get_metadata_path(self, video):
        return os.path.join(self.root, "metadata", f"{video}_metadata.json")


class Data:
    def __init__(self, paths):
        self.paths = paths

    def load_frames_from_json(self, video):
        with open(self.paths.get_metadata_path(video)) as f:
            return [item["frame"] for item in json.load(f)]


VIDEOS = {"va": (300, np.float32), "vh": (200, np.float16), "vb": (150, np.float32)}


@pytest.fixture()
def service(gpu, tmp_path, monkeypatch):
    import torch
    from miclip import api, service as S, weights
    root = tmp_path / "state"
    (root / "metadata").mkdir(parents=True)
    (root / "embedding").mkdir(parents=True)
    paths = Paths(str(root))
    svc = S.EmbeddingService(Cache(), paths, Data(paths), device="cuda", model_name="test-small")
    cfg = svc.original_model.cfg
    for j, (v, (n, dt)) in enumerate(VIDEOS.items()):
        rows = (weights.synthetic_corpus(n, cfg.embed_dim, seed=60 + j) * (1.0 + j)).astype(dt)
        np.save(paths.get_embeddings_path(v), rows)
        with open(paths.get_metadata_path(v), "w") as f:
            json.dump([{"frame": f"frames/{v}/{i:04d}.jpg"} for i in range(n)], f)
    monkeypatch.setattr(api, "tokenize", lambda texts, *a, **k: torch.from_numpy(np.concatenate(
        [weights.synthetic_tokens(1, cfg.context_length, cfg.vocab_size, seed=zlib.crc32(t.encode()) % 1000)
         for t in texts])))
    return svc


def _score(svc, query, video, frame):
    """The frame's rank score, as the per-video path computes it (bitwise comparable)."""
    import torch
    from miclip import retrieval
    rows, norm = svc._corpus_on_device(video)
    i = svc._frames(video).index(frame)
    t = torch.from_numpy(np.asarray(svc.get_text_features(query, None), dtype=np.float32)).to(rows.device)
    s, _ = retrieval.rank_topk(rows[i:i + 1], t, 1, norm=norm)
    return float(s[0, 0])


def test_service_search_all(service):
    svc = service
    names = list(VIDEOS)
    query, k = "a red car at night", 20
    got = svc.search_top_frames_all(query, k, names)
    assert len(got) == k and len(set(got)) == k and {v for v, _ in got} <= set(names)
    scores = [_score(svc, query, v, f) for v, f in got]
    assert all(a >= b for a, b in zip(scores, scores[1:]))
    for v, (n, _) in VIDEOS.items():
        full = svc.search_top_frames(query, n, v)
        mine = [f for vv, f in got if vv == v]
        assert mine == full[:len(mine)]                               # a prefix of the video's own ranking
        if len(mine) < n:                                             # the best excluded frame scores no higher
            assert _score(svc, query, v, full[len(mine)]) <= scores[-1]
    assert svc.search_top_frames_all(query, k, names) == got         # the cached library
    assert svc._library[3] is svc._frame_library(names)
    one = svc.search_top_frames_all(query, 7, ["vh"])
    assert [f for _, f in one] == svc.search_top_frames(query, 7, "vh") and {v for v, _ in one} == {"vh"}


def test_service_allow_frames(service):
    svc = service
    names = list(VIDEOS)
    query, k = "people walking", 5
    unfiltered = svc.search_top_frames_all(query, 64, names)
    deep = svc.search_top_frames(query, 300, "va")[200]               # far below top_k * 3 unfiltered
    assert ("va", deep) not in unfiltered
    allow = {"va": [os.path.basename(deep), "0007.jpg"], "vh": [f"frames/vh/{i:04d}.jpg" for i in range(0, 200, 40)]}
    allowed = {("va", deep), ("va", "frames/va/0007.jpg")} | {("vh", f) for f in allow["vh"]}
    got = svc.search_top_frames_all(query, k * 3, names, allow_frames=allow)
    # "vb" is absent from the dict: excluded; fewer allowed frames than top_k * 3: all of them, the deep one too
    assert len(got) == len(allowed) and set(got) == allowed
    scores = [_score(svc, query, v, f) for v, f in got]
    assert all(a >= b for a, b in zip(scores, scores[1:]))
    assert svc.search_top_frames_all(query, 3, names, allow_frames=allow) == got[:3]
    assert svc.search_top_frames_all(query, 5, names, allow_frames={}) == []


def test_service_missing_file_and_invalidation(service):
    svc = service
    assert svc.search_top_frames_all("anything", 5, ["va", "missing_video"]) == []
    assert svc.search_top_frames_all("anything", 5, []) == []
    got = svc.search_top_frames_all("anything", 5, ["va", "vb"])
    assert len(got) == 5
    lib = svc._library[3]
    path = svc.path_service.get_embeddings_path("vb")
    rows = np.load(path)
    np.save(path, rows[::-1].copy())
    os.utime(path, (1, 1))                                            # another mtime: the library is rebuilt
    again = svc.search_top_frames_all("anything", 5, ["va", "vb"])
    assert svc._library[3] is not lib
    flip = {f"frames/vb/{i:04d}.jpg": f"frames/vb/{149 - i:04d}.jpg" for i in range(150)}
    assert again == [(v, flip[f]) if v == "vb" else (v, f) for v, f in got]
