"""GPU: mi_rank_exclude (csrc/rank_exclude.hip), the exclusion-mask pass, and the filled distinct
top-k built on it (retrieval.rank_topk_distinct(fill=True), FrameLibrary.search(fill=True), the
service), against tests/exclude_ref.py (NumPy float64): mask bits and counts exactly, filled hits
and counts exactly against the collapse walk over the GPU's own full ranking, scores bitwise.
Every case keeps the cosines it decides on away from the threshold by far more than the kernel's
f32 error (2 D 2^-24: 6.1e-5 at D = 512, 1.2e-4 at D = 1024): planted rows by 1e-2, the real rows
by 1e-4 (tests/test_exclude_host.py), asserted in float64 on the widened rows."""
import json
import os
import zlib

import numpy as np
import pytest

from collapse_ref import cosines
from exclude_ref import exclude_ref, fill_ref
from test_gpu_rank_collapse import _global, _t, _wide, planted

pytestmark = pytest.mark.gpu

NEG_INF_BITS = np.float32(float("-inf")).view(np.uint32)
BIG_N = 20_011


def _unpack(mask, n):
    """Packed device words -> bool [n]; the word count and the zero bits at and beyond n checked."""
    import torch
    assert mask.dtype == torch.int32 and mask.shape == ((n + 31) // 32,)
    bits = np.unpackbits(mask.cpu().numpy().view(np.uint8), bitorder="little")
    assert not bits[n:].any(), "bits of rows >= N must be 0"
    return bits[:n].astype(bool)


def _hit_margin(rows64, hits64):
    """|cos| table of rows x hits in float64 (NaN where a norm is zero or not finite)."""
    with np.errstate(all="ignore"):
        nr, nh = np.sqrt((rows64 * rows64).sum(axis=1)), np.sqrt((hits64 * hits64).sum(axis=1))
        return (rows64 @ hits64.T) / np.outer(nr, nh)


def _check(corpus, hits, hit_index, theta, vis=None, base=0, how="bool", margin=1e-2):
    """exclude_similar against exclude_ref.  hits: device [H, D]; hit_index: host int64 global
    indices or None; vis: host bool [N] or None; how: the mask goes in as a bool tensor ("bool"),
    as packed words ("packed") or as packed words that are also the output ("inplace")."""
    import torch
    from miclip import retrieval
    n = corpus.shape[0]
    rows64, hits64 = _wide(corpus), _wide(hits)
    d = np.abs(_hit_margin(rows64, hits64) - theta)
    assert not np.isfinite(d).any() or d[np.isfinite(d)].min() >= margin, d[np.isfinite(d)].min()
    rel = None if hit_index is None else np.asarray(hit_index, np.int64) - base
    want_mask, want_count = exclude_ref(rows64, hits64, rel, theta, vis)
    row_mask = out = None
    if vis is not None:
        row_mask = torch.from_numpy(np.asarray(vis, bool)).to(corpus.device)
        if how != "bool":
            row_mask = retrieval.pack_row_mask(row_mask)
            before = row_mask.clone()
        if how == "inplace":
            out = row_mask
    mask, count = retrieval.exclude_similar(corpus, hits, None if hit_index is None else torch.from_numpy(
        np.asarray(hit_index, np.int64)), theta, row_mask=row_mask, index_base=base, out=out, count=True)
    if how == "inplace" and vis is not None:
        assert mask.data_ptr() == row_mask.data_ptr()
    elif how == "packed" and vis is not None:
        assert torch.equal(row_mask, before)                       # the input words are left alone
    assert count.dtype == torch.int32
    got = _unpack(mask, n)
    np.testing.assert_array_equal(got, want_mask)
    np.testing.assert_array_equal(count.cpu().numpy(), want_count)
    seen = np.ones(n, bool) if vis is None else np.asarray(vis, bool)
    assert int(want_count.sum()) == int((seen & ~want_mask).sum())
    nomask, nocount = retrieval.exclude_similar(corpus, hits, None if hit_index is None else torch.from_numpy(
        np.asarray(hit_index, np.int64)), theta, row_mask=None if vis is None else torch.from_numpy(
        np.asarray(vis, bool)).to(corpus.device), index_base=base)
    assert nocount is None and torch.equal(nomask, mask)           # count=False: the same mask
    return got, count.cpu().numpy()


# ------------------------------------------------------------------ 1. shapes, widths, dtypes
BASES = {32: 0, 512: 1000, 768: 7, 1024: 1 << 33}


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("D", [32, 512, 768, 1024])
def test_shapes(gpu, D, dtype):
    """N = 1 (a partial word), 33 (a second word with one live bit), 385 (crosses a 384-row
    workgroup range), 1000 and 20 011 (several workgroups, a ragged tail); H = 1, 5, 32 and 40
    (two chained calls)."""
    big, small = _t(gpu, planted(D, n=BIG_N, seed=3)[0], dtype), _t(gpu, planted(D, n=1000, seed=3)[0], dtype)
    base = BASES[D]
    rng = np.random.default_rng(D)
    removed = 0
    for n in (1, 33, 385, 1000, BIG_N):
        corpus = big if n == BIG_N else small[:n].contiguous()
        for H, masked in ((32, False), (40, True)) if n == BIG_N else [(H, m) for H in (1, 5, 32, 40)
                                                                         for m in (False, True)]:
            idx = rng.integers(0, n, H)                             # with repeats when H > n
            vis = rng.random(n) < 0.7 if masked else None
            got, count = _check(corpus, corpus.index_select(0, _t(gpu, idx)).float(), idx + base, 0.9, vis, base,
                                how="packed")
            removed += int(count.sum())
            if n >= 1000:
                assert (count > 1).any()                            # clusters, not only the hits themselves
    assert removed > 100


MANY_N, MANY_D = 600_011, 32


def _many_tiles():
    """(rows f32 [600 011, 32], cluster id): 2 000 clusters of ~300 rows, rows interleaved."""
    rng = np.random.default_rng(41)
    centres = rng.standard_normal((2000, MANY_D))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    ids = rng.integers(0, 2000, MANY_N)
    rows = centres[ids] + rng.standard_normal((MANY_N, MANY_D)) * (0.08 / np.sqrt(MANY_D))
    rows *= rng.uniform(0.5, 3.0, (MANY_N, 1))
    return rows.astype(np.float32), ids


def test_several_tiles_per_wave(gpu):
    """Up to 196 608 rows a workgroup's range is 384 rows and each of its 12 waves scores one tile.
    At 600 011 rows the 512 workgroups take 1 536 rows each, so a wave walks four tiles (t = 0 .. 3,
    rows (wave + 12 t) 32 of the range): the tile cursors, the word of tile t > 0, the ring across
    tile boundaries and the reused norms are what this case adds.  The mask kills tile t = 1 of every
    wave in the even workgroups (a dead tile between two live tiles of one wave), 30 % of the other
    words and one whole workgroup; the last word is ragged (11 rows); the hits lie in tiles t >= 1."""
    chunks = max(min((MANY_N + 383) // 384, 512), (MANY_N + 24575) // 24576)
    rpw = ((MANY_N + chunks - 1) // chunks + 383) // 384 * 384
    assert rpw == 1536 and MANY_N % 32 == 11                       # four tiles per wave, a ragged tail
    rows, ids = _many_tiles()
    corpus = _t(gpu, rows)
    rng = np.random.default_rng(42)
    words = (MANY_N + 31) // 32
    w = np.arange(words)
    wg, t = w // 48, (w % 48) // 12                                 # the word's workgroup and tile ordinal
    live = rng.random(words) < 0.7
    live[(wg % 2 == 0) & (t == 1)] = False
    live[(wg % 2 == 0) & ((t == 0) | (t == 2))] = True
    live[wg == 100] = False
    live[-1] = True
    vis = np.repeat(live, 32)[:MANY_N] & (rng.random(MANY_N) < 0.7)
    vis[-11:] = True
    tile = (np.arange(MANY_N) % rpw) // 384
    idx = rng.choice(np.flatnonzero(vis & (tile >= 1)), 40, replace=False)   # 40 hits: two chained calls
    idx[0] = MANY_N - 3                                             # one hit in the ragged last word
    assert (tile[idx] >= 1).all() and len(set(tile[idx].tolist())) == 3
    got, count = _check(corpus, corpus.index_select(0, _t(gpu, idx)), idx + 9, 0.9, vis, 9, how="inplace")
    assert (count > 50).sum() >= 20                                 # whole clusters, from every tile ordinal
    gone = vis & ~got
    assert all(gone[tile == o].sum() > 100 for o in range(4)) and not got[~vis].any()
    # everything visible: no word is skipped
    idx = rng.choice(np.flatnonzero(tile >= 2), 32, replace=False)
    _check(corpus, corpus.index_select(0, _t(gpu, idx)), idx, 0.9, None)


# ------------------------------------------------------------------ 2. the mask that comes in
@pytest.fixture(scope="module")
def thousand(gpu):
    rows, ids = planted(512, n=1000, seed=3)
    corpus = _t(gpu, rows)
    idx = np.random.default_rng(8).permutation(1000)[:32]
    return corpus, idx, corpus.index_select(0, _t(gpu, idx))


@pytest.mark.parametrize("how", ["bool", "packed", "inplace"])
def test_mask_in(thousand, how):
    corpus, idx, hits = thousand
    rng = np.random.default_rng(5)
    _check(corpus, hits, idx, 0.9, None)
    _check(corpus, hits, idx, 0.9, rng.random(1000) < 0.5, how=how)
    # all zero: nothing visible, nothing removed, nothing counted
    got, count = _check(corpus, hits, idx, 0.9, np.zeros(1000, bool), how=how)
    assert not got.any() and not count.any()
    # whole dead tiles, and a whole dead workgroup (rows 384 .. 767 of three 384-row ranges)
    vis = rng.random(1000) < 0.6
    vis[64:192] = False
    vis[384:800] = False
    got, count = _check(corpus, hits, idx, 0.9, vis, how=how)
    assert not got[384:800].any() and count.sum() > 0
    # one live bit in an otherwise dead corpus
    vis = np.zeros(1000, bool)
    vis[idx[3]] = True
    got, count = _check(corpus, hits, idx, 0.9, vis, how=how)
    assert not got.any() and count.sum() == 1


def test_index_base_and_hit_index(gpu, thousand):
    corpus, idx, hits = thousand
    for base in (5, 1 << 40, -300):
        _check(corpus, hits, idx + base, 0.9, None, base)
    # no indices at all; indices that name no row (before the base, past the rows, another corpus')
    _check(corpus, hits, None, 0.9, None, 77)
    far = idx.astype(np.int64) + 77
    far[[0, 5, 9, 31]] = [76, 77 + 1000, -1, 1 << 50]
    _check(corpus, hits, far, 0.9, None, 77)
    # foreign hit vectors naming rows they are not similar to: the rows go, each counted once
    foreign = _t(gpu, planted(512, n=5, seed=77)[0])
    named = np.array([10, 11, 500, 999, 10], np.int64)
    got, count = _check(corpus, foreign, named, 0.9, None, 0)
    assert count.tolist() == [1, 1, 1, 1, 0] and (~got).sum() == 4


def test_zero_rows_zero_hit_nan_row(gpu):
    rows = planted(512, n=300, seed=3)[0].copy()
    rows[[7, 31]] = 0.0
    rows[50, 3] = np.nan
    rows[51, 500] = np.inf
    corpus = _t(gpu, rows)
    idx = np.array([7, 100, 50], np.int64)                          # a zero-norm hit, a plain one, a NaN hit
    got, count = _check(corpus, corpus.index_select(0, _t(gpu, idx)), idx, 0.9, None)
    assert count[0] == 1 and count[2] == 1 and not got[7] and got[31] and not got[50] and got[51]
    # the same hits unnamed: the zero-norm and the NaN hit remove nothing
    got, count = _check(corpus, corpus.index_select(0, _t(gpu, idx)), None, 0.9, None)
    assert count[0] == 0 and count[2] == 0 and got[7] and got[50] and count[1] >= 1


def test_theta_minus_two_removes_every_valid_row(gpu, thousand):
    corpus, idx, hits = thousand
    rows = corpus.clone()
    rows[[3, 640]] = 0.0
    rows[900, 0] = float("nan")
    vis = np.random.default_rng(2).random(1000) < 0.8
    vis[[3, 640, 900, 901]] = True
    assert idx[0] not in (3, 640, 900)
    got, count = _check(rows, hits, None, -2.0, vis)
    assert got.sum() == 3 and got[[3, 640, 900]].all()              # only the invalid rows stay
    assert count[0] == vis.sum() - 3 and not count[1:].any()        # all attributed to slot 0


# ------------------------------------------------------------------ 3. real rows
def _fill_expected(rows64, s_full, i_full, k, theta, base=0):
    """fill_ref per query over a full ranking (s f32, i int64 [Q, n], host; -1 = empty) ->
    (score bits uint32 [Q, k], index, count)."""
    Q = i_full.shape[0]
    bits = np.ascontiguousarray(s_full).view(np.uint32)
    es = np.full((Q, k), NEG_INF_BITS, np.uint32)
    ei = np.full((Q, k), -1, np.int64)
    ec = np.zeros((Q, k), np.int32)
    for q in range(Q):
        ranking = i_full[q][i_full[q] >= 0] - base
        hit, ec[q] = fill_ref(rows64, ranking, k, theta)
        for t in np.flatnonzero(hit >= 0):
            j = int(np.flatnonzero(ranking == hit[t])[0])
            es[q, t], ei[q, t] = bits[q, j], hit[t] + base
    return es, ei, ec


def _same_fill(got, want, what=""):
    import torch
    gs, gi, gc = got
    assert gs.dtype == torch.float32 and gi.dtype == torch.int64 and gc.dtype == torch.int32
    np.testing.assert_array_equal(gi.cpu().numpy(), want[1], err_msg=f"index {what}")
    np.testing.assert_array_equal(gc.cpu().numpy(), want[2], err_msg=f"count {what}")
    np.testing.assert_array_equal(gs.contiguous().cpu().numpy().view(np.uint32), want[0], err_msg=f"score bits {what}")


@pytest.fixture(scope="module")
def real(gpu):
    from conftest import golden
    from miclip import retrieval
    g = golden("rank_video_test_4.npz")
    rows = np.asarray(g["corpus"], np.float32)
    corpus = _t(gpu, rows)
    s, i = retrieval.rank_topk(corpus, corpus, rows.shape[0])       # every row as a query: the full ranking
    return corpus, rows.astype(np.float64), s.cpu().numpy(), i.cpu().numpy(), _t(gpu, np.asarray(g["queries"],
                                                                                              np.float32))


@pytest.mark.parametrize("theta", [0.85, 0.9, 0.95])
def test_real_rows_exclude_the_filled_hits(real, theta):
    from miclip import retrieval
    corpus, rows64, _, _, queries = real
    assert queries.shape[0] == 8
    _, hit, count = retrieval.rank_topk_distinct(corpus, queries, 10, theta, fill=True)
    assert (hit >= 0).all()
    for q in range(8):
        idx = hit[q].cpu().numpy()
        _, c = _check(corpus, corpus.index_select(0, hit[q]), idx, theta, None, margin=1e-4)
        np.testing.assert_array_equal(c, count[q].cpu().numpy())     # the filled search's counts are these


@pytest.mark.parametrize("theta,k,pool", [(0.9, 10, 10), (0.9, 20, 20), (0.85, 16, 16)])
def test_fill_real_rows_every_query(real, theta, k, pool):
    """Every row as a query (231 / 282 / 364 of the 387 need a second round at these settings,
    tests/test_exclude_host.py): hits and counts are the collapse walk over the GPU's own full
    ranking, scores bitwise that ranking's."""
    from miclip import retrieval
    corpus, rows64, s_full, i_full, _ = real
    short = retrieval.rank_topk_distinct(corpus, corpus, k, theta, pool=pool)
    got = retrieval.rank_topk_distinct(corpus, corpus, k, theta, pool=pool, fill=True)
    _same_fill(got, _fill_expected(rows64, s_full, i_full, k, theta), f"theta {theta} k {k} pool {pool}")
    refilled = int(((short[1] < 0).any(dim=1) & (got[1] >= 0).sum(dim=1).gt((short[1] >= 0).sum(dim=1))).sum())
    print(f"theta {theta} k {k} pool {pool}: {refilled} of {corpus.shape[0]} queries gained hits from the refill")
    assert refilled >= 100


def test_fill_changes_nothing_when_the_pool_suffices(real):
    """Pool 30, k = 10, theta 0.9: no query under-fills (tests/test_exclude_host.py)."""
    import torch
    from miclip import retrieval
    corpus = real[0]
    s0, i0, _, _ = retrieval.rank_topk_distinct(corpus, corpus, 10, 0.9)
    s1, i1, _ = retrieval.rank_topk_distinct(corpus, corpus, 10, 0.9, fill=True)
    assert (i0 >= 0).all() and torch.equal(i0, i1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32))


# ------------------------------------------------------------------ 4. built cases
def clusters(D, sizes, seed, noise=0.05):
    """(rows f32 [sum sizes, D], cluster id): near-orthogonal centres plus small noise, row lengths
    between 0.5 and 3, rows interleaved; pairs inside a cluster at cosine >= 0.97, others <= 0.6."""
    rng = np.random.default_rng(seed)
    centres = np.linalg.qr(rng.standard_normal((D, len(sizes))))[0].T
    ids = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    rows = centres[ids] + rng.standard_normal((len(ids), D)) * (noise / np.sqrt(D))
    rows *= rng.uniform(0.5, 3.0, (len(ids), 1))
    return rows.astype(np.float32), ids


def _assert_cluster_margin(rows64, ids, theta=0.9, margin=1e-2):
    cos, valid = cosines(rows64)
    same = ids[:, None] == ids[None, :]
    off = ~np.eye(len(ids), dtype=bool)
    assert valid.all() and cos[same & off].min(initial=1.0) >= 0.97 and cos[~same].max() <= 0.6
    assert np.abs(cos[off] - theta).min() >= margin


def test_static_corpus(gpu):
    """2 000 copies of one row and 5 mutually dissimilar rows: the un-filled search returns one
    frame, the filled one k = 4, the first with the 2 000 copies counted."""
    import torch
    from miclip import retrieval
    six, ids = clusters(512, [1] * 6, seed=4)
    _assert_cluster_margin(six.astype(np.float64), ids)
    rows = np.repeat(six[:1], 2005, axis=0)
    others = [3, 500, 1000, 1500, 2004]
    rows[others] = six[1:]
    corpus = _t(gpu, rows)
    q = _t(gpu, six[:1] + 0.02 * six[1:].sum(axis=0, keepdims=True))
    base = 1000
    s0, i0, c0, _ = retrieval.rank_topk_distinct(corpus, q, 4, 0.9, pool=64, index_base=base)
    assert (i0[0] >= 0).sum() == 1 and c0[0].tolist() == [64, 0, 0, 0]
    s1, i1, c1 = retrieval.rank_topk_distinct(corpus, q, 4, 0.9, pool=64, fill=True, index_base=base)
    assert (i1[0] >= 0).all() and c1[0].tolist() == [2000, 1, 1, 1]
    assert i1[0, 0] == i0[0, 0] == base and set((i1[0, 1:] - base).tolist()) <= set(others)
    s_full, i_full = retrieval.rank_topk(corpus, q, 2005, index_base=base)
    _same_fill((s1, i1, c1), _fill_expected(rows.astype(np.float64), s_full.cpu().numpy(), i_full.cpu().numpy(), 4,
                                            0.9, base))
    assert torch.equal(s1[0, :1].view(torch.int32), s0[0, :1].view(torch.int32))


def test_exhaustion(gpu):
    """200 rows in 6 clusters, k = 10: 6 hits, 4 empty slots, the counts sum to 200."""
    from miclip import retrieval
    rows, ids = clusters(512, [90, 50, 30, 15, 10, 5], seed=6)
    _assert_cluster_margin(rows.astype(np.float64), ids)
    corpus = _t(gpu, rows)
    q = _t(gpu, rows[[int(np.flatnonzero(ids == 0)[0]), int(np.flatnonzero(ids == 5)[0])]])
    s, i, c = retrieval.rank_topk_distinct(corpus, q, 10, 0.9, fill=True)
    assert ((i >= 0).sum(dim=1) == 6).all() and (i[:, 6:] == -1).all() and (c[:, 6:] == 0).all()
    assert (s[:, 6:] == float("-inf")).all() and c.sum(dim=1).tolist() == [200, 200]
    assert sorted(c[0].tolist()) == [0, 0, 0, 0, 5, 10, 15, 30, 50, 90] and c[0, 0] == 90 and c[1, 0] == 5
    s_full, i_full = retrieval.rank_topk(corpus, q, 200)
    _same_fill((s, i, c), _fill_expected(rows.astype(np.float64), s_full.cpu().numpy(), i_full.cpu().numpy(), 10, 0.9))
    assert ((retrieval.rank_topk_distinct(corpus, q, 10, 0.9)[1] >= 0).sum(dim=1) < 6).any()   # the pool alone: fewer


def test_one_underfilled_query_among_three(gpu):
    """Q = 3, pool 8, k = 5: the query inside a large cluster refills; the two that had k hits
    keep their scores (bit for bit) and indices."""
    import torch
    from miclip import retrieval
    rows, ids = planted(512)
    corpus = _t(gpu, rows)
    s0, i0, _, _ = retrieval.rank_topk_distinct(corpus, corpus, 5, 0.9, pool=8)
    nh = (i0 >= 0).sum(dim=1).cpu().numpy()
    under, full = np.flatnonzero(nh < 5), np.flatnonzero(nh == 5)
    assert len(under) >= 1 and len(full) >= 2
    pick = _t(gpu, np.array([full[0], under[0], full[-1]], np.int64))
    q = corpus.index_select(0, pick)
    s1, i1, c1 = retrieval.rank_topk_distinct(corpus, q, 5, 0.9, pool=8, fill=True)
    for a in (0, 2):
        assert torch.equal(i1[a], i0[pick[a]]) and torch.equal(s1[a].view(torch.int32), s0[pick[a]].view(torch.int32))
    assert (i1[1] >= 0).all() and torch.equal(i1[1, :nh[under[0]]], i0[pick[1], :nh[under[0]]])
    s_full, i_full = retrieval.rank_topk(corpus, q, 200)
    _same_fill((s1, i1, c1), _fill_expected(_wide(corpus), s_full.cpu().numpy(), i_full.cpu().numpy(), 5, 0.9))


def test_fill_under_a_row_mask(gpu):
    """row_mask=: the filled search over the visible rows equals the walk over the gathered rows."""
    import torch
    from miclip import retrieval
    rows, ids = planted(512)
    corpus = _t(gpu, rows)
    vis = np.random.default_rng(12).random(200) < 0.6
    where = np.flatnonzero(vis)
    q = _t(gpu, planted(512, seed=23)[0][:6])
    base = 40
    got = retrieval.rank_topk_distinct(corpus, q, 10, 0.9, pool=10, fill=True, row_mask=_t(gpu, vis), index_base=base)
    s_g, i_g = retrieval.rank_topk(_t(gpu, rows[where]), q, len(where))   # the gathered rows' full ranking
    i_full = where[i_g.cpu().numpy()] + base                              # (the gather keeps the index order)
    _same_fill(got, _fill_expected(_wide(corpus), s_g.cpu().numpy(), i_full, 10, 0.9, base))
    short = retrieval.rank_topk_distinct(corpus, q, 10, 0.9, pool=10, row_mask=_t(gpu, vis), index_base=base)
    assert ((short[1] >= 0).sum(dim=1) < (got[1] >= 0).sum(dim=1)).any()   # the refill did something
    packed = retrieval.pack_row_mask(_t(gpu, vis))
    keep = packed.clone()
    again = retrieval.rank_topk_distinct(corpus, q, 10, 0.9, pool=10, fill=True, row_mask=packed, index_base=base)
    assert torch.equal(packed, keep) and all(torch.equal(a, b) for a, b in zip(got[1:], again[1:]))


# ------------------------------------------------------------------ 5. the library
@pytest.fixture(scope="module")
def library(gpu):
    from miclip import library as L
    rows, ids = clusters(512, [6] * 10, seed=9)
    lib = L.FrameLibrary(device=gpu)
    lib.add("h", rows[:30].astype(np.float16))       # float16 video: global rows 30 .. 59
    lib.add("a", rows[30:])                          # f32 video: global rows 0 .. 29
    gid = np.concatenate([ids[30:], ids[:30]])       # cluster id by global index
    rows64 = np.vstack([_wide(g.corpus()) for g in lib._groups])
    _assert_cluster_margin(rows64, gid)
    assert all(((gid[:30] == c).any() and (gid[30:] == c).any()) for c in range(10))   # clusters span both videos
    return lib, rows64, gid, _t(gpu, rows[[0, 7, 31, 44]])


@pytest.mark.parametrize("kw", [dict(), dict(allow={"a": True, "h": np.arange(0, 30, 2)}), dict(video="h"),
                                dict(video=["a", None, "h", None])])
def test_library_fill(library, kw):
    """One f32 and one float16 video, pool 6, k = 5: the pool holds one cluster, the refill finds
    the rest; against the walk over the full visible ranking (at most 60 rows: one plain search)."""
    lib, rows64, gid, q = library
    k, pool = 5, 6
    ps, pv, pr = lib.search(q, 60, **kw)                                # every visible row, ranked
    i_full = _global(lib, pv, pr)
    want = _fill_expected(rows64, ps.cpu().numpy(), i_full, k, 0.9)
    short = lib.search(q, k, distinct=0.9, pool=pool, **kw)
    s, vid, row, count = lib.search(q, k, distinct=0.9, pool=pool, fill=True, **kw)
    np.testing.assert_array_equal(_global(lib, vid, row), want[1])
    np.testing.assert_array_equal(count.cpu().numpy(), want[2])
    np.testing.assert_array_equal(s.contiguous().cpu().numpy().view(np.uint32), want[0])
    assert ((short[1] >= 0).sum(dim=1) < k).any() and (vid >= 0).all()   # under-filled before, full now
    hits = want[1]
    for h in hits:
        assert len(set(gid[h].tolist())) == k                          # one frame per cluster
    if "video" not in kw:
        assert (hits < 30).any() and (hits >= 30).any()                 # hits from both groups
    if not kw:
        assert (want[2] == 6).all()                                     # a cluster's rows in both groups, all counted


def test_library_fill_needs_distinct(library):
    from miclip import _native
    with pytest.raises(_native.MiClipError):
        library[0].search(library[3], 5, fill=True)


# ------------------------------------------------------------------ 6. the service
SVC_N = 130


@pytest.fixture()
def service(gpu, tmp_path, monkeypatch):
    import torch
    from miclip import api, service as S, weights
    from test_gpu_rank_filter import Cache, Data, Paths
    root = tmp_path / "state"
    (root / "metadata").mkdir(parents=True)
    (root / "embedding").mkdir(parents=True)
    paths = Paths(str(root))
    svc = S.EmbeddingService(Cache(), paths, Data(paths), device="cuda", model_name="test-small")
    cfg = svc.original_model.cfg
    monkeypatch.setattr(api, "tokenize", lambda texts, *a, **k: torch.from_numpy(np.concatenate(
        [weights.synthetic_tokens(1, cfg.context_length, cfg.vocab_size, seed=zlib.crc32(t.encode()) % 1000)
         for t in texts])))
    # a static shot: the frame the query describes, repeated, and 12 other moments
    still = np.asarray(svc.get_text_features("a static shot", "still"), np.float32).reshape(-1)
    other, ids = clusters(cfg.embed_dim, [1] * 13, seed=21)
    other = other[np.argsort(-np.abs(other @ still))][1:]             # drop the one closest to the still
    rows = np.repeat(still[None] * 2.0, SVC_N, axis=0)
    where = np.arange(5, SVC_N, 10)[:12]
    rows[where] = other
    cos = cosines(np.vstack([still[None], other]).astype(np.float64))[0]
    assert np.abs(cos[np.triu_indices(13, 1)]).max() <= 0.6
    np.save(paths.get_embeddings_path("still"), rows)
    with open(paths.get_metadata_path("still"), "w") as f:
        json.dump([{"frame": f"frames/still/{i:04d}.jpg"} for i in range(SVC_N)], f)
    return svc, rows, where


def _num(frame):
    return int(os.path.basename(frame)[:4])


def test_service_fill(service):
    svc, rows, where = service
    k = 5
    plain = svc.search_top_frames_distinct("a static shot", k, "still")
    assert [_num(f) for f in plain] == [0]                              # the pool of 15 is one frame
    filled = svc.search_top_frames_distinct("a static shot", k, "still", fill=True)
    assert len(filled) == k and _num(filled[0]) == 0 and {_num(f) for f in filled[1:]} <= set(where.tolist())
    # keyed separately in the cache, each served from it afterwards
    assert svc.search_top_frames_distinct("a static shot", k, "still") == plain
    assert svc.search_top_frames_distinct("a static shot", k, "still", fill=True) == filled
    keys = [key for key in svc.cache_service.d if key[0] == "s"]
    assert sum(key[1].endswith("_fill") for key in keys) == 1 and len(keys) == 2
    # with groups: every frame of the video collapsed into the hit, in frame order
    groups = svc.search_top_frames_distinct("a static shot", k, "still", with_groups=True, fill=True)
    assert [g[0] for g in groups] == filled
    assert [_num(f) for f in groups[0][1]] == [i for i in range(1, SVC_N) if i not in set(where.tolist())]
    assert all(g[1] == [] for g in groups[1:])
    by_image = svc.search_top_frames_by_image_distinct(rows[0], k, "still", fill=True)
    assert by_image == filled and len(svc.search_top_frames_by_image_distinct(rows[0], k, "still")) == 1
    # errors are swallowed
    assert svc.search_top_frames_distinct("a static shot", k, "missing_video", fill=True) == []
    assert svc.search_top_frames_by_image_distinct(rows[0], k, "missing_video", fill=True, with_groups=True) == []
