"""GPU: mi_rank_collapse (csrc/rank_collapse.hip), the distinct top-k of a ranked candidate list,
against tests/collapse_ref.py (the walk in NumPy float64) on the pool the GPU ranking produced:
index, count and slot exactly, scores bitwise against the pool's scores.  Every case keeps the
pairs' cosines away from the threshold by far more than the kernel's f32 error (2 D 2^-24:
6.1e-5 at D = 512, 1.2e-4 at D = 1024), which each test asserts in float64 on the widened rows."""
import functools
import json
import os
import zlib

import numpy as np
import pytest

from collapse_ref import collapse_ref, cosines, min_margin

pytestmark = pytest.mark.gpu

NEG_INF = float("-inf")
THETA25 = float(np.cos(np.deg2rad(25.0)))


def _t(gpu, a, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return t if dtype is None else t.to(getattr(torch, dtype))


def _wide(t):
    """The stored rows widened exactly, float64 on the host."""
    return t.float().cpu().numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def planted(D, n=200, seed=11):
    """(rows f32 [n, D], cluster id [n]): cluster centres plus small noise, cluster sizes 1-7,
    rows interleaved, row lengths between 0.5 and 3."""
    rng = np.random.default_rng(seed + D)
    sizes = []
    while sum(sizes) < n:
        sizes.append(int(rng.integers(1, 8)))
    sizes[-1] -= sum(sizes) - n
    ids = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    centres = rng.standard_normal((len(sizes), D))
    centres /= np.linalg.norm(centres, axis=1, keepdims=True)
    rows = centres[ids] + rng.standard_normal((n, D)) * (0.08 / np.sqrt(D))
    rows *= rng.uniform(0.5, 3.0, (n, 1))
    return rows.astype(np.float32), ids


def _assert_planted_margin(rows64, ids, theta=0.9, margin=1e-2):
    cos, valid = cosines(rows64)
    same = ids[:, None] == ids[None, :]
    off = ~np.eye(len(ids), dtype=bool)
    assert valid.all()
    assert cos[same & off].min() >= 0.97 and cos[~same].max() <= 0.8
    assert np.abs(cos[off] - theta).min() >= margin


def _expected(rows64, s, i, k, theta, base=0):
    """collapse_ref per query on the pool (s f32, i int64 [Q, P], host) -> (score bits uint32 [Q, k],
    index, count, slot)."""
    Q, P = i.shape
    bits = s.view(np.uint32)
    es = np.full((Q, k), np.float32(NEG_INF).view(np.uint32), np.uint32)
    ei = np.full((Q, k), -1, np.int64)
    ec = np.zeros((Q, k), np.int32)
    eslot = np.full((Q, P), -1, np.int32)
    for q in range(Q):
        rel = np.where(i[q] >= 0, i[q] - base, -1)
        hit, ec[q], eslot[q] = collapse_ref(rows64, rel, k, theta)
        for t in range(k):
            if hit[t] >= 0:
                j = int(np.flatnonzero(eslot[q] == t)[0])   # the hit is the first candidate of its slot
                es[q, t], ei[q, t] = bits[q, j], i[q, j]
                assert hit[t] == rel[j]
    return es, ei, ec, eslot


def _same(got, want, what=""):
    import torch
    gs, gi, gc, gslot = got
    assert gs.dtype == torch.float32 and gi.dtype == torch.int64 and gc.dtype == torch.int32 and \
        gslot.dtype == torch.int32
    np.testing.assert_array_equal(gi.cpu().numpy(), want[1], err_msg=f"index {what}")
    np.testing.assert_array_equal(gc.cpu().numpy(), want[2], err_msg=f"count {what}")
    np.testing.assert_array_equal(gslot.cpu().numpy(), want[3], err_msg=f"slot {what}")
    np.testing.assert_array_equal(gs.contiguous().cpu().numpy().view(np.uint32), want[0], err_msg=f"score bits {what}")


def _collapse_and_check(corpus, s, i, k, theta, base=0, corpus2=None, what=""):
    from miclip import retrieval
    got = retrieval.collapse_topk(corpus, s, i, k, theta, index_base=base, corpus2=corpus2)
    rows64 = _wide(corpus) if corpus2 is None else np.vstack([_wide(corpus), _wide(corpus2)])
    want = _expected(rows64, s.cpu().numpy(), i.cpu().numpy(), k, theta, base)
    _same(got, want, what)
    return got, want


# ------------------------------------------------------------------ 1. identity
def test_identity_thresholds(gpu):
    import torch
    from miclip import retrieval
    rows, ids = planted(512)
    corpus = _t(gpu, rows)
    q = _t(gpu, planted(512, seed=5)[0][:5])
    P, k = 30, 10
    s, i = retrieval.rank_topk(corpus, q, P, index_base=3)
    i[1, 4] = -1                                            # empty slots inside a list
    i[1, 17] = -1
    # nothing is similar at theta = 2: the first k non-empty candidates, one each
    (gs, gi, gc, gslot), _ = _collapse_and_check(corpus, s, i, k, 2.0, base=3, what="theta 2")
    assert torch.equal(gi[0], i[0, :k]) and (gc == 1).all()
    assert gslot[0].tolist() == list(range(k)) + [-1] * (P - k)
    assert gslot[1].tolist() == [0, 1, 2, 3, -1, 4, 5, 6, 7, 8, 9] + [-1] * (P - 11)
    # everything is similar at theta = -2: one hit holding every non-empty candidate
    (gs, gi, gc, gslot), _ = _collapse_and_check(corpus, s, i, k, -2.0, base=3, what="theta -2")
    assert torch.equal(gi[:, 0], i[:, 0]) and (gi[:, 1:] == -1).all() and (gs[:, 1:] == NEG_INF).all()
    assert gc[:, 0].tolist() == [P, P - 2, P, P, P] and (gc[:, 1:] == 0).all()
    assert (gslot[1] == torch.where(i[1] >= 0, 0, -1)).all()


# ------------------------------------------------------------------ 2. planted clusters
PK = [(1, 1), (31, 10), (32, 32), (33, 10), (64, 1), (64, 10), (64, 64)]
BASES = {32: 0, 512: 1000, 768: 7, 1024: 1 << 33}


@pytest.mark.parametrize("dtype", ["float32", "bfloat16", "float16"])
@pytest.mark.parametrize("D", [32, 512, 768, 1024])
def test_planted_clusters(gpu, D, dtype):
    from miclip import retrieval
    rows, ids = planted(D)
    corpus = _t(gpu, rows, dtype)
    rows64 = _wide(corpus)
    _assert_planted_margin(rows64, ids)
    base = BASES[D]
    q = _t(gpu, planted(D, seed=23)[0][:70])
    s64, i64 = retrieval.rank_topk(corpus, q, 64, index_base=base)
    for P, k in PK:
        # a prefix of a ranked list is a ranked list; fewer queries are a prefix of the batch
        s, i = s64[:, :P].contiguous(), i64[:, :P].contiguous()
        got = retrieval.collapse_topk(corpus, s, i, k, 0.9, index_base=base)
        want = _expected(rows64, s.cpu().numpy(), i.cpu().numpy(), k, 0.9, base)
        _same(got, want, f"P {P} k {k} Q 70")
        # one frame per cluster among the hits
        hit = got[1].cpu().numpy()
        for row in hit:
            c = ids[row[row >= 0] - base]
            assert len(set(c.tolist())) == len(c)
        for Q in (1, 33):
            _same(retrieval.collapse_topk(corpus, s[:Q], i[:Q], k, 0.9, index_base=base),
                  tuple(w[:Q] for w in want), f"P {P} k {k} Q {Q}")


# ------------------------------------------------------------------ 3. the chain
def test_chain_and_tie(gpu):
    a = np.deg2rad(np.array([0.0, 20.0, 40.0]))
    rows = np.zeros((3, 512), np.float32)
    rows[:, 100], rows[:, 301] = np.cos(a), np.sin(a)
    rows *= np.array([[1.0], [2.5], [0.3]], np.float32)
    corpus = _t(gpu, rows)
    assert min_margin(rows, [0, 1, 2], THETA25) > 3e-2
    i = _t(gpu, np.array([[0, 1, 2], [2, 1, 0], [1, 0, 2], [0, 2, 1]], np.int64))
    s = _t(gpu, np.tile(np.array([0.9, 0.8, 0.7], np.float32), (4, 1)))
    (gs, gi, gc, gslot), _ = _collapse_and_check(corpus, s, i, 3, THETA25)
    # a~b, b~c, a!~c: hits a (2) and c (1); mirrored; b first absorbs both; the tie goes to the lower slot
    assert gi.tolist() == [[0, 2, -1], [2, 0, -1], [1, -1, -1], [0, 2, -1]]
    assert gc.tolist() == [[2, 1, 0], [2, 1, 0], [3, 0, 0], [2, 1, 0]]
    assert gslot.tolist() == [[0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 1, 0]]
    assert gs[:, 0].tolist() == [np.float32(0.9)] * 4 and gs[0, 1] == np.float32(0.7) and gs[3, 1] == np.float32(0.8)


# ------------------------------------------------------------------ 4. empty slots
def test_empty_slots_from_the_filtered_pass(gpu):
    import torch
    from miclip import retrieval
    allrows, ids = planted(512)
    rows = allrows[np.unique(ids, return_index=True)[1][:5]].copy()  # five clusters
    rows[3] = rows[0] * 1.5 + planted(512, seed=2)[0][0] * 1e-2     # a near-copy of row 0
    corpus = _t(gpu, rows)
    q = _t(gpu, rows[[0, 1]])
    mask = torch.tensor([True, False, True, True, False], device=gpu)
    ranges = torch.tensor([[0, 5], [4, 4]], device=gpu)               # the second query sees nothing
    s, i = retrieval.rank_topk_filtered(corpus, q, 16, row_mask=mask, query_range=ranges)
    assert (i[0, 3:] == -1).all() and (i[1] == -1).all()
    assert min_margin(rows, [0, 2, 3], 0.9) > 1e-2
    (gs, gi, gc, gslot), _ = _collapse_and_check(corpus, s, i, 10, 0.9)
    assert sorted(gi[0, :2].tolist()) == [0, 2] and (gi[0, 2:] == -1).all()
    assert sorted(gc[0, :2].tolist()) == [1, 2] and (gc[0, 2:] == 0).all() and (gslot[0, 3:] == -1).all()
    assert (gi[1] == -1).all() and (gc[1] == 0).all() and (gs[1] == NEG_INF).all() and (gslot[1] == -1).all()


# ------------------------------------------------------------------ 5. zero rows
def test_zero_rows_first_one_hit_each(gpu):
    import torch
    from miclip import retrieval
    rows, ids = planted(512)
    rows = rows[:60].copy()
    rows[[7, 31]] = 0.0
    corpus = _t(gpu, rows)
    q = _t(gpu, planted(512, seed=9)[0][:3])
    s, i = retrieval.rank_topk(corpus, q, 40, nan_policy="first")
    assert i[:, :2].tolist() == [[7, 31]] * 3 and torch.isnan(s[:, :2]).all()
    (gs, gi, gc, gslot), _ = _collapse_and_check(corpus, s, i, 10, 0.9)
    assert gi[:, :2].tolist() == [[7, 31]] * 3 and (gc[:, :2] == 1).all() and torch.isnan(gs[:, :2]).all()
    assert (gslot[:, :2] == torch.tensor([0, 1], device=gpu, dtype=torch.int32)).all()
    # even at theta = -2 they absorb nothing and join nothing
    (gs, gi, gc, gslot), _ = _collapse_and_check(corpus, s, i, 10, -2.0)
    assert gc[:, :3].tolist() == [[1, 1, 38]] * 3 and (gi[:, 3:] == -1).all()


# ------------------------------------------------------------------ 6. two corpora
@pytest.mark.parametrize("first", ["float32", "float16"])
def test_two_corpora(gpu, first):
    import torch
    from miclip import retrieval
    rows, ids = planted(512)
    n0 = 120
    second = "float16" if first == "float32" else "bfloat16"
    c0, c1 = _t(gpu, rows[:n0], first), _t(gpu, rows[n0:], second)
    rows64 = np.vstack([_wide(c0), _wide(c1)])
    _assert_planted_margin(rows64, ids)
    assert len(set(ids[:n0]) & set(ids[n0:])) > 10                 # clusters span both corpora
    base = 50
    q = _t(gpu, planted(512, seed=23)[0][:9])
    s0, i0 = retrieval.rank_topk(c0, q, 40, index_base=base)
    s1, i1 = retrieval.rank_topk(c1, q, 40, index_base=base + n0)
    s, i = retrieval.merge_topk(torch.cat([s0, s1], 1), torch.cat([i0, i1], 1), 40)
    assert ((i >= base + n0).any(dim=1) & (i < base + n0).any(dim=1)).all()
    i[0, 1] = base + 200                                            # just past both corpora
    i[2, 0] = 1 << 40
    i[3, 5] = base - 1                                              # just before the first
    got, want = _collapse_and_check(c0, s, i, 10, 0.9, base=base, corpus2=c1, what=first)
    assert want[3][0, 1] == -1 and want[3][2, 0] == -1 and want[3][3, 5] == -1
    # without the second corpus its candidates are empty slots
    only0 = retrieval.collapse_topk(c0, s, i, 40, 0.9, index_base=base)   # k = P: no candidate is dropped
    assert ((only0[3] == -1) == ((i < base) | (i >= base + n0))).all()


# ------------------------------------------------------------------ 7. real rows
@pytest.fixture(scope="module")
def real(gpu):
    from conftest import golden
    from miclip import retrieval
    g = golden("rank_video_test_4.npz")
    rows = np.asarray(g["corpus"], np.float32)
    corpus = _t(gpu, rows)
    s, i = retrieval.rank_topk(corpus, corpus, 64)                  # every row as a query
    qs, qi = retrieval.rank_topk(corpus, _t(gpu, np.asarray(g["queries"], np.float32)), 60)
    return corpus, rows.astype(np.float64), (s, i), (qs, qi)


@pytest.mark.parametrize("theta", [0.85, 0.9, 0.95])
@pytest.mark.parametrize("P", [30, 64])
def test_real_rows_every_query(real, P, theta):
    corpus, rows64, (s, i), _ = real
    s, i = s[:, :P].contiguous(), i[:, :P].contiguous()
    got, want = _collapse_and_check(corpus, s, i, 10, theta, what=f"P {P} theta {theta}")
    changed = int((want[1] != i[:, :10].cpu().numpy()).any(axis=1).sum())
    print(f"P {P} theta {theta}: {changed} of {i.shape[0]} top-10 lists change")
    assert changed >= 100


@pytest.mark.parametrize("theta", [0.85, 0.9, 0.95])
def test_real_rows_fixture_queries(real, theta):
    corpus, rows64, _, (s, i) = real
    assert min(min_margin(rows64, p, theta) for p in i.cpu().numpy()) >= 1e-4
    _collapse_and_check(corpus, s, i, 10, theta, what=f"fixture queries theta {theta}")


# ------------------------------------------------------------------ 8. layers
def test_rank_topk_distinct_is_rank_then_collapse(gpu):
    import torch
    from miclip import retrieval
    rows, ids = planted(512)
    corpus = _t(gpu, rows)
    q = _t(gpu, planted(512, seed=23)[0][:6])
    for k, pool, want_pool in ((10, None, 30), (30, None, 64), (10, 50, 50), (5, 5, 5)):
        s, i = retrieval.rank_topk(corpus, q, want_pool, index_base=9)
        want = retrieval.collapse_topk(corpus, s, i, k, 0.9, index_base=9)
        got = retrieval.rank_topk_distinct(corpus, q, k, 0.9, pool=pool, index_base=9)
        for g, w in zip(got, want):
            assert g.shape == w.shape and torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g,
                                                      w.view(torch.int32) if w.dtype == torch.float32 else w)
    # the pool is clipped to the row count; slots past the rows stay empty
    small = corpus[:7].contiguous()
    s, i, c, slot = retrieval.rank_topk_distinct(small, q, 10, 2.0)
    assert s.shape == (6, 10) and slot.shape == (6, 10) and (i[:, 7:] == -1).all() and (c[:, :7] == 1).all()


@pytest.fixture(scope="module")
def library(gpu):
    from miclip import library as L
    rows, ids = planted(512)
    lib = L.FrameLibrary(device=gpu)
    lib.add("h", rows[:70].astype(np.float16))       # float16 video: global rows 130 .. 199
    lib.add("a", rows[70:150])                       # f32 videos: global rows 0 .. 129
    lib.add("b", rows[150:])
    gid = np.concatenate([ids[70:], ids[:70]])       # cluster id by global index
    rows64 = np.vstack([_wide(g.corpus()) for g in lib._groups])
    _assert_planted_margin(rows64, gid)
    return lib, rows64, gid, _t(gpu, planted(512, seed=23)[0][:5])


def _global(lib, vid, row):
    """(video_index, row) -> global index, -1 kept."""
    off = {lib.names.index(n): o for n, o, _, _ in lib.segments()}
    v, r = vid.cpu().numpy(), row.cpu().numpy()
    return np.where(v >= 0, np.vectorize(lambda x: off.get(x, 0))(v) + r, -1)


@pytest.mark.parametrize("kw", [dict(), dict(video="h"), dict(video=["a", None, "h", "b", None]),
                                dict(allow={"a": True, "h": np.arange(0, 70, 2)}), dict(pool=64)])
def test_library_distinct(library, kw):
    import torch
    lib, rows64, gid, q = library
    k = 10
    kw = dict(kw)
    pool = kw.pop("pool", None)
    P = pool or 30
    ps, pv, pr = lib.search(q, P, **kw)                             # the pool: the plain search
    s, vid, row, count = lib.search(q, k, distinct=0.9, pool=pool, **kw)
    assert count.dtype == torch.int32 and s.shape == vid.shape == row.shape == count.shape == (5, k)
    pi = _global(lib, pv, pr)
    want = _expected(rows64, ps.cpu().numpy(), pi, k, 0.9)
    np.testing.assert_array_equal(_global(lib, vid, row), want[1])
    np.testing.assert_array_equal(count.cpu().numpy(), want[2])
    np.testing.assert_array_equal(s.contiguous().cpu().numpy().view(np.uint32), want[0])
    for hits in want[1]:
        c = gid[hits[hits >= 0]]
        assert len(set(c.tolist())) == len(c)
    assert (want[2] > 1).any()                                       # something was collapsed
    # without `distinct` the call is what it was
    assert len(lib.search(q, k, **kw)) == 3


SVC_N, SVC_D = 150, 256


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
    assert cfg.embed_dim == SVC_D
    rows, ids = planted(SVC_D, n=SVC_N)
    _assert_planted_margin(rows.astype(np.float64), ids)
    np.save(paths.get_embeddings_path("dup"), rows)
    with open(paths.get_metadata_path("dup"), "w") as f:
        json.dump([{"frame": f"frames/dup/{i:04d}.jpg"} for i in range(SVC_N)], f)
    monkeypatch.setattr(api, "tokenize", lambda texts, *a, **k: torch.from_numpy(np.concatenate(
        [weights.synthetic_tokens(1, cfg.context_length, cfg.vocab_size, seed=zlib.crc32(t.encode()) % 1000)
         for t in texts])))
    return svc, rows, ids


def _cluster(ids, frame):
    return int(ids[int(os.path.basename(frame)[:4])])


def _check_service(ids, rows, pool_frames, plain, hits, groups, k):
    """hits / groups against collapse_ref on the pool the plain search returned."""
    pool_idx = [int(os.path.basename(f)[:4]) for f in pool_frames]
    hit, count, slot = collapse_ref(rows.astype(np.float64), pool_idx, k, 0.9)
    assert [int(os.path.basename(f)[:4]) for f in hits] == hit[hit >= 0].tolist()
    cl = [_cluster(ids, f) for f in hits]
    assert len(set(cl)) == len(cl)                                   # one frame per cluster
    assert [g[0] for g in groups] == hits
    for t, (frame, members) in enumerate(groups):
        want = [pool_frames[j] for j in np.flatnonzero(slot == t)]
        assert [frame] + members == want
        assert all(_cluster(ids, m) == _cluster(ids, frame) for m in members)
    assert any(g[1] for g in groups)
    pc = [_cluster(ids, f) for f in plain]
    assert plain == pool_frames[:k] and len(set(pc)) < len(pc)      # the plain search keeps its duplicates


def test_service_distinct_text(service):
    svc, rows, ids = service
    k = 10
    for query in ("a red car at night", "people walking"):
        plain = svc.search_top_frames(query, k, "dup")
        pool_frames = svc.search_top_frames(query, 30, "dup")
        hits = svc.search_top_frames_distinct(query, k, "dup")
        groups = svc.search_top_frames_distinct(query, k, "dup", with_groups=True)
        assert svc.search_top_frames_distinct(query, k, "dup") == hits             # the cached path
        _check_service(ids, rows, pool_frames, plain, hits, groups, k)
        assert svc.search_top_frames(query, k, "dup") == plain
        # similarity and pool are part of the cache key
        assert svc.search_top_frames_distinct(query, k, "dup", similarity=2.0) == plain
        wide = svc.search_top_frames_distinct(query, k, "dup", pool=64)
        hit64 = collapse_ref(rows.astype(np.float64), [int(os.path.basename(f)[:4]) for f in
                                                        svc.search_top_frames(query, 64, "dup")], k, 0.9)[0]
        assert [int(os.path.basename(f)[:4]) for f in wide] == hit64.tolist() and len(wide) == k
    assert svc.search_top_frames_distinct("anything", 5, "missing_video") == []
    assert svc.search_top_frames_distinct("anything", 5, "missing_video", with_groups=True) == []


def test_service_distinct_by_image(service):
    svc, rows, ids = service
    k = 10
    big = int(np.argmax(np.bincount(ids)))                              # a query inside the largest cluster
    img = rows[int(np.flatnonzero(ids == big)[0])]
    plain = svc.search_top_frames_by_image(img, k, "dup")
    pool_frames = svc.search_top_frames_by_image(img, 30, "dup")
    hits = svc.search_top_frames_by_image_distinct(img, k, "dup")
    groups = svc.search_top_frames_by_image_distinct(img, k, "dup", with_groups=True)
    _check_service(ids, rows, pool_frames, plain, hits, groups, k)
    assert len(groups[0][1]) == int((ids == big).sum()) - 1             # the query's own cluster, collapsed
    assert svc.search_top_frames_by_image(img, k, "dup") == plain
    assert svc.search_top_frames_by_image_distinct(img, 5, "missing_video") == []
