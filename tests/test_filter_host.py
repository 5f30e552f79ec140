"""CPU: the filtered ranking entry points (mi_rank_topk_filtered,
mi_rank_filtered_workspace_bytes) are exported and validate their arguments before
any HIP call, and FrameLibrary's bookkeeping (segments, global index -> (video, row),
video= -> ranges, allow= -> mask words) with the rank call stubbed."""
import re

import numpy as np
import pytest

F32, BF16, F16 = 0, 1, 2


def _lib():
    from miclip import _native
    return _native.lib()


def test_symbols_exported():
    from miclip import _native
    L = _lib()
    out = __import__("os").popen(f"nm -D --defined-only {_native.LIB_PATH}").read()
    for name in ("mi_rank_topk_filtered", "mi_rank_filtered_workspace_bytes"):
        assert name in _native.EXPORTS and hasattr(L, name)
        assert re.search(rf"\bT {name}$", out, re.M), f"{name} not exported"
    assert L.mi_abi_version() == 7


def _call(L, N=10, D=512, dt=F32, Q=1, k=10, norm=0, nan=0, ws=0):
    return L.mi_rank_topk_filtered(None, N, D, dt, None, Q, k, 0, norm, nan, None, None, None, None, None, ws, None)


def test_argument_errors_without_gpu():
    L = _lib()
    for k in (0, 65):
        assert _call(L, k=k) == -3 and b"k must be in [1, 64]" in L.mi_last_error()
    assert _call(L, D=500) == -3 and b"multiple of 32" in L.mi_last_error()
    assert _call(L, D=1056) == -3 and b"1024" in L.mi_last_error()
    assert _call(L, norm=3) == -1 and b"norm_mode" in L.mi_last_error()
    assert _call(L, nan=2) == -1 and b"nan_policy" in L.mi_last_error()
    assert _call(L, dt=3) == -1 and b"dtype" in L.mi_last_error()
    assert _call(L, N=-1) == -1
    # a short workspace (every other argument valid in form): refused before the pointers are looked at
    need = L.mi_rank_filtered_workspace_bytes(10, 1, 10)
    assert need > 0
    assert _call(L, ws=need - 1) == -1 and b"workspace too small" in L.mi_last_error()
    # the size is accepted; the call then fails on the null pointers, still without a GPU
    import ctypes
    buf = ctypes.create_string_buffer(need)
    rc = L.mi_rank_topk_filtered(None, 10, 512, F32, None, 1, 10, 0, 0, 0, None, None, None, None,
                                 ctypes.cast(buf, ctypes.c_void_p), need, None)
    assert rc == -1 and b"null pointer" in L.mi_last_error()
    assert _call(L, D=1024, k=64) == -1 and b"workspace" in L.mi_last_error()   # D = 1024, k = 64 accepted
    assert _call(L, Q=0) == 0                                                    # nothing to do


def test_workspace_monotone():
    L = _lib()
    f = L.mi_rank_filtered_workspace_bytes
    assert f(1000, 4, 0) == 0 and f(1000, 4, 65) == 0 and f(-1, 4, 10) == 0
    Ns = [0, 1, 31, 32, 33, 383, 384, 385, 5000, 100_003, 196_608, 196_609, 1_000_000, 12_582_912, 12_582_913,
          50_000_000, 400_000_000]
    Qs = [1, 2, 31, 32, 33, 64, 1000]
    ks = [1, 2, 10, 16, 17, 60, 64]
    for k in ks:
        for Q in Qs:
            v = [f(N, Q, k) for N in Ns]
            assert all(a <= b for a, b in zip(v, v[1:])), (k, Q, v)
    for k in ks:
        for N in Ns:
            v = [f(N, Q, k) for Q in Qs]
            assert all(a <= b for a, b in zip(v, v[1:])), (k, N, v)
    for Q in Qs:
        for N in Ns:
            v = [f(N, Q, k) for k in ks]
            assert all(a <= b for a, b in zip(v, v[1:])), (Q, N, v)
    # candidates of every workgroup: at least k (score, index) pairs per query
    assert f(1, 1, 1) >= 12 and f(1_000_000, 32, 10) >= 32 * 10 * 12


def test_pack_row_mask_matches_packbits():
    import torch
    from miclip import retrieval
    rng = np.random.default_rng(0)
    for n in (1, 31, 32, 33, 64, 100, 1000):
        m = rng.random(n) < 0.4
        m[-1] = True                      # the top bit of a word included (n % 32 == 0)
        want = np.packbits(np.pad(m, (0, -n % 32)), bitorder="little").view("<u4")
        got = retrieval.pack_row_mask(torch.from_numpy(m)).numpy().view(np.uint32)
        assert got.dtype == np.uint32 and np.array_equal(got, want), n


class _Stub:
    """Records FrameLibrary's filtered rank calls; answers with the first visible rows."""

    def __init__(self):
        self.calls = []

    def __call__(self, corpus, queries, k, row_mask=None, query_range=None, index_base=0, norm="l2",
                 nan_policy="first"):
        import torch
        self.calls.append(dict(rows=corpus.shape[0], dtype=corpus.dtype, queries=queries.clone(), k=k,
                               mask=None if row_mask is None else row_mask.clone(), range=query_range.clone(),
                               base=index_base, norm=norm, nan=nan_policy))
        Q = queries.shape[0]
        s = torch.full((Q, k), float("-inf"))
        i = torch.full((Q, k), -1, dtype=torch.int64)
        n = corpus.shape[0]
        vis = np.ones(n, bool) if row_mask is None else np.unpackbits(
            row_mask.numpy().view(np.uint8), bitorder="little")[:n].astype(bool)
        for q in range(Q):
            b, e = (int(x) for x in query_range[q])
            rows = [r for r in range(max(b, 0), min(e, n)) if vis[r]][:k]
            # the score carries the query's first component: the un-permute is visible in it
            s[q, :len(rows)] = queries[q, 0] - torch.arange(len(rows)) * 1e-3 - (0.5 if norm == "none" else 0.0)
            i[q, :len(rows)] = torch.tensor(rows, dtype=torch.int64) + index_base
        return s, i


def _merge_stub(cs, ci, k, nan_policy="first"):
    import torch
    key = torch.where(ci >= 0, cs, torch.full_like(cs, float("-inf")))
    order = torch.argsort(-key, dim=1, stable=True)[:, :k]
    return torch.gather(key, 1, order), torch.gather(ci, 1, order)


@pytest.fixture()
def lib5(monkeypatch):
    import torch
    from miclip import library
    stub = _Stub()
    monkeypatch.setattr(library, "rank_topk_filtered", stub)
    monkeypatch.setattr(library, "merge_topk", _merge_stub)
    monkeypatch.setattr(library, "normalize_rows_f16", lambda t, out=None: t)
    lib = library.FrameLibrary(device="cpu")
    rng = np.random.default_rng(1)
    lib.add("a", rng.standard_normal((40, 32)).astype(np.float32))
    lib.add("h1", rng.standard_normal((33, 32)).astype(np.float16))
    lib.add("b", torch.from_numpy(rng.standard_normal((70, 32)).astype(np.float32)))
    lib.add("empty", np.zeros((0, 32), np.float32))
    lib.add("h2", rng.standard_normal((5, 32)).astype(np.float16))
    lib.add("c", rng.standard_normal((7, 32)).astype(np.float64))       # ranked as f32
    return lib, stub


def test_library_segments_and_locate(lib5):
    import torch
    from miclip import _native
    lib, _ = lib5
    assert lib.names == ["a", "h1", "b", "empty", "h2", "c"] and len(lib) == 155
    # f32 group first (order of addition), then the float16 group
    assert lib.segments() == [("a", 0, 40, "l2"), ("b", 40, 70, "l2"), ("empty", 110, 0, "l2"), ("c", 110, 7, "l2"),
                              ("h1", 117, 33, "none"), ("h2", 150, 5, "none")]
    idx = torch.tensor([[0, 39, 40, 109, 110], [116, 117, 149, 150, 154], [-1, -1, 5, -1, 151]])
    vid, row = lib.locate(idx)
    assert vid.dtype == torch.int32 and row.dtype == torch.int64
    assert vid.tolist() == [[0, 0, 2, 2, 5], [5, 1, 1, 4, 4], [-1, -1, 0, -1, 4]]
    assert row.tolist() == [[0, 39, 0, 69, 0], [6, 0, 32, 0, 4], [-1, -1, 5, -1, 1]]
    with pytest.raises(_native.MiClipError):
        lib.add("a", np.zeros((3, 32), np.float32))
    with pytest.raises(_native.MiClipError):
        lib.add("d64", np.zeros((3, 64), np.float32))


def test_library_video_ranges(lib5):
    lib, stub = lib5
    q = np.arange(4 * 32, dtype=np.float32).reshape(4, 32)
    lib.search(q, 3)                                      # all videos
    assert [c["rows"] for c in stub.calls] == [117, 38] and [c["norm"] for c in stub.calls] == ["l2", "none"]
    assert [c["base"] for c in stub.calls] == [0, 117] and all(c["mask"] is None for c in stub.calls)
    assert stub.calls[0]["range"].tolist() == [[0, 117]] * 4 and stub.calls[1]["range"].tolist() == [[0, 38]] * 4
    stub.calls.clear()
    s, vid, row = lib.search(q, 3, video="b")             # one name: its segment in its group, nothing in the other
    assert stub.calls[0]["range"].tolist() == [[40, 110]] * 4
    assert all(b >= e for b, e in stub.calls[1]["range"].tolist())
    assert vid.tolist() == [[2, 2, 2]] * 4 and row.tolist() == [[0, 1, 2]] * 4
    stub.calls.clear()
    s, vid, row = lib.search(q, 3, video=["h2", None, "empty", "c"])
    r0, r1 = stub.calls[0]["range"].tolist(), stub.calls[1]["range"].tolist()
    assert r0[1] == [0, 117] and r0[3] == [110, 117] and r0[0][0] >= r0[0][1] and r0[2][0] >= r0[2][1]
    assert r1[0] == [33, 38] and r1[1] == [0, 38] and r1[2][0] >= r1[2][1] and r1[3][0] >= r1[3][1]
    assert vid[0].tolist() == [4, 4, 4] and row[0].tolist() == [0, 1, 2]
    assert vid[2].tolist() == [-1, -1, -1] and row[2].tolist() == [-1, -1, -1] and np.isinf(s[2].numpy()).all()
    assert vid[3].tolist() == [5, 5, 5] and row[3].tolist() == [0, 1, 2]
    assert vid[1].tolist() == [0, 0, 0]                   # all videos: the stub's f32 scores lead
    from miclip import _native
    with pytest.raises(_native.MiClipError):
        lib.search(q, 3, video="nope")
    with pytest.raises(_native.MiClipError):
        lib.search(q, 3, video=["a", "b"])


def test_library_allow_mask_words(lib5):
    lib, stub = lib5
    q = np.ones((2, 32), np.float32)
    flags_b = np.zeros(70, bool)
    flags_b[[0, 31, 32, 69]] = True
    allow = {"a": True, "b": flags_b, "h2": np.array([4, 1]), "c": [], "empty": True}
    s, vid, row = lib.search(q, 8, allow=allow)
    want0 = np.zeros(117, bool)
    want0[:40] = True
    want0[40 + np.array([0, 31, 32, 69])] = True          # "c" allows nothing
    want1 = np.zeros(38, bool)
    want1[33 + np.array([1, 4])] = True                   # "h1" is absent from the dict: excluded
    for call, want in zip(stub.calls, (want0, want1)):
        words = np.packbits(np.pad(want, (0, -len(want) % 32)), bitorder="little").view("<u4")
        assert np.array_equal(call["mask"].numpy().view(np.uint32), words)
    assert vid[0].tolist() == [0] * 8 and row[0].tolist() == list(range(8))
    stub.calls.clear()
    s, vid, row = lib.search(q, 4, video="h2", allow=allow)
    assert vid[0].tolist() == [4, 4, -1, -1] and row[0].tolist() == [1, 4, -1, -1]
    from miclip import _native
    with pytest.raises(_native.MiClipError):
        lib.search(q, 4, allow={"b": np.array([70])})
    with pytest.raises(_native.MiClipError):
        lib.search(q, 4, allow={"zzz": True})


def test_library_sorts_queries_by_range_begin(lib5):
    lib, stub = lib5
    Q = 40
    q = np.zeros((Q, 32), np.float32)
    q[:, 0] = np.arange(Q)                                # the stub's scores carry the query's identity
    videos = [("c", "a", "b", None)[i % 4] for i in range(Q)]
    s, vid, row = lib.search(q, 2, video=videos)
    begins = stub.calls[0]["range"][:, 0].tolist()
    assert begins == sorted(begins)                       # the kernel sees the queries sorted by begin
    assert sorted(stub.calls[0]["queries"][:, 0].tolist()) == list(range(Q))
    want = {"a": 0, "b": 2, "c": 5, None: 0}
    for i in range(Q):                                    # outputs are back in the caller's order
        assert vid[i].tolist() == [want[videos[i]]] * 2 and row[i].tolist() == [0, 1]
        assert abs(float(s[i, 0]) - i) < 1e-6
    stub.calls.clear()
    lib.search(q[:32], 2, video=videos[:32])              # up to 32 queries: one block, no permutation
    assert stub.calls[0]["queries"][:, 0].tolist() == list(range(32))
