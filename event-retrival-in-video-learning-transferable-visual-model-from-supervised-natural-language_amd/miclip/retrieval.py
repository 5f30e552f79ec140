"""Device-side ranking: the fused normalise + cosine + top-k kernel and the
R@K helpers, behind torch tensors.

Reference call sites this replaces:
  ``np.dot(embeddings, text_features.T)`` + ``np.argsort(s)[::-1][:top_k]``
      Backend/services/embedding_service.py:314-320 (text) and :365-372 (image query)
  ``image_features @ text_features.T`` + per-query ``np.argsort(-s)`` rank of GT
      Backend/content/Test_compare_model/compare_models.py:999-1016, 1045-1062

Order rule (documented in include/miclip.h): score descending, then index
ascending; NaN (a zero-norm row divided by its norm) first for the
``search_top_frames`` semantics (``argsort(s)[::-1]``), last for the
``compare_models`` semantics (``argsort(-s)``).
"""
from __future__ import annotations

import threading

from . import _native as N

_NORMS = {"l2": N.MI_NORM_L2, "l2_guard": N.MI_NORM_L2_GUARD, "none": N.MI_NORM_NONE}
_NANS = {"first": N.MI_NAN_FIRST, "last": N.MI_NAN_LAST}
REG_K = 64          # fused single-pass top-k (register lists) up to this k
MAX_K = 1 << 24     # above REG_K: exact scores + radix select + sort (rank.hip)
MAX_D = 1024

_ws_lock = threading.Lock()
_ws = {}


def _workspace(device, nbytes):
    """Scratch for mi_rank_topk, one buffer per (device, stream): kernels of
    two threads on different streams never share it (same-stream callers are
    ordered by the stream)."""
    import torch
    key = (device, N.stream_ptr(device))
    with _ws_lock:
        buf = _ws.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
            _ws[key] = buf
        return buf


def _corpus(corpus):
    import torch
    if corpus.dim() != 2:
        raise N.MiClipError("corpus must be [N, D]")
    if corpus.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        corpus = corpus.float()
    return corpus.contiguous()


def _queries(queries, device):
    import torch
    q = queries if queries.dim() == 2 else queries.reshape(1, -1)
    return q.to(device=device, dtype=torch.float32).contiguous()


def rank_topk(corpus, queries, k, index_base=0, norm="l2", nan_policy="first"):
    """Top-k rows of ``corpus`` [N,D] (device) for each query [Q,D].

    Returns (scores f32 [Q, min(k,N)], index int64 [Q, min(k,N)]) on the device.
    """
    import torch
    if not corpus.is_cuda:
        raise N.MiClipError("rank_topk runs on the GPU: move the corpus to the device first")
    c = _corpus(corpus)
    q = _queries(queries, c.device)
    if q.shape[1] != c.shape[1]:
        raise N.MiClipError(f"dimension mismatch: corpus D={c.shape[1]}, queries D={q.shape[1]}")
    Nrows, D = c.shape
    Q = q.shape[0]
    if not 1 <= k <= MAX_K:
        raise N.MiClipError(f"k must be in [1, {MAX_K}]")
    if not (32 <= D <= MAX_D and D % 32 == 0):
        raise N.MiClipError(f"D must be a multiple of 32 in [32, {MAX_D}], got {D}")
    out_s = torch.empty((Q, k), dtype=torch.float32, device=c.device)
    out_i = torch.empty((Q, k), dtype=torch.int64, device=c.device)
    L = N.lib()
    nbytes = L.mi_rank_workspace_bytes(Nrows, Q, k)
    with torch.cuda.device(c.device):
        ws = _workspace(c.device, nbytes)
        N.check(L.mi_rank_topk(c.data_ptr(), Nrows, D, N.dtype_code(c.dtype), q.data_ptr(), Q, k, int(index_base),
                               _NORMS[norm], _NANS[nan_policy], out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(),
                               ws.numel(), N.stream_ptr(c.device)), "mi_rank_topk")
    kk = min(k, Nrows)
    return out_s[:, :kk], out_i[:, :kk]


def pack_row_mask(mask):
    """A bool row mask [N] as the filtered rank kernel's words: int32 [(N+31)//32],
    bit ``r & 31`` of word ``r >> 5`` = ``mask[r]`` (``np.packbits(..., bitorder="little")``
    viewed as little-endian uint32).  Torch ops on the mask's device: no host round trip."""
    import torch
    m = mask.reshape(-1).to(torch.bool)
    n = m.shape[0]
    words = (n + 31) // 32
    bits = torch.zeros(words * 32, dtype=torch.int64, device=m.device)
    bits[:n] = m
    v = (bits.view(words, 32) << torch.arange(32, dtype=torch.int64, device=m.device)).sum(dim=1)
    return torch.where(v >= (1 << 31), v - (1 << 32), v).to(torch.int32)


def _row_mask(row_mask, nrows, device):
    import torch
    words = (nrows + 31) // 32
    if row_mask.dtype == torch.bool:
        if row_mask.numel() != nrows:
            raise N.MiClipError(f"row_mask: {row_mask.numel()} flags for {nrows} rows")
        return pack_row_mask(row_mask.to(device))
    if row_mask.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):
        raise N.MiClipError("row_mask must be a bool tensor [N] or packed int32 / uint32 words")
    if row_mask.numel() < words:
        raise N.MiClipError(f"row_mask: {row_mask.numel()} words for {nrows} rows ({words} needed)")
    return row_mask.to(device).contiguous()


def _query_range(query_range, Q, device):
    import torch
    if isinstance(query_range, (tuple, list)) and len(query_range) == 2 and not torch.is_tensor(query_range[0]) \
            and not isinstance(query_range[0], (tuple, list)):
        query_range = torch.tensor([[int(query_range[0]), int(query_range[1])]], dtype=torch.int64).expand(Q, 2)
    r = torch.as_tensor(query_range).to(device=device, dtype=torch.int64).contiguous()
    if r.shape != (Q, 2):
        raise N.MiClipError(f"query_range must be [Q, 2] = {(Q, 2)} or a (begin, end) pair, got {tuple(r.shape)}")
    return r


def rank_topk_filtered(corpus, queries, k, row_mask=None, query_range=None, index_base=0, norm="l2",
                       nan_policy="first"):
    """``rank_topk`` over the rows each query may see (``mi_rank_topk_filtered``,
    csrc/rank_filter.hip): row ``r`` is visible to query ``q`` iff ``row_mask`` is None or has
    ``r`` set, and ``begin_q <= r < end_q``.  ``row_mask``: a device bool tensor [N] (packed on
    the device, ``pack_row_mask``) or packed int32 / uint32 words; ``query_range``: int64 [Q, 2]
    or one ``(begin, end)`` pair for all queries.  Indices stay global (``index_base + r``).

    Returns (scores f32 [Q, k], index int64 [Q, k]) on the device; slots beyond a query's
    visible rows are (-inf, -1).  1 <= k <= 64.  A visible row's score is bit-identical to
    ``rank_topk``'s, so this equals ``rank_topk`` over the gathered visible rows.
    """
    import torch
    if not corpus.is_cuda:
        raise N.MiClipError("rank_topk_filtered runs on the GPU: move the corpus to the device first")
    c = _corpus(corpus)
    q = _queries(queries, c.device)
    if q.shape[1] != c.shape[1]:
        raise N.MiClipError(f"dimension mismatch: corpus D={c.shape[1]}, queries D={q.shape[1]}")
    Nrows, D = c.shape
    Q = q.shape[0]
    if not 1 <= k <= REG_K:
        raise N.MiClipError(f"rank_topk_filtered: k must be in [1, {REG_K}]")
    if not (32 <= D <= MAX_D and D % 32 == 0):
        raise N.MiClipError(f"D must be a multiple of 32 in [32, {MAX_D}], got {D}")
    mask = None if row_mask is None else _row_mask(row_mask, Nrows, c.device)
    rng = None if query_range is None else _query_range(query_range, Q, c.device)
    out_s = torch.empty((Q, k), dtype=torch.float32, device=c.device)
    out_i = torch.empty((Q, k), dtype=torch.int64, device=c.device)
    L = N.lib()
    nbytes = L.mi_rank_filtered_workspace_bytes(Nrows, Q, k)
    with torch.cuda.device(c.device):
        ws = _workspace(c.device, nbytes)
        N.check(L.mi_rank_topk_filtered(c.data_ptr(), Nrows, D, N.dtype_code(c.dtype), q.data_ptr(), Q, k,
                                        int(index_base), _NORMS[norm], _NANS[nan_policy],
                                        mask.data_ptr() if mask is not None else None,
                                        rng.data_ptr() if rng is not None else None,
                                        out_s.data_ptr(), out_i.data_ptr(), ws.data_ptr(), ws.numel(),
                                        N.stream_ptr(c.device)), "mi_rank_topk_filtered")
    return out_s, out_i


def collapse_topk(corpus, cand_scores, cand_index, k, threshold, index_base=0, corpus2=None):
    """Distinct top-k of ranked candidate lists (``mi_rank_collapse``, csrc/rank_collapse.hip).

    ``cand_scores`` f32 / ``cand_index`` int64 [Q, P] are what ``rank_topk``,
    ``rank_topk_filtered``, ``MirroredCorpus.topk`` or ``merge_topk`` returned (index -1 =
    empty slot), trusted as ordered; 1 <= k <= P <= 64.  Candidates are walked in order: one
    whose cosine to an accepted hit's stored row is >= ``threshold`` joins the hit in the
    lowest such slot; otherwise it becomes the next hit while fewer than k are accepted, and
    is dropped after that.  Rows of index ``index_base + r``, r < N, come from ``corpus``
    [N, D]; r in [N, N + N2) from ``corpus2`` [N2, D] (dtypes may differ); any other index is
    an empty slot.  Zero-norm rows are similar to nothing.

    Returns (scores f32 [Q, k] copied bit for bit, index int64 [Q, k], count int32 [Q, k],
    slot int32 [Q, P]) on the device: unused hit slots are (-inf, -1, 0); ``slot[q, j]`` is
    the hit candidate j went into, -1 for empty or dropped candidates.
    """
    import torch
    if not corpus.is_cuda:
        raise N.MiClipError("collapse_topk runs on the GPU: move the corpus to the device first")
    c = _corpus(corpus)
    c2 = None if corpus2 is None else _corpus(corpus2).to(c.device)
    if c2 is not None and c2.shape[1] != c.shape[1]:
        raise N.MiClipError(f"dimension mismatch: corpus D={c.shape[1]}, corpus2 D={c2.shape[1]}")
    s = cand_scores.to(device=c.device, dtype=torch.float32).contiguous()
    i = cand_index.to(device=c.device, dtype=torch.int64).contiguous()
    if s.dim() != 2 or s.shape != i.shape:
        raise N.MiClipError("collapse_topk: cand_scores and cand_index must both be [Q, P]")
    Q, P = s.shape
    D = c.shape[1]
    if not 1 <= k <= P <= REG_K:
        raise N.MiClipError(f"collapse_topk: needs 1 <= k <= P <= {REG_K} (k={k}, P={P})")
    if not (32 <= D <= MAX_D and D % 32 == 0):
        raise N.MiClipError(f"D must be a multiple of 32 in [32, {MAX_D}], got {D}")
    out_s = torch.empty((Q, k), dtype=torch.float32, device=c.device)
    out_i = torch.empty((Q, k), dtype=torch.int64, device=c.device)
    out_c = torch.empty((Q, k), dtype=torch.int32, device=c.device)
    out_slot = torch.empty((Q, P), dtype=torch.int32, device=c.device)
    L = N.lib()
    nbytes = L.mi_rank_collapse_workspace_bytes(Q, P, D)
    with torch.cuda.device(c.device):
        ws = _workspace(c.device, nbytes)
        N.check(L.mi_rank_collapse(c.data_ptr(), c.shape[0], N.dtype_code(c.dtype),
                                   c2.data_ptr() if c2 is not None else None,
                                   c2.shape[0] if c2 is not None else 0,
                                   N.dtype_code(c2.dtype) if c2 is not None else 0,
                                   D, int(index_base), s.data_ptr(), i.data_ptr(), Q, P, int(k), float(threshold),
                                   out_s.data_ptr(), out_i.data_ptr(), out_c.data_ptr(), out_slot.data_ptr(),
                                   ws.data_ptr(), ws.numel(), N.stream_ptr(c.device)), "mi_rank_collapse")
    return out_s, out_i, out_c, out_slot


EXCLUDE_H = 32      # hits per mi_rank_exclude call (one 32-column MFMA block)


def exclude_similar(corpus, hits, hit_index=None, threshold=0.9, row_mask=None, index_base=0, out=None, count=False):
    """Remove from a row mask every visible row similar to one of ``hits`` (``mi_rank_exclude``,
    csrc/rank_exclude.hip): one streaming pass over ``corpus`` [N, D] (device).

    ``hits`` [H, D]: the hits' stored rows (any dtype, moved to the device and widened with
    ``.float()``); ``hit_index`` int64 [H] or None: their global indices, so that a zero-norm hit
    removes its own row (an index outside ``[index_base, index_base + N)`` names no row).
    ``row_mask``: None (every row visible), a bool tensor [N] or packed int32 / uint32 words, as
    ``rank_topk_filtered`` takes it.  A visible row is removed when its cosine (``collapse_topk``'s)
    to some hit is >= ``threshold`` or a hit names it.  ``out``: the int32 words to write (may be
    the packed ``row_mask`` itself: in place).  More than 32 hits run as chained calls of 32, each
    on the previous call's mask.

    Returns (mask int32 [(N + 31) // 32], count int32 [H] or None) on the device; with
    ``count=True`` ``count[m]`` is the number of removed rows attributed to hit m: the lowest
    similar slot, else the lowest slot naming the row.
    """
    import torch
    if not corpus.is_cuda:
        raise N.MiClipError("exclude_similar runs on the GPU: move the corpus to the device first")
    c = _corpus(corpus)
    Nrows, D = c.shape
    h = hits if hits.dim() == 2 else hits.reshape(1, -1)
    h = h.to(c.device).float().contiguous()
    H = h.shape[0]
    if h.shape[1] != D:
        raise N.MiClipError(f"dimension mismatch: corpus D={D}, hits D={h.shape[1]}")
    if H < 1:
        raise N.MiClipError("exclude_similar: needs at least one hit")
    if not (32 <= D <= MAX_D and D % 32 == 0):
        raise N.MiClipError(f"D must be a multiple of 32 in [32, {MAX_D}], got {D}")
    hi = None
    if hit_index is not None:
        hi = torch.as_tensor(hit_index).reshape(-1).to(device=c.device, dtype=torch.int64).contiguous()
        if hi.shape[0] != H:
            raise N.MiClipError(f"exclude_similar: {hi.shape[0]} indices for {H} hits")
    words = (Nrows + 31) // 32
    mask = None if row_mask is None else _row_mask(row_mask, Nrows, c.device)
    if out is None:
        out = torch.empty(words, dtype=torch.int32, device=c.device)
    elif not (out.is_cuda and out.device == c.device and out.dtype == torch.int32 and out.is_contiguous()
              and out.numel() >= words):
        raise N.MiClipError(f"exclude_similar: out must be {words} contiguous int32 words on the corpus' device")
    cnt = torch.zeros(H, dtype=torch.int32, device=c.device) if count else None
    if Nrows == 0:
        return out[:words], cnt
    L = N.lib()
    with torch.cuda.device(c.device):
        ws = _workspace(c.device, L.mi_rank_exclude_workspace_bytes(Nrows, EXCLUDE_H))
        for b in range(0, H, EXCLUDE_H):
            n = min(EXCLUDE_H, H - b)
            N.check(L.mi_rank_exclude(c.data_ptr(), Nrows, D, N.dtype_code(c.dtype), h[b:b + n].data_ptr(),
                                      hi[b:b + n].data_ptr() if hi is not None else None, n, int(index_base),
                                      float(threshold), mask.data_ptr() if mask is not None else None,
                                      out.data_ptr(), cnt[b:b + n].data_ptr() if count else None,
                                      ws.data_ptr(), ws.numel(), N.stream_ptr(c.device)), "mi_rank_exclude")
            mask = out
    return out[:words], cnt


def _pool_candidates(corpus, queries, pool, mask, rank_kwargs):
    """[Q, pool] ranked candidates of ``rank_topk`` (or, under a mask, ``rank_topk_filtered``),
    padded with empty slots when the corpus holds fewer rows."""
    import torch
    if mask is None:
        s, i = rank_topk(corpus, queries, pool, **rank_kwargs)
    else:
        s, i = rank_topk_filtered(corpus, queries, pool, row_mask=mask, **rank_kwargs)
    if s.shape[1] < pool:
        pad = pool - s.shape[1]
        s = torch.cat([s, s.new_full((s.shape[0], pad), float("-inf"))], dim=1)
        i = torch.cat([i, i.new_full((i.shape[0], pad), -1)], dim=1)
    return s, i


def rank_topk_distinct(corpus, queries, k, threshold, pool=None, fill=False, row_mask=None, **rank_kwargs):
    """Top-k distinct rows: ``rank_topk`` for ``pool`` candidates (default ``min(64, 3 k)``, the
    reference's ``top_k * 3`` over-fetch, clipped to the row count), then ``collapse_topk`` at
    ``threshold``.  ``rank_kwargs`` go to ``rank_topk`` (index_base, norm, nan_policy).
    ``row_mask`` (bool [N] or packed words): only these rows are visible; the pool then comes
    from ``rank_topk_filtered``.
    Returns ``collapse_topk``'s (scores, index, count, slot); hit slots beyond the distinct
    rows the pool holds are (-inf, -1, 0).

    ``fill=True``: the distinct top-k of ALL visible rows (the greedy walk of the whole ranking,
    tests/exclude_ref.py ``fill_ref``) instead of the pool's.  Round 1 is the path above.  A
    query left with fewer than k hits by a full pool goes on alone: ``exclude_similar`` removes
    every row similar to its new hits from its mask, ``rank_topk_filtered`` ranks ``pool`` rows
    under the mask, ``collapse_topk`` fills the remaining slots, until k hits or a short pool
    (the visible rows are exhausted); at most k rounds, each a full pool's first candidate at
    least.  Returns (scores, index, count): a query that had k hits keeps its scores (bit for
    bit) and indices, ``count`` is the number of visible corpus rows in the hit's group, itself
    included, and there is no ``slot`` (no single pool to refer to).  Cost: the corpus-wide
    counts take one ``exclude_similar`` pass over the corpus per query and round's hits, so a
    query whose pool already gave k hits pays one pass too, and Q queries run at least Q passes
    one after another; the only query that costs nothing extra is one whose short pool held every
    visible row (fewer than k hits, nothing left to rank: its pool counts are the corpus').  The rounds read hit counts on the host: ``fill=True``
    synchronises and cannot be captured in a graph.
    """
    import torch
    if not 1 <= k <= REG_K:
        raise N.MiClipError(f"rank_topk_distinct: k must be in [1, {REG_K}]")
    pool = min(REG_K, 3 * k) if pool is None else int(pool)
    if not k <= pool <= REG_K:
        raise N.MiClipError(f"rank_topk_distinct: pool must be in [k, {REG_K}] (got {pool})")
    Nrows = corpus.shape[0]
    pool = max(min(pool, Nrows), k)   # rank_topk pads to k columns only when k > N
    base = rank_kwargs.get("index_base", 0)
    mask0 = None if row_mask is None else _row_mask(row_mask, Nrows, corpus.device)
    s, i = _pool_candidates(corpus, queries, pool, mask0, rank_kwargs)
    res = collapse_topk(corpus, s, i, k, threshold, index_base=base)
    if not fill:
        return res
    out_s, out_i, out_c, _ = res
    if Nrows == 0:
        return out_s, out_i, out_c
    c = _corpus(corpus)
    q = _queries(queries, c.device)
    fkw = {n: v for n, v in rank_kwargs.items() if n in ("norm", "nan_policy")}
    nhit = (out_i >= 0).sum(dim=1)
    state = torch.stack([nhit, (i[:, pool - 1] >= 0).to(nhit.dtype)], dim=1).tolist()   # host read: synchronises
    for qi, (have, full) in enumerate(state):
        if not full and have < k:
            continue   # the pool held every visible row: hits and counts are the corpus' already
        new = out_i[qi, :have]
        mask, rounds, counts = mask0, 1, []
        while True:
            assert rounds <= k, "rank_topk_distinct: a full pool's first candidate is always accepted"
            rows = c.index_select(0, new - base)
            mask, cnt = exclude_similar(c, rows, new, threshold, row_mask=mask, index_base=base,
                                        out=None if mask is mask0 else mask, count=True)
            counts.append(cnt)
            if have >= k or not full:
                break
            s2, i2 = rank_topk_filtered(c, q[qi:qi + 1], pool, row_mask=mask, index_base=base, **fkw)
            ns, ni, _, _ = collapse_topk(c, s2, i2, k - have, threshold, index_base=base)
            rounds += 1
            got, full = torch.stack([(ni[0] >= 0).sum(), (i2[0, pool - 1] >= 0).to(torch.int64)]).tolist()
            if got == 0:
                break
            out_s[qi, have:have + got] = ns[0, :got]
            out_i[qi, have:have + got] = ni[0, :got]
            new = ni[0, :got]
            have += got
        out_c[qi, :have] = torch.cat(counts)
    return out_s, out_i, out_c


def normalize_rows_f16(rows, out=None):
    """``embeddings / np.linalg.norm(embeddings, axis=-1, keepdims=True)`` for a
    float16 corpus, bit for bit as NumPy evaluates it in float16
    (Backend/services/embedding_service.py:209-210 on the reference's fp16
    ``.npy`` files; ``mi_normalize_rows_f16``, csrc/corpus.hip).  ``rows``: device
    fp16 [N, D]; returns the normalised fp16 rows (``out`` may be ``rows``)."""
    import torch
    if not rows.is_cuda or rows.dtype != torch.float16 or rows.dim() != 2:
        raise N.MiClipError("normalize_rows_f16 takes device float16 [N, D] rows")
    r = rows.contiguous()
    o = torch.empty_like(r) if out is None else out
    if o.shape != r.shape or o.dtype != torch.float16 or not o.is_contiguous():
        raise N.MiClipError("normalize_rows_f16: out must be contiguous float16 of the rows' shape")
    with torch.cuda.device(r.device):
        N.check(N.lib().mi_normalize_rows_f16(r.data_ptr(), r.shape[0], r.shape[1], o.data_ptr(),
                                              N.stream_ptr(r.device)), "mi_normalize_rows_f16")
    return o


def merge_topk(cand_scores, cand_index, k, nan_policy="first"):
    """Merge [Q, C] candidate lists (index -1 = empty) into the top-k (device)."""
    import torch
    s = cand_scores.to(torch.float32).contiguous()
    i = cand_index.to(torch.int64).contiguous()
    Q, C = s.shape
    out_s = torch.empty((Q, k), dtype=torch.float32, device=s.device)
    out_i = torch.empty((Q, k), dtype=torch.int64, device=s.device)
    with torch.cuda.device(s.device):
        N.check(N.lib().mi_rank_merge(s.data_ptr(), i.data_ptr(), Q, C, k, _NANS[nan_policy], out_s.data_ptr(),
                                      out_i.data_ptr(), N.stream_ptr(s.device)), "mi_rank_merge")
    return out_s, out_i


def score_matrix(corpus, queries, norm="none"):
    """[Q, N] f32 scores <q, c/|c|> with fp32-exact products (device)."""
    import torch
    c = _corpus(corpus)
    q = _queries(queries, c.device)
    out = torch.empty((q.shape[0], c.shape[0]), dtype=torch.float32, device=c.device)
    with torch.cuda.device(c.device):
        N.check(N.lib().mi_score_matrix(c.data_ptr(), c.shape[0], c.shape[1], N.dtype_code(c.dtype), q.data_ptr(),
                                        q.shape[0], _NORMS[norm], out.data_ptr(), N.stream_ptr(c.device)),
                "mi_score_matrix")
    return out


def rank_of_targets(scores, pair_query, pair_target):
    """1-based rank of scores[q, g] in argsort(-scores[q]) for each (q, g) pair."""
    import torch
    s = scores.to(torch.float32).contiguous()
    pq = torch.as_tensor(pair_query, dtype=torch.int64).to(s.device).contiguous()
    pt = torch.as_tensor(pair_target, dtype=torch.int64).to(s.device).contiguous()
    out = torch.empty(pq.shape[0], dtype=torch.int64, device=s.device)
    with torch.cuda.device(s.device):
        N.check(N.lib().mi_rank_of_targets(s.data_ptr(), s.shape[0], s.shape[1], pq.data_ptr(), pt.data_ptr(),
                                           pq.shape[0], out.data_ptr(), N.stream_ptr(s.device)),
                "mi_rank_of_targets")
    return out


def event_block_cols(n):
    """Columns one workgroup of ``mi_event_topk`` covers at ``n`` columns (introspection, for
    tests that place events on workgroup boundaries)."""
    return int(N.lib().mi_debug_event_block_cols(int(n)))


def event_topk(scores, threshold, k, max_gap=0, min_count=1, row_time=None, row_mask=None, query_range=None,
               index_base=0):
    """Top-k temporal runs of matching frames per query (``mi_event_topk``, csrc/rank_events.hip).

    ``scores``: device f32 [Q, N], columns in time order (``score_matrix``'s output).
    ``threshold``: a number or [Q].  Column t is hot for q iff it is visible and
    ``scores[q, t] >= threshold[q]`` (false for NaN).  ``row_time``: int64 [N], non-decreasing
    (checked here on the host when given as a host array or list; a device tensor is trusted), or
    None: time = column.  Consecutive hot columns whose times differ by at most ``max_gap`` chain
    into one event; an event qualifies with at least ``min_count`` hot columns.  ``row_mask`` (bool
    [N] or packed words) and ``query_range`` ([Q, 2] or one pair, in columns) are
    ``rank_topk_filtered``'s.  1 <= k <= 64.

    Returns (score f32, peak int64, begin int64, end int64, count int32, each [Q, k], total int32
    [Q]) on the device: the qualifying events by peak score descending, then begin ascending;
    peak / begin / end are ``index_base`` + column (end inclusive); unused slots are
    -inf / -1 / -1 / -1 / 0; ``total`` counts the query's qualifying events whatever k.
    """
    import torch
    if not scores.is_cuda:
        raise N.MiClipError("event_topk runs on the GPU: the scores must be on the device")
    if scores.dim() != 2:
        raise N.MiClipError("event_topk: scores must be [Q, N]")
    s = scores.to(torch.float32).contiguous()
    Q, n = s.shape
    dev = s.device
    if not 1 <= k <= REG_K:
        raise N.MiClipError(f"event_topk: k must be in [1, {REG_K}]")
    if int(max_gap) < 0 or int(min_count) < 1:
        raise N.MiClipError("event_topk: needs max_gap >= 0 and min_count >= 1")
    tau = torch.as_tensor(threshold, dtype=torch.float32).reshape(-1).to(dev)
    tau = (tau.expand(Q) if tau.numel() == 1 else tau).contiguous()
    if tau.shape != (Q,):
        raise N.MiClipError(f"event_topk: threshold must be a number or [Q] = {Q} values, got {tuple(tau.shape)}")
    times = None
    if row_time is not None:
        if not (torch.is_tensor(row_time) and row_time.is_cuda):
            host = torch.as_tensor(row_time).to(torch.int64).reshape(-1)
            if host.numel() > 1 and bool((host[1:] < host[:-1]).any()):
                raise N.MiClipError("event_topk: row_time must be non-decreasing")
            row_time = host
        times = row_time.to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        if times.numel() != n:
            raise N.MiClipError(f"event_topk: {times.numel()} times for {n} columns")
    mask = None if row_mask is None else _row_mask(row_mask, n, dev)
    rng = None if query_range is None else _query_range(query_range, Q, dev)
    out_s = torch.empty((Q, k), dtype=torch.float32, device=dev)
    out_p, out_b, out_e = (torch.empty((Q, k), dtype=torch.int64, device=dev) for _ in range(3))
    out_c = torch.empty((Q, k), dtype=torch.int32, device=dev)
    out_t = torch.empty(Q, dtype=torch.int32, device=dev)
    L = N.lib()
    with torch.cuda.device(dev):
        ws = _workspace(dev, L.mi_event_workspace_bytes(n, Q, k))
        N.check(L.mi_event_topk(s.data_ptr(), n, Q, tau.data_ptr(),
                                times.data_ptr() if times is not None else None,
                                mask.data_ptr() if mask is not None else None,
                                rng.data_ptr() if rng is not None else None,
                                int(max_gap), int(min_count), int(k), int(index_base),
                                out_s.data_ptr(), out_p.data_ptr(), out_b.data_ptr(), out_e.data_ptr(),
                                out_c.data_ptr(), out_t.data_ptr(), ws.data_ptr(), ws.numel(),
                                N.stream_ptr(dev)), "mi_event_topk")
    return out_s, out_p, out_b, out_e, out_c, out_t


def rank_events(corpus, queries, k, threshold, max_gap=0, min_count=1, row_time=None, row_mask=None,
                query_range=None, index_base=0, norm="l2"):
    """``score_matrix`` followed by ``event_topk``: the top-k events of each query over the rows
    of ``corpus`` [N, D] (device), which must already be in time order.  The scores are the exact
    f32 scores every rank kernel ranks by."""
    if not corpus.is_cuda:
        raise N.MiClipError("rank_events runs on the GPU: move the corpus to the device first")
    return event_topk(score_matrix(corpus, queries, norm=norm), threshold, k, max_gap=max_gap, min_count=min_count,
                      row_time=row_time, row_mask=row_mask, query_range=query_range, index_base=index_base)


class MirroredCorpus:
    """HBM-resident corpus with an fp16 ranking mirror and the master kept for
    exact re-scoring (csrc/rank_mirror.hip).

    The mirror holds every row as an fp16 unit vector (``mi_mirror_build``,
    the exact path's reciprocal norm), so ``topk`` streams half the f32 bytes
    on the fp16 MFMA for the top 16 mirror candidates per query, re-scores
    them against the master with the exact path's arithmetic, and certifies
    the result per query: with the mirror's score error bounded by delta
    (rank_mirror.hip), every row outside the candidates scores at most
    ``s_mirror[15] + delta``, so once the exact k-th score exceeds that bound
    the answer is bit-identical to ``rank_topk(master, ...)``.  Queries that
    fail the certificate (near-ties across the candidate edge, NaN rows) and
    requests the mirror does not cover (k > MAX_K, norm other than "l2",
    D not in {512, 768}) take the exact pass; ``fallbacks`` counts them.
    MAX_K = 12 < 16: the certificate needs a score gap between the k-th
    exact and the 16th mirror candidate, which k = 16 never has.

    Reference semantics: ``EmbeddingService.search_top_frames`` ranks
    ``get_embeddings`` rows (embedding_service.py:209-210, 314-320); the stored
    ``.npy`` rows stay the master (embedding_service.py:505).
    """

    MAX_K = 12

    def __init__(self, master):
        import torch
        if not master.is_cuda:
            raise N.MiClipError("MirroredCorpus lives in HBM: move the master rows to the device first")
        self.master = _corpus(master)
        n, d = self.master.shape
        self.mirror = None
        self.fallbacks = 0
        self.certified = 0
        if n > 0 and d in (512, 768):
            self.mirror = torch.empty((n, d), dtype=torch.float16, device=self.master.device)
            with torch.cuda.device(self.master.device):
                N.check(N.lib().mi_mirror_build(self.master.data_ptr(), n, d, N.dtype_code(self.master.dtype),
                                                self.mirror.data_ptr(), N.stream_ptr(self.master.device)),
                        "mi_mirror_build")

    def __len__(self):
        return self.master.shape[0]

    def topk(self, queries, k, norm="l2", nan_policy="first", index_base=0):
        import torch
        q = _queries(queries, self.master.device)
        n, d = self.master.shape
        Q = q.shape[0]
        if q.shape[1] != d:
            raise N.MiClipError(f"dimension mismatch: corpus D={d}, queries D={q.shape[1]}")
        if self.mirror is None or norm != "l2" or not 1 <= k <= self.MAX_K or Q == 0:
            self.fallbacks += Q
            return rank_topk(self.master, q, k, index_base=index_base, norm=norm, nan_policy=nan_policy)
        dev = self.master.device
        out_s = torch.empty((Q, k), dtype=torch.float32, device=dev)
        out_i = torch.empty((Q, k), dtype=torch.int64, device=dev)
        cert = torch.empty(Q, dtype=torch.int32, device=dev)
        L = N.lib()
        with torch.cuda.device(dev):
            ws = _workspace(dev, L.mi_rank_mirror_workspace_bytes(n, Q))
            N.check(L.mi_rank_mirror(self.mirror.data_ptr(), self.master.data_ptr(), n, d,
                                     N.dtype_code(self.master.dtype), q.data_ptr(), Q, k, int(index_base),
                                     _NANS[nan_policy], out_s.data_ptr(), out_i.data_ptr(), cert.data_ptr(),
                                     ws.data_ptr(), ws.numel(), N.stream_ptr(dev)), "mi_rank_mirror")
        bad = torch.nonzero(cert == 0).flatten()
        nb = int(bad.numel())
        self.fallbacks += nb
        self.certified += Q - nb
        if nb:
            sf, jf = rank_topk(self.master, q.index_select(0, bad), k, index_base=index_base, norm=norm,
                               nan_policy=nan_policy)
            out_s[bad, :sf.shape[1]] = sf
            out_i[bad, :jf.shape[1]] = jf
        kk = min(k, n)
        return out_s[:, :kk], out_i[:, :kk]
