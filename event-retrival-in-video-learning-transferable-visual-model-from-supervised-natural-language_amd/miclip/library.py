"""``FrameLibrary``: a resident multi-video index over the filtered rank kernel.

The reference's UI offers a video filter whose default is all videos
(Backend/app.py:402-429, 567-588, 605) but ranks one video's ``.npy`` per call
(embedding_service.py:284-344), and its hybrid strategies take CLIP's
``top_k*3`` and intersect afterwards with the frames a keyword / object filter
allows (query_strategies.py:253-361, 466-599, 601-775).  Here every video's rows
stay in HBM once, concatenated, and one ``rank_topk_filtered`` pass answers
"this video", "all videos", "a video per query" and "only these frames": a
video is a row range, an allow-list is a row mask, no corpus is copied.

Rows are kept by ``EmbeddingService._corpus_on_device``'s rule: f32 rows raw,
ranked with norm "l2"; float16 rows normalised once in NumPy's float16
arithmetic (``normalize_rows_f16``) and ranked with norm "none".  So the library
holds at most two concatenated corpora, one per norm mode, each with a segment
table ``(name, offset, rows)``; a search runs one filtered pass per non-empty
corpus and merges the two candidate lists with ``merge_topk``.

Global index: the f32 ("l2") corpus' rows first, in order of addition, then the
float16 ("none") corpus' rows, in order of addition.  Exact score ties across
videos resolve by that global index ascending: f32 videos before float16
videos, then the order the videos were added, then the row.
"""
from __future__ import annotations

import numpy as np

from . import _native as N
from .retrieval import (collapse_topk, event_topk, exclude_similar, merge_topk, normalize_rows_f16, pack_row_mask,
                        rank_topk_filtered, score_matrix)

TIME_BITS = 40          # frame times and max_gap are below 2^40; a column's time is (video ordinal << 41) + t,
                        # so two videos' columns are more than any max_gap apart

SORT_MIN_QUERIES = 32   # above it the queries are sorted by range begin (the kernel skips per 32-query block)


class _Group:
    """One concatenated corpus (one norm mode) and its segment table."""

    def __init__(self, norm):
        self.norm = norm
        self.parts = []
        self.segments = []      # (name, offset, rows)
        self.times = []         # per segment: None or host int64 [rows]
        self.rows = 0
        self._cat = None
        self._order = None

    def append(self, name, t, times=None):
        self.segments.append((name, self.rows, int(t.shape[0])))
        self.times.append(times)
        self.parts.append(t)
        self.rows += int(t.shape[0])
        self._cat = None
        self._order = None

    def time_order(self):
        """(perm, col_time, gather): column c of the group's time-ordered score matrix is stored
        row perm[c] (a stable sort by time within each video, videos stay contiguous); col_time[c]
        = (video ordinal << 41) + t, a video without times using its row number; gather = some
        video's times are not already sorted (perm is not the identity).  Host int64 arrays."""
        if self._order is None:
            perm = np.arange(self.rows, dtype=np.int64)
            col_time = np.zeros(self.rows, np.int64)
            gather = False
            for ordinal, ((_, off, rows), t) in enumerate(zip(self.segments, self.times)):
                if t is None:
                    t = np.arange(rows, dtype=np.int64)
                elif rows > 1 and (t[1:] < t[:-1]).any():
                    order = np.argsort(t, kind="stable")
                    perm[off:off + rows] = off + order
                    t = t[order]
                    gather = True
                col_time[off:off + rows] = (np.int64(ordinal) << (TIME_BITS + 1)) + t
            self._order = (perm, col_time, gather)
        return self._order

    def corpus(self):
        import torch
        if self._cat is None:
            self._cat = self.parts[0] if len(self.parts) == 1 else torch.cat(self.parts, dim=0)
            self.parts = [self._cat]
        return self._cat

    def segment(self, name):
        for s in self.segments:
            if s[0] == name:
                return s
        return None


class FrameLibrary:
    def __init__(self, device="cuda"):
        self.device = device
        self.names = []                                   # video_index -> name, order of addition
        self._groups = [_Group("l2"), _Group("none")]     # global index order
        self.dim = None

    # ------------------------------------------------------------------ build
    def add(self, name, rows, times=None):
        """Append a video's embedding rows [n, D] (NumPy or torch; f32 or float16,
        anything else is ranked as f32).  ``times``: optional integers [n], 0 <= t < 2^40, in
        any order: the rows' positions on the video's time axis (frame numbers), used by
        ``search_events`` only; storage and every other search are unchanged."""
        import torch
        if name in self.names:
            raise N.MiClipError(f"FrameLibrary: video {name!r} was already added")
        t = torch.as_tensor(np.ascontiguousarray(rows) if isinstance(rows, np.ndarray) else rows)
        if t.dim() != 2:
            raise N.MiClipError("FrameLibrary.add: rows must be [n, D]")
        if self.dim is not None and t.shape[1] != self.dim:
            raise N.MiClipError(f"FrameLibrary.add: D = {t.shape[1]}, the library holds D = {self.dim}")
        if t.dtype not in (torch.float32, torch.float16):
            t = t.to(torch.float32)
        if times is not None:
            tm = np.asarray(times)
            if tm.shape != (t.shape[0],) or (tm.size and tm.dtype.kind not in "iu"):
                raise N.MiClipError(f"FrameLibrary.add: times must be {t.shape[0]} integers")
            times = tm.astype(np.int64)
            if times.size and (times.min() < 0 or times.max() >= 1 << TIME_BITS):
                raise N.MiClipError(f"FrameLibrary.add: times must be in [0, 2^{TIME_BITS})")
        t = t.to(self.device).contiguous()
        if t.dtype == torch.float16:
            if t.shape[0]:
                t = normalize_rows_f16(t, out=t)
            self._groups[1].append(name, t, times)
        else:
            self._groups[0].append(name, t, times)
        self.dim = int(t.shape[1])
        self.names.append(name)

    def __len__(self):
        return sum(g.rows for g in self._groups)

    def segments(self):
        """[(name, global offset, rows, norm)] in global index order."""
        out, base = [], 0
        for g in self._groups:
            out += [(n, base + off, rows, g.norm) for n, off, rows in g.segments]
            base += g.rows
        return out

    def locate(self, index):
        """Global indices (any shape, tensor) -> (video_index int32, row int64), -1 for index -1."""
        import torch
        segs = self.segments()
        idx = index.to(torch.int64)
        if not segs:
            neg = torch.full_like(idx, -1)
            return neg.to(torch.int32), neg
        starts = torch.tensor([s[1] for s in segs], dtype=torch.int64, device=idx.device)
        vids = torch.tensor([self.names.index(s[0]) for s in segs], dtype=torch.int64, device=idx.device)
        valid = idx >= 0
        safe = torch.where(valid, idx, torch.zeros_like(idx))
        # the last segment starting at or before the index (empty videos share a start: the last
        # of them is the one that holds rows)
        seg = torch.searchsorted(starts, safe.reshape(-1), right=True).reshape(idx.shape) - 1
        row = torch.where(valid, safe - starts[seg], torch.full_like(idx, -1))
        vid = torch.where(valid, vids[seg], torch.full_like(idx, -1)).to(torch.int32)
        return vid, row

    # ----------------------------------------------------------------- search
    def _ranges(self, g, video, Q):
        """int64 [Q, 2] host ranges of each query in group ``g``'s rows."""
        if video is None or isinstance(video, str):
            video = [video] * Q
        if len(video) != Q:
            raise N.MiClipError(f"FrameLibrary.search: {len(video)} videos for {Q} queries")
        out = np.zeros((Q, 2), np.int64)
        for i, v in enumerate(video):
            if v is None:
                out[i] = (0, g.rows)
                continue
            if v not in self.names:
                raise N.MiClipError(f"FrameLibrary.search: unknown video {v!r}")
            s = g.segment(v)
            if s is not None:
                out[i] = (s[1], s[1] + s[2])
        return out

    def _mask(self, g, allow):
        """Packed mask words of group ``g`` for ``allow`` (None: no mask)."""
        import torch
        flags = self._flags(g, allow)
        return None if flags is None else pack_row_mask(torch.from_numpy(flags).to(self.device))

    def _flags(self, g, allow):
        """Host bool flags [rows] of group ``g`` for ``allow`` (None: no mask)."""
        if allow is None:
            return None
        flags = np.zeros(g.rows, np.bool_)
        for name, off, rows in g.segments:
            a = allow.get(name)
            if a is None or a is False:
                continue
            if a is True:
                flags[off:off + rows] = True
                continue
            a = np.asarray(a)
            if a.dtype == np.bool_:
                if a.shape != (rows,):
                    raise N.MiClipError(f"FrameLibrary.search: allow[{name!r}] has {a.shape} flags for {rows} rows")
                flags[off:off + rows] = a
            elif a.size:
                a = a.astype(np.int64).reshape(-1)
                if a.min() < 0 or a.max() >= rows:
                    raise N.MiClipError(f"FrameLibrary.search: allow[{name!r}] holds a row outside [0, {rows})")
                flags[off + a] = True
        return flags

    def _fill(self, q, s, i, count, pool_i, k, pool, theta, video, allow, nan_policy):
        """The refill rounds of a distinct search (``rank_topk_distinct(fill=True)`` over two
        corpora): per query left short by a full pool, one mask per non-empty group, starting
        from ``allow`` and the query's video range; ``exclude_similar`` on each group with the
        same gathered hit rows, the filtered pass per group, ``merge_topk`` and the two-corpus
        ``collapse_topk`` as in round 1.  Counts add up over the groups (a row belongs to one)."""
        import torch
        Q = q.shape[0]
        groups, base = [], 0
        for g in self._groups:
            if g.rows:
                groups.append((g, base, self._flags(g, allow), self._ranges(g, video, Q)))
                base += g.rows
        second = groups[1][0].corpus() if len(groups) > 1 else None
        state = torch.stack([(i >= 0).sum(dim=1), (pool_i[:, pool - 1] >= 0).to(torch.int64)], dim=1).tolist()
        for qi, (have, full) in enumerate(state):   # (a host read: the rounds synchronise)
            if not full and have < k:
                continue   # the pool held every visible row
            masks = []
            for g, _, flags, rng in groups:
                vis = np.zeros(g.rows, np.bool_)
                vis[rng[qi, 0]:rng[qi, 1]] = True if flags is None else flags[rng[qi, 0]:rng[qi, 1]]
                masks.append(pack_row_mask(torch.from_numpy(vis).to(self.device)))
            new, rounds, counts = i[qi, :have], 1, []
            while True:
                assert rounds <= k, "FrameLibrary.search: a full pool's first candidate is always accepted"
                vec = torch.empty((new.shape[0], self.dim), dtype=torch.float32, device=self.device)
                for g, b, _, _ in groups:
                    here = (new >= b) & (new < b + g.rows)
                    vec[here] = g.corpus().index_select(0, new[here] - b).float()
                cnt = 0
                for (g, b, _, _), m in zip(groups, masks):
                    cnt = cnt + exclude_similar(g.corpus(), vec, new, theta, row_mask=m, index_base=b, out=m,
                                                count=True)[1]
                counts.append(cnt)
                if have >= k or not full:
                    break
                cand = [rank_topk_filtered(g.corpus(), q[qi:qi + 1], pool, row_mask=m, index_base=b, norm=g.norm,
                                           nan_policy=nan_policy) for (g, b, _, _), m in zip(groups, masks)]
                s2, i2 = cand[0] if len(cand) == 1 else merge_topk(
                    torch.cat([c[0] for c in cand], dim=1), torch.cat([c[1] for c in cand], dim=1), pool,
                    nan_policy=nan_policy)
                ns, ni, _, _ = collapse_topk(groups[0][0].corpus(), s2, i2, k - have, theta, corpus2=second)
                rounds += 1
                got, full = torch.stack([(ni[0] >= 0).sum(), (i2[0, pool - 1] >= 0).to(torch.int64)]).tolist()
                if got == 0:
                    break
                s[qi, have:have + got] = ns[0, :got]
                i[qi, have:have + got] = ni[0, :got]
                new = ni[0, :got]
                have += got
            count[qi, :have] = torch.cat(counts)
        return s, i, count

    def search(self, queries, k, video=None, allow=None, nan_policy="first", distinct=None, pool=None, fill=False):
        """Top-k frames per query over the library.

        ``video``: None (all videos), one name, or a length-Q list of names / None (each
        query's video is its row range).  ``allow``: None or a dict name -> True | bool
        array | index array of frame rows (the row mask); a video absent from the dict
        is excluded.  Returns (scores f32 [Q, k], video_index int32 [Q, k], row int64
        [Q, k]); video_index (into ``names``) and row (inside its video) are -1 and the
        score -inf in slots beyond a query's visible frames.  1 <= k <= 64.

        ``distinct=theta``: the top-k distinct frames instead.  ``pool`` candidates (default
        ``min(64, 3 k)``, k <= pool <= 64) are fetched through the same filtered pass and
        merge, then collapsed at cosine >= theta over both corpora (``collapse_topk``);
        returns (scores, video_index, row, count int32 [Q, k]), count = the pool's frames
        collapsed into the hit, itself included (0 in unused slots).

        ``fill=True`` (with ``distinct``): the distinct top-k of all visible frames instead of
        the pool's, by refill rounds (``retrieval.rank_topk_distinct(fill=True)``): a query
        that a full pool left short of k hits excludes everything similar to its hits and ranks
        again, until k hits or no visible frame is left.  count then covers every visible
        frame of the library.  Reads hit counts on the host between rounds."""
        import torch
        want = k
        if fill and distinct is None:
            raise N.MiClipError("FrameLibrary.search: fill is an option of a distinct search")
        if distinct is not None:
            pool = min(64, 3 * k) if pool is None else int(pool)
            if not 1 <= want <= pool <= 64:
                raise N.MiClipError(f"FrameLibrary.search: distinct needs 1 <= k <= pool <= 64 (k={want}, pool={pool})")
            k = pool
        elif pool is not None:
            raise N.MiClipError("FrameLibrary.search: pool is the candidate count of a distinct search")
        q = torch.as_tensor(queries)
        q = (q if q.dim() == 2 else q.reshape(1, -1)).to(device=self.device, dtype=torch.float32)
        Q = q.shape[0]
        if allow is not None:
            unknown = [n for n in allow if n not in self.names]
            if unknown:
                raise N.MiClipError(f"FrameLibrary.search: unknown video {unknown[0]!r} in allow")
        cand_s, cand_i, base = [], [], 0
        for g in self._groups:
            if g.rows == 0:
                continue
            rng = self._ranges(g, video, Q)
            mask = self._mask(g, allow)
            perm = None
            qg = q
            if Q > SORT_MIN_QUERIES:
                # a 32-query block then shares a narrow hull of ranges, which the kernel skips around
                perm = torch.from_numpy(np.argsort(rng[:, 0], kind="stable")).to(self.device)
                qg = q.index_select(0, perm)
                rng = rng[perm.cpu().numpy()]
            s, i = rank_topk_filtered(g.corpus(), qg, k, row_mask=mask,
                                      query_range=torch.from_numpy(rng).to(self.device), index_base=base,
                                      norm=g.norm, nan_policy=nan_policy)
            if perm is not None:
                su, iu = torch.empty_like(s), torch.empty_like(i)
                su[perm] = s
                iu[perm] = i
                s, i = su, iu
            cand_s.append(s)
            cand_i.append(i)
            base += g.rows
        if not cand_s:
            s = torch.full((Q, k), float("-inf"), dtype=torch.float32, device=self.device)
            i = torch.full((Q, k), -1, dtype=torch.int64, device=self.device)
        elif len(cand_s) == 1:
            s, i = cand_s[0], cand_i[0]
        else:
            s, i = merge_topk(torch.cat(cand_s, dim=1), torch.cat(cand_i, dim=1), k, nan_policy=nan_policy)
        if distinct is not None:
            live = [g for g in self._groups if g.rows]
            if not live:
                count = torch.zeros((Q, want), dtype=torch.int32, device=self.device)
                s, i = s[:, :want], i[:, :want]
            else:
                # the global index runs over the non-empty groups' corpora in this order
                second = live[1].corpus() if len(live) > 1 else None
                pool_i = i
                s, i, count, _ = collapse_topk(live[0].corpus(), s, i, want, distinct, corpus2=second)
                if fill:
                    s, i, count = self._fill(q, s, i, count, pool_i, want, pool, distinct, video, allow, nan_policy)
            vid, row = self.locate(i)
            return s, vid, row, count
        vid, row = self.locate(i)
        return s, vid, row

    def search_events(self, queries, k, threshold, max_gap, min_count=1, video=None, allow=None):
        """Top-k events per query over the library (``retrieval.event_topk``): the runs of frames
        scoring >= ``threshold`` whose consecutive times differ by at most ``max_gap`` (in the
        units of ``add``'s ``times``; a video added without times counts its rows), with at least
        ``min_count`` frames.  Events never cross videos.  ``video`` and ``allow`` are ``search``'s.

        Per non-empty corpus: ``score_matrix`` over the resident rows, the score columns gathered
        into time order when some video's times are not sorted, ``event_topk``; the two corpora's
        lists are merged by (peak score descending, global begin column ascending).

        Returns (score f32 [Q, k], video_index int32 [Q, k], peak_row, begin_row, end_row int64
        [Q, k], count int32 [Q, k], total int32 [Q]): the rows are the caller's row numbers
        inside the video of the event's best, first and last frame in time order; unused slots
        are -inf / -1 / -1 / -1 / -1 / 0.  ``total`` counts the query's qualifying events."""
        import torch
        if not 0 <= int(max_gap) < 1 << TIME_BITS:
            raise N.MiClipError(f"FrameLibrary.search_events: max_gap must be in [0, 2^{TIME_BITS})")
        q = torch.as_tensor(queries)
        q = (q if q.dim() == 2 else q.reshape(1, -1)).to(device=self.device, dtype=torch.float32)
        Q = q.shape[0]
        if allow is not None:
            unknown = [n for n in allow if n not in self.names]
            if unknown:
                raise N.MiClipError(f"FrameLibrary.search_events: unknown video {unknown[0]!r} in allow")
        found, col2idx, base = [], [], 0
        for g in self._groups:
            if g.rows == 0:
                continue
            perm, col_time, gather = g.time_order()
            rng = self._ranges(g, video, Q)          # a video's columns are its rows' range
            flags = self._flags(g, allow)
            scores = score_matrix(g.corpus(), q, norm=g.norm)
            perm_dev = torch.from_numpy(perm).to(self.device)
            if gather:
                scores = scores.index_select(1, perm_dev)
                flags = None if flags is None else flags[perm]
            mask = None if flags is None else pack_row_mask(torch.from_numpy(flags).to(self.device))
            found.append(event_topk(scores, threshold, k, max_gap=max_gap, min_count=min_count,
                                    row_time=torch.from_numpy(col_time).to(self.device), row_mask=mask,
                                    query_range=torch.from_numpy(rng).to(self.device), index_base=base))
            col2idx.append(perm_dev + base)
            base += g.rows
        if not found:
            neg = torch.full((Q, k), -1, dtype=torch.int64, device=self.device)
            return (torch.full((Q, k), float("-inf"), dtype=torch.float32, device=self.device), neg.to(torch.int32),
                    neg, neg.clone(), neg.clone(), torch.zeros((Q, k), dtype=torch.int32, device=self.device),
                    torch.zeros(Q, dtype=torch.int32, device=self.device))
        if len(found) == 1:
            s, peak, begin, end, count, total = found[0]
        else:
            cat = [torch.cat([f[j] for f in found], dim=1) for j in range(5)]
            s, begin = merge_topk(cat[0], cat[2], k)
            # begin is unique among a query's events: the payload is gathered by it (an empty slot
            # finds an empty slot)
            src = (cat[2].unsqueeze(1) == begin.unsqueeze(2)).to(torch.int8).argmax(dim=2)
            peak, end, count = (cat[j].gather(1, src) for j in (1, 3, 4))
            total = found[0][5] + found[1][5]
        col2idx = torch.cat(col2idx)

        def rows_of(col):
            safe = torch.where(col >= 0, col, torch.zeros_like(col))
            return self.locate(torch.where(col >= 0, col2idx[safe], col))

        vid, begin_row = rows_of(begin)
        return s, vid, rows_of(peak)[1], begin_row, rows_of(end)[1], count, total
