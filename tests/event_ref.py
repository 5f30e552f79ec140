"""The statement of event search (include/miclip.h mi_event_topk) as a serial NumPy loop over one
query's scores: no cleverness.

Column t is HOT iff it is visible (mask[t], lo <= t < hi) and scores[t] >= tau (false for a NaN
score or a NaN tau).  Two hot columns a < b with no hot column between them are LINKED iff
time[b] - time[a] <= max_gap.  An EVENT is a maximal chain of linked hot columns: begin, end (first
and last hot column), count (hot columns), peak (largest score), peak_col (lowest column attaining
it).  It QUALIFIES iff count >= min_count.  Order: peak descending, then begin ascending.
"""
import numpy as np


def event_ref(scores, tau, max_gap=0, min_count=1, times=None, mask=None, rng=None):
    """-> (records, total): records = the query's qualifying events in order, each
    (peak_score f32, peak_col, begin, end, count); total = len(records)."""
    s = np.asarray(scores, np.float32)
    n = s.shape[0]
    tau = np.float32(tau)
    lo, hi = (0, n) if rng is None else (max(int(rng[0]), 0), min(int(rng[1]), n))
    events, cur, last_t = [], None, None
    for t in range(n):
        if not (lo <= t < hi) or (mask is not None and not mask[t]):
            continue
        if not (s[t] >= tau):          # NaN compares false
            continue
        tm = int(times[t]) if times is not None else t
        if cur is not None and tm - last_t <= max_gap:
            cur["end"] = t
            cur["count"] += 1
            if s[t] > cur["peak"]:     # strictly: the lowest column keeps a tie
                cur["peak"], cur["peak_col"] = s[t], t
        else:
            if cur is not None:
                events.append(cur)
            cur = {"begin": t, "end": t, "count": 1, "peak": s[t], "peak_col": t}
        last_t = tm
    if cur is not None:
        events.append(cur)
    good = [e for e in events if e["count"] >= min_count]
    good.sort(key=lambda e: (-float(e["peak"]), e["begin"]))
    return [(np.float32(e["peak"]), e["peak_col"], e["begin"], e["end"], e["count"]) for e in good], len(good)


def event_ref_arrays(scores, tau, k, max_gap=0, min_count=1, times=None, mask=None, rng=None, index_base=0):
    """The [Q, k] output arrays of mi_event_topk for a [Q, N] score matrix: (score, peak, begin,
    end, count, total); tau a scalar or [Q]; rng None, one (lo, hi) or [Q, 2]."""
    s = np.asarray(scores, np.float32)
    Q = s.shape[0]
    tau = np.broadcast_to(np.asarray(tau, np.float32), (Q,))
    r = None if rng is None else np.broadcast_to(np.asarray(rng, np.int64), (Q, 2))
    o_s = np.full((Q, k), -np.inf, np.float32)
    o_p, o_b, o_e = (np.full((Q, k), -1, np.int64) for _ in range(3))
    o_c = np.zeros((Q, k), np.int32)
    o_t = np.zeros(Q, np.int32)
    for q in range(Q):
        recs, o_t[q] = event_ref(s[q], tau[q], max_gap, min_count, times, mask, None if r is None else r[q])
        for j, (ps, pc, b, e, c) in enumerate(recs[:k]):
            o_s[q, j], o_p[q, j], o_b[q, j], o_e[q, j], o_c[q, j] = ps, index_base + pc, index_base + b, index_base + e, c
    return o_s, o_p, o_b, o_e, o_c, o_t


def real_case(rows):
    """The real-row case of the host and GPU tests: every row of a fixture corpus as a query.
    -> (float64 scores [n, n] of the L2-normalised rows, tau [n], half_gap [n]): tau_i is the
    midpoint of the largest gap between consecutive sorted scores at ranks 20 .. 60 (between 20 and
    60 hot frames per query), half_gap_i its distance to the nearest score."""
    rows = np.asarray(rows, np.float64)
    unit = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    s = unit @ unit.T
    sd = -np.sort(-s, axis=1)
    gaps = sd[:, 20:60] - sd[:, 21:61]
    j = gaps.argmax(axis=1)
    i = np.arange(s.shape[0])
    return s, (sd[i, 20 + j] + sd[i, 21 + j]) / 2, gaps[i, j] / 2
