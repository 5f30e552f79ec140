"""The exclusion-mask pass (include/miclip.h mi_rank_exclude) and the filled
distinct top-k built on it, stated in NumPy float64: what csrc/rank_exclude.hip and
``rank_topk_distinct(fill=True)`` must return."""
import numpy as np

from collapse_ref import collapse_ref, cosines


def exclude_ref(rows64, hits64, hit_index, theta, mask_in):
    """``rows64`` [N, D]: the stored rows; ``hits64`` [H, D]: the hits' rows; ``hit_index`` [H]
    (row numbers, already relative to the corpus; outside [0, N) = names no row) or None;
    ``mask_in`` bool [N] or None (every row visible).  Returns (mask bool [N], count int32 [H]):
    a visible row is removed when it is similar to some hit or a hit names it, and counted for
    the lowest similar slot, else for the lowest slot naming it.  Any H (the chained calls of
    32 hits add up to this one statement)."""
    rows64 = np.asarray(rows64, np.float64)
    hits64 = np.asarray(hits64, np.float64).reshape(-1, rows64.shape[1])
    n, H = rows64.shape[0], hits64.shape[0]
    vis = np.ones(n, bool) if mask_in is None else np.asarray(mask_in, bool).copy()
    sim = np.zeros((n, H), bool)
    for b in range(0, n, 128):   # collapse_ref's cosine, a block of rows at a time
        e = min(n, b + 128)
        cos, valid = cosines(np.vstack([rows64[b:e], hits64]))
        with np.errstate(invalid="ignore"):   # NaN >= theta is False
            sim[b:e] = (cos[:e - b, e - b:] >= theta) & valid[:e - b, None] & valid[None, e - b:]
    named = np.zeros((n, H), bool)
    if hit_index is not None:
        for m, r in enumerate(np.asarray(hit_index, np.int64).reshape(-1)):
            if 0 <= r < n:
                named[r, m] = True
    removed = vis & (sim.any(axis=1) | named.any(axis=1))
    slot = np.where(sim.any(axis=1), sim.argmax(axis=1), named.argmax(axis=1))   # argmax: the first True
    count = np.bincount(slot[removed], minlength=H).astype(np.int32)
    return vis & ~removed, count


def fill_ref(rows64, ranking, k, theta):
    """The filled distinct top-k: the collapse walk over the full visible ranking.
    Returns (hit int64 [k], count int32 [k])."""
    hit, count, _ = collapse_ref(rows64, ranking, k, theta)
    return hit, count


def rounds_ref(rows64, ranking, k, theta, pool):
    """The round loop: collapse the first ``pool`` visible rows of the ranking into the remaining
    slots, exclude everything similar to the new hits, again; until k hits or a short pool.
    Returns (hit int64 [k], count int32 [k], rounds)."""
    rows64 = np.asarray(rows64, np.float64)
    ranking = np.asarray(ranking, np.int64).reshape(-1)
    n = rows64.shape[0]
    vis = np.zeros(n, bool)
    vis[ranking] = True
    hit = np.full(k, -1, np.int64)
    count = np.zeros(k, np.int32)
    have, rounds = 0, 0
    while True:
        cand = ranking[vis[ranking]][:pool]
        rounds += 1
        assert rounds <= max(k, 1)
        new, _, _ = collapse_ref(rows64, cand, k - have, theta)
        new = new[new >= 0]
        if len(new) == 0:
            break
        vis, cnt = exclude_ref(rows64, rows64[new], new, theta, vis)
        hit[have:have + len(new)] = new
        count[have:have + len(new)] = cnt
        have += len(new)
        if have >= k or len(cand) < pool:
            break
    return hit, count, rounds
