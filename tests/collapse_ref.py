"""The distinct top-k walk (include/miclip.h mi_rank_collapse) stated in NumPy
float64: what csrc/rank_collapse.hip must return for a candidate list."""
import numpy as np


def cosines(rows64):
    """(cos [n, n] float64, valid [n]): valid rows have a finite, non-zero sum of squares."""
    r = np.asarray(rows64, np.float64)
    with np.errstate(all="ignore"):
        n2 = (r * r).sum(axis=1)
        valid = np.isfinite(n2) & (n2 > 0)
        nrm = np.sqrt(np.where(valid, n2, 1.0))
        cos = (r @ r.T) / np.outer(nrm, nrm)
    return cos, valid


def collapse_ref(rows64, cand_index, k, theta):
    """``rows64`` [n, D]: the stored rows (widened), addressed by the entries of ``cand_index``
    [P] (a ranked list; negative or >= n = empty slot).  Returns (hit int64 [k] = the accepted
    candidates' indices, -1 padded; count int32 [k]; slot int32 [P])."""
    rows64 = np.asarray(rows64, np.float64)
    cand = np.asarray(cand_index, np.int64).reshape(-1)
    P = cand.shape[0]
    present = (cand >= 0) & (cand < rows64.shape[0])
    cos, valid = cosines(rows64[np.where(present, cand, 0)]) if P else (np.zeros((0, 0)), np.zeros(0, bool))
    hit = np.full(k, -1, np.int64)
    count = np.zeros(k, np.int32)
    slot = np.full(P, -1, np.int32)
    taken = []                          # candidate positions of the accepted hits, slot order
    for j in range(P):
        if not present[j]:
            continue
        s = -1
        for t, i in enumerate(taken):   # the lowest slot wins
            if valid[i] and valid[j] and cos[i, j] >= theta:
                s = t
                break
        if s < 0 and len(taken) < k:
            s = len(taken)
            taken.append(j)
            hit[s] = cand[j]
        if s >= 0:
            count[s] += 1
        slot[j] = s
    return hit, count, slot


def min_margin(rows64, pool, theta):
    """The smallest |cos - theta| over the pairs of the pool's valid rows (inf without a pair)."""
    pool = np.asarray(pool, np.int64).reshape(-1)
    pool = pool[(pool >= 0) & (pool < np.asarray(rows64).shape[0])]
    cos, valid = cosines(np.asarray(rows64, np.float64)[pool])
    iu = np.triu_indices(len(pool), 1)
    ok = valid[iu[0]] & valid[iu[1]]
    d = np.abs(cos[iu][ok] - theta)
    return float(d.min()) if d.size else float("inf")
