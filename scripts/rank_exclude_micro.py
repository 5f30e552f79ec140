"""The exclusion-mask pass (mi_rank_exclude, csrc/rank_exclude.hip) beside the unchanged
mi_rank_topk_filtered call over the same rows, and the filled distinct search beside the un-filled
one: ONE process, product build, interleaved rounds, HIP events on the launch stream.

  python scripts/rank_exclude_micro.py [rounds]
  rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python scripts/rank_exclude_micro.py --trace
  python scripts/rank_exclude_micro.py --summarise DIR/NAME_results.db

Mask pass, 1M x 512 f32 rows, H = 32 hits (corpus rows), threshold 0.9; per case min / median / max
of the rounds' mean call time (20 calls per round, enqueued behind a ~10 ms device spin, so the
events bracket back-to-back device work and not the host's enqueue rate):
  filtered_all    retrieval.rank_topk_filtered(corpus, q, 10), Q = 32, everything visible
  exclude_all     retrieval.exclude_similar(..., count=True), everything visible
  filtered_words  the filtered call under a mask with 1/16 of the 32-row words set
                  (scripts/rank_filter_micro.py's case e)
  exclude_words   the mask pass under that mask
--trace runs each case 10 times with no timing, for a kernel trace of its own.

Whole search, 125k x 512 f32 rows, 90 % of them one planted near-duplicate cluster, the query
inside it, k = 10, pool 30: rank_topk_distinct with and without fill=True, wall time per call
around a device synchronise (the filled search synchronises between rounds itself), the rounds it
took (1 + its filtered passes) and the hits both return.
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "event-retrival-in-video-learning-transferable-visual-model-from-supervised-natural-language_amd"))

import torch  # noqa: E402
from miclip import retrieval  # noqa: E402

CALLS = 20
N, D, Q, H, K, THETA = 1_000_000, 512, 32, 32, 10, 0.9
SEARCH_N, SEARCH_POOL = 125_000, 30


def mask_pass(dev, g, rounds, trace):
    stream = torch.cuda.current_stream(dev)
    corpus = torch.randn(N, D, device=dev, generator=g)
    q = torch.nn.functional.normalize(torch.randn(Q, D, device=dev, generator=g), dim=1)
    idx = torch.randint(0, N, (H,), device=dev, generator=g)
    hits = corpus.index_select(0, idx)
    words = (N + 31) // 32
    w_live = torch.rand(words, device=dev, generator=g) < 1 / 16
    p_words = retrieval.pack_row_mask(w_live.repeat_interleave(32)[:N].contiguous())
    out = torch.empty(words, dtype=torch.int32, device=dev)
    cases = {
        "filtered_all": lambda: retrieval.rank_topk_filtered(corpus, q, K),
        "exclude_all": lambda: retrieval.exclude_similar(corpus, hits, idx, THETA, out=out, count=True),
        "filtered_words": lambda: retrieval.rank_topk_filtered(corpus, q, K, row_mask=p_words),
        "exclude_words": lambda: retrieval.exclude_similar(corpus, hits, idx, THETA, row_mask=p_words, out=out,
                                                           count=True),
    }
    # random rows are similar to themselves alone: each hit removes its own row (once per distinct row)
    _, count = cases["exclude_all"]()
    assert int(count.sum()) == int(idx.unique().numel()), count.tolist()
    mask, count = cases["exclude_words"]()
    live = w_live[idx // 32]
    assert int(count.sum()) == int(idx[live].unique().numel()), count.tolist()
    if trace:
        for fn in cases.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize(dev)
        return {}
    times = {c: [] for c in cases}
    host = {c: [] for c in cases}
    for _ in range(rounds):
        for c, fn in cases.items():
            fn()
            torch.cuda.synchronize(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda._sleep(20_000_000)   # ~10 ms: the calls below queue up behind it
            e0.record(stream)
            h0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            host[c].append((time.perf_counter() - h0) * 1e6 / CALLS)
            e1.record(stream)
            torch.cuda.synchronize(dev)
            times[c].append(e0.elapsed_time(e1) * 1000 / CALLS)
    res = {c: {"us_min": round(min(t), 1), "us_median": round(statistics.median(t), 1), "us_max": round(max(t), 1),
               "host_us_per_call": round(statistics.median(host[c]), 1)} for c, t in times.items()}
    res["live_words"] = int(w_live.sum())
    res["words"] = words
    for a, b in (("exclude_all", "filtered_all"), ("exclude_words", "filtered_words")):
        res[f"{a}_over_{b}"] = round(res[a]["us_median"] / res[b]["us_median"], 3)
    return res


def whole_search(dev, g, rounds):
    n_dup = SEARCH_N * 9 // 10
    centre = torch.randn(1, D, device=dev, generator=g)
    rows = torch.randn(SEARCH_N, D, device=dev, generator=g)
    dup = torch.randperm(SEARCH_N, device=dev, generator=g)[:n_dup]
    rows[dup] = centre + 0.02 * torch.randn(n_dup, D, device=dev, generator=g)
    q = centre + 0.02 * torch.randn(1, D, device=dev, generator=g)
    passes = [0]
    filtered = retrieval.rank_topk_filtered

    def counted(*a, **kw):
        passes[0] += 1
        return filtered(*a, **kw)

    cases = {"unfilled": lambda: retrieval.rank_topk_distinct(rows, q, K, THETA, pool=SEARCH_POOL),
             "filled": lambda: retrieval.rank_topk_distinct(rows, q, K, THETA, pool=SEARCH_POOL, fill=True)}
    short = cases["unfilled"]()
    retrieval.rank_topk_filtered = counted   # the rounds of one untimed call; restored before any timing
    try:
        full = cases["filled"]()
    finally:
        retrieval.rank_topk_filtered = filtered
    n_rounds = 1 + passes[0]
    times = {c: [] for c in cases}
    for _ in range(rounds):
        for c, fn in cases.items():
            fn()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(CALLS):
                fn()
            torch.cuda.synchronize(dev)
            times[c].append((time.perf_counter() - t0) * 1e6 / CALLS)
    res = {c: {"us_min": round(min(t), 1), "us_median": round(statistics.median(t), 1), "us_max": round(max(t), 1)}
           for c, t in times.items()}
    res["rounds"] = n_rounds
    res["us_per_round"] = round(res["filled"]["us_median"] / n_rounds, 1)
    res["hits_unfilled"] = int((short[1] >= 0).sum())
    res["hits_filled"] = int((full[1] >= 0).sum())
    res["first_hit_count"] = int(full[2][0, 0])
    return res


def summarise(db):
    """Per-kernel times of a --trace run from rocprofv3's database: the two cases of a kernel
    differ by more than 2x, so its dispatches split at 250 us into all-visible and 1/16-words."""
    import sqlite3
    con = sqlite3.connect(db)
    for kernel in ("rank_exclude_kernel", "rank_exclude_sum", "rank_filter_stream", "rank_merge_kernel"):
        us = [r[0] / 1000.0 for r in con.execute('select "end" - start from kernels where name like ? order by start',
                                                  (f"%{kernel}%",))]
        for case, v in (("all", [x for x in us if x > 250]), ("words_or_small", [x for x in us if x <= 250])):
            if v:
                print(f"{kernel} {case}: n {len(v)} median {statistics.median(v):.1f} us "
                      f"min {min(v):.1f} max {max(v):.1f}")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        return summarise(sys.argv[2])
    trace = "--trace" in sys.argv[1:]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 5
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)
    mp = mask_pass(dev, g, rounds, trace)
    if trace:
        return
    print(f"mask_pass rows{N}_D{D}_H{H}", json.dumps(mp), flush=True)
    ws = whole_search(dev, g, rounds)
    print(f"whole_search rows{SEARCH_N}_D{D}_k{K}_pool{SEARCH_POOL}", json.dumps(ws), flush=True)
    print(json.dumps({"rank_exclude_micro": {"mask_pass": mp, "whole_search": ws}, "rounds": rounds,
                      "calls_per_round": CALLS, "threshold": THETA}))


if __name__ == "__main__":
    main()
