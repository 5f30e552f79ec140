"""The distinct top-k collapse (mi_rank_collapse, csrc/rank_collapse.hip) beside the mi_rank_topk
call that produced its pool: ONE process, interleaved rounds, HIP events on the launch stream.

  python scripts/rank_collapse_micro.py [rounds]

Shapes (Q, P, D): (1, 60, 512), (32, 64, 512), (32, 64, 768), each over 125,000 and 1,000,000 f32
rows, k = 10, threshold 0.9.  The corpus is planted with near-duplicates (groups of four rows at
cosine ~0.99), so the pools hold frames to collapse.  Per (shape, rows) two cases:
  pool      retrieval.rank_topk(corpus, q, P): the pool call
  collapse  retrieval.collapse_topk on that pool
Per case: min / median / max of the rounds' mean call time (20 calls per round).  The 20 calls of
a round are enqueued behind a ~10 ms device spin, so the events bracket back-to-back device work
and not the host's enqueue rate (host_us_per_call is reported beside it).
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
SHAPES = ((1, 60, 512), (32, 64, 512), (32, 64, 768))
ROWS = (125_000, 1_000_000)
K, THETA = 10, 0.9


def planted(n, d, dev, g):
    base = torch.randn(n // 4, d, device=dev, generator=g)
    rows = base.repeat_interleave(4, dim=0)
    rows += 0.08 * torch.randn(n, d, device=dev, generator=g)
    return rows


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)
    stream = torch.cuda.current_stream(dev)
    res = {}
    for n in ROWS:
        for d in sorted({s[2] for s in SHAPES}):
            corpus = planted(n, d, dev, g)
            for Q, P, D in SHAPES:
                if D != d:
                    continue
                # queries near corpus rows: their pools are full of near-duplicates
                q = corpus[torch.randint(0, n, (Q,), device=dev, generator=g)] + \
                    0.5 * torch.randn(Q, d, device=dev, generator=g)
                pool_s, pool_i = retrieval.rank_topk(corpus, q, P)
                cases = {"pool": lambda: retrieval.rank_topk(corpus, q, P),
                         "collapse": lambda: retrieval.collapse_topk(corpus, pool_s, pool_i, K, THETA)}
                _, hit, count, _ = cases["collapse"]()
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
                key = f"rows{n}_Q{Q}_P{P}_D{D}"
                res[key] = {c: {"us_min": round(min(t), 1), "us_median": round(statistics.median(t), 1),
                                "us_max": round(max(t), 1), "host_us_per_call": round(statistics.median(host[c]), 1)}
                            for c, t in times.items()}
                res[key]["hits_per_query"] = round(float((hit >= 0).sum()) / Q, 2)
                res[key]["pool_frames_per_hit"] = round(float(count.sum()) / max(int((hit >= 0).sum()), 1), 2)
                res[key]["collapse_over_pool"] = round(res[key]["collapse"]["us_median"] / res[key]["pool"]["us_median"], 3)
                print(key, json.dumps(res[key]), flush=True)
            del corpus
    print(json.dumps({"rank_collapse_micro": res, "rounds": rounds, "calls_per_round": CALLS, "k": K,
                      "threshold": THETA}))


if __name__ == "__main__":
    main()
