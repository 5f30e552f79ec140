"""Event search (mi_event_topk, csrc/rank_events.hip) beside the mi_score_matrix call that feeds it:
ONE process, product build, interleaved rounds, HIP events on the launch stream.

  python scripts/event_micro.py [rounds]
  rocprofv3 --kernel-trace --stats -d DIR -o NAME -- python scripts/event_micro.py --trace
  python scripts/event_micro.py --summarise DIR/NAME_results.db

1M x 512 f32 rows, Q = 1 and Q = 32, k = 10, max_gap = 1, NULL times; per case min / median / max of
the rounds' mean call time (20 calls per round, enqueued behind a ~10 ms device spin, so the events
bracket back-to-back device work and not the host's enqueue rate):
  score      retrieval.score_matrix(corpus, q, norm="l2"): reads the corpus, writes [Q, N] f32
  sparse     retrieval.event_topk on those scores, threshold = each query's 99th percentile
  dense      ... its median (about half the columns hot, events of a few columns)
  all_hot    ... -inf: one event of N columns per query
By bytes the event call reads the scores twice (2 x 4 Q N) against the corpus' 4 N D.
--trace runs each case 10 times with no timing, for a kernel trace of its own.
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
N, D, K, GAP = 1_000_000, 512, 10, 1


def run(dev, corpus, Q, g, rounds, trace):
    stream = torch.cuda.current_stream(dev)
    q = torch.nn.functional.normalize(torch.randn(Q, D, device=dev, generator=g), dim=1)
    scores = retrieval.score_matrix(corpus, q, norm="l2")
    tau = {"sparse": scores.kthvalue(N - N // 100, dim=1).values.contiguous(),
           "dense": scores.kthvalue(N // 2, dim=1).values.contiguous(),
           "all_hot": torch.full((Q,), float("-inf"), device=dev)}
    cases = {"score": lambda: retrieval.score_matrix(corpus, q, norm="l2")}
    for name, t in tau.items():
        cases[name] = lambda t=t: retrieval.event_topk(scores, t, K, max_gap=GAP)
    shape = {}
    for name in tau:
        out = cases[name]()
        total, count = out[5].tolist(), out[4][:, 0].tolist()
        shape[name] = {"events_min": min(total), "events_max": max(total), "best_event_frames_max": max(count)}
    assert shape["all_hot"]["events_max"] == 1 and shape["all_hot"]["best_event_frames_max"] == N, shape
    hot = (scores >= tau["sparse"][:, None]).sum(dim=1)
    assert int(hot.min()) >= N // 100 and int(hot.max()) <= N // 100 + 64, hot.tolist()
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
    for name in tau:
        res[name].update(shape[name])
        res[f"{name}_over_score"] = round(res[name]["us_median"] / res["score"]["us_median"], 3)
    res["block_cols"] = retrieval.event_block_cols(N)
    return res


def summarise(db):
    """Per-kernel times of a --trace run from rocprofv3's database."""
    import sqlite3
    con = sqlite3.connect(db)
    rows = list(con.execute('select name, "end" - start from kernels order by start'))
    for kernel in ("event_walk<false>", "event_scan", "event_walk<true>", "event_reduce", "score"):
        us = [ns / 1000.0 for name, ns in rows if kernel in name or kernel.replace("<false>", "ILb0").replace("<true>", "ILb1") in name]
        # the Q = 1 and the Q = 32 dispatches of a kernel differ several-fold: report the two halves apart
        us.sort()
        for part, v in (("fast half (Q = 1)", us[:len(us) // 2]), ("slow half (Q = 32)", us[len(us) // 2:])):
            if v:
                print(f"{kernel} {part}: n {len(v)} median {statistics.median(v):.1f} us min {min(v):.1f} max {max(v):.1f}")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        return summarise(sys.argv[2])
    trace = "--trace" in sys.argv[1:]
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if args else 5
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)
    corpus = torch.randn(N, D, device=dev, generator=g)
    out = {}
    for Q in (1, 32):
        res = run(dev, corpus, Q, g, rounds, trace)
        if not trace:
            print(f"events rows{N}_D{D}_Q{Q}_k{K}", json.dumps(res), flush=True)
            out[f"Q{Q}"] = res
    if not trace:
        print(json.dumps({"event_micro": out, "rounds": rounds, "calls_per_round": CALLS, "max_gap": GAP}))


if __name__ == "__main__":
    main()
