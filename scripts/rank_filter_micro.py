"""The filtered rank pass (mi_rank_topk_filtered, csrc/rank_filter.hip) beside mi_rank_topk on
one shape, ONE process, interleaved rounds, HIP events on the launch stream.

  python scripts/rank_filter_micro.py [rounds] [rows]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o rf -- python scripts/rank_filter_micro.py --trace
  python scripts/rank_filter_micro.py --summarise DIR/.../rf_kernel_trace.csv

Shape: rows x 512 f32 (default 1M), Q = 32, k = 10.  Cases:
  a_topk          mi_rank_topk as the product runs it (certified pass + gated exact pass here)
  stream          mi_rank_topk through rank_stream, the kernel the filtered pass shares its body with
                  (A/B build: MICLIP_RANK_REG=0)
  b_all           filtered, no mask and no range: everything visible
  c_range_eighth  filtered, every query ranged to the same eighth of the rows
  d_mask_random   filtered, a random row mask of density 1/16 (nearly every 32-row word is live)
  e_mask_words    filtered, a mask with 1/16 of the 32-row words set (whole words)
Each case is checked first: b equals a bit for bit, c / d / e equal mi_rank_topk over the gathered
visible rows.  Per case: min / median / max of the rounds' mean call time (20 calls per round), so
the spread of a_topk between rounds is on the same line as the differences.  The 20 calls of a
round are enqueued behind a ~10 ms device spin, so the events bracket back-to-back device work
and not the host's enqueue rate (host_us_per_call is reported beside it: a short case is otherwise
host-bound).  --trace runs every case 2 + 20 times with nothing else, for a kernel trace;
--summarise prints the per-kernel times of such a trace per case (the filtered cases share kernel
names: their dispatches are split by order, 22 per case, the first 2 dropped).
"""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "event-retrival-in-video-learning-transferable-visual-model-from-supervised-natural-language_amd"))
os.environ.setdefault("MICLIP_LIB", "ab")   # A/B build: the MICLIP_RANK_REG switch

import torch  # noqa: E402
from miclip import retrieval  # noqa: E402

CALLS = 20
SWITCHES = ("MICLIP_RANK_REG", "MICLIP_RANK_CERT")


FILTERED = ("b_all", "c_range_eighth", "d_mask_random", "e_mask_words")
WARM = 2


def summarise(path):
    import csv
    import re
    rows = list(csv.DictReader(open(path)))
    col = {k.lower(): k for k in rows[0]}
    name, t0, t1 = col["kernel_name"], col["start_timestamp"], col["end_timestamp"]
    rows.sort(key=lambda r: int(r[t0]))
    by = {}
    for r in rows:
        m = re.search(r"(rank_filter_stream|rank_filter_tiles|rank_merge_kernel|rank_stream|fold_merge_kernel|"
                      r"rank_reg|rank_cert\w*|rescore\w*)", r[name])
        if m:
            by.setdefault(m.group(1), []).append((int(r[t1]) - int(r[t0])) / 1e3)
    out = {}
    for k, d in by.items():
        if k in ("rank_filter_stream", "rank_merge_kernel") and len(d) == len(FILTERED) * (WARM + CALLS):
            for j, c in enumerate(FILTERED):
                part = d[j * (WARM + CALLS) + WARM:(j + 1) * (WARM + CALLS)]
                out[f"{c}:{k}"] = {"calls": len(part), "us_avg": round(sum(part) / len(part), 1),
                                   "us_min": round(min(part), 1), "us_max": round(max(part), 1)}
        else:
            out[k] = {"calls": len(d), "us_avg": round(sum(d) / len(d), 1), "us_min": round(min(d), 1),
                      "us_max": round(max(d), 1)}
    for k in sorted(out):
        print(k, json.dumps(out[k]))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--summarise":
        return summarise(sys.argv[2])
    trace = len(sys.argv) > 1 and sys.argv[1] == "--trace"
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rounds = int(args[0]) if len(args) > 0 else 5
    N = int(args[1]) if len(args) > 1 else 1_000_000
    D, Q, k = 512, 32, 10
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(3)
    corpus = torch.randn(N, D, device=dev, generator=g)
    q = torch.nn.functional.normalize(torch.randn(Q, D, device=dev, generator=g), dim=1)
    eighth = torch.tensor([[3 * (N // 8), 4 * (N // 8)]] * Q, dtype=torch.int64, device=dev)
    m_rand = torch.rand(N, device=dev, generator=g) < 1 / 16
    words = (N + 31) // 32
    w_live = torch.rand(words, device=dev, generator=g) < 1 / 16
    m_words = w_live.repeat_interleave(32)[:N].contiguous()
    p_rand, p_words = retrieval.pack_row_mask(m_rand), retrieval.pack_row_mask(m_words)

    def topk(env):
        def run():
            for s in SWITCHES:
                os.environ.pop(s, None)
            os.environ.update(env)
            return retrieval.rank_topk(corpus, q, k)
        return run

    cases = {
        "a_topk": topk({}),
        "stream": topk({"MICLIP_RANK_REG": "0", "MICLIP_RANK_CERT": "0"}),
        "b_all": lambda: retrieval.rank_topk_filtered(corpus, q, k),
        "c_range_eighth": lambda: retrieval.rank_topk_filtered(corpus, q, k, query_range=eighth),
        "d_mask_random": lambda: retrieval.rank_topk_filtered(corpus, q, k, row_mask=p_rand),
        "e_mask_words": lambda: retrieval.rank_topk_filtered(corpus, q, k, row_mask=p_words),
    }

    def same(a, b, what):
        assert torch.equal(a[1], b[1]) and torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)), what

    def gathered(vis):
        s, i = retrieval.rank_topk(corpus.index_select(0, vis), q, k)
        return s, vis[i]

    if trace:   # every case WARM + CALLS times, in order, and nothing else on the device
        for c, fn in cases.items():
            for _ in range(WARM + CALLS):
                fn()
            torch.cuda.synchronize(dev)
        return
    ref = cases["a_topk"]()
    same(cases["stream"](), ref, "stream")
    same(cases["b_all"](), ref, "b_all")
    same(cases["c_range_eighth"](), gathered(torch.arange(3 * (N // 8), 4 * (N // 8), device=dev)), "c_range_eighth")
    same(cases["d_mask_random"](), gathered(m_rand.nonzero().flatten()), "d_mask_random")
    same(cases["e_mask_words"](), gathered(m_words.nonzero().flatten()), "e_mask_words")
    print(json.dumps({"checked": "b == a; c, d, e == mi_rank_topk over the gathered visible rows (bitwise)",
                      "rows": N, "D": D, "Q": Q, "k": k, "visible_d": int(m_rand.sum()), "visible_e": int(m_words.sum()),
                      "live_words_d": int(m_rand.view(-1)[:words * 32 - 32].view(-1, 32).any(1).sum())}), flush=True)

    stream = torch.cuda.current_stream(dev)
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
    nb = corpus.numel() * corpus.element_size()
    res = {c: {"us_min": round(min(t), 1), "us_median": round(statistics.median(t), 1), "us_max": round(max(t), 1),
               "host_us_per_call": round(statistics.median(host[c]), 1),
               "corpus_gbs_at_min": round(nb / min(t) / 1e3, 1)} for c, t in times.items()}
    for c, r in res.items():
        print(c, json.dumps(r), flush=True)
    print(json.dumps({"rank_filter_micro": res, "rounds": rounds, "calls_per_round": CALLS}))


if __name__ == "__main__":
    main()
