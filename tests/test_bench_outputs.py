"""bench.py's plain run, --full and --dump-outputs.

* dump_outputs writes the step's four arrays as float32 / float64 .npy, whole when they fit their
  share of the 64 MB limit and as a fixed, seeded row sample (rows numbered beside it) when not.
* --full is an option of every run (rehearsed with --dry-run, no GPU).
* On the GPU: a plain run prints the headline line only, and two runs with equal arguments dump
  identical outputs (seeded inputs).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, "bench.py")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("roofline", "rank_roofline", "parity_mode", "verify", "kernels", "cpu_baseline")


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f), allow_pickle=False) for f in sorted(os.listdir(d))}


def test_dump_outputs_whole_and_sampled(tmp_path):
    import torch
    import bench
    g = torch.Generator().manual_seed(0)
    emb, txt = torch.randn(300, 512, generator=g), torch.randn(8, 512, generator=g)
    s, i = torch.randn(8, 10, generator=g), torch.randint(0, 1 << 40, (8, 10), generator=g)
    bench.dump_outputs(str(tmp_path / "a"), emb, txt, s, i)
    a = _load(tmp_path / "a")
    assert sorted(a) == ["image_embeddings", "text_embeddings", "topk_indices", "topk_scores"]
    assert a["image_embeddings"].dtype == np.float32 and np.array_equal(a["image_embeddings"], emb.numpy())
    assert a["topk_indices"].dtype == np.float64 and np.array_equal(a["topk_indices"].astype(np.int64), i.numpy())
    assert np.array_equal(a["topk_scores"], s.numpy()) and np.array_equal(a["text_embeddings"], txt.numpy())
    # 40 000 x 512 f32 = 82 MB: above the limit, so a fixed sample of rows, the same on every call
    big = torch.arange(40_000, dtype=torch.float32)[:, None].expand(40_000, 512)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), big, txt, s, i)
    b, c = _load(tmp_path / "b"), _load(tmp_path / "c")
    rows = b["image_embeddings_rows"]
    assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0) and rows[-1] < 40_000
    assert np.array_equal(b["image_embeddings"][:, 0], rows.astype(np.float32))      # row r holds r
    assert all(np.array_equal(b[k], c[k]) for k in b)
    total = sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b"))
    assert total <= 64_000_000 and b["image_embeddings"].shape[0] > 10_000


def test_full_is_an_option():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--dry-run"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([sys.executable, BENCH, "--steps", "0", "--dry-run"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr


def _bench(args):
    env = dict(os.environ)
    for v in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(v, None)
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--model", "test-tiny", "--frames", "300",
                        "--queries", "4", "--steps", "2", "--warmup", "1"] + args,
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return lines[0]


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_are_reproducible(gpu, tmp_path):
    a = _bench(["--dump-outputs", str(tmp_path / "a")])
    b = _bench(["--dump-outputs", str(tmp_path / "b")])
    for key in HEADLINE:
        assert key in a
    assert a["steps"] == 2 and a["ms_per_step"] > 0 and not any(k in a for k in FULL_ONLY)
    # value = frames / step time (ms_per_step is rounded to 1 us: 1 % of a step of 0.05 ms or more)
    assert abs(a["value"] - 300 / (a["ms_per_step"] / 1e3)) <= 2e-2 * a["value"]
    da, db = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert da["image_embeddings"].shape[0] == 300 and da["topk_indices"].shape == (4, 10)
    for k in da:
        assert da[k].dtype in (np.float32, np.float64) and np.isfinite(da[k]).all()
        assert np.array_equal(da[k], db[k]), k
    # the dumped ranking belongs to the dumped embeddings: the top-1 score is that row's cosine and no
    # row beats it (1e-4: f32 arithmetic over a few hundred terms of magnitude <= 1 stays below 1e-5)
    e, t = da["image_embeddings"].astype(np.float64), da["text_embeddings"].astype(np.float64)
    cos = (t / np.linalg.norm(t, axis=1, keepdims=True)) @ (e / np.linalg.norm(e, axis=1, keepdims=True)).T
    q = np.arange(4)
    top = cos[q, da["topk_indices"][:, 0].astype(np.int64)]
    assert np.abs(top - da["topk_scores"][:, 0]).max() < 1e-4 and (cos.max(1) - top).max() < 1e-4
