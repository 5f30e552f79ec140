"""The A/B switches of the encoder orchestration (internal.hpp ab_env_int) that no other test sets, one
at a time through the A/B library and all inside this one process: the library reads a switch on
every call (MICLIP_F32_SPLIT when a context is created), so each case runs the tower code behind
its switch although earlier cases and tests already ran the library with the defaults.

test-small (3 layers, width 256, 10 vision tokens; W % 256 == 0, so the folded, MX and 8-phase
paths apply) at 300 frames (3000 rows: the CLS-row last block, and 2700 >= 1024 patch rows for the
fused patch gather) and at 8 frames (80 rows: the small-shape fallbacks), plus 32 text rows where
the switch reaches the text tower.  Outputs are finite and within the tower's float64 tolerance of
oracle.clip_ref: COS_TOL for bf16, 1 - cos <= 1e-9 and relative error < 2e-5 for fp32.

Left out: the MX-fp8 tower with MICLIP_RESID16=0.  With these inputs it misses FP8_COS = 1e-3
(1 - cos 1.24e-3 at 300 frames, 1.05e-3 at 8), and so does the MX tower with no switch set
(1.15e-3, 1.06e-3), both measured at the commit before this file: test-small's three random
layers sit at that bound, whichever way the switch is set."""
import functools

import numpy as np
import pytest

from conftest import state_dict

pytestmark = pytest.mark.gpu

NAME = "test-small"
COS_TOL = 1e-3                  # bf16 towers (tests/test_gpu_encode.py)
F32_COS, F32_REL = 1e-9, 2e-5   # fp32 tower (tests/test_gpu_rk_flow.py)
FRAMES = (300, 8)


@functools.lru_cache(maxsize=1)
def _inputs():
    """Pixels, tokens and their float64 references, computed once: bf16 / fp8 towers read the
    pixels as bf16 (the fused patch gather needs them), so their reference reads the rounded ones."""
    import torch
    from miclip import config, weights
    from oracle import clip_ref
    cfg, sd = config.get_config(NAME), state_dict(NAME)
    d = {"cfg": cfg}
    for n in FRAMES:
        px = torch.from_numpy(weights.synthetic_pixels(n, cfg.image_resolution, seed=n))
        d["px", "fp32", n] = px
        d["px", "bf16", n] = px.bfloat16()
        d["ref", "fp32", n] = clip_ref.encode_image(px.numpy(), sd, cfg, np.float64)
        d["ref", "bf16", n] = clip_ref.encode_image(px.bfloat16().float().numpy(), sd, cfg, np.float64)
    tk = weights.synthetic_tokens(32, cfg.context_length, cfg.vocab_size, seed=32)
    d["tk"] = torch.from_numpy(tk)
    d["ref_txt"] = clip_ref.encode_text(tk, sd, cfg, np.float64)
    return d


def _encode(gpu, monkeypatch, wts, env, text):
    """{300: image rows, 8: image rows, "txt": text rows or None} of the A/B library under env."""
    from miclip import _native, model as M
    d = _inputs()
    monkeypatch.setattr(_native, "lib", _native.lib_ab)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = M.CLIP(d["cfg"], state_dict(NAME), device=gpu, weights=wts, image_chunk=max(FRAMES), text_chunk=32)
    out = {n: m.encode_image(d["px", wts, n].to(gpu)).cpu().numpy() for n in FRAMES}
    out["txt"] = m.encode_text(d["tk"]).cpu().numpy() if text else None
    del m
    monkeypatch.undo()
    return out


def _within(got, ref, wts, what):
    from oracle.clip_ref import cosine
    assert np.isfinite(got).all(), what
    dcos = 1 - cosine(got, ref).min()
    rel = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{what}: 1-cos {dcos:.3e}, max rel err {rel:.3e}")
    if wts == "fp32":
        assert dcos <= F32_COS and rel < F32_REL, (what, dcos, rel)
    else:
        assert dcos < COS_TOL, (what, dcos)


def _check(out, wts, what):
    d = _inputs()
    for n in FRAMES:
        _within(out[n], d["ref", wts, n], wts, f"{what}, {n} frames")
    if out["txt"] is not None:
        _within(out["txt"], d["ref_txt"], wts, f"{what}, text")


# (weights, switches, reaches the text tower, frames at which the result must differ from the
# defaults' -- the switch changes the arithmetic there, so an equal result would mean it was not read)
BF16 = [
    ({"MICLIP_RESID16": "0"}, False, 8),           # 300 frames run the folded tower, fp16 stream either way
    ({"MICLIP_PATCH_FUSED": "0"}, False, None),    # im2col + plain GEMM: the same products
    ({"MICLIP_EMBED_LN1": "0", "MICLIP_LNFOLD": "0"}, False, None),
    ({"MICLIP_GEMM_VARIANT": "98"}, True, 300),    # also turns the fused residual add off
]


@pytest.mark.parametrize("env,text,differs", BF16, ids=lambda v: "+".join(f"{k[7:]}={x}" for k, x in v.items())
                         if isinstance(v, dict) else None)
def test_bf16_tower_switches(gpu, monkeypatch, env, text, differs):
    out = _encode(gpu, monkeypatch, "bf16", env, text)
    _check(out, "bf16", f"bf16 {env}")
    if differs:
        base = _encode(gpu, monkeypatch, "bf16", {}, False)
        assert not np.array_equal(out[differs], base[differs]), f"{env} was not read at this call"


@pytest.mark.parametrize("which", ["QKV", "OUT", "FC", "PROJ"])
def test_bf16_per_gemm_schedule_bit_identical(gpu, monkeypatch, which):
    """The unfolded tower (MICLIP_LNFOLD=0) with one GEMM on schedule 98: within tolerance and
    bit-identical to MICLIP_LNFOLD=0 alone (v98 == v110 for K >= 256,
    test_gemm_8phase_schedules_bit_identical), image and text."""
    plain = _encode(gpu, monkeypatch, "bf16", {"MICLIP_LNFOLD": "0"}, True)
    out = _encode(gpu, monkeypatch, "bf16", {"MICLIP_LNFOLD": "0", f"MICLIP_GEMM_VARIANT_{which}": "98"}, True)
    _check(out, "bf16", f"bf16 LNFOLD=0 GEMM_VARIANT_{which}=98")
    for k in (*FRAMES, "txt"):
        assert np.array_equal(out[k].view(np.int32), plain[k].view(np.int32)), k


@pytest.mark.parametrize("env,text", [({"MICLIP_F32_ATTN_FUSED": "0"}, False),   # 300 frames: the plain-attention CLS gather
                                      ({"MICLIP_F32_FUSED_SPLIT": "0"}, True),
                                      ({"MICLIP_F32_SPLIT": "0"}, True),
                                      ({"MICLIP_F32_SPLIT": "6"}, True)],
                         ids=lambda v: "+".join(f"{k[7:]}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_fp32_tower_switches(gpu, monkeypatch, env, text):
    """MICLIP_F32_SPLIT=6 (the split-bf16 tower) meets the fp32 tolerance as the others do: with
    these inputs, before the orchestration refactor, 1 - cos 3.5e-13 / 2.6e-13 / 9.2e-13 and
    relative error 9.7e-7 / 8.1e-7 / 1.0e-6 (300 frames / 8 frames / text)."""
    _check(_encode(gpu, monkeypatch, "fp32", env, text), "fp32", f"fp32 {env}")
