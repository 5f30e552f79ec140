"""The S <= 64 attention (attention.hip attention_s64_kernel): every shape of the A/B build
(MICLIP_ATTN_SHORT = 100 + shape; bit 0: 2 waves x 2 tiles, bit 1: K fragments from global memory, bit 2:
V row-major in LDS and read transposed, + 8 x the output store form: 1 16-byte stores, 3 whole lines through
LDS, 4 / 5 the same nontemporal) and the product default against the flash body's single-chunk instance
(MICLIP_ATTN_SHORT=30), bit for bit; the default against float64; and the last vision block's CLS-row
form, whose attention writes row 0 of every sequence into compact rows."""
import numpy as np
import pytest

from conftest import state_dict

pytestmark = pytest.mark.gpu

BASELINE = "30"                              # attention_flash_kernel<1, 2, 1>
# attention_s64_kernel's shapes (the whole-line stores take the K image's LDS: shapes without bit 1)
SHAPES = [str(100 + i) for i in list(range(16)) + [24, 25, 28, 29] + list(range(32, 34)) + [36, 37, 40, 41, 44, 45]]


def _native():
    from miclip import _native
    return _native


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _run(lib, qkv, B, S, W, causal):
    """One launch into a NaN-filled output: a row left unwritten fails every comparison."""
    import torch
    out = torch.full((B * S, W), float("nan"), dtype=torch.bfloat16, device=qkv.device)
    assert lib.mi_op_attention(qkv.data_ptr(), out.data_ptr(), B, S, W, causal, _stream()) == 0, lib.mi_last_error()
    torch.cuda.synchronize()
    assert not torch.isnan(out).any()
    return out


def _ref64(qkv, B, S, W, causal):
    import torch
    x = qkv.double().reshape(B, S, 3, W // 64, 64)
    q, k, v = (x[:, :, i].transpose(1, 2) for i in range(3))
    s = q @ k.transpose(-1, -2) * 0.125
    if causal:
        s = s.masked_fill(torch.triu(torch.ones(S, S, dtype=torch.bool, device=qkv.device), 1), float("-inf"))
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B * S, W)


def _all_equal_baseline(monkeypatch, qkv, B, S, W, causal, what):
    import torch
    N_ = _native()
    La = N_.lib_ab()
    monkeypatch.setenv("MICLIP_ATTN_SHORT", BASELINE)
    base = _run(La, qkv, B, S, W, causal)
    for v in SHAPES:
        monkeypatch.setenv("MICLIP_ATTN_SHORT", v)
        assert torch.equal(_run(La, qkv, B, S, W, causal), base), f"MICLIP_ATTN_SHORT={v} differs: {what}"
    monkeypatch.delenv("MICLIP_ATTN_SHORT")
    assert torch.equal(_run(La, qkv, B, S, W, causal), base), f"the A/B build's default differs: {what}"
    assert torch.equal(_run(N_.lib(), qkv, B, S, W, causal), base), f"the product default differs: {what}"
    return base


@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("S", [2, 15, 16, 17, 32, 33, 49, 50, 63, 64])
def test_s64_shapes_bit_identical(gpu, monkeypatch, S, causal):
    """S: one key, a partial and a whole single tile, one row into the second, the 32-key boundary of the
    P V k-steps on both sides, the product's 50 and its neighbour, a last tile short of one key, all 64
    keys; W = 128 / 768 (2 / 12 heads); B = 1, 3, 37 sequences (odd item counts)."""
    import torch
    for W in (128, 768):
        for B in (1, 3, 37):
            g = torch.Generator(device="cpu").manual_seed(1000 * S + W + 7 * B + causal)
            qkv = (torch.randn(B * S, 3 * W, generator=g) * 1.5).bfloat16().to(gpu)
            _all_equal_baseline(monkeypatch, qkv, B, S, W, causal, f"S={S} W={W} B={B} causal={causal}")


@pytest.mark.parametrize("S", [50, 64])
def test_s64_growing_max(gpu, monkeypatch, S):
    """Scores whose row max grows along the keys by far more than the lazy-rescale threshold (2^8 in the
    log2 domain): the running max is set from the chunk's and P spans its whole range.  Every shape
    equals the baseline bit for bit, and the result is within test_attention_growing_max's bound."""
    import torch
    B, W = 3, 256
    g = torch.Generator(device="cpu").manual_seed(S)
    qkv = torch.randn(B, S, 3, W // 64, 64, generator=g)
    qkv[:, :, 0] = qkv[:, :, 0].abs() * 0.5 + 0.5                                        # q > 0
    qkv[:, :, 1] = qkv[:, :, 1].abs() * torch.linspace(0.05, 4.0, S).reshape(1, S, 1, 1)   # k grows with the key
    qkv = qkv.reshape(B * S, 3 * W).bfloat16().to(gpu)
    out = _all_equal_baseline(monkeypatch, qkv, B, S, W, 0, f"growing max S={S}")
    err = (out.double() - _ref64(qkv, B, S, W, 0)).abs().max().item()
    print(f"growing max S={S}: max err {err}")
    assert err < 3e-2, err


@pytest.mark.parametrize("B,S,W,causal", [(3, 50, 768, 0), (3, 17, 128, 1)])
def test_s64_default_against_float64(gpu, B, S, W, causal):
    """The product default against the float64 softmax, at tests/test_gpu_ops.py::test_attention's bound."""
    import torch
    g = torch.Generator(device="cpu").manual_seed(B * S + W + causal)
    qkv = (torch.randn(B * S, 3 * W, generator=g) * 1.5).bfloat16().to(gpu)
    out = _run(_native().lib(), qkv, B, S, W, causal)
    ref = _ref64(qkv, B, S, W, causal)
    err = (out.double() - ref).abs().max().item()
    print(f"S={S} W={W} causal={causal}: max err {err}")
    assert err < 3e-2 * max(1.0, ref.abs().max().item()), err


@pytest.mark.parametrize("name,n", [("test-small", 300), ("test-small", 257), ("ViT-B/32", 257)])
def test_cls_rows_written_by_attention(gpu, monkeypatch, name, n):
    """The folded bf16 tower's last block at >= 256 frames: its attention computes the CLS query of every
    sequence alone and writes it into compact rows (the default).  The embeddings equal, bit for bit,
    those of the full last block (A/B build, MICLIP_CLS_LAST=0), of the first 16-query tile written in
    place and gathered (MICLIP_CLS_ATT=0), and of every workgroup shape of the CLS form.  n = 257: the
    last sequence alone past the 256-row tile.  test-small: W = 256, S = 10; ViT-B/32: W = 768, S = 50."""
    import torch
    from miclip import _native, config, model as M, weights
    cfg = config.get_config(name)
    px = torch.from_numpy(weights.synthetic_pixels(n, cfg.image_resolution, seed=n)).to(gpu).bfloat16()

    def encode():
        m = M.CLIP(cfg, state_dict(name), device=gpu, image_chunk=n)
        return m.encode_image(px).cpu().numpy().view(np.int32)

    got = encode()
    monkeypatch.setattr(_native, "lib", _native.lib_ab)
    assert np.array_equal(encode(), got), "A/B build, defaults"
    monkeypatch.setenv("MICLIP_CLS_ATT", "0")
    assert np.array_equal(encode(), got), "MICLIP_CLS_ATT=0: tile 0 in place, CLS rows gathered"
    monkeypatch.delenv("MICLIP_CLS_ATT")
    monkeypatch.setenv("MICLIP_CLS_LAST", "0")
    assert np.array_equal(encode(), got), "MICLIP_CLS_LAST=0: the full last block"
    monkeypatch.delenv("MICLIP_CLS_LAST")
    for v in SHAPES[:8] if name == "test-small" else ():   # (every shape's CLS form: on the small tower)
        monkeypatch.setenv("MICLIP_ATTN_SHORT", v)
        assert np.array_equal(encode(), got), f"MICLIP_ATTN_SHORT={v}"
