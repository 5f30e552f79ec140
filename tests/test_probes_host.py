"""The exact-result probes (tests/probes.py) are right and have teeth, shown without a GPU:
each builder's closed-form expectation equals a plain int64 / float64 reference at small shapes,
and subtly wrong references -- one k dropped, two k of one operand swapped, one key dropped, one
zero-score padded key added, the next sequence's first row let in, the causal mask shifted by
one -- are rejected by the very comparison functions test_gpu_exact.py applies to the kernels."""
import numpy as np
import pytest

import probes

GEMM_SHAPES = [(1, 64, 64), (37, 128, 192), (200, 256, 256), (70, 96, 768), (33, 64, 1088), (300, 40, 128)]


def _gemm_ref(p, drop_k=None, swap_k=None):
    """Plain float64 A W^T + bias (every value an integer or a small dyadic: exact), with the
    mutations: column drop_k of A left out; columns swap_k of A exchanged (W untouched)."""
    A = p.A.astype(np.float64)
    if drop_k is not None:
        A[:, drop_k] = 0
    if swap_k is not None:
        A[:, list(swap_k)] = A[:, list(swap_k)[::-1]]
    return A @ p.W.astype(np.float64).T + p.bias.astype(np.float64)


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("unit", [False, True])
def test_hadamard_closed_form(M, N, K, unit):
    p = probes.hadamard_operands(M, N, K, seed=K + M, unit=unit)
    assert p.A.shape == (M, K) and p.W.shape == (N, K)
    if not unit:       # the int64 product, no floating point at all
        ref = p.A.astype(np.int64) @ p.W.astype(np.int64).T + p.bias.astype(np.int64)
        assert np.array_equal(ref, p.expected.astype(np.int64))
    probes.assert_equal(_gemm_ref(p), p.expected)
    # dense +-{1,2,3} operands, exact in bf16 (and so in fp16 / f32), e4m3-exact magnitudes
    scale = 2.0 ** p.p if unit else 1.0
    assert set(np.unique(np.abs(p.A * scale))) <= {1.0, 2.0, 3.0} and set(np.unique(np.abs(p.W))) <= {1.0, 2.0, 3.0}
    probes.bf16_bits(p.A), probes.bf16_bits(p.W), probes.bf16_bits(p.expected)
    assert np.array_equal(p.expected.astype(np.float16).astype(np.float32), p.expected)
    # nearly everywhere the bias; matches in every row and column, at least 2^p off it
    assert p.match.any(axis=1).all() and p.match.any(axis=0).all()
    assert (p.core[~p.match] == 0).all() and (np.abs(p.core[p.match]) >= (1 if unit else p.P)).all()
    if M >= 32 and N >= 64:
        assert p.match.mean() < 0.1
    # the index maps differ per block
    r, c = probes.hadamard_maps(M, N, p.b, p.P)
    if M > 8:
        assert len({tuple(x) for x in r}) == len(r) and len({tuple(x) for x in c}) == len(c)


@pytest.mark.parametrize("M,N,K", [(37, 128, 192), (200, 256, 256), (70, 96, 768)])
def test_hadamard_rejects_wrong_k(M, N, K):
    """One dropped k, one dropped aligned 8-vector and two swapped k of one operand, each rounded to
    bf16 as a kernel's output would be, all fail the equality the GPU tests assert."""
    p = probes.hadamard_operands(M, N, K, seed=1)
    out = lambda x: probes.bf16_rne(x)
    probes.assert_equal(out(_gemm_ref(p)), p.expected)
    for k in (0, 5, K // 2 + 3, K - 1):
        with pytest.raises(AssertionError):
            probes.assert_equal(out(_gemm_ref(p, drop_k=k)), p.expected)
    with pytest.raises(AssertionError):
        probes.assert_equal(out(_gemm_ref(p, drop_k=slice(K - 8, K))), p.expected)
    for pair in ((0, 1), (6, 7), (3, K - 1), (31, 32)):
        with pytest.raises(AssertionError):
            probes.assert_equal(out(_gemm_ref(p, swap_k=pair)), p.expected)


@pytest.mark.parametrize("M,N,K", [(37, 128, 192), (200, 256, 256)])
def test_quickgelu_probe_rejects_wrong_k(M, N, K):
    """The QuickGELU form (unit scale, |x| <= 32): the float64 QuickGELU of the exact x passes the
    one-ulp comparison with exact zeros; with one k dropped or two swapped the x = 0 entries are
    no longer 0 and it fails."""
    p = probes.hadamard_operands(M, N, K, seed=2, unit=True)
    assert np.abs(p.expected).max() <= 32 and (p.expected == 0).mean() > 0.3
    gelu = lambda x: probes.bf16_rne(probes.quickgelu64(x))
    want = probes.quickgelu64(p.expected)
    zero = p.expected == 0
    probes.assert_bf16_ulps(gelu(_gemm_ref(p)), want, 1, exact=zero)
    with pytest.raises(AssertionError):
        probes.assert_bf16_ulps(gelu(_gemm_ref(p, drop_k=K - 1)), want, 1, exact=zero)
    with pytest.raises(AssertionError):
        probes.assert_bf16_ulps(gelu(_gemm_ref(p, swap_k=(2, 3))), want, 1, exact=zero)


def test_ulp_comparisons():
    one = np.float32(1.0)
    up = probes.bf16_from_bits(np.array([0x3F81], np.uint16))            # 1 + 2^-7
    up2 = probes.bf16_from_bits(np.array([0x3F82], np.uint16))
    probes.assert_bf16_ulps(up, np.array([1.0]), 1)
    with pytest.raises(AssertionError):
        probes.assert_bf16_ulps(up2, np.array([1.0]), 1)
    with pytest.raises(AssertionError):
        probes.assert_bf16_ulps(up, np.array([1.0]), 1, exact=np.array([True]))
    probes.assert_bf16_ulps(np.array([-0.0], np.float32), np.array([0.0]), 0)
    with pytest.raises(AssertionError):
        probes.assert_bf16_ulps(np.array([np.nan], np.float32), np.array([0.0]), 1)
    probes.assert_f32_ulps(np.nextafter(one, np.float32(2)), np.array([1.0]), 2)
    with pytest.raises(AssertionError):
        probes.assert_f32_ulps(np.float32(1.0 + 3 * 2.0 ** -23), np.array([1.0]), 2)
    # bf16_rne rounds ties to even, straight from float64
    assert probes.bf16_rne(1 + 2.0 ** -8) == 1.0 and probes.bf16_rne(1 + 3 * 2.0 ** -8) == 1 + 2.0 ** -6
    assert probes.bf16_rne(1 + 2.0 ** -8 + 2.0 ** -40) == 1 + 2.0 ** -7
    assert list(probes.significant_bits(np.array([0, 1, 3, 255, 256, 257, 96.0, 0.375]))) == [0, 1, 2, 8, 1, 9, 2, 2]


def _attn_ref(p, drop_key=None, pad_key=False, leak_next=False, shift=0):
    """float64 softmax(q k^T / 8 (+ causal mask)) v per (sequence, head) on the probe's packed rows,
    with the mutations: key drop_key left out; one padded key (k = 0, v = 0: score 0) added; the
    next sequence's first row let in as a key; the causal mask moved by `shift` keys."""
    B, S, H = p.B, p.S, p.H
    W = 64 * H
    x = p.qkv.astype(np.float64).reshape(B, S, 3, H, 64)
    q, k, v = x[:, :, 0], x[:, :, 1], x[:, :, 2]
    if pad_key or leak_next:
        if leak_next:
            ek, ev = np.roll(k, -1, axis=0)[:, :1], np.roll(v, -1, axis=0)[:, :1]
        else:
            ek, ev = np.zeros((B, 1, H, 64)), np.zeros((B, 1, H, 64))
        k, v = np.concatenate([k, ek], 1), np.concatenate([v, ev], 1)
    s = np.einsum("bqhd,bkhd->bhqk", q, k) / 8.0
    if p.causal:      # (an added key S is not masked: that is the defect it stands for)
        masked = np.arange(S)[None, :] > np.arange(S)[:, None] + shift
        s[..., :S] = np.where(masked, -np.inf, s[..., :S])
    if drop_key is not None:
        s[..., drop_key] = -np.inf
    with np.errstate(invalid="ignore"):
        e = np.exp(s - s.max(-1, keepdims=True))
    e = np.nan_to_num(e)                          # (a row whose every key is masked: weights 0)
    den = e.sum(-1, keepdims=True)
    pr = e / np.where(den == 0, 1, den)
    return np.einsum("bhqk,bkhd->bqhd", pr, v).reshape(B * S, W)


ATTN_SHAPES = [(2, 1, 2, 0), (2, 17, 2, 0), (2, 50, 2, 0), (2, 10, 2, 1), (3, 77, 2, 1), (4, 97, 2, 0)]


@pytest.mark.parametrize("B,S,H,causal", ATTN_SHAPES)
def test_attention_impulse_closed_form(B, S, H, causal):
    p = probes.attention_impulse(B, S, H, causal, seed=S)
    probes.bf16_bits(p.qkv)
    ref = _attn_ref(p)
    assert np.abs(ref - p.expected).max() < 1e-15
    assert np.array_equal(np.unique(p.keys), np.arange(S))       # every key position is hit
    assert (p.qkv[:, :64 * H] == 0).all() and (p.qkv[:, 64 * H:128 * H] != 0).any()
    for f32, rnd in ((False, probes.bf16_rne), (True, lambda a: a.astype(np.float32))):
        probes.check_impulse(rnd(ref), p, f32=f32)
        muts = [dict(drop_key=0), dict(drop_key=S - 1), dict(leak_next=True)]
        if S <= 64 or f32:     # 1 / (n + 1) of the value: above one bf16 ulp (2^-8 .. 2^-7) for short rows only
            muts.append(dict(pad_key=True))
        if causal:
            muts += [dict(shift=1), dict(shift=-1)]
        for m in muts:
            if S == 1 and ("drop_key" in m):
                continue      # (nothing left to attend to)
            with pytest.raises(AssertionError):
                probes.check_impulse(rnd(_attn_ref(p, **m)), p, f32=f32)


@pytest.mark.parametrize("B,S,H,causal", ATTN_SHAPES + [(2, 257, 1, 0), (2, 130, 1, 1)])
def test_attention_select_closed_form(B, S, H, causal):
    p = probes.attention_select(B, S, H, causal, seed=1)
    probes.bf16_bits(p.qkv)
    ref = _attn_ref(p)
    assert np.abs(ref - p.expected).max() < 1e-7                 # S e^-24 max|v|
    t = p.targets
    need = {0, S - 1} | {c + o for c in range(16, S, 16) for o in (-1, 0)}
    for b in range(B):
        for h in range(H):
            assert need <= set(t[b, h].tolist())
            if causal:
                assert (t[b, h] <= np.arange(S)).all() and t[b, h, S - 1] == S - 1
                assert S < 8 or 0.25 < (t[b, h] == np.arange(S)).mean() < 0.85
    for f32, rnd in ((False, probes.bf16_rne), (True, lambda a: a.astype(np.float32))):
        probes.check_select(rnd(ref), p, f32=f32)
        if S == 1:
            continue
        muts = [dict(drop_key=0), dict(drop_key=S - 1), dict(drop_key=min(16, S - 1))]
        if causal:
            muts.append(dict(shift=-1))                          # the diagonal targets are masked
        for m in muts:
            with pytest.raises(AssertionError):
                probes.check_select(rnd(_attn_ref(p, **m)), p, f32=f32)


@pytest.mark.parametrize("S", [97, 257, 577, 640])
def test_attention_select_margin(S):
    """At the GPU tests' lengths and seeds the random keys meet the margin as drawn: the largest
    off-target dot product is <= 36 (a logit margin >= 28) and no head is drawn again."""
    for seed in (0, 1, 2):
        p = probes.attention_select(2, S, 1, 0, seed=seed)
        assert p.redraws == 0 and p.max_off <= 36, (seed, p.redraws, p.max_off)
