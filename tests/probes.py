"""Exact-result probes: inputs whose correct GEMM / attention output is known in closed form
and is exactly representable in the output type, so that equality (or one or two output ulps)
is the assertion and a single misplaced element fails it.  Pure numpy on the CPU; the GPU tests
(test_gpu_exact.py) and the host tests (test_probes_host.py) share the builders and the
comparison functions below.

Builders
  hadamard_operands   dense +-1 GEMM operands from Sylvester-Hadamard rows
  attention_impulse   q = 0 (uniform weights), one non-zero V entry per output column
  attention_select    q_i = 8 k_t(i) with +-1 keys: the softmax selects key t(i)

Comparisons (raise AssertionError with the first offending entries)
  assert_equal, assert_bf16_ulps, assert_f32_ulps, check_impulse, check_select
"""
from types import SimpleNamespace

import numpy as np


# ------------------------------------------------------------------ number formats
def bf16_rne(x):
    """float64 -> the nearest bf16 value (round to nearest even, straight from float64: no
    double rounding through f32), returned as float64.  Normal range only."""
    x = np.asarray(x, np.float64)
    m, e = np.frexp(x)                       # x = m 2^e, |m| in [0.5, 1): 8 significant bits = m 2^8
    return np.ldexp(np.rint(m * 256.0), e - 8)


def bf16_bits(x):
    """bf16-exact values -> their bit patterns (uint16)."""
    f = np.ascontiguousarray(np.asarray(x, np.float32))
    u = f.view(np.uint32)
    assert not (u & 0xFFFF).any(), "value is not exact in bf16"
    return (u >> 16).astype(np.uint16)


def bf16_from_bits(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def _ordinal(bits, width):
    """Sign-magnitude bit patterns -> integers in value order (+0 and -0 both 0)."""
    s = np.asarray(bits).astype(np.int64)
    sign = 1 << (width - 1)
    mag = s & (sign - 1)
    return np.where(s & sign, -mag, mag)


def significant_bits(v):
    """Bits between the highest and lowest set bit of |v| (integers, or integer multiples of a
    power of two); 0 for 0."""
    v = np.abs(np.asarray(v, np.float64))
    m, _ = np.frexp(v)                       # m in [0.5, 1)
    bits = np.zeros(v.shape, np.int64)
    for n in range(1, 54):
        todo = (bits == 0) & (v != 0)
        if not todo.any():
            break
        f = m * 2.0 ** n
        bits = np.where(todo & (f == np.floor(f)), n, bits)
    return bits


def _first(mask, *arrays):
    idx = np.argwhere(mask)[:5]
    return [(tuple(int(t) for t in i), *(a[tuple(i)] for a in arrays)) for i in idx]


# ------------------------------------------------------------------ comparisons
def assert_equal(got, want, what="output"):
    """Exact equality of values (bf16 / fp16 / f32 outputs widened exactly to float)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    bad = ~(got == want)                     # (a NaN fails)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first (index, got, want): " \
                          f"{_first(bad, got, want)}"


def assert_bf16_ulps(got, want64, max_ulps, exact=None, what="output"):
    """got: bf16 values (any float array holding them exactly); want64: the float64 result.
    |ordinal(got) - ordinal(bf16_rne(want64))| <= max_ulps everywhere, and 0 where `exact`."""
    got = np.asarray(got, np.float32)
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    w = bf16_rne(want64)
    d = np.abs(_ordinal(bf16_bits(got), 16) - _ordinal(bf16_bits(w), 16))
    bad = d > max_ulps
    if exact is not None:
        bad |= np.asarray(exact) & (d != 0)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} beyond {max_ulps} bf16 ulp(s), first " \
                          f"(index, got, want, ulps): {_first(bad, got, w, d)}"


def assert_f32_ulps(got, want64, max_ulps, what="output"):
    got = np.ascontiguousarray(np.asarray(got, np.float32))
    assert np.isfinite(got).all(), f"{what}: non-finite values"
    w = np.ascontiguousarray(np.asarray(want64, np.float64).astype(np.float32))
    d = np.abs(_ordinal(got.view(np.uint32), 32) - _ordinal(w.view(np.uint32), 32))
    bad = d > max_ulps
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} beyond {max_ulps} f32 ulp(s), first " \
                          f"(index, got, want, ulps): {_first(bad, got, w, d)}"


F32_ATTN_TOL = 2e-6          # test_attention_f32_vs_float64's: 2e-6 * max(1, |ref|.max())


def check_impulse(got, p, f32=False):
    """The impulse probe's assertions on an output [B*S, W]: exactly 0 where the column's key is
    not visible to the row; elsewhere at most one bf16 ulp from bf16_rne(val / n_i) (bf16
    outputs), or the f32 attention tolerance (f32 outputs)."""
    got = np.asarray(got, np.float64)
    assert got.shape == p.expected.shape, (got.shape, p.expected.shape)
    hidden = ~p.visible
    leak = hidden & ~(got == 0)
    assert not leak.any(), f"impulse: {int(leak.sum())} non-zero outputs where the key is not visible, first " \
                           f"(index, got): {_first(leak, got)}"
    if f32:
        tol = F32_ATTN_TOL * max(1.0, np.abs(p.expected).max())
        bad = ~(np.abs(got - p.expected) <= tol)
        assert not bad.any(), f"impulse: {int(bad.sum())} beyond {tol}, first (index, got, want): " \
                              f"{_first(bad, got, p.expected)}"
    else:
        assert_bf16_ulps(got, p.expected, 1, what="impulse")


def check_select(got, p, f32=False):
    """The select probe's assertion: out[i] = v[t(i)], within two bf16 ulps (bf16 outputs: one
    rounding of P, one of the output) or the f32 attention tolerance."""
    got = np.asarray(got, np.float64)
    assert got.shape == p.expected.shape, (got.shape, p.expected.shape)
    if f32:
        tol = F32_ATTN_TOL * max(1.0, np.abs(p.expected).max())
        bad = ~(np.abs(got - p.expected) <= tol)
        assert not bad.any(), f"select: {int(bad.sum())} beyond {tol}, first (index, got, want): " \
                              f"{_first(bad, got, p.expected)}"
    else:
        assert_bf16_ulps(got, p.expected, 2, what="select")


# ------------------------------------------------------------------ GEMM probe
def hadamard(P):
    """Sylvester-Hadamard matrix H_P (P a power of two) as int8: H[r][k] = (-1)^popcount(r & k)."""
    assert P >= 1 and P & (P - 1) == 0
    H = np.ones((1, 1), np.int8)
    while H.shape[0] < P:
        H = np.block([[H, H], [H, -H]])
    return H


def _coprime_mul(Q):
    for c in (5, 7, 11, 13, 17, 19):
        if np.gcd(c, Q) == 1:
            return c
    raise AssertionError(Q)


MATCH_BLOCKS = 3   # blocks whose index maps may coincide; later blocks (K = b 2^p, b > 3) never match


def hadamard_maps(M, N, b, P):
    """Row-index maps r_j(m), c_j(n) into H_P for the blocks j < b; they differ per block.
    Block 0 is built so that every output row and every output column has a match:
    r_0(m) = m mod Q, c_0(n) = (u (n mod Q) + 1) mod Q with Q = min(P, M, N) and u coprime to Q, a
    bijection of [0, Q), Q <= M, N.  Blocks 1, 2 are affine maps mod P (matches at density 1 / P).
    Blocks >= 3 take even rows for A and odd rows for W: they never match, so the count of
    matching blocks stays <= 3 whatever b."""
    m, n = np.arange(M, dtype=np.int64), np.arange(N, dtype=np.int64)
    Q = min(P, M, N)
    r, c = [m % Q], [(_coprime_mul(Q) * (n % Q) + 1) % Q]
    for j in range(1, b):
        if j < MATCH_BLOCKS:
            r.append((m * (2 * j + 1) + 7 * j) % P)
            c.append((n * (2 * j + 3) + 11 * j + 5) % P)
        else:
            assert P >= 2
            r.append(2 * ((m + j) % (P // 2)))
            c.append(2 * ((3 * n + j) % (P // 2)) + 1)
    return r, c


def hadamard_operands(M, N, K, seed=0, unit=False, bias=True, shift=0):
    """Dense +-1 operands with a closed-form product.  K = b 2^p (p = the number of trailing zero
    bits of K; b in {1, 3} for the towers' K, any b <= 32 accepted).  Row m of A is the
    concatenation of H_{2^p}[r_j(m)], j < b, times a_m 2^-shift; row n of W that of H[c_j(n)] times
    w_n; a_m, w_n in {1, 2, 3}.  Orthogonality of Hadamard rows gives

        out[m, n] = bias_n + a_m w_n 2^(p - shift) #{j : r_j(m) = c_j(n)}

    which is bias_n nearly everywhere.  Every operand value is exact in bf16, fp16, f32 and (scaled
    by a power of two per block) e4m3; every partial sum is an integer multiple of 2^-shift below
    2^24 of them, exact in f32 in any order.  The bias is a multiple of g = max(1, 2^(p - shift) / 8)
    with |bias_n| <= min(2 g, 128) and < 2^(8 - shift), so that every expected value has at most 8 significant bits
    (asserted: exact in bf16 and fp16) and an unmatched entry moved by one k (+- a_m w_n 2^-shift)
    is still a different bf16 value (asserted for the smallest such move).
    unit: shift = p (matches are a_m w_n, |out| <= 29) and the bias is a small integer, zero on
    half the columns -- the QuickGELU probe, whose pre-activation must stay small; there only the
    x = 0 entries resolve a single k (the GPU test asserts 0 ulp on them).
    Returns A [M, K], W [N, K], bias [N] (float32), expected [M, N] (float32, bias included),
    core (expected - bias), a, w, P, b, match (bool [M, N])."""
    p = (K & -K).bit_length() - 1
    P, b = 1 << p, K >> p
    assert K > 0 and b <= 32 and P >= 32, (K, b, P)
    if unit:
        shift = p
    assert 0 <= shift <= p
    rng = np.random.default_rng(seed)
    a = rng.integers(1, 4, M).astype(np.int64)
    w = rng.integers(1, 4, N).astype(np.int64)
    r, c = hadamard_maps(M, N, b, P)
    H = hadamard(P)
    A = np.concatenate([H[rj] for rj in r], axis=1).astype(np.float32) * a[:, None].astype(np.float32)
    W = np.concatenate([H[cj] for cj in c], axis=1).astype(np.float32) * w[:, None].astype(np.float32)
    count = np.zeros((M, N), np.int32)
    for j in range(min(b, MATCH_BLOCKS)):
        count += r[j][:, None] == c[j][None, :]
    for j in range(MATCH_BLOCKS, b):
        assert not (r[j] & 1).any() and (c[j] & 1).all()
    assert count.max(axis=1).min() >= 1 and count.max(axis=0).min() >= 1, "a row or column without a match"
    aw = a[:, None] * w[None, :]
    Ps = P >> shift                                  # a match's size per unit a_m w_n
    A *= np.float32(2.0 ** -shift)
    core = (aw * count * Ps).astype(np.float32)
    if unit:
        bvec = rng.integers(-2, 3, N) * rng.integers(0, 2, N) if bias else np.zeros(N, np.int64)
    else:
        g = max(1, Ps // 8)
        smax = min(2, 128 // g, (2 ** (8 - min(shift, 8)) - 1) // g)   # |bias| + 2^-shift within 8 bits
        bvec = g * rng.integers(-smax, smax + 1, N) if bias else np.zeros(N, np.int64)
        # the smallest single-k move of an unmatched entry survives the bf16 rounding
        for sgn in (-1.0, 1.0):
            assert (bf16_rne(bvec + sgn * 2.0 ** -shift) != bvec).all()
    bvec = bvec.astype(np.float32)
    expected = core + bvec[None, :]
    assert significant_bits(np.unique(expected)).max() <= 8,"an expected value is not exact in bf16 / fp16"
    assert np.abs(expected).max() < 65504 and np.abs(core).max() * 2 < 2 ** 24
    return SimpleNamespace(A=A, W=W, bias=bvec, expected=expected, core=core, a=a, w=w, P=P, b=b, p=p,
                           shift=shift, match=count > 0, M=M, N=N, K=K)


def quickgelu64(x):
    """QuickGELU x sigmoid(1.702 x) in float64."""
    x = np.asarray(x, np.float64)
    return x / (1.0 + np.exp(-1.702 * x))


# ------------------------------------------------------------------ attention probes
def _pack_qkv(q, k, v):
    """q, k, v [B, S, H, 64] -> packed rows [B*S, 3W] (q | k | v), float32."""
    B, S, H, _ = q.shape
    return np.concatenate([x.reshape(B * S, H * 64) for x in (q, k, v)], axis=1).astype(np.float32)


def _bf16_round32(x):
    return bf16_rne(np.asarray(x, np.float64)).astype(np.float32)


IMPULSE_VALUES = (1.0, -1.5, 1.25, -1.75, 1.375, -1.125)   # bf16-exact; neighbours in b differ


def impulse_keys(B, S, H, seed=0):
    """j*(b, h, d): the key that carries column d's only non-zero V entry.  Per head g = b H + h
    (lo = min(S, 64)):
      d <   4   keys 0..3 in EVERY head: the rows right behind the previous sequence's last key --
                what a padded key that leaks by one to four rows reads;
      d <  16   early keys (d 4 + g) mod lo: the rest of that tile's reach, a fourth of it per head;
      d <  20   keys S - 1 .. S - 4 in every head;
      d <  32   the last keys S - 1 - ((d - 16) 4 + g) mod lo: the last key tile;
      d >= 32   a fixed permutation of [0, S) walked 32 keys per head: with B H 32 >= S every
                key position is hit (asserted)."""
    assert B * H * 32 >= S, "too few columns to hit every key position"
    sweep = np.random.default_rng(seed).permutation(S)
    g = (np.arange(B)[:, None] * H + np.arange(H)[None, :])[:, :, None]          # [B, H, 1]
    d = np.arange(64)[None, None, :]
    lo = min(S, 64)
    early = np.where(d < 4, d % lo, (d * 4 + g) % lo)
    late = S - 1 - np.where(d < 20, (d - 16) % lo, ((d - 16) * 4 + g) % lo)
    j = np.where(d < 16, early, np.where(d < 32, late, sweep[(g * 32 + (d - 32)) % S]))
    assert np.array_equal(np.unique(j), np.arange(S))
    assert (j[:, :, :4] == np.arange(4) % lo).all()
    return j                                                                     # [B, H, 64]


def attention_impulse(B, S, H, causal, seed=0):
    """q = 0: every visible key has weight exactly 1 / n_i (n_i = S, or i + 1 when causal); k is
    random (~4 N(0,1)) and must not matter; v is zero except v[j*(b,h,d), d] = val(b,h,d).
    Expected out[i, d] = val / n_i where j* is visible to row i, else exactly 0: every key position
    against every query row in one launch -- padded keys of the last tile, the causal count of
    each row, and leakage from the next sequence's rows (its early keys carry other values)."""
    rng = np.random.default_rng(seed)
    q = np.zeros((B, S, H, 64), np.float32)
    k = _bf16_round32(rng.standard_normal((B, S, H, 64)) * 4).reshape(B, S, H, 64)
    j = impulse_keys(B, S, H, seed)
    b_, h_, d_ = np.meshgrid(np.arange(B), np.arange(H), np.arange(64), indexing="ij")
    val = np.asarray(IMPULSE_VALUES, np.float32)[(b_ + h_ + d_) % len(IMPULSE_VALUES)]
    v = np.zeros((B, S, H, 64), np.float32)
    v[b_, j, h_, d_] = val
    i = np.arange(S)[None, :, None, None]
    n = (i + 1 if causal else np.full_like(i, S)).astype(np.float64)
    visible = (j[:, None] <= i) if causal else np.ones((B, S, H, 64), bool)
    expected = np.where(visible, val[:, None].astype(np.float64) / n, 0.0)
    return SimpleNamespace(qkv=_pack_qkv(q, k, v), expected=expected.reshape(B * S, H * 64),
                           visible=np.broadcast_to(visible, (B, S, H, 64)).reshape(B * S, H * 64),
                           keys=j, B=B, S=S, H=H, causal=causal)


def select_targets(S, causal, rng):
    """t(i): key 0, key S - 1 and both sides of every 16-key boundary (hence of every 32 / 64 one)
    are targets of some row; causal: t(i) = i on about half the rows, a random t(i) <= i on the
    rest; non-causal: the other rows' targets are random, early and late.
    Causal rows for the required keys are taken latest key first, each a random unused row at or
    after its key: row c itself is always unused then (rows used so far serve later keys and lie
    at or after them), so no assignment can displace another."""
    need = sorted({0, S - 1} | {c + o for c in range(16, S, 16) for o in (-1, 0)})
    if not causal:
        t = rng.integers(0, S, S)
        rows = rng.permutation(S)
        t[rows[:len(need)]] = need
    else:
        diag = rng.random(S) < 0.5
        t = np.where(diag, np.arange(S), (rng.random(S) * (np.arange(S) + 1)).astype(np.int64))
        used = np.zeros(S, bool)
        for c in reversed(need):
            rows = np.flatnonzero(~used[c:]) + c
            row = rows[rng.integers(0, len(rows))]
            used[row] = True
            t[row] = c
        assert (t <= np.arange(S)).all() and t[S - 1] == S - 1
    assert set(need) <= set(t.tolist())
    return t


def attention_select(B, S, H, causal, seed=0):
    """Random +-1 keys per (sequence, head) and q_i = 8 k_t(i): the target's logit q.k / 8 is 64,
    every other one k_t.k_j <= 40 (asserted here; a head whose random keys miss that is drawn again,
    `redraws` counts them), so the other keys' total weight is below
    S e^-24 < 2^-24 and out[i] = v[t(i)].  v is random bf16 with |v| >= 2^-6, so that this residue
    (S e^-24 max|v| < 2e-7) is far below an output ulp (>= 2^-14)."""
    rng = np.random.default_rng(seed)
    k = np.zeros((B, S, H, 64), np.float32)
    redraws = 0
    for b in range(B):
        for h in range(H):
            while True:      # (a head whose keys miss the margin is drawn again: ~1 % of them at S = 640)
                kh = rng.integers(0, 2, (S, 64)).astype(np.float32) * 2 - 1
                gram = kh @ kh.T
                np.fill_diagonal(gram, -64)
                if gram.max() <= 40:
                    break
                redraws += 1
            k[b, :, h] = kh
    v = _bf16_round32(rng.standard_normal((B, S, H, 64))).reshape(B, S, H, 64)
    v = np.where(np.abs(v) < 2.0 ** -6, np.copysign(np.float32(2.0 ** -6), v), v).astype(np.float32)
    t = np.stack([np.stack([select_targets(S, causal, rng) for _ in range(H)]) for _ in range(B)])   # [B, H, S]
    bi, hi = np.arange(B)[:, None, None], np.arange(H)[None, :, None]
    q = 8 * k[bi, t, hi].transpose(0, 2, 1, 3)                                   # [B, S, H, 64]
    dots = np.einsum("bihd,bjhd->bhij", q / 8, k)                                # k_t(i) . k_j
    off = dots.copy()
    off[bi, hi, np.arange(S)[None, None, :], t] = -np.inf
    assert (dots[bi, hi, np.arange(S)[None, None, :], t] == 64).all()
    assert S == 1 or off.max() <= 40, f"largest off-target dot product {off.max()} (seed {seed})"
    expected = v[bi, t, hi].transpose(0, 2, 1, 3).astype(np.float64)
    return SimpleNamespace(qkv=_pack_qkv(q, k, v), expected=expected.reshape(B * S, H * 64), targets=t,
                           B=B, S=S, H=H, causal=causal, redraws=redraws, max_off=float(off.max()))
