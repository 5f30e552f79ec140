"""Exact-result probes for the GEMM and attention kernels of the product library (no A/B build).

The parity tests of test_gpu_ops.py compare against a float reference with one global tolerance
(2e-2 / 3e-2 of the largest output), or bit for bit against another kernel of this repository.
One dropped, doubled or mis-paired k element of a K = 768 GEMM moves an output by ~0.02, one key
left out of (or let into) a 577-key softmax by ~|v| / 577: both far inside those tolerances, and
a defect shared by the variants passes the bit-identity tests too.  Here the inputs come from
tests/probes.py: their correct result is known in closed form and is exactly representable in
the output type, so the assertion is equality (or one / two output ulps where a transcendental or
a reciprocal is involved) and any single misplaced element fails it.  test_probes_host.py shows on
the CPU that the closed forms are right and that the comparisons used here reject such defects.

Every tolerance below is one of: 0; 1 or 2 output ulps (derived where used); the per-element
rounding bound of test_gemm_elementwise_bound / test_gemm_ln_elementwise_bound; or an existing
test's value (test_gemm_residual's statistics, test_attention_f32_vs_float64's 2e-6).

Shapes are the smallest that reach each dispatch branch, read off launch<EPI>() in gemm.hip,
gemm_mx() in gemm_mx.hip, attention() in attention.hip and attention_f32() in precise.hip for a
256-CU part; each parametrisation id names its branch.
"""
import numpy as np
import pytest

import probes
from oracle import mx_ref

pytestmark = pytest.mark.gpu


def _lib():
    from miclip import _native
    return _native


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _dev(x, gpu, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to(gpu)


def _assert_bits_equal(out, expected, what):
    """out (bf16 / fp16 / f32 tensor on the GPU) == expected (float32 numpy, exact in out's type),
    compared as bits on the device; the first offending entries are printed on a mismatch."""
    import torch
    want = torch.from_numpy(expected).to(out.device).to(out.dtype)
    assert torch.equal(want.float().cpu(), torch.from_numpy(expected)), "expectation not exact in the output type"
    ity = torch.int32 if out.dtype == torch.float32 else torch.int16
    if not torch.equal(out.view(ity), want.view(ity)):
        probes.assert_equal(out.float().cpu().numpy(), expected, what)
        raise AssertionError(f"{what}: values equal but bits differ (a -0)")


# ------------------------------------------------------------------------------ mi_op_gemm
# launch<EPI>() in gemm.hip, product build, cus = 256; nt = ceil(M / 256) (N / 256), big = N % 256 == 0
# and M >= 1024, staged = big and K >= 96, gemm_8q_ok = N % 256 == 0, K % 128 == 0, K >= 256, M >= 256.
# Epilogue 0 with nt < 64 takes the small-grid path first: 64 x 64 tiles when nt2 (the count of 128 x 128
# tiles) < cus, else 128 x 128 tiles.  tile_count() floors N / bn, so N = 384 counts one 256-wide but three
# 128-wide n-tiles: with N % 256 == 0, nt < 64 gives nt2 <= 4 nt <= 252 < cus and the 128 x 128 branch cannot
# be taken on 256 CUs; with N % 256 == 128 it can.
GEMM_EXACT = [
    pytest.param(0, 200, 256, 256, id="epi0-200x256x256-tiles64"),
    pytest.param(0, 10900, 384, 256, id="epi0-10900x384x256-smallgrid-tiles128"),
    pytest.param(0, 16384, 384, 64, id="epi0-16384x384x64-generic128"),
    pytest.param(3, 300, 384, 256, id="epi3-300x384x256-generic128"),
    pytest.param(3, 1024, 256, 64, id="epi3-1024x256x64-generic256"),
    pytest.param(2, 1024, 256, 64, id="epi2-1024x256x64-generic256"),
    pytest.param(0, 4096, 1024, 64, id="epi0-4096x1024x64-generic256"),
    pytest.param(0, 4096, 1024, 192, id="epi0-4096x1024x192-pingpong-persistent"),
    pytest.param(0, 4096, 1024, 1088, id="epi0-4096x1024x1088-pingpong-rowstores"),
    pytest.param(3, 1024, 256, 256, id="epi3-1024x256x256-pingpong-staged-f32"),
    pytest.param(2, 1100, 256, 256, id="epi2-1100x256x256-pingpong-staged-f32"),
    pytest.param(0, 4096, 1024, 256, id="epi0-4096x1024x256-gemm8q-one-tile"),
    pytest.param(0, 8500, 2048, 256, id="epi0-8500x2048x256-gemm8q-persistent"),
    pytest.param(0, 5400, 3072, 768, id="epi0-5400x3072x768-gemm8q-grouped"),
]


@pytest.mark.parametrize("epi,M,N,K", GEMM_EXACT)
def test_gemm_exact(gpu, epi, M, N, K):
    """mi_op_gemm epilogues 0 (bf16), 2 (f32 out += an integer base) and 3 (f32) on the Hadamard
    probe: torch.equal against the closed form, bf16 outputs compared as bits.  One dropped,
    repeated or mis-paired k moves an unmatched entry by +- a_m w_n >= 1 off its bias value
    (|bias| <= 128: a different bf16 value); a lost block of k moves the matched entries.
    Shapes (GEMM_EXACT; launch<EPI>() on 256 CUs), each the smallest that reaches its branch:
      epi0 200x256x256      small-grid path, 64 x 64 tiles: any epi-0 shape with nt < 64 and nt2 < 256; ragged M
      epi0 10900x384x256    small-grid path, 128 x 128 tiles: nt < 64 and nt2 >= 256 needs N % 256 == 128 (N / 256 is
                            floored: nt = 43 x 1, nt2 = 86 x 3 = 258).  N = 384 is the smallest such N that fits
                            (N = 128 needs M > 32640) and M = 10900 > 85 x 128 the smallest M; ragged last M tile
      epi0 16384x384x64     generic 128 x 128: N % 256 != 0 and nt = 64 x 1 = 64, the fewest the path above leaves
      epi3 300x384x256      generic 128 x 128, f32 output: not big (N % 256 != 0); ragged M, 3 x 3 tiles
      epi2/3 1024x256x64    generic 256 x 256: big (M >= 1024, the smallest) with K / 32 < 3, so not staged
      epi0 4096x1024x64     the same at epi 0: 64 tiles
      epi0 4096x1024x192    persistent ping-pong: big, staged, K % 128 != 0 keeps gemm_8q out, K <= 1024.
                            K = 192 = 3 x 64 is the probe shape: not a multiple of 128, three 64-k blocks
                            (K = 128 would reach the kernel too, through gemm_8q's K >= 256)
      epi0 4096x1024x1088   ping-pong with row stores: big, K > 1024, K % 128 != 0, N < 2048.  No K = b 2^p with
                            b in {1, 3} qualifies (K > 1024 makes it a multiple of 128); K = 17 x 64 does, with the
                            builder's never-matching blocks 3..16
      epi3 1024x256x256, epi2 1100x256x256   ping-pong with LDS-staged f32 rows: big, staged; 1100: a partial M tile
      epi0 4096x1024x256    gemm_8q, one tile per workgroup: 64 tiles is where epi 0 first reaches it; K = 4 x 64,
                            its shortest K (two 128-k pairs)
      epi0 8500x2048x256    gemm_8q persistent walk: 34 x 8 = 272 tiles > 256 CUs, partial last M tile
      epi0 5400x3072x768    gemm_8q grouped tile order (default_ngroup_8q(12, 768) = 6): 22 x 12 = 264 tiles, the
                            smallest M that puts two tiles on a workgroup; partial last M tile"""
    import torch
    N_ = _lib()
    p = probes.hadamard_operands(M, N, K, seed=epi + M + N + K)
    A, W, bias = _dev(p.A, gpu, torch.bfloat16), _dev(p.W, gpu, torch.bfloat16), _dev(p.bias, gpu)
    expected = p.expected
    if epi == 0:
        out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=gpu)
    elif epi == 3:
        out = torch.full((M, N), float("nan"), device=gpu)
    else:
        base = np.random.default_rng(M).integers(-1000, 1001, (M, N)).astype(np.float32)
        out = _dev(base, gpu)
        expected = expected + base
    N_.check(N_.lib().mi_op_gemm(A.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr(), M, N, K, epi,
                                 _stream()), "gemm")
    torch.cuda.synchronize()
    _assert_bits_equal(out, expected, f"gemm epi {epi} {M}x{N}x{K}")


def test_gemm_exact_sees_one_flipped_element(gpu):
    """The comparison above has teeth on the device too: with the sign of ONE element of A flipped
    (row 137, k 201 of the 200 x 256 x 256 probe) the kernel's output differs from the closed form
    in that row, at every unmatched entry (bias_n -+ 2 a_m w_n), and nowhere else."""
    import torch
    N_ = _lib()
    M, N, K, m0, k0 = 200, 256, 256, 137, 201
    p = probes.hadamard_operands(M, N, K, seed=5)
    A = p.A.copy()
    A[m0, k0] = -A[m0, k0]
    Ad, W, bias = _dev(A, gpu, torch.bfloat16), _dev(p.W, gpu, torch.bfloat16), _dev(p.bias, gpu)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=gpu)
    N_.check(N_.lib().mi_op_gemm(Ad.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr(), M, N, K, 0,
                                 _stream()), "gemm")
    torch.cuda.synchronize()
    with pytest.raises(AssertionError):
        _assert_bits_equal(out, p.expected, "gemm with one flipped element")
    diff = out.float().cpu().numpy() != p.expected
    assert not np.delete(diff, m0, axis=0).any()
    assert diff[m0][~p.match[m0]].all()
    want = p.expected[m0] + 2 * A[m0, k0] * p.W[:, k0]          # (the flipped product, once removed and once added)
    probes.assert_equal(out[m0].float().cpu().numpy()[~p.match[m0]], want[~p.match[m0]])


GEMM_GELU = [
    pytest.param(300, 256, 256, id="300x256x256-gemm8q-one-tile"),
    pytest.param(300, 256, 3072, id="300x256x3072-gemm8q-long-k"),
    pytest.param(1024, 256, 192, id="1024x256x192-pingpong-persistent"),
    pytest.param(1024, 256, 1088, id="1024x256x1088-pingpong-rowstores"),
    pytest.param(1024, 256, 64, id="1024x256x64-generic256"),
    pytest.param(300, 384, 256, id="300x384x256-generic128"),
]


def _assert_quickgelu(out, p, what):
    """bf16 QuickGELU outputs against bf16_rne(x sigmoid(1.702 x)) of the exact pre-activation x, in
    float64: at most one bf16 ulp, and exactly 0 where x = 0.  Derived, not measured: the device's
    exp and reciprocal are accurate to a few f32 ulps (2^-22 relative), far below the bf16 half-ulp
    (2^-9), so only a near-tie can move the rounding, by one step."""
    x = p.expected.astype(np.float64)
    assert np.abs(x).max() <= 32
    probes.assert_bf16_ulps(out.float().cpu().numpy(), probes.quickgelu64(x), 1, exact=(x == 0), what=what)


@pytest.mark.parametrize("M,N,K", GEMM_GELU)
def test_gemm_quickgelu_exact_preactivation(gpu, M, N, K):
    """mi_op_gemm epilogue 1 on the unit-scale Hadamard probe (|x| <= 32, x = 0 on about half the
    entries): a single wrong k turns a zero into +- a_m w_n 2^-p / 2, which the 0-ulp clause sees.
    Shapes (GEMM_GELU): epi 1 never takes the small-grid path, so the smallest shape of each branch serves:
      300x256x256    gemm_8q (M >= 256, N % 256 == 0, K % 128 == 0, K >= 256): its shortest K, a partial second M tile
      300x256x3072   the same with c_proj's K = 3072 (24 pairs of K tiles)
      1024x256x192   persistent ping-pong (big: M >= 1024; K % 128 != 0, K <= 1024)
      1024x256x1088  ping-pong with row stores (K > 1024, K % 128 != 0, N < 2048; K = 17 x 64)
      1024x256x64    generic 256 x 256 (big, K / 32 < 3)
      300x384x256    generic 128 x 128 (N % 256 != 0)"""
    import torch
    N_ = _lib()
    p = probes.hadamard_operands(M, N, K, seed=M + N + K, unit=True)
    A, W, bias = _dev(p.A, gpu, torch.bfloat16), _dev(p.W, gpu, torch.bfloat16), _dev(p.bias, gpu)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=gpu)
    N_.check(N_.lib().mi_op_gemm(A.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr(), M, N, K, 1,
                                 _stream()), "gemm")
    torch.cuda.synchronize()
    _assert_quickgelu(out, p, f"gemm epi 1 {M}x{N}x{K}")


# ------------------------------------------------------------------------------ mi_op_gemm_ln
def _half_slots(x16):
    """fp16 rows [rows, W] in the half-slot layout: f32 slots whose first halves hold the row."""
    import torch
    rows, W = x16.shape
    slot = torch.zeros(rows, W, dtype=torch.float32)
    slot.view(torch.float16).view(rows, 2 * W)[:, :W] = x16
    return slot


def _ln_vectors(p, gelu, seed):
    """rs[m] = (2^e_m, q_m 2^e_m), colsum, colc for the gemm_ln probe, and the expected output
    2^e acc - q 2^e colsum + colc, every term a small dyadic: exact in f32 in any evaluation order.
    Plain probe (gelu 0): e in {-1, 0, 1}, q in {-1, 0, 1}, colsum in {0, +-32, +-64} P/256, colc in
    {0, +-64} P/256.  With acc = a w P count (a w count <= 27) the result is a multiple of 2^e P / 8
    below 256 of them -- 8 significant bits, exact in bf16 -- and an unmatched entry, at most
    (64 + 64 2^e) P/256 in size, moved by one k (+- a w 2^e) is another bf16 value (both asserted).
    Unit probe (gelu 1): acc = a w count <= 27, e in {-1, 0}, q, colsum in {-1, 0, 1}, colc in {-2..2}
    and zero on half the columns: |x| <= 27 + 1 + 2 <= 32, and x = 0 on about a third of the entries."""
    rng = np.random.default_rng(seed)
    M, N = p.M, p.N
    acc = p.core.astype(np.float64)
    if gelu:
        e = rng.integers(-1, 1, M)
        q = rng.integers(-1, 2, M)
        colsum = rng.integers(-1, 2, N).astype(np.float64)
        colc = (rng.integers(-2, 3, N) * rng.integers(0, 2, N)).astype(np.float64)
    else:
        assert p.P % 256 == 0 and p.shift == 0
        f = p.P // 256
        e = rng.integers(-1, 2, M)
        q = rng.integers(-1, 2, M)
        colsum = (32 * f * rng.integers(-2, 3, N)).astype(np.float64)
        colc = (64 * f * rng.integers(-1, 2, N)).astype(np.float64)
    rstd = 2.0 ** e
    expected = rstd[:, None] * acc - (q * rstd)[:, None] * colsum[None, :] + colc[None, :]
    assert probes.significant_bits(np.unique(expected)).max() <= 8
    if not gelu:
        un = np.where(p.match, np.nan, expected)
        for sgn in (-1.0, 1.0):
            moved = probes.bf16_rne(np.nan_to_num(un + sgn * rstd[:, None]))
            assert (moved != expected)[~p.match].all()
    rs = np.zeros((M + 256, 2), np.float32)          # readable for M + 256 rows (the header's contract)
    rs[:M, 0], rs[:M, 1] = rstd, q * rstd
    return rs, colsum.astype(np.float32), colc.astype(np.float32), expected.astype(np.float32)


GEMM_LN = [
    pytest.param(256, 256, 256, True, id="256x256x256-halfslot-one-tile"),     # the smallest shape it accepts
    pytest.param(300, 256, 768, True, id="300x256x768-halfslot-partial-tile"),   # partial last M tile, K = 3 x 256
    pytest.param(300, 512, 256, False, id="300x512x256-plain-rows"),            # lda = K
    pytest.param(8500, 2048, 256, True, id="8500x2048x256-halfslot-persistent"),  # 272 tiles > 256 CUs
    pytest.param(5400, 3072, 768, False, id="5400x3072x768-plain-grouped"),     # grouped tile order, 264 tiles
]


@pytest.mark.parametrize("gelu", [0, 1])
@pytest.mark.parametrize("M,N,K,half_slot", GEMM_LN)
def test_gemm_ln_exact(gpu, M, N, K, half_slot, gelu):
    """mi_op_gemm_ln with x16 / Wf the Hadamard probe in fp16 and rs, colsum, colc chosen by
    _ln_vectors (not derived from Wf: the kernel must use the vectors it is given): gelu 0 equals the
    closed form bit for bit; gelu 1 is within one bf16 ulp of the float64 QuickGELU of the exact
    pre-activation and exactly 0 where that is 0 (as test_gemm_quickgelu_exact_preactivation).
    Shapes (GEMM_LN): the folded epilogues run on gemm_8q only (M >= 256, N % 256 == 0, K % 128 == 0, K >= 256):
      256x256x256    the smallest shape it accepts: one tile, two 128-k pairs, half-slot rows (lda = 2 K)
      300x256x768    a partial last M tile, K = 3 x 256, half-slot rows
      300x512x256    plain rows (lda = K), two n-tiles
      8500x2048x256  272 tiles > 256 CUs: the persistent walk, some workgroups take two tiles; half-slot rows
      5400x3072x768  264 tiles in the grouped order (default_ngroup_8q(12, 768) = 6), plain rows: c_fc's N and K"""
    import torch
    N_ = _lib()
    p = probes.hadamard_operands(M, N, K, seed=M + N + K + gelu, unit=bool(gelu), bias=False)
    rs, colsum, colc, expected = _ln_vectors(p, gelu, seed=M + K)
    x16 = torch.from_numpy(p.A).half()
    xd = _half_slots(x16).to(gpu) if half_slot else x16.to(gpu)
    lda = 2 * K if half_slot else K
    Wd, rsd, sd, cd = _dev(p.W, gpu, torch.float16), _dev(rs, gpu), _dev(colsum, gpu), _dev(colc, gpu)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=gpu)
    N_.check(N_.lib().mi_op_gemm_ln(xd.data_ptr(), lda, rsd.data_ptr(), Wd.data_ptr(), sd.data_ptr(), cd.data_ptr(),
                                    out.data_ptr(), M, N, K, gelu, _stream()), "gemm_ln")
    torch.cuda.synchronize()
    if gelu:
        p.expected = expected
        _assert_quickgelu(out, p, f"gemm_ln gelu {M}x{N}x{K}")
    else:
        _assert_bits_equal(out, expected, f"gemm_ln {M}x{N}x{K}")


# ------------------------------------------------------------------------------ mi_op_gemm_residual
GEMM_RESIDUAL = [
    pytest.param(256, 256, 256, True, id="256x256x256-one-tile"),
    pytest.param(300, 768, 3072, True, id="300x768x3072-partial-tile-long-k"),
    pytest.param(300, 1024, 256, False, id="300x1024x256-plain-rows"),
    pytest.param(16500, 1024, 256, True, id="16500x1024x256-walk-longer-than-grid"),   # 65 x 4 = 260 tiles > 256 CUs
]


@pytest.mark.parametrize("M,W,K,half_slot", GEMM_RESIDUAL)
def test_gemm_residual_exact(gpu, M, W, K, half_slot):
    """mi_op_gemm_residual: x16 small integers, A / W the Hadamard probe scaled so that a match is
    64 a w (shift = p - 6): the stored stream f16(x16 + bf16(A W^T + bias)) is x16 + the closed form,
    an integer of magnitude <= 2048 (asserted), exact in fp16 -- compared bit for bit, without going
    through mi_op_gemm.  A single wrong k moves an unmatched entry by a w 2^-shift >= 2^-4, which
    survives the bf16 rounding of the delta (|bias| <= 16, asserted by the builder) and the fp16
    rounding of the sum (|x16 + bias| < 64).  rs and ps against float64 statistics of the expected
    rows with test_gemm_residual's tolerances.
    Shapes (GEMM_RESIDUAL; gemm_8q's EPI_RES16_BF16, W % 256 == 0, W <= 1024, K % 128 == 0, M >= 256):
      256x256x256    the smallest shape it accepts, half-slot rows (ldx = 2 W)
      300x768x3072   a partial last M tile, c_proj's W and K (K = 3 x 1024)
      300x1024x256   plain rows (ldx = W), the widest W
      16500x1024x256 65 x 4 = 260 tiles > 256 CUs: a walk longer than the grid, partial last M tile"""
    import torch
    N_ = _lib()
    p0 = (K & -K).bit_length() - 1
    p = probes.hadamard_operands(M, W, K, seed=M + W + K, shift=p0 - 6)
    x16 = np.random.default_rng(K + M).integers(-20, 21, (M, W)).astype(np.float32)
    s = x16 + p.expected
    assert np.abs(s).max() <= 2048 and np.abs(x16 + p.bias).max() < 64 and (s == np.rint(s)).all()
    Ad, Wd, bd = _dev(p.A, gpu, torch.bfloat16), _dev(p.W, gpu, torch.bfloat16), _dev(p.bias, gpu)
    xh = torch.from_numpy(x16).half()
    xd = _half_slots(xh).to(gpu) if half_slot else xh.to(gpu)
    ldx = 2 * W if half_slot else W
    ps = torch.full((M, W // 64, 2), float("nan"), device=gpu)
    rs = torch.full((M, 2), float("nan"), device=gpu)
    N_.check(N_.lib().mi_op_gemm_residual(xd.data_ptr(), ldx, Ad.data_ptr(), K, Wd.data_ptr(), bd.data_ptr(),
                                          ps.data_ptr(), rs.data_ptr(), M, W, K, _stream()), "gemm_residual")
    torch.cuda.synchronize()
    got = xd.view(torch.float16).view(M, 2 * W)[:, :W].contiguous() if half_slot else xd
    _assert_bits_equal(got, s, f"gemm_residual {M}x{W}x{K}")
    sd = s.astype(np.float64)
    mean = sd.mean(1)
    rstd = 1 / np.sqrt(((sd - mean[:, None]) ** 2).mean(1) + 1e-5)
    np.testing.assert_allclose(rs[:, 0].cpu().double().numpy(), rstd, rtol=2e-6)
    np.testing.assert_allclose(rs[:, 1].cpu().double().numpy(), rstd * mean, rtol=2e-6, atol=2e-6)
    blk = sd.reshape(M, W // 64, 64)
    psum = blk.sum(2)
    pm2 = ((blk - psum[..., None] / 64) ** 2).sum(2)
    np.testing.assert_allclose(ps[..., 0].cpu().double().numpy(), psum, rtol=1e-5, atol=1e-3)
    np.testing.assert_allclose(ps[..., 1].cpu().double().numpy(), pm2, rtol=1e-5, atol=1e-3)


# ------------------------------------------------------------------------------ mi_op_gemm_f32
@pytest.mark.parametrize("M,N,K", [pytest.param(1, 64, 64, id="1x64x64-single-row"),
                                   pytest.param(77, 100, 256, id="77x100x256-ragged-M-N-not-multiple-of-64"),
                                   pytest.param(300, 192, 768, id="300x192x768-several-tiles")])
@pytest.mark.parametrize("epi", [0, 1, 2, 3])
def test_gemm_f32_exact(gpu, M, N, K, epi):
    """mi_op_gemm_f32 (one kernel, a grid of square tiles over any M, N; K % 32 == 0): epilogues 0
    (store), 2 (+= an integer base) and 3 (ReLU) equal the closed form exactly; epilogue 1 is within
    2 f32 ulps of the float64 QuickGELU of the exact pre-activation (unit probe)."""
    import torch
    N_ = _lib()
    p = probes.hadamard_operands(M, N, K, seed=3 * M + N + K + epi, unit=(epi == 1))
    A, W, bias = _dev(p.A, gpu), _dev(p.W, gpu), _dev(p.bias, gpu)
    expected = p.expected
    if epi == 2:
        base = np.random.default_rng(M).integers(-1000, 1001, (M, N)).astype(np.float32)
        out = _dev(base, gpu)
        expected = expected + base
    else:
        out = torch.full((M, N), float("nan"), device=gpu)
    if epi == 3:
        assert M == 1 or (expected < 0).any()      # (the ReLU has something to clamp)
        expected = np.maximum(expected, 0)
    N_.check(N_.lib().mi_op_gemm_f32(A.data_ptr(), W.data_ptr(), bias.data_ptr(), out.data_ptr(), M, N, K, epi,
                                     _stream()), "gemm_f32")
    torch.cuda.synchronize()
    if epi == 1:
        probes.assert_f32_ulps(out.cpu().numpy(), probes.quickgelu64(expected), 2, what="gemm_f32 QuickGELU")
    else:
        _assert_bits_equal(out, expected, f"gemm_f32 epi {epi} {M}x{N}x{K}")


# ------------------------------------------------------------------------------ mi_op_gemm_split2h
SPLIT2H = [
    pytest.param(300, 256, 128, True, 0, id="300x256xK128-gemm8q"),
    pytest.param(300, 256, 128, True, 0x100, id="300x256xK128-gemm8q-role2"),
    pytest.param(1024, 256, 64, True, 0, id="1024x256xK64-pingpong-staged"),
    pytest.param(300, 256, 128, False, 0, id="300x256xK128-nobias-generic128"),
    pytest.param(300, 384, 64, True, 0, id="300x384xK64-generic128"),
]


@pytest.mark.parametrize("epi", [3, 2])
@pytest.mark.parametrize("M,N,K,with_bias,flag", SPLIT2H)
def test_gemm_split2h_exact(gpu, M, N, K, with_bias, flag, epi):
    """mi_op_gemm_split2h on operands produced by mi_op_split2h from the +-{1,2,3} probe: first
    x2 == 0 and power-of-two scales (the split is exact: x1 = x s), then the f32 output equals the
    closed form exactly (epi 3 store, epi 2 += an integer base).
    Shapes (SPLIT2H; launch<EPI>()'s a_f16 branch, K3 = 3 K):
      300x256 K128          gemm_8q: a bias, M >= 256, N % 256 == 0, K3 = 384 (% 128 == 0, >= 256), its shortest K
      300x256 K128 | 0x100  the role-2 [x1 x2] rows read as [x1 x1 x2] (gemm_8q only)
      1024x256 K64          fallback 1, the ping-pong kernel with LDS-staged f32 rows: big and K3 = 192 (% 128 != 0)
      300x256 K128 no bias  fallback 2, the generic 128 x 128 kernel on fp16 operands: no bias keeps gemm_8q out,
                            M < 1024 is not big.  (The generic 256 x 256 kernel cannot be reached: big needs
                            K3 / 32 < 3, and K3 is a multiple of 96.)
      300x384 K64           the generic 128 x 128 kernel with a bias (N % 256 != 0)"""
    import torch
    N_ = _lib()
    L = N_.lib()
    p = probes.hadamard_operands(M, N, K, seed=M + N + K + flag, bias=with_bias)
    A, W = _dev(p.A, gpu), _dev(p.W, gpu)
    role = 2 if flag else 0
    A3 = torch.full((M, (2 if flag else 3) * K), -1, dtype=torch.int16, device=gpu)
    W3 = torch.full((N, 3 * K), -1, dtype=torch.int16, device=gpu)
    sa, sw = torch.empty(M, device=gpu), torch.empty(N, device=gpu)
    N_.check(L.mi_op_split2h(A.data_ptr(), K, M, K, role, 0, A3.data_ptr(), sa.data_ptr(), _stream()), "split2h A")
    N_.check(L.mi_op_split2h(W.data_ptr(), K, N, K, 1, 0, W3.data_ptr(), sw.data_ptr(), _stream()), "split2h W")
    torch.cuda.synchronize()
    a_x2 = A3[:, K:] if flag else A3[:, 2 * K:]
    assert not (a_x2 & 0x7FFF).any() and not (W3[:, K:2 * K] & 0x7FFF).any(), "x2 != 0: the probe is not exact in fp16"
    for sc in (sa, sw):
        m, _ = np.frexp(sc.cpu().numpy())
        assert (m == 0.5).all(), "a scale is not a power of two"
    a1 = A3[:, :K].view(torch.float16).float() * sa[:, None]
    assert torch.equal(a1.cpu(), torch.from_numpy(p.A))
    bias = _dev(p.bias, gpu) if with_bias else None
    expected = p.expected
    if epi == 2:
        base = np.random.default_rng(M + 1).integers(-1000, 1001, (M, N)).astype(np.float32)
        out = _dev(base, gpu)
        expected = expected + base
    else:
        out = torch.full((M, N), float("nan"), device=gpu)
    N_.check(L.mi_op_gemm_split2h(A3.data_ptr(), W3.data_ptr(), sa.data_ptr(), sw.data_ptr(),
                                  bias.data_ptr() if with_bias else None, out.data_ptr(), M, N, 3 * K, epi | flag,
                                  _stream()), "gemm_split2h")
    torch.cuda.synchronize()
    _assert_bits_equal(out, expected, f"gemm_split2h epi {epi} {M}x{N}xK{K}")


# ------------------------------------------------------------------------------ mi_op_gemm_mx
def _quant_gpu(x_bf16):
    import torch
    N_ = _lib()
    rows, K = x_bf16.shape
    q = torch.empty(rows, K, dtype=torch.uint8, device=x_bf16.device)
    s = torch.zeros((K // 128) * (rows + (rows & 1)) * 2, dtype=torch.uint8, device=x_bf16.device)
    N_.check(N_.lib().mi_op_quantize_mx(x_bf16.data_ptr(), q.data_ptr(), s.data_ptr(), rows, K, _stream()), "quant")
    return q, s


GEMM_MX = [
    pytest.param(300, 256, 128, False, 3, id="epi3-300x256x128-dbuf-16x16x128"),
    pytest.param(300, 256, 128, False, 0, id="epi0-300x256x128-dbuf-16x16x128"),
    pytest.param(300, 256, 256, False, 3, id="epi3-300x256x256-pingpong-32x32x64"),
    pytest.param(300, 256, 256, False, 0, id="epi0-300x256x256-pingpong-32x32x64"),
    pytest.param(300, 512, 768, True, 3, id="epi3-300x512x768-pingpong-block-scales"),
    pytest.param(16500, 1024, 256, False, 3, id="epi3-16500x1024x256-persistent"),
    pytest.param(16500, 1024, 256, False, 0, id="epi0-16500x1024x256-persistent"),
    pytest.param(5400, 3072, 256, False, 3, id="epi3-5400x3072x256-persistent-grouped"),
    pytest.param(5400, 3072, 256, False, 0, id="epi0-5400x3072x256-persistent-grouped"),
]


@pytest.mark.parametrize("M,N,K,scaled,epi", GEMM_MX)
def test_gemm_mx_exact(gpu, M, N, K, scaled, epi):
    """mi_op_gemm_mx epilogues 0 (bf16) and 3 (f32) on the Hadamard probe quantised by
    mi_op_quantize_mx: first the dequantised operands (oracle/mx_ref.py) return the probe exactly
    (+-{1,2,3} 2^e are e4m3 values under a power-of-two block scale), then the output equals the
    closed form exactly.  scaled: A' = A 2^(e_m - f_kb), W' = W 2^(h_n + f_kb) with e, h in [-3, 3]
    per row and f in [-6, 6] per 64-k block, as test_gemm_mx_block_scales: the block factors cancel
    in every product and out = bias + core 2^(e_m + h_n), still exact (f32 output only: the scaled
    values need more than bf16's 8 bits).
    Shapes (GEMM_MX; gemm_mx()'s product dispatch: staged = K / 64 >= 3, persistent = at least one tile per CU
    and K <= 2048):
      300x256x128     K = 128, two 64-k blocks: the double-buffered 16x16x128 kernel, the only K that reaches it
      300x256x256     the ping-pong 32x32x64 kernel, one workgroup per tile: its shortest K, 2 tiles < 256 CUs
      300x512x768     the same kernel with the block scales, K = 3 x 256
      16500x1024x256  65 x 4 = 260 tiles >= 256 CUs: the persistent kernel (m-major walk: 4 n-tiles), some
                      workgroups walk two tiles
      5400x3072x256   the persistent kernel's grouped tile order (n-tiles in groups of 6: N / 256 >= 12 and
                      6 x 256 x K <= 2400000): 12 n-tiles is the narrowest such N, 22 x 12 = 264 tiles the fewest
                      M tiles that keep it persistent; its shortest staged K"""
    import torch
    N_ = _lib()
    p = probes.hadamard_operands(M, N, K, seed=M + N + K + epi)
    A, W, expected = p.A, p.W, p.expected
    if scaled:
        rng = np.random.default_rng(K)
        e, h = rng.integers(-3, 4, M), rng.integers(-3, 4, N)
        f = np.repeat(rng.integers(-6, 7, K // 64), 64)
        A = (A * 2.0 ** (e[:, None] - f[None, :])).astype(np.float32)
        W = (W * 2.0 ** (h[:, None] + f[None, :])).astype(np.float32)
        expected = (p.bias[None, :] + p.core.astype(np.float64) * 2.0 ** (e[:, None] + h[None, :])).astype(np.float32)
    qa, sa = _quant_gpu(_dev(A, gpu, torch.bfloat16))
    qw, sw = _quant_gpu(_dev(W, gpu, torch.bfloat16))
    torch.cuda.synchronize()
    for q, s, x, rows in ((qa, sa, A, M), (qw, sw, W, N)):
        back = mx_ref.dequantize(q.cpu().numpy(), mx_ref.from_stage_major(s.cpu().numpy(), rows, K))
        assert np.array_equal(back, x.astype(np.float64)), "quantisation does not return the probe"
    bias = _dev(p.bias, gpu)
    out = torch.full((M, N), float("nan"), dtype=torch.float32 if epi == 3 else torch.bfloat16, device=gpu)
    N_.check(N_.lib().mi_op_gemm_mx(qa.data_ptr(), sa.data_ptr(), qw.data_ptr(), sw.data_ptr(), bias.data_ptr(),
                                    out.data_ptr(), M, N, K, epi, _stream()), "gemm_mx")
    torch.cuda.synchronize()
    _assert_bits_equal(out, expected, f"gemm_mx epi {epi} {M}x{N}x{K}")


# ------------------------------------------------------------------------------ mi_op_attention
# attention() in attention.hip, product build:
#   S <= 64                      attention_flash_kernel<1, 2, 1> (one chunk, 4 waves)
#   64 < S <= 320, non-causal    attention_res_kernel<8>
#   S > 320, non-causal          attention_r32_kernel<12>
#   S > 64 causal, or flag 0x200 attention_flash_kernel<NT, 1>, NT = ceil(ceil(S / 16) / 8) = 1..5
def _attn_kernel(S, causal, flag):
    if S <= 64:
        return "flash-1-2-1"
    if causal or flag:
        return f"flash-NT{((S + 15) // 16 + 7) // 8}"
    return "res8" if S <= 320 else "r32-12"


ATTN_CASES = [(S, 0, 0, 128) for S in (1, 17, 50, 64, 65, 77, 97, 257, 321, 577)] + [(640, 0, 0, 640)] + \
             [(S, 1, 0, 128) for S in (10, 77, 128, 300)] + [(640, 1, 0, 640)] + \
             [(S, 0, 0x200, 128) for S in (65, 257, 577)] + [(50, 0, 0, 768)]
ATTN_PARAMS = [pytest.param(S, c, f, W, id=f"S{S}-{'causal' if c else 'full'}-W{W}-{_attn_kernel(S, c, f)}")
               for S, c, f, W in ATTN_CASES]


def _run_attention(gpu, p, flags):
    import torch
    N_ = _lib()
    B, S, W = p.B, p.S, 64 * p.H
    qkv = _dev(p.qkv, gpu, torch.bfloat16)
    out = torch.full((B * S, W), float("nan"), dtype=torch.bfloat16, device=gpu)
    N_.check(N_.lib().mi_op_attention(qkv.data_ptr(), out.data_ptr(), B, S, W, flags, _stream()), "attention")
    torch.cuda.synchronize()
    return out.float().cpu().numpy()


@pytest.mark.parametrize("S,causal,flag,W", ATTN_PARAMS)
def test_attention_impulse(gpu, S, causal, flag, W):
    """q = 0: every visible key weighs exactly 1 and the row sum is the integer n_i, so only the
    reciprocal and the final rounding remain: at most one bf16 ulp from bf16_rne(val / n_i), and
    exactly 0 where the column's key is not visible (causal).  Every key position meets every query
    row: a padded key of the last 16 / 32 / 64-key tile that leaks reads the next sequence's first
    rows, whose early keys carry other values (B >= 2; B H 32 >= S so that all positions are hit).
    Keys 0..3 carry a value in every head, so a leak of one to four rows is seen in every head; rows
    further behind carry one in every fourth head.
    (A counted key whose V row is all zero only moves n_i by one: that is above one bf16 ulp for
    rows of fewer than ~128 keys -- S <= 97 here and the early causal rows -- and is seen at every
    length by the f32 kernels' tolerance in test_attention_f32_probes.)
    Lengths (ATTN_CASES; the id names the kernel attention() picks):
      S <= 64 attention_flash_kernel<1, 2, 1>: 1 (one key), 17 and 50 (a partial 16- / 64-key tile; B/32's 50
        tokens, once at W = 768, twelve heads), 64 (its last length, no padding)
      64 < S <= 320 non-causal attention_res_kernel<8>: 65 (its first length: one key in the last tile), 77 and 97
        (partial tiles of 16, 32 and 64 keys), 257 (L/14: one key in the last tile)
      S > 320 non-causal attention_r32_kernel<12>: 321 (its first length), 577 (L/14@336), 640 (the longest; W = 640)
      causal S > 64 attention_flash_kernel<NT, 1>: 77 (text), 128 (whole tiles), 300, 640 (NT = 1, 1, 3, 5); causal 10
        runs on the S <= 64 kernel
      flag 0x200, the streaming kernel on non-causal rows: 65, 257, 577 (NT = 1, 3, 5)"""
    H = W // 64
    B = max(2, -(-S // (32 * H)))
    p = probes.attention_impulse(B, S, H, causal, seed=S + causal)
    probes.check_impulse(_run_attention(gpu, p, causal | flag), p)


@pytest.mark.parametrize("S,causal,flag,W", ATTN_PARAMS)
def test_attention_select(gpu, S, causal, flag, W):
    """q_i = 8 k_t(i) on +-1 keys: logit 64 on the target, <= 40 elsewhere, so out[i] = v[t(i)] up to
    S e^-24.  At most two bf16 ulps: with the lazy rescale (RESCALE = 8) the target's weight is
    bf16(2^x) / l with x up to 8, not 1 -- one rounding of P (2^-9 relative) and one of the output;
    a wrong key is off by O(|v|) in nearly every column.  Targets cover key 0, key S - 1, both sides
    of every 16-key boundary, and for causal rows the diagonal."""
    H = W // 64
    p = probes.attention_select(2, S, H, causal, seed=S % 3)
    probes.check_select(_run_attention(gpu, p, causal | flag), p)


# ------------------------------------------------------------------------------ mi_op_attention_f32
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("S", [1, 33, 64, 65, 128, 129, 257])
@pytest.mark.parametrize("probe", ["impulse", "select"])
def test_attention_f32_probes(gpu, probe, S, causal):
    """Both probes through mi_op_attention_f32 at test_attention_f32_vs_float64's tolerance
    (2e-6 max(1, |ref|)), plus exact zeros in the impulse probe where the key is masked.
    Lengths (attention_f32()): S <= 64 attn_f32s_kernel (split-f16 operands): 1, 33 and 64 (two key tiles, partial
    and whole); 64 < S <= 128 attn_f32_mfma_kernel: 65 and 128 (three and four key tiles, the first and last
    length); S > 128 attn_f32_kernel (per row): 129 (its first length) and 257 (L/14's)."""
    import torch
    N_ = _lib()
    H = 2
    if probe == "impulse":
        p = probes.attention_impulse(max(2, -(-S // (32 * H))), S, H, causal, seed=S + causal)
    else:
        p = probes.attention_select(2, S, H, causal, seed=S % 3)
    B, W = p.B, 64 * H
    d = _dev(p.qkv, gpu)
    out = torch.full((B * S, W), float("nan"), device=gpu)
    N_.check(N_.lib().mi_op_attention_f32(d.data_ptr(), out.data_ptr(), B, S, W, causal, _stream()), "attn f32")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.isfinite(got).all()
    (probes.check_impulse if probe == "impulse" else probes.check_select)(got, p, f32=True)


# ------------------------------------------------------------------------------ per-element bounds on random inputs
def _bound_check(got, ref, bound, what):
    err = np.abs(got - ref)
    ratio = err / bound
    i = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"{what}: max err / bound = {ratio[i]:.3f} at {i} (err {err[i]:.3e}, bound {bound[i]:.3e}, ref {ref[i]:.4f})")
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} beyond the bound; worst err / bound {ratio[i]:.3f}"


@pytest.mark.parametrize("M,N,K", [(100, 128, 64), (513, 384, 768), (3200, 2304, 768)])
@pytest.mark.parametrize("epi", [0, 1])
def test_gemm_elementwise_bound(gpu, M, N, K, epi):
    """test_gemm's random inputs, each output against its own bound (small outputs count too), at three of
    its shapes: 100x128x64 (64 x 64 tiles at epi 0, generic 128 x 128 at epi 1), 513x384x768 (several tiles
    of the same kernels) and 3200x2304x768 (13 x 9 tiles on gemm_8q, the towers' main kernel):

        |got - ref| <= 2^-8 |ref| + L c K 2^-24 (|A| |W|^T)[m, n],   c = 2, L = 1 (1.1 for QuickGELU)

    ref = A W^T + bias (then QuickGELU) in float64 on the bf16 operands.  Second term: the f32
    accumulation of K products and the bias add, in any order, is off by at most
    gamma_(K+1) sum_k |a_k w_k| + 2^-24 |bias| <= 2 K 2^-24 sum|a w| (the standard bound, u = 2^-24;
    the products of bf16 values are exact in f32); QuickGELU x sigmoid(1.702 x) has Lipschitz constant
    < 1.1 (its derivative peaks at 1.0998), and its f32 evaluation adds a few 2^-24 |g|.  First term:
    rounding the f32 value to bf16 (8 significant bits) is off by at most half an ulp <= 2^-8 of it.
    The factor c = 2 leaves room for the (1 + 2^-8) cross term and the bias add."""
    import torch
    N_ = _lib()
    g = torch.Generator(device="cpu").manual_seed(M * 7 + N + K + epi)
    A = (torch.randn(M, K, generator=g) * 0.5).bfloat16()
    W = (torch.randn(N, K, generator=g) * K ** -0.5).bfloat16()
    bias = torch.randn(N, generator=g).float()
    Ad, Wd, bd = A.to(gpu), W.to(gpu), bias.to(gpu)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=gpu)
    N_.check(N_.lib().mi_op_gemm(Ad.data_ptr(), Wd.data_ptr(), bd.data_ptr(), out.data_ptr(), M, N, K, epi,
                                 _stream()), "gemm")
    torch.cuda.synchronize()
    ref = (A.double() @ W.double().t() + bias.double()).numpy()
    mag = (A.double().abs() @ W.double().abs().t()).numpy()
    lip = 1.0
    if epi == 1:
        ref, lip = probes.quickgelu64(ref), 1.1
    bound = 2.0 ** -8 * np.abs(ref) + lip * 2 * K * 2.0 ** -24 * mag
    _bound_check(out.double().cpu().numpy(), ref, bound, f"gemm epi {epi} {M}x{N}x{K}")


@pytest.mark.parametrize("M,N,K", [(256, 256, 256), (1000, 2304, 768)])
@pytest.mark.parametrize("gelu", [0, 1])
def test_gemm_ln_elementwise_bound(gpu, M, N, K, gelu):
    """test_gemm_ln's random inputs (half-slot rows), each output against its own bound:

        |got - ref| <= 2^-8 |ref| + L rstd_m (c K 2^-24 sum_k |x_k| |Wf_nk| + 2^-11 sum_k |x_k| |W_nk gamma_k|)

    c = 2, L = 1 (1.1 with QuickGELU); ref = LN(x) W^T + b in float64 with the unfolded weights.
    The kernel computes rstd (x . Wf) - rstd mean colsum + colc: the f32 accumulation error of
    x . Wf (as test_gemm_elementwise_bound) and the rounding of Wf = fp16(W gamma) (11 significant
    bits: 2^-11 relative per element) both enter multiplied by rstd; the roundings of colsum, colc, rs
    and of the three-term epilogue are a few 2^-24 of terms no larger than sum |x| |Wf|, inside c = 2."""
    import torch
    N_ = _lib()
    g = torch.Generator(device="cpu").manual_seed(M + N + K + gelu)
    x16 = (torch.randn(M, K, generator=g) * 2 + 0.5).half()
    W = torch.randn(N, K, generator=g) * K ** -0.5
    gamma = 1 + 0.2 * torch.randn(K, generator=g)
    beta = 0.1 * torch.randn(K, generator=g)
    bias = 0.1 * torch.randn(N, generator=g)
    Wg = W.double() * gamma.double()
    Wf = Wg.half()
    colsum = Wf.double().sum(1).float()
    colc = (bias.double() + W.double() @ beta.double()).float()
    xs = x16.double()
    mean = xs.mean(1)
    rstd = 1 / torch.sqrt(((xs - mean[:, None]) ** 2).mean(1) + 1e-5)
    rs = torch.zeros(M + 256, 2)
    rs[:M, 0], rs[:M, 1] = rstd.float(), (rstd * mean).float()
    xd, rsd, Wd, sd, cd = _half_slots(x16).to(gpu), rs.to(gpu), Wf.to(gpu), colsum.to(gpu), colc.to(gpu)
    out = torch.full((M, N), float("nan"), dtype=torch.bfloat16, device=gpu)
    N_.check(N_.lib().mi_op_gemm_ln(xd.data_ptr(), 2 * K, rsd.data_ptr(), Wd.data_ptr(), sd.data_ptr(), cd.data_ptr(),
                                    out.data_ptr(), M, N, K, gelu, _stream()), "gemm_ln")
    torch.cuda.synchronize()
    ln = torch.nn.functional.layer_norm(xs, (K,), gamma.double(), beta.double(), 1e-5)
    ref = (ln @ W.double().t() + bias.double()).numpy()
    acc_mag = (xs.abs() @ Wf.double().abs().t()).numpy()
    fold_mag = (xs.abs() @ Wg.abs().t()).numpy()
    lip = 1.0
    if gelu:
        ref, lip = probes.quickgelu64(ref), 1.1
    bound = 2.0 ** -8 * np.abs(ref) + lip * rstd.numpy()[:, None] * (2 * K * 2.0 ** -24 * acc_mag + 2.0 ** -11 * fold_mag)
    _bound_check(out.double().cpu().numpy(), ref, bound, f"gemm_ln gelu {gelu} {M}x{N}x{K}")
