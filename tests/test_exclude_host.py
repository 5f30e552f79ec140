"""CPU: the exclusion-mask pass and the refill rounds as tests/exclude_ref.py states them, the
mi_rank_exclude entry points (exported, arguments validated before any HIP call, workspace size),
and the preconditions that make the GPU tests on the real rows (test_gpu_rank_exclude.py) neither
vacuous nor flaky."""
import ctypes
import functools
import re

import numpy as np
import pytest

from collapse_ref import collapse_ref, cosines
from conftest import golden
from exclude_ref import exclude_ref, fill_ref, rounds_ref

F32, BF16, F16 = 0, 1, 2
SETTINGS = [(0.9, 10, 10), (0.9, 20, 20), (0.85, 16, 16)]   # (theta, k, pool)


def _plane(degrees, D=8):
    """Unit rows at the given angles in the plane of the first two coordinates."""
    a = np.deg2rad(np.asarray(degrees, np.float64))
    rows = np.zeros((len(a), D))
    rows[:, 0], rows[:, 1] = np.cos(a), np.sin(a)
    return rows


THETA25 = float(np.cos(np.deg2rad(25.0)))


# ------------------------------------------------------------------ the reference, by hand
def test_ref_zero_norm_hit_removes_its_own_row():
    rows = np.vstack([_plane([0, 5]), np.zeros((2, 8)), _plane([90])])
    mask, count = exclude_ref(rows, rows[[2]], [2], 0.9, None)
    assert mask.tolist() == [True, True, False, True, True] and count.tolist() == [1]   # not the other zero row
    mask, count = exclude_ref(rows, rows[[2]], None, 0.9, None)                          # unnamed: removes nothing
    assert mask.all() and count.tolist() == [0]
    mask, count = exclude_ref(rows, rows[[2]], [2], 0.9, [True, True, False, True, True])   # invisible: not counted
    assert mask.tolist() == [True, True, False, True, True] and count.tolist() == [0]
    mask, count = exclude_ref(rows, rows[[2, 0]], [7, -1], 0.9, None)                    # out of range names no row
    assert mask.tolist() == [False, False, True, True, True] and count.tolist() == [0, 2]


def test_ref_lowest_slot_attribution():
    rows = _plane([0, 40, 20, 200])            # 20 deg is similar to both hits
    mask, count = exclude_ref(rows, rows[[0, 1]], [0, 1], THETA25, None)
    assert mask.tolist() == [False, False, False, True] and count.tolist() == [2, 1]
    mask, count = exclude_ref(rows, rows[[1, 0]], [1, 0], THETA25, None)
    assert mask.tolist() == [False, False, False, True] and count.tolist() == [2, 1]
    # similar beats named: row 1 is named by slot 0 (a foreign vector) and similar to slot 1
    mask, count = exclude_ref(rows, rows[[3, 1]], [1, 1], THETA25, None)
    assert mask.tolist() == [True, False, False, False] and count.tolist() == [1, 2]
    # theta = -2: every valid visible row, all to slot 0
    mask, count = exclude_ref(rows, rows[[3, 1]], None, -2.0, [True, True, False, True])
    assert not mask.any() and count.tolist() == [3, 0]


def test_ref_nan_rows_untouched():
    rows = _plane([0, 3, 6, 100])
    rows[1, 4] = np.nan
    rows[3, 2] = np.inf
    mask, count = exclude_ref(rows, rows[[0]], [0], -2.0, None)
    assert mask.tolist() == [False, True, False, True] and count.tolist() == [2]
    mask, count = exclude_ref(rows, rows[[1]], [1], -2.0, None)     # a NaN hit: only the row it names
    assert mask.tolist() == [True, False, True, True] and count.tolist() == [1]


def test_ref_chaining_two_blocks_is_one_statement():
    rng = np.random.default_rng(3)
    centres = rng.standard_normal((60, 64))
    rows = np.repeat(centres, 5, axis=0) + rng.standard_normal((300, 64)) * 0.05
    rows[17] = 0.0
    order = rng.permutation(300)
    rows = rows[order]
    hits = rng.permutation(300)[:40]
    vis = rng.random(300) < 0.8
    mask, count = exclude_ref(rows, rows[hits], hits, 0.9, vis)
    m1, c1 = exclude_ref(rows, rows[hits[:32]], hits[:32], 0.9, vis)
    m2, c2 = exclude_ref(rows, rows[hits[32:]], hits[32:], 0.9, m1)
    assert (m2 == mask).all() and np.concatenate([c1, c2]).tolist() == count.tolist()
    assert count.sum() == (vis & ~mask).sum() and (count > 1).sum() >= 10 and (c2 > 0).any()


# ------------------------------------------------------------------ the C entry points
def _lib():
    from miclip import _native
    return _native.lib()


def test_symbols_exported():
    from miclip import _native
    L = _lib()
    out = __import__("os").popen(f"nm -D --defined-only {_native.LIB_PATH}").read()
    for name in ("mi_rank_exclude", "mi_rank_exclude_workspace_bytes"):
        assert name in _native.EXPORTS and hasattr(L, name)
        assert re.search(rf"\bT {name}$", out, re.M), f"{name} not exported"
    assert L.mi_abi_version() == 7


ONE = ctypes.c_void_p(64)   # a non-null pointer that no argument check dereferences


def _call(L, corpus=ONE, N=10, D=512, dt=F32, hits=ONE, H=5, theta=0.9, out=ONE, ws=None, nbytes=0):
    return L.mi_rank_exclude(corpus, N, D, dt, hits, None, H, 0, theta, None, out, None, ws, nbytes, None)


def test_argument_errors_without_gpu():
    L = _lib()
    for kw in (dict(corpus=None), dict(hits=None), dict(out=None)):
        assert _call(L, **kw) == -1 and b"null pointer" in L.mi_last_error()
    for H in (0, 33, -1):
        assert _call(L, H=H) == -3 and b"H must be in [1, 32]" in L.mi_last_error()
    assert _call(L, D=500) == -3 and b"multiple of 32" in L.mi_last_error()
    assert _call(L, D=0) == -3 and _call(L, D=1056) == -3 and b"1024" in L.mi_last_error()
    assert _call(L, dt=3) == -1 and b"bad corpus dtype" in L.mi_last_error()
    assert _call(L, N=-1) == -1 and b"negative size" in L.mi_last_error()
    assert _call(L, theta=float("nan")) == -1 and b"NaN" in L.mi_last_error()
    need = L.mi_rank_exclude_workspace_bytes(10, 5)
    assert need >= 128
    assert _call(L) == -1 and b"workspace too small" in L.mi_last_error()
    buf = ctypes.create_string_buffer(need)
    assert _call(L, ws=ctypes.cast(buf, ctypes.c_void_p), nbytes=need - 1) == -1 and \
        b"workspace too small" in L.mi_last_error()
    assert _call(L, N=0) == 0                                                    # nothing to do


def test_workspace_one_line_per_workgroup():
    f = _lib().mi_rank_exclude_workspace_bytes
    assert f(-1, 5) == 0 and f(10, 0) == 0 and f(10, 33) == 0
    Ns = [0, 1, 383, 384, 385, 20_011, 196_608, 196_609, 1_000_000, 12_582_912, 12_582_913, 100_000_000]
    v = [f(n, 32) for n in Ns]
    assert all(a <= b for a, b in zip(v, v[1:])), v
    for n, b in zip(Ns, v):
        # rank_pass.hpp row_split: row ranges are multiples of 384, at most 512 workgroups until a
        # workgroup's rows would pass 24576 (64 tiles per wave)
        chunks = max(min((n + 383) // 384, 512), (n + 24575) // 24576, 1)
        rpw = ((max(n, 1) + chunks - 1) // chunks + 383) // 384 * 384
        nwg = (max(n, 1) + rpw - 1) // rpw
        assert rpw <= 24576 and b >= nwg * 32 * 4, (n, b, nwg)
        assert f(n, 1) == b                                                     # a line holds all 32 slots


# ------------------------------------------------------------------ the real rows
@functools.lru_cache(maxsize=None)
def _real():
    rows = golden("rank_video_test_4.npz")["corpus"].astype(np.float64)
    cos, valid = cosines(rows)
    assert valid.all()
    unit = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    order = np.argsort(-(unit @ unit.T), axis=1, kind="stable")
    return rows, cos, order


@pytest.mark.parametrize("theta,k,pool", SETTINGS)
def test_rounds_equal_the_full_walk(theta, k, pool):
    """Every row of the fixture corpus as a query: the round loop returns the hits and counts of
    the collapse walk over the full ranking; no pair of rows has a cosine within 1e-4 of the
    threshold (the kernel's f32 bound at D = 512 is 6.1e-5); at least 100 queries refill."""
    rows, cos, order = _real()
    n = rows.shape[0]
    iu = np.triu_indices(n, 1)
    worst = float(np.abs(cos[iu] - theta).min())
    print(f"theta {theta}: smallest |cos - theta| over all row pairs {worst:.3e}")
    assert worst >= 1e-4, (theta, worst)
    multi = 0
    for q in range(n):
        hit, count, rounds = rounds_ref(rows, order[q], k, theta, pool)
        want_hit, want_count = fill_ref(rows, order[q], k, theta)
        assert hit.tolist() == want_hit.tolist() and count.tolist() == want_count.tolist(), q
        multi += rounds >= 2
    print(f"theta {theta} k {k} pool {pool}: {multi} of {n} queries need a second round")
    assert multi >= 100, multi


def test_default_pool_fills_in_one_round():
    """Pool 30, k = 10, theta 0.9: no query under-fills, so the filled hits are the un-filled."""
    rows, cos, order = _real()
    under = 0
    for q in range(rows.shape[0]):
        hit = collapse_ref(rows, order[q, :30], 10, 0.9)[0]
        under += (hit < 0).any()
        assert hit.tolist() == fill_ref(rows, order[q], 10, 0.9)[0].tolist()
        assert rounds_ref(rows, order[q], 10, 0.9, 30)[2] == 1
    assert under == 0
