"""CPU: the distinct top-k walk as tests/collapse_ref.py states it, the mi_rank_collapse entry
points (exported, arguments validated before any HIP call, workspace size), and the precondition
that makes the GPU test on the real rows (test_gpu_rank_collapse.py) neither vacuous nor flaky."""
import ctypes
import re

import numpy as np
import pytest

from collapse_ref import collapse_ref, min_margin
from conftest import golden

F32, BF16, F16 = 0, 1, 2


def _plane(degrees, D=8):
    """Unit rows at the given angles in the plane of the first two coordinates."""
    a = np.deg2rad(np.asarray(degrees, np.float64))
    rows = np.zeros((len(a), D))
    rows[:, 0], rows[:, 1] = np.cos(a), np.sin(a)
    return rows


THETA25 = float(np.cos(np.deg2rad(25.0)))


def test_ref_chain_is_not_transitive():
    rows = _plane([0, 20, 40])          # a~b, b~c, a!~c
    hit, count, slot = collapse_ref(rows, [0, 1, 2], 3, THETA25)
    assert hit.tolist() == [0, 2, -1] and count.tolist() == [2, 1, 0] and slot.tolist() == [0, 0, 1]
    # b first: it absorbs both
    hit, count, slot = collapse_ref(rows, [1, 0, 2], 3, THETA25)
    assert hit.tolist() == [1, -1, -1] and count.tolist() == [3, 0, 0] and slot.tolist() == [0, 0, 0]
    # c, b, a: the mirror image of the first order
    hit, count, slot = collapse_ref(rows, [2, 1, 0], 3, THETA25)
    assert hit.tolist() == [2, 0, -1] and count.tolist() == [2, 1, 0] and slot.tolist() == [0, 0, 1]


def test_ref_lower_slot_wins():
    rows = _plane([0, 40, 20])          # hits a (slot 0) and c' = 40 deg (slot 1); 20 deg is similar to both
    hit, count, slot = collapse_ref(rows, [0, 1, 2], 3, THETA25)
    assert hit.tolist() == [0, 1, -1] and count.tolist() == [2, 1, 0] and slot.tolist() == [0, 1, 0]


def test_ref_beyond_kth_hit():
    rows = _plane([0, 90, 180, 5, 270, 95])
    hit, count, slot = collapse_ref(rows, [0, 1, 2, 3, 4, 5], 2, THETA25)
    # 180 and 270 deg are distinct frames beyond the 2nd hit; 5 and 95 deg are still counted
    assert hit.tolist() == [0, 1] and count.tolist() == [2, 2] and slot.tolist() == [0, 1, -1, 0, -1, 1]


def test_ref_empty_slots_and_zero_rows():
    rows = np.vstack([_plane([0, 3]), np.zeros((2, 8)), _plane([6])])
    hit, count, slot = collapse_ref(rows, [-1, 0, -1, 1, 99], 2, 0.9)
    assert hit.tolist() == [0, -1] and count.tolist() == [2, 0] and slot.tolist() == [-1, 0, -1, 0, -1]
    # zero rows (rows 2, 3): similar to nothing, not even to each other; one hit each
    hit, count, slot = collapse_ref(rows, [2, 3, 0, 1, 4], 4, 0.9)
    assert hit.tolist() == [2, 3, 0, -1] and count.tolist() == [1, 1, 3, 0] and slot.tolist() == [0, 1, 2, 2, 2]
    hit, count, slot = collapse_ref(rows, [2, 3, 0], 3, -2.0)
    assert hit.tolist() == [2, 3, 0] and count.tolist() == [1, 1, 1]
    hit, count, slot = collapse_ref(rows, [-1, -1], 1, 0.9)
    assert hit.tolist() == [-1] and count.tolist() == [0] and slot.tolist() == [-1, -1]
    assert min_margin(rows, [2, 3], 0.9) == float("inf") and min_margin(_plane([0, 60]), [0, 1], 0.9) == pytest.approx(0.4)


# ------------------------------------------------------------------ the C entry points
def _lib():
    from miclip import _native
    return _native.lib()


def test_symbols_exported():
    from miclip import _native
    L = _lib()
    out = __import__("os").popen(f"nm -D --defined-only {_native.LIB_PATH}").read()
    for name in ("mi_rank_collapse", "mi_rank_collapse_workspace_bytes"):
        assert name in _native.EXPORTS and hasattr(L, name)
        assert re.search(rf"\bT {name}$", out, re.M), f"{name} not exported"
    assert L.mi_abi_version() == 7


def _call(L, N=10, dt=F32, N2=0, dt2=0, D=512, Q=1, P=30, k=10, theta=0.9, ws=0, c2=None):
    return L.mi_rank_collapse(None, N, dt, c2, N2, dt2, D, 0, None, None, Q, P, k, theta, None, None, None, None,
                              None, ws, None)


def test_argument_errors_without_gpu():
    L = _lib()
    for P in (0, 65):
        assert _call(L, P=P, k=1) == -3 and b"P must be in [1, 64]" in L.mi_last_error()
    for k in (0, 65):
        assert _call(L, P=64, k=k) == -3 and b"k must be in [1, 64]" in L.mi_last_error()
    assert _call(L, P=10, k=11) == -1 and b"exceeds the pool" in L.mi_last_error()
    assert _call(L, D=500) == -3 and b"multiple of 32" in L.mi_last_error()
    assert _call(L, D=0) == -3 and _call(L, D=1056) == -3 and b"1024" in L.mi_last_error()
    assert _call(L, dt=3) == -1 and b"bad corpus dtype" in L.mi_last_error()
    assert _call(L, N2=5, dt2=3) == -1 and b"bad corpus2 dtype" in L.mi_last_error()
    for kw in (dict(N=-1), dict(N2=-1), dict(Q=-1)):
        assert _call(L, **kw) == -1 and b"negative size" in L.mi_last_error()
    assert _call(L, theta=float("nan")) == -1 and b"NaN" in L.mi_last_error()
    need = L.mi_rank_collapse_workspace_bytes(1, 30, 512)
    assert need > 0
    assert _call(L, ws=need - 1) == -1 and b"workspace too small" in L.mi_last_error()
    buf = ctypes.create_string_buffer(need)
    rc = L.mi_rank_collapse(None, 10, F32, None, 0, 0, 512, 0, None, None, 1, 30, 10, 0.9, None, None, None, None,
                            ctypes.cast(buf, ctypes.c_void_p), need, None)
    assert rc == -1 and b"null pointer" in L.mi_last_error()
    assert _call(L, D=1024, P=64, k=64, dt=BF16, N2=3, dt2=F16) == -1 and b"workspace" in L.mi_last_error()
    assert _call(L, Q=0) == 0                                                    # nothing to do


def test_workspace_monotone():
    f = _lib().mi_rank_collapse_workspace_bytes
    assert f(4, 0, 512) == 0 and f(4, 65, 512) == 0 and f(-1, 10, 512) == 0
    Qs, Ps, Ds = [0, 1, 2, 31, 32, 33, 1000, 100_000], [1, 2, 10, 31, 32, 33, 60, 64], [32, 64, 512, 768, 1024]
    for P in Ps:
        for D in Ds:
            v = [f(Q, P, D) for Q in Qs]
            assert all(a <= b for a, b in zip(v, v[1:])), (P, D, v)
    for Q in Qs:
        for D in Ds:
            v = [f(Q, P, D) for P in Ps]
            assert all(a <= b for a, b in zip(v, v[1:])), (Q, D, v)
    for Q in Qs:
        for P in Ps:
            v = [f(Q, P, D) for D in Ds]
            assert all(a <= b for a, b in zip(v, v[1:])), (Q, P, v)
    assert f(1, 1, 32) >= 8 and f(32, 64, 512) >= 32 * 64 * 8   # one 64-bit conflict mask per candidate


# ------------------------------------------------------------------ the real rows
def test_fixture_precondition():
    """Every row of the fixture corpus as a query: no pool (30 or 64 best by float64 order) holds
    a pair whose cosine is within 1e-4 of a tested threshold (the kernel's f32 bound at D = 512 is
    6.1e-5), and collapsing at 0.9 changes at least 200 of the 387 top-10 lists."""
    rows = golden("rank_video_test_4.npz")["corpus"].astype(np.float64)
    unit = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    order = np.argsort(-(unit @ unit.T), axis=1, kind="stable")
    for theta in (0.85, 0.9, 0.95):
        worst = min(min_margin(rows, order[q, :64], theta) for q in range(rows.shape[0]))
        print(f"theta {theta}: smallest |cos - theta| over all pools {worst:.3e}")
        assert worst >= 1e-4, (theta, worst)   # pools of 30 are prefixes of the pools of 64
    for P in (30, 64):
        changed = sum(collapse_ref(rows, order[q, :P], 10, 0.9)[0].tolist() != order[q, :10].tolist()
                      for q in range(rows.shape[0]))
        print(f"P = {P}: {changed} of {rows.shape[0]} top-10 lists change at 0.9")
        assert changed >= 200, (P, changed)
