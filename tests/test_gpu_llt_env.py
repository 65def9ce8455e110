"""orbm_llt_env_solve_dev on the MI355X.  Its yardstick is exact: on a matrix that is zero outside the tile envelope
the live tiles of L, x and ok EQUAL the dense orbm_llt_solve_dev's, device against device, as numbers (np.array_equal; the sign of a
zero is the one thing skipping a zero tile may change, tests/test_cpu_llt_env.py shows where) -- for every named envelope at every
tile-relative size, whatever the scratch held; the bytes of the numpy restatement of the dense contract on inputs without exact
zeros in live tiles; beyond the dense solver's 3,072 rows two independent halves against the dense solver on each, and a coupled
system against Higham's bound; planted failures."""
import numpy as np
import pytest
import torch

import llt_env_reference as E
import llt_reference as R
from orb_slam2_e_amd import _lib, bundle

pytestmark = pytest.mark.gpu
T = bundle.llt_tile()
DEV = "cuda:0"
SIZES = [1, 63, 64, 65, 129, 197, 390, 780]


def dense_solve(A, b):
    """orbm_llt_solve_dev on fresh buffers: (L with zeros above the diagonal, x, ok)"""
    n = len(b)
    S = torch.from_numpy(np.ascontiguousarray(np.tril(A).T)).to(DEV)
    x = torch.zeros(n, dtype=torch.float64, device=DEV)
    ok = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    bundle.llt_solve_device(S, torch.from_numpy(np.array(b)).to(DEV), x, ok)
    torch.cuda.synchronize()
    return np.tril(S.cpu().numpy().T), x.cpu().numpy(), int(ok.item())


def env_solve(A, b, first, scratch=None, bufs=None):
    """One call.  scratch: the float64 value W and x hold before it on fresh buffers (None: zeros); bufs = (tiles, W, x, ok) of an
    earlier call: used as they are, with the new system's tiles copied in.  What the solver never reads (rows beyond n, the upper
    part of a diagonal tile) is NaN.  Returns (L [n][n] with zeros where nothing is stored, x, ok, launches, plan, bufs)."""
    n = len(b)
    plan = bundle.llt_env_plan(n, first)
    packed = torch.from_numpy(E.pack(np.asarray(A), first, T)).to(DEV)
    if bufs is None:
        tiles = packed
        W = torch.zeros_like(tiles)
        x = torch.zeros(n, dtype=torch.float64, device=DEV)
        if scratch is not None:
            W.copy_(torch.from_numpy(np.full(tuple(W.shape), scratch)).to(DEV))
            x.copy_(torch.from_numpy(np.full(n, scratch)).to(DEV))
        ok = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    else:
        tiles, W, x, ok = bufs
        tiles.copy_(packed)
    bundle.llt_env_solve_device(first, torch.from_numpy(plan["device"]).to(DEV), tiles, W, torch.from_numpy(np.array(b)).to(DEV), x, ok)
    torch.cuda.synchronize()
    launches = _lib.lib().orbm_debug_last_llt_launches()
    return E.unpack(tiles.cpu().numpy(), n, first, T), x.cpu().numpy(), int(ok.item()), launches, plan, (tiles, W, x, ok)


FF = float(np.frombuffer(b"\xff" * 8, np.float64)[0])            # a NaN whose every byte is 0xFF


@pytest.mark.parametrize("n", SIZES)
def test_live_tiles_x_and_flag_equal_the_dense_solver_whatever_the_scratch_held(n):
    nt = E.ntiles(n, T)
    for pattern in E.PATTERNS:
        first = E.envelope(pattern, nt)
        live = E.live_mask(n, first, T)
        sys = [E.masked_spd(n, first, T, seed) for seed in (0, 1)]
        want = [dense_solve(A, b) for A, b in sys]
        for L, _, ok in want:
            assert ok == 1 and not L[~live].any(), (pattern, n)  # the dense fill stays inside the envelope
        bufs = None
        # fresh NaN scratch, fresh 0xFF scratch, then on the 0xFF call's buffers another system and the first one again
        for name, k, scratch, reuse in (("NaN", 0, np.nan, False), ("0xFF", 0, FF, False), ("another system's leftovers", 1, None, True),
                                        ("its own leftovers", 0, None, True)):
            (A, b), (L, x, ok) = sys[k], want[k]
            gL, gx, gok, launches, plan, bufs = env_solve(A, b, first, scratch=scratch, bufs=bufs if reuse else None)
            assert gok == ok, (pattern, n, name)
            assert np.array_equal(gL[live], L[live]) and np.array_equal(gx, x), (pattern, n, name, int((gL != L).sum()), int((gx != x).sum()))
            assert launches == plan["launches"] <= 4 * nt - 1, (pattern, n)


@pytest.mark.parametrize("n", [s for s in SIZES if s <= 197])
def test_bytes_of_the_dense_restatement_where_no_live_entry_is_zero(n):
    for pattern in E.PATTERNS:
        first = E.envelope(pattern, E.ntiles(n, T))
        live = E.live_mask(n, first, T)
        A, b = E.masked_spd(n, first, T)
        L, x, ok = R.llt_solve(A, b)
        assert ok == 1 and L[live].all() and x.all()             # no exact zero where the two orders could differ in its sign
        gL, gx, gok, _, _, _ = env_solve(A, b, first, scratch=np.nan)
        assert gok == 1 and gL[live].tobytes() == L[live].tobytes() and gx.tobytes() == x.tobytes(), (pattern, n)


def test_two_independent_halves_beyond_the_dense_limit_equal_the_dense_solver_on_each():
    """4,000 rows as two 2,000-row systems.  2,000 is no multiple of T, so the first half is padded with identity rows to the tile
    boundary 2,048, where the second starts: n = 4,048 > 3,072, first[] restarts at tile 32."""
    h, pad = 2000, 2048
    (A0, b0), (A1, b1) = R.spd(h, 3), R.spd(h, 4)
    A0p, b0p = np.eye(pad), np.ones(pad)
    A0p[:h, :h], b0p[:h] = A0, b0
    n = pad + h
    A, b = np.zeros((n, n)), np.concatenate([b0p, b1])
    A[:pad, :pad], A[pad:, pad:] = A0p, A1
    nt = E.ntiles(n, T)
    first = np.where(np.arange(nt) < pad // T, 0, pad // T).astype(np.int32)
    live = E.live_mask(n, first, T)
    gL, gx, gok, launches, plan, _ = env_solve(A, b, first, scratch=np.nan)
    assert gok == 1 and launches == plan["launches"] <= 4 * nt - 1
    for lo, hi, (Ah, bh) in ((0, pad, (A0p, b0p)), (pad, n, (A1, b1))):
        L, x, ok = dense_solve(Ah, bh)
        assert ok == 1
        m = live[lo:hi, lo:hi]
        assert np.array_equal(gL[lo:hi, lo:hi][m], L[m]) and np.array_equal(gx[lo:hi], x), lo


def test_a_coupled_system_beyond_the_dense_limit_is_within_highams_bound():
    """n = 4,160 = 65 tiles: a band three tiles wide whose last row tile is full (a loop closure's rows).  Random entries in the live
    tiles, positive definite by strict diagonal dominance (B B^T of this size would cost more than the solve)."""
    n = 4160
    nt = E.ntiles(n, T)
    first = np.maximum(np.arange(nt) - 3, 0).astype(np.int32); first[-1] = 0
    rng = np.random.default_rng(4160)
    m = E.live_mask(n, first, T)
    A = np.where(m, rng.standard_normal((n, n)), 0.0)
    A = np.tril(A, -1) + np.tril(A, -1).T
    np.fill_diagonal(A, np.abs(A).sum(1) + 1.0)
    b = rng.standard_normal(n)
    gL, gx, gok, launches, plan, _ = env_solve(A, b, first, scratch=np.nan)
    fact, slv, bound = R.backward_errors(A, b, gL, gx)
    print("n = 4,160, %d live tiles: backward error of L L^T %.3e, of the solve %.3e, bound %.3e, launches %d"
          % (plan["live_tiles"], fact, slv, bound, launches))
    assert gok == 1 and fact <= bound and slv <= bound
    assert launches == plan["launches"] <= 4 * nt - 1


def test_a_pivot_that_is_not_positive_gives_ok_0_and_x_0():
    """ordinary inputs the contract handles: a diagonal entry lowered at column 0, T - 1, T, in the mid-matrix tile whose row starts
    at itself (tile 2 of 0 0 2 1), at n - 1; a NaN inside a live tile.  A good call on the same buffers is exact again."""
    n = 3 * T + 5
    first = E.envelope("non_monotone", E.ntiles(n, T))
    assert list(first) == [0, 0, 2, 1]
    live = E.live_mask(n, first, T)
    A, b = E.masked_spd(n, first, T)
    L, x, _ = dense_solve(A, b)
    cases = []
    for c in (0, T - 1, T, 2 * T + 3, n - 1):
        B = A.copy(); B[c, c] = -1.0
        cases.append((f"column {c}", B))
    B = A.copy(); B[3 * T + 1, T + 7] = np.nan
    cases.append(("NaN", B))
    bufs = None
    for name, B in cases:
        assert dense_solve(B, b)[2] == 0, name
        _, gx, gok, _, _, bufs = env_solve(B, b, first, scratch=7.5, bufs=bufs)
        assert gok == 0 and gx.tobytes() == np.zeros(n).tobytes(), name
        gL, gx, gok, _, _, bufs = env_solve(A, b, first, bufs=bufs)
        assert gok == 1 and np.array_equal(gL[live], L[live]) and np.array_equal(gx, x), name
