"""orbm_llt_solve_dev on the MI355X against the numpy restatement of its arithmetic contract (tests/llt_reference.py): L's lower
triangle, x and ok EQUAL, value by value (and byte by byte on the block-sparse input, where an exact zero's sign tells `0.0 + p`
from `p`), at every tile-relative size; the same bytes whatever the scratch held; planted failures; n = 3,072 once."""
import numpy as np
import pytest
import torch

import llt_reference as R
from orb_slam2_e_amd import _lib, bundle

pytestmark = pytest.mark.gpu
T = bundle.llt_tile()
SIZES = R.sizes(T)
DEV = "cuda:0"


def column_major(full):
    """the device image of an [n][n] array of (row, column) entries: element [j][i] is entry (i, j)"""
    return torch.from_numpy(np.ascontiguousarray(full.T)).to(DEV)


def solve(A, b, upper=None, x0=None, bufs=None):
    """One call on fresh buffers (or on bufs = (S, x, ok) as they are).  upper: what the strict upper triangle holds before the call
    (an [n][n] array whose strict upper triangle is used; default zeros).  Returns (L with zeros above the diagonal, x, ok, bufs)."""
    n = len(b)
    if bufs is None:
        full = np.tril(A) if upper is None else np.where(np.triu(np.ones((n, n), bool), 1), upper, np.tril(A))
        S = column_major(full)
        x = torch.from_numpy(np.zeros(n) if x0 is None else x0.copy()).to(DEV)
        ok = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    else:
        S, x, ok = bufs
        lower = torch.from_numpy(np.array(np.tril(A).T, order="C")).to(DEV)
        mask = torch.triu(torch.ones((n, n), dtype=torch.bool, device=DEV))         # [j][i], i >= j: the lower triangle's image
        S.copy_(torch.where(mask, lower, S))
    bd = torch.from_numpy(np.array(b)).to(DEV)
    bundle.llt_solve_device(S, bd, x, ok)
    torch.cuda.synchronize()
    return np.tril(S.cpu().numpy().T), x.cpu().numpy(), int(ok.item()), (S, x, ok)


@pytest.mark.parametrize("n", SIZES)
def test_factor_solution_and_flag_equal_the_restatement(n):
    for kind in ("spd", "block"):
        A, b, L, x, ok = R.case(kind, n)
        gL, gx, gok, _ = solve(A, b)
        assert gok == ok == 1, (kind, n)
        assert (gL == L).all() and (gx == x).all(), (kind, n, int((gL != L).sum()), int((gx != x).sum()))
        if kind == "block":
            assert gL.tobytes() == L.tobytes() and gx.tobytes() == x.tobytes(), n
            assert (L[np.tril_indices(n)] == 0).any() or n < 30                     # the exact zeros are there
    assert _lib.lib().orbm_debug_last_llt_launches() == 4 * ((n + T - 1) // T) - 1


@pytest.mark.parametrize("n", [T - 1, 2 * T + 1, 390])
def test_scratch_contents_change_nothing(n):
    A, b, L, x, _ = R.case("block", n)
    ref = (L.tobytes(), x.tobytes())
    nan = np.full((n, n), np.nan)
    ff = np.frombuffer(b"\xff" * (8 * n * n), np.float64).reshape(n, n)
    for name, upper, x0 in (("NaN", nan, np.full(n, np.nan)), ("0xFF", ff, ff[0].copy())):
        gL, gx, gok, bufs = solve(A, b, upper=upper, x0=x0)
        assert gok == 1 and (gL.tobytes(), gx.tobytes()) == ref, (name, n)
    # a second call on the SAME buffers: the upper triangle and x hold the first call's leftovers
    gL, gx, gok, bufs = solve(A, b, bufs=bufs)
    assert gok == 1 and (gL.tobytes(), gx.tobytes()) == ref, n
    # and another system's leftovers
    A2, b2, L2, x2, _ = R.case("spd", n)
    gL, gx, gok, bufs = solve(A2, b2, bufs=bufs)
    assert gok == 1 and (gL == L2).all() and (gx == x2).all(), n


def _failures(n):
    """(name, matrix): one diagonal entry lowered far enough that its pivot is not > 0, or one NaN below the diagonal"""
    A, _, _, _, _ = R.case("spd", n)
    out = []
    for c in sorted({0, T - 1, T, n - 1}):
        if c < n:
            B = A.copy(); B[c, c] = -1.0
            out.append((f"column {c}", B))
    B = A.copy(); B[n - 1, n // 2] = np.nan
    out.append(("NaN", B))
    return out


@pytest.mark.parametrize("n", [5, T + 1, 3 * T + 5])
def test_a_pivot_that_is_not_positive_gives_ok_0_and_x_0(n):
    A, b, L, x, _ = R.case("spd", n)
    bufs = None
    for name, B in _failures(n):
        rL, rx, rok = R.llt_solve(B, b)
        assert rok == 0 and not rx.any(), name
        _, gx, gok, bufs = solve(B, b, x0=np.full(n, 7.5)) if bufs is None else solve(B, b, bufs=bufs)
        assert gok == 0 and gx.tobytes() == np.zeros(n).tobytes(), (name, n)
        # a good call on the same buffers is exact again
        gL, gx, gok, bufs = solve(A, b, bufs=bufs)
        assert gok == 1 and (gL == L).all() and (gx == x).all(), (name, n)


def test_the_largest_system_once():
    n = 3072
    A, b = R.spd(n)
    gL, gx, gok, _ = solve(A, b)
    fact, slv, bound = R.backward_errors(A, b, gL, gx)
    launches = _lib.lib().orbm_debug_last_llt_launches()
    print("n = 3,072: backward error of L L^T %.3e, of the solve %.3e, bound %.3e, launches %d" % (fact, slv, bound, launches))
    assert gok == 1 and fact <= bound and slv <= bound
    assert launches == 4 * ((n + T - 1) // T) - 1
