"""orbm_llt_solve_dev, the part that needs no device: the numpy restatement of its arithmetic contract (tests/llt_reference.py, what
tests/test_gpu_llt.py compares the device with) against a literal scalar loop, its backward error against Higham's bound, the
failure rule, the ABI surface, and the refusals that come before any device work."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import llt_reference as R
from orb_slam2_e_amd import _lib, bundle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1


@pytest.mark.parametrize("n", [1, 2, 3, 6, 7, 13, 24])
def test_restatement_equals_the_scalar_triple_loop(n):
    for kind in (R.spd, R.block_sparse):
        A, b = kind(n)
        L, x, ok = R.llt_solve(A, b)
        Ls, xs, oks = R.llt_solve_scalar(A, b)
        assert ok == oks == 1
        assert L.tobytes() == Ls.tobytes() and x.tobytes() == xs.tobytes(), (kind.__name__, n)


def test_the_first_product_initialises_the_dot():
    """Where the two orders differ: a[i][j] = -0.0 with L[i][0] L[j][0] = -0.0.  dot = -0.0 gives -0.0 - -0.0 = +0.0; starting from
    0.0 + -0.0 = +0.0 gives -0.0 - 0.0 = -0.0.  The restatement and the scalar loop both hold the contract's +0.0."""
    A = np.array([[4.0, 0.0, 0.0], [-0.0, 9.0, 0.0], [2.0, -0.0, 16.0]])         # L[1][0] = -0.0, L[2][0] = 1: their product is -0.0
    b = np.ones(3)
    L, _, ok = R.llt_solve(A, b)
    Ls, _, _ = R.llt_solve_scalar(A, b)
    assert ok == 1 and np.signbit(L[1, 0]) and L[2, 1] == 0.0 and not np.signbit(L[2, 1])
    assert L.tobytes() == Ls.tobytes()


@pytest.mark.parametrize("n", [1, 6, 65, 197, 390, 780])
def test_backward_error_is_within_highams_bound(n):
    for kind in ("spd", "block"):
        A, b, L, x, ok = R.case(kind, n)
        fact, slv, bound = R.backward_errors(A, b, L, x)
        print("%s n = %d: backward error of L L^T %.3e, of the solve %.3e, bound %.3e" % (kind, n, fact, slv, bound))
        assert ok == 1 and fact <= bound and slv <= bound
        assert not np.triu(L, 1).any()


def test_a_pivot_that_is_not_positive_gives_ok_0_and_x_0():
    A, b = R.spd(12)
    for c in (0, 5, 11):
        for v in (-1.0, np.nan):
            B = A.copy(); B[c, c] = v
            for f in (R.llt_solve, R.llt_solve_scalar):
                _, x, ok = f(B, b)
                assert ok == 0 and x.tobytes() == np.zeros(12).tobytes(), (c, v)
    B = A.copy(); B[3, 3] = 0.0                                # a zero diagonal entry under a positive dot: the pivot is < 0
    assert R.llt_solve(B, b)[2] == 0
    B = A.copy(); B[7, 2] = np.nan                               # a NaN below the diagonal reaches a pivot
    assert R.llt_solve(B, b)[2] == 0 and R.llt_solve_scalar(B, b)[2] == 0
    B = A.copy(); B[2, 7] = np.nan                               # the upper triangle is never read
    assert R.llt_solve(B, b)[2] == 1


def test_entry_points_are_declared_exported_and_bound():
    protos = _lib.prototypes()
    vp, i = C.c_void_p, C.c_int
    assert protos["orbm_llt_tile"] == (i, [])
    assert protos["orbm_llt_solve_dev"] == (i, [i, vp, vp, vp, vp, vp])
    assert protos["orbm_debug_last_llt_launches"] == (i, [])
    assert protos["orbm_global_bundle_adjustment"] == protos["orbm_bundle_adjustment"] == (i, [vp] * 5)
    assert protos["orbm_global_ba_plan"] == protos["orbm_ba_plan"] == (i, [vp] * 8)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.build()]).decode()
    for fn in ("orbm_llt_tile", "orbm_llt_solve_dev", "orbm_debug_last_llt_launches", "orbm_global_bundle_adjustment", "orbm_global_ba_plan"):
        assert f" T {fn}\n" in out, fn
        assert callable(getattr(_lib.lib(), fn))
    assert _lib.lib().orbx_abi_version() == 136
    assert bundle.llt_tile() in (32, 48, 64)
    for f in (bundle.run_global, bundle.plan_global, bundle.global_bundle_adjustment, bundle.llt_solve_device):
        assert callable(f)


def test_refusals_come_before_any_device_work():
    """n outside 1 .. 3,072 and every NULL pointer: ORBX_ERR_ARG -- on a machine without a device too, where anything later would
    answer ORBX_ERR_NO_DEVICE, and with pointers that no device could read."""
    L = _lib.lib()
    p = 4096                                                     # never dereferenced: the refusal comes first
    for n in (0, -1, 3073, 1 << 30):
        assert L.orbm_llt_solve_dev(n, p, p, p, p, None) == ERR_ARG, n
    assert b"3,072" in L.orbx_last_error()
    for k in range(4):
        args = [p] * 4
        args[k] = None
        assert L.orbm_llt_solve_dev(64, *args, None) == ERR_ARG, k
    assert b"null" in L.orbx_last_error()


def test_the_solver_unit_leases_nothing():
    src = open(os.path.join(ROOT, "orb_slam2_e_amd", "csrc", "orbm_llt.hip")).read()
    assert "StagedCall" not in src and "WorkspaceLease" not in src and "hipMalloc" not in src and "Synchronize" not in src
    assert "__builtin_amdgcn_mfma" not in src and not re.search(r"atomicAdd|atomic_fetch_add|unsafeAtomic", src)
    assert "orbm_llt.hip" in open(os.path.join(ROOT, "orb_slam2_e_amd", "csrc", "Makefile")).read()
