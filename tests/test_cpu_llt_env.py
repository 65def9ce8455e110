"""orbm_llt_env_solve_dev, the part that needs no device: the theorem the envelope solver rests on -- the restatement
of its contract (tests/llt_env_reference.py), which never touches an entry outside a live tile, gives the DENSE contract's L and x
(tests/llt_reference.py) as numbers -- for small tile edges; orbm_llt_env_plan against lists built in numpy; the refusals, which
come before any device work and leave the outputs alone; the ABI surface."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import llt_env_reference as E
import llt_reference as R
from orb_slam2_e_amd import _lib, bundle

ERR_ARG, ERR_UNSUPPORTED = -1, -5
T64 = 64


def sizes(T):
    """n <= T, n not a multiple of T, several tiles, up to 96 rows at every tile edge (48 tiles of 2)"""
    return sorted({1, T - 1, T, T + 1, 3 * T, 5 * T + 1, min(95, 11 * T + T // 2), 96})


@pytest.mark.parametrize("pattern", E.PATTERNS)
@pytest.mark.parametrize("T", [2, 3, 8])
def test_restatement_on_live_tiles_equals_the_dense_contract(T, pattern):
    """"Equal" is np.array_equal: the sign of a zero is the one thing skipping a zero tile may change."""
    for n in sizes(T):
        for seed in (0, 1):
            first = E.envelope(pattern, E.ntiles(n, T), seed)
            A, b = E.masked_spd(n, first, T, seed)
            L, x, ok = R.llt_solve(A, b)
            eL, ex, eok = E.env_solve(A, b, first, T)            # asserts itself that nothing outside a live tile was written
            live = E.live_mask(n, first, T)
            assert ok == eok == 1, (T, pattern, n)
            assert not L[~live].any()                            # fill stays inside the tile envelope
            assert np.isnan(eL[~live]).all()                     # and the restatement has nothing there
            assert np.array_equal(eL[live], L[live]) and np.array_equal(ex, x), (T, pattern, n, seed)


def test_every_named_envelope_is_what_its_name_says():
    nt = 9
    f = {p: E.envelope(p, nt) for p in E.PATTERNS}
    assert not f["full"].any() and (f["block_diagonal"] == np.arange(nt)).all()
    assert (f["band"][1:] == np.arange(nt - 1)).all() and f["arrow"][-1] == 0 and (f["arrow"][:-1] == f["band"][:-1]).all()
    assert (np.diff(f["non_monotone"]) < 0).any() and (f["non_monotone"] == np.arange(nt)).any()
    for p in E.PATTERNS:
        assert ((0 <= f[p]) & (f[p] <= np.arange(nt))).all()


def test_zero_signs_are_the_only_difference_and_they_do_occur():
    """Why equality is of numbers and not of bytes.  Entry (3, 2), a = -0.0: the dense dot is the skipped panel's +0.0 plus the live
    product -0.5 * 0.0 = -0.0, that is +0.0, and -0.0 - +0.0 = -0.0; on the envelope the live product STARTS the dot, and
    -0.0 - -0.0 = +0.0."""
    T, n = 1, 4
    first = np.array([0, 0, 1, 1], np.int32)
    A = np.diag([4.0, 9.0, 16.0, 25.0])
    A[3, 1] = A[1, 3] = -1.5
    A[3, 2] = A[2, 3] = -0.0
    b = np.ones(n)
    L, x, _ = R.llt_solve(A, b)
    eL, ex, _ = E.env_solve(A, b, first, T)
    live = E.live_mask(n, first, T)
    assert np.array_equal(eL[live], L[live]) and np.array_equal(ex, x)
    assert L[3, 1] == -0.5 and L[3, 2] == 0.0 and np.signbit(L[3, 2]) and not np.signbit(eL[3, 2])


def test_a_pivot_that_is_not_positive_gives_ok_0_and_x_0():
    T, n = 3, 14
    first = E.envelope("non_monotone", E.ntiles(n, T))
    A, b = E.masked_spd(n, first, T)
    for c in (0, T - 1, T, 2 * T, n - 1):                       # 2 T: a diagonal tile whose row starts at itself
        for v in (-1.0, np.nan):
            B = A.copy(); B[c, c] = v
            _, x, ok = E.env_solve(B, b, first, T)
            assert ok == 0 and x.tobytes() == np.zeros(n).tobytes() and R.llt_solve(B, b)[2] == 0, (c, v)
    B = A.copy(); B[4, 1] = np.nan                               # inside live tile (1, 0)
    assert E.env_solve(B, b, first, T)[2] == 0


def _envelope_with(nt, live):
    """first[nt] with exactly `live` live tiles: the block diagonal, its last rows widened as far as it takes"""
    first = np.arange(nt, dtype=np.int32)
    need = live - nt
    for r in range(nt - 1, -1, -1):
        take = min(r, need)
        first[r] -= take
        need -= take
    assert need == 0
    return first


def _c_plan(n, first, sentinel=-7):
    """orbm_llt_env_plan's outputs in sentinel-filled arrays, and its return code"""
    nt = E.ntiles(max(n, 1), T64)
    first = np.ascontiguousarray(first, np.int32)
    out = {k: np.full(nt + 1, sentinel, np.int32) for k in ("off", "row_start", "trail_start")}
    out["rows"] = np.full(9000, sentinel, np.int32)
    out["trail"] = np.full((400000, 2), sentinel, np.int32)
    out["counts"] = np.full(4, sentinel, np.int32)
    p = _lib.ptr
    rc = _lib.lib().orbm_llt_env_plan(n, p(first), p(out["off"]), p(out["row_start"]), p(out["rows"]), p(out["trail_start"]),
                                      p(out["trail"]), p(out["counts"]))
    return rc, out


@pytest.mark.parametrize("pattern", E.PATTERNS)
def test_plan_equals_the_lists_built_in_numpy(pattern):
    assert bundle.llt_tile() == T64
    for n in (1, 63, 64, 65, 129, 197, 390, 780, 3150):
        nt = E.ntiles(n, T64)
        first = E.envelope(pattern, nt)
        want = E.plan(n, first, T64)
        rc, got = _c_plan(n, first)
        assert rc == 0
        for k in ("off", "row_start", "trail_start"):
            assert np.array_equal(got[k], want[k]), (pattern, n, k)
        nr, ntr = len(want["rows"]), len(want["trail"])
        assert np.array_equal(got["rows"][:nr], want["rows"]) and (got["rows"][nr:] == -7).all()
        assert np.array_equal(got["trail"][:ntr], want["trail"]) and (got["trail"][ntr:] == -7).all()
        assert list(got["counts"]) == [want["live_tiles"], nr, ntr, want["launches"]]
        assert want["launches"] <= 4 * nt - 1
        py = bundle.llt_env_plan(n, first)                       # the Python form, sized by a first call with NULL lists
        assert np.array_equal(py["rows"], want["rows"]) and np.array_equal(py["trail"], want["trail"])
        assert py["live_tiles"] == want["live_tiles"] and py["launches"] == want["launches"]
        assert np.array_equal(py["device"], np.concatenate([first, want["off"], want["row_start"], want["rows"]]))


def test_plan_launch_counts_and_empty_panels():
    """the full envelope launches the dense solver's 4 nt - 1; a block diagonal has no row tile at all: every panel's lists are
    empty and only the diagonal tiles and the substitutions are launched"""
    n, nt = 390, 7
    full, blocks = E.plan(n, E.envelope("full", nt), T64), E.plan(n, E.envelope("block_diagonal", nt), T64)
    assert full["launches"] == 4 * nt - 1 and full["live_tiles"] == nt * (nt + 1) // 2
    assert blocks["launches"] == 3 * nt and blocks["live_tiles"] == nt and len(blocks["rows"]) == len(blocks["trail"]) == 0
    assert _c_plan(n, E.envelope("block_diagonal", nt))[1]["counts"][3] == 3 * nt
    nm = E.plan(n, E.envelope("non_monotone", nt), T64)          # 0 0 2 1 2 5 4: panels 2 has rows (3, 4), panel 4 has none ...
    assert [list(nm["rows"][nm["row_start"][K]:nm["row_start"][K + 1]]) for K in range(nt)] == [[1], [3], [3, 4], [4], [6], [6], []]
    assert nm["launches"] == 1 + 2 * nt + 2 * 6


def test_the_largest_system_and_the_tile_cap_are_accepted_at_their_edge():
    nt = 448
    rc, got = _c_plan(28672, E.envelope("band", nt))
    assert rc == 0 and got["counts"][0] == 2 * nt - 1 and got["counts"][3] == 4 * nt - 1
    first = np.zeros(127, np.int32)                              # the full envelope at nt = 127: 8,128 live tiles
    rc, got = _c_plan(127 * 64, first)
    assert rc == 0 and got["counts"][0] == 8128 and got["counts"][2] == sum(m * (m + 1) // 2 for m in range(127))
    first = _envelope_with(200, 8192)
    assert int(np.sum(np.arange(200) - first + 1)) == 8192 and _c_plan(200 * 64, first)[0] == 0


def test_refusals_come_before_any_device_work_and_write_nothing():
    L = _lib.lib()
    ok_first = np.zeros(448, np.int32)
    too_many = _envelope_with(200, 8193)
    assert int(np.sum(np.arange(200) - too_many + 1)) == 8193
    past_r = np.array([0, 2, 0], np.int32)
    negative = np.array([0, -1, 0], np.int32)
    p = 4096                                                     # never dereferenced: the refusal comes first
    for n, first, code, word in ((0, ok_first, ERR_ARG, b"28,672"), (-3, ok_first, ERR_ARG, b"28,672"), (28673, np.arange(449, dtype=np.int32), ERR_ARG, b"28,672"),
                                 (200 * 64, too_many, ERR_UNSUPPORTED, b"8,192"), (150, past_r, ERR_ARG, b"first"), (150, negative, ERR_ARG, b"first")):
        rc, got = _c_plan(n, first)
        assert rc == code and word in L.orbx_last_error(), (n, code)
        assert all((v == -7).all() for v in got.values()), n     # nothing written
        assert L.orbm_llt_env_solve_dev(n, _lib.ptr(np.ascontiguousarray(first)), p, p, p, p, p, p, None) == code, n
    assert L.orbm_llt_env_plan(64, None, None, None, None, None, None, None) == ERR_ARG
    first = np.zeros(1, np.int32)
    for k in range(6):
        args = [p] * 6
        args[k] = None
        assert L.orbm_llt_env_solve_dev(64, _lib.ptr(first), *args, None) == ERR_ARG, k
    assert b"null" in L.orbx_last_error()


def test_entry_points_are_declared_exported_and_bound():
    protos = _lib.prototypes()
    vp, i = C.c_void_p, C.c_int
    assert protos["orbm_llt_env_plan"] == (i, [i] + [vp] * 7)
    assert protos["orbm_llt_env_solve_dev"] == (i, [i] + [vp] * 8)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.build()]).decode()
    for fn in ("orbm_llt_env_plan", "orbm_llt_env_solve_dev"):
        assert f" T {fn}\n" in out, fn
        assert callable(getattr(_lib.lib(), fn))
    assert _lib.lib().orbx_abi_version() == 136
    import orb_slam2_e_amd
    assert callable(orb_slam2_e_amd.llt_env_plan) and callable(orb_slam2_e_amd.llt_env_solve_device)
