"""The one copy of g2o's Levenberg step rule (orb_slam2_e_amd/csrc/orbm_levenberg.h) alone, on the host: tests/cxx/levenberg_rule.cpp
drives start / verdict / end_iteration through scripted trials, and every lambda, ni, rho, decision and result code is compared by
its bits with the restatement below (optimization_algorithm_levenberg.cpp:97-115, :201-239, written from g2o, not from the header).
The program is built twice: plainly, and with the address and undefined-behaviour sanitizers."""
import math
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DBL_MAX = 1.7976931348623157e308
INF, NAN = float("inf"), float("nan")


def _hex(d):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", d))[0]


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or _hex(a) == _hex(b)


def _restated(current_chi, lambda_init, script):
    """One optimize() call as g2o runs it.  Returns the trial records (rho, scale, accepted, lambda, ni, currentChi), the iteration
    records (qmax, result, nBad) and the number of trials used."""
    trials, iterations, k = [], [], 0
    lam = ni = n_bad = None
    iteration = 0
    while k < len(script):
        ini_chi = current_chi
        if iteration == 0:
            lam, ni, n_bad = lambda_init, 2.0, 0
        rho, qmax = 0.0, 0
        while True:
            temp_chi, scale, ok = script[k]
            k += 1
            if not ok:
                temp_chi, scale = DBL_MAX, 0.0
            rho = current_chi - temp_chi
            scale = scale + 1e-3
            rho = rho / scale
            accepted = rho > 0 and math.isfinite(temp_chi)
            if accepted:
                alpha = 1.0 - math.pow(2 * rho - 1, 3.0)
                alpha = min(alpha, 2.0 / 3.0)
                lam *= max(alpha, 1.0 / 3.0)
                ni = 2.0
                current_chi = temp_chi
            else:
                lam *= ni
                ni *= 2
            trials.append((rho, scale, int(accepted), lam, ni, current_chi))
            qmax += 1
            if not (rho < 0 and qmax < 10) or k == len(script):
                break
        if qmax == 10 or rho == 0:
            result = 2
        else:
            n_bad = n_bad + 1 if (ini_chi - current_chi) * 1e3 < ini_chi else 0
            result = 2 if n_bad >= 3 else 1
        iterations.append((qmax, result, n_bad))
        iteration += 1
        if result != 1:
            break
    return trials, iterations, k


# (currentChi, lambda_init, [(tempChi, scale, ok) ...]): every case ends with the trial that gives Terminate
CASES = [
    # alpha inside the clamps (rho 0.9), a rejection and alpha clamped at 2/3 (rho 0.5), alpha clamped at 1/3 (rho 2), a failed solve
    # (its tempChi and scale are not read) and an acceptance behind it, then rho == 0 exactly
    (100.0, 1e-5 * 37.5, [(90.0, 10.0 / 0.9 - 1e-3, 1),
                          (95.0, 3.0, 1), (80.0, 20.0 - 1e-3, 1),
                          (70.0, 5.0 - 1e-3, 1),
                          (1.0, 1.0, 0), (60.0, 12.0, 1),
                          (60.0, 4.0, 1)]),
    # ten rejections in a row: qmax == 10, ni = 2^11
    (50.0, 1e-6, [(50.0 + 0.5 * k, 1.0 + k, 1) for k in range(1, 11)]),
    # NaN; +inf over a negative scale (rho > 0, tempChi not finite); an iteration with progress; three without
    (1000.0, 2.5e-3, [(NAN, 1.0, 1),
                      (INF, -2.0, 1),
                      (400.0, 700.0, 1),
                      (399.9, 0.11, 1), (399.8, 0.12, 1), (399.7, 0.13, 1)]),
    # the first of three iterations without progress resets behind a good one: 1, 2, good, 1, 2, 3
    (1000.0, 10.0, [(999.9, 0.11, 1), (999.8, 0.12, 1), (500.0, 600.0, 1), (499.99, 0.011, 1), (499.98, 0.012, 1), (499.97, 0.013, 1)]),
]


def test_the_script_reaches_every_decision_edge():
    """(of the restatement: the comparison below then pins the header to it at each of them)"""
    t0, i0, _ = _restated(*CASES[0])
    assert [t[2] for t in t0] == [1, 0, 1, 1, 0, 1, 0]
    assert 1 / 3 < t0[0][3] / CASES[0][1] < 2 / 3                        # inside the clamps
    assert t0[1][3] == t0[0][3] * 2.0 and t0[1][4] == 4.0               # rho < 0: lambda *= ni, ni *= 2
    assert _hex(t0[2][3]) == _hex(t0[1][3] * (2.0 / 3.0)) and t0[2][4] == 2.0
    assert _hex(t0[3][3]) == _hex(t0[2][3] * (1.0 / 3.0)) and t0[3][0] > 1.9
    assert t0[4][0] < 0 and t0[4][1] == 1e-3 and t0[4][5] == 70.0      # DBL_MAX from the failed solve: rejected
    assert t0[6][0] == 0.0 and i0[-1] == (1, 2, 0) and [i[1] for i in i0[:-1]] == [1, 1, 1, 1]
    t1, i1, _ = _restated(*CASES[1])
    assert [t[2] for t in t1] == [0] * 10 and t1[-1][4] == 2.0 ** 11 and i1 == [(10, 2, 0)]
    assert _hex(t1[-1][3]) == _hex(1e-6 * 2.0 ** 55)                     # 2 * 4 * ... * 2^10
    t2, i2, _ = _restated(*CASES[2])
    assert math.isnan(t2[0][0]) and t2[0][2] == 0 and i2[0] == (1, 1, 1)           # left the trial loop, no Terminate
    assert t2[1][0] == INF and t2[1][2] == 0 and i2[1] == (1, 1, 2)
    assert i2[2:] == [(1, 1, 0), (1, 1, 1), (1, 1, 2), (1, 2, 3)]
    _, i3, _ = _restated(*CASES[3])
    assert [i[1:] for i in i3] == [(1, 1), (1, 2), (1, 0), (1, 1), (1, 2), (2, 3)]


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_the_header_takes_the_restatements_decisions(sanitize, tmp_path):
    exe = str(tmp_path / "levenberg_rule")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + flags +
                          ["-I", os.path.join(ROOT, "orb_slam2_e_amd", "csrc"), os.path.join(ROOT, "tests", "cxx", "levenberg_rule.cpp"), "-o", exe])
    text = ""
    for chi, lam, script in CASES:
        text += "C %s %s %d\n" % (_hex(chi), _hex(lam), len(script))
        text += "".join("%s %s %d\n" % (_hex(c), _hex(s), ok) for c, s, ok in script)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = [l.split() for l in out.stdout.splitlines()]
    for case in CASES:
        trials, iterations, used = _restated(*case)
        assert used == len(case[2]) and iterations[-1][1] == 2
        for it in iterations:
            for _ in range(it[0]):
                got, ref = lines.pop(0), trials.pop(0)
                assert got[0] == "T" and int(got[3]) == ref[2], (got, ref)
                vals = [struct.unpack("<d", struct.pack("<Q", int(got[k], 16)))[0] for k in (1, 2, 4, 5, 6)]
                assert all(_same(v, r) for v, r in zip(vals, (ref[0], ref[1], ref[3], ref[4], ref[5]))), (got, ref)
            assert lines.pop(0) == ["I"] + [str(v) for v in it]
        assert lines.pop(0) == ["C", str(used)] and not trials
    assert not lines
