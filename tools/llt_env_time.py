#!/usr/bin/env python3
"""Times of orbm_llt_env_solve_dev alone, beside tools/llt_time.py's `solver` table.  One JSON line per measurement.

  default   at n = 384, 768, 1,536 and 3,072, which the dense solver accepts too, for the envelopes full, arrow (a band three tiles
            wide whose last row tile is full), band3, band1 and block diagonal: the envelope solver and orbm_llt_solve_dev on the
            SAME matrix in alternating calls, device events around each call (the matrix is restored by a device copy outside the
            events), median and spread over --reps calls after --warmup; live tiles, launches, and whether L and x are equal.
  --large   the envelope solver alone at n = 7,168, 14,336 and 28,672 for arrow, band3 and band1.
The matrix is made on the device: uniform entries in (-0.5, 0.5) in every live tile and a diagonal that dominates its row."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from orb_slam2_e_amd import bundle            # noqa: E402

SMALL_N, LARGE_N = [384, 768, 1536, 3072], [7168, 14336, 28672]
DEV = "cuda:0"


def envelope(name, nt):
    r = np.arange(nt)
    if name == "full":
        f = np.zeros(nt, int)
    elif name == "block_diagonal":
        f = r.copy()
    else:
        f = np.maximum(r - (1 if name == "band1" else 3), 0)
        if name == "arrow":
            f[-1] = 0
    return f.astype(np.int32)


def device_tiles(n, first, plan, seed=1):
    """[live][T][T] on the device: element [tile][j][i] = entry (i, j) of the tile; positive definite by its diagonal.  An entry has
    at most 2 nt T others in its row and column, of mean size 0.25."""
    import torch
    T = bundle.llt_tile()
    g = torch.Generator(device=DEV); g.manual_seed(seed)
    tiles = torch.rand((plan["live_tiles"], T, T), dtype=torch.float64, device=DEV, generator=g) - 0.5
    diag = torch.from_numpy((plan["off"][1:] - 1).astype(np.int64)).to(DEV)        # the diagonal tile closes every row tile
    tiles[diag] += torch.eye(T, dtype=torch.float64, device=DEV) * (T * (float(np.max(np.arange(len(first)) - first)) + 2))
    return tiles


def dense_image(tiles, n, first):
    """the [n][n] image orbm_llt_solve_dev takes (element [j][i] = entry (i, j), i >= j), zeros outside the live tiles"""
    import torch
    T = bundle.llt_tile()
    nt = len(first)
    S = torch.zeros((nt * T, nt * T), dtype=torch.float64, device=DEV)
    k = 0
    for R in range(nt):
        for C in range(int(first[R]), R + 1):
            S[C * T:(C + 1) * T, R * T:(R + 1) * T] = tiles[k]
            k += 1
    return torch.triu(S)[:n, :n].contiguous()                                      # [j][i] with i >= j: the image's upper triangle


def solver_ms(n, first, reps=20, warmup=3, against_dense=False):
    """median and spread of the envelope solver between device events; against_dense: the dense solver on the same matrix too"""
    import torch
    T = bundle.llt_tile()
    plan = bundle.llt_env_plan(n, first)
    src = device_tiles(n, first, plan)
    A, W = torch.empty_like(src), torch.empty_like(src)
    b = torch.ones(n, dtype=torch.float64, device=DEV)
    x, xd = torch.zeros_like(b), torch.zeros_like(b)
    ok, okd = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    pd = torch.from_numpy(plan["device"]).to(DEV)
    S0 = dense_image(src, n, first) if against_dense else None
    S = torch.empty_like(S0) if against_dense else None

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    env, dense = [], []
    for k in range(warmup + reps):                                                  # alternating calls
        A.copy_(src)
        t = timed(lambda: bundle.llt_env_solve_device(first, pd, A, W, b, x, ok))
        if against_dense:
            S.copy_(S0)
            td = timed(lambda: bundle.llt_solve_device(S, b, xd, okd))
        if k >= warmup:
            env.append(t)
            if against_dense:
                dense.append(td)
    assert int(ok.item()) == 1
    out = {"n": n, "tile": T, "row_tiles": len(first), "live_tiles": plan["live_tiles"], "launches": plan["launches"], "reps": reps,
           "env_ms": round(float(np.median(env)), 4), "env_spread_ms": [round(min(env), 4), round(max(env), 4)]}
    if against_dense:
        assert int(okd.item()) == 1
        nt = len(first)
        Sp = torch.zeros((nt * T, nt * T), dtype=torch.float64, device=DEV)
        Sp[:n, :n] = S
        same, k = bool(torch.equal(x, xd)), 0
        for R in range(nt):
            for C in range(int(first[R]), R + 1):
                got, want = A[k], Sp[C * T:(C + 1) * T, R * T:(R + 1) * T]
                keep = torch.triu(torch.ones((T, T), dtype=torch.bool, device=DEV)) if R == C else torch.ones((T, T), dtype=torch.bool, device=DEV)
                keep = keep & (torch.arange(T, device=DEV)[None, :] + R * T < n)
                same = same and bool(torch.equal(got[keep], want[keep]))
                k += 1
        spread = max(max(env) - min(env), max(dense) - min(dense))
        out.update(dense_ms=round(float(np.median(dense)), 4), dense_spread_ms=[round(min(dense), 4), round(max(dense), 4)],
                   dense_launches=4 * nt - 1, equal_numbers=same, env_not_slower=bool(np.median(env) <= np.median(dense) + spread))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--large", action="store_true")
    a = ap.parse_args()
    T = bundle.llt_tile()
    for n in (LARGE_N if a.large else SMALL_N):
        for name in (("arrow", "band3", "band1") if a.large else ("full", "arrow", "band3", "band1", "block_diagonal")):
            line = {"what": "env solver", "envelope": name}
            line.update(solver_ms(n, envelope(name, (n + T - 1) // T), a.reps, a.warmup, against_dense=not a.large))
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
