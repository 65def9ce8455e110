"""The numpy restatement of orbm_llt_env_solve_dev (include/orbslam_hip.h) with the tile edge T as a parameter, the
plan's lists built in numpy, the named envelopes and inputs of its tests, and the packing of a matrix into live tiles (test
infrastructure: never part of the product).

The restatement works tile by tile as the device does: a diagonal tile is factorised, the panel's row tiles solve against it, the
panel's trailing tiles add its T products in ascending k.  The running dot of a tile is ASSIGNED by the first product it ever
receives and added to afterwards, products and sums are separate numpy operations.  It works on an [n][n] array in which every
entry outside a live tile, and the strict upper part of every diagonal tile, is NaN from start to end: a read of such an entry would
poison the result, and env_solve itself checks before it returns that none was written."""
import numpy as np

import llt_reference as R

PATTERNS = ("full", "block_diagonal", "band", "arrow", "non_monotone", "random")


def ntiles(n, T):
    return (n + T - 1) // T


def envelope(pattern, nt, seed=0):
    """first[nt] of a named envelope"""
    r = np.arange(nt)
    if pattern == "full":
        f = np.zeros(nt, int)
    elif pattern == "block_diagonal":
        f = r.copy()
    elif pattern == "band":                                      # one tile beside the diagonal
        f = np.maximum(r - 1, 0)
    elif pattern == "arrow":                                     # the band, and the last row tile full
        f = np.maximum(r - 1, 0); f[-1] = 0
    elif pattern == "non_monotone":                              # 0 0 2 1 2 5 4 5 8 ...: a row that starts at itself after wider ones
        f = np.where(r % 3 == 2, r, np.maximum(r - 2, 0))
    elif pattern == "random":
        rng = np.random.default_rng(77 + 13 * nt + seed)
        f = np.array([int(rng.integers(0, R_ + 1)) for R_ in range(nt)])
    else:
        raise ValueError(pattern)
    return f.astype(np.int32)


def live_mask(n, first, T):
    """[n][n] bool: the entries (i >= j) of live tiles"""
    t = np.arange(n) // T
    f = np.asarray(first)[t]
    return (t[None, :] >= f[:, None]) & (np.arange(n)[None, :] <= np.arange(n)[:, None])


def masked_spd(n, first, T, seed=0):
    """B B^T + n I (llt_reference.spd) masked to the envelope and made positive definite by its diagonal (strict diagonal dominance);
    no entry inside a live tile is an exact zero.  (A symmetric, b)"""
    A, b = R.spd(n, seed)
    m = live_mask(n, first, T)
    A = np.where(m | m.T, A, 0.0)
    np.fill_diagonal(A, 0.0)
    np.fill_diagonal(A, np.abs(A).sum(1) + n)
    return A, b


def plan(n, first, T):
    """what orbm_llt_env_plan returns, from its definitions"""
    nt = ntiles(n, T)
    first = [int(v) for v in first]
    off = np.concatenate([[0], np.cumsum([r - first[r] + 1 for r in range(nt)])]).astype(np.int32)
    row_start, rows, trail_start, trail = [0], [], [0], []
    launches = 1 + 2 * nt
    for K in range(nt):
        rl = [r for r in range(K + 1, nt) if first[r] <= K]
        rows += rl
        trail += [(r, c) for r in rl for c in rl if c <= r]
        row_start.append(len(rows)); trail_start.append(len(trail))
        if K + 1 < nt:
            launches += 2 if rl else 1
    return {"off": off, "row_start": np.array(row_start, np.int32), "rows": np.array(rows, np.int32),
            "trail_start": np.array(trail_start, np.int32), "trail": np.array(trail, np.int32).reshape(-1, 2),
            "live_tiles": int(off[-1]), "launches": launches}


def env_solve(A, b, first, T):
    """(L, x, ok).  L is [n][n] with NaN wherever the solver has no storage; ok = 0 at a pivot that is not > 0: x = 0."""
    A = np.asarray(A, np.float64); b = np.asarray(b, np.float64)
    n = len(b); nt = ntiles(n, T)
    first = [int(v) for v in first]
    assert len(first) == nt and all(0 <= first[r] <= r for r in range(nt))
    sl = lambda K: slice(K * T, min((K + 1) * T, n))
    stored = live_mask(n, first, T)
    L = np.where(stored, A, np.nan)
    dot = np.full((n, n), np.nan)
    started = np.zeros((nt, nt), bool)

    def done(x, ok):
        assert np.isnan(L[~stored]).all() and np.isnan(dot[~(stored | stored.T)]).all()     # nothing outside a live tile was written
        return L, x, ok

    for K in range(nt):
        D, dd, s = L[sl(K), sl(K)], dot[sl(K), sl(K)], bool(started[K, K])
        assert s == (first[K] < K)
        for j in range(D.shape[0]):
            col = D[j:, j] - dd[j:, j] if s else D[j:, j].copy()
            if not col[0] > 0.0:
                return done(np.zeros(n), 0)
            piv = np.sqrt(col[0])
            D[j, j] = piv
            D[j + 1:, j] = col[1:] / piv
            c = D[j + 1:, j]
            outer = c[:, None] * c[None, :]
            dd[j + 1:, j + 1:] = dd[j + 1:, j + 1:] + outer if s else outer
            s = True
        rl = [r for r in range(K + 1, nt) if first[r] <= K]
        for Rt in rl:                                            # the row tiles against the final diagonal tile
            a, d, s = L[sl(Rt), sl(K)], dot[sl(Rt), sl(K)], bool(started[Rt, K])
            assert s == (max(first[Rt], first[K]) < K)
            for j in range(T):
                col = a[:, j] - d[:, j] if s else a[:, j].copy()
                l = col / D[j, j]
                a[:, j] = l
                outer = l[:, None] * D[j + 1:, j][None, :]
                d[:, j + 1:] = d[:, j + 1:] + outer if s else outer
                s = True
        for Rt in rl:                                            # the trailing tiles: the pairs of the row list
            for Ct in rl:
                if Ct > Rt:
                    continue
                Lr, Lc, d, s = L[sl(Rt), sl(K)], L[sl(Ct), sl(K)], dot[sl(Rt), sl(Ct)], bool(started[Rt, Ct])
                assert s == (max(first[Rt], first[Ct]) < K)
                for k in range(T):
                    outer = Lr[:, k][:, None] * Lc[:, k][None, :]
                    d[:, :] = d + outer if s else outer
                    s = True
                started[Rt, Ct] = True
    y = b.copy()
    for Rt in range(nt):
        yr = y[sl(Rt)]
        for K in range(first[Rt], Rt):
            Lt = L[sl(Rt), sl(K)]
            for j in range(T):
                yr[:] = yr - Lt[:, j] * y[K * T + j]
        D = L[sl(Rt), sl(Rt)]
        for j in range(len(yr)):
            yr[j] = yr[j] / D[j, j]
            yr[j + 1:] = yr[j + 1:] - D[j + 1:, j] * yr[j]
    for K in range(nt - 1, -1, -1):
        yk = y[sl(K)]
        D = L[sl(K), sl(K)]
        for j in range(len(yk) - 1, -1, -1):
            yk[j] = yk[j] / D[j, j]
            yk[:j] = yk[:j] - D[j, :j] * yk[j]
        for Rt in range(first[K], K):
            Lt, yr = L[sl(K), sl(Rt)], y[sl(Rt)]
            for j in range(len(yk) - 1, -1, -1):
                yr[:] = yr - Lt[j, :] * yk[j]
    return done(y, 1)


def pack(A, first, T, fill=np.nan):
    """[live][T][T] float64: element [tile][j][i] = entry (i, j) of the tile, tiles in the solver's order; what it never reads
    (rows at or beyond n, the strict upper part of a diagonal tile) holds `fill`"""
    n = len(A); nt = ntiles(n, T)
    out = []
    for Rt in range(nt):
        for Ct in range(int(first[Rt]), Rt + 1):
            t = np.full((T, T), fill)
            blk = A[Rt * T:(Rt + 1) * T, Ct * T:(Ct + 1) * T]
            t[:blk.shape[0], :blk.shape[1]] = blk
            if Rt == Ct:
                t[np.triu_indices(T, 1)] = fill
            out.append(t.T)
    return np.ascontiguousarray(np.array(out))


def unpack(tiles, n, first, T, outside=0.0):
    """the [n][n] lower triangle of packed tiles, `outside` wherever the solver has no storage"""
    nt = ntiles(n, T)
    L = np.full((n, n), outside)
    k = 0
    for Rt in range(nt):
        for Ct in range(int(first[Rt]), Rt + 1):
            h, w = min(T, n - Rt * T), min(T, n - Ct * T)
            L[Rt * T:Rt * T + h, Ct * T:Ct * T + w] = tiles[k].T[:h, :w]
            k += 1
    return np.where(live_mask(n, first, T), L, outside)
