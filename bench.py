#!/usr/bin/env python3
"""bench.py -- frames/s of the ORB extract + Hamming match hot path on MI355X.

Contract (see the task brief): `python bench.py --gpus N --steps K --warmup W`;
one rank per GPU.  For N>1 either torch.distributed.run starts the ranks (WORLD_SIZE set; it must equal N) or, started
plainly, this process becomes the parent of N rank processes before anything touches the GPU (orb_slam2_e_amd/launch.py),
relays rank 0's line and fails if any rank fails.  A *step* is one pass
of the hot path over one batch: 64 synthetic 640x480 frames per GPU ->
ORBextractor (2000 features, 8 levels, FAST 20/7) -> 2000x2000 brute-force
Hamming match of every frame against its successor in the batch (+ TH_LOW / 0.6
ratio filter) -> gather of the fixed-size result records on rank 0 (N>1 only).
Inputs are resident in HBM before the timed region.  Rank 0 prints ONE JSON line.

A plain run does only what that line's headline needs: set-up, the W warm-up steps, the K timed steps and the line
(`metric`, `value` = frames/s of the K steps, `unit`, `higher_is_better`, `dtype`, `ms_per_step`).  `--dump-outputs DIR`
writes the last timed step's results (rank 0's shard) as DIR/<name>.npy, float32.  `--full` adds everything else the
bench measures or checks, after the same timed region: the per-kernel split and roofline, the clock-conditioned
region, the oracle check (`verified`), the PCIe / one-frame legs, the FEM, matcher-loop, BoW and stereo legs and the
CPU baseline; the `--no-*` options below prune those legs of a `--full` run.

`roofline`: dominant kernel's algorithmic bytes / its mean launch time, timed
with HIP events on the launch stream inside the timed region (the events of the
kernel's own start and end: hipExtLaunchKernelGGL inside the library).  `cpu_baseline`:
the CPU oracle (single thread) on a bounded sample of the same workload.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

W, H, BATCH = 640, 480, 64
PARAMS = (2000, 1.2, 8, 20, 7)
HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
# Vector-instruction issue ceiling of the whole chip, MEASURED (tools/ubench/mfma_overlap.hip, round 4: 3,072 waves of dependent
# v_med3 / v_min / v_add on 1,024 SIMDs, 590 M wave64 instructions in 0.843 ms): a SIMD issues one wave64 VALU instruction per
# ~2.3 clocks when several waves have one ready, and the clock settles at 1.5-1.6 GHz under that load -- 1.46 ns per instruction
# and SIMD.  (Rounds 1-3 priced against 1024 x 2.4 GHz / 4 = 614: one instruction per 4 clocks is what ONE wave sustains.)
VALU_PEAK_GINST = 700.0
# MI355X_MICROARCH.md, Matrix cores: FP4 (v_mfma_f32_32x32x64_f8f6f4) dense peak; the all-pairs matcher runs on it
MFMA_FP4_PEAK_TFLOPS = 10000.0
# SURVEY 8(d) algorithmic bytes per 640x480 frame, by stage
PYR_PX = 950532
ALG_BYTES = {
    "k_pyr_level0": 307200 + 307200,            # read L0 input + write level 0
    "k_pyr_resize": (PYR_PX - 307200) * 2,      # read level l-1 (approx. its own size class) + write level l, levels 1..7
    "k_fast_cells": PYR_PX,                     # FAST read of the pyramid
    "k_octree": 0,
    "k_blur": 2 * PYR_PX,                       # blur read + write
    "k_describe": 2000 * 749 + 2000 * 512 + 2000 * 60,
    "k_match_sets_mfma": 144000,                # 2 x 2000 x 32 B read + 2000 x 8 B written
}
FRAME_BYTES = 6751328  # whole extract path per frame
KERNEL_KINDS = ["k_pyr_level0", "k_pyr_resize", "k_fast_cells", "k_octree", "k_blur", "k_describe"]  # orbx_profile_enable bit order


def cpu_baseline_child(legs, fem_csr=None, timeout=600):
    """SURVEY 8(d) CPU-baseline protocol in a child process (oracle/cpu_bench.py): the oracle built -O3 -march=native
    -ffp-contract=off on this host, one thread pinned to one core, 3 warm-ups, medians of >= 20 runs, plus the
    all-cores figure (one pinned worker per core).  The child never touches the GPU; this process only waits."""
    import subprocess
    cmd = [sys.executable, os.path.join(ROOT, "oracle", "cpu_bench.py"), "--legs", ",".join(legs)]
    if fem_csr:
        cmd += ["--fem-csr", fem_csr]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout, text=True)
    if r.returncode != 0:
        return {"error": r.stderr[-400:]}
    return json.loads(r.stdout.strip().splitlines()[-1])


def verify_against_oracle(frames, kps, desc, counts, best, second, idx, match12, nmatch, pair_b):
    """The checker, outside the timed region: every frame's keypoints (float bits) and descriptors and every pair's
    best / second / arg-best / accepted match / match count against the CPU oracle (ORBextractor.cc:1051-1113,
    ORBmatcher.cc:645-676 selection + TH_LOW / ratio acceptance).  Returns (ok, first mismatch or None)."""
    import oracle
    o = oracle.OrbOracle(*PARAMS)
    B = len(frames)
    od = []
    for f in range(B):
        okps, odesc = o.extract(frames[f])
        n = int(counts[f])
        if n != len(okps):
            return False, f"frame {f}: {n} keypoints, oracle {len(okps)}"
        if not np.array_equal(kps[f, :n].view(np.uint8), okps.view(np.uint8)) or not np.array_equal(desc[f, :n], odesc):
            return False, f"frame {f}: keypoints / descriptors differ"
        od.append(odesc)
    for f in range(B):
        g = int(pair_b[f])
        rb, rs, ri = oracle.match_bruteforce(od[f], od[g])
        rm, rn = oracle.match_filter(rb, rs, ri, 45, 0.6)
        n = len(od[f])
        if not (np.array_equal(best[f, :n], rb) and np.array_equal(second[f, :n], rs) and np.array_equal(idx[f, :n], ri)
                and np.array_equal(match12[f, :n], rm) and int(nmatch[f]) == rn):
            return False, f"pair ({f}, {g}): match result differs"
    return True, None


def dump_outputs(dirname, ctx, pack, lay, dev):
    """--dump-outputs: the results of the step context `ctx` ran last, as its caller receives them, to dirname/<name>.npy in float32
    (every value is an integer below 2^24 or a float32 already, so the conversion is exact).  Only each frame's first counts[f]
    rows are results (the rest of the fixed-capacity buffers is never written), so the per-frame rows are concatenated in
    frame order and `keypoint_counts` splits them again.  At most 64 x 2,024 rows: 22 MB in all."""
    import torch
    from orb_slam2_e_amd.extractor import KP_DTYPE
    u = ctx.user
    rec = torch.empty(lay.rec_bytes, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(u.tstream):
        pack(ctx, rec)
    torch.cuda.synchronize()
    R = lay.unpack(rec.cpu().numpy())
    best, second, idx = (t.cpu().numpy() for t in (u.best, u.second, u.idx))
    counts = R["counts"].astype(np.int64)
    rows = lambda a: np.concatenate([a[f, :n] for f, n in enumerate(counts)])
    kps = rows(R["kps"])
    out = {
        "keypoints": np.stack([kps[name].astype(np.float32) for name in KP_DTYPE.names], axis=1),   # x y size angle response octave class_id
        "descriptors": rows(R["desc"]).astype(np.float32),                                          # 32 bytes per keypoint
        "keypoint_counts": counts.astype(np.float32),
        "match_best_dist": rows(best).astype(np.float32),      # frame f's keypoints against frame f+1 mod 64
        "match_second_dist": rows(second).astype(np.float32),
        "match_best_idx": rows(idx).astype(np.float32),
        "match12": rows(R["match12"]).astype(np.float32),     # accepted match (TH_LOW, ratio) or -1
        "match_count": R["nmatch"].astype(np.float32),
    }
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    os.makedirs(dirname, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(dirname, name + ".npy"), a)


def fem_bench(rank, world, dist, torch, dev, cdev, nmesh=256, iters=200, csr_out=None):
    """Config 3 (10,368-tet / 6,591-dof mesh, E=3500, nu=0.495): assemble K + 200
    CG iterations, single mesh and a batch of `nmesh` distinct matrices per GPU; for N > 1 the nodal
    displacements of every rank's meshes are gathered on rank 0 inside the timed region."""
    from orb_slam2_e_amd.fem import FEA2, FEM_TET4
    from orb_slam2_e_amd.shard import gather_displacements, max_over_ranks
    from orb_slam2_e_amd.synth import synth_tet_batch

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    from orb_slam2_e_amd.fem import FEA2Batch
    from orb_slam2_e_amd.synth import synth_tet_batch_distinct
    out = {}
    # legs: the single config-3 mesh; `nmesh` config-3 meshes sharing a topology (268 MB of matrix per iteration: the size of the
    # 256-MiB Infinity Cache, which therefore serves part of it); `nmesh` meshes of their own topologies and sizes; and `nmesh`
    # meshes of 12,288 dofs (15^3 cells) whose live working set -- 560 MB of matrix + 150 MB of vectors per iteration -- is more
    # than twice the Infinity Cache: the leg the HBM roofline is quoted on
    legs = (("single", 1, 12), ("batch", nmesh, 12), ("batch_distinct_topologies", nmesh, 12), ("batch_beyond_infinity_cache", nmesh, 15))
    for label, nm, ncell in legs:
        t0 = time.perf_counter()
        if label == "batch_distinct_topologies":
            # every mesh its own topology and size (grids of 10..14 cells per side: 6,591 dofs on average), as the reference
            # builds a new mesh on every call; one block-diagonal system in global numbering
            nodes_l, tets_l, fixed_l, load_l = synth_tet_batch_distinct(nm, seed=11 + 7919 * rank)
            t_synth = time.perf_counter() - t0
            t0 = time.perf_counter()
            fea = FEA2Batch(nodes_l, tets_l, FEM_TET4)
            t_create = time.perf_counter() - t0
            fixed = np.concatenate([fea.dof0[k] + fx for k, fx in enumerate(fixed_l)]).astype(np.int32)
            b = np.concatenate(load_l)[None].copy(); b[:, fixed] = 0
        else:
            nodes, tets, fixed, load = synth_tet_batch(nm, ncell, seed=11 + 7919 * rank)
            t_synth = time.perf_counter() - t0
            t0 = time.perf_counter()
            fea = FEA2(nodes, tets, FEM_TET4)
            t_create = time.perf_counter() - t0
            b = np.tile(load, (nm, 1)); b[:, fixed] = 0
        fea.profile(True)
        t0 = time.perf_counter(); fea.MatrixAssembly(); t_asm = time.perf_counter() - t0
        fea.eliminate_dofs(fixed)
        fea.cg_setup(b)
        fea.profile(True)
        fea.cg_iterate(iters); fea.cg_result()        # warm + per-kernel split (untimed pass, all kinds): the same length as the timed
                                                      # pass -- the first full-length launch after a set-up runs ~6 % longer than the next ones
        split = {k: v[0] / max(v[1], 1) for k, v in fea.profile_read().items() if v[1]}
        # the timed region, three times: a leg is ONE launch of 7-25 ms, so a transient dip of the card's clocks would be the whole
        # measurement.  The MEDIAN pass is what the line reports (`ms_per_iter`, `cg_mesh_iters_per_s`, the resident kernel's
        # roofline); the best pass stands beside it as `*_best` (rounds 2-4 reported the better of two passes alone).  The
        # iterations are deterministic, every pass leaves the same x.
        passes = []
        for attempt in range(3):
            fea.cg_setup(b)
            fea.profile((4 | 32) if nm > 1 else 0)        # events around k_fem_spmv / k_fem_cg_resident only (batch);
            barrier()                                     # (the single mesh launches phase by phase)
            t0 = time.perf_counter()
            fea.cg_iterate(iters)
            x, rel = fea.cg_result()                       # synchronises
            xall = gather_displacements(x, rank, world, cdev)   # N > 1: [world * nm, ndof] on rank 0
            barrier()
            dt_a = max_over_ranks(time.perf_counter() - t0, world, cdev)
            passes.append((dt_a, fea.profile_read()))
        passes.sort(key=lambda q: q[0])
        dt, prof = passes[1]
        dt_best = passes[0][0]
        n, nnz = fea.Ksize, fea.nnz
        distinct = label == "batch_distinct_topologies"
        spmv_ms = prof["k_fem_spmv"][0] / max(prof["k_fem_spmv"][1], 1) if prof["k_fem_spmv"][1] else split.get("k_fem_spmv", 0.0)
        # batches whose meshes fit a compute unit each: ONE launch runs all iterations (k_fem_cg_resident), the matrix is the only stream
        res = prof.get("k_fem_cg_resident", (0.0, 0))
        resident = bool(res[1])
        nblocks = 1 if distinct else nm                             # Ksize / nnz are totals for the concatenated batch
        spmv_bytes = nblocks * (nnz * 8 + (n + 1) * 4 + 2 * n * 8)  # nnz(val+4)+(n+1)4+2n*val', f32 K, f64 x/y
        spb = 48 if nblocks * ((n + 95) // 96) < 512 and not distinct else 96      # rows per SpMV workgroup (fem.hip: create_model)
        grid_threads = 256 * (sum((int(fea.dof0[k + 1] - fea.dof0[k]) + 95) // 96 for k in range(nm)) if distinct else nm * ((n + spb - 1) // spb))
        # what the kernel's 3 x 3 block form needs: values, ONE column index per block (nnz / 9), block-row table, x and y
        # (shared topology: the index and block-row tables once -- every mesh reads them, L2 serves them)
        block_bytes = nblocks * (nnz * 4 + 2 * n * 8) + (nnz // 9) * 4 + (n // 3 + 1) * 4
        # the resident form per iteration: values, one column index per block, the chunk table; p and Ap stay in LDS (meshes
        # above 7,168 dofs keep p only: Ap, x and 1/diag go through the batch vectors, 48 bytes per dof)
        big = distinct and max(int(fea.dof0[k + 1] - fea.dof0[k]) for k in range(nm)) > 7168 or (not distinct and n > 7168)
        resident_bytes = nblocks * nnz * 4 + (nnz // 9) * 4 + (n // 3 + 1) * 4 + (nblocks * n * 48 if big else 0)
        out[label] = {"meshes_per_gpu": nm, "n_dof": n, "nnz": nnz, "cg_iters": iters, "create_ms": t_create * 1e3, "synth_ms_host_numpy": t_synth * 1e3,
                      "spmv_grid_threads": grid_threads,
                      "cg_mesh_iters_per_s": world * nm * iters / dt, "ms_per_iter": dt / iters * 1e3,
                      "cg_mesh_iters_per_s_best": world * nm * iters / dt_best, "ms_per_iter_best": dt_best / iters * 1e3,
                      "timed_passes": "3; the median pass is reported, the best beside it as *_best",
                      "assemble_ms": t_asm * 1e3, "relres_after": float(rel.max()),
                      "spmv_avg_launch_ms": spmv_ms, "spmv_alg_bytes_per_launch": spmv_bytes, "spmv_block_form_bytes_per_launch": block_bytes,
                      "spmv_GBps": spmv_bytes / (spmv_ms * 1e-3) / 1e9 if spmv_ms > 0 else 0.0,
                      "resident": ({"kernel": "k_fem_cg_resident", "launch_ms": res[0] / res[1], "iters_per_launch": iters * 1.0 / res[1],
                                    "ms_per_iter_kernel": res[0] / iters, "alg_bytes_per_iter": resident_bytes,
                                    "GBps": resident_bytes / (res[0] / iters * 1e-3) / 1e9, "p_only_in_lds": bool(big)} if resident else None),
                      "displacements_gathered": None if xall is None else list(xall.shape),
                      "kernel_ms_per_launch_untimed_pass": split}
        # time to tolerance (what a user pays; the contract metric above is iterations/s): the same system to relres <= 1e-8 in
        # slices of 25 iterations, every slice followed by the residuals' trip to the host (8 bytes per mesh), under both
        # preconditioners; setup = fem_cg_setup (block-major copy of K, and for the two-level form the coarse space, the 48
        # products of Z^T K Z and its inverse)
        fea.profile(0)
        tt = {}
        for kind in ("jacobi", "two_level"):
            fea.cg_preconditioner(kind)
            fea.cg_setup(b); fea.cg_iterate(25); fea.cg_relres()        # untimed: first launch of this kernel variant
            barrier()
            t0 = time.perf_counter()
            fea.cg_setup(b)
            t_set = time.perf_counter() - t0
            it_tol, rel_tol = 0, 1.0
            while it_tol < 6000 and rel_tol > 1e-8:
                fea.cg_iterate(25); it_tol += 25
                rel_tol = float(fea.cg_relres().max())
            tt[kind] = {"iterations": it_tol, "ms": (time.perf_counter() - t0) * 1e3, "setup_ms": t_set * 1e3, "relres_reached": rel_tol}
        fea.cg_preconditioner("jacobi"); fea.cg_setup(b)
        out[label]["to_tolerance"] = {"relres": 1e-8, "iterations": tt["jacobi"]["iterations"], "ms": tt["jacobi"]["ms"],
                                      "relres_reached": tt["jacobi"]["relres_reached"], "preconditioner": "point Jacobi", "jacobi": tt["jacobi"],
                                      "two_level": dict(tt["two_level"], preconditioner="Jacobi + rigid-body modes of 2 x 2 x 2 aggregates (fem_cg_preconditioner)"),
                                      "speedup_two_level": tt["jacobi"]["ms"] / tt["two_level"]["ms"]}
        if nm > 1:
            # north_star names "the FEM SpMV": k_fem_spmv by itself on the same resident matrix and vectors (the launch-per-phase
            # kernel; the batches' CG runs in k_fem_cg_resident, which contains the same product), 50 launches under HIP events
            fea.profile(4)
            fea.spmv_repeat(50)
            fea.cg_result()
            sp = fea.profile_read()["k_fem_spmv"]
            if sp[1]:
                sms = sp[0] / sp[1]
                out[label]["spmv_alone"] = {"kernel": "k_fem_spmv", "launch_ms": sms, "block_form_bytes_per_launch": block_bytes,
                                            "GBps": block_bytes / (sms * 1e-3) / 1e9, "frac_of_8000": block_bytes / (sms * 1e-3) / 1e9 / HBM_PEAK_GBS}
                trs = load_fem_traffic().get(label, {}).get("k_fem_spmv") if nmesh == 256 else None    # the PMC passes ran the 256-mesh batches
                if trs:
                    out[label]["spmv_alone"].update({"traffic": trs["hbm_bytes_per_launch"], "traffic_source": trs["source"]})
            fea.profile(0)
        # the checker, outside the timed region, on every rank: the iterate the TIMED launches left (the single mesh; the first,
        # the largest and the last mesh of each batch -- the batches' 200 iterations ran in k_fem_cg_resident) against the
        # oracle's CG on the mesh's exported CSR, 1e-5 relative on the nodal displacements (north_star)
        import oracle
        if distinct:
            sizes = [int(fea.dof0[k + 1] - fea.dof0[k]) for k in range(nm)]
            picks = sorted({0, int(np.argmax(sizes)), nm - 1})
        else:
            picks = sorted({0, nm // 2, nm - 1})
        devs = {}
        for k in picks:
            rp, col, val = fea.csr(k)
            if distinct:
                d0, d1 = int(fea.dof0[k]), int(fea.dof0[k + 1])
                bk, xk = b[0, d0:d1], x[0, d0:d1]
            else:
                bk, xk = b[k], x[k]
            ox, _, orel = oracle.fem_cg(rp, col, val, bk, iters, 0.0)
            devs[k] = float(np.abs(xk - ox).max() / np.abs(ox).max())
            if label == "single" and rank == 0 and csr_out:
                np.savez(csr_out, rp=rp, col=col, val=val, b=bk)
        worst = max(devs.values())
        ok = bool(np.isfinite(x).all() and worst <= 1e-5)
        if world > 1:
            oks = [None] * world
            dist.all_gather_object(oks, (ok, worst))
            ok, worst = all(o[0] for o in oks), max(o[1] for o in oks)
        out[label]["max_rel_dev_vs_oracle"] = worst
        out[label]["verified_meshes"] = picks
        out[label]["verified"] = ok
        out["verified"] = bool(out.get("verified", True) and ok)
        del fea
    traffic = load_traffic()
    fem_tr = load_fem_traffic()
    HBM_ACHIEVABLE_GBS = 6300.0   # MI355X_MICROARCH.md: what a streaming kernel sustains out of the 8 TB/s specification
    for key, label in (("roofline", "batch_beyond_infinity_cache"), ("roofline_infinity_cache_resident", "batch"),
                       ("roofline_distinct_topologies", "batch_distinct_topologies")):
        bt = out[label]
        if bt["resident"]:
            rs = bt["resident"]
            tr = fem_tr.get(label) if (nmesh == 256 and bt["cg_iters"] == 200) else None   # the PMC passes ran 256 meshes x 200 iterations
            out[key] = {"bound": "hbm", "kernel": "k_fem_cg_resident", "achieved": rs["GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": rs["GBps"] / HBM_PEAK_GBS, "frac_of_achievable_6300": rs["GBps"] / HBM_ACHIEVABLE_GBS,
                        "traffic": tr["hbm_bytes_per_launch"] if tr else None, "traffic_source": tr["source"] if tr else None,
                        "avg_launch_ms": rs["launch_ms"],
                        "alg_bytes_per_launch": rs["alg_bytes_per_iter"] * rs["iters_per_launch"],
                        "working_set_bytes_per_iteration": rs["alg_bytes_per_iter"],
                        "infinity_cache_bytes": 256 << 20,
                        "note": "one launch = all CG iterations of the batch, one workgroup per mesh; algorithmic bytes per iteration = the "
                                "block-major values, ONE column index per nine values and the chunk table (p and Ap live in LDS, x / r / "
                                "1/diag in registers; meshes above 7,168 dofs: + 48 B per dof for Ap, x and 1/diag)",
                        "batch": {"batch": "INFINITY-CACHE-RESIDENT: one topology shared by all meshes; the 268 MB an iteration streams are the size "
                                           "of the 256-MiB Infinity Cache, which serves part of them (FETCH_SIZE counts its hits as fetches), so "
                                           "this rate is NOT an HBM rate and may exceed the HBM peak it is priced against",
                                  "batch_beyond_infinity_cache": "one topology, 12,288 dofs per mesh: the working set of an iteration is more than "
                                                                 "twice the Infinity Cache, every byte comes from HBM every iteration",
                                  "batch_distinct_topologies": "every mesh its own topology (1.4x the Infinity Cache per iteration); one workgroup "
                                                               "per mesh, so the launch lasts as long as its largest mesh (10,125 dofs against "
                                                               "6,591 on average)"}[label]}
            continue
        ms = bt["spmv_avg_launch_ms"]
        blk_gbps = bt["spmv_block_form_bytes_per_launch"] / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
        rf = {"bound": "hbm", "kernel": "k_fem_spmv", "achieved": blk_gbps, "peak": HBM_PEAK_GBS,
              "unit": "GB/s", "frac": blk_gbps / HBM_PEAK_GBS, "traffic": None,
              "avg_launch_ms": ms, "alg_bytes_per_launch": bt["spmv_block_form_bytes_per_launch"],
              "note": "algorithmic bytes of the kernel's 3 x 3 node-block form: values, ONE column index per nine values, x and y. "
                      "SURVEY 8(d)'s formula charges a CSR SpMV 4 index bytes per non-zero (survey_csr_bytes_per_launch); at this "
                      "launch time that would read as frac_if_charged_survey_csr_bytes, bytes the kernel never moves",
              "survey_csr_bytes_per_launch": bt["spmv_alg_bytes_per_launch"],
              "frac_if_charged_survey_csr_bytes": bt["spmv_GBps"] / HBM_PEAK_GBS,
              "batch": "one topology shared by all meshes (one column-index array, L2-resident)" if label == "batch" else
                       "every mesh its own topology (its own column indices, streamed from HBM)"}
        tr = traffic.get(f"k_fem_spmv@{bt['spmv_grid_threads']}") if nmesh == 256 else None   # PMC passes: the 256-mesh batches
        if tr:
            rf["traffic"] = tr["hbm_bytes_per_launch"]
            rf["traffic_source"] = tr["source"]
            if bt["spmv_avg_launch_ms"] > 0:
                # what HBM delivers by the counters (FETCH_SIZE x 2 + WRITE_SIZE of the PMC passes; the x 2 is calibrated
                # on 16-byte-per-lane streams, this kernel streams 12 bytes per lane: an upper bound)
                rf["frac_of_counter_traffic"] = tr["hbm_bytes_per_launch"] / (bt["spmv_avg_launch_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBS
        out[key] = rf
    return out


def fem_compute1_bench():
    """What Optimizer::PoseOptimizationNR pays per call on the FEM side (Optimizer.cc:480, :723; FEA2::Compute(1), FEA2.cc:80-121,
    its numeric half) at the reference's own mesh sizes -- the four surface meshes of tests/golden as prism models: fem_create
    (symbolic phase on the host + ONE staged upload), fem_assemble, the Dirichlet penalty and fem_trial_setup, each timed on
    its own with a synchronisation behind it, and one LM trial (levenberg.cpp:159-175) on the resident state."""
    from orb_slam2_e_amd.fem import FEA2, FEM_C3D6, extrude_elems, second_layer
    out = {}
    for name in ("min", "median", "p90", "large"):
        m = np.load(os.path.join(ROOT, "tests", "golden", f"fem_mesh_{name}.npz"))
        top, tris = m["points"], m["triangles"]
        p = top[tris]
        tris = tris[~((p[:, 0] == p[:, 1]).all(1) | (p[:, 0] == p[:, 2]).all(1) | (p[:, 1] == p[:, 2]).all(1))]
        nodes = second_layer(top, 0.5); elems = extrude_elems(tris, len(top))
        ids = np.arange(len(top), 2 * len(top), dtype=np.int32)
        u0 = nodes.ravel()
        reps = 30
        acc = np.zeros(5)
        per_rep = []
        fea = None
        for r in range(reps + 3):
            t = [time.perf_counter()]
            fea = FEA2(nodes, elems, FEM_C3D6); t.append(time.perf_counter())
            fea.MatrixAssembly(); t.append(time.perf_counter())          # (every one of these calls ends with a wait for the model's stream)
            fea.ImposeDirichletEncastre_K(ids); t.append(time.perf_counter())
            fea.trial_setup(u0, ids, len(top), None); t.append(time.perf_counter())
            if r >= 3:
                per_rep.append(np.diff(t))
        pts = top.astype(np.float64) + 0.003
        acc[:4] = np.median(np.array(per_rep), axis=0) * reps        # the median call of each phase
        trial_med, trial_best = batch_ms(lambda: fea.trial_energy(pts, want_a=False), 100, warm=10, batch=20)   # as the hook: estimates in, the two energies out
        acc[4] = trial_med * 1e-3 * reps
        ms = acc / reps * 1e3
        out[name] = {"Ksize": int(fea.Ksize), "elements": int(len(elems)), "create_ms": ms[0], "assemble_ms": ms[1], "dirichlet_ms": ms[2],
                     "trial_setup_ms": ms[3], "compute1_ms": float(ms[:4].sum()), "lm_trial_ms": ms[4], "lm_trial_ms_best": trial_best}
    return out


def fem_compute1_all_meshes(trials=40):
    """The FEM side of one Optimizer::PoseOptimizationNR call on EVERY surface mesh the reference tree holds (853 dumps under
    output/PointClouds, tests/golden/fem_meshes_all.npz; degenerate triangles removed), one call per mesh, cold: FEA2::Compute(1)'s
    numeric half (create, assemble, Dirichlet penalty, hook set-up) + the 4 x 10 Levenberg trials' energy evaluations
    (levenberg.cpp:159-199).  BASELINE.md's `timeD` medians (27-160 ms per file) time the reference's whole call INCLUDING its PCL
    meshing (MLS + greedy triangulation, FEA2.cc:205-438), which is out of scope here: context, not a like-for-like baseline."""
    from orb_slam2_e_amd.fem import FEA2, FEM_C3D6, extrude_elems, second_layer
    z = dict(np.load(os.path.join(ROOT, "tests", "golden", "fem_meshes_all.npz")))
    c1, tr, npts = [], [], []
    for k in range(len(z["frame"])):
        top = z["points"][z["pt_off"][k]:z["pt_off"][k + 1]]; tris = z["triangles"][z["tri_off"][k]:z["tri_off"][k + 1]]
        p = top[tris]
        tris = tris[~((p[:, 0] == p[:, 1]).all(1) | (p[:, 0] == p[:, 2]).all(1) | (p[:, 1] == p[:, 2]).all(1))]
        if not len(tris):
            continue
        nodes = second_layer(top, 0.5); elems = extrude_elems(tris, len(top))
        ids = np.arange(len(top), 2 * len(top), dtype=np.int32)
        u0 = nodes.ravel(); pts = top.astype(np.float64) + 0.003
        t0 = time.perf_counter()
        fea = FEA2(nodes, elems, FEM_C3D6); fea.MatrixAssembly(); fea.ImposeDirichletEncastre_K(ids); fea.trial_setup(u0, ids, len(top), None)
        t1 = time.perf_counter()
        for _ in range(trials):
            fea.trial_energy(pts, want_a=False)
        t2 = time.perf_counter()
        c1.append((t1 - t0) * 1e3); tr.append((t2 - t1) * 1e3); npts.append(len(top))
        del fea
    c1, tr = np.array(c1), np.array(tr)
    tot = c1 + tr
    q = lambda a: {"median": float(np.median(a)), "p90": float(np.percentile(a, 90)), "max": float(a.max())}
    return {"meshes": len(c1), "points_median": int(np.median(npts)), "points_max": int(max(npts)), "lm_trials_per_mesh": trials,
            "compute1_ms": q(c1), "lm_trials_ms": q(tr), "fem_side_of_one_call_ms": q(tot), "all_meshes_s": float(tot.sum() * 1e-3),
            "reference_timeD_ms_medians": "27.3 - 159.1 per log file (BASELINE.md 2): the reference's WHOLE PoseOptimizationNR incl. PCL meshing + g2o, hardware unstated -- context only"}


def _newest_profile(suffix):
    """profiles/rNN_<suffix> of the highest round number present (the passes are re-made on every round's final library)."""
    import glob
    import re
    best = None
    for f in glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_" + suffix)):
        r = int(re.match(r"r(\d\d)_", os.path.basename(f)).group(1))
        if best is None or r > best[0]:
            best = (r, f)
    return best[1] if best else None


def load_fem_traffic():
    """HBM bytes per 200-iteration launch of the batched CG legs (tools/fem_traffic.py over separate FETCH_SIZE / WRITE_SIZE passes)."""
    f = _newest_profile("fem_traffic.json")
    return json.load(open(f)) if f else {}


def load_traffic():
    """HBM bytes / VALU instruction counts per launch from the committed PMC passes (newest round)."""
    f = _newest_profile("traffic.json")
    return json.load(open(f)) if f else {}


def batch_ms(f, reps, warm=5, batch=10):
    """Per-call latency of f in ms: `warm` untimed calls, then reps calls in batches of `batch`.  Returns (median, best) of the
    batch means.  These legs are single calls of 30-150 us issued from an otherwise idle process: the card's power management now
    and then runs a batch at a fraction of its clocks (0.79 ms where 0.086 is the rule, seen in isolation) -- the MEDIAN batch is
    what the line reports under the plain key, the best batch beside it as `<key>_best` (rounds 1-4 reported the best alone)."""
    for _ in range(warm): f()
    t = []
    for _ in range(max(3, reps // batch)):
        t0 = time.perf_counter()
        for _ in range(batch): f()
        t.append((time.perf_counter() - t0) / batch)
    return float(np.median(t)) * 1e3, min(t) * 1e3


def put_ms(out, key, f, reps, warm=5, batch=10):
    """out[key] = median batch mean of f in ms, out[key + '_best'] = best batch mean."""
    assert key.endswith("_ms")
    out[key], out[key + "_best"] = batch_ms(f, reps, warm, batch)
    return out[key]


def matcher_loops_bench():
    """Tracking-time matching: one call = one whole ORBmatcher loop, host arrays in and out
    (PCIe and the per-call host work included); the oracle's literal loops on the same inputs are timed by
    oracle/cpu_bench.py."""
    from orb_slam2_e_amd.matcher import ORBmatcher
    from orb_slam2_e_amd.synth import synth_bow_case, synth_projection_case
    from orb_slam2_e_amd.vocabulary import feature_vector_arrays

    q, qd, qa, takes, kps, desc, bounds, occ, ur = synth_projection_case(0, n=2000, nq=2000, hot=2000)
    d1, a1, node1, keep1, valid1, d2, a2, node2, keep2, valid2 = synth_bow_case(0)
    fv1 = feature_vector_arrays(node1, keep1); fv2 = feature_vector_arrays(node2, keep2)
    m = ORBmatcher(0.6, True)
    from orb_slam2_e_amd.synth import synth_initialization_case
    ik1, id1, ik2, id2, iprev, ibounds = synth_initialization_case(0)
    mi = ORBmatcher(0.9, True)
    # the same searches on a frame that stays in HBM between calls (orbm_frame: grid built once per frame, on the device), and
    # the per-frame call of Tracking::TrackWithMotionModel as ONE whole function (projection prefix + search + resolver)
    from orb_slam2_e_amd import Frame, Points, View
    from orb_slam2_e_amd.synth import synth_tracking_scene
    fr = Frame(kps, desc, bounds, ur)
    sc = synth_tracking_scene(11)
    lm = sc["last_mp"]
    cur = Frame(sc["kps"], sc["desc"], sc["bounds"])
    view = View(*sc["cam"], sc["mb"], sc["mbf"], sc["log_scale_factor"], sc["scale_factors"])
    last = Points(sc["last_valid"], sc["pos"][lm], sc["mp_desc"][lm], takes=sc["last_takes"], octave=sc["last_octave"], angle=sc["last_angle"])
    npnt = len(sc["pos"])
    pts = Points(np.ones(npnt, np.uint8), sc["pos"], sc["mp_desc"], normal=sc["normal"], min_distance=sc["mind"], max_distance=sc["maxd"],
                 takes=np.ones(npnt, np.uint8))
    # SearchByBoW with both frames resident: positions do not matter to it, any keypoints carrying the case's angles will do
    from orb_slam2_e_amd import KP_DTYPE
    brng = np.random.default_rng(5)

    def bow_frame(d, a):
        k = np.zeros(len(d), KP_DTYPE)
        k["x"] = brng.uniform(0, 640, len(d)); k["y"] = brng.uniform(0, 480, len(d)); k["angle"] = a
        return Frame(k, d, (0.0, 0.0, 640.0, 480.0))
    bf1, bf2 = bow_frame(d1, a1), bow_frame(d2, a2)
    out = {"timing": "per call: median of the means of 10-call batches; `_best` = the best batch (the only figure of rounds 1-4)"}
    for key, f, reps in (
            ("search_for_initialization_2000x2200_ms", lambda: mi.SearchForInitialization(ik1, id1, ik2, id2, iprev, ibounds, 100), 30),
            ("search_by_projection_2000x2000_ms", lambda: m.frame_search_projection(fr, q, qd, qa, takes, occ, 95), 100),
            ("search_by_projection_2000x2000_host_arrays_ms", lambda: m.search_projection(q, qd, qa, takes, kps, desc, bounds, occ, ur, 95), 50),
            ("search_by_projection_last_frame_whole_2000x2000_ms", lambda: m.SearchByProjectionLast(cur, view, sc["Tcw"], sc["Tlw"], last, sc["occupied"], 7.0, True), 100),
            ("search_local_points_whole_2500x2000_ms", lambda: m.SearchByProjectionPoints(cur, view, sc["Tcw"], pts, sc["occupied"], 1.0), 100),
            ("frame_create_2000_ms", lambda: Frame(kps, desc, bounds, ur).close(), 50),
            ("search_by_bow_2000x2100_ms", lambda: m.SearchByBoW(fv1, valid1, d1, a1, fv2, valid2, d2, a2, False), 50),
            ("search_by_bow_2000x2100_resident_ms", lambda: m.frame_search_by_bow(bf1, fv1, valid1, bf2, fv2, None, False), 50),
            ("search_window_2000x2000_ms", lambda: m.frame_search_window(fr, q, qd, occ), 100),
            ("search_window_2000x2000_host_arrays_ms", lambda: m.search_window(q, qd, kps, desc, bounds, occ, ur), 50)):
        put_ms(out, key, f, reps)
    fr.close(); cur.close(); bf1.close(); bf2.close()
    return out


BOW_K, BOW_L, BOW_SETS, BOW_CAP = 10, 6, 64, 2000     # ORBvoc's shape (k = 10, L = 6: 1,111,111 nodes), 64 frames x 2000 descriptors


def bow_case():
    """The vocabulary and the descriptor sets of the bow_transform leg (the CPU baseline child builds the same)."""
    from orb_slam2_e_amd.synth import synth_vocabulary, synth_vocabulary_features
    voc = synth_vocabulary(BOW_K, BOW_L, seed=0)
    feats = synth_vocabulary_features(voc, BOW_SETS * BOW_CAP, seed=1).reshape(BOW_SETS, BOW_CAP, 32)
    return voc, feats


def distinctive_case(m=2000, seed=3):
    """m map points with 2..40 observations each (MapPoint::ComputeDistinctiveDescriptors' input, MapPoint.cc:305-370)."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 41, m)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    base = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    desc = np.repeat(base, sizes, axis=0) ^ np.packbits(rng.random((int(off[-1]), 256)) < 0.1, axis=1, bitorder="little")
    return desc, off


def bow_bench(torch, dev, batch_only=False):
    """SURVEY 8(f) rank 2 at the reference's real vocabulary shape: DBoW2 transform's tree descent (TemplatedVocabulary.h:1218-1262,
    levelsup = 4 as Frame.cc:415) of 64 x 2000 resident descriptors through a k = 10, L = 6 tree (35.6 MB of node descriptors --
    the gather pattern of ORBvoc.txt, which is missing from the reference mount), one launch; and rank 4,
    ComputeDistinctiveDescriptors over 2000 map points, one call on host arrays."""
    import oracle
    from orb_slam2_e_amd.matcher import ORBmatcher
    from orb_slam2_e_amd.vocabulary import ORBVocabulary
    voc, feats = bow_case()
    t0 = time.perf_counter()
    v = ORBVocabulary(*voc)
    create_ms = (time.perf_counter() - t0) * 1e3
    d_f = torch.from_numpy(feats).to(dev)
    d_cnt = torch.full((BOW_SETS,), BOW_CAP, dtype=torch.int32, device=dev)
    d_w = torch.full((BOW_SETS, BOW_CAP), -7, dtype=torch.int32, device=dev); d_n = torch.full_like(d_w, -7)
    ts = torch.cuda.Stream(device=dev)
    run = lambda: v.descend_batch_device(d_f.data_ptr(), d_cnt.data_ptr(), BOW_CAP, BOW_SETS, 4, d_w.data_ptr(), d_n.data_ptr(), ts.cuda_stream)
    reps = 50
    from orb_slam2_e_amd._lib import lib
    L = lib()
    with torch.cuda.stream(ts):
        for _ in range(5): run()
        ts.synchronize()
        # the kernel's own start and end events on the stream it is launched on (hipExtLaunchKernelGGL inside the library: two event
        # records around a 20-us launch measured 30 us), one read per launch for the median
        t = []
        for _ in range(reps):
            L.orbm_profile_enable(2)
            run()
            ms, nl = C.c_double(0), C.c_int64(0)
            L.orbm_profile_read_bow(C.byref(ms), C.byref(nl))
            t.append(ms.value / max(nl.value, 1))
        L.orbm_profile_enable(0)
    t = np.array(t)
    # whole-batch wall time, back to back without events
    t0 = time.perf_counter()
    for _ in range(reps): run()
    ts.synchronize()
    wall_ms = (time.perf_counter() - t0) / reps * 1e3
    nd = BOW_SETS * BOW_CAP
    alg = nd * (BOW_L * BOW_K * 32 + 32 + 8)        # every level's children descriptors + the feature + word id and node id out
    avg = float(t.mean())
    # the checker, outside the timed region: all 128,000 descents against the oracle
    ref = oracle.bow_descend(*voc, feats.reshape(-1, 32), 4)
    ok = bool(np.array_equal(d_w.cpu().numpy().ravel(), ref[0]) and np.array_equal(d_n.cpu().numpy().ravel(), ref[1]))
    out = {"vocabulary": {"k": BOW_K, "L": BOW_L, "nodes": int(len(voc[3])), "words": int((voc[3] >= 0).sum()), "node_descriptor_bytes": int(voc[2].nbytes),
                          "what": "synthetic complete tree in ORBvoc's shape (orb_slam2_e_amd/synth.py: synth_vocabulary); ORBvoc.txt itself is not in the reference mount",
                          "create_ms": create_ms},
           "descriptors": nd, "sets": BOW_SETS, "levelsup": 4, "launch_ms_avg": avg, "launch_ms_median": float(np.median(t)), "wall_ms_per_batch": wall_ms,
           "descriptors_per_s": nd / (wall_ms * 1e-3), "verified": ok,
           "roofline": {"bound": "hbm", "kernel": "k_bow_transform", "achieved": alg / (avg * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": alg / (avg * 1e-3) / 1e9 / HBM_PEAK_GBS, "traffic": None, "avg_launch_ms": avg, "alg_bytes_per_launch": alg,
                        "note": "algorithmic bytes per descriptor = L x k x 32 B of children descriptors + 32 B feature + 8 B out (1,960 B); the kernel "
                                "also reads a 16-byte record per child (its own children's range, node id, word id: +960 B). The whole tree "
                                "(35.6 + 17.8 MB) fits the 256-MiB Infinity Cache: a gather bound by round-trip latency x levels, not by HBM"}}
    tr = load_traffic().get("k_bow_transform")
    if tr:
        out["roofline"]["traffic"] = tr["hbm_bytes_per_launch"]; out["roofline"]["traffic_source"] = tr["source"]
        # `frac` above prices ALGORITHMIC bytes and exceeds 1: the tree's upper levels are served by L2 and the Infinity Cache.  What the
        # memory side really delivers (counter bytes over the same launch time):
        out["roofline"]["frac_of_counter_traffic"] = tr["hbm_bytes_per_launch"] / (avg * 1e-3) / 1e9 / HBM_PEAK_GBS
    if batch_only:      # (tools/bow_transform_prof.py: a trace in which every k_bow_transform launch is the 64 x 2000 one)
        out["verified"] = bool(ok)
        del v
        return out
    put_ms(out, "transform_2000_host_arrays_ms", lambda: v.descend(feats[0], 4), 50)
    desc, off = distinctive_case()
    got = ORBmatcher.distinctive_descriptors(desc, off)
    dd = {"map_points": int(len(off) - 1), "observations": int(off[-1]), "verified": bool(np.array_equal(got, oracle.distinctive_descriptors(desc, off))),
          "alg_bytes_per_call": int(off[-1]) * 32 + (len(off) - 1) * 4,
          "what": "MapPoint::ComputeDistinctiveDescriptors (MapPoint.cc:305-370) for 2000 map points of 2..40 observations in one call, host arrays in and out"}
    put_ms(dd, "call_ms", lambda: ORBmatcher.distinctive_descriptors(desc, off), 50)
    out["distinctive_descriptors"] = dd
    out["verified"] = bool(ok and dd["verified"])
    del v
    return out


def stereo_bench():
    """Config 5: one 1242x375 KITTI-shaped pair through the drop-in calls -- left and right ORBextractor::operator()
    (host image in, keypoints / descriptors out) and Frame::ComputeStereoMatches on the two resident pyramids."""
    from orb_slam2_e_amd import ComputeStereoMatches, ORBextractor
    from orb_slam2_e_amd.synth import synth_stereo_pair
    fx, bf = 718.856, 386.1448                      # Examples/Stereo/KITTI00-02.yaml:8,25
    mb = np.float32(bf) / np.float32(fx)
    left, right = synth_stereo_pair(0)
    eL, eR = ORBextractor(*PARAMS), ORBextractor(*PARAMS)

    # the reference extracts the two images on two threads (Frame.cc:78-81: threadLeft / threadRight, then join); distinct
    # extractor handles are concurrently usable and ctypes releases the GIL for the duration of a call
    from concurrent.futures import ThreadPoolExecutor
    pool = ThreadPoolExecutor(1)

    def frame():
        fr = pool.submit(eR, right)
        eL(left)
        fr.result()
        return ComputeStereoMatches(eL, eR, mb, np.float32(bf))

    u, d = frame()
    reps = 50
    t_all, t_all_best = (x * 1e-3 for x in batch_ms(frame, reps))
    # the same frame from ONE host thread: orbx_extract_pair enqueues both images' kernel chains before it waits for either
    from orb_slam2_e_amd import extract_pair
    def frame_one_call():
        extract_pair(eL, eR, left, right)
        return ComputeStereoMatches(eL, eR, mb, np.float32(bf))
    u1, d1 = frame_one_call()
    t_one, t_one_best = (x * 1e-3 for x in batch_ms(frame_one_call, reps)) if np.array_equal(u1, u) and np.array_equal(d1, d) else (float("nan"),) * 2
    t_st, t_st_best = (x * 1e-3 for x in batch_ms(lambda: ComputeStereoMatches(eL, eR, mb, np.float32(bf)), reps))
    pool.shutdown()
    out = {"pair": "1242x375, 2000 features per image", "stereo_frame_ms": t_all * 1e3, "stereo_frame_one_call_ms": t_one * 1e3,
           "compute_stereo_matches_ms": t_st * 1e3,
           "stereo_frame_ms_best": t_all_best * 1e3, "stereo_frame_one_call_ms_best": t_one_best * 1e3, "compute_stereo_matches_ms_best": t_st_best * 1e3,
           "threads": "left and right extraction on two host threads, as Frame.cc:78-81",
           "timing": "per-call latencies of this leg, the matcher loops and the LM trial: MEDIAN of the means of 10-call batches, `_best` = the best batch (batch_ms); Compute(1) phases: medians of 30 calls",
           "stereo_pairs_per_s": 1.0 / t_all, "matched": int((u >= 0).sum())}

    # ORBmatcher::SearchForTriangulation (ORBmatcher.cc:858-1024) on the pair's own keypoints as two keyframes one KITTI
    # baseline apart: the whole function through the Python mirror (co-iteration and rotation check on the host) and its
    # gated loop alone (orbm_match_triangulation: host arrays in, host arrays out)
    from orb_slam2_e_amd import ORBmatcher
    from orb_slam2_e_amd.synth import synth_keyframe_pair_case
    kL, dL = eL(left); kR, dR = eR(right)
    fv1, fv2, has1, has2, s1, s2, F12, ex, ey = synth_keyframe_pair_case(kL, dL, kR, dR, stereo1=u >= 0)
    sf, sg = eR.GetScaleFactors(), eR.GetScaleSigmaSquares()
    m = ORBmatcher(0.6, True)
    off, idx = ORBmatcher.feature_vector_candidates(len(kL), fv1, fv2)
    whole = lambda: m.SearchForTriangulation(kL, dL, fv1, has1, s1, kR, dR, fv2, has2, s2, F12, ex, ey, sf, sg, False)
    inner = lambda: m.match_triangulation(kL, dL, kR, dR, off, idx, has1, has2, s1, s2, F12, ex, ey, sf, sg, False)
    for name, fn in (("search_for_triangulation_ms", whole), ("search_for_triangulation_gated_loop_ms", inner)):
        put_ms(out, name, fn, reps)
    out["search_for_triangulation"] = {"keypoints": [len(kL), len(kR)], "candidates": int(len(idx)), "matches": int(whole()[1])}
    # ... and with the two keyframes resident in HBM (stereo = the frame's right coordinate; lists shared per node)
    from orb_slam2_e_amd import Frame
    tb = (0.0, 0.0, float(left.shape[1]), float(left.shape[0]))
    fL = Frame(kL, dL, tb, np.where(np.asarray(s1, bool), 1.0, -1.0).astype(np.float32))
    fR = Frame(kR, dR, tb, np.where(np.asarray(s2, bool), 1.0, -1.0).astype(np.float32))
    resident = lambda: m.frame_search_for_triangulation(fL, fv1, has1, fR, fv2, has2, F12, ex, ey, sf, sg, False)
    put_ms(out, "search_for_triangulation_resident_ms", resident, reps)
    out["search_for_triangulation"]["resident_equal"] = bool(np.array_equal(resident()[2], whole()[2]))
    fL.close(); fR.close()

    # the same path with the batch as the unit: 64 resident pairs, left and right extract_batch on two handles and ONE
    # orbx_stereo_match over all frames, everything queued on one stream
    import torch
    Bp = 64
    pairs = [synth_stereo_pair(100 + k) for k in range(4)]
    dl = torch.from_numpy(np.stack([pairs[k % 4][0] for k in range(Bp)])).cuda()
    dr = torch.from_numpy(np.stack([pairs[k % 4][1] for k in range(Bp)])).cuda()
    from orb_slam2_e_amd import stereo_download_batch, stereo_match_batch
    ts = torch.cuda.Stream(); st = ts.cuda_stream
    ts2 = torch.cuda.Stream(); st2 = ts2.cuda_stream
    bL, bR = ORBextractor(*PARAMS), ORBextractor(*PARAMS)
    Hs, Ws = pairs[0][0].shape

    def batch_step():
        # left and right extraction on two streams (they overlap as the pipeline contexts of the frames/s leg do), the matcher
        # on the left one: the library orders it behind the right extraction, and the next right extraction behind it, by events
        bL.extract_batch_device(dl.data_ptr(), Bp, Hs, Ws, st)
        bR.extract_batch_device(dr.data_ptr(), Bp, Hs, Ws, st2)
        stereo_match_batch(bL, bR, mb, np.float32(bf), st)

    for _ in range(3): batch_step()
    ts.synchronize(); ts2.synchronize()
    nb = 20
    t0 = time.perf_counter()
    for _ in range(nb): batch_step()
    ts.synchronize(); ts2.synchronize()
    t_b = (time.perf_counter() - t0) / nb
    U, D, cnt = stereo_download_batch(bL)
    # outside the timed region: the batch's first four frames are the four distinct pairs -- against the oracle
    import oracle
    ok = True
    for f in range(4):
        oL, oR = oracle.OrbOracle(*PARAMS), oracle.OrbOracle(*PARAMS)
        okL, odL = oL.extract(pairs[f][0]); okR, odR = oR.extract(pairs[f][1])
        ou, od, _ = oracle.stereo_matches(oL, oR, okL, odL, okR, odR, mb, np.float32(bf))
        n = int(cnt[f])
        ok = ok and n == len(okL) and np.array_equal(U[f, :n].view(np.uint32), ou.view(np.uint32)) and \
            np.array_equal(D[f, :n].view(np.uint32), od.view(np.uint32))
    out["batch"] = {"pairs": Bp, "ms_per_batch": t_b * 1e3, "pairs_per_s": Bp / t_b, "verified": bool(ok),
                    "what": "64 resident 1242x375 pairs: left and right extract_batch on two streams, one orbx_stereo_match over all frames on the left one (ordered by events inside the library)"}
    return out


PRECONDITION_STEPS = 300   # untimed steps in front of the SECOND timed region (ms_per_step_conditioned; see main())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-verify", action="store_true", help="skip the oracle comparison of one step's results (outside the timed region)")
    ap.add_argument("--no-gather", action="store_true")
    ap.add_argument("--gather-every", type=int, default=4,
                    help="N > 1: steps of a context whose records travel in one RCCL gather (default 4: every gather costs two "
                         "cross-stream dependencies of tens of microseconds each on this stack -- a quarter of them per step; partial "
                         "buckets are flushed before every barrier).  Not measurable on the one-GPU development box: tune against SCALE_rNN.json")
    ap.add_argument("--pipeline", type=int, default=3, help="independent contexts/streams the steps rotate over")
    ap.add_argument("--dist-backend", default="nccl", help="nccl (= RCCL) for real runs; gloo only to rehearse N>1 on one GPU")
    ap.add_argument("--no-host-io", action="store_true", help="skip the PCIe-inclusive leg (host images in, host results out)")
    ap.add_argument("--no-fem", action="store_true", help="skip the FEM, matcher-loop and stereo legs")
    ap.add_argument("--match-kernel", choices=["auto", "popcount"], default="auto",
                    help="all-pairs matcher: auto = FP4 matrix-core kernel (default), popcount = XOR + v_bcnt kernel; same results")
    ap.add_argument("--fem-meshes", type=int, default=256)
    ap.add_argument("--no-pin", action="store_true", help="N > 1: leave the ranks' CPU placement to the scheduler")
    ap.add_argument("--no-gather-sweep", action="store_true", help="N > 1: skip the short timed regions at other --gather-every values")
    ap.add_argument("--launch-timeout", type=float, default=None, help="--gpus N > 1 started without a launcher: seconds the N ranks may run")
    ap.add_argument("--full", action="store_true",
                    help="after the timed region, also run every other measurement and check (roofline, conditioned region, oracle "
                         "check, host-I/O, FEM / matcher-loop / BoW / stereo legs, CPU baseline); off: the headline line only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's results (rank 0's 64 frames: keypoints, descriptors, counts, match results) "
                         "as DIR/<name>.npy in float32")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("bench: --steps must be >= 1 and --warmup >= 0")

    # N > 1 and not yet a rank of a launcher: this process becomes the parent of N ranks (fresh child processes running this same
    # command line with RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* set) and relays rank 0's line.  Nothing above or in
    # `launch` imports torch or touches the GPU.
    from orb_slam2_e_amd import launch
    if args.gpus < 1:
        raise SystemExit("bench: --gpus must be >= 1")
    if launch.should_spawn(args.gpus):
        sys.exit(launch.run_parent(os.path.abspath(__file__), sys.argv[1:], args.gpus, timeout=args.launch_timeout))
    world = launch.check_world(args.gpus)    # a launcher's WORLD_SIZE must be what --gpus says
    # one rank, one set of cores -- before anything touches the GPU (the HIP runtime's threads inherit the mask)
    _lr = int(os.environ.get("LOCAL_RANK", "0"))
    affinity = None if args.no_pin else launch.pin_rank(_lr, world, dev_index=0 if args.dist_backend != "nccl" else _lr)   # (a gloo rehearsal puts every rank on GPU 0)

    import torch
    import torch.distributed as dist

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    rehearse = args.dist_backend != "nccl"   # all ranks on GPU 0, collectives staged through the CPU (gloo)
    dev_index = 0 if (world == 1 or rehearse) else local_rank
    if dev_index >= torch.cuda.device_count():   # (counting devices does not initialise the GPU)
        raise SystemExit(f"bench: rank {rank} needs GPU {dev_index}, this node shows {torch.cuda.device_count()} "
                         f"(--dist-backend gloo rehearses N > 1 with every rank on GPU 0)")
    torch.cuda.set_device(dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearse:
            dist.init_process_group(args.dist_backend)
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
    dev = torch.device("cuda", dev_index)
    cdev = torch.device("cpu") if rehearse else dev   # where collective payloads live

    from orb_slam2_e_amd import ORBextractor, ORBmatcher
    from orb_slam2_e_amd._lib import lib
    from orb_slam2_e_amd.shard import RecordLayout, ShardedPipeline, max_over_ranks
    from orb_slam2_e_amd.synth import synth_sequence

    # ---- inputs resident in HBM (weak scaling: each rank owns its own 64 frames = one camera pan over its own scene)
    frames = synth_sequence(BATCH, W, H, start=rank * BATCH)
    d_frames = torch.from_numpy(frames).to(dev)
    m = ORBmatcher(0.6)
    L = lib()
    if args.match_kernel == "popcount":
        ORBmatcher.set_allpairs_kernel(ORBmatcher.ALLPAIRS_POPCOUNT)
    qa = torch.arange(BATCH, dtype=torch.int32, device=dev)
    qb = ((qa + 1) % BATCH).to(torch.int32)

    # `--pipeline P` independent contexts (extractor workspace + result buffers + HIP stream): step k runs
    # on context k % P, so the latency-bound stages of one batch (pyramid, octree) overlap the VALU-bound
    # stages of the next (FAST, match).  Every step still does the full work on its own buffers.
    class Work:
        pass

    def make_context(c):
        u = Work()
        u.ex = ORBextractor(*PARAMS)
        # always a stream of its own, also for one context: handed the NULL stream the extractor and the matcher each fall back
        # to their own streams, and the match of step k then runs beside the extraction of step k + 1
        u.tstream = torch.cuda.Stream(device=dev)
        u.stream = u.tstream.cuda_stream
        cap = u.ex.capacity
        u.best = torch.empty((BATCH, cap), dtype=torch.int32, device=dev)
        u.second = torch.empty_like(u.best); u.idx = torch.empty_like(u.best); u.match12 = torch.empty_like(u.best)
        u.nmatch = torch.zeros(BATCH, dtype=torch.int32, device=dev)
        u.ex.extract_batch_device(d_frames.data_ptr(), BATCH, H, W, u.stream)  # sizes the workspace
        u.kps_p, u.desc_p, u.cnt_p, _ = u.ex.result_dev()
        return u

    def compute(c, k):
        u = c.user
        u.ex.extract_batch_device(d_frames.data_ptr(), BATCH, H, W, u.stream)
        m.match_batch_device(u.desc_p, u.cnt_p, cap, qa.data_ptr(), qb.data_ptr(), BATCH, u.best.data_ptr(),
                             u.second.data_ptr(), u.idx.data_ptr(), u.match12.data_ptr(), u.nmatch.data_ptr(),
                             stream=u.stream)

    def pack(c, dst):
        """fixed-size record {kps[CAP], desc[CAP][32], counts, match12[CAP], nmatch} of this step -> dst (device)"""
        u = c.user
        p0 = dst.data_ptr()
        L.orbx_copy_results_dev(u.ex._h, C.c_void_p(p0 + lay.o_kps), C.c_void_p(p0 + lay.o_desc), C.c_void_p(p0 + lay.o_cnt),
                                C.c_void_p(u.stream))
        dst[lay.o_m12:lay.o_nm].copy_(u.match12.view(torch.uint8).reshape(-1), non_blocking=True)
        dst[lay.o_nm:lay.rec_bytes].copy_(u.nmatch.view(torch.uint8).reshape(-1), non_blocking=True)

    cap = PARAMS[0] + 3 * PARAMS[2]
    lay = RecordLayout(BATCH, cap)
    captured = {}

    def on_receive(k, r, rec):
        if captured.get("want") == k:
            captured[r] = rec.cpu().clone()

    pipe = ShardedPipeline(rank, world, lay.rec_bytes, max(1, args.pipeline), args.gather_every, compute, pack,
                           make_context=make_context, stream_ctx=lambda c: torch.cuda.stream(c.user.tstream),
                           on_receive=None, send_device=dev, coll_device=cdev, enable_gather=not args.no_gather)
    # (rank 0 looks at the received records only for the checker step after the timed region: no per-record host work inside it)
    ctxs = [c.user for c in pipe.ctxs]
    assert ctxs[0].ex.capacity == cap
    GE = pipe.GE
    torch.cuda.synchronize()
    counts_t = torch.zeros(BATCH, dtype=torch.int32, device=dev)
    step = pipe.step

    def sync():
        pipe.flush()           # partial buckets: every step's records are on rank 0 before the barrier
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    # cold pass: every context's first step (module load, first-touch of its buffers) before anything is measured
    for k in range(len(pipe.ctxs)):
        step(k)
    sync()

    def read_profiles():
        kern = {}
        for c in ctxs:
            names = (C.c_char_p * 16)(); ms = (C.c_double * 16)(); ln = (C.c_int64 * 16)(); nk = C.c_int(0)
            L.orbx_profile_read(c.ex._h, 16, names, ms, ln, C.byref(nk))
            for i in range(nk.value):
                a, b = kern.get(names[i].decode(), (0.0, 0))
                kern[names[i].decode()] = (a + ms[i], b + ln[i])
        mm, ml = C.c_double(0), C.c_int64(0)
        L.orbm_profile_read(C.byref(mm), C.byref(ml))
        kern["k_match_sets_mfma"] = (mm.value, ml.value)
        return kern

    # untimed pass, one context, one step at a time: every run has it in front of the W warm-ups (a plain run as well -- the
    # clocks the K timed steps start from depend on it); --full puts events around every kernel: the per-kernel split and the
    # dominant kernel
    KINDS = [n for n in KERNEL_KINDS]
    dom = None
    if args.full:
        for c in ctxs:
            L.orbx_profile_enable(c.ex._h, -1)
        L.orbm_profile_enable(1)
    nprof = 3
    for k in range(nprof):      # one context, one step at a time: no overlap in the per-kernel split
        step(0)
        torch.cuda.synchronize()
    sync()
    if args.full:
        kern_all = read_profiles()
        split_ms = {k: v[0] / nprof for k, v in kern_all.items()}
        # a start/stop event pair inflates each measured launch by ~10-20 us (rocprof traces in profiles/); rank the
        # kinds by time net of 15 us per launch so that a multi-launch chain is not picked for its event overhead
        dom = max(split_ms, key=lambda k: split_ms[k] - 0.015 * kern_all[k][1] / nprof)
    # timed region of a --full run: events around the dominant kernel only (each event costs dispatch-gap time); a plain run has none
    def enable_dominant():      # (re-)arming also clears the accumulated times
        if dom is None:
            return
        for c in ctxs:
            L.orbx_profile_enable(c.ex._h, (1 << KINDS.index(dom)) if dom in KINDS else 0)
        L.orbm_profile_enable(1 if dom == "k_match_sets_mfma" else 0)

    # The contract's region: W warm-up steps, run exactly as the timed ones (pipelined, same events), then EXACTLY K timed steps
    # between barriers -- nothing else in front.  `value` / `ms_per_step` come from here (= `ms_per_step_unconditioned`).
    enable_dominant()
    for k in range(args.warmup):
        step(k)
    sync()
    enable_dominant()
    t0 = time.perf_counter()
    for k in range(args.steps):
        step(k)
    sync()
    dt = max_over_ranks(time.perf_counter() - t0, world, cdev)
    if args.full:
        kern = read_profiles()      # the dominant kernel's launch times of THIS region (HIP events on the launch stream)

    # what the last timed step computed, read before anything else runs on its context
    last = pipe.ctxs[(args.steps - 1) % len(pipe.ctxs)]
    L.orbx_copy_results_dev(last.user.ex._h, None, None, C.c_void_p(counts_t.data_ptr()), C.c_void_p(last.user.stream))
    torch.cuda.synchronize()
    counts, nmatch = counts_t, last.user.nmatch.clone()
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last, pack, lay, dev)

    # --full, beside the headline and never `value`: the same K steps after clock conditioning.  The passes above leave the card
    # nearly idle, and from there it takes tens of milliseconds of load to reach the clocks it then sustains -- a 20-step region
    # is 5-6 ms.  Measured on one box, 20 timed steps: 0.280-0.289 ms per step after W = 2 or 10 warm-up steps alone, 0.261-0.269
    # ms after 200 more.  So PRECONDITION_STEPS (~80 ms) of the same pipelined steps, W warm-ups again, and K timed steps:
    # `ms_per_step_conditioned` (rounds 3-4 reported THIS figure as `value`; the driver's --warmup could not see the preamble).
    if args.full:
        for k in range(PRECONDITION_STEPS):
            step(k)
        sync()
        for k in range(args.warmup):
            step(k)
        sync()
        t0 = time.perf_counter()
        for k in range(args.steps):
            step(k)
        sync()
        dt_cond = max_over_ranks(time.perf_counter() - t0, world, cdev)

    # N > 1, --full: the same steps at other gather cadences, short regions after the headline one (a single multi-GPU run then
    # tunes --gather-every; the headline keeps the value it was started with)
    sweep = None
    if args.full and world > 1 and pipe.do_gather and not args.no_gather_sweep:
        from orb_slam2_e_amd.shard import gather_sweep
        sweep = gather_sweep(pipe, sync, world, cdev, values=tuple(sorted({1, 4, 16, GE})))
    for c in ctxs:
        L.orbx_profile_enable(c.ex._h, 0)
    L.orbm_profile_enable(0)

    # ---- the checker (--full, outside the timed region): one more step on context 0, its results against the CPU oracle on
    # every rank; for N > 1 rank 0 also compares the records it received with the senders' own bytes (checksums)
    verified, verify_note = None, None
    if args.full and not args.no_verify:
        import hashlib
        captured["want"] = args.steps
        pipe.on_receive = on_receive
        step(args.steps)                        # args.steps % P need not be 0: any context does the full work
        sync()
        u = pipe.ctxs[args.steps % len(pipe.ctxs)].user
        rec = torch.empty(lay.rec_bytes, dtype=torch.uint8, device=dev)
        with torch.cuda.stream(u.tstream):
            pack(pipe.ctxs[args.steps % len(pipe.ctxs)], rec)
        torch.cuda.synchronize()
        rec_h = rec.cpu().numpy()
        R = lay.unpack(rec_h)
        best, second, idx = (t.cpu().numpy() for t in (u.best, u.second, u.idx))
        ok, why = verify_against_oracle(frames, R["kps"], R["desc"], R["counts"], best, second, idx, R["match12"], R["nmatch"],
                                        qb.cpu().numpy())
        digest = hashlib.sha256(rec_h.tobytes()).hexdigest()
        if world > 1:
            oks = [None] * world
            dist.all_gather_object(oks, (bool(ok), why, digest))
            ok = all(o[0] for o in oks)
            why = next((f"rank {r}: {o[1]}" for r, o in enumerate(oks) if not o[0]), None)
            if rank == 0 and pipe.do_gather:
                for r in range(world):
                    got = captured.get(r)
                    if got is None or hashlib.sha256(got.numpy().tobytes()).hexdigest() != oks[r][2]:
                        ok, why = False, f"record gathered from rank {r} differs from what that rank produced"
                        break
        verified, verify_note = bool(ok), why

    host_io = None
    if args.full and not args.no_host_io and rank == 0:
        # PCIe-inclusive rate: 64 host frames in, every frame's keypoints / descriptors / counts out.  (a) the plain
        # synchronous calls on pageable memory; (b) what a batch front-end does: pinned buffers, the upload, the kernels
        # and the download of a batch queued on one stream per context, contexts rotating.
        c = ctxs[0]
        c.ex.extract_batch(frames); c.ex.download_batch()
        t0 = time.perf_counter()
        reps = 10
        for _ in range(reps):
            c.ex.extract_batch(frames)
            c.ex.download_batch()
        rate_sync = reps * BATCH / (time.perf_counter() - t0)
        for c in ctxs:
            c.pin_in = torch.from_numpy(frames).pin_memory()
            c.d_in = torch.empty((BATCH, H, W), dtype=torch.uint8, device=dev)
            c.pin_kps = torch.empty(cap * 28 * BATCH, dtype=torch.uint8).pin_memory()
            c.pin_desc = torch.empty(cap * 32 * BATCH, dtype=torch.uint8).pin_memory()
            c.pin_cnt = torch.empty(BATCH, dtype=torch.int32).pin_memory()

        def io_step(k):
            c = ctxs[k % len(ctxs)]
            with torch.cuda.stream(c.tstream):
                c.d_in.copy_(c.pin_in, non_blocking=True)
                c.ex.extract_batch_device(c.d_in.data_ptr(), BATCH, H, W, c.stream)
                L.orbx_copy_results_dev(c.ex._h, C.c_void_p(c.pin_kps.data_ptr()), C.c_void_p(c.pin_desc.data_ptr()),
                                        C.c_void_p(c.pin_cnt.data_ptr()), C.c_void_p(c.stream))
        for k in range(30): io_step(k)
        torch.cuda.synchronize()
        reps = 300
        t0 = time.perf_counter()
        for k in range(reps): io_step(k)
        torch.cuda.synchronize()
        rate_pipe = reps * BATCH / (time.perf_counter() - t0)
        big_h = torch.empty(64 << 20, dtype=torch.uint8).pin_memory(); big_d = torch.empty(64 << 20, dtype=torch.uint8, device=dev)
        bw = {}
        for name, dst, src in (("h2d", big_d, big_h), ("d2h", big_h, big_d)):
            dst.copy_(src, non_blocking=True); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(5): dst.copy_(src, non_blocking=True)
            torch.cuda.synchronize()
            bw[name] = 5 * (64 << 20) / (time.perf_counter() - t0) / 1e9
        # (c) the live tracker's shape: ONE frame per call through ORBextractor::operator() -- host image in, keypoints and descriptors out
        one = ORBextractor(2000, 1.2, 8, 20, 7)
        for k in range(8): one(frames[k])
        call_ms = batch_ms(lambda: one(frames[3]), 200, warm=10)
        del one
        # (d) THIS fork's own settings (20 of its launch files: 1200 features, scale 1.1, 6 levels, FAST 24 / 7) at Hamlyn's frame size: one
        # frame per call, and 64 resident frames per batch (extract only, one context, events-free wall time)
        from orb_slam2_e_amd.synth import synth_frame
        fk = ORBextractor(1200, 1.1, 6, 24, 7)
        ff = np.stack([synth_frame(k, w=640, h=360) for k in range(BATCH)])
        for k in range(8): fk(ff[k])
        fork_call = batch_ms(lambda: fk(ff[3]), 200, warm=10)
        d_ff = torch.from_numpy(ff).to(dev)
        for _ in range(5): fk.extract_batch_device(d_ff.data_ptr(), BATCH, 360, 640)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(50): fk.extract_batch_device(d_ff.data_ptr(), BATCH, 360, 640)
        torch.cuda.synchronize()
        fork_rate = 50 * BATCH / (time.perf_counter() - t0)
        del fk, d_ff
        fork = {"settings": "ORBextractor(1200, 1.1, 6, 24, 7), 640x360 (roslaunch/sHamlyn*.yaml)", "one_frame_operator_call_ms": fork_call[0],
                "one_frame_operator_call_ms_best": fork_call[1], "frames_per_s_extract_only_resident_batches_of_64": fork_rate}
        host_io = {"pcie_pinned_copy_GBps": bw, "fork_settings": fork, "frames_per_s_extract_only_sync_pageable": rate_sync, "frames_per_s_extract_only_pinned_pipelined": rate_pipe,
                   "bytes_per_frame": W * H + cap * 60 + 4,
                   "one_frame_operator_call_ms": call_ms[0], "one_frame_operator_call_ms_best": call_ms[1],
                   "note": "64 host u8 frames in over PCIe, all keypoints+descriptors+counts out; no match; never `value`; one_frame_*: a "
                           "single 640x480 frame per ORBextractor::operator() call (pyramid levels 1.. in one launch: k_pyr_chain)"}
        for c in ctxs:
            del c.pin_in, c.d_in, c.pin_kps, c.pin_desc, c.pin_cnt

    fem = None
    fem_csr = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"orbx_bench_fem_csr_{os.getpid()}.npz")
    if args.full and not args.no_fem:
        fem = fem_bench(rank, world, dist, torch, dev, cdev, nmesh=args.fem_meshes, csr_out=fem_csr)
        if rank == 0:
            fem["compute1_per_frame"] = fem_compute1_bench()
            fem["compute1_all_reference_meshes"] = fem_compute1_all_meshes()

    if rank == 0:
        total_frames = world * BATCH * args.steps
        value = total_frames / dt
        out = {
            "metric": "frames/s ORB extract+match (640x480, 2000 feat)",
            "value": value, "unit": "frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "verified": verified,           # the oracle check runs in a --full run only (None: not checked)
            "full": bool(args.full),
            "config": {"workload": (f"{world}xMI355X: {world * BATCH}-frame batch sharded {BATCH}/GPU, " if world > 1 else
                                    f"1xMI355X: batch of {BATCH} ") + "synthetic 640x480 frames, ORB extract (2000 feat, 8 levels) "
                                   "+ 2000x2000 brute-force Hamming match per frame" +
                                   ((", gloo gather on rank 0 staged through the host (REHEARSAL: all ranks share GPU 0)" if rehearse else
                                     ", RCCL gather on rank 0") if world > 1 else ""),
                       "frames": "synth_sequence: each GPU's 64 frames are one camera pan (2, 1) px per frame over its own scene of "
                                 "rectangles and discs + per-frame noise; frame i is matched against frame i+1 mod 64",
                       "frames_per_gpu": BATCH, "global_batch": world * BATCH, "pipeline_contexts": len(ctxs),
                       "preconditioning_steps": 0,                    # in front of the region `value` is timed on: none since round 5
                       "allpairs_kernel": "k_match_sets (popcount)" if args.match_kernel == "popcount" else "k_match_sets_mfma_shared (FP4 matrix cores, train tiles shared through LDS)",
                       "parallelism": (f"frames sharded {BATCH}/rank, results gathered on rank 0 ({GE} steps per "
                                        f"{'gloo' if rehearse else 'RCCL'} gather)") if world > 1 else "single GPU",
                       "dist_backend": (args.dist_backend if world > 1 else None),
                       "rank0_cpu_affinity": affinity,
                       "mean_keypoints_per_frame": float(counts.float().mean().item()),
                       "mean_matches_per_frame": float(nmatch.float().mean().item())},
        }
        if verified is not None:
            out["verified_what"] = ("one step's keypoints (float bits), descriptors, best/second/arg-best, accepted matches and match counts "
                                    "of all frames of every rank == CPU oracle, outside the timed region" +
                                    ("; gathered records == the senders' bytes (sha256)" if world > 1 and pipe.do_gather else "") +
                                    (f"; FAILED: {verify_note}" if not verified else ""))
        if args.full:
            launches_per_step = max(kern[dom][1] // max(args.steps, 1), 1)
            avg_launch_ms = kern[dom][0] / max(kern[dom][1], 1)
            alg = ALG_BYTES[dom] * BATCH / launches_per_step  # algorithmic bytes per launch
            achieved = alg / (avg_launch_ms * 1e-3) / 1e9 if avg_launch_ms > 0 else 0.0
            out.update({
                "ms_per_step_unconditioned": dt / args.steps * 1e3,     # = ms_per_step: the K steps directly behind the W warm-ups
                "ms_per_step_conditioned": dt_cond / args.steps * 1e3,  # the same K steps after PRECONDITION_STEPS more untimed ones (never `value`)
                "value_conditioned": total_frames / dt_cond,
                "roofline": {"bound": "hbm", "kernel": dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                             "avg_launch_ms": avg_launch_ms, "alg_bytes_per_launch": alg},
                "pipeline_hbm_frac": value / world * FRAME_BYTES / 1e9 / HBM_PEAK_GBS,
                "kernel_ms_per_step_untimed_pass": split_ms,
            })
            out["config"]["preconditioning_steps_of_ms_per_step_conditioned"] = PRECONDITION_STEPS
            # the all-pairs matcher is the one contraction on the path: 2 x 256 FP4 multiply-adds per descriptor pair
            nk = counts.double().clamp(max=cap).cpu()
            pair_flops = 512.0 * float((nk[qa.cpu().long()] * nk[qb.cpu().long()]).sum())
            mm_ms = split_ms.get("k_match_sets_mfma", 0.0)
            if mm_ms > 0 and args.match_kernel != "popcount":
                out["matcher_mfma"] = {"kernel": "k_match_sets_mfma_shared", "bound": "mfma", "achieved": pair_flops / (mm_ms * 1e-3) / 1e12,
                                       "peak": MFMA_FP4_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": pair_flops / (mm_ms * 1e-3) / 1e12 / MFMA_FP4_PEAK_TFLOPS,
                                       "flops_per_launch": pair_flops, "launch_ms_untimed_pass": mm_ms,
                                       "note": "FP4 MFMA computes the selection keys; one key per MFMA result enters the running pair, the winner's group is finished with popcounts; bounded by matrix time + LDS round trips at two waves per SIMD"}
            if dom == "k_match_sets_mfma" and args.match_kernel != "popcount":
                tf = pair_flops / (avg_launch_ms * 1e-3) / 1e12
                out["roofline"].update({"bound": "mfma", "achieved": tf, "peak": MFMA_FP4_PEAK_TFLOPS, "unit": "TFLOP/s",
                                        "frac": tf / MFMA_FP4_PEAK_TFLOPS, "flops_per_launch": pair_flops})
            tr = load_traffic()   # HBM bytes per launch from the committed PMC passes (FETCH_SIZE x2 + WRITE_SIZE)
            if dom in tr:
                out["roofline"]["traffic"] = tr[dom]["hbm_bytes_per_launch"]
                out["roofline"]["traffic_source"] = tr[dom]["source"]
                if tr[dom].get("valu_wave_insts_per_launch"):
                    # the kernels that dominate this path are bound by integer VALU issue, not by HBM:
                    # the same launch time priced against the instruction count of the committed PMC pass
                    ginst = tr[dom]["valu_wave_insts_per_launch"] / (avg_launch_ms * 1e-3) / 1e9
                    out["roofline"]["valu"] = {"achieved": ginst, "peak": VALU_PEAK_GINST, "unit": "G wave64-instr/s",
                                               "frac": ginst / VALU_PEAK_GINST,
                                               "wave_insts_per_launch": tr[dom]["valu_wave_insts_per_launch"]}
            # avg_launch_ms is the kernel's launch-to-end time IN the pipelined run, where it shares the chip with the other two
            # contexts' kernels; the same two fractions for the kernel running by itself (the untimed one-context pass; its event
            # pair adds ~3 us to the time, so these are lower bounds)
            alone_ms = split_ms.get(dom, 0.0) / max(1, kern_all[dom][1] // nprof) if dom in kern_all else 0.0
            if alone_ms > 0 and out["roofline"]["bound"] == "hbm":
                out["roofline"]["alone"] = {"launch_ms": alone_ms, "frac": alg / (alone_ms * 1e-3) / 1e9 / HBM_PEAK_GBS}
                if dom in tr and tr[dom].get("valu_wave_insts_per_launch"):
                    out["roofline"]["alone"]["valu_frac"] = tr[dom]["valu_wave_insts_per_launch"] / (alone_ms * 1e-3) / 1e9 / VALU_PEAK_GINST
        if sweep is not None:
            out["gather_sweep"] = {"ms_per_step_by_gather_every": sweep, "gather_every_of_value": GE,
                                   "note": "24-step regions after the headline one, same steps, MAX over ranks"}
        if host_io is not None:
            out["host_io"] = host_io
        if fem is not None:
            out["fem"] = fem
            if verified is not None and "verified" in fem:
                out["verified"] = bool(verified and fem["verified"])
        if args.full and not args.no_fem:
            out["matcher_loops"] = matcher_loops_bench()
            out["bow_transform"] = bow_bench(torch, dev)
            out["stereo"] = stereo_bench()
            if out["verified"] is not None:
                out["verified"] = bool(out["verified"] and out["stereo"]["batch"]["verified"] and out["bow_transform"]["verified"])
        if args.full and not args.no_cpu_baseline:
            # (N > 1: rank 0 times the extract + match leg alone -- the others wait at the closing barrier; the FEM / stereo / loop
            # baselines belong to the N = 1 line)
            legs = ["extract"] + ([] if (args.no_fem or world > 1) else ["fem", "stereo", "loops", "bow"])
            cb = cpu_baseline_child(legs, fem_csr if os.path.exists(fem_csr) else None)
            out["cpu_baseline"] = cb.get("extract_match", cb)
            if "fem" in cb and fem is not None: out["fem"]["cpu_baseline"] = cb["fem"]
            if "stereo" in cb and "stereo" in out: out["stereo"]["cpu_baseline"] = cb["stereo"]
            if "matcher_loops" in cb and "matcher_loops" in out: out["matcher_loops"]["cpu_baseline"] = cb["matcher_loops"]
            if "bow_transform" in cb and "bow_transform" in out: out["bow_transform"]["cpu_baseline"] = cb["bow_transform"]
        if os.path.exists(fem_csr):
            os.unlink(fem_csr)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
