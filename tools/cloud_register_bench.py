#!/usr/bin/env python3
"""Point-to-point ICP (diffmvs_amd.cloud_register.icp) on a seeded pair of clouds of Tanks&Temples size: prints one JSON line
(profiles/cloud_register_line.json).

    python tools/cloud_register_bench.py [--source 10000000] [--target 10000000] [--iters 10] [--max_corr 0.5] [--reps 3] [--cpu 1]

The clouds: a rippled surface sampled at about 0.05 spacing (so 10^7 points cover a 160 x 160 patch), the source with 0.02 noise and 2 %
outliers, displaced by 1 degree and 0.2 units.  A FIXED number of iterations (rel_fitness = rel_rmse = 0: the stopping rule never
fires), so that both back ends do the same work.  Reported: the wall time of icp() between device events after a warm-up call, the
event-timed search and moments kernels per iteration, the rest (host closed form, transfers, the one-off grid build and sort), the
moments kernel's bytes per second against HBM, and -- if scipy can be imported -- the same ICP (same inputs, same iteration count)
with scipy.spatial.cKDTree(...).query(workers=16, distance_upper_bound=max_corr) on the CPU of the same box."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffmvs_amd import cloud_register as CR  # noqa: E402
from diffmvs_amd.ops import Ops  # noqa: E402

HBM_PEAK_GBS = 8000.0      # MI355X


def make_pair(n_src, n_tgt, dev, seed=0):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    side = 0.05 * math.sqrt(n_tgt)

    def surf(n, lo, hi):
        x = lo + (hi - lo) * torch.rand(n, generator=gen, device=dev, dtype=torch.float64)
        y = lo + (hi - lo) * torch.rand(n, generator=gen, device=dev, dtype=torch.float64)
        return torch.stack([x, y, 6 * torch.sin(x / 5) * torch.cos(y / 6) + 1.5 * torch.sin(x / 1.4 + y / 2.2) + 0.2 * x], -1)
    tgt = surf(n_tgt, 0.0, side)
    src = surf(n_src, 0.1 * side, 0.9 * side) + 0.02 * torch.randn(n_src, 3, generator=gen, device=dev, dtype=torch.float64)
    out = torch.randperm(n_src, generator=gen, device=dev)[:n_src // 50]
    src[out] += 3.0 * torch.randn(out.numel(), 3, generator=gen, device=dev, dtype=torch.float64)
    th = math.radians(1.0)
    R = torch.tensor([[math.cos(th), -math.sin(th), 0], [math.sin(th), math.cos(th), 0], [0, 0, 1]], dtype=torch.float64, device=dev)
    c = torch.tensor([side / 2, side / 2, 0], dtype=torch.float64, device=dev)
    src = (src - c) @ R.T + c + torch.tensor([0.12, -0.1, 0.12], dtype=torch.float64, device=dev)
    return src.float().contiguous(), tgt.float().contiguous()


def cpu_icp(src, tgt, max_corr, iters):
    from scipy.spatial import cKDTree
    t0 = time.perf_counter()
    tree = cKDTree(tgt)
    t_build = time.perf_counter() - t0
    T, s64, t_query = np.eye(4), src.astype(np.float64), 0.0
    for _ in range(iters + 1):
        moved = s64 @ T[:3, :3].T + T[:3, 3]
        q0 = time.perf_counter()
        d, i = tree.query(moved, workers=16, distance_upper_bound=max_corr)
        t_query += time.perf_counter() - q0
        ok = np.isfinite(d)
        fitness, rmse = ok.mean(), math.sqrt((d[ok] ** 2).mean())
        T = CR.umeyama(moved[ok], tgt[i[ok]].astype(np.float64), with_scale=False) @ T
    return {"seconds": round(time.perf_counter() - t0, 2), "build_seconds": round(t_build, 2), "query_seconds": round(t_query, 2), "workers": 16,
            "fitness": float(fitness), "inlier_rmse": float(rmse)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--source", type=int, default=10000000)
    ap.add_argument("--target", type=int, default=10000000)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--max_corr", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu", type=int, default=1)
    a = ap.parse_args()
    ops = Ops.for_device("cuda:0")
    src, tgt = make_pair(a.source, a.target, ops.device)
    kw = dict(max_corr=a.max_corr, max_iter=a.iters, rel_fitness=0.0, rel_rmse=0.0)
    res = CR.icp(ops, src, tgt, **kw)          # warm-up
    torch.cuda.synchronize()
    names = {"search": "dmvs_cloud_nn_index_f32", "moments": "dmvs_cloud_pair_moments_f64"}
    walls, splits = [], []
    try:
        for _ in range(a.reps):
            ops.timers = {n: [] for n in names.values()}
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.record()
            res = CR.icp(ops, src, tgt, **kw)
            en.record()
            torch.cuda.synchronize()
            walls.append(st.elapsed_time(en))
            splits.append({k: [s.elapsed_time(e) for s, e in ops.timers[n]] for k, n in names.items()})
    finally:
        ops.timers = None
    i = int(np.argmin(walls))
    search, moments = splits[i]["search"], splits[i]["moments"]
    launches = len(search)
    mom_ms = float(np.median(moments))
    mom_bytes = a.source * (12 + 4 + 12)          # source, index, one gathered target per point
    line = {"metric": "ICP wall ms (icp: grid build + source sort + %d evaluations)" % launches,
            "command": "python tools/cloud_register_bench.py " + " ".join(sys.argv[1:]),
            "workload": {"source_points": a.source, "target_points": a.target, "iterations": a.iters, "max_corr": a.max_corr, "outliers": 0.02},
            "wall_ms": round(walls[i], 2), "wall_ms_all": [round(w, 2) for w in walls], "reps": a.reps,
            "per_iteration_ms": {"search": round(float(np.median(search)), 3), "search_first": round(search[0], 3), "moments": round(mom_ms, 3),
                                 "host_and_rest": round((walls[i] - sum(search) - sum(moments)) / launches, 3)},
            "moments_roofline": {"bound": "hbm", "algorithmic_bytes": mom_bytes, "achieved_GBs": round(mom_bytes / (mom_ms * 1e-3) / 1e9, 1),
                                 "peak_GBs": HBM_PEAK_GBS, "frac": round(mom_bytes / (mom_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 3)},
            "result": {k: res[k] for k in ("fitness", "inlier_rmse", "iterations", "pairs")}}
    line["cpu_kdtree"] = "not measured"
    if a.cpu:
        try:
            import scipy.spatial  # noqa: F401
            cpu = cpu_icp(src.cpu().numpy(), tgt.cpu().numpy(), a.max_corr, a.iters)
            cpu["ratio_to_wall"] = round(cpu["seconds"] * 1e3 / walls[i], 1)
            line["cpu_kdtree"] = cpu
        except ImportError:
            pass
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
