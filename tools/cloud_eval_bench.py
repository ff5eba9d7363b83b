#!/usr/bin/env python3
"""Point-cloud scoring (diffmvs_amd.cloud_eval.evaluate) on seeded clouds of a DTU-like size: prints one JSON line
(profiles/cloud_eval_line.json).

    python tools/cloud_eval_bench.py [--pred 20000000] [--gt 5000000] [--density 0.2] [--max_dist 20] [--outliers 0.02] [--reps 3] [--cpu 1]

The clouds: a rippled, tilted surface sampled at about one raw prediction point per `density` voxel (so that the thinning has
work to do) with 0.1 noise, the ground truth on the same surface, and `outliers` of the prediction displaced by 25 .. 100,
beyond max_dist.  Surfaces with noise, not uniform volumes: what a cell holds, and how early a query stops, depends on it.
Reported: the wall time of evaluate() between device events after a warm-up, the event-timed kernels, the share of the wall time
that is torch sorting, the early-exit figures of both searches, and -- if scipy can be imported -- the same two searches with
scipy.spatial.cKDTree(...).query(workers=16, distance_upper_bound=max_dist) on the CPU of the same box."""
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
from diffmvs_amd import cloud_eval as CE  # noqa: E402
from diffmvs_amd.ops import Ops  # noqa: E402


def make_surface(n, side, gen, dev):
    x = torch.rand(n, generator=gen, device=dev, dtype=torch.float64) * side
    y = torch.rand(n, generator=gen, device=dev, dtype=torch.float64) * side
    z = 300 + 0.3 * x - 0.2 * y + 15 * torch.sin(x / 40) * torch.cos(y / 55)
    return torch.stack([x, y, z], -1)


def make_clouds(n_pred, n_gt, density, outliers, dev, seed=0):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    side = density * math.sqrt(n_pred)
    pred = make_surface(n_pred, side, gen, dev) + 0.1 * torch.randn(n_pred, 3, generator=gen, device=dev, dtype=torch.float64)
    n_out = int(outliers * n_pred)
    v = torch.randn(n_out, 3, generator=gen, device=dev, dtype=torch.float64)
    v = v / v.norm(dim=1, keepdim=True) * (25 + 75 * torch.rand(n_out, 1, generator=gen, device=dev, dtype=torch.float64))
    pred[torch.randperm(n_pred, generator=gen, device=dev)[:n_out]] += v
    return pred.float().contiguous(), make_surface(n_gt, side, gen, dev).float().contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pred", type=int, default=20000000)
    ap.add_argument("--gt", type=int, default=5000000)
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--max_dist", type=float, default=20.0)
    ap.add_argument("--outliers", type=float, default=0.02)
    ap.add_argument("--thresholds", type=float, nargs="*", default=[0.5, 1.0, 2.0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cpu", type=int, default=1)
    a = ap.parse_args()
    ops = Ops.for_device("cuda:0")
    pred, gt = make_clouds(a.pred, a.gt, a.density, a.outliers, ops.device)

    sort_events, real_sort = [], torch.sort

    def timed_sort(*args, **kw):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        out = real_sort(*args, **kw)
        en.record()
        sort_events.append((st, en))
        return out

    res = CE.evaluate(ops, pred, gt, a.max_dist, a.thresholds, density=a.density)          # warm-up
    torch.cuda.synchronize()
    names = ("dmvs_cloud_nn_dist_f32", "dmvs_cloud_stats_f32")
    walls, kernels, sorts = [], {n: [] for n in names}, []
    torch.sort = timed_sort
    try:
        for _ in range(a.reps):
            ops.timers = {n: [] for n in names}
            sort_events.clear()
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.record()
            res = CE.evaluate(ops, pred, gt, a.max_dist, a.thresholds, density=a.density)
            en.record()
            torch.cuda.synchronize()
            walls.append(st.elapsed_time(en))
            for n in names:
                kernels[n].append(sum(s.elapsed_time(e) for s, e in ops.timers[n]))
            sorts.append(sum(s.elapsed_time(e) for s, e in sort_events))
    finally:
        torch.sort = real_sort
        ops.timers = None
    # the early-exit figures of both searches (untimed: the work output costs a store per query)
    thinned = CE.voxel_downsample(pred, a.density)[0].contiguous()
    exits = {}
    for name, q, t in (("pred_to_gt", thinned, gt), ("gt_to_pred", gt, thinned)):
        exits[name] = {}
        CE.nn_distance(ops, q, t, a.max_dist, cell=2.0 * a.density, stats=exits[name])
    i = int(np.argmin(walls))
    line = {"metric": "cloud scoring wall ms (evaluate: thinning + two searches + statistics)",
            "workload": {"pred_points": a.pred, "pred_points_thinned": res["pred"]["points"], "gt_points": a.gt, "density": a.density,
                         "max_dist": a.max_dist, "outliers": a.outliers, "thresholds": a.thresholds},
            "wall_ms": round(walls[i], 2), "wall_ms_all": [round(w, 2) for w in walls], "reps": a.reps,
            "kernel_ms": {"nn_dist": round(kernels[names[0]][i], 2), "stats": round(kernels[names[1]][i], 3)},
            "sort_ms": round(sorts[i], 2), "sort_share_of_wall": round(sorts[i] / walls[i], 3),
            "early_exit": exits,
            "scores": {k: res[k] for k in ("accuracy", "completeness", "overall", "precision", "recall", "fscore")},
            "out_of_range": {"pred": res["pred"]["out_of_range"], "gt": res["gt"]["out_of_range"]}}
    line["cpu_kdtree"] = "not measured"
    if a.cpu:
        try:
            from scipy.spatial import cKDTree
        except ImportError:
            cKDTree = None
        if cKDTree is not None:
            p, g = thinned.cpu().numpy(), gt.cpu().numpy()
            t0 = time.perf_counter()
            d1 = cKDTree(g).query(p, workers=16, distance_upper_bound=a.max_dist)[0]
            d2 = cKDTree(p).query(g, workers=16, distance_upper_bound=a.max_dist)[0]
            cpu_s = time.perf_counter() - t0
            gpu_search_ms = kernels[names[0]][i] + sorts[i]
            acc = float(d1[np.isfinite(d1)].mean())
            line["cpu_kdtree"] = {"seconds": round(cpu_s, 2), "workers": 16, "what": "build + query of both trees on the thinned prediction and the ground truth",
                                  "ratio_to_wall": round(cpu_s * 1e3 / walls[i], 1), "ratio_to_sorts_plus_nn_kernels": round(cpu_s * 1e3 / gpu_search_ms, 1),
                                  "accuracy": acc, "completeness": float(d2[np.isfinite(d2)].mean())}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
