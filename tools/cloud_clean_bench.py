#!/usr/bin/env python3
"""Point-cloud cleaning (dmvs_cloud_knn_f32, diffmvs_amd.cloud_clean) on the vertices of the project's own mesh: prints one JSON line
(profiles/cloud_clean_line.json).

    python tools/cloud_clean_bench.py [--views 49] [--size 864 1152] [--dim 512] [--reps 5] [--out FILE]

The cloud is the vertex set of the mesh tools/mesh_clean_bench.py extracts (the scene of tools/tsdf_bench.py fused at --dim^3 voxels):
a surface sample at about the voxel spacing, the density a fused cloud has.  Timed with device events (the outputs come from torch's
caching allocator, warm after the first call), the median of --reps after a warm-up:
  the search kernel alone as a self search at k = 8 and k = 16 on the grid clean() would build (cell = twice the estimated spacing,
  max_dist = NEAR_RINGS cells), with the targets it tested per query from its `work` output;
  dmvs_cloud_nn_index_f32 as a self search WITHOUT self-exclusion on the same grid (every query finds itself at distance 0 in its own
  cell): the floor of the walk, which the k-best list adds to;
and on the wall clock, synchronised at both ends, the whole clean(knn = 8) call (spacing estimate, sort, search, statistics, mask).
Beside them the only other way to these numbers on the machine: scipy.spatial.cKDTree(points).query(points, k + 1, workers = 16) on the
host, including the device-to-host copy and the build of the tree; the GPU's neighbour distances are compared with the tree's."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tsdf_bench as TB  # noqa: E402
import mesh_clean_bench as MB  # noqa: E402
from diffmvs_amd import cloud_clean as CC, cloud_grid as G  # noqa: E402
from diffmvs_amd.ops import Ops  # noqa: E402


def work_stats(wk):
    w = wk.double()
    return {"rings_mean": round(float(w[:, 0].mean()), 2), "targets_tested_mean": round(float(w[:, 1].mean()), 1), "targets_tested_max": int(wk[:, 1].max())}


def host_knn(points_dev, k):
    """-> (distances [N,k] to the k nearest others, seconds) or (None, None) without scipy"""
    try:
        from scipy.spatial import cKDTree
    except ImportError:
        return None, None
    t0 = time.perf_counter()
    p = points_dev.cpu().numpy()
    d = cKDTree(p).query(p, k + 1, workers=16)[0][:, 1:]
    return d, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--size", type=int, nargs=2, default=[864, 1152], help="H W")
    ap.add_argument("--dim", type=int, default=512, help="the volume the mesh is extracted from has this many voxels a side")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    ops = Ops.for_device("cuda:0")
    verts, faces, h = MB.own_mesh(ops, a)
    del faces
    pts = verts.contiguous()
    N = int(pts.shape[0])
    cell = CC.default_cell(pts)
    md = float(np.float32(G.NEAR_RINGS * cell))
    grid = G.build_grid(pts, cell)
    args = (grid["target"], grid["target"], grid["keys"], grid["start"], grid["origin"], grid["cell"], grid["dims"], md)
    me = torch.arange(N, dtype=torch.int32, device=pts.device)

    # ---- the floor: the nearest search on the same grid
    ops.cloud_nn_index(*args, work=True)
    nn_ms = TB.timed(lambda: ops.cloud_nn_index(*args), a.reps)
    nn_work = work_stats(ops.cloud_nn_index(*args, work=True)[2])

    # ---- the k-best search
    knn = {}
    for k in (8, 16):
        res = ops.cloud_knn(*args, k, self_index=me, d2=True, work=True)
        ms = TB.timed(lambda: ops.cloud_knn(*args, k, self_index=me), a.reps)
        host_d, host_s = host_knn(grid["target"], k)
        row = {"ms": round(ms, 3), "queries_per_s": round(N / (ms * 1e-3)), "over_nearest": round(ms / nn_ms, 2), **work_stats(res["work"]),
               "found_all_k": int((res["found"] == k).sum())}
        if host_d is not None:
            full = (res["found"] == k).cpu().numpy()
            gpu_d = np.sqrt(res["d2"].cpu().numpy().astype(np.float64))
            row["host"] = {"how": "scipy.spatial.cKDTree.query(k + 1, workers=16)", "s": round(host_s, 3), "includes": "the device-to-host copy and the tree",
                           "over_gpu": round(host_s * 1e3 / ms, 1),
                           "max_abs_difference_of_the_distances": float(np.abs(gpu_d[full] - host_d[full]).max()) if full.any() else None}
        knn[str(k)] = row

    # ---- the whole call
    def whole():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = CC.clean(ops, pts, knn=8, std_ratio=2.0)
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3
    whole()
    runs = [whole() for _ in range(a.reps)]
    info = runs[-1][0][4]

    shown = [w for i, w in enumerate(sys.argv[1:]) if w != "--out" and (i == 0 or sys.argv[i] != "--out")]
    line = {"metric": "k nearest neighbours of every point of a cloud / statistical outlier removal, ms",
            "command": ("python tools/cloud_clean_bench.py " + " ".join(shown)).strip(), "reps": a.reps, "voxels": a.dim ** 3, "voxel": h, "points": N,
            "cell": cell, "max_dist": md, "occupied_cells": int(grid["keys"].numel()),
            "nearest_self_search": {"ms": round(nn_ms, 3), **nn_work}, "knn": knn,
            "clean_knn8_wall_ms": round(float(np.median([r[1] for r in runs])), 2), "clean_info": info}
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
