#!/usr/bin/env python3
"""Depth maps from a cloud (diffmvs_amd.cloud_render) at DTU size: prints one JSON line (profiles/cloud_render_line.json).

    python tools/cloud_render_bench.py [--points 10000000] [--views 49] [--size 1152 1600] [--reps 3] [--host_views 2] [--referee_views 2] [--out FILE]

The cloud: a rippled, slanted surface sampled at random (10^7 points over 800 x 640 units: 0.23 units apart, 1.5 points per pixel), in the
order of cloud_render.sort_for_locality; the cameras: synth.synth_scene's 7-wide rig (30 units apart, turned towards the scene) with
f = 1.2 W.  Reported, event-timed on the launch stream after a warm-up pass and as the median of --reps: the z-min pass with and without
the pre-test, the sum pass and the resolve; point-views per second; footprint pixels and atomics issued (the kernel's own `work` counters)
per second; the bytes the passes are MODELLED to move (points once per launch of 8 views, a 4-byte load per footprint pixel, 4 / 12 bytes per
atomic) -- no counter pass was taken.  Two yardsticks, neither a pass/fail threshold:
  torch   zbuf.scatter_reduce_("amin") on the same device for the single-pixel case radius = 0, r_min = r_max = 0.5 (one pixel per point:
          ceil(u - 0.5); with r_min = 0 the contract's footprint ceil(u) .. floor(u) is empty), with and without the fp64 projection that
          produces its indices.  The line says how many pixels of the two z-buffers differ (`differing_pixels`, per-run) and, for
          --referee_views views (the first that differ, else the first and the last), how many pixels of EACH side differ from a numpy fp64
          rendering of all points on the host (`numpy_referee`): a ratio against a result that is not the same is not a yardstick;
  numpy   the fp64 restatement of include/dmvs.h on the host at 1/100 of the points and --host_views views, scaled to the full job."""
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
from diffmvs_amd import _lib, cloud_render as R  # noqa: E402
from diffmvs_amd.cloud_grid import pow2_scale_below  # noqa: E402
from diffmvs_amd.ops import Ops  # noqa: E402


def cameras(V, H, W, grid_w=7):
    K = np.array([[1.2 * W, 0, W / 2.0], [0, 1.2 * W, H / 2.0], [0, 0, 1.0]])
    grid = np.array([(v % grid_w, v // grid_w) for v in range(V)], np.float64)
    E = np.zeros((V, 4, 4))
    for v, (gx, gy) in enumerate(grid - grid.mean(0)):
        ay, ax = 0.05 * gx, -0.02 * gy
        Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        E[v] = np.eye(4)
        E[v, :3, :3], E[v, :3, 3] = Rx @ Ry, [-30.0 * gx, -30.0 * gy, 0.0]
    return np.repeat(K[None], V, 0), E


def surface(n, dev, seed=0):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    x = -400.0 + 800.0 * torch.rand(n, generator=gen, device=dev, dtype=torch.float64)
    y = -320.0 + 640.0 * torch.rand(n, generator=gen, device=dev, dtype=torch.float64)
    z = 650.0 + 0.15 * x - 0.1 * y + 12.0 * torch.sin(x / 40.0) * torch.cos(y / 55.0)
    return torch.stack([x, y, z], -1).float().contiguous()


def timed(fn, reps):
    """median milliseconds of fn() between events on the current stream, and its last result"""
    ms, out = [], None
    for _ in range(reps):
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.record()
        out = fn()
        en.record()
        torch.cuda.synchronize()
        ms.append(st.elapsed_time(en))
    return float(np.median(ms)), out


def torch_single_pixel(pts, table, H, W):
    """the single-pixel z-min with torch: fp64 projection in the contract's order, then scatter_reduce(amin).  -> (zbuf, projection ms, scatter ms)"""
    V = table.shape[0]
    zbuf = torch.full((V * H * W,), float("inf"), dtype=torch.float32, device=pts.device)
    X, Y, Z = (pts[:, i].double() for i in range(3))
    t_proj = t_scat = 0.0
    for k in range(V):
        q = [float(v) for v in table[k]]

        def project():
            x = ((q[0] * X + q[1] * Y) + q[2] * Z) + q[3]
            y = ((q[4] * X + q[5] * Y) + q[6] * Z) + q[7]
            z = ((q[8] * X + q[9] * Y) + q[10] * Z) + q[11]
            col, row = torch.ceil(x / z - 0.5), torch.ceil(y / z - 0.5)
            ok = (z > q[13]) & (z <= q[14]) & (col >= 0) & (col <= W - 1) & (row >= 0) & (row <= H - 1) & (col <= torch.floor(x / z + 0.5)) & \
                (row <= torch.floor(y / z + 0.5))
            return (k * H * W + row.long() * W + col.long())[ok], z.float()[ok]
        ms, (idx, z32) = timed(project, 1)
        t_proj += ms
        ms, _ = timed(lambda: zbuf.scatter_reduce_(0, idx, z32, "amin", include_self=True), 1)
        t_scat += ms
    return zbuf.view(V, H, W), t_proj, t_scat


def numpy_single_pixel(points, table, H, W, views, kernel, other):
    """the referee of yardstick 1: the single-pixel z-min of `views` in numpy fp64 on the host, ALL points, against both z-buffers.
    -> per view {view, seen, kernel_differs, torch_differs, two_pixel_points (u or v exactly at .5: the contract draws both)}"""
    X, Y, Z = (points[:, i].astype(np.float64) for i in range(3))
    out = []
    for k in views:
        q = table[k]
        with np.errstate(all="ignore"):
            x, y, z = ((q[0] * X + q[1] * Y) + q[2] * Z) + q[3], ((q[4] * X + q[5] * Y) + q[6] * Z) + q[7], ((q[8] * X + q[9] * Y) + q[10] * Z) + q[11]
            u, v = x / z, y / z
            c0, c1 = np.fmax(np.ceil(u - 0.5), 0.0), np.fmin(np.floor(u + 0.5), W - 1.0)
            r0, r1 = np.fmax(np.ceil(v - 0.5), 0.0), np.fmin(np.floor(v + 0.5), H - 1.0)
            on = np.isfinite(X + Y + Z) & (z > q[13]) & (z <= q[14]) & np.isfinite(u) & np.isfinite(v) & (c0 <= c1) & (r0 <= r1)
        z32 = z.astype(np.float32)[on]
        ref = np.full(H * W, np.inf, np.float32)
        for cc, rr in ((c0, r0), (c1, r0), (c0, r1), (c1, r1)):
            np.minimum.at(ref, rr[on].astype(np.int64) * W + cc[on].astype(np.int64), z32)
        ref = ref.reshape(H, W).view(np.uint32)
        out.append({"view": int(k), "seen": int((ref != 0x7f800000).sum()), "kernel_differs": int((kernel[k].view(np.uint32) != ref).sum()),
                    "torch_differs": int((other[k].view(np.uint32) != ref).sum()), "two_pixel_points": int((on & ((c1 > c0) | (r1 > r0))).sum())})
    return out


def numpy_restatement(points, table, H, W, radius, r_min, r_max, tau, scale):
    """include/dmvs.h in numpy fp64 with a loop over the drawn points: both passes.  -> seconds"""
    t0 = time.perf_counter()
    X, Y, Z = (points[:, i].astype(np.float64) for i in range(3))
    for q in table:
        zbuf, total, cnt = np.full((H, W), np.inf, np.float32), np.zeros((H, W), np.int64), np.zeros((H, W), np.int32)
        with np.errstate(all="ignore"):
            x, y, z = ((q[0] * X + q[1] * Y) + q[2] * Z) + q[3], ((q[4] * X + q[5] * Y) + q[6] * Z) + q[7], ((q[8] * X + q[9] * Y) + q[10] * Z) + q[11]
            u, v = x / z, y / z
            r = np.fmin(np.fmax(radius * q[12] / z, r_min), r_max)
            c0, c1 = np.fmax(np.ceil(u - r), 0.0), np.fmin(np.floor(u + r), W - 1.0)
            r0, r1 = np.fmax(np.ceil(v - r), 0.0), np.fmin(np.floor(v + r), H - 1.0)
            on = np.isfinite(X + Y + Z) & (z > q[13]) & (z <= q[14]) & np.isfinite(u) & np.isfinite(v) & (c0 <= c1) & (r0 <= r1)
        z32 = z.astype(np.float32)
        idx = np.nonzero(on)[0]
        box = [(int(r0[i]), int(r1[i]) + 1, int(c0[i]), int(c1[i]) + 1) for i in idx]
        for i, (a, b, c, d) in zip(idx, box):
            np.minimum(zbuf[a:b, c:d], z32[i], out=zbuf[a:b, c:d])
        fixed = np.rint(z32[idx].astype(np.float64) * scale).astype(np.int64)
        for i, f, (a, b, c, d) in zip(idx, fixed, box):
            m = np.float64(z32[i]) <= zbuf[a:b, c:d].astype(np.float64) * (1.0 + tau)
            total[a:b, c:d][m] += f
            cnt[a:b, c:d][m] += 1
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=10000000)
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--size", type=int, nargs=2, default=[1152, 1600], help="H W")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host_views", type=int, default=2)
    ap.add_argument("--r_min", type=float, default=0.5)
    ap.add_argument("--r_max", type=float, default=8.0)
    ap.add_argument("--tau", type=float, default=0.01)
    ap.add_argument("--referee_views", type=int, default=2, help="views of the single-pixel case that numpy re-renders on the host from all points")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    ops = Ops.for_device("cuda:0")
    (H, W), V, N = a.size, a.views, a.points
    K, E = cameras(V, H, W)
    pts = R.sort_for_locality(surface(N, ops.device))
    radius = math.sqrt(800.0 * 640.0 / N)                      # the sampling's own spacing
    table = R.view_table(K, E, 100.0, 2000.0)
    scale = pow2_scale_below(2000.0, N)
    launches = -(-V // _lib.SPLAT_VIEW_CHUNK)
    zbuf = torch.empty(V, H, W, dtype=torch.float32, device=ops.device)

    def zmin(pretest, rad=radius, r_min=a.r_min, r_max=a.r_max):
        zbuf.fill_(float("inf"))                               # (inside the timed region: part of the pass)
        return ops.cloud_splat_zmin(pts, table, (H, W), rad, r_min, r_max, zbuf=zbuf, pretest=pretest, work=True)
    zmin(True)                                                 # warm-up
    torch.cuda.synchronize()
    ms_pre, (_, counts, wk_pre) = timed(lambda: zmin(True), a.reps)
    wk_pre = wk_pre.cpu().tolist()
    nearest = torch.where(torch.isinf(zbuf), torch.zeros_like(zbuf), zbuf)
    ms_nopre, (_, _, wk_nopre) = timed(lambda: zmin(False), a.reps)
    wk_nopre = wk_nopre.cpu().tolist()
    same = bool(torch.equal(torch.where(torch.isinf(zbuf), torch.zeros_like(zbuf), zbuf).view(torch.int32), nearest.view(torch.int32)))
    ms_sum, (total, cnt) = timed(lambda: ops.cloud_splat_sum(pts, table, (H, W), radius, a.r_min, a.r_max, zbuf, a.tau, scale), a.reps)
    ms_res, mean = timed(lambda: R.resolve_mean(total, cnt, scale), a.reps)
    adds = int(cnt.sum())
    drawn = N * V - int(counts[:, :3].sum())
    covered = float((cnt > 0).float().mean())
    del total, cnt, mean, nearest
    # yardstick 1: the single-pixel case against torch
    ms_single, (_, _, wk_single) = timed(lambda: zmin(True, 0.0, 0.5, 0.5), a.reps)
    single = zbuf.clone()
    tz, t_proj, t_scat = torch_single_pixel(pts, table, H, W)
    differing = (tz.view(torch.int32) != single.view(torch.int32)).flatten(1).sum(1).cpu().tolist()
    single_same = sum(differing) == 0
    referee = numpy_single_pixel(pts.cpu().numpy(), table, H, W, ([k for k in range(V) if differing[k]] or [0, V - 1])[:a.referee_views],
                                 single.cpu().numpy(), tz.cpu().numpy())
    del tz, single
    # yardstick 2: the numpy restatement on the host, 1/100 of the points and a few views, scaled
    hv = max(1, min(a.host_views, V))
    sub = pts[::100].cpu().numpy()
    host_s = numpy_restatement(sub, table[:hv], H, W, radius, a.r_min, a.r_max, a.tau, scale)
    host_scaled = host_s * (N / len(sub)) * (V / hv)
    pv = N * V
    shown = [w for i, w in enumerate(sys.argv[1:]) if w != "--out" and (i == 0 or sys.argv[i] != "--out")]
    gb = lambda b: round(b / 1e9, 2)  # noqa: E731
    line = {"metric": "cloud -> depth maps, ms per pass over all views",
            "command": ("python tools/cloud_render_bench.py " + " ".join(shown)).strip(),      # (without --out: where the line goes is not the workload)
            "workload": {"points": N, "views": V, "size": [H, W], "radius": round(radius, 4), "r_min": a.r_min, "r_max": a.r_max, "tau": a.tau,
                         "views_per_launch": _lib.SPLAT_VIEW_CHUNK, "launches_per_pass": launches, "covered": round(covered, 4),
                         "drawn_point_views": drawn, "footprint_pixels": wk_pre[0]},
            "reps": a.reps,
            "nearest_ms": {"zmin": round(ms_pre, 2)}, "mean_ms": {"zmin": round(ms_pre, 2), "sum": round(ms_sum, 2), "resolve": round(ms_res, 2),
                                                                  "total": round(ms_pre + ms_sum + ms_res, 2)},
            "point_views_per_s": {"nearest": round(pv / (ms_pre * 1e-3), 0), "mean": round(pv / ((ms_pre + ms_sum + ms_res) * 1e-3), 0)},
            "zmin_pass": {"with_pretest": {"ms": round(ms_pre, 2), "atomics": wk_pre[1], "atomics_per_s": round(wk_pre[1] / (ms_pre * 1e-3), 0),
                                           "footprint_pixels_per_s": round(wk_pre[0] / (ms_pre * 1e-3), 0)},
                          "without_pretest": {"ms": round(ms_nopre, 2), "atomics": wk_nopre[1], "atomics_per_s": round(wk_nopre[1] / (ms_nopre * 1e-3), 0)},
                          "same_bits": same},
            "sum_pass": {"ms": round(ms_sum, 2), "pixels_added": adds, "atomics": 2 * adds, "atomics_per_s": round(2 * adds / (ms_sum * 1e-3), 0)},
            "modelled_GB": {"zmin": {"points_minimum_12N_per_launch": gb(12 * N * launches), "pretest_loads": gb(4 * wk_pre[0]), "atomics": gb(4 * wk_pre[1]),
                                     "zbuf_fill": gb(4 * V * H * W)},
                            "sum": {"points_minimum_12N_per_launch": gb(12 * N * launches), "zbuf_loads": gb(4 * wk_pre[0]), "atomics": gb(12 * adds),
                                    "zeroing": gb(12 * V * H * W)},
                            "note": "modelled from the kernel's counters, not measured: no counter pass was taken"},
            "yardstick_torch_single_pixel": {"this_ms": round(ms_single, 2), "this_atomics": wk_single.cpu().tolist()[1],
                                             "torch_scatter_reduce_amin_ms": round(t_scat, 2), "torch_projection_ms": round(t_proj, 2),
                                             "ratio_scatter_only": round(t_scat / ms_single, 2), "ratio_with_projection": round((t_scat + t_proj) / ms_single, 2),
                                             "same_bits": single_same, "differing_pixels": sum(differing), "views_differing": sum(1 for d in differing if d),
                                             "numpy_referee": referee, "case": "radius 0, r_min = r_max = 0.5"},
            "yardstick_numpy_host": {"points": len(sub), "views": hv, "seconds": round(host_s, 2), "scaled_to_full_job_s": round(host_scaled, 0),
                                     "ratio_to_mean_mode": round(host_scaled * 1e3 / (ms_pre + ms_sum + ms_res), 0)}}
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
