#!/usr/bin/env python3
"""Oriented normals of depth maps (dmvs_depth_normals_f32) at Tanks&Temples size: prints one JSON line (profiles/depth_normals_line.json).

    python tools/depth_normals_bench.py [--size 1056 1920] [--radius 2] [--reps 20] [--out FILE]

The depth: a rippled, slanted surface with a 10 % step down the middle and fp32 noise, seen by f = 1.2 W cameras; the mask: 5 % of the pixels
out, at random.  Timed with device events around --reps back-to-back calls of the library entry point (the zeroing of the 32 count bytes per view and
the launch; no allocation inside the window) after a warm-up, for ONE view and for a CHUNK of 8 views (one launch).  Bytes: what the
algorithm has to move, 4 (depth) + 1 (mask) read and 16 (normal, cosine) written per pixel, over that time.
The yardstick: the same fit written with torch fp64 tensor operations on the same device (shifted slices of the padded inverse depth,
integer sums as int32 tensors, the contract's operation order), timed the same way with --torch_reps calls; the line also says in how
many values the two results differ."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffmvs_amd import _lib  # noqa: E402
from diffmvs_amd.ops import Ops, _ptr  # noqa: E402


def scene(B, H, W, dev, seed=0):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    depth = torch.stack([650.0 + 10.0 * v + 0.05 * xs - 0.03 * ys + 8.0 * torch.sin(xs / 90.0 + v) * torch.cos(ys / 70.0) for v in range(B)])
    depth[:, :, W // 2:] += 65.0
    depth = (depth + 0.05 * torch.randn(depth.shape, generator=gen, device=dev, dtype=torch.float64)).float().contiguous()
    valid = (torch.rand(depth.shape, generator=gen, device=dev) > 0.05).to(torch.uint8).contiguous()
    K = np.repeat(np.array([[1.2 * W, 0.0, W / 2.0], [0.0, 1.2 * W, H / 2.0], [0.0, 0.0, 1.0]])[None], B, 0)
    E = np.repeat(np.eye(4)[None], B, 0)
    for v in range(B):
        a = 0.05 * (v - B // 2)
        E[v, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        E[v, :3, 3] = [-30.0 * v, 4.0 * v, 0.0]
    return depth, valid, Ops.normal_cams(K, E)


def torch_fit(depth, valid, cams, r, rel_jump, min_pts):
    """include/dmvs.h, the normals contract, with torch fp64 tensor operations -> (out [B,H,W,4] fp32, counts [B,4] int64)"""
    B, H, W = depth.shape
    dev = depth.device
    usable = torch.isfinite(depth) & (depth > 0) & (valid != 0)
    w = torch.where(usable, 1.0 / depth.double(), torch.zeros((), dtype=torch.float64, device=dev))
    pad = torch.nn.functional.pad(w, (r, r, r, r))
    zi = lambda: torch.zeros((B, H, W), dtype=torch.int32, device=dev)  # noqa: E731
    zf = lambda: torch.zeros((B, H, W), dtype=torch.float64, device=dev)  # noqa: E731
    n, Sx, Sy, Sxx, Sxy, Syy, Tw, Tx, Ty = zi(), zi(), zi(), zi(), zi(), zi(), zf(), zf(), zf()
    gate = rel_jump * w
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            wj = pad[:, r + dy:r + dy + H, r + dx:r + dx + W]
            dl = wj - w
            take = (wj > 0) & (dl.abs() <= gate)
            ti = take.to(torch.int32)
            n, Sx, Sy, Sxx, Sxy, Syy = n + ti, Sx + ti * dx, Sy + ti * dy, Sxx + ti * (dx * dx), Sxy + ti * (dx * dy), Syy + ti * (dy * dy)
            Tw, Tx, Ty = torch.where(take, Tw + dl, Tw), torch.where(take, Tx + float(dx) * dl, Tx), torch.where(take, Ty + float(dy) * dl, Ty)
    C00, C01, C02 = Syy * n - Sy * Sy, -(Sxy * n - Sx * Sy), Sxy * Sy - Syy * Sx
    C11, C12, C22 = Sxx * n - Sx * Sx, -(Sxx * Sy - Sxy * Sx), Sxx * Syy - Sxy * Sxy
    D = Sxx * C00 + Sxy * C01 + Sx * C02
    f = lambda q: q.double()  # noqa: E731
    a = ((f(C00) * Tx + f(C01) * Ty) + f(C02) * Tw) / f(D)
    b = ((f(C01) * Tx + f(C11) * Ty) + f(C12) * Tw) / f(D)
    c = ((f(C02) * Tx + f(C12) * Ty) + f(C22) * Tw) / f(D)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    cm = torch.from_numpy(cams).to(dev).view(B, 3, 3, 3, 1, 1)                        # [view, K | Kinv | R, row, column, 1, 1]
    K, Kinv, R = cm[:, 0], cm[:, 1], cm[:, 2]
    wf = w + c
    c0 = (wf - a * xs) - b * ys
    g = [(K[:, 0, i] * a + K[:, 1, i] * b) + K[:, 2, i] * c0 for i in range(3)]
    ln = torch.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
    ray = [(Kinv[:, i, 0] * xs + Kinv[:, i, 1] * ys) + Kinv[:, i, 2] for i in range(3)]
    rl = torch.sqrt((ray[0] * ray[0] + ray[1] * ray[1]) + ray[2] * ray[2])
    s1 = (n < min_pts) | (D == 0)
    s2 = ~(wf > 0) | ~torch.isfinite(ln) | (ln == 0)
    ok = usable & ~s1 & ~s2
    nc = [-g[i] / ln for i in range(3)]
    res = [(R[:, 0, i] * nc[0] + R[:, 1, i] * nc[1]) + R[:, 2, i] * nc[2] for i in range(3)] + [wf / (ln * rl)]
    out = torch.stack([torch.where(ok, q, torch.zeros((), dtype=torch.float64, device=dev)).float() for q in res], -1)
    slot = torch.where(~usable, 0, torch.where(s1, 1, torch.where(s2, 2, 3)))
    counts = torch.stack([(slot == k).flatten(1).sum(1) for k in range(4)], 1)
    return out, counts


def timed(fn, reps):
    """milliseconds per call of `reps` back-to-back fn() between two events on the current stream"""
    st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    st.record()
    for _ in range(reps):
        fn()
    en.record()
    torch.cuda.synchronize()
    return st.elapsed_time(en) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[1056, 1920], help="H W")
    ap.add_argument("--radius", type=int, default=2)
    ap.add_argument("--rel_jump", type=float, default=0.02)
    ap.add_argument("--min_pts", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--torch_reps", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    ops = Ops.for_device("cuda:0")
    H, W = a.size
    cases = {}
    for name, B in (("one_view", 1), ("chunk_of_8", _lib.NORMAL_VIEW_CHUNK)):
        depth, valid, cams = scene(B, H, W, ops.device)
        out = torch.empty((B, H, W, 4), dtype=torch.float32, device=ops.device)
        counts = torch.empty((B, _lib.NORMAL_SLOTS), dtype=torch.int64, device=ops.device)
        args = (_ptr(depth), _ptr(valid), cams.ctypes.data, B, H, W, a.radius, a.rel_jump, a.min_pts, _ptr(out), _ptr(counts), ops.stream())
        call = lambda: ops.lib.call("dmvs_depth_normals_f32", *args)  # noqa: E731
        call()                                                     # warm-up
        ms = timed(call, a.reps)
        want, counts_w = torch_fit(depth, valid, cams, a.radius, a.rel_jump, a.min_pts)      # warm-up of the yardstick, and its result
        differ = int((out != want).sum())
        same_counts = bool(torch.equal(counts, counts_w))
        del want
        ms_torch = timed(lambda: torch_fit(depth, valid, cams, a.radius, a.rel_jump, a.min_pts), a.torch_reps)
        nbytes = B * H * W * (4 + 1 + 16)
        cases[name] = {"views": B, "kernel_ms": round(ms, 4), "bytes": nbytes, "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1),
                       "pixels_per_s": round(B * H * W / (ms * 1e-3), 0), "torch_fp64_ms": round(ms_torch, 2), "ratio": round(ms_torch / ms, 1),
                       "beats_yardstick": bool(ms < ms_torch), "values_differing_from_torch": differ, "counts_equal": same_counts,
                       "slots": counts.sum(0).cpu().tolist()}
    shown = [w for i, w in enumerate(sys.argv[1:]) if w != "--out" and (i == 0 or sys.argv[i] != "--out")]
    line = {"metric": "depth maps -> oriented normals, ms per call", "command": ("python tools/depth_normals_bench.py " + " ".join(shown)).strip(),
            "workload": {"size": [H, W], "radius": a.radius, "rel_jump": a.rel_jump, "min_pts": a.min_pts, "taps": (2 * a.radius + 1) ** 2},
            "reps": a.reps, "torch_reps": a.torch_reps, "bytes_model": "4 (depth) + 1 (mask) read, 16 written per pixel: the algorithm's own, not a counter pass",
            **cases}
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
