#!/usr/bin/env python3
"""View-selection scoring of the COLMAP import (dmvs_view_select_scores_f64) on a synthetic large model: prints one JSON line
(profiles/view_select_line.json).

    python tools/view_select_bench.py [--images 2000] [--points 1000000] [--track 8] [--reps 10] [--numpy 1]

The model: `images` cameras on a ring around a cloud of `points` points; each point is listed by 2 + Poisson(track - 2) images
(mean track length `track`).  Reported: the kernel's event-timed mean after a warm-up, terms per second, the atomic bytes per
second (8-byte integer adds) against the chip-wide float-atomic rate of MI355X_MICROARCH.md (about 1.3 TB/s), the whole
convert() wall time without the image copy (model read from .bin, cameras, scores, cam files and pair.txt), and the same scores
from a vectorised numpy restatement (point-major, fp64) timed on the CPU."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffmvs_amd import colmap as CM  # noqa: E402
from diffmvs_amd.ops import Ops  # noqa: E402

ATOMIC_RATE_BPS = 1.3e12


def make_model(N, P, track, seed=0):
    rs = np.random.RandomState(seed)
    xyz = rs.uniform(-2.0, 2.0, (P, 3))
    L = np.minimum(N, 2 + rs.poisson(track - 2, P))
    # point r is seen by L[r] images near a random ring position (neighbouring cameras see the same points)
    start = rs.randint(0, N, P)
    img = ((np.repeat(start, L) + np.arange(L.sum()) - np.repeat(np.cumsum(L) - L, L)) % N).astype(np.int64)
    pt = np.repeat(np.arange(P), L)
    order = np.lexsort((pt, img))
    img, pt = img[order], pt[order]
    bounds = np.searchsorted(img, np.arange(N + 1))
    images = []
    for i in range(N):
        ang = 2 * np.pi * i / N
        c = np.array([8 * np.sin(ang), 0.3 * np.sin(5 * ang), -8 * np.cos(ang)])
        q = (np.cos(ang / 2), 0.0, np.sin(-ang / 2), 0.0)
        R = CM.quaternion_to_rotation_matrix(q)
        ids = pt[bounds[i]:bounds[i + 1]] + 1
        images.append(CM.Image(i + 1, tuple(map(float, q)), tuple(map(float, -R @ c)), 1, "%06d.jpg" % i, np.zeros((len(ids), 2)), ids))
    toff = np.zeros(P + 1, np.int64)
    pts = CM.Points3D(np.arange(1, P + 1, dtype=np.int64), xyz, np.zeros((P, 3), np.uint8), np.zeros(P), toff, np.zeros((0, 2), np.int32))
    return CM.Model({1: CM.Camera(1, "PINHOLE", 640, 480, (500.0, 500.0, 320.0, 240.0))}, images, pts)


def numpy_scores(xyz, offsets, imgs, mult, centres, theta0=5.0, sigma1=1.0, sigma2=10.0):
    """the point-major pass vectorised in numpy (fp64, the kernel's arithmetic without the fixed point)"""
    N = len(centres)
    L = np.diff(offsets)
    S = np.zeros(N * N)
    for Lv in np.unique(L[L >= 2]):
        pts = np.nonzero(L == Lv)[0]
        k, l = np.triu_indices(Lv, 1)
        e0 = offsets[pts][:, None]
        a, b, m = imgs[e0 + k], imgs[e0 + l], mult[e0 + k]
        p = xyz[pts][:, None, :]
        u, v = centres[a] - p, centres[b] - p
        nu, nv = np.linalg.norm(u, axis=2), np.linalg.norm(v, axis=2)
        with np.errstate(divide="ignore", invalid="ignore"):
            th = (180 / np.pi) * np.arccos(np.clip((u * v).sum(2) / nu / nv, -1, 1))
        s = np.where(th <= theta0, sigma1, sigma2)
        f = np.where((nu > 0) & (nv > 0), np.exp(-(th - theta0) * (th - theta0) / (2 * s * s)), 0.0) * m
        S += np.bincount((a * N + b).ravel(), f.ravel(), N * N)
    S = S.reshape(N, N)
    return S + S.T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--track", type=float, default=8.0)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--numpy", type=int, default=1)
    a = ap.parse_args()
    ops = Ops.for_device("cuda:0")
    model = make_model(a.images, a.points, a.track)
    extr = [CM.extrinsic(im) for im in model.images]
    centres = CM.camera_centres(extr)
    rows = CM._point_rows(model)
    offsets, imgs, mult = CM.point_image_csr(rows, a.points)
    L = np.diff(offsets)
    terms = int((L * (L - 1) // 2).sum())
    dev = ops.device
    t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (model.points.xyz, offsets, imgs, mult, centres)]
    ops.timers = {"dmvs_view_select_scores_f64": []}
    for _ in range(2):
        ops.view_scores(*t)
    torch.cuda.synchronize()
    ops.timers["dmvs_view_select_scores_f64"].clear()
    for _ in range(a.reps):
        score = ops.view_scores(*t)
    torch.cuda.synchronize()
    ms = [s.elapsed_time(e) for s, e in ops.timers["dmvs_view_select_scores_f64"]]
    ops.timers = None
    kernel_s = float(np.mean(ms)) / 1e3
    with tempfile.TemporaryDirectory() as tmp:
        CM.write_model(model, os.path.join(tmp, "in", "sparse"), ".bin")
        t0 = time.perf_counter()
        phases = CM.convert(os.path.join(tmp, "in"), os.path.join(tmp, "out"), num_src_images=10, ops=ops, copy_images=False)
        convert_s = time.perf_counter() - t0
    line = {"metric": "view-selection terms/sec", "workload": {"images": a.images, "points": a.points, "mean_track": float(L.mean()),
            "terms": terms, "csr_entries": int(len(imgs))},
            "kernel_ms": round(kernel_s * 1e3, 4), "kernel_ms_min": round(min(ms), 4), "reps": a.reps,
            "terms_per_s": terms / kernel_s,
            "atomic": {"bytes_per_s_upper_bound": 8 * terms / kernel_s, "chip_float_atomic_rate_Bps": ATOMIC_RATE_BPS,
                       "frac_of_rate": 8 * terms / kernel_s / ATOMIC_RATE_BPS,
                       "note": "8-byte integer adds, one per nonzero term (an upper bound on the atomics issued); the guide's rate is for float adds"},
            "convert_s_without_images": round(convert_s, 3), "convert_phases_s": {k: round(v, 3) for k, v in phases.items() if k.endswith("_s")}}
    if a.numpy:
        t0 = time.perf_counter()
        ref = numpy_scores(model.points.xyz, offsets, imgs.astype(np.int64), mult, centres)
        np_s = time.perf_counter() - t0
        got = score.cpu().numpy()
        line["numpy"] = {"seconds": round(np_s, 3), "speedup_vs_kernel": np_s / kernel_s, "max_abs_diff": float(np.abs(got - ref).max())}
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
