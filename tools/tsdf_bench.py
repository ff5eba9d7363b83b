#!/usr/bin/env python3
"""TSDF fusion of depth maps and surface nets (dmvs_tsdf_*) at DTU size: prints one JSON line (profiles/tsdf_line.json).

    python tools/tsdf_bench.py [--views 49] [--size 864 1152] [--dims 256 512] [--reps 5] [--out FILE]

The scene: a rippled sphere of radius about 1 in the box [-1.25, 1.25]^3, seen by --views cameras on three rings at distance 3.4 with
f = 1.1 W, the depth maps rendered analytically with a little noise, the mask = the pixels that hit it, random colours.  The truncation is 4
voxels.  Timed with device events around ONE call of the library entry point that integrates all the views (ceil(views / 8) launches; no
allocation inside the window) into a zeroed volume with colour sums, the median of --reps calls after a warm-up; with the cull and with
DMVS_TSDF_NO_CULL; the two volumes are compared.  Bytes: what the algorithm has to move: S and Wt read and written once per launch
(16 bytes per voxel and launch), the depth, mask and colour maps once (8 bytes per pixel); the colour sums (32 bytes per voxel and launch
that adds to them) are left out, so the fraction is a lower bound.  Extraction: Ops.tsdf_extract as a whole (two flag launches, two
torch.cumsum, two host reads of the totals, the vertex and face launches), min_weight 2.
The yardstick: the same integration written with torch fp64 tensor operations on the same device in the contract's operation order, one
view at a time over the whole volume, timed the same way for --torch_reps calls; the line also says in how many voxels the two differ."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffmvs_amd import _lib, mesh  # noqa: E402
from diffmvs_amd.ops import Ops, _ptr  # noqa: E402

HBM_PEAK_GBS = 8000.0      # the spec peak bench.py uses


def look_at(c):
    z = -c / np.linalg.norm(c)
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(z, x), z])
    E = np.eye(4)
    E[:3, :3], E[:3, 3] = R, -R @ c
    return E


def scene(V, H, W, dev, seed=0):
    gen = torch.Generator(device=dev)
    gen.manual_seed(seed)
    K = np.array([[1.1 * W, 0.0, W / 2.0], [0.0, 1.1 * W, H / 2.0], [0.0, 0.0, 1.0]])
    Es = []
    for v in range(V):
        az, el = 2 * np.pi * v / V * 3.0, (v % 3 - 1) * 0.6
        Es.append(look_at(3.4 * np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)])))
    Es = np.stack(Es)
    ys, xs = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float64), torch.arange(W, device=dev, dtype=torch.float64), indexing="ij")
    Kinv = torch.from_numpy(np.linalg.inv(K)).to(dev)
    ray = torch.stack([xs, ys, torch.ones_like(xs)], -1) @ Kinv.T
    depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    valid = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    for v in range(V):
        c = torch.from_numpy(Es[v, :3, 3].copy()).to(dev)
        a, b, cc = (ray * ray).sum(-1), -2.0 * (ray @ c), float(c @ c) - 1.0
        disc = b * b - 4 * a * cc
        t = (-b - torch.sqrt(disc.clamp_min(0))) / (2 * a)
        t = t * (1.0 + 0.02 * torch.sin(xs / 40.0 + v) * torch.cos(ys / 35.0)) + 0.002 * torch.randn(t.shape, generator=gen, device=dev, dtype=torch.float64)
        depth[v] = torch.where(disc > 0, t, torch.zeros_like(t)).float()
        valid[v] = (disc > 0).to(torch.uint8)
    rgb = torch.randint(0, 256, (V, H, W, 3), generator=gen, device=dev, dtype=torch.uint8)
    return depth, valid, rgb, mesh.tsdf_views(np.repeat(K[None], V, 0), Es)


def torch_integrate(depth, valid, rgb, views, dims, origin, h, tau):
    """include/dmvs.h, dmvs_tsdf_integrate_f32, with torch fp64 tensor operations -> S, Wt [nz,ny,nx] int32, C [nz,ny,nx,4] int32"""
    nx, ny, nz = dims
    V, H, W = depth.shape
    dev = depth.device
    k, j, i = torch.meshgrid(torch.arange(nz, device=dev, dtype=torch.float64), torch.arange(ny, device=dev, dtype=torch.float64),
                             torch.arange(nx, device=dev, dtype=torch.float64), indexing="ij")
    X, Y, Z = origin[0] + i * h, origin[1] + j * h, origin[2] + k * h
    S, Wt = (torch.zeros((nz, ny, nx), dtype=torch.int32, device=dev) for _ in range(2))
    Cs = torch.zeros((nz, ny, nx, 4), dtype=torch.int32, device=dev)
    for v in range(V):
        p = [float(q) for q in views[v]]
        x = ((p[0] * X + p[1] * Y) + p[2] * Z) + p[3]
        y = ((p[4] * X + p[5] * Y) + p[6] * Z) + p[7]
        z = ((p[8] * X + p[9] * Y) + p[10] * Z) + p[11]
        u, w = x / z, y / z
        pu, pw = torch.round(u), torch.round(w)                    # (torch.round: ties to even)
        ok = (z > 0) & torch.isfinite(u) & torch.isfinite(w) & (pu >= 0) & (pu <= W - 1) & (pw >= 0) & (pw <= H - 1)
        pix = torch.where(ok, pw, torch.zeros_like(pw)).long() * W + torch.where(ok, pu, torch.zeros_like(pu)).long()
        d = depth[v].reshape(-1)[pix].double()
        ok &= (valid[v].reshape(-1)[pix] != 0) & torch.isfinite(d) & (d > 0)
        sdf = d - z
        ok &= ~(sdf < -tau)
        q = torch.round(torch.clamp_max(sdf / tau, 1.0) * 16384.0)
        S += torch.where(ok, q, torch.zeros_like(q)).to(torch.int32)
        Wt += ok.to(torch.int32)
        c = ok & (sdf <= tau)
        Cs[..., :3] += torch.where(c[..., None], rgb[v].reshape(-1, 3)[pix].to(torch.int32), torch.zeros((), dtype=torch.int32, device=dev))
        Cs[..., 3] += c.to(torch.int32)
    return S, Wt, Cs


def timed(fn, reps, before=lambda: None):
    """the median, in milliseconds, of `reps` single fn() calls, each between two events on the current stream, before() outside the window"""
    ms = []
    for _ in range(reps):
        before()
        st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        st.record()
        fn()
        en.record()
        torch.cuda.synchronize()
        ms.append(st.elapsed_time(en))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--size", type=int, nargs=2, default=[864, 1152], help="H W")
    ap.add_argument("--dims", type=int, nargs="+", default=[256, 512], help="cubic volumes of this many voxels a side")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch_reps", type=int, default=1)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    ops = Ops.for_device("cuda:0")
    H, W = a.size
    V = a.views
    depth, valid, rgb, views = scene(V, H, W, ops.device)
    launches = -(-V // _lib.TSDF_VIEW_CHUNK)
    cases = {}
    for n in a.dims:
        h = 2.5 / (n - 1)
        origin, tau = np.array([-1.25, -1.25, -1.25]), 4 * h
        vol = ops.tsdf_volume((n, n, n), origin, h)

        def zero():
            vol.S.zero_(), vol.Wt.zero_(), vol.C.zero_()

        def integrate(flags):
            ops.lib.call("dmvs_tsdf_integrate_f32", _ptr(depth), _ptr(valid), _ptr(rgb), views.ctypes.data, V, H, W, n, n, n, origin.ctypes.data, h, tau,
                         flags, _ptr(vol.S), _ptr(vol.Wt), _ptr(vol.C), ops.stream())
        integrate(0)                                                  # warm-up
        ms_nocull = timed(lambda: integrate(_lib.TSDF_NO_CULL), a.reps, zero)
        keep = (vol.S.clone(), vol.Wt.clone(), vol.C.clone())
        ms = timed(lambda: integrate(0), a.reps, zero)
        same = all(bool(torch.equal(p, q)) for p, q in zip(keep, (vol.S, vol.Wt, vol.C)))
        del keep
        vol.views = V
        ops.tsdf_extract(vol, min_weight=2)                           # warm-up
        out = {}
        ms_extract = timed(lambda: out.update(r=ops.tsdf_extract(vol, min_weight=2)), a.reps)
        nv, nf = int(out["r"][0].shape[0]), int(out["r"][2].shape[0])
        out.clear()
        torch_integrate(depth[:1], valid[:1], rgb[:1], views[:1], (n, n, n), origin, h, tau)      # warm-up of the yardstick
        ms_torch = timed(lambda: out.update(r=torch_integrate(depth, valid, rgb, views, (n, n, n), origin, h, tau)), a.torch_reps)
        differ = sum(int((p != q).sum()) for p, q in zip(out["r"], (vol.S, vol.Wt, vol.C)))
        out.clear()
        nbytes = launches * n ** 3 * 16 + V * H * W * 8
        cases[f"{n}^3"] = {"voxels": n ** 3, "voxel": h, "integrate_ms": round(ms, 3), "integrate_no_cull_ms": round(ms_nocull, 3),
                           "cull_changes_no_bit": same, "voxel_views_per_s": round(n ** 3 * V / (ms * 1e-3), 0), "bytes": nbytes,
                           "GB_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1), "frac_of_hbm_peak": round(nbytes / (ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                           "observed_voxels": int((vol.Wt >= 2).sum()), "extract_ms": round(ms_extract, 3), "vertices": nv, "faces": nf,
                           "torch_fp64_ms": round(ms_torch, 1), "ratio": round(ms_torch / ms, 1), "voxels_differing_from_torch": differ}
        del vol
        torch.cuda.empty_cache()
    shown = [w for i, w in enumerate(sys.argv[1:]) if w != "--out" and (i == 0 or sys.argv[i] != "--out")]
    line = {"metric": "depth maps -> TSDF volume -> surface-nets mesh, ms", "command": ("python tools/tsdf_bench.py " + " ".join(shown)).strip(),
            "workload": {"views": V, "size": [H, W], "trunc_voxels": 4, "launches": launches, "colour": True, "min_weight": 2},
            "reps": a.reps, "torch_reps": a.torch_reps, "hbm_peak_GBs": HBM_PEAK_GBS,
            "bytes_model": "16 per voxel and launch (S, Wt read and written) + 8 per pixel (depth, mask, colour) once; colour sums left out: a lower bound",
            **cases}
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
