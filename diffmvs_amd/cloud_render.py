"""Ground-truth depth maps from a scanned cloud: what DTU's `Depths_raw` are to its scans, for any tree.

    python -m diffmvs_amd.cloud_render --cloud gt.ply --tree <mvs tree> [--dataset general|dtu|tank|eth3d] [--testlist scans.txt]
        [--transform T.txt [--invert]] [--out <tree>] [--mode mean|nearest] [--radius R] [--r_min 0.5] [--r_max 8] [--tau 0.01] [--overwrite]

renders the cloud into every view of the tree -- at the size and with the intrinsics formats.MVSDataset.load_view produces for it, inside
each `_cam.txt`'s depth range -- and writes <out>/<scan>/depth_gt/%08d.pfm, mask/%08d.png (0 / 255) and render.json: the layout
depth_eval, `eval --gt_depth` and `train_driver --trainpath / --valpath` read.

Every point is splatted as a square of half-width r = clamp(radius * f / z, r_min, r_max) pixels (dmvs_cloud_splat_zmin_f32 /
dmvs_cloud_splat_sum_f32, include/dmvs.h): `radius` is a WORLD length, by default the cloud's point spacing (cloud_grid.estimate_spacing),
so that the front surface is watertight at any distance and the surface behind it does not show through.  Two modes:
  nearest  the z-buffer itself: per pixel the smallest depth of the points whose footprint covers it.  Biased TOWARDS the camera on a
           slanted or noisy surface -- it is the minimum of several points;
  mean     (default) the mean of the points within (1 + tau) of that minimum: the front surface only, without the bias.  The sums are
           fixed point (llrint(z * 2^k), u64) and the result is (float)((sum / cnt) / 2^k) in fp64: a function of integers.
Integer atomics only: a map is the same bits whatever the launch shape, the order of the points or the view chunking."""
from __future__ import annotations

import argparse
import json
import math
import os
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import cloud_grid as G
from . import formats as IO

BUFFER_BYTES = 1 << 30        # z-buffer + sum + count (16 bytes per pixel) of one chunk of views stay below this
SORT_CELLS = 256              # the points are ordered by a grid of about this many cells along the cloud's longest side


def view_table(K, E, near, far) -> np.ndarray:
    """K [V,3,3], E [V,4,4], near / far (numbers or [V]) -> the [V,15] fp64 table of the splat kernels: rows 0 and 1 of P = K E[:3], row 2
    of E, f = K[0,0], near, far.  The products are formed here, in fp64."""
    K, E = np.asarray(K, np.float64).reshape(-1, 3, 3), np.asarray(E, np.float64).reshape(-1, 4, 4)
    V = K.shape[0]
    if E.shape[0] != V:
        raise ValueError(f"{V} intrinsics for {E.shape[0]} extrinsics")
    P = np.einsum("vij,vjk->vik", K, E[:, :3, :])
    t = np.zeros((V, _lib.SPLAT_VIEW_DOUBLES), np.float64)
    t[:, 0:4], t[:, 4:8], t[:, 8:12], t[:, 12] = P[:, 0], P[:, 1], E[:, 2], K[:, 0, 0]
    t[:, 13], t[:, 14] = np.broadcast_to(np.asarray(near, np.float64), (V,)), np.broadcast_to(np.asarray(far, np.float64), (V,))
    return t


def sort_for_locality(points: torch.Tensor) -> torch.Tensor:
    """the points in the order of a coarse grid's key (cloud_grid.build_grid): a wave's 64 footprints then fall into few cache lines of
    every view.  Points with a non-finite coordinate go last.  The rendered bits do not depend on this."""
    if points.shape[0] < 2:
        return points
    ok = torch.isfinite(points).all(1)
    good = points if bool(ok.all()) else points[ok]
    if good.shape[0] >= 2:
        extent = float((good.max(0).values - good.min(0).values).max())
        if extent > 0 and math.isfinite(extent):
            good = G.build_grid(good.contiguous(), extent / SORT_CELLS)["target"]
    return good if good.shape[0] == points.shape[0] else torch.cat([good, points[~ok]]).contiguous()


def default_range(points: torch.Tensor, E: np.ndarray):
    """per view (1e-6 * median |z|, 2 * max |z|) over the cloud's finite points (z in fp32 here: the range only has to be generous).  The
    far end is finite and close to the data on purpose: the fixed-point scale of the mean is chosen from it."""
    V = E.shape[0]
    ok = torch.isfinite(points).all(1)
    pts = points if bool(ok.all()) else points[ok]
    if pts.shape[0] == 0:
        return np.full(V, 1e-6), np.full(V, 1.0)
    sample = pts[::max(1, pts.shape[0] // (1 << 20))]
    near, far = np.zeros(V), np.zeros(V)
    for v in range(V):
        e = torch.tensor(E[v, 2], dtype=torch.float32, device=pts.device)
        med = float(((sample @ e[:3]) + e[3]).abs().median())
        top = float(((pts @ e[:3]) + e[3]).abs().max())
        near[v] = max(1e-6 * med, 1e-30)
        far[v] = min(max(2.0 * top, 2.0 * near[v]), 1e37)
    return near, far


def render_depth(ops, cloud, K, E, size, radius: Optional[float] = None, r_min: float = 0.5, r_max: float = 8.0, mode: str = "mean",
                 tau: float = 0.01, depth_range=None, view_chunk: Optional[int] = None, transform=None, sort: bool = True, blocks: int = 0,
                 pretest: bool = True) -> dict:
    """cloud [N,3]; K [V,3,3], E [V,4,4] (world -> camera, the `_cam.txt` convention); size = (H, W).
    radius: the splat's world-space half-width; None = cloud_grid.estimate_spacing of the cloud (probe cell: 1/64 of its longest side).
    depth_range: None (default_range: 1e-6 of the median depth .. twice the largest, per view), one (near, far) or V of them; points
    outside (near, far] are not drawn.  transform: a 4x4 / 3x4 matrix applied to the cloud first (fp64 products, one rounding to fp32).
    view_chunk: views rendered per pass, None = as many as keep the WORKING buffers (z-buffer, sum, count: 16 bytes per pixel) below
    BUFFER_BYTES; the results (depth, and count in mean mode: 8 bytes per pixel) of all V views stay on the device.
    pretest: the plain load in front of every atomic-min (same bits either way; dmvs.h DMVS_SPLAT_NO_PRETEST).
    -> {"depth" [V,H,W] fp32 (0 = nothing seen), "mask" bool, "count" int32 (mean mode: points averaged per pixel), "counts" int64 [V,4]
    (points with a non-finite coordinate, outside the depth range, off the image, drawn with the radius clamped at r_max), "radius"}"""
    if mode not in ("mean", "nearest"):
        raise ValueError(f"mode must be 'mean' or 'nearest', got {mode!r}")
    pts = G.to_cloud(ops, cloud)
    Kn = (K.detach().cpu().numpy() if torch.is_tensor(K) else np.asarray(K)).astype(np.float64).reshape(-1, 3, 3)
    En = (E.detach().cpu().numpy() if torch.is_tensor(E) else np.asarray(E)).astype(np.float64).reshape(-1, 4, 4)
    V, (H, W) = Kn.shape[0], (int(size[0]), int(size[1]))
    if sort:
        pts = sort_for_locality(pts)
    if radius is None:
        ok = torch.isfinite(pts).all(1)
        good = pts if bool(ok.all()) else pts[ok]
        extent = float((good.max(0).values - good.min(0).values).max()) if good.shape[0] > 1 else 0.0
        radius = G.estimate_spacing(good, extent / 64.0) if extent > 0 else 0.0
        if transform is not None:                             # a similarity scales the spacing with the cloud
            radius *= abs(float(np.linalg.det(np.asarray(transform, np.float64).reshape(-1, 4)[:3, :3]))) ** (1.0 / 3.0)
    if depth_range is None:
        moved = pts if transform is None else _moved(pts, transform)
        near, far = default_range(moved, En)
    else:
        r = np.asarray(depth_range, np.float64)
        near, far = (r[0], r[1]) if r.ndim == 1 else (r[:, 0], r[:, 1])
    table = view_table(Kn, En, near, far)
    N = int(pts.shape[0])
    scale = G.pow2_scale_below(float(table[:, 14].max()), N) if V else 1.0
    if view_chunk is None:
        view_chunk = max(1, BUFFER_BYTES // max(1, 16 * H * W))
    dev = ops.device
    depth = torch.zeros(V, H, W, dtype=torch.float32, device=dev)
    count = torch.zeros(V, H, W, dtype=torch.int32, device=dev) if mode == "mean" else None
    counts = torch.zeros(V, _lib.SPLAT_SLOTS, dtype=torch.int64, device=dev)
    for v0 in range(0, V, int(view_chunk)):
        v1 = min(V, v0 + int(view_chunk))
        zbuf, counts[v0:v1] = ops.cloud_splat_zmin(pts, table[v0:v1], (H, W), radius, r_min, r_max, transform=transform, blocks=blocks,
                                                       pretest=pretest)
        if mode == "nearest":
            depth[v0:v1] = torch.where(torch.isinf(zbuf), torch.zeros_like(zbuf), zbuf)
            continue
        total, cnt = ops.cloud_splat_sum(pts, table[v0:v1], (H, W), radius, r_min, r_max, zbuf, tau, scale, transform=transform, blocks=blocks)
        depth[v0:v1], count[v0:v1] = resolve_mean(total, cnt, scale), cnt
    out = {"depth": depth, "mask": depth > 0, "counts": counts, "radius": float(radius)}
    if count is not None:
        out["count"] = count
    return out


def resolve_mean(total: torch.Tensor, cnt: torch.Tensor, scale: float) -> torch.Tensor:
    """cnt > 0 ? (float)(((double)sum / (double)cnt) / scale) : 0 -- two fp64 divisions and one rounding to fp32"""
    seen = cnt > 0
    mean = (total.double() / cnt.clamp_min(1).double()) / float(scale)
    return torch.where(seen, mean, torch.zeros_like(mean)).float()


def _moved(pts: torch.Tensor, transform) -> torch.Tensor:
    m = torch.as_tensor(np.asarray(transform, np.float64).reshape(-1, 4)[:3], device=pts.device)
    return (pts.double() @ m[:, :3].T + m[:, 3]).float()


# ------------------------------------------------------------------------------------------ trees
def scene_views(tree: str, out: str, dataset: str, scan: str):
    """the reference views of one scan's pair.txt, grouped by image size -> (base, {(H, W): [(view id, K, E, depth_min, depth_max), ...]});
    base is where the scan's depth_gt/, mask/ and render.json go"""
    ds = IO.MVSDataset(tree, dataset=dataset, scan=[scan])
    base = os.path.join(out, scan) if dataset != "general" else out
    groups = {}
    for vid in sorted({ref for _, ref, _ in ds.metas}):
        img, k, e, d0, d1 = ds.load_view(scan, vid)
        groups.setdefault(img.shape[:2], []).append((vid, k, e, d0, d1))
    return base, groups


def clear_maps(base: str):
    """-> (depth_gt/, mask/) of `base`, made and emptied of .pfm / .png files (main has refused by now unless --overwrite: maps of views
    that are no longer in pair.txt must not survive beside the new render.json)"""
    ddir, mdir = os.path.join(base, "depth_gt"), os.path.join(base, "mask")
    for d, ext in ((ddir, ".pfm"), (mdir, ".png")):
        os.makedirs(d, exist_ok=True)
        for f in os.listdir(d):
            if f.endswith(ext):
                os.remove(os.path.join(d, f))
    return ddir, mdir


def write_maps(ddir: str, mdir: str, vid: int, depth: np.ndarray) -> None:
    """depth_gt/%08d.pfm and mask/%08d.png (0 / 255 where depth > 0) of one view"""
    from PIL import Image
    IO.save_pfm(os.path.join(ddir, f"{vid:08d}.pfm"), depth)
    Image.fromarray(np.where(depth > 0, 255, 0).astype(np.uint8)).save(os.path.join(mdir, f"{vid:08d}.png"))


def render_scene(ops, cloud, tree: str, out: str, dataset: str, scan: str, transform=None, **kw) -> dict:
    """one scan of the tree: every reference view of its pair.txt, grouped by image size -> the render.json record.  REPLACES the .pfm / .png
    files of <out>/<scan>/depth_gt and mask (the command line refuses beforehand unless --overwrite)"""
    base, groups = scene_views(tree, out, dataset, scan)
    ddir, mdir = clear_maps(base)
    record = {"scan": scan, "mode": kw.get("mode", "mean"), "views": {}}
    for (H, W), views in groups.items():
        res = render_depth(ops, cloud, np.stack([v[1] for v in views]), np.stack([v[2] for v in views]), (H, W),
                           depth_range=[(v[3], v[4]) for v in views], transform=transform, **kw)
        depth, counts = res["depth"].cpu().numpy(), res["counts"].cpu().tolist()
        record["radius"] = res["radius"]
        for i, (vid, *_rest) in enumerate(views):
            write_maps(ddir, mdir, vid, depth[i])
            record["views"][f"{vid:08d}"] = {"size": [H, W], "non_finite": counts[i][0], "outside_depth_range": counts[i][1], "off_image": counts[i][2],
                                             "radius_clamped": counts[i][3], "covered": float((depth[i] > 0).mean()), "radius": res["radius"]}
    with open(os.path.join(base, "render.json"), "w") as f:
        json.dump(record, f, indent=1)
    return record


def add_tree_arguments(ap, what: str) -> None:
    """the options every renderer of a tree shares (cloud_render, mesh_render)"""
    ap.add_argument("--tree", required=True, help="the MVS tree whose views are rendered (formats.MVSDataset layout)")
    ap.add_argument("--dataset", default="general", choices=["dtu", "tank", "eth3d", "general"])
    ap.add_argument("--testlist", default=None, help="file with one scan per line (dtu / tank / eth3d)")
    ap.add_argument("--transform", default=None, help=f"4x4 text file as cloud_register writes it: applied to the {what} first")
    ap.add_argument("--invert", action="store_true", help=f"apply the inverse of --transform (a ground-truth {what} into the tree's frame)")
    ap.add_argument("--out", default=None, help="where depth_gt/, mask/ and render.json go (default: the tree itself)")
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--device", default="cuda:0")


def tree_arguments(a, prog: str):
    """-> (scans, transform or None, out) of the parsed options of add_tree_arguments.  Refuses BEFORE anything is written: no scan may
    already hold a depth_gt/ unless --overwrite"""
    scans = [""]
    if a.dataset != "general":
        if not a.testlist:
            raise SystemExit(f"{prog}: --dataset {a.dataset} keeps one directory per scan: name them with --testlist")
        with open(a.testlist) as f:
            scans = [ln.strip() for ln in f if ln.strip()]
    T = None
    if a.transform:
        from .cloud_register import load_transform
        T = load_transform(a.transform)
        T = np.linalg.inv(T) if a.invert else T
    elif a.invert:
        raise SystemExit(f"{prog}: --invert needs --transform")
    out = a.out or a.tree
    for scan in scans:
        ddir = os.path.join(out, scan, "depth_gt") if a.dataset != "general" else os.path.join(out, "depth_gt")
        if os.path.isdir(ddir) and os.listdir(ddir) and not a.overwrite:
            raise SystemExit(f"{prog}: {ddir} exists; pass --overwrite to replace it")
    return scans, T, out


def main(argv=None, ops=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cloud", required=True, help="the ground-truth cloud (PLY)")
    add_tree_arguments(ap, "cloud")
    ap.add_argument("--mode", default="mean", choices=["mean", "nearest"])
    ap.add_argument("--radius", type=float, default=None, help="world-space half-width of a splat (default: the cloud's point spacing)")
    ap.add_argument("--r_min", type=float, default=0.5)
    ap.add_argument("--r_max", type=float, default=8.0)
    ap.add_argument("--tau", type=float, default=0.01, help="mean mode: points within (1 + tau) of a pixel's nearest depth are averaged")
    a = ap.parse_args(argv)
    if ops is None:
        from .ops import Ops
        ops = Ops.for_device(a.device)
    scans, T, out = tree_arguments(a, "cloud_render")
    cloud = G.to_cloud(ops, IO.read_ply(a.cloud)[0])
    res = {"cloud": a.cloud, "points": int(cloud.shape[0]), "scans": {}}
    for scan in scans:
        res["scans"][scan] = render_scene(ops, cloud, a.tree, out, a.dataset, scan, transform=T, radius=a.radius,
                                          r_min=a.r_min, r_max=a.r_max, mode=a.mode, tau=a.tau)
    print(json.dumps({"points": res["points"], "scans": {s: {"views": len(r["views"]), "radius": r.get("radius")} for s, r in res["scans"].items()}}), flush=True)
    return res


if __name__ == "__main__":
    main()
