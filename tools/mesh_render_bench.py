#!/usr/bin/env python3
"""The mesh rasteriser (dmvs_mesh_raster_*) at DTU size: prints one JSON line (profiles/mesh_render_line.json).

    python tools/mesh_render_bench.py [--views 49] [--size 864 1152] [--dim 512] [--reps 5] [--out FILE]

(a) The scene of tools/tsdf_bench.py -- a rippled sphere seen by --views cameras -- fused at --dim^3 voxels and extracted with colours, then
    rendered back into the same views: the project's own meshes, whose faces cover 1 to 3 pixels.  Timed with device events around the fill
    + raster call and around the resolve call (depth and face only, and with normal and colour), no allocation inside the window, the
    median of --reps calls after a warm-up.  Beside it the existing way to such maps: cloud_render's z-buffer (`nearest`) over the mesh's
    VERTICES, sorted for locality as render_depth does, with the voxel side as the radius, timed the same way; and how much of the
    analytic silhouette either one covers.
(b) 2 000 triangles of about 200 pixels a side at random places and depths into 8 views: through the wave pass (a queue that holds them
    all) and with queue_cap = 0 (every box walked by the lane that projected it); the two z-buffers are compared."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tsdf_bench as TB  # noqa: E402
from diffmvs_amd import _lib, cloud_render as CR, mesh_render as MR  # noqa: E402
from diffmvs_amd.ops import Ops, _ptr  # noqa: E402


def raster_calls(ops, verts, faces, table, H, W, vrgb, queue_cap):
    """-> (raster(), resolve(full), buffers): the library calls alone, every buffer allocated here"""
    V, N, F = len(table), int(verts.shape[0]), int(faces.shape[0])
    dev = ops.device
    zid = torch.empty((V, H, W), dtype=torch.int64, device=dev)
    counts = torch.empty((V, _lib.RASTER_SLOTS), dtype=torch.int64, device=dev)
    work = torch.empty(3, dtype=torch.int64, device=dev)
    queue = torch.empty(1 + queue_cap, dtype=torch.int64, device=dev) if queue_cap else None
    depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    face = torch.empty((V, H, W), dtype=torch.int32, device=dev)
    normal = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev)
    rgb = torch.empty((V, H, W, 3), dtype=torch.uint8, device=dev)
    tp = table.ctypes.data

    def raster():
        ops.lib.call("dmvs_mesh_raster_fill_u64", _ptr(zid), zid.numel(), ops.stream())
        ops.lib.call("dmvs_mesh_raster_zid_u64", _ptr(verts), N, _ptr(faces), F, None, tp, V, H, W, 0, 0, _ptr(zid), _ptr(counts), _ptr(work),
                     _ptr(queue), queue_cap, ops.stream())

    def resolve(full):
        ops.lib.call("dmvs_mesh_raster_resolve_f32", _ptr(zid), _ptr(verts), N, _ptr(faces), F, None, tp, V, H, W, _ptr(vrgb) if full else None,
                     _ptr(depth), _ptr(face), _ptr(normal) if full else None, _ptr(rgb) if full else None, ops.stream())
    return raster, resolve, {"zid": zid, "counts": counts, "work": work, "depth": depth}


def case_own_mesh(ops, a):
    H, W = a.size
    V, n = a.views, a.dim
    depth, valid, rgb, views = TB.scene(V, H, W, ops.device)
    h = 2.5 / (n - 1)
    vol = ops.tsdf_volume((n, n, n), np.array([-1.25, -1.25, -1.25]), h)
    ops.tsdf_integrate(vol, depth, valid, rgb, views, 4 * h)
    verts, vrgb, faces = ops.tsdf_extract(vol, min_weight=2)
    del vol
    torch.cuda.empty_cache()
    K = np.array([[1.1 * W, 0.0, W / 2.0], [0.0, 1.1 * W, H / 2.0], [0.0, 0.0, 1.0]])
    Es = np.zeros((V, 4, 4))
    for v in range(V):                                                # (TB.scene's cameras again: its view table keeps only row 2 of E)
        az, el = 2 * np.pi * v / V * 3.0, (v % 3 - 1) * 0.6
        Es[v] = TB.look_at(3.4 * np.array([np.cos(az) * np.cos(el), np.sin(az) * np.cos(el), np.sin(el)]))
    Ks = np.repeat(K[None], V, 0)
    table = MR.view_table(Ks, Es, 1.0, 6.0)
    raster, resolve, buf = raster_calls(ops, verts, faces, table, H, W, vrgb, min(int(faces.shape[0]) * 8, 1 << 20))
    raster(), resolve(True)                                           # warm-up
    ms_raster = TB.timed(raster, a.reps)
    ms_resolve = TB.timed(lambda: resolve(False), a.reps)
    ms_resolve_full = TB.timed(lambda: resolve(True), a.reps)
    counts, work = buf["counts"].sum(0).tolist(), buf["work"].tolist()
    silhouette = valid.bool()
    mesh_cover = float(((buf["depth"] > 0) & silhouette).sum() / silhouette.sum())
    # the existing way: the z-buffer splat of the vertices
    pts = CR.sort_for_locality(verts)
    splat = CR.view_table(Ks, Es, 1.0, 6.0)
    zbuf = torch.empty((V, H, W), dtype=torch.float32, device=ops.device)
    scounts = torch.empty((V, _lib.SPLAT_SLOTS), dtype=torch.int64, device=ops.device)
    out = torch.empty_like(zbuf)

    def nearest():
        zbuf.fill_(float("inf"))
        ops.lib.call("dmvs_cloud_splat_zmin_f32", _ptr(pts), int(pts.shape[0]), None, splat.ctypes.data, V, H, W, h, 0.5, 8.0, 0, 0, _ptr(zbuf),
                     _ptr(scounts), None, ops.stream())
        torch.where(torch.isinf(zbuf), torch.zeros_like(zbuf), zbuf, out=out)
    nearest()
    ms_nearest = TB.timed(nearest, a.reps)
    splat_cover = float(((out > 0) & silhouette).sum() / silhouette.sum())
    both = (out > 0) & (buf["depth"] > 0)
    bias = float((out[both].double() - buf["depth"][both].double()).mean())
    fv = int(faces.shape[0]) * V
    return {"voxels": n ** 3, "voxel": h, "vertices": int(verts.shape[0]), "faces": int(faces.shape[0]), "views": V, "size": [H, W],
            "raster_ms": round(ms_raster, 3), "resolve_depth_face_ms": round(ms_resolve, 3), "resolve_with_normal_rgb_ms": round(ms_resolve_full, 3),
            "face_views_per_s": round(fv / (ms_raster * 1e-3), 0), "slots": dict(zip(MR.SLOT_NAMES, counts)),
            "covered_pixels": work[0], "atomics_issued": work[1], "fell_back": work[2], "covered_pixels_per_drawn_face": round(work[0] / max(1, counts[7]), 2),
            "silhouette_covered_by_mesh": round(mesh_cover, 5), "cloud_render_nearest_ms": round(ms_nearest, 3),
            "silhouette_covered_by_splat": round(splat_cover, 5), "splat_minus_mesh_mean_depth": bias, "splat_radius": h,
            "ratio_nearest_over_raster_plus_resolve": round(ms_nearest / (ms_raster + ms_resolve), 2)}


def case_large_triangles(ops, a):
    H, W = a.size
    rs = np.random.RandomState(0)
    F, V, side = 2000, 8, 200.0
    f = 1.1 * W
    K = np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])
    Es = np.stack([np.eye(4)] * V)
    Es[:, 0, 3] = 0.01 * np.arange(V)
    z = rs.uniform(2.0, 4.0, F)
    c = np.stack([rs.uniform(0, W, F), rs.uniform(0, H, F)], 1)
    ang = rs.uniform(0, 2 * np.pi, F)[:, None] + np.array([0.0, 2.1, 4.2])[None, :]
    px = c[:, None, :] + side / np.sqrt(3.0) * np.stack([np.cos(ang), np.sin(ang)], -1)             # [F,3,2] pixel positions in view 0
    verts = np.stack([(px[..., 0] - W / 2.0) * z[:, None] / f, (px[..., 1] - H / 2.0) * z[:, None] / f, np.repeat(z[:, None], 3, 1)], -1).reshape(-1, 3)
    verts = torch.from_numpy(verts.astype(np.float32)).to(ops.device)
    faces = torch.arange(3 * F, dtype=torch.int32, device=ops.device).reshape(F, 3)
    table = MR.view_table(np.repeat(K[None], V, 0), Es, 1.0, 6.0)
    res = {}
    keep = None
    for name, cap in (("wave", F * V), ("lane_only", 0)):
        raster, _, buf = raster_calls(ops, verts, faces, table, H, W, None, cap)
        raster()
        ms = TB.timed(raster, a.reps)
        work = buf["work"].tolist()
        res[name] = {"raster_ms": round(ms, 3), "covered_pixels": work[0], "atomics_issued": work[1], "fell_back": work[2],
                     "covered_pixels_per_s": round(work[0] / (ms * 1e-3), 0)}
        if keep is None:
            keep = buf["zid"].clone()
        else:
            res["same_bits"] = bool(torch.equal(keep, buf["zid"]))
    res.update({"faces": F, "views": V, "size": [H, W], "side_px": side, "lane_only_over_wave": round(res["lane_only"]["raster_ms"] / res["wave"]["raster_ms"], 2)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--size", type=int, nargs=2, default=[864, 1152], help="H W")
    ap.add_argument("--dim", type=int, default=512, help="the volume the mesh of case (a) is extracted from has this many voxels a side")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    ops = Ops.for_device("cuda:0")
    shown = [w for i, w in enumerate(sys.argv[1:]) if w != "--out" and (i == 0 or sys.argv[i] != "--out")]
    line = {"metric": "triangle mesh -> depth / face / normal / colour maps, ms", "command": ("python tools/mesh_render_bench.py " + " ".join(shown)).strip(),
            "reps": a.reps, "raster_small": _lib.RASTER_SMALL, "own_mesh": case_own_mesh(ops, a), "large_triangles": case_large_triangles(ops, a)}
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
