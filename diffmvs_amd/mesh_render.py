"""Triangle meshes into the views of a tree: depth, face index, normal and colour per pixel -- what BlendedMVS's `rendered_depth_maps` are
to its meshes, for any mesh (mesh.py's `mesh.ply` included) and any tree.

    python -m diffmvs_amd.mesh_render --mesh mesh.ply --tree <mvs tree> [--dataset general|dtu|tank|eth3d] [--testlist scans.txt]
        [--transform T.txt [--invert]] [--out <tree>] [--cull neg|pos] [--preview DIR] [--overwrite]

renders the mesh into every view of the tree -- at the size and with the intrinsics formats.MVSDataset.load_view produces for it, inside
each `_cam.txt`'s depth range -- and writes <out>/<scan>/depth_gt/%08d.pfm, mask/%08d.png (0 / 255) and render.json, in cloud_render's
layout: what depth_eval, `eval --gt_depth` and `train_driver --trainpath / --valpath` read.  --preview DIR also writes a shaded
%08d.png per view: the interpolated vertex colour (mid-grey without one) times 0.25 + 0.75 |n_z| of the camera-space normal, on black.

A z-buffer rasteriser (dmvs_mesh_raster_zid_u64 / dmvs_mesh_raster_resolve_f32, include/dmvs.h): vertices are projected in fp64 and
snapped to 1/256 pixel, coverage is exact integer arithmetic with a tie rule that gives a pixel centre on a shared edge to exactly one of
the two faces, the depth is interpolated in 1 / z, and a pixel keeps the minimum of (depth bits << 32 | face) under one integer atomic:
the same bits on every run.  There is NO near-plane clipping: a face with a vertex at or in front of `near` is not drawn and leaves a
hole; render.json counts those faces per view (`not_drawn_near_plane`) and the command line warns about them."""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Optional

import numpy as np
import torch

from . import _lib
from . import cloud_grid as G
from . import cloud_render as CR
from . import formats as IO

ZID_BYTES = 1 << 30           # the uint64 z-buffer (8 bytes per pixel) of one chunk of views stays below this
SLOT_NAMES = ("invalid_vertex", "not_drawn_near_plane", "beyond_far", "guard_band", "zero_area", "culled", "off_image", "drawn")
GREY = 128


def view_table(K, E, near, far) -> np.ndarray:
    """K [V,3,3], E [V,4,4], near / far (numbers or [V]) -> the [V,22] fp64 table of the raster kernels: rows 0 and 1 of P = K E[:3],
    E[:3], near, far.  The products are formed here, in fp64."""
    K, E = np.asarray(K, np.float64).reshape(-1, 3, 3), np.asarray(E, np.float64).reshape(-1, 4, 4)
    V = K.shape[0]
    if E.shape[0] != V:
        raise ValueError(f"{V} intrinsics for {E.shape[0]} extrinsics")
    P = np.einsum("vij,vjk->vik", K, E[:, :3, :])
    t = np.zeros((V, _lib.RASTER_VIEW_DOUBLES), np.float64)
    t[:, 0:4], t[:, 4:8], t[:, 8:20] = P[:, 0], P[:, 1], E[:, :3].reshape(V, 12)
    t[:, 20], t[:, 21] = np.broadcast_to(np.asarray(near, np.float64), (V,)), np.broadcast_to(np.asarray(far, np.float64), (V,))
    return t


def render_mesh(ops, verts, faces, K, E, size, rgb=None, depth_range=None, cull: Optional[str] = None, transform=None,
                view_chunk: Optional[int] = None, normals: bool = False, queue_cap: Optional[int] = None, blocks: int = 0) -> dict:
    """verts [N,3], faces [F,3]; K [V,3,3], E [V,4,4] (world -> camera, the `_cam.txt` convention); size = (H, W).
    rgb: None or [N,3] uint8 vertex colours (interpolated into "rgb").  depth_range: None (cloud_render.default_range of the vertices),
    one (near, far) or V of them; a face with a vertex at z <= near is NOT drawn, nothing is drawn beyond far.  cull: None, "neg" or "pos":
    drop the faces whose snapped image-space area has that sign.  transform: a 4x4 / 3x4 matrix applied to the vertices first.
    view_chunk: views rendered per pass, None = as many as keep the uint64 z-buffer below ZID_BYTES.  queue_cap, blocks: the shape of
    the launches (Ops.mesh_raster_zid); no output bit depends on them.
    -> {"depth" [V,H,W] fp32 (0 = nothing seen), "mask" bool, "face" int32 (-1 = none), "counts" int64 [V,8] (SLOT_NAMES), "work" int64
    [3] (covered pixels, atomics issued, faces that fell back)[, "normal" [V,H,W,3] fp32 (world frame, towards the camera)][, "rgb"
    [V,H,W,3] uint8]}"""
    vt = G.to_cloud(ops, verts)
    fc = torch.as_tensor(np.asarray(faces) if not torch.is_tensor(faces) else faces).to(device=ops.device, dtype=torch.int32).reshape(-1, 3).contiguous()
    vrgb = None
    if rgb is not None:
        vrgb = torch.as_tensor(np.asarray(rgb) if not torch.is_tensor(rgb) else rgb).to(device=ops.device, dtype=torch.uint8).reshape(-1, 3).contiguous()
        if vrgb.shape[0] != vt.shape[0]:
            raise ValueError(f"{vrgb.shape[0]} colours for {vt.shape[0]} vertices")
    Kn = (K.detach().cpu().numpy() if torch.is_tensor(K) else np.asarray(K)).astype(np.float64).reshape(-1, 3, 3)
    En = (E.detach().cpu().numpy() if torch.is_tensor(E) else np.asarray(E)).astype(np.float64).reshape(-1, 4, 4)
    V, (H, W) = Kn.shape[0], (int(size[0]), int(size[1]))
    if depth_range is None:
        near, far = CR.default_range(vt if transform is None else CR._moved(vt, transform), En)
    else:
        r = np.asarray(depth_range, np.float64)
        near, far = (r[0], r[1]) if r.ndim == 1 else (r[:, 0], r[:, 1])
    table = view_table(Kn, En, near, far)
    if view_chunk is None:
        view_chunk = max(1, ZID_BYTES // max(1, 8 * H * W))
    dev = ops.device
    out = {"depth": torch.zeros(V, H, W, dtype=torch.float32, device=dev), "face": torch.full((V, H, W), -1, dtype=torch.int32, device=dev),
           "counts": torch.zeros(V, _lib.RASTER_SLOTS, dtype=torch.int64, device=dev), "work": torch.zeros(3, dtype=torch.int64, device=dev)}
    if normals:
        out["normal"] = torch.zeros(V, H, W, 3, dtype=torch.float32, device=dev)
    if vrgb is not None:
        out["rgb"] = torch.zeros(V, H, W, 3, dtype=torch.uint8, device=dev)
    for v0 in range(0, V, int(view_chunk)):
        v1 = min(V, v0 + int(view_chunk))
        zid, out["counts"][v0:v1], wk = ops.mesh_raster_zid(vt, fc, table[v0:v1], (H, W), cull=cull, transform=transform, queue_cap=queue_cap,
                                                            blocks=blocks, work=True)
        out["work"] += wk
        out["depth"][v0:v1], out["face"][v0:v1], nm, cl = ops.mesh_raster_resolve(zid, vt, fc, table[v0:v1], transform=transform, vrgb=vrgb,
                                                                                  normals=normals)
        if normals:
            out["normal"][v0:v1] = nm
        if vrgb is not None:
            out["rgb"][v0:v1] = cl
    out["mask"] = out["face"] >= 0
    return out


def shade(res: dict, E) -> torch.Tensor:
    """the preview of render_mesh(..., normals=True): colour (mid-grey without "rgb") times 0.25 + 0.75 |n_cam,z|, black where nothing
    was drawn -> [V,H,W,3] uint8.  At least 1 on every drawn pixel, so that the preview is non-black exactly where the mask is set."""
    n = res["normal"].double()
    R2 = torch.as_tensor(np.asarray(E, np.float64).reshape(-1, 4, 4)[:, 2, :3], device=n.device)
    nz = (n * R2[:, None, None, :]).sum(-1).abs()
    col = res["rgb"].double() if "rgb" in res else torch.full_like(n, float(GREY))
    img = torch.round(col * (0.25 + 0.75 * nz)[..., None]).clamp(1, 255)
    return torch.where(res["mask"][..., None], img, torch.zeros_like(img)).to(torch.uint8)


# ------------------------------------------------------------------------------------------ trees
def render_scene(ops, verts, faces, rgb, tree: str, out: str, dataset: str, scan: str, transform=None, cull=None, preview=None) -> dict:
    """one scan of the tree (cloud_render.scene_views) -> the render.json record.  REPLACES the .pfm / .png files of <out>/<scan>/depth_gt
    and mask (the command line refuses beforehand unless --overwrite)"""
    from PIL import Image
    base, groups = CR.scene_views(tree, out, dataset, scan)
    ddir, mdir = CR.clear_maps(base)
    pdir = None
    if preview:
        pdir = os.path.join(preview, scan) if dataset != "general" else preview
        os.makedirs(pdir, exist_ok=True)
    record = {"scan": scan, "mode": "mesh", "cull": cull, "not_drawn_near_plane": 0, "views": {}}
    for (H, W), views in groups.items():
        Es = np.stack([v[2] for v in views])
        res = render_mesh(ops, verts, faces, np.stack([v[1] for v in views]), Es, (H, W), rgb=rgb if pdir else None,
                          depth_range=[(v[3], v[4]) for v in views], cull=cull, transform=transform, normals=bool(pdir))
        depth, counts = res["depth"].cpu().numpy(), res["counts"].cpu().tolist()
        shaded = shade(res, Es).cpu().numpy() if pdir else None
        for i, (vid, *_rest) in enumerate(views):
            CR.write_maps(ddir, mdir, vid, depth[i])
            if pdir:
                Image.fromarray(shaded[i]).save(os.path.join(pdir, f"{vid:08d}.png"))
            record["views"][f"{vid:08d}"] = {"size": [H, W], **dict(zip(SLOT_NAMES, counts[i])), "covered": float((depth[i] > 0).mean())}
            record["not_drawn_near_plane"] += counts[i][1]
    with open(os.path.join(base, "render.json"), "w") as f:
        json.dump(record, f, indent=1)
    return record


def main(argv=None, ops=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="the triangle mesh (binary PLY: formats.read_ply_mesh)")
    CR.add_tree_arguments(ap, "mesh")
    ap.add_argument("--cull", default=None, choices=["neg", "pos"], help="drop the faces whose image-space area has this sign")
    ap.add_argument("--preview", default=None, help="also write a shaded %%08d.png per view here")
    a = ap.parse_args(argv)
    if ops is None:
        from .ops import Ops
        ops = Ops.for_device(a.device)
    scans, T, out = CR.tree_arguments(a, "mesh_render")
    xyz, rgb, faces = IO.read_ply_mesh(a.mesh)
    if faces.shape[0] == 0:
        raise SystemExit(f"mesh_render: {a.mesh} has no faces (cloud_render renders clouds)")
    res = {"mesh": a.mesh, "vertices": int(xyz.shape[0]), "faces": int(faces.shape[0]), "scans": {}}
    for scan in scans:
        r = res["scans"][scan] = render_scene(ops, xyz, faces, rgb, a.tree, out, a.dataset, scan, transform=T, cull=a.cull, preview=a.preview)
        if r["not_drawn_near_plane"]:
            print(f"mesh_render: {scan or a.tree}: {r['not_drawn_near_plane']} (face, view) pairs reach the near plane and were NOT drawn "
                  "(no near clipping): they leave holes", file=sys.stderr)
    print(json.dumps({"vertices": res["vertices"], "faces": res["faces"],
                      "scans": {s: {"views": len(r["views"]), "not_drawn_near_plane": r["not_drawn_near_plane"]} for s, r in res["scans"].items()}}),
          flush=True)
    return res


if __name__ == "__main__":
    main()
