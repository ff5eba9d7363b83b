"""A surface from a scene's depth maps on the MI355X: truncated signed distance fusion into a dense voxel volume and surface nets
over its zero set (dmvs_tsdf_* of include/dmvs.h, csrc/tsdf.hip; Ops.tsdf_integrate / Ops.tsdf_extract).

    python -m diffmvs_amd.mesh --outdir <eval output> [--testpath <root> --dataset dtu --testlist list.txt]
        [--voxel S | --resolution N] [--trunc 4] [--min_weight 2] [--bounds x0 y0 z0 x1 y1 z1] [--out mesh.ply] [--min_component N]
        [--simplify V]

reads the tree diffmvs_amd.eval (--filter) leaves behind -- cams/, images/, depth_fused/ (fusion.filter_depth(write_fused=True): the
depth averaged over the consistent views) or else depth_est/, and mask/*_final.png or else every finite positive depth -- and writes a
binary PLY with vertices, colours and triangles.  Integer sums and fp64 geometry in a fixed order: the same files give the same mesh bit
for bit, whatever the chunking of the views."""
from __future__ import annotations

import argparse
import json
import os
from typing import Sequence

import numpy as np
import torch

from . import _lib
from . import formats as IO
from .ops import Ops


def tsdf_views(K, E) -> np.ndarray:
    """K [V,3,3], E [V,4,4] (world -> camera) -> the HOST [V,12] fp64 table of dmvs_tsdf_integrate_f32: rows 0 and 1 of P = K E[:3],
    then row 2 of E (the first 12 doubles of cloud_render.view_table's layout, the cameras' own)"""
    K, E = (np.asarray(m.detach().cpu().numpy() if torch.is_tensor(m) else m, np.float64) for m in (K, E))
    if K.ndim != 3 or K.shape[1:] != (3, 3) or E.shape != (K.shape[0], 4, 4):
        raise _lib.DmvsError(f"tsdf_views: K must be [V,3,3] and E [V,4,4], got {K.shape} and {E.shape}")
    P = np.matmul(K, E[:, :3, :])
    return np.ascontiguousarray(np.concatenate([P[:, 0], P[:, 1], E[:, 2]], 1))


def make_volume(ops: Ops, bounds, voxel=None, resolution=512, max_voxels=2 ** 29, colour=True):
    """A zeroed volume over bounds = (lo [3], hi [3]): voxel side `voxel`, or else the longest axis in `resolution` voxels.  Voxel 0 sits at
    lo and the last voxel of an axis at or beyond hi.  More than max_voxels voxels raises, naming the side that would fit."""
    lo, hi = (np.asarray(b, np.float64).reshape(3) for b in bounds)
    ext = hi - lo
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (ext >= 0).all() and ext.max() > 0):
        raise _lib.DmvsError(f"make_volume: bounds {lo} .. {hi} are not a box")
    if voxel is None:
        if int(resolution) < 2:
            raise _lib.DmvsError(f"make_volume: resolution {resolution}; at least 2 voxels along the longest axis")
        voxel = float(ext.max()) / (int(resolution) - 1)
    h = float(voxel)
    if not (h > 0.0 and np.isfinite(h)):
        raise _lib.DmvsError(f"make_volume: voxel side {voxel}")

    def dims_at(side):
        return [int(np.ceil(e / side - 1e-9)) + 1 for e in ext]

    def count(side):
        d = dims_at(side)
        return d[0] * d[1] * d[2]

    cap = min(int(max_voxels), 2 ** 31 - 1)
    if count(h) > cap:
        fit = h * (count(h) / cap) ** (1.0 / 3.0)
        while count(fit) > cap:
            fit *= 1.02
        raise _lib.DmvsError(f"make_volume: {' x '.join(map(str, dims_at(h)))} voxels of side {h:.6g} are more than max_voxels = {cap}; "
                             f"a side of {fit:.6g} would fit")
    return ops.tsdf_volume(dims_at(h), lo, h, colour=colour)


def unproject_device(depth: torch.Tensor, K, E) -> torch.Tensor:
    """depth [H,W] on a device -> the world points [H,W,3] of its pixels in fp64 (pixel centres at integer coordinates)"""
    dev = depth.device
    Kinv = torch.from_numpy(np.linalg.inv(np.asarray(K, np.float64))).to(dev)
    Einv = torch.from_numpy(np.linalg.inv(np.asarray(E, np.float64))).to(dev)
    H, W = depth.shape
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    cam = torch.stack([x, y, torch.ones_like(x)], -1) @ Kinv.T * depth.double()[..., None]
    return cam @ Einv[:3, :3].T + Einv[:3, 3]


def auto_bounds(depths: Sequence[torch.Tensor], valids: Sequence[torch.Tensor], Ks, Es, stride=4, quantiles=(0.01, 0.99), pad=0.0):
    """The box of a scene: every stride-th pixel (both ways) of every view with valid != 0 and a finite positive depth is unprojected on
    the device; per axis the points are sorted and the box runs from the `quantiles` entries (index floor(q (n - 1))), widened by pad.
    depths / valids: per view [H,W] tensors on the device (valid None: every pixel).  -> (lo [3], hi [3]) fp64"""
    pts = []
    for d, m, K, E in zip(depths, valids, Ks, Es):
        ok = torch.isfinite(d) & (d > 0)
        if m is not None:
            ok &= m != 0
        sub = (slice(None, None, int(stride)), slice(None, None, int(stride)))
        pts.append(unproject_device(torch.where(ok, d, torch.ones_like(d)), K, E)[sub][ok[sub]])
    pts = torch.cat(pts, 0) if pts else torch.zeros((0, 3), dtype=torch.float64)
    n = int(pts.shape[0])
    if n == 0:
        raise _lib.DmvsError("auto_bounds: no pixel with a usable depth")
    srt = torch.sort(pts, 0).values
    lo = srt[int(np.floor(quantiles[0] * (n - 1)))].cpu().numpy() - pad
    hi = srt[int(np.floor(quantiles[1] * (n - 1)))].cpu().numpy() + pad
    return lo, hi


def scene_views(out_folder, pair_folder, dataset):
    """the reference views of pair.txt, or without one every view that has a camera file"""
    pair = os.path.join(pair_folder, "pair.txt") if pair_folder else None
    if pair and os.path.exists(pair):
        return [ref for ref, _ in IO.read_pair_file(pair, dataset)]
    return sorted(int(f[:8]) for f in os.listdir(os.path.join(out_folder, "cams")) if f.endswith("_cam.txt"))


def mesh_scene(out_folder, pair_folder=None, dataset="dtu", voxel=None, resolution=512, trunc=4.0, min_weight=2, bounds=None, out=None,
               device="cuda:0", ops: Ops | None = None, chunk=_lib.TSDF_VIEW_CHUNK, max_voxels=2 ** 29, stride=4, colour=True,
               min_component_faces=0, simplify_voxels=None) -> dict:
    """One scene's output tree -> <out_folder>/mesh.ply (or `out`).  The truncation distance is trunc voxels; bounds (x0 y0 z0 x1 y1 z1)
    default to auto_bounds widened by tau + h.  The views stream through the volume `chunk` at a time.
    min_component_faces > 0: connected components with fewer faces are dropped before the file is written (mesh_clean.clean).
    simplify_voxels: after that the mesh is clustered on a lattice of cells this many voxels wide, anchored at the volume's origin
    (mesh_simplify.simplify).
    -> {"ply", "vertices", "faces", "dims", "voxel", "observed_voxels" (Wt >= min_weight), "views", "bounds"[, "cleaned"][, "simplified"]}"""
    from PIL import Image
    ops = ops or Ops.for_device(device)
    dev = ops.device
    ids = scene_views(out_folder, pair_folder, dataset)
    if not ids:
        raise _lib.DmvsError(f"mesh_scene: no views under {out_folder}")
    if len(ids) > _lib.TSDF_MAX_VIEWS:
        raise _lib.DmvsError(f"mesh_scene: {len(ids)} views; a volume takes at most {_lib.TSDF_MAX_VIEWS}")
    fused = os.path.isdir(os.path.join(out_folder, "depth_fused"))

    def load(v):
        k, e, _, _ = IO.read_camera_parameters(os.path.join(out_folder, f"cams/{v:0>8}_cam.txt"))
        d = np.ascontiguousarray(IO.read_pfm(os.path.join(out_folder, ("depth_fused" if fused else "depth_est") + f"/{v:0>8}.pfm"))[0], dtype=np.float32)
        mfile = os.path.join(out_folder, f"mask/{v:0>8}_final.png")
        m = (np.array(Image.open(mfile)) > 0) if os.path.exists(mfile) else (np.isfinite(d) & (d > 0))
        img = (IO.read_img(os.path.join(out_folder, f"images/{v:0>8}.jpg"))[0] * 255).astype(np.uint8) if colour else None
        if m.shape != d.shape or (img is not None and img.shape[:2] != d.shape):
            raise _lib.DmvsError(f"mesh_scene: view {v}: depth {d.shape}, mask {m.shape} and image {None if img is None else img.shape[:2]} differ in size")
        return (torch.from_numpy(d).to(dev), torch.from_numpy(np.ascontiguousarray(m, dtype=np.uint8)).to(dev),
                None if img is None else torch.from_numpy(np.ascontiguousarray(img)).to(dev), k.astype(np.float64), e.astype(np.float64))

    if bounds is None:
        views = [load(v) for v in ids]      # (the bounds need every view once; the depth maps then stay on the device)
        lo, hi = auto_bounds([w[0] for w in views], [w[1] for w in views], [w[3] for w in views], [w[4] for w in views], stride=stride)
        h = float(voxel) if voxel is not None else float((hi - lo).max()) / max(int(resolution) - 1, 1)
        lo, hi = lo - (float(trunc) * h + h), hi + (float(trunc) * h + h)
    else:
        views = None
        b = np.asarray(bounds, np.float64).reshape(2, 3)
        lo, hi = b[0], b[1]
        h = float(voxel) if voxel is not None else None
    vol = make_volume(ops, (lo, hi), voxel=h, resolution=resolution, max_voxels=max_voxels, colour=colour)
    tau = float(trunc) * vol.h
    i0 = 0
    while i0 < len(ids):
        batch = [views[i0] if views is not None else load(ids[i0])]
        while len(batch) < int(chunk) and i0 + len(batch) < len(ids):      # (views of one size go together)
            nxt = views[i0 + len(batch)] if views is not None else load(ids[i0 + len(batch)])
            if nxt[0].shape != batch[0][0].shape:
                break
            batch.append(nxt)
        ops.tsdf_integrate(vol, torch.stack([w[0] for w in batch]), torch.stack([w[1] for w in batch]),
                           torch.stack([w[2] for w in batch]) if colour else None,
                           tsdf_views(np.stack([w[3] for w in batch]), np.stack([w[4] for w in batch])), tau)
        i0 += len(batch)
    verts, rgb, faces = ops.tsdf_extract(vol, min_weight=min_weight)
    cleaned = None
    if int(min_component_faces) > 0:
        from . import mesh_clean
        verts, rgb, faces, cleaned = mesh_clean.clean(ops, verts, rgb, faces, min_faces=int(min_component_faces))
    simplified = None
    if simplify_voxels is not None:
        from . import mesh_simplify
        verts, rgb, faces, simplified = mesh_simplify.simplify(ops, verts, rgb, faces, float(simplify_voxels) * vol.h, origin=vol.origin)
    out = out or os.path.join(out_folder, "mesh.ply")
    if os.path.dirname(out):
        os.makedirs(os.path.dirname(out), exist_ok=True)
    IO.write_ply(out, verts.cpu().numpy(), rgb.cpu().numpy(), faces=faces.cpu().numpy())
    res = {"ply": out, "vertices": int(verts.shape[0]), "faces": int(faces.shape[0]), "dims": list(vol.dims), "voxel": vol.h,
           "observed_voxels": int((vol.Wt >= int(min_weight)).sum()), "views": len(ids), "bounds": [float(x) for x in np.concatenate([lo, hi])]}
    if cleaned is not None:
        res["cleaned"] = cleaned
    if simplified is not None:
        res["simplified"] = simplified
    return res


def main(argv=None, device="cuda:0", ops=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--outdir", required=True, help="the output tree of diffmvs_amd.eval (cams/, images/, depth_est/ or depth_fused/, mask/)")
    ap.add_argument("--testpath", default=None, help="the dataset root with <scene>/pair.txt (default: every view with a camera file)")
    ap.add_argument("--dataset", default="general", choices=["dtu", "tank", "eth3d", "general"])
    ap.add_argument("--testlist", default=None, help="file with one scene per line (default: the single scene '')")
    ap.add_argument("--voxel", type=float, default=None, help="voxel side in world units")
    ap.add_argument("--resolution", type=int, default=512, help="without --voxel: voxels along the longest axis of the bounds")
    ap.add_argument("--trunc", type=float, default=4.0, help="truncation distance in voxels")
    ap.add_argument("--min_weight", type=int, default=2, help="a voxel counts as observed from this many views on")
    ap.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("x0", "y0", "z0", "x1", "y1", "z1"))
    ap.add_argument("--out", default=None, help="the PLY to write (default: <outdir>/<scene>/mesh.ply)")
    ap.add_argument("--min_component", type=int, default=0, help="drop connected components with fewer faces (floaters) before writing")
    ap.add_argument("--simplify", type=float, default=None, metavar="V", help="cluster the mesh on a lattice of cells V voxels wide before writing "
                    "(diffmvs_amd.mesh_simplify; after --min_component)")
    a = ap.parse_args(argv)
    scenes = [""]
    if a.testlist:
        with open(a.testlist) as f:
            scenes = [ln.strip() for ln in f if ln.strip()]
    if a.out and len(scenes) > 1:
        raise SystemExit("--out names one file: mesh one scene at a time with it")
    res = {}
    for scene in scenes:
        res[scene] = mesh_scene(os.path.join(a.outdir, scene), os.path.join(a.testpath, scene) if a.testpath else None, a.dataset, voxel=a.voxel,
                                resolution=a.resolution, trunc=a.trunc, min_weight=a.min_weight, bounds=a.bounds, out=a.out, device=device, ops=ops,
                                min_component_faces=a.min_component, simplify_voxels=a.simplify)
    print(json.dumps({"mesh": res}), flush=True)
    return res


if __name__ == "__main__":
    main()
