"""Make an extracted mesh lighter on the MI355X: vertex clustering on a uniform lattice, each cluster's vertex at the minimum of its
faces' summed plane quadrics (dmvs_mesh_cluster_* of include/dmvs.h, csrc/mesh_simplify.hip).

    python -m diffmvs_amd.mesh_simplify --mesh in.ply --out out.ply (--cell S | --target_faces T) [--placement quadric|mean] [--reg R]

Every vertex goes to the lattice cell it lies in; a cell's vertices become one vertex, a face whose corners fall into fewer than three
cells disappears, and of several faces between the same three cells in the same orientation the first stays.  The new vertex minimises
the summed squared distances to the planes of the cluster's faces (area-weighted), pulled towards the mean of its vertices by `reg`
times the quadric's trace: on a flat patch that leaves it in the plane at the mean, on an edge or a corner it keeps the edge or the
corner.  Integer sums and fp64 in a fixed order: the same mesh gives the same result bit for bit, whatever the launch.  Output vertices
are in ascending lattice-key order, surviving faces in input order."""
from __future__ import annotations

import argparse
import json
import math

import numpy as np
import torch

from . import _lib
from . import formats as IO
from . import cloud_grid as G
from .mesh_clean import _mesh, area_scale
from .ops import Ops

MAX_WEIGHT = 1024.0      # a face larger than this many cells (in area) weighs as this many
MAX_PROBES = 16          # simplify_to_faces: cell sizes tried


def _lattice(verts: torch.Tensor, cell: float, origin=None):
    """-> (cluster [N] int32: the rank of the vertex's lattice key among the occupied keys, -1 for a vertex with a non-finite coordinate;
    cells [K,3] int64: the occupied cells in ascending key order; origin: three floats, the given one shifted by whole cells so that no
    cell is negative, by default the minimum corner of the finite vertices)"""
    if not (cell > 0 and math.isfinite(cell)):
        raise ValueError(f"cell size must be positive and finite, got {cell}")
    dev, N = verts.device, int(verts.shape[0])
    ok = torch.isfinite(verts).all(1) if N else torch.zeros(0, dtype=torch.bool, device=dev)
    cluster = torch.full((N,), -1, dtype=torch.int32, device=dev)
    if origin is not None:
        origin = tuple(float(v) for v in origin)
        if len(origin) != 3 or not all(math.isfinite(v) for v in origin):
            raise ValueError(f"the origin must be three finite numbers, got {origin}")
    if not bool(ok.any()):
        return cluster, torch.zeros((0, 3), dtype=torch.int64, device=dev), origin or (0.0, 0.0, 0.0)
    p = verts[ok]
    if origin is None:
        origin = tuple(float(v) for v in p.min(0).values.double().cpu())
    c = G.cells(p, origin, cell)
    for _ in range(4):      # (the cells are recomputed from the shifted origin: they are what the kernels' floor() gives)
        low = [int(v) for v in c.min(0).values.cpu()]
        if min(low) >= 0:
            break
        origin = tuple(o + min(v, 0) * float(cell) for o, v in zip(origin, low))
        c = G.cells(p, origin, cell)
    if int(c.min()) < 0 or not all(math.isfinite(v) for v in origin):
        raise ValueError(f"no whole-cell shift of the origin makes the cells of side {cell} non-negative")
    dims = tuple(int(v) + 1 for v in c.max(0).values.cpu())
    if sum(G.bits(n) for n in dims) > _lib.CLOUD_MAX_KEY_BITS:
        raise ValueError(f"a grid of {dims} cells of side {cell} exceeds the {_lib.CLOUD_MAX_KEY_BITS}-bit key: raise the cell size")
    keys, inverse = torch.unique(G.key(c, dims), sorted=True, return_inverse=True)
    if keys.numel() > 2 ** 31 - 1:
        raise ValueError(f"{keys.numel()} occupied cells; at most 2^31 - 1 are supported: raise the cell size")
    cluster[ok] = inverse.to(torch.int32)
    bx, by = G.bits(dims[0]), G.bits(dims[1])
    cells = torch.stack([keys & ((1 << bx) - 1), (keys >> bx) & ((1 << by) - 1), keys >> (bx + by)], 1).contiguous()
    return cluster, cells, origin


def _survivors(faces_k: torch.Tensor, keep: torch.Tensor, K: int):
    """faces_k [F,3] int32 (rotated cluster triples), keep [F] uint8 -> (the kept triples [M,3] int64 without repeats: of equal triples the
    one with the lowest input index, survivors in input order; how many repeats were dropped)"""
    idx = torch.nonzero(keep != 0).squeeze(1)
    t = faces_k[idx].long()
    M = int(t.shape[0])
    if M == 0:
        return t, 0
    order = torch.sort(t[:, 1] * int(max(K, 1)) + t[:, 2], stable=True).indices      # (K < 2^31: the pair fits an int64)
    order = order[torch.sort(t[order, 0], stable=True).indices]                      # lexicographic, equal triples in input order
    s = t[order]
    first = torch.ones(M, dtype=torch.bool, device=t.device)
    first[1:] = (s[1:] != s[:-1]).any(1)
    stay = torch.zeros(M, dtype=torch.bool, device=t.device)
    stay[order[first]] = True
    return t[stay], M - int(first.sum())


def _rgb(ops: Ops, rgb, n: int):
    if rgb is None:
        return None
    rgb = torch.as_tensor(np.ascontiguousarray(rgb) if isinstance(rgb, np.ndarray) else rgb).to(device=ops.device, dtype=torch.uint8).contiguous()
    if tuple(rgb.shape) != (n, 3):
        raise _lib.DmvsError(f"simplify: colours {tuple(rgb.shape)} for {n} vertices")
    return rgb


def _count_faces(ops: Ops, verts, faces, cell: float, origin, blocks: int) -> int:
    """the faces simplify() would leave at this cell: the lattice, the remap and the removal of repeats only"""
    cluster, cells, _ = _lattice(verts, cell, origin)
    K = int(cells.shape[0])
    faces_k, keep, _ = ops.mesh_cluster_remap(verts, faces, cluster, K, blocks=blocks)
    return int(_survivors(faces_k, keep, K)[0].shape[0])


def simplify(ops: Ops, verts, rgb, faces, cell: float, *, origin=None, placement: str = "quadric", reg: float = 2.0 ** -10, blocks: int = 0):
    """verts [N,3], rgb [N,3] uint8 or None, faces [F,3] -> (verts' fp32, rgb' or None, faces' int32, info).  cell: the lattice's side;
    origin: a lattice corner (default: the minimum corner of the finite vertices); placement "quadric" or "mean" (the cluster's mean
    vertex); reg: the pull towards the mean, as a share of the quadric's trace.  A cluster no surviving face names is dropped.  info =
    {clusters (occupied cells), vertices, faces, bad_faces (an index outside [0, N) or a non-finite vertex), flat_faces (zero or non-finite
    area: no quadric), degenerate_faces (fewer than three clusters), duplicate_faces, flipped_faces (survivors of the degenerate test whose
    normal turned by more than a right angle), fallback_clusters (quadric placement left its cell or was singular: placed at the mean), cell,
    origin, scale}"""
    if placement not in ("quadric", "mean"):
        raise ValueError(f"placement must be 'quadric' or 'mean', got {placement!r}")
    if not (reg > 0 and math.isfinite(reg)):
        raise ValueError(f"reg must be positive and finite, got {reg}")
    verts, faces = _mesh(ops, verts, faces)
    N, F = int(verts.shape[0]), int(faces.shape[0])
    rgb = _rgb(ops, rgb, N)
    cluster, cells, origin = _lattice(verts, float(cell), origin)
    K = int(cells.shape[0])
    big = area_scale(verts, F)
    cap = min(MAX_WEIGHT, (big[1] / big[0]) / (float(cell) * float(cell)))
    scale = G.pow2_scale_below(cap, 3 * F)
    cnt, pos_q, rgb_sum = ops.mesh_cluster_verts(verts, rgb, cluster, K, origin, cell, blocks=blocks)
    quad_q, st_sum = ops.mesh_cluster_quadrics(verts, faces, cluster, K, origin, cell, scale, cap, blocks=blocks)
    new_verts, new_rgb, st_place = ops.mesh_cluster_place(cnt, pos_q, rgb_sum, quad_q, cells, origin, cell, scale, reg, mean=placement == "mean")
    faces_k, keep, st_map = ops.mesh_cluster_remap(verts, faces, cluster, K, new_verts=new_verts, blocks=blocks)
    kept, repeats = _survivors(faces_k, keep, K)
    used = torch.zeros(K, dtype=torch.bool, device=ops.device)
    used[kept.reshape(-1)] = True
    new_index = torch.cumsum(used, 0) - 1
    bad, flat = (int(v) for v in st_sum.cpu())
    degenerate, flipped, _ = (int(v) for v in st_map.cpu())
    info = {"clusters": K, "vertices": int(used.sum()), "faces": int(kept.shape[0]), "bad_faces": bad, "flat_faces": flat,
            "degenerate_faces": degenerate, "duplicate_faces": repeats, "flipped_faces": flipped, "fallback_clusters": int(st_place.cpu()[0]),
            "cell": float(cell), "origin": [float(v) for v in origin], "scale": scale}
    return new_verts[used], None if new_rgb is None else new_rgb[used], new_index[kept].to(torch.int32).reshape(-1, 3), info


def simplify_to_faces(ops: Ops, verts, rgb, faces, target_faces: int, *, origin=None, placement: str = "quadric", reg: float = 2.0 ** -10,
                      blocks: int = 0):
    """simplify() at the smallest cell, of at most 16 tried, that leaves at most target_faces faces: the longest side of the vertices'
    bounding box first, then a bisection (in the logarithm) down towards the shortest side / 2^20; a probe runs the lattice, the remap and
    the removal of repeats only.  info gains `probes`."""
    verts, faces = _mesh(ops, verts, faces)
    target = int(target_faces)
    ok = torch.isfinite(verts).all(1) if verts.shape[0] else None
    if ok is None or not bool(ok.any()):
        raise _lib.DmvsError("simplify_to_faces: no vertex with finite coordinates")
    ext = (verts[ok].max(0).values - verts[ok].min(0).values).double().cpu().numpy()
    hi = float(ext.max())
    if not (hi > 0 and math.isfinite(hi)):
        raise _lib.DmvsError("simplify_to_faces: the vertices' bounding box has no extent")
    lo = float(ext[ext > 0].min()) / 2.0 ** 20

    def count(cell):
        try:
            return _count_faces(ops, verts, faces, cell, origin, blocks)
        except ValueError as e:      # (more cells than the key holds: as too many faces)
            if "exceeds" not in str(e):
                raise
            return None

    n = count(hi)
    probes, best = 1, hi
    if n is None or n > target:
        raise _lib.DmvsError(f"simplify_to_faces: {n} faces are left at a cell of the bounding box's longest side {hi:.6g}; target_faces = {target}")
    while probes < MAX_PROBES and n != target and hi / lo > 1.0 + 2.0 ** -10:
        mid = math.sqrt(lo * hi)
        n_mid = count(mid)
        probes += 1
        if n_mid is not None and n_mid <= target:
            hi, best, n = mid, mid, n_mid
        else:
            lo = mid
    v, c, f, info = simplify(ops, verts, rgb, faces, best, origin=origin, placement=placement, reg=reg, blocks=blocks)
    return v, c, f, dict(info, probes=probes)


def simplify_file(ops: Ops, mesh_ply: str, out_ply: str, cell=None, target_faces=None, **kw) -> dict:
    if (cell is None) == (target_faces is None):
        raise ValueError("simplify_file: give a cell or target_faces, one of the two")
    verts, rgb, faces = IO.read_ply_mesh(mesh_ply)
    if cell is not None:
        v, c, f, info = simplify(ops, verts, rgb, faces, float(cell), **kw)
    else:
        v, c, f, info = simplify_to_faces(ops, verts, rgb, faces, int(target_faces), **kw)
    colours = c.cpu().numpy() if c is not None else np.zeros((int(v.shape[0]), 3), np.uint8)
    IO.write_ply(out_ply, v.cpu().numpy(), colours, faces=f.cpu().numpy())
    return dict(info, ply=out_ply, faces_in=int(np.asarray(faces).shape[0]), vertices_in=int(np.asarray(verts).shape[0]))


def main(argv=None, device="cuda:0", ops=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="the triangle mesh to simplify (binary PLY)")
    ap.add_argument("--out", required=True, help="the PLY to write")
    size = ap.add_mutually_exclusive_group(required=True)
    size.add_argument("--cell", type=float, default=None, help="the lattice's cell side in world units")
    size.add_argument("--target_faces", type=int, default=None, help="the smallest cell (of at most 16 tried) that leaves at most this many faces")
    ap.add_argument("--placement", default="quadric", choices=["quadric", "mean"])
    ap.add_argument("--reg", type=float, default=2.0 ** -10, help="pull towards the cluster's mean vertex, as a share of the quadric's trace")
    a = ap.parse_args(argv)
    res = simplify_file(ops or Ops.for_device(device), a.mesh, a.out, cell=a.cell, target_faces=a.target_faces, placement=a.placement, reg=a.reg)
    print(json.dumps({"mesh_simplify": res}), flush=True)
    return res


if __name__ == "__main__":
    main()
