"""What the point-cloud tools (diffmvs_amd.cloud_eval, diffmvs_amd.cloud_register) stand on: clouds as [N,3] fp32 tensors, the uniform
grid the search kernels walk (cell coordinates, the key with power-of-two strides, the sorted target and its cell table), the voxel
thinning and the power-of-two scale of the fixed-point sums.  torch only: the kernels themselves are reached through Ops."""
from __future__ import annotations

import math

import numpy as np
import torch

from . import _lib

NEAR_RINGS = 4      # nn_distance: the fine pass searches this many cells far ...
FAR_RINGS = 8       # ... the coarse pass covers max_dist in this many


def to_cloud(ops, x) -> torch.Tensor:
    t = torch.as_tensor(np.ascontiguousarray(x) if isinstance(x, np.ndarray) else x)
    if t.dim() != 2 or t.shape[1] != 3:
        raise ValueError(f"a cloud is an [N,3] array, got {tuple(t.shape)}")
    return t.to(device=ops.device, dtype=torch.float32).contiguous()


def pow2_scale_below(big: float, n: int) -> float:
    """the largest power of two with big * scale * max(n, 1) < 2^62: a u64 sum of n terms rint(v * scale), |v| <= big, cannot overflow"""
    big, n = float(big), max(1, n)
    e = math.floor(math.log2(2.0 ** 62 / (big * n)))
    while big * 2.0 ** e * n >= 2.0 ** 62:
        e -= 1
    return 2.0 ** e


# ------------------------------------------------------------------------------------------ cells and keys
def bits(n: int) -> int:
    return max(0, int(n) - 1).bit_length()


def cells(xyz: torch.Tensor, origin, h: float) -> torch.Tensor:
    """integer cell coordinates floor((p - origin) / h) in fp64: the arithmetic the kernel repeats for its queries"""
    o = torch.tensor(list(origin), dtype=torch.float64, device=xyz.device)
    return torch.floor((xyz.double() - o) / float(h)).long()


def key(c: torch.Tensor, dims) -> torch.Tensor:
    """cell coordinates [N,3] -> (z << (bx + by)) | (y << bx) | x: cells adjacent in x are adjacent in key order"""
    bx, by = bits(dims[0]), bits(dims[1])
    return (c[:, 2] << (bx + by)) | (c[:, 1] << bx) | c[:, 0]


def build_grid(target: torch.Tensor, cell: float) -> dict:
    """sort `target` [M,3] fp32 into a uniform grid of cell side `cell` whose origin is the cloud's minimum corner.
    -> {target (sorted), keys [C], start [C+1], origin, dims, cell}: the operands of Ops.cloud_nn_dist; and order [M] int64, the input
    position of every sorted target (target_sorted = target[order]: what a self search scatters its results back with)"""
    if not (cell > 0 and math.isfinite(cell)):
        raise ValueError(f"cell size must be positive and finite, got {cell}")
    dev = target.device
    if target.shape[0] == 0:
        z = torch.zeros(0, dtype=torch.int64, device=dev)
        return {"target": target.reshape(0, 3).contiguous(), "keys": z, "start": torch.zeros(1, dtype=torch.int64, device=dev),
                "origin": (0.0, 0.0, 0.0), "dims": (1, 1, 1), "cell": float(cell), "order": z}
    if not bool(torch.isfinite(target).all()):
        raise ValueError("the target cloud holds non-finite coordinates")
    lo = target.min(0).values.double()
    origin = tuple(float(v) for v in lo.cpu())
    c = cells(target, origin, cell)
    dims = tuple(int(v) + 1 for v in c.max(0).values.cpu())
    if sum(bits(n) for n in dims) > _lib.CLOUD_MAX_KEY_BITS:
        raise ValueError(f"a grid of {dims} cells of side {cell} exceeds the {_lib.CLOUD_MAX_KEY_BITS}-bit key: raise the cell size")
    skey, order = torch.sort(key(c, dims))
    keys, counts = torch.unique_consecutive(skey, return_counts=True)
    start = torch.zeros(keys.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=start[1:])
    return {"target": target[order].contiguous(), "keys": keys, "start": start, "origin": origin, "dims": dims, "cell": float(cell),
            "order": order}


def order_by_grid(points: torch.Tensor, grid: dict):
    """the order of `points` by the grid's key (non-finite coordinates and cells outside the grid clamped into it): neighbouring lanes
    then walk and gather the same cells.  None when there is nothing to sort (no points, or an empty grid)"""
    if points.shape[0] == 0 or grid["keys"].numel() == 0:
        return None
    dims = grid["dims"]
    hi = torch.tensor([n - 1 for n in dims], device=points.device)
    c = cells(torch.nan_to_num(points, nan=0.0, posinf=3e38, neginf=-3e38), grid["origin"], grid["cell"])
    return torch.sort(key(torch.minimum(c.clamp_min_(0), hi), dims)).indices


def estimate_spacing(points: torch.Tensor, probe: float) -> float:
    """typical distance between neighbouring points of a SURFACE sample: with n points in an occupied probe cell of side s, a
    surface patch of area ~ s^2 holds them at spacing s / sqrt(n)"""
    if points.shape[0] < 2:
        return float(probe)
    lo = points.min(0).values.double()
    c = torch.floor((points.double() - lo) / probe).long()
    c = c - c.min(0).values
    ny, nz = int(c[:, 1].max()) + 1, int(c[:, 2].max()) + 1
    occupied = torch.unique((c[:, 0] * ny + c[:, 1]) * nz + c[:, 2]).numel()
    return float(probe / math.sqrt(max(1.0, points.shape[0] / occupied)))


# ------------------------------------------------------------------------------------------ thinning
def voxel_downsample(xyz, voxel: float):
    """keep, per occupied voxel of side `voxel` (lattice anchored at the coordinate origin), the point with the lowest input
    index.  -> (points [K,3], index [K] int64 ascending) on the input's device.

    This STANDS IN for the DTU scorer's thinning and is not the same algorithm: the MATLAB program walks the points in input
    order and drops every point closer than `voxel` to one it has kept (greedy, serial, order-dependent; kept points are at
    least `voxel` apart), whereas a voxel lattice keeps points that may be arbitrarily close across a voxel face and about as
    many per area.  Scores computed after this thinning are therefore close to the official ones, not identical to them."""
    t = torch.as_tensor(np.ascontiguousarray(xyz) if isinstance(xyz, np.ndarray) else xyz)
    if not (voxel > 0 and math.isfinite(voxel)):
        raise ValueError(f"voxel size must be positive and finite, got {voxel}")
    if t.shape[0] == 0:
        return t, torch.zeros(0, dtype=torch.int64, device=t.device)
    c = torch.floor(t.double() / float(voxel)).long()
    c = c - c.min(0).values
    n = [int(v) + 1 for v in c.max(0).values.cpu()]
    if sum(bits(v) for v in n) > _lib.CLOUD_MAX_KEY_BITS:
        raise ValueError(f"a lattice of {n} voxels of side {voxel} exceeds the {_lib.CLOUD_MAX_KEY_BITS}-bit key")
    skey, order = torch.sort(key(c, n), stable=True)      # stable: the first entry of a run of equal keys is the lowest input index
    first = torch.ones_like(skey, dtype=torch.bool)
    first[1:] = skey[1:] != skey[:-1]
    idx = torch.sort(order[first]).values
    return t[idx], idx
