"""Clean a fused point cloud on the GPU: drop the isolated points ("floaters") that two views happened to agree on, before the cloud
is meshed, uploaded or looked at.

    python -m diffmvs_amd.cloud_clean --cloud in.ply --out out.ply [--voxel V] [--min_neighbours N --radius R] [--knn K --std_ratio S]
                                      [--max_dist D] [--cell C]

Both common filters stand on ONE search, dmvs_cloud_knn_f32 (csrc/cloud_clean.hip): the k nearest OTHER points of every point, over
the grid, the key and the pruned walk of the scorer (cloud_grid.py, csrc/cloud_walk.h).

  radius filter (Open3D remove_radius_outlier): keep a point with at least N other points strictly closer than R.  That is exactly
      "its N-th nearest neighbour is closer than R": a search with k = N, max_dist = R, keep where all N were found.
  statistical filter (Open3D remove_statistical_outlier, PCL StatisticalOutlierRemoval): with m_i the mean distance of point i to its
      K nearest neighbours, keep m_i <= mean(m) + S * std(m).  Here the statistics are exact integers: q_i = rint(m_i * scale) with a
      power-of-two scale, n, sum q and sum q^2 as integers, mean and population deviation from those in fp64, and the comparison on the
      integers -- so the kept set is the same bits on every run, for any order of the input and any cell size.
      The search is bounded by max_dist.  A point with fewer than K neighbours inside max_dist counts as ISOLATED: it is dropped and
      left out of the statistics (its mean over fewer neighbours would not compare with the others').  By default max_dist is
      NEAR_RINGS cells = 8 typical point spacings (cell = 2 * the spacing estimated from the cloud's density).

clean() runs, in this order and each on the survivors of the one before: non-finite coordinates out, the voxel thinning of
cloud_grid.voxel_downsample, the radius filter, the statistical filter.  Survivors keep their input order; colours and normals follow.
"""
from __future__ import annotations

import argparse
import json
import math

import numpy as np
import torch

from . import _lib
from . import formats as IO
from .cloud_grid import FAR_RINGS, NEAR_RINGS, build_grid, estimate_spacing, to_cloud, voxel_downsample
from .ops import Ops

FIXED_POINT_BITS = 30      # the statistical filter's q = rint(mean * scale) stays <= 2^30: q^2 fits 64 bits


def default_cell(points: torch.Tensor) -> float:
    """twice the typical point spacing, estimated with probe cells of 1/128 of the longest box side (1.0 for a cloud without extent)"""
    if points.shape[0] < 2:
        return 1.0
    side = float((points.max(0).values.double() - points.min(0).values.double()).max())
    return 2.0 * estimate_spacing(points, side / 128.0) if side > 0.0 else 1.0


def _search_cell(cell: float, max_dist: float) -> float:
    """the grid of a search out to max_dist: the given cell, raised so that max_dist is at most FAR_RINGS cells (the walk looks through
    up to (2R + 1)^2 rows of cells, R = max_dist / cell, around a point that has nothing near it)"""
    return max(float(cell), float(max_dist) / FAR_RINGS)


def knn(ops: Ops, points, k: int, max_dist: float, cell: float | None = None, d2: bool = False, work: bool = False) -> dict:
    """the k nearest OTHER points of every point of a cloud (finite coordinates), closer than max_dist: a self search.  The cloud sorted
    into its grid is target and query at once, every query excludes its own position, and the results are scattered back.
    -> {"mean" [N] fp32: mean distance to the found neighbours (max_dist where none), "kth" [N] fp32: distance to the k-th (max_dist where
    fewer were found), "found" [N] int32[, "d2" [N,k] fp32 ascending, padded with max_dist^2][, "work" [N,2] int32]} in input order.
    Nothing depends on `cell` but the time (include/dmvs.h)."""
    if not (max_dist > 0 and math.isfinite(max_dist)):
        raise ValueError(f"max_dist must be positive and finite, got {max_dist}")
    if not 1 <= int(k) <= _lib.CLOUD_MAX_K:
        raise ValueError(f"k = {k}; 1..{_lib.CLOUD_MAX_K} neighbours are supported")
    pts = to_cloud(ops, points)
    cell = _search_cell(default_cell(pts), max_dist) if cell is None else float(cell)
    if math.ceil(max_dist / cell) > _lib.CLOUD_MAX_RINGS:
        raise ValueError(f"max_dist / cell = {max_dist / cell:.0f} rings; at most {_lib.CLOUD_MAX_RINGS} are supported: raise the cell size")
    grid = build_grid(pts, cell)
    order = grid["order"]
    me = torch.arange(pts.shape[0], dtype=torch.int32, device=pts.device)
    res = ops.cloud_knn(grid["target"], grid["target"], grid["keys"], grid["start"], grid["origin"], grid["cell"], grid["dims"], max_dist, int(k),
                        self_index=me, d2=d2, work=work)
    out = {}
    for name, r in res.items():
        out[name] = torch.empty_like(r)
        out[name][order] = r
    return out


_search = knn      # (clean() has a parameter of that name)


def statistics(mean: torch.Tensor, max_dist: float) -> dict:
    """the exact statistics of the statistical filter over mean distances (all <= max_dist): q = rint((double)mean * scale) as int64,
    scale the largest power of two with max_dist * scale <= 2^30; n, sum q, sum q^2 as Python integers (torch's int64 sums are exact;
    q^2 is summed as its high and low 30 bits); mu = S1 / n and the population deviation sd = sqrt(S2 n - S1^2) / n in fp64.
    -> {"q", "scale", "n", "S1", "S2", "mu", "sd"} with mu and sd in units of 1 / scale"""
    e = math.floor(math.log2(2.0 ** FIXED_POINT_BITS / max_dist))
    while max_dist * 2.0 ** e > 2.0 ** FIXED_POINT_BITS:
        e -= 1
    scale = 2.0 ** e
    q = torch.round(mean.double() * scale).long()          # (torch.round is round-half-to-even: rint)
    n = int(q.numel())
    sq = q * q
    S1 = int(q.sum())
    S2 = (int((sq >> FIXED_POINT_BITS).sum()) << FIXED_POINT_BITS) + int((sq & ((1 << FIXED_POINT_BITS) - 1)).sum())
    mu = S1 / n if n else None
    sd = math.sqrt(S2 * n - S1 * S1) / n if n else None
    return {"q": q, "scale": scale, "n": n, "S1": S1, "S2": S2, "mu": mu, "sd": sd}


def _take(a, keep: torch.Tensor):
    if a is None:
        return None
    return a[keep.to(a.device)] if torch.is_tensor(a) else np.asarray(a)[keep.cpu().numpy()]


def clean(ops: Ops, xyz, rgb=None, normals=None, voxel: float | None = None, min_neighbours: int | None = None, radius: float | None = None,
          knn: int | None = None, std_ratio: float = 2.0, max_dist: float | None = None, cell: float | None = None):
    """-> (xyz', rgb', normals', keep, info): the rows of the inputs that survive, in input order (arrays stay arrays, tensors tensors);
    keep [N] bool on the binding's device; info = {"points", "kept", "removed": the count each stage dropped, "mu", "sd", "threshold":
    the statistical filter's mean, deviation and bound in length units (None when it did not run), "cell", "max_dist"}.

    voxel: thin to one point per voxel of this side (cloud_grid.voxel_downsample: the lowest input index of a voxel stays).
    min_neighbours, radius (together): keep a point with at least min_neighbours others strictly closer than radius.
    knn, std_ratio: the statistical filter over the mean distance to the knn nearest neighbours (the module's docstring);
    max_dist bounds its search: a point with fewer than knn neighbours inside it is isolated and dropped.  Default NEAR_RINGS * cell.
    cell: the side of the grid cells of both searches (raised where a search radius exceeds FAR_RINGS of them); default: twice the
    point spacing estimated from the survivors that reach the first search.  The result does not depend on it."""
    if (min_neighbours is None) != (radius is None):
        raise ValueError("min_neighbours and radius go together")
    for name, v in (("min_neighbours", min_neighbours), ("knn", knn)):
        if v is not None and not 1 <= int(v) <= _lib.CLOUD_MAX_K:
            raise ValueError(f"{name} = {v}; 1..{_lib.CLOUD_MAX_K} neighbours are supported")
    for name, v in (("radius", radius), ("max_dist", max_dist), ("cell", cell)):
        if v is not None and not (v > 0 and math.isfinite(v)):
            raise ValueError(f"{name} must be positive and finite, got {v}")
    if not (std_ratio >= 0 and math.isfinite(std_ratio)):
        raise ValueError(f"std_ratio must be finite and not negative, got {std_ratio}")
    pts = to_cloud(ops, xyz)
    N = int(pts.shape[0])
    for name, a in (("rgb", rgb), ("normals", normals)):
        if a is not None and len(a) != N:
            raise ValueError(f"{name} has {len(a)} rows, the cloud {N}")
    removed = {}
    idx = torch.nonzero(torch.isfinite(pts).all(1)).squeeze(1)          # the survivors so far, as ascending input positions
    removed["non_finite"] = N - int(idx.numel())
    if voxel is not None:
        sub = voxel_downsample(pts[idx], float(voxel))[1]
        removed["voxel"] = int(idx.numel() - sub.numel())
        idx = idx[sub]
    info = {"points": N, "mu": None, "sd": None, "threshold": None, "cell": None, "max_dist": None}
    if (min_neighbours is not None or knn is not None) and cell is None:
        cell = default_cell(pts[idx])
    info["cell"] = cell
    if min_neighbours is not None:
        found = _search(ops, pts[idx], int(min_neighbours), float(radius), _search_cell(cell, radius))["found"]
        ok = found == int(min_neighbours)
        removed["radius"] = int((~ok).sum())
        idx = idx[ok]
    if knn is not None:
        md = float(np.float32(NEAR_RINGS * cell if max_dist is None else max_dist))      # (the kernel's clamp is fp32)
        info["max_dist"] = md
        res = _search(ops, pts[idx], int(knn), md, _search_cell(cell, md))
        full = res["found"] == int(knn)
        removed["isolated"] = int((~full).sum())
        idx = idx[full]
        st = statistics(res["mean"][full], md)
        removed["statistical"] = 0
        if st["n"]:
            bound = math.floor(st["mu"] + float(std_ratio) * st["sd"])
            ok = st["q"] <= bound
            removed["statistical"] = int((~ok).sum())
            idx = idx[ok]
            info.update(mu=st["mu"] / st["scale"], sd=st["sd"] / st["scale"], threshold=bound / st["scale"])
    keep = torch.zeros(N, dtype=torch.bool, device=pts.device)
    keep[idx] = True
    info.update(kept=int(idx.numel()), removed=removed)
    return _take(xyz, keep), _take(rgb, keep), _take(normals, keep), keep, info


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cloud", required=True, help="the cloud to clean (PLY; colours and, if present, normals are carried through)")
    ap.add_argument("--out", required=True, help="the cleaned cloud (PLY)")
    ap.add_argument("--voxel", type=float, default=None, help="first thin to one point per voxel of this side")
    ap.add_argument("--min_neighbours", type=int, default=None, help="radius filter: keep points with at least N others closer than --radius (1..%d)" % _lib.CLOUD_MAX_K)
    ap.add_argument("--radius", type=float, default=None)
    ap.add_argument("--knn", type=int, default=None, help="statistical filter over the mean distance to the K nearest neighbours (1..%d)" % _lib.CLOUD_MAX_K)
    ap.add_argument("--std_ratio", type=float, default=2.0, help="--knn: keep mean distances up to the cloud's mean + this many deviations")
    ap.add_argument("--max_dist", type=float, default=None, help="--knn: the search radius; a point with fewer than K neighbours inside it is dropped as "
                    "isolated (default: %d grid cells = %d point spacings)" % (NEAR_RINGS, 2 * NEAR_RINGS))
    ap.add_argument("--cell", type=float, default=None, help="side of the grid cells (default: twice the estimated point spacing; changes the time only)")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    xyz, rgb, nrm = IO.read_ply(a.cloud, with_normals=True)
    xyz, rgb, nrm, _, info = clean(Ops.for_device(a.device), xyz, rgb, nrm, voxel=a.voxel, min_neighbours=a.min_neighbours, radius=a.radius, knn=a.knn,
                                   std_ratio=a.std_ratio, max_dist=a.max_dist, cell=a.cell)
    IO.write_ply(a.out, xyz, rgb, nrm)
    res = {"cloud_clean": info}
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
