"""Scores of a fused point cloud against a ground-truth cloud: accuracy, completeness, F-score.

    python -m diffmvs_amd.cloud_eval --pred pc.ply --gt gt.ply --max_dist 20 --density 0.2 --thresholds 1 2 5 \\
        [--dtu_obs_mask ObsMask/ObsMask1_10.mat --dtu_plane ObsMask/Plane1.mat | --roi roi.npz] [--error_ply out.ply]

The definitions are those of the DTU scorer (accuracy = mean distance from the prediction to the ground truth over the points
closer than max_dist, completeness = the same from the ground truth to the prediction, overall = their mean) and of the
Tanks&Temples / ETH3D F-score (precision / recall = the share of prediction / ground-truth points closer than a threshold,
fscore = 2 P R / (P + R)).  Both are two nearest-neighbour searches between the clouds; they run on the GPU
(dmvs_cloud_nn_dist_f32, dmvs_cloud_stats_f32: csrc/cloud_eval.hip), torch sorts the points into the uniform grid the kernel
walks.  Clouds that do not share a frame and a region of interest yet are aligned and cropped first: --transform T.txt (a 4x4
alignment), --register MAX_CORR (ICP refinement of it on the GPU) and --crop crop.json (a Tanks&Temples crop volume) -- see
diffmvs_amd.cloud_register.  The official MATLAB / Tanks&Temples tools remain the authority for published numbers:
`voxel_downsample` (diffmvs_amd.cloud_grid) is NOT the DTU scorer's thinning (see its docstring)."""
from __future__ import annotations

import argparse
import json
import math

import numpy as np
import torch

from . import _lib
from . import cloud_register as CR
from . import formats as IO
from .cloud_grid import FAR_RINGS, NEAR_RINGS, build_grid, estimate_spacing, order_by_grid, pow2_scale_below, to_cloud, voxel_downsample  # noqa: F401
from .ops import Ops


# ------------------------------------------------------------------------------------------ search
def grid_nn(ops: Ops, query: torch.Tensor, grid: dict, max_dist: float, work: bool = False):
    """one launch of the kernel on a built grid: the queries are sorted by the grid's key first (neighbouring lanes then read the
    same cells) and the results scattered back.  -> dist [Q] fp32 (and work [Q,2] int32 with work=True)"""
    order = order_by_grid(query, grid)
    q = query.contiguous() if order is None else query[order].contiguous()
    res = ops.cloud_nn_dist(q, grid["target"], grid["keys"], grid["start"], grid["origin"], grid["cell"], grid["dims"], max_dist, work=work)
    if order is None:
        return res

    def unsort(r):
        out = torch.empty_like(r)
        out[order] = r
        return out
    return (unsort(res[0]), unsort(res[1])) if work else unsort(res)


def nn_distance(ops: Ops, query, target, max_dist: float, cell: float | None = None, passes: int = 2, stats: dict | None = None) -> torch.Tensor:
    """min(|q - nearest target|, max_dist) for every query, fp32 [Q] on the binding's device.

    cell: the side of the grid cells; default: twice the target's point spacing (about four surface points per cell), estimated
    from its density.  It is NOT max_dist: with DTU's protocol max_dist is 100 point spacings, and a cell of that size would be
    brute force.  But a query with nothing near it has to look through up to (2R + 1)^2 rows of cells, R = ceil(max_dist / cell),
    to know so.  Hence two passes (passes=2): the first searches the fine grid only NEAR_RINGS cells far (the kernel's clamp makes
    that a search of its own); the queries it leaves at its clamp -- outliers and holes, a few per cent of a fused cloud -- go
    through a second launch on a coarse grid of cell max_dist / FAR_RINGS.  passes=1 is one launch on the grid of side `cell`
    with the full max_dist.  The result does not depend on `cell` or `passes` (the kernel returns the exact minimum of the fp32
    distances).  stats: a dict that receives the early-exit figures (tools/cloud_eval_bench.py)."""
    if not (max_dist > 0 and math.isfinite(max_dist)):
        raise ValueError(f"max_dist must be positive and finite, got {max_dist}")
    query, target = to_cloud(ops, query), to_cloud(ops, target)
    if cell is None:
        cell = min(float(max_dist), 2.0 * estimate_spacing(target, max_dist / FAR_RINGS)) if target.shape[0] else float(max_dist)
    cell = float(cell)
    near = float(np.float32(NEAR_RINGS * cell))      # (the kernel's clamp is fp32: the unresolved queries sit exactly here)
    want = stats is not None
    if passes == 1 or near >= max_dist or target.shape[0] == 0:
        if math.ceil(max_dist / cell) > _lib.CLOUD_MAX_RINGS:
            raise ValueError(f"max_dist / cell = {max_dist / cell:.0f} rings; at most {_lib.CLOUD_MAX_RINGS} are supported: raise the cell size")
        res = grid_nn(ops, query, build_grid(target, cell), max_dist, work=want)
        if want:
            stats.update(_work_stats(res[1], None, cell, None))
            return res[0]
        return res
    res = grid_nn(ops, query, build_grid(target, cell), near, work=want)
    d, wk = res if want else (res, None)
    far = torch.nonzero(d >= near).squeeze(1)
    wk2 = None
    if far.numel():
        cell2 = max(cell, float(max_dist) / FAR_RINGS)
        res2 = grid_nn(ops, query[far].contiguous(), build_grid(target, cell2), max_dist, work=want)
        d[far] = res2[0] if want else res2
        wk2 = res2[1] if want else None
    if want:
        stats.update(_work_stats(wk, wk2, cell, max(cell, float(max_dist) / FAR_RINGS)))
    return d


def _work_stats(wk, wk2, cell, cell2) -> dict:
    n = max(1, wk.shape[0])
    out = {"cell": cell, "queries": int(wk.shape[0]), "early_exit_rate": float((wk[:, 0] <= 2).sum()) / n,
           "mean_targets_tested": float(wk[:, 1].double().mean()) if wk.shape[0] else 0.0}
    if wk2 is not None:
        out.update({"far_cell": cell2, "far_queries": int(wk2.shape[0]), "far_share": wk2.shape[0] / n,
                    "far_mean_targets_tested": float(wk2[:, 1].double().mean())})
    return out


# ------------------------------------------------------------------------------------------ region of interest
def make_roi(mask, origin, resolution: float, plane=None) -> dict:
    """mask: boolean voxel volume [X,Y,Z]; a point p belongs to voxel round((p - origin) / resolution) (nearest voxel, half away from
    zero: the DTU scorer's indexing of ObsMask).  plane: optional (a, b, c, d); the half-space kept is a x + b y + c z + d > 0."""
    mask = np.asarray(mask).astype(bool)
    if mask.ndim != 3:
        raise ValueError("the ROI mask is a 3-D boolean volume")
    return {"mask": mask, "origin": np.asarray(origin, np.float64).reshape(3), "resolution": float(resolution),
            "plane": None if plane is None else np.asarray(plane, np.float64).reshape(4)}


def load_roi(path: str) -> dict:
    """an ROI saved with numpy.savez(path, mask=, origin=, resolution=[, plane=])"""
    z = np.load(path, allow_pickle=False)
    return make_roi(z["mask"], z["origin"], float(z["resolution"]), z["plane"] if "plane" in z.files else None)


def load_dtu_roi(obs_mask_mat: str, plane_mat: str | None = None) -> dict:
    """DTU's ObsMask/ObsMask<scan>_10.mat (ObsMask, BB, Res) and ObsMask/Plane<scan>.mat (P).  Needs scipy for the .mat container."""
    try:
        from scipy.io import loadmat
    except ImportError as e:
        raise ImportError("load_dtu_roi reads MATLAB .mat files through scipy (scipy.io.loadmat), which is not installed; "
                          "convert the masks with numpy.savez(mask=, origin=, resolution=, plane=) and use load_roi / --roi instead") from e
    m = loadmat(obs_mask_mat)
    plane = None if plane_mat is None else np.asarray(loadmat(plane_mat)["P"], np.float64).reshape(4)
    return make_roi(m["ObsMask"], np.asarray(m["BB"], np.float64)[0], float(np.asarray(m["Res"]).reshape(-1)[0]), plane)


def roi_volume_mask(points: torch.Tensor, roi: dict) -> torch.Tensor:
    """points [N,3] -> uint8 [N]: 1 where the point's voxel exists and is set"""
    dev = points.device
    vol = torch.from_numpy(roi["mask"]).to(dev)
    u = (points.double() - torch.from_numpy(roi["origin"]).to(dev)) / roi["resolution"]
    v = (torch.sign(u) * torch.floor(u.abs() + 0.5)).long()
    shape = torch.tensor(vol.shape, device=dev)
    inside = ((v >= 0) & (v < shape)).all(1)
    v = torch.minimum(v.clamp_min(0), shape - 1)
    return (inside & vol[v[:, 0], v[:, 1], v[:, 2]]).to(torch.uint8).contiguous()


def roi_plane_mask(points: torch.Tensor, roi: dict):
    if roi["plane"] is None:
        return None
    p = torch.from_numpy(roi["plane"]).to(points.device)
    return ((points.double() @ p[:3] + p[3]) > 0).to(torch.uint8).contiguous()


# ------------------------------------------------------------------------------------------ metrics
def fixed_scale(max_dist: float, n: int) -> float:
    """the largest power of two with max_dist * scale * max(n, 1) < 2^62: the u64 sum of rint(d * scale) cannot overflow"""
    return pow2_scale_below(max_dist, n)


def side_stats(ops: Ops, dist: torch.Tensor, valid, max_dist: float, thresholds, blocks: int = 0) -> dict:
    """one direction's counters -> {points, valid, in_range, out_of_range, sum_fixed, scale, mean, below: [..]} (python ints; mean is None when no point is in range)"""
    scale = fixed_scale(max_dist, dist.numel())
    raw = [int(v) for v in ops.cloud_stats(dist, valid, max_dist, thresholds, scale, blocks=blocks).cpu()]
    n_valid, n_in, s = raw[0], raw[1], raw[2]
    return {"points": int(dist.numel()), "valid": n_valid, "in_range": n_in, "out_of_range": n_valid - n_in, "sum_fixed": s, "scale": scale,
            "mean": (s / scale / n_in) if n_in else None, "below": raw[3:]}


def evaluate(ops: Ops, pred, gt, max_dist: float, thresholds, density: float | None = None, roi: dict | None = None, cell: float | None = None,
             return_distances: bool = False, transform=None, crop: dict | None = None, register: dict | None = None) -> dict:
    """pred, gt: [N,3] clouds (numpy or torch).  density: thin the prediction with voxel_downsample(pred, density) first (the
    ground truth is taken as it is).  roi (make_roi / load_roi / load_dtu_roi): prediction points outside the volume are left out
    of accuracy and precision, ground-truth points outside the half-space out of completeness and recall -- both searches still
    run against the WHOLE other cloud, as the DTU scorer's do.
    -> accuracy, completeness, overall, thresholds, precision / recall / fscore per threshold, and the counters of both
    directions under "pred" and "gt" (points, valid, in_range, out_of_range, sum_fixed, scale, below).

    transform: a 4x4 that moves the prediction into the ground truth's frame first.  register: keyword arguments of
    cloud_register.register (e.g. {"schedule": [(voxel, max_corr, max_iter)], "with_scale": False}) -- the transform (identity if
    none) is refined by ICP of the thinned prediction onto the ground truth before it is applied.  crop (cloud_register.make_crop /
    load_crop_json): moved prediction points outside the volume are left out of accuracy / precision, ground-truth points outside it
    out of completeness / recall, through the same masks as `roi`.  With any of the three the result also holds "transformation"
    (and "registration"); without them nothing changes."""
    thresholds = [float(t) for t in thresholds]
    pred, gt = to_cloud(ops, pred), to_cloud(ops, gt)
    n_pred_in = int(pred.shape[0])
    kept = None
    if density is not None:
        pred, kept = voxel_downsample(pred, density)
        pred = pred.contiguous()
    if cell is None and density is not None:
        cell = 2.0 * float(density)
    reg = None
    if register is not None:
        reg = CR.register(ops, pred, gt, init=transform, crop=crop, **register)
        transform = np.array(reg["transformation"])
    if transform is not None:
        transform = np.array(transform, np.float64).reshape(4, 4)
        pred = CR.apply_transform(pred, transform)
    valid_p = roi_volume_mask(pred, roi) if roi is not None else None
    valid_g = roi_plane_mask(gt, roi) if roi is not None else None
    if crop is not None:
        cp, cg = CR.crop_mask(ops, pred, crop), CR.crop_mask(ops, gt, crop)
        valid_p = cp if valid_p is None else valid_p * cp
        valid_g = cg if valid_g is None else valid_g * cg
    d_pred = nn_distance(ops, pred, gt, max_dist, cell=cell)
    d_gt = nn_distance(ops, gt, pred, max_dist, cell=cell)
    sp, sg = side_stats(ops, d_pred, valid_p, max_dist, thresholds), side_stats(ops, d_gt, valid_g, max_dist, thresholds)
    precision = [b / sp["valid"] if sp["valid"] else 0.0 for b in sp["below"]]
    recall = [b / sg["valid"] if sg["valid"] else 0.0 for b in sg["below"]]
    res = {"accuracy": sp["mean"], "completeness": sg["mean"], "overall": None if None in (sp["mean"], sg["mean"]) else 0.5 * (sp["mean"] + sg["mean"]), "max_dist": float(max_dist),
           "thresholds": thresholds, "precision": precision, "recall": recall,
           "fscore": [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(precision, recall)],
           "density": density, "pred_points_read": n_pred_in, "pred": sp, "gt": sg}
    if transform is not None:
        res["transformation"] = transform.tolist()
    if reg is not None:
        res["registration"] = reg
    if return_distances:
        res["_distances"] = (pred, d_pred, gt, d_gt, kept)
    return res


def error_colours(dist: torch.Tensor, max_dist: float) -> np.ndarray:
    """clamped distance -> uint8 RGB [N,3]: blue (0) over green to red (max_dist)"""
    t = (dist.double() / float(max_dist)).clamp(0, 1).cpu().numpy()
    rgb = np.stack([np.clip(2 * t - 1, 0, 1), np.clip(1 - np.abs(2 * t - 1), 0, 1), np.clip(1 - 2 * t, 0, 1)], -1)
    return (rgb * 255 + 0.5).astype(np.uint8)


def evaluate_files(ops: Ops, pred_ply: str, gt_ply: str, max_dist: float, thresholds, density=None, roi=None, error_ply=None, transform=None, crop=None,
                   register=None) -> dict:
    pred, gt = IO.read_ply(pred_ply)[0], IO.read_ply(gt_ply)[0]
    res = evaluate(ops, pred, gt, max_dist, thresholds, density=density, roi=roi, return_distances=error_ply is not None, transform=transform, crop=crop,
                   register=register)
    if error_ply is not None:
        p, d = res.pop("_distances")[:2]
        IO.write_ply(error_ply, p.cpu().numpy(), error_colours(d, max_dist))
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pred", required=True, help="the cloud to score (PLY)")
    ap.add_argument("--gt", required=True, help="the ground-truth cloud (PLY)")
    ap.add_argument("--max_dist", type=float, required=True, help="distances are clamped here; points at the clamp count as outliers (DTU: 20)")
    ap.add_argument("--density", type=float, default=None, help="thin the prediction to one point per voxel of this side first (DTU: 0.2)")
    ap.add_argument("--thresholds", type=float, nargs="*", default=[], help="F-score thresholds (at most %d)" % _lib.CLOUD_MAX_THRESHOLDS)
    ap.add_argument("--dtu_obs_mask", default=None, help="DTU ObsMask<scan>_10.mat (needs scipy)")
    ap.add_argument("--dtu_plane", default=None, help="DTU Plane<scan>.mat (needs scipy)")
    ap.add_argument("--roi", default=None, help="an ROI saved with numpy.savez(mask=, origin=, resolution=[, plane=])")
    ap.add_argument("--error_ply", default=None, help="write the (thinned) prediction coloured by its clamped distance")
    ap.add_argument("--transform", default=None, help="4x4 text file: moves the prediction into the ground truth's frame first")
    ap.add_argument("--crop", default=None, help="crop volume .json (Tanks&Temples): points outside it are left out of the scores")
    ap.add_argument("--register", type=float, default=None, metavar="MAX_CORR", help="refine the transform by ICP with this correspondence distance first")
    ap.add_argument("--register_voxel", type=float, default=None, help="--register: thin both clouds to this voxel size for the ICP")
    ap.add_argument("--register_max_iter", type=int, default=30)
    ap.add_argument("--register_with_scale", action="store_true", help="--register: estimate a scale as well")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if a.roi and (a.dtu_obs_mask or a.dtu_plane):
        raise SystemExit("--roi and --dtu_obs_mask / --dtu_plane are alternatives")
    if a.dtu_plane and not a.dtu_obs_mask:
        raise SystemExit("--dtu_plane needs --dtu_obs_mask")
    roi = load_roi(a.roi) if a.roi else (load_dtu_roi(a.dtu_obs_mask, a.dtu_plane) if a.dtu_obs_mask else None)
    extra = {}
    if a.transform or a.crop or a.register is not None:
        extra = {"transform": CR.load_transform(a.transform) if a.transform else None, "crop": CR.load_crop_json(a.crop) if a.crop else None,
                 "register": None if a.register is None else {"schedule": [(a.register_voxel, a.register, a.register_max_iter)], "with_scale": a.register_with_scale}}
    res = evaluate_files(Ops.for_device(a.device), a.pred, a.gt, a.max_dist, a.thresholds, density=a.density, roi=roi, error_ply=a.error_ply, **extra)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
