"""Rigid / similarity registration (point-to-point ICP) and polygon-prism cropping of point clouds on the GPU: what has to happen before
diffmvs_amd.cloud_eval's scores mean anything when the clouds do not already share a frame and a region of interest.

    python -m diffmvs_amd.cloud_register --pred a.ply --gt b.ply [--init T.txt] [--crop crop.json] [--with_scale]
        (--max_corr D [--voxel V] | --schedule tanks --dtau D) --out_transform T.txt [--out_ply aligned.ply]

One ICP iteration is one dmvs_cloud_nn_index_f32 launch (the grid walk of the scorer, returning which target is nearest, with the
current transform applied to the source inside the kernel), one dmvs_cloud_pair_moments_f64 launch (20 fixed-point sums), 20 integers
to the host, the closed form (`kabsch`) and a 4x4 product.  The moved cloud is never materialised.  csrc/cloud_register.hip.

The stopping rule is that of Open3D's registration_icp restated from its published source (evaluate, then repeat { update, evaluate }
until both |fitness - previous| < rel_fitness and |inlier_rmse - previous| < rel_rmse, or max_iter updates); no Open3D is available
to pin it against.  The Tanks&Temples / Open3D tools remain the authority for published numbers."""
from __future__ import annotations

import argparse
import json
import math
from fractions import Fraction

import numpy as np
import torch

from . import _lib
from . import cloud_grid as G
from . import formats as IO
from .ops import Ops

AXES = {"X": 0, "Y": 1, "Z": 2}
_UV = {0: (1, 2), 1: (0, 2), 2: (0, 1)}      # the polygon's plane per orthogonal axis: (u, v, w) = (1,2,0) / (0,2,1) / (0,1,2)


# ------------------------------------------------------------------------------------------ closed forms
def _closed_form(n, mean_p, mean_t, cov_tp, var_p, with_scale, noise=0.0):
    """Umeyama (1991): the similarity x -> c R x + t minimising sum |c R p + t - q|^2, from the centroids, the cross-covariance
    cov_tp = mean (t - mean_t)(p - mean_p)^T and the variance of p.  noise: what the entries of cov_tp may be off by (the fixed point's
    resolution); a second singular value below it is not evidence of a second dimension.  -> (c, R, t)"""
    if n < 3:
        raise ValueError(f"registration needs at least 3 pairs, got {n}")
    if not (np.isfinite(cov_tp).all() and np.isfinite(mean_p).all() and np.isfinite(mean_t).all() and math.isfinite(var_p)):
        raise ValueError("registration: the pair statistics are not finite")
    U, D, Vt = np.linalg.svd(cov_tp)
    if not (D[0] > 0 and D[1] > max(1e-12 * D[0], 4.0 * noise) and var_p > 0):
        raise ValueError("registration: degenerate pairs (the cross-covariance has rank < 2: coincident or collinear points); "
                         "the rotation is not determined")
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:      # the best orthogonal matrix is a reflection: flip the weakest axis
        S[2] = -1.0
    R = (U * S) @ Vt
    c = float((D * S).sum() / var_p) if with_scale else 1.0
    return c, R, mean_t - c * (R @ mean_p)


def _matrix(c, R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = c * R, t
    return T


def kabsch(moments, scale, centres, with_scale: bool = False) -> np.ndarray:
    """the 4x4 float64 update of one ICP step from the sums of dmvs_cloud_pair_moments_f64.

    moments: the 20 (or the first 19) integers; scale: (scale_linear, scale_quadratic); centres: (center_p, center_q).  The
    covariance about the centroids is formed EXACTLY from the integers (rationals: n * sum p t^T - sum p sum t^T), so the centring
    costs no cancellation; SVD of the 3x3 cross-covariance, reflection guard, Umeyama's scale when with_scale.  Fewer than 3 pairs or a
    cross-covariance of rank < 2 (collinear points) raise ValueError: the result is never NaN.  (A planar configuration is fine.)"""
    m = [int(v) for v in moments]
    if len(m) < 19:
        raise ValueError("kabsch: expected the 19 sums of dmvs_cloud_pair_moments_f64")
    s1, s2 = (Fraction(float(s)) for s in scale)
    cp, cq = (np.asarray(c, np.float64).reshape(3) for c in centres)
    n = m[0]
    if n < 3:
        raise ValueError(f"registration needs at least 3 pairs, got {n}")
    sp, st = [Fraction(v) / s1 for v in m[1:4]], [Fraction(v) / s1 for v in m[4:7]]
    cov_pt = np.array([[float((Fraction(m[7 + 3 * a + b]) / s2 * n - sp[a] * st[b]) / (n * n)) for b in range(3)] for a in range(3)])
    var_p = float((Fraction(m[16]) / s2 * n - sum(v * v for v in sp)) / (n * n))
    mean_p, mean_t = np.array([float(v / n) for v in sp]), np.array([float(v / n) for v in st])
    # a mean of rounded terms is within 0.5 / scale of the exact mean; cov = mean(p t) - mean(p) mean(t), 3x3 entries
    noise = 3.0 * (0.5 / float(s2) + (np.abs(mean_p).max() + np.abs(mean_t).max()) * 0.5 / float(s1))
    c, R, t = _closed_form(n, mean_p + cp, mean_t + cq, cov_pt.T, var_p, with_scale, noise=noise)
    return _matrix(c, R, t)


def umeyama(points_a, points_b, with_scale: bool = True) -> np.ndarray:
    """host, fp64: the 4x4 similarity (rigid with with_scale=False) that best maps points_a [K,3] onto the corresponding points_b
    [K,3] -- an initial guess from corresponding camera centres (cams/*_cam.txt against a ground-truth trajectory .log)"""
    a, b = np.asarray(points_a, np.float64), np.asarray(points_b, np.float64)
    if a.ndim != 2 or a.shape[1] != 3 or a.shape != b.shape:
        raise ValueError(f"umeyama: two [K,3] arrays of corresponding points, got {a.shape} and {b.shape}")
    if len(a) < 3:
        raise ValueError(f"registration needs at least 3 pairs, got {len(a)}")
    ma, mb = a.mean(0), b.mean(0)
    da, db = a - ma, b - mb
    return _matrix(*_closed_form(len(a), ma, mb, db.T @ da / len(a), float((da * da).sum() / len(a)), with_scale))


def apply_transform(points: torch.Tensor, transform) -> torch.Tensor:
    """[N,3] fp32 -> fp32(((m0 x + m1 y) + m2 z) + m3) per row in fp64: the arithmetic of the kernels' `transform` argument, bit for bit"""
    m = np.asarray(transform, np.float64)
    p = points.double()
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    rows = [((float(m[r, 0]) * x + float(m[r, 1]) * y) + float(m[r, 2]) * z) + float(m[r, 3]) for r in range(3)]
    return torch.stack(rows, 1).float().contiguous()


# ------------------------------------------------------------------------------------------ ICP
def moment_scales(n: int, bound: float, max_corr: float):
    """the largest powers of two the entry point accepts: n bound s1 < 2^62 and n max(3 bound^2, (1.001 max_corr)^2) s2 < 2^62"""
    return G.pow2_scale_below(bound, n), G.pow2_scale_below(max(3.0 * bound * bound, (1.001 * float(np.float32(max_corr))) ** 2), n)


def icp(ops: Ops, source, target, init=None, max_corr: float = None, max_iter: int = 30, rel_fitness: float = 1e-6, rel_rmse: float = 1e-6,
        with_scale: bool = False, valid=None, cell: float | None = None, grid: dict | None = None) -> dict:
    """point-to-point ICP of `source` [N,3] onto `target` [M,3] from the 4x4 `init` (identity by default).

    -> {transformation (4x4 float64 nested list: source -> target frame), fitness (pairs / source points), inlier_rmse
    (sqrt(sum d^2 / pairs)), pairs, iterations (updates applied), converged, history: [{fitness, inlier_rmse, pairs}] (entry 0 = the
    initial transform)}.  A pair is a source point whose nearest target lies within max_corr.  valid: optional uint8 [N], points with
    0 take no part (and do not count as source points).  The target grid is built once (or passed in: cloud_grid.build_grid), the
    source is sorted by the grid key of its initially transformed position once.  Raises ValueError when an update is undetermined
    (fewer than 3 pairs, collinear pairs)."""
    if max_corr is None or not (max_corr > 0 and math.isfinite(max_corr)):
        raise ValueError(f"max_corr must be positive and finite, got {max_corr}")
    src, tgt = G.to_cloud(ops, source), G.to_cloud(ops, target)
    if src.shape[0] == 0 or tgt.shape[0] == 0:
        raise ValueError("icp: both clouds must hold points")
    T = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
    if valid is not None:
        valid = torch.as_tensor(valid).to(device=ops.device, dtype=torch.uint8).contiguous()
    if grid is None:
        if cell is None:
            cell = min(float(max_corr), max(2.0 * G.estimate_spacing(tgt, max_corr / G.FAR_RINGS), float(max_corr) / G.FAR_RINGS))
        grid = G.build_grid(tgt, float(cell))
    order = G.order_by_grid(apply_transform(src, T), grid)
    if order is not None:
        src = src[order].contiguous()
        valid = None if valid is None else valid[order].contiguous()
    n_src = int(src.shape[0]) if valid is None else int((valid != 0).sum())
    gt_sorted = grid["target"]
    lo, hi = gt_sorted.min(0).values.double().cpu().numpy(), gt_sorted.max(0).values.double().cpu().numpy()
    centre = 0.5 * (lo + hi)
    # a counted pair is within max_corr of its target, so both members stay inside the target's box grown by max_corr
    bound = (float((hi - lo).max()) * 0.5 + float(max_corr)) * 1.0001 + 1e-30
    scales = moment_scales(int(src.shape[0]), bound, max_corr)

    def evaluate(Tm):
        index = ops.cloud_nn_index(src, gt_sorted, grid["keys"], grid["start"], grid["origin"], grid["cell"], grid["dims"], max_corr, transform=Tm, dist=False)[1]
        mom = ops.cloud_pair_moments(src, Tm, gt_sorted, index, valid, max_corr, centre, centre, bound, scales[0], scales[1])
        m = [int(v) for v in mom.cpu()]
        if m[19]:
            raise RuntimeError(f"icp: {m[19]} pairs left the fixed-point bound {bound}")
        n = m[0]
        return m, {"fitness": n / n_src if n_src else 0.0, "inlier_rmse": math.sqrt(max(0.0, m[18] / scales[1]) / n) if n else 0.0, "pairs": n}

    m, cur = evaluate(T)
    history, converged, it = [cur], False, 0
    while it < max_iter:
        T = kabsch(m, scales, (centre, centre), with_scale=with_scale) @ T
        it += 1
        prev = cur
        m, cur = evaluate(T)
        history.append(cur)
        if abs(prev["fitness"] - cur["fitness"]) < rel_fitness and abs(prev["inlier_rmse"] - cur["inlier_rmse"]) < rel_rmse:
            converged = True
            break
    return {"transformation": T.tolist(), "fitness": cur["fitness"], "inlier_rmse": cur["inlier_rmse"], "pairs": cur["pairs"], "iterations": it,
            "converged": converged, "history": history, "source_points": n_src, "max_corr": float(max_corr), "with_scale": bool(with_scale)}


# ------------------------------------------------------------------------------------------ crop volume, files
def make_crop(axis, axis_min: float, axis_max: float, polygon) -> dict:
    """axis: 'X' / 'Y' / 'Z' (or 0 / 1 / 2); polygon: [K,2] (u, v) vertices in the plane of the other two axes, or [K,3] points"""
    ax = AXES[axis.upper()] if isinstance(axis, str) else int(axis)
    if ax not in (0, 1, 2):
        raise ValueError(f"the orthogonal axis is X, Y or Z, got {axis!r}")
    poly = np.asarray(polygon, np.float64)
    if poly.ndim == 2 and poly.shape[1] == 3:
        poly = poly[:, list(_UV[ax])]
    if poly.ndim != 2 or poly.shape[1] != 2 or not 3 <= len(poly) <= _lib.CLOUD_MAX_POLYGON:
        raise ValueError(f"a crop polygon has 3..{_lib.CLOUD_MAX_POLYGON} vertices, got an array of shape {poly.shape}")
    if not (np.isfinite(poly).all() and axis_min <= axis_max):
        raise ValueError("the crop volume needs finite vertices and axis_min <= axis_max")
    return {"axis": ax, "axis_min": float(axis_min), "axis_max": float(axis_max), "polygon": np.ascontiguousarray(poly)}


def load_crop_json(path: str) -> dict:
    """the crop file of a Tanks&Temples scene (Open3D's SelectionPolygonVolume): orthogonal_axis, axis_min, axis_max, bounding_polygon"""
    with open(path) as f:
        j = json.load(f)
    return make_crop(j["orthogonal_axis"], j["axis_min"], j["axis_max"], j["bounding_polygon"])


def crop_mask(ops: Ops, points, volume: dict, transform=None) -> torch.Tensor:
    """uint8 [N]: 1 where the point (moved by the 4x4 `transform` first, if given) lies inside the volume (dmvs_cloud_crop_prism_f32)"""
    pts = G.to_cloud(ops, points)
    poly = torch.from_numpy(volume["polygon"]).to(ops.device).contiguous()
    return ops.cloud_crop_prism(pts, poly, volume["axis"], volume["axis_min"], volume["axis_max"], transform=transform)


def load_transform(path: str) -> np.ndarray:
    """a 4x4 matrix as whitespace-separated text (the alignment file of a Tanks&Temples scene)"""
    v = np.loadtxt(path, dtype=np.float64).reshape(-1)
    if v.size != 16 or not np.isfinite(v).all():
        raise ValueError(f"{path}: expected 16 finite numbers (a 4x4 matrix), got {v.size}")
    return v.reshape(4, 4)


def save_transform(path: str, transform) -> None:
    with open(path, "w") as f:
        for row in np.asarray(transform, np.float64).reshape(4, 4):
            f.write(" ".join(repr(float(v)) for v in row) + "\n")


def load_trajectory_log(path: str):
    """a camera trajectory .log: blocks of an index line (integers) and a 4x4 camera-to-world matrix.  -> [(indices, 4x4)]"""
    with open(path) as f:
        rows = [ln.split() for ln in f if ln.strip()]
    if len(rows) % 5:
        raise ValueError(f"{path}: a trajectory log is blocks of 5 lines, got {len(rows)} lines")
    out = []
    for k in range(0, len(rows), 5):
        mat = np.array([[float(v) for v in r] for r in rows[k + 1:k + 5]], np.float64)
        if mat.shape != (4, 4):
            raise ValueError(f"{path}: block {k // 5} does not hold a 4x4 matrix")
        out.append(([int(v) for v in rows[k]], mat))
    return out


# ------------------------------------------------------------------------------------------ coarse to fine
def tanks_schedule(dtau: float):
    """the three refinement stages of the Tanks&Temples evaluation toolbox, as (voxel, max_corr, max_iter)"""
    return [(float(dtau), 80.0 * dtau, 20), (0.5 * dtau, 20.0 * dtau, 20), (None, 2.0 * dtau, 20)]


def register(ops: Ops, pred, gt, init=None, schedule=None, crop: dict | None = None, with_scale: bool = False, rel_fitness: float = 1e-6,
             rel_rmse: float = 1e-6) -> dict:
    """coarse-to-fine ICP: `schedule` is a list of stages (voxel, max_corr, max_iter); each stage thins both clouds with
    cloud_grid.voxel_downsample(voxel) (voxel None: not at all), keeps only the prediction points that its starting transform puts
    inside `crop` (if given) and runs `icp` from the previous stage's result.  -> the last stage's dict plus "stages".

    tanks_schedule(dtau) fills in the Tanks&Temples toolbox's stages (voxel dtau / corr 80 dtau, voxel dtau / 2 / corr 20 dtau, no
    voxel / corr 2 dtau; 20 iterations each) as restated from its published source; every number is an argument.  Known deviations:
    (1) the thinning keeps the first point of every voxel, the toolbox (Open3D voxel_down_sample) the centroid of its points;
    (2) the stopping rule is this module's restatement (see the module docstring), not a pinned Open3D build;
    (3) the toolbox's last stage thins by taking every k-th point down to a maximum size, this one uses all points."""
    if not schedule:
        raise ValueError("register: an empty schedule")
    pred, gt = G.to_cloud(ops, pred), G.to_cloud(ops, gt)
    T = np.eye(4) if init is None else np.array(init, np.float64).reshape(4, 4)
    stages, res = [], None
    for voxel, max_corr, max_iter in schedule:
        s = pred if voxel is None else G.voxel_downsample(pred, voxel)[0].contiguous()
        t = gt if voxel is None else G.voxel_downsample(gt, voxel)[0].contiguous()
        if crop is not None:
            s = s[crop_mask(ops, s, crop, transform=T).bool()].contiguous()
        res = icp(ops, s, t, init=T, max_corr=max_corr, max_iter=int(max_iter), rel_fitness=rel_fitness, rel_rmse=rel_rmse, with_scale=with_scale)
        T = np.array(res["transformation"])
        stages.append({"voxel": voxel, "max_corr": float(max_corr), "max_iter": int(max_iter), "source_points": int(s.shape[0]), "target_points": int(t.shape[0]),
                       "fitness": res["fitness"], "inlier_rmse": res["inlier_rmse"], "iterations": res["iterations"], "converged": res["converged"]})
    out = {k: v for k, v in res.items() if k != "history"}
    out["stages"] = stages
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pred", required=True, help="the cloud to move (PLY)")
    ap.add_argument("--gt", required=True, help="the cloud to register it to (PLY)")
    ap.add_argument("--init", default=None, help="initial 4x4 transform (text); default: identity")
    ap.add_argument("--crop", default=None, help="crop volume .json: only prediction points inside it take part")
    ap.add_argument("--with_scale", action="store_true", help="estimate a similarity (rotation, translation AND scale)")
    ap.add_argument("--max_corr", type=float, default=None, help="one stage: pairs farther apart than this are ignored")
    ap.add_argument("--voxel", type=float, default=None, help="with --max_corr: thin both clouds to one point per voxel of this side first")
    ap.add_argument("--max_iter", type=int, default=30)
    ap.add_argument("--schedule", choices=["tanks"], default=None, help="tanks: the three stages of the Tanks&Temples toolbox (needs --dtau)")
    ap.add_argument("--dtau", type=float, default=None, help="the scene's distance threshold")
    ap.add_argument("--out_transform", required=True, help="where the 4x4 result is written (text)")
    ap.add_argument("--out_ply", default=None, help="write the moved prediction")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if (a.max_corr is None) == (a.schedule is None):
        raise SystemExit("give either --max_corr D [--voxel V] or --schedule tanks --dtau D")
    if a.schedule and a.dtau is None:
        raise SystemExit("--schedule tanks needs --dtau")
    ops = Ops.for_device(a.device)
    pred, colour = IO.read_ply(a.pred)
    gt = IO.read_ply(a.gt)[0]
    schedule = tanks_schedule(a.dtau) if a.schedule else [(a.voxel, a.max_corr, a.max_iter)]
    res = register(ops, pred, gt, init=load_transform(a.init) if a.init else None, schedule=schedule,
                   crop=load_crop_json(a.crop) if a.crop else None, with_scale=a.with_scale)
    save_transform(a.out_transform, res["transformation"])
    if a.out_ply:
        moved = apply_transform(G.to_cloud(ops, pred), res["transformation"]).cpu().numpy()
        IO.write_ply(a.out_ply, moved, colour if colour is not None else np.zeros((len(moved), 3), np.uint8))
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
