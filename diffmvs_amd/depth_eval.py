"""Depth-map scoring: an estimated depth map against a ground-truth depth map, on the GPU, as integers.

    python -m diffmvs_amd.depth_eval --outdir <eval output> --gtpath <tree> [--testlist scans.txt] [--thresholds 2 4 8] [--dataset dtu]

scores every <outdir>/<scan>/depth_est/%08d.pfm that has a <gtpath>/<scan>/depth_gt/%08d.pfm (the layout train_driver.TreeTrainSet reads;
an optional mask/%08d.png is honoured) and prints one JSON object: the metrics per scene, overall, and the counters.

The figures are the reference's `AbsDepthError_metrics` (utils.py:150-187: mean |est - gt| over the mask, per image), BASELINE.json's
"DTU abs-rel" (mean |est - gt| / gt), the RMSE and the share of pixels with |est - gt| below each threshold.  They are computed from the
integer rows of dmvs_depth_stats_f32 (include/dmvs.h): counts and FIXED-POINT sums, llrint(term * 2^k) per pixel with the per-pixel
arithmetic in fp64.  Integer sums do not depend on the order of summation, so a metric is the same number whatever the grid, the batch size
or the number of ranks that computed it -- the convention of dmvs_cloud_stats_f32 and the GroupNorm statistics.  A term is rounded by at
most 2^-(k+1); k comes from cloud_grid.pow2_scale_below(big, H * W), the largest that cannot overflow (k = 31 for a DTU-sized map with
big = 935).  Nothing is hidden by the kernel's clamps and exclusions: pixels left out (non-finite estimate or ground truth, gt <= 0) and
terms clamped at `big` are counted in the rows, carried into every summary, and printed by every tool when they are not zero.

formats.abs_depth_error / formats.abs_rel_error stay what they are (small fp32 torch helpers): the tests hold this module against them."""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from . import formats as IO
from .cloud_grid import pow2_scale_below

SLOTS = _lib.DEPTH_SLOTS
HEAD = 2                      # a scored row = [k, k_sq, the DEPTH_SLOTS + T integers of the kernel]: 2^k and 2^k_sq are the scales of its sums
MASKED, SCORED, LEFT_OUT, SATURATED, SUM_ABS, SUM_REL, SUM_SQ = range(HEAD, HEAD + SLOTS)


def scale_exponents(big: float, pixels: int):
    """(k, k_sq): the sums of |e| and |e| / gt are in units of 2^-k, the sum of e^2 in units of 2^-k_sq.  2^k = pow2_scale_below(big, pixels);
    2^k_sq = 2^k / p with p the smallest power of two >= big -- the rule of dmvs_depth_stats_f32, so that big^2 * 2^k_sq <= big * 2^k"""
    k = int(math.log2(pow2_scale_below(big, pixels)))
    mant, ex = math.frexp(float(big))
    return k, k - (ex - 1 if mant == 0.5 else ex)


def score(ops, est, gt, mask=None, thresholds: Sequence[float] = (2, 4, 8), band=None, big=None, blocks: int = 0) -> torch.Tensor:
    """est, gt [B,H,W] (mask: None or [B,H,W], in where > 0.5) -> int64 [B, 2 + 7 + T] ON THE DEVICE, one row per item: the two scale
    exponents (scale_exponents) and the integers of Ops.depth_stats.  Nothing is read back here; summarise() reads the rows once.
    big: the clamp of a term and the bound the scale is chosen for -- a number, or one per item (the sample's depth_max); None = the largest
    finite ground-truth depth of the batch (one readback).  band = (lo, hi): only pixels with lo <= |e| <= hi are scored, the `thres` of
    AbsDepthError_metrics."""
    dev = ops.device
    est, gt, mask = (None if t is None else torch.as_tensor(t).to(device=dev, dtype=torch.float32).contiguous() for t in (est, gt, mask))
    T = len(thresholds)
    if est.dim() != 3:
        raise _lib.DmvsError(f"depth_eval.score: depth maps are [B,H,W], got {tuple(est.shape)}")
    B, HW = int(est.shape[0]), int(est.shape[1] * est.shape[2])
    if big is None:
        finite = gt[torch.isfinite(gt)] if gt.numel() else gt
        big = float(finite.max()) if finite.numel() and float(finite.max()) > 0 else 1.0
    bigs = [float(b) for b in (big.reshape(-1).tolist() if torch.is_tensor(big) else (list(big) if isinstance(big, (list, tuple, np.ndarray)) else [big] * B))]
    if len(bigs) != B:
        raise _lib.DmvsError(f"depth_eval.score: {len(bigs)} clamps for {B} items")
    out = torch.empty(B, HEAD + SLOTS + T, dtype=torch.int64, device=dev)
    if B == 0:
        ops.depth_stats(est, gt, mask, thresholds, 1.0, 1.0, band=band, blocks=blocks)      # (argument checks only: nothing is launched)
    b0 = 0
    while b0 < B:                                         # one launch per run of items that share a clamp: one launch for a batch of one dataset
        b1 = b0 + 1
        while b1 < B and bigs[b1] == bigs[b0]:
            b1 += 1
        k, k_sq = scale_exponents(bigs[b0], HW)
        out[b0:b1, HEAD:] = ops.depth_stats(est[b0:b1], gt[b0:b1], None if mask is None else mask[b0:b1], thresholds, bigs[b0], 2.0 ** k,
                                            band=band, blocks=blocks)
        out[b0:b1, 0], out[b0:b1, 1] = k, k_sq
        b0 = b1
    return out


def _name(t) -> str:
    return "inlier_" + format(float(t), "g")


def summarise(rows, thresholds: Sequence[float] = (2, 4, 8)) -> dict:
    """rows: what score() returned (or several of them concatenated, in sample order; a tensor or nested lists of integers) -> a dict:
      abs_err, abs_rel, rmse, inlier_<t>  the mean over the items of the per-item mean: what the reference reports with its batch of 1;
      pooled: the same figures over all scored pixels at once;
      items, empty_items, masked, scored, left_out, saturated.
    An item without a scored pixel (an empty mask) is EXCLUDED from the per-item mean and counted in `empty_items`; the reference takes the
    mean of an empty tensor there and reports NaN.  With no scored pixel at all the figures are None.
    A pure function of the integers, taken in the order given: per item exact integer ratios rounded once to fp64, then a left-to-right
    fp64 sum over the items; the pooled figures are exact integer sums brought to one scale."""
    if torch.is_tensor(rows):
        rows = rows.detach().cpu().tolist()               # the one readback
    rows = [[int(v) for v in r] for r in rows]
    T = len(thresholds)
    names = ["abs_err", "abs_rel", "rmse"] + [_name(t) for t in thresholds]
    for r in rows:
        if len(r) != HEAD + SLOTS + T:
            raise ValueError(f"a row of {len(r)} integers does not belong to {T} thresholds")
    per_item = {n: 0.0 for n in names}
    live = [r for r in rows if r[SCORED] > 0]

    def ratio(num: int, den: int, k: int) -> float:       # num / (den * 2^k), exact integers, one rounding
        return num / (den << k) if k >= 0 else (num << -k) / den

    for r in live:
        n = r[SCORED]
        vals = [ratio(r[SUM_ABS], n, r[0]), ratio(r[SUM_REL], n, r[0]), math.sqrt(ratio(r[SUM_SQ], n, r[1]))] + \
               [r[HEAD + SLOTS + t] / n for t in range(T)]
        for name, v in zip(names, vals):
            per_item[name] += v
    out = {n: (per_item[n] / len(live) if live else None) for n in names}
    pooled = {n: None for n in names}
    if live:
        n = sum(r[SCORED] for r in live)
        k, k_sq = max(r[0] for r in live), max(r[1] for r in live)
        pooled["abs_err"] = ratio(sum(r[SUM_ABS] << (k - r[0]) for r in live), n, k)
        pooled["abs_rel"] = ratio(sum(r[SUM_REL] << (k - r[0]) for r in live), n, k)
        pooled["rmse"] = math.sqrt(ratio(sum(r[SUM_SQ] << (k_sq - r[1]) for r in live), n, k_sq))
        for t in range(T):
            pooled[_name(thresholds[t])] = sum(r[HEAD + SLOTS + t] for r in live) / n
    out["pooled"] = pooled
    out.update(items=len(rows), empty_items=len(rows) - len(live), masked=sum(r[MASKED] for r in rows), scored=sum(r[SCORED] for r in rows),
               left_out=sum(r[LEFT_OUT] for r in rows), saturated=sum(r[SATURATED] for r in rows))
    return out


def warn_hidden(summary: dict, what: str, file=None) -> None:
    """the line every tool prints when a summary holds pixels the kernel left out or terms it clamped"""
    if summary["left_out"] or summary["saturated"] or summary["empty_items"]:
        print(f"[depth_eval] {what}: {summary['left_out']} pixels left out (non-finite or gt <= 0), {summary['saturated']} terms clamped, "
              f"{summary['empty_items']} of {summary['items']} maps without a scored pixel", file=file or sys.stderr, flush=True)


# ------------------------------------------------------------------------------------------ trees
def _views(outdir: str, gtpath: str, scene: str):
    est_dir = os.path.join(outdir, scene, "depth_est")
    if not os.path.isdir(est_dir):
        return [], 0
    names = sorted(f for f in os.listdir(est_dir) if f.endswith(".pfm"))
    have = [n for n in names if os.path.exists(os.path.join(gtpath, scene, "depth_gt", n))]
    return have, len(names) - len(have)


def _load_view(outdir: str, gtpath: str, scene: str, name: str):
    """-> est [H,W], gt [H,W] (subsampled to the estimate's size if it is the image's), mask [H,W] fp32, big"""
    est = np.ascontiguousarray(IO.read_pfm(os.path.join(outdir, scene, "depth_est", name))[0]).astype(np.float32)
    gfile = os.path.join(gtpath, scene, "depth_gt", name)
    gt = np.ascontiguousarray(IO.read_pfm(gfile)[0]).astype(np.float32)
    mfile = os.path.join(gtpath, scene, "mask", name[:-4] + ".png")
    m = None
    if os.path.exists(mfile):
        from PIL import Image
        m = (np.array(Image.open(mfile).convert("L")) > 10).astype(np.float32)      # TreeTrainSet's rule
        if m.shape != gt.shape:
            raise ValueError(f"{mfile}: {m.shape} does not match the ground truth {gt.shape}")
    if gt.shape != est.shape:
        # ground truth at the image's size, estimate at a stage's: nearest-neighbour subsampling like TreeTrainSet (datasets/dtu.py:100-112)
        f = gt.shape[0] // max(1, est.shape[0])
        if f < 1 or gt[::f, ::f].shape != est.shape or gt.shape[0] % est.shape[0] or gt.shape[1] % est.shape[1]:
            raise ValueError(f"{gfile}: {gt.shape} is no whole multiple of the estimate {est.shape}")
        gt = np.ascontiguousarray(gt[::f, ::f])
        m = None if m is None else np.ascontiguousarray(m[::f, ::f])
    cam = os.path.join(outdir, scene, "cams", name[:-4] + "_cam.txt")
    lo = hi = None
    if os.path.exists(cam):                               # written by eval next to the estimate: "depth_max depth_min" on its last line
        with open(cam) as fh:
            last = [ln for ln in fh.read().splitlines() if ln.strip()][-1].split()
        hi, lo = float(last[0]), float(last[1])
    if m is None:
        m = ((gt > lo) & (gt < hi)) if lo is not None else (gt > 0)
        m = m.astype(np.float32)
    finite = gt[np.isfinite(gt)]
    big = hi if hi is not None and hi > 0 else (float(finite.max()) if finite.size and finite.max() > 0 else 1.0)
    return est, gt, m, big


def score_tree(ops, outdir: str, gtpath: str, scenes: Sequence[str] = ("",), thresholds: Sequence[float] = (2, 4, 8), band=None) -> dict:
    """the command line's work: {"thresholds", "scenes": {scene: summary}, "overall": summary, "counters": {...}}.  The rows of all views stay on
    the device until the end and are read back once."""
    per_scene, missing = [], 0
    for scene in scenes:
        names, no_gt = _views(outdir, gtpath, scene)
        missing += no_gt
        rows = []
        for name in names:
            est, gt, m, big = _load_view(outdir, gtpath, scene, name)
            t = lambda a: torch.from_numpy(a)[None].to(ops.device)  # noqa: E731
            rows.append(score(ops, t(est), t(gt), t(m), thresholds, band=band, big=big))
        per_scene.append((scene, rows))
    flat = [r for _, rows in per_scene for r in rows]
    host = torch.cat(flat).cpu().tolist() if flat else []
    out, at = {"thresholds": [float(t) for t in thresholds], "scenes": {}}, 0
    for scene, rows in per_scene:
        if rows:
            out["scenes"][scene] = summarise(host[at:at + len(rows)], thresholds)
            at += len(rows)
    out["overall"] = summarise(host, thresholds)
    out["counters"] = {"views": len(host), "views_without_ground_truth": missing,
                       **{k: out["overall"][k] for k in ("empty_items", "masked", "scored", "left_out", "saturated")}}
    return out


def main(argv=None, ops=None) -> dict:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--outdir", required=True, help="what diffmvs_amd.eval wrote: <outdir>/<scan>/depth_est/%%08d.pfm")
    ap.add_argument("--gtpath", required=True, help="tree with <scan>/depth_gt/%%08d.pfm (and optionally <scan>/mask/%%08d.png)")
    ap.add_argument("--testlist", default=None, help="file with one scene per line (default: the single scene '' of a general dataset)")
    ap.add_argument("--dataset", default="general", choices=["dtu", "tank", "eth3d", "general"],
                    help="general (default): one scene directly under --outdir / --gtpath, as eval writes it (--testlist is not read); "
                         "dtu / tank / eth3d: one directory per scene of --testlist under both")
    ap.add_argument("--thresholds", type=float, nargs="*", default=[2.0, 4.0, 8.0], help="absolute errors below which a pixel is an inlier")
    ap.add_argument("--band", type=float, nargs=2, default=None, help="score only pixels with lo <= |error| <= hi (utils.py AbsDepthError_metrics thres)")
    ap.add_argument("--device", default="cuda:0")
    a = ap.parse_args(argv)
    if ops is None:
        from .ops import Ops
        ops = Ops.for_device(a.device)
    scenes = [""]                                         # MVSDataset: a general dataset is the single scene ''
    if a.dataset != "general":
        if not a.testlist:
            raise SystemExit(f"depth_eval: --dataset {a.dataset} keeps one directory per scene: name them with --testlist")
        with open(a.testlist) as f:
            scenes = [ln.strip() for ln in f if ln.strip()]
    res = score_tree(ops, a.outdir, a.gtpath, scenes, a.thresholds, band=a.band)
    warn_hidden(res["overall"], a.outdir)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    main()
