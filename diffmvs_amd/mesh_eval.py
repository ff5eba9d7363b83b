"""Scores of a triangle mesh against a ground-truth cloud: the surface is sampled evenly by area on the MI355X
(dmvs_mesh_face_tally_i64, dmvs_mesh_sample_f32 of include/dmvs.h, csrc/mesh_clean.hip) and the samples are scored as a cloud
(diffmvs_amd.cloud_eval: accuracy, completeness, F-score).

    python -m diffmvs_amd.mesh_eval --mesh m.ply --gt gt.ply --spacing S --max_dist D [--thresholds ..] [--transform T.txt]
        [--crop c.json] [--min_faces N] [--samples_ply out.ply]

A mesh's vertices cannot stand in for its surface -- surface nets put one per cell, not one per unit of area.  Here every `spacing`^2 of
area gets one sample (systematic sampling along the faces' running area sum, the R2 sequence inside a face): integers and fp64 in a fixed
order, so the same mesh gives the same samples bit for bit.  The distances are point to sample, not point to triangle: `spacing` is
part of the score's definition."""
from __future__ import annotations

import argparse
import json
import math

import numpy as np
import torch

from . import _lib
from . import cloud_eval as CE
from . import cloud_register as CR
from . import formats as IO
from . import mesh_clean as MC
from .ops import Ops


def _sample(ops: Ops, verts, faces, spacing: float, blocks: int = 0):
    verts, faces = MC._mesh(ops, verts, faces)
    if not (spacing > 0 and math.isfinite(spacing)):
        raise ValueError(f"spacing must be positive and finite, got {spacing}")
    N, F = int(verts.shape[0]), int(faces.shape[0])
    scale, cap = MC.area_scale(verts, F)
    # (every face goes to root 0: only area_q is wanted here)
    area_q = ops.mesh_face_tally(verts, faces, torch.zeros(N, dtype=torch.int32, device=ops.device), scale, cap, blocks=blocks)[0]
    area_cum = torch.cumsum(area_q, 0)
    total = int(area_cum[-1]) if F else 0
    a0 = max(1, int(np.rint(float(spacing) ** 2 * scale)))
    M = total // a0
    if M > 2 ** 31 - 1:
        raise _lib.DmvsError(f"sample_surface: a spacing of {spacing:.6g} asks for {M} samples, more than 2^31 - 1; "
                             f"a spacing of {float(spacing) * math.sqrt(M / (2.0 ** 31 - 1)) * 1.001:.6g} would fit")
    if M == 0:
        points, face_of = torch.zeros((0, 3), dtype=torch.float32, device=ops.device), torch.zeros((0,), dtype=torch.int32, device=ops.device)
    else:
        points, face_of = ops.mesh_sample(verts, faces, area_cum, a0, M, blocks=blocks)
    return points, face_of, {"a0": a0, "scale": scale, "area_fixed": total, "area": total / scale, "area_q": area_q}


def sample_surface(ops: Ops, verts, faces, spacing: float, blocks: int = 0):
    """One point per spacing^2 of surface: a0 = max(1, rint(spacing^2 scale)) units of the faces' scaled areas (mesh_clean.area_scale),
    M = total // a0 samples.  -> (points [M,3] fp32, face_of [M] int32: the face each lies in)"""
    return _sample(ops, verts, faces, spacing, blocks=blocks)[:2]


def evaluate_mesh(ops: Ops, verts, faces, gt, spacing: float, max_dist: float, thresholds, min_faces: int = 0, return_samples: bool = False, **kw) -> dict:
    """cloud_eval.evaluate of sample_surface's points against the cloud gt (its keyword arguments transform, crop, roi, cell pass through;
    `density` is not applied: the samples are even already), plus "samples", "spacing" and "area" (and "cleaned" with min_faces > 0:
    components with fewer faces are dropped first, mesh_clean.clean)"""
    if "density" in kw:
        raise TypeError("evaluate_mesh: the samples are spread evenly already; `density` is not applied")
    info = None
    if int(min_faces) > 0:
        verts, _, faces, info = MC.clean(ops, verts, None, faces, min_faces=int(min_faces))
    points, _, s = _sample(ops, verts, faces, spacing)
    res = CE.evaluate(ops, points, gt, max_dist, thresholds, **kw)
    res.update({"samples": int(points.shape[0]), "spacing": float(spacing), "area": s["area"]})
    if info is not None:
        res["cleaned"] = info
    if return_samples:
        res["_samples"] = points
    return res


def evaluate_files(ops: Ops, mesh_ply: str, gt_ply: str, spacing, max_dist, thresholds, samples_ply=None, **kw) -> dict:
    verts, _, faces = IO.read_ply_mesh(mesh_ply)
    res = evaluate_mesh(ops, verts, faces, IO.read_ply(gt_ply)[0], spacing, max_dist, thresholds, return_samples=samples_ply is not None, **kw)
    if samples_ply is not None:
        p = res.pop("_samples").cpu().numpy()
        IO.write_ply(samples_ply, p, np.full((len(p), 3), 255, np.uint8))
    return res


def main(argv=None, device="cuda:0", ops=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="the triangle mesh to score (binary PLY)")
    ap.add_argument("--gt", required=True, help="the ground-truth cloud (PLY)")
    ap.add_argument("--spacing", type=float, required=True, help="one sample per spacing^2 of surface area")
    ap.add_argument("--max_dist", type=float, required=True, help="distances are clamped here; points at the clamp count as outliers")
    ap.add_argument("--thresholds", type=float, nargs="*", default=[], help="F-score thresholds (at most %d)" % _lib.CLOUD_MAX_THRESHOLDS)
    ap.add_argument("--transform", default=None, help="4x4 text file: moves the samples into the ground truth's frame first")
    ap.add_argument("--crop", default=None, help="crop volume .json (Tanks&Temples): points outside it are left out of the scores")
    ap.add_argument("--min_faces", type=int, default=0, help="drop components with fewer faces before sampling")
    ap.add_argument("--samples_ply", default=None, help="write the samples (in the mesh's frame)")
    a = ap.parse_args(argv)
    extra = {}
    if a.transform or a.crop:
        extra = {"transform": CR.load_transform(a.transform) if a.transform else None, "crop": CR.load_crop_json(a.crop) if a.crop else None}
    res = evaluate_files(ops or Ops.for_device(device), a.mesh, a.gt, a.spacing, a.max_dist, a.thresholds, samples_ply=a.samples_ply,
                         min_faces=a.min_faces, **extra)
    print(json.dumps({"mesh_eval": res}), flush=True)
    return res


if __name__ == "__main__":
    main()
