"""Take the floaters out of an extracted mesh on the MI355X: connected components by pointer jumping, their face counts and areas,
and the removal of the small ones (dmvs_mesh_label_round_i32, dmvs_mesh_face_tally_i64 of include/dmvs.h, csrc/mesh_clean.hip).

    python -m diffmvs_amd.mesh_clean --mesh in.ply --out out.ply [--min_faces N] [--min_fraction F] [--keep_largest K]

Two vertices are connected when a face names both.  The labels are the smallest vertex index of each component and the sums are integers:
the same mesh gives the same result bit for bit, whatever the launch.  Surviving vertices and faces keep their order."""
from __future__ import annotations

import argparse
import json
import math

import numpy as np
import torch

from . import _lib
from . import formats as IO
from .cloud_grid import pow2_scale_below
from .ops import Ops

ROUNDS_PER_READ = 2      # components(): rounds issued per host read of their counters
MAX_ROUNDS = 4096


def _mesh(ops: Ops, verts, faces):
    v = None if verts is None else torch.as_tensor(np.ascontiguousarray(verts) if isinstance(verts, np.ndarray) else verts)
    f = torch.as_tensor(np.ascontiguousarray(faces) if isinstance(faces, np.ndarray) else faces)
    if f.dim() != 2 or f.shape[1] != 3 or f.dtype not in (torch.int32, torch.int64) or (v is not None and (v.dim() != 2 or v.shape[1] != 3)):
        raise _lib.DmvsError(f"a mesh is verts [N,3] and integer faces [F,3], got {None if v is None else tuple(v.shape)} and {f.dtype} {tuple(f.shape)}")
    if v is not None:
        v = v.to(device=ops.device, dtype=torch.float32).contiguous()
    return v, f.to(device=ops.device, dtype=torch.int32).contiguous()


def components(ops: Ops, faces, n_verts: int, blocks: int = 0, per_read: int = ROUNDS_PER_READ):
    """faces [F,3] int32, n_verts vertices -> (label [N] int32: the smallest vertex index of every vertex's component (itself for a vertex
    no face names), {"rounds": rounds run up to and including the first that wrote nothing, "bad_faces": faces with an index outside
    [0, N), which connect nothing}).  per_read rounds are issued per host read of their counters; the labels do not depend on it."""
    _, faces = _mesh(ops, None, faces)
    N, per_read = int(n_verts), max(1, int(per_read))
    if not 0 <= N <= 2 ** 31 - 1:
        raise _lib.DmvsError(f"components: {n_verts} vertices; 0 .. 2^31 - 1 are supported")
    label = torch.arange(N, dtype=torch.int32, device=ops.device)
    states = torch.empty((per_read, 2), dtype=torch.int32, device=ops.device)
    rounds = 0
    while True:
        for k in range(per_read):
            ops.mesh_label_round(faces, label, state=states[k], blocks=blocks)
        host = states.cpu().numpy()
        quiet = np.nonzero(host[:, 0] == 0)[0]
        if quiet.size:      # (after a round that wrote nothing, nothing changes any more)
            return label, {"rounds": rounds + int(quiet[0]) + 1, "bad_faces": int(host[0, 1])}
        rounds += per_read
        if rounds >= MAX_ROUNDS:
            raise _lib.DmvsError(f"components: no fixpoint after {rounds} rounds")


def area_scale(verts: torch.Tensor, n_faces: int):
    """(scale, cap) of dmvs_mesh_face_tally_i64: no triangle inside the bounding box of the finite vertices has more area than half its
    squared diagonal, and scale = pow2_scale_below(that, F) keeps the int64 sum of F scaled areas below 2^62"""
    ok = torch.isfinite(verts).all(1) if verts.shape[0] else None
    big = 0.0
    if ok is not None and bool(ok.any()):
        p = verts[ok].double()
        big = 0.5 * float(((p.max(0).values - p.min(0).values) ** 2).sum())
    if not (big > 0.0 and math.isfinite(big)):
        big = 1.0
    scale = pow2_scale_below(big, int(n_faces))
    return scale, big * scale


def component_table(ops: Ops, verts, faces, label, blocks: int = 0) -> dict:
    """-> {"roots" [C] int64 ascending: the components that have a face, "faces" [C] int64, "area_fixed" [C] int64, "area" [C] fp64
    (= area_fixed / scale), "area_q" [F] int64: every face's scaled area (0 for a face with an index outside [0, N)), "scale", "cap"}"""
    verts, faces = _mesh(ops, verts, faces)
    scale, cap = area_scale(verts, faces.shape[0])
    area_q, cf, ca = ops.mesh_face_tally(verts, faces, label, scale, cap, blocks=blocks)
    roots = torch.nonzero(cf > 0).squeeze(1)
    return {"roots": roots, "faces": cf[roots].long(), "area_fixed": ca[roots], "area": ca[roots].double() / scale, "area_q": area_q,
            "scale": scale, "cap": cap}


def clean(ops: Ops, verts, rgb, faces, min_faces: int = 0, min_fraction: float | None = None, keep_largest: int | None = None, blocks: int = 0):
    """Drops every component that has fewer than min_faces faces, fewer than min_fraction of the largest component's faces, or is not
    among the keep_largest by face count (ties go to the smaller root); with them go the faces with an index outside [0, N) and the
    vertices no kept face names.  rgb: [N,3] or None.  -> (verts', rgb', faces' int32, info): survivors in their order; info =
    {components, kept, faces_removed, vertices_removed, bad_faces, rounds, largest_faces, largest_area}"""
    verts, faces = _mesh(ops, verts, faces)
    if rgb is not None:
        rgb = torch.as_tensor(np.ascontiguousarray(rgb) if isinstance(rgb, np.ndarray) else rgb).to(ops.device)
        if rgb.shape[0] != verts.shape[0]:
            raise _lib.DmvsError(f"clean: {rgb.shape[0]} colours for {verts.shape[0]} vertices")
    N, F = int(verts.shape[0]), int(faces.shape[0])
    label, lab = components(ops, faces, N, blocks=blocks)
    tab = component_table(ops, verts, faces, label, blocks=blocks)
    roots, nf = tab["roots"], tab["faces"]
    C = int(roots.numel())
    keep = torch.ones(C, dtype=torch.bool, device=ops.device)
    largest = int(nf.max()) if C else 0
    keep &= nf >= int(min_faces)
    if min_fraction is not None:
        keep &= nf.double() >= float(min_fraction) * largest
    if keep_largest is not None:
        order = torch.sort(-nf, stable=True).indices      # (roots ascend: of equal counts the smaller root comes first)
        top = torch.zeros(C, dtype=torch.bool, device=ops.device)
        top[order[:max(0, int(keep_largest))]] = True
        keep &= top
    keep_root = torch.zeros(N, dtype=torch.bool, device=ops.device)
    keep_root[roots[keep]] = True
    lf = faces.long()
    in_range = ((lf >= 0) & (lf < N)).all(1)
    keep_face = in_range.clone()
    if N > 0 and F > 0:
        keep_face &= keep_root[label.long()[lf[:, 0].clamp(0, N - 1)]]
    kept_faces = lf[keep_face]
    used = torch.zeros(N, dtype=torch.bool, device=ops.device)
    used[kept_faces.reshape(-1)] = True
    new_index = torch.cumsum(used, 0) - 1
    info = {"components": C, "kept": int(keep.sum()), "faces_removed": F - int(kept_faces.shape[0]), "vertices_removed": N - int(used.sum()),
            "bad_faces": lab["bad_faces"], "rounds": lab["rounds"], "largest_faces": largest,
            "largest_area": float(tab["area"][torch.argmax(nf)]) if C else 0.0}
    return verts[used], None if rgb is None else rgb[used], new_index[kept_faces].to(torch.int32), info


def clean_file(ops: Ops, mesh_ply: str, out_ply: str, **kw) -> dict:
    verts, rgb, faces = IO.read_ply_mesh(mesh_ply)
    v, c, f, info = clean(ops, verts, rgb, faces, **kw)
    colours = c.cpu().numpy() if c is not None else np.zeros((int(v.shape[0]), 3), np.uint8)
    IO.write_ply(out_ply, v.cpu().numpy(), colours, faces=f.cpu().numpy())
    return dict(info, ply=out_ply, vertices=int(v.shape[0]), faces=int(f.shape[0]))


def main(argv=None, device="cuda:0", ops=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--mesh", required=True, help="the triangle mesh to clean (binary PLY)")
    ap.add_argument("--out", required=True, help="the PLY to write")
    ap.add_argument("--min_faces", type=int, default=0, help="drop components with fewer faces")
    ap.add_argument("--min_fraction", type=float, default=None, help="drop components with less than this share of the largest one's faces")
    ap.add_argument("--keep_largest", type=int, default=None, help="keep only this many components, by face count")
    a = ap.parse_args(argv)
    res = clean_file(ops or Ops.for_device(device), a.mesh, a.out, min_faces=a.min_faces, min_fraction=a.min_fraction, keep_largest=a.keep_largest)
    print(json.dumps({"mesh_clean": res}), flush=True)
    return res


if __name__ == "__main__":
    main()
