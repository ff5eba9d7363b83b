#!/usr/bin/env python3
"""Mesh cleaning and sampling (dmvs_mesh_label_round_i32, dmvs_mesh_face_tally_i64, dmvs_mesh_sample_f32) on the project's own mesh:
prints one JSON line (profiles/mesh_clean_line.json).

    python tools/mesh_clean_bench.py [--views 49] [--size 864 1152] [--dim 512] [--reps 5] [--out FILE]

The scene of tools/tsdf_bench.py -- a rippled sphere seen by --views cameras -- fused at --dim^3 voxels and extracted, as
tools/mesh_render_bench.py does.  Timed with device events, no allocation inside the window, the median of --reps after a warm-up:
  labelling: rounds to the fixpoint INCLUDING the host reads of their counters (1, 2 and 4 rounds per read), and one round alone;
  the tally with the in-wave combine and without it (csrc/mesh_clean.hip compiled with -DDMVS_MESH_TALLY_PLAIN into a library of its own
  beside the product), alternating call by call; the sums are compared;
  sampling at spacing = the voxel side.
Bytes are the algorithm's own (modelled from the arrays each lane touches, not measured), over the kernel time, as a share of the HBM peak.
Beside them the only other way to those labels: scipy.sparse.csgraph.connected_components on the host if scipy imports, else a numpy
min-label iteration; that figure includes the device-to-host copy of the faces."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import tsdf_bench as TB  # noqa: E402
from diffmvs_amd import _lib, build as B, mesh_clean as MC  # noqa: E402
from diffmvs_amd.ops import Ops, _ptr  # noqa: E402

HBM_PEAK_GBS = 8000.0      # the spec peak bench.py uses


def own_mesh(ops, a):
    H, W = a.size
    depth, valid, rgb, views = TB.scene(a.views, H, W, ops.device)
    h = 2.5 / (a.dim - 1)
    vol = ops.tsdf_volume((a.dim,) * 3, np.array([-1.25, -1.25, -1.25]), h)
    ops.tsdf_integrate(vol, depth, valid, rgb, views, 4 * h)
    verts, _, faces = ops.tsdf_extract(vol, min_weight=2)
    del vol, depth, valid, rgb
    torch.cuda.empty_cache()
    return verts, faces, h


def plain_tally_lib():
    """csrc/mesh_clean.hip alone with the in-wave combine compiled out -> diffmvs_amd/libdmvs_mesh_tally_plain.so (built when stale)"""
    src, lib = os.path.join(B.CSRC, "mesh_clean.hip"), os.path.join(B.PKG, "libdmvs_mesh_tally_plain.so")
    deps = [src, os.path.join(B.CSRC, "cloud_walk.h"), os.path.join(B.CSRC, "dmvs_common.h"), os.path.join(B.ROOT, "include", "dmvs.h")]
    if not os.path.exists(lib) or any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-DDMVS_MESH_TALLY_PLAIN",
                        "-I", os.path.join(B.ROOT, "include"), "-I", B.CSRC, src, "-o", lib], check=True)
    dll = C.CDLL(lib)
    dll.dmvs_mesh_face_tally_i64.argtypes, dll.dmvs_mesh_face_tally_i64.restype = _lib.SIGNATURES["dmvs_mesh_face_tally_i64"], C.c_int
    return dll


def host_labels(faces_dev, N):
    """-> (labels as the smallest vertex index of each component, seconds, which)"""
    t0 = time.perf_counter()
    f = faces_dev.cpu().numpy().astype(np.int64)
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        which = "scipy.sparse.csgraph.connected_components"
        rows, cols = np.concatenate([f[:, 0], f[:, 1]]), np.concatenate([f[:, 1], f[:, 2]])
        comp = connected_components(coo_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(N, N)), directed=False)[1]
        smallest = np.full(comp.max() + 1 if N else 0, N, np.int64)
        np.minimum.at(smallest, comp, np.arange(N))
        lab = smallest[comp]
    except ImportError:
        which = "numpy min-label iteration"
        lab = np.arange(N, dtype=np.int64)
        while True:
            new = lab.copy()
            np.minimum.at(new, f.ravel(), np.repeat(lab[f].min(1), 3))
            new = np.minimum(new, new[new])
            if np.array_equal(new, lab):
                break
            lab = new
    return lab.astype(np.int32), time.perf_counter() - t0, which


def gbs(nbytes, ms):
    g = nbytes / (ms * 1e-3) / 1e9
    return {"bytes": int(nbytes), "GB_per_s": round(g, 1), "frac_of_hbm_peak": round(g / HBM_PEAK_GBS, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--size", type=int, nargs=2, default=[864, 1152], help="H W")
    ap.add_argument("--dim", type=int, default=512, help="the volume the mesh is extracted from has this many voxels a side")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    ops = Ops.for_device("cuda:0")
    dev = ops.device
    verts, faces, h = own_mesh(ops, a)
    N, F = int(verts.shape[0]), int(faces.shape[0])
    call, st = ops.lib.call, ops.stream

    # ---- labelling
    iota = torch.arange(N, dtype=torch.int32, device=dev)
    label = iota.clone()
    states = torch.empty((4, 2), dtype=torch.int32, device=dev)
    pinned = torch.empty((4, 2), dtype=torch.int32).pin_memory()
    rounds = {}

    def label_loop(per_read):
        n = 0
        while True:
            for k in range(per_read):
                call("dmvs_mesh_label_round_i32", _ptr(faces), F, N, _ptr(label), _ptr(states[k]), 0, st())
            pinned[:per_read].copy_(states[:per_read], non_blocking=True)
            torch.cuda.current_stream().synchronize()
            quiet = np.nonzero(pinned[:per_read, 0].numpy() == 0)[0]
            if quiet.size:
                rounds[per_read] = n + int(quiet[0]) + 1
                return
            n += per_read

    label_loop(1)                                                     # warm-up
    label_ms = {str(p): round(TB.timed(lambda p=p: label_loop(p), a.reps, before=lambda: label.copy_(iota)), 3) for p in (1, 2, 4)}
    final = label.clone()
    one_round_ms = TB.timed(lambda: call("dmvs_mesh_label_round_i32", _ptr(faces), F, N, _ptr(label), _ptr(states[0]), 0, st()), a.reps,
                            before=lambda: label.copy_(iota))          # the first round: every face writes
    settled_round_ms = TB.timed(lambda: call("dmvs_mesh_label_round_i32", _ptr(faces), F, N, _ptr(label), _ptr(states[0]), 0, st()), a.reps,
                                before=lambda: label.copy_(final))     # a round at the fixpoint: reads only
    round_bytes = 12 * F + 24 * F + 8 * N                             # faces, two loads per vertex of a face, two per vertex in the shortcut
    host_lab, host_s, which = host_labels(faces, N)
    lab2, info = MC.components(ops, faces, N)
    same_labels = bool(np.array_equal(final.cpu().numpy(), host_lab)) and bool(torch.equal(lab2, final))

    # ---- tally, with and without the in-wave combine, alternating
    scale, cap = MC.area_scale(verts, F)
    area_q = torch.empty(F, dtype=torch.int64, device=dev)
    cf = torch.empty(N, dtype=torch.int32, device=dev)
    ca = torch.empty(N, dtype=torch.int64, device=dev)

    plain = plain_tally_lib()

    def tally():
        call("dmvs_mesh_face_tally_i64", _ptr(verts), N, _ptr(faces), F, _ptr(final), scale, cap, _ptr(area_q), _ptr(cf), _ptr(ca), 0, st())

    def tally_plain():
        rc = plain.dmvs_mesh_face_tally_i64(_ptr(verts), N, _ptr(faces), F, _ptr(final), scale, cap, _ptr(area_q), _ptr(cf), _ptr(ca), 0, st())
        assert rc == 0, rc

    ms, keep = {"combine": [], "plain": []}, {}
    for rep in range(a.reps + 1):
        for mode, fn in (("combine", tally), ("plain", tally_plain)):
            t = TB.timed(fn, 1)
            if rep:                                                   # (rep 0 is the warm-up of both)
                ms[mode].append(t)
            keep[mode] = (area_q.clone(), cf.clone(), ca.clone())
    same_sums = all(torch.equal(x, y) for x, y in zip(keep["combine"], keep["plain"]))
    tally_ms = {k: round(float(np.median(v)), 3) for k, v in ms.items()}
    tally_bytes = 12 * F + 36 * F + 4 * F + 8 * F + 12 * N            # faces, three vertices, a label, area_q; the two zeroed tables
    roots = torch.nonzero(cf > 0).squeeze(1)

    # ---- sampling at spacing = the voxel side
    tally()
    area_cum = torch.cumsum(area_q, 0)
    a0 = max(1, int(np.rint(h * h * scale)))
    M = int(area_cum[-1]) // a0
    points = torch.empty((M, 3), dtype=torch.float32, device=dev)
    face_of = torch.empty(M, dtype=torch.int32, device=dev)

    def sample():
        call("dmvs_mesh_sample_f32", _ptr(verts), N, _ptr(faces), F, _ptr(area_cum), a0, M, _ptr(points), _ptr(face_of), 0, st())
    sample()
    sample_ms = TB.timed(sample, a.reps)
    sample_bytes = M * (16 + 12 + 36 + 8 * int(np.ceil(np.log2(max(F, 2)))))      # outputs, a face, its vertices, the search's loads

    shown = [w for i, w in enumerate(sys.argv[1:]) if w != "--out" and (i == 0 or sys.argv[i] != "--out")]
    line = {"metric": "mesh components / face tally / area sampling, ms", "command": ("python tools/mesh_clean_bench.py " + " ".join(shown)).strip(),
            "reps": a.reps, "hbm_peak_GBs": HBM_PEAK_GBS, "voxels": a.dim ** 3, "voxel": h, "vertices": N, "faces": F,
            "components": int(roots.numel()), "largest_component_faces": int(cf.max()) if N else 0,
            "label": {"rounds": rounds, "ms_by_rounds_per_read": label_ms, "rounds_per_read_default": MC.ROUNDS_PER_READ, "first_round_ms": round(one_round_ms, 3),
                      "settled_round_ms": round(settled_round_ms, 3), "settled_round": gbs(round_bytes, settled_round_ms),
                      "components_call": info, "same_labels_as_host": same_labels},
            "host_labels": {"how": which, "s": round(host_s, 3), "includes": "the device-to-host copy of the faces",
                            "over_gpu": round(host_s * 1e3 / label_ms[str(MC.ROUNDS_PER_READ)], 1)},
            "tally": {"ms": tally_ms, "same_sums": same_sums, "combine": gbs(tally_bytes, tally_ms["combine"]), "plain": gbs(tally_bytes, tally_ms["plain"])},
            "sample": {"spacing": h, "a0": a0, "M": M, "ms": round(sample_ms, 3), **gbs(sample_bytes, sample_ms)},
            "bytes": "modelled from the arrays a lane touches, not measured"}
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
