#!/usr/bin/env python3
"""Mesh simplification (dmvs_mesh_cluster_verts_i64, dmvs_mesh_cluster_quadrics_i64, dmvs_mesh_cluster_place_f32,
dmvs_mesh_cluster_remap_i32) on the project's own mesh: prints one JSON line (profiles/mesh_simplify_line.json).

    python tools/mesh_simplify_bench.py [--views 49] [--size 864 1152] [--dim 512] [--reps 5] [--cells 2 4] [--out FILE]

The mesh of tools/mesh_clean_bench.py (the rippled sphere of tools/tsdf_bench.py fused at --dim^3 voxels and extracted), clustered on
lattices of --cells voxels.  Timed with device events, no allocation inside the window, the median of --reps after a warm-up:
  the vertex pass, the face pass with the in-wave combine of runs and without it (csrc/mesh_simplify.hip compiled with
  -DDMVS_MESH_QUADRIC_PLAIN into a library of its own beside the product), alternating call by call, the sums compared; the cluster
  pass and the remap; the torch plumbing (the lattice and the removal of repeats) and the whole simplify() call on the wall clock.
The baseline is the numpy restatement of the two summing passes on the host (np.add.at), at the first cell.  Fidelity: the simplified
mesh's samples against the original mesh's samples at spacing = one voxel (diffmvs_amd.mesh_eval / cloud_eval), for both placements."""
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
import mesh_clean_bench as MB  # noqa: E402
from diffmvs_amd import _lib, build as B, cloud_eval as CE, cloud_grid as G, mesh_clean as MC, mesh_eval as ME, mesh_simplify as MS  # noqa: E402
from diffmvs_amd.ops import Ops, _ptr  # noqa: E402

PLAIN_LIB = os.path.join(B.PKG, "libdmvs_mesh_quadric_plain.so")


def plain_lib(load=True):
    """csrc/mesh_simplify.hip alone with the in-wave combine compiled out -> diffmvs_amd/libdmvs_mesh_quadric_plain.so (built when stale)"""
    src = os.path.join(B.CSRC, "mesh_simplify.hip")
    deps = [src, os.path.join(B.CSRC, "cloud_walk.h"), os.path.join(B.CSRC, "dmvs_common.h"), os.path.join(B.ROOT, "include", "dmvs.h")]
    if not os.path.exists(PLAIN_LIB) or any(os.path.getmtime(d) > os.path.getmtime(PLAIN_LIB) for d in deps):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                        "-DDMVS_MESH_QUADRIC_PLAIN", "-I", os.path.join(B.ROOT, "include"), "-I", B.CSRC, src, "-o", PLAIN_LIB], check=True)
    if not load:
        return None
    dll = C.CDLL(PLAIN_LIB)
    for name in ("dmvs_mesh_cluster_verts_i64", "dmvs_mesh_cluster_quadrics_i64"):
        getattr(dll, name).argtypes, getattr(dll, name).restype = _lib.SIGNATURES[name], C.c_int
    return dll


def host_sums(verts, faces, cluster, K, origin, cell, scale, cap):
    """the two summing passes in numpy (include/dmvs.h restated) -> (cnt, pos_q, quad_q, seconds without the copies)"""
    V, f, cl = verts.cpu().numpy().astype(np.float64), faces.cpu().numpy().astype(np.int64), cluster.cpu().numpy().astype(np.int64)
    t0 = time.perf_counter()
    t = (V - np.asarray(origin)) / cell
    U = t - (np.floor(t) + 0.5)
    cnt = np.bincount(cl, minlength=K)
    pos_q, quad_q = np.zeros((K, 3), np.int64), np.zeros((K, 10), np.int64)
    np.add.at(pos_q, cl, np.rint(U * 2.0 ** 32).astype(np.int64))
    P, kf = V[f], cl[f]
    a, b = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    c = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    l = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
    live = l > 0
    with np.errstate(all="ignore"):
        n, w = c / l[:, None], np.minimum((0.5 * l) / (cell * cell), cap)
    for j in range(3):
        new = live.copy()
        for before in range(j):
            new &= kf[:, j] != kf[:, before]
        u = U[f[:, j]]
        d = -((n[:, 0] * u[:, 0] + n[:, 1] * u[:, 1]) + n[:, 2] * u[:, 2])
        wx, wy, wz, wd = w * n[:, 0], w * n[:, 1], w * n[:, 2], w * d
        T = np.stack([wx * n[:, 0], wx * n[:, 1], wx * n[:, 2], wy * n[:, 1], wy * n[:, 2], wz * n[:, 2], wd * n[:, 0], wd * n[:, 1], wd * n[:, 2], wd * d], 1)
        np.add.at(quad_q, kf[new, j], np.rint(T[new] * scale).astype(np.int64))
    return cnt, pos_q, quad_q, time.perf_counter() - t0


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(out)), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=49)
    ap.add_argument("--size", type=int, nargs=2, default=[864, 1152], help="H W")
    ap.add_argument("--dim", type=int, default=512, help="the volume the mesh is extracted from has this many voxels a side")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0], help="lattice cells, in voxels")
    ap.add_argument("--build_only", action="store_true", help="build the comparison library and stop (no device needed)")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    if a.build_only:
        plain_lib(load=False)
        return
    ops = Ops.for_device("cuda:0")
    dev = ops.device
    verts, faces, h = MB.own_mesh(ops, a)
    N, F = int(verts.shape[0]), int(faces.shape[0])
    call, st = ops.lib.call, ops.stream
    plain = plain_lib()
    vol_origin = (-1.25, -1.25, -1.25)
    reference = ME.sample_surface(ops, verts, faces, h)[0]
    per_cell = {}
    for i, voxels in enumerate(a.cells):
        cell = voxels * h
        cluster, cells, origin = MS._lattice(verts, cell, vol_origin)
        K = int(cells.shape[0])
        o = (C.c_double * 3)(*origin)
        big = MC.area_scale(verts, F)
        cap = min(MS.MAX_WEIGHT, (big[1] / big[0]) / (cell * cell))
        scale = G.pow2_scale_below(cap, 3 * F)
        cnt = torch.empty(K, dtype=torch.int32, device=dev)
        pos_q = torch.empty((K, 3), dtype=torch.int64, device=dev)
        quad_q = torch.empty((K, 10), dtype=torch.int64, device=dev)
        state = torch.empty(3, dtype=torch.int64, device=dev)
        new_verts = torch.empty((K, 3), dtype=torch.float32, device=dev)
        out_faces = torch.empty((F, 3), dtype=torch.int32, device=dev)
        keep = torch.empty(F, dtype=torch.uint8, device=dev)

        def vert_args():
            return (_ptr(verts), None, N, _ptr(cluster), K, o, cell, _ptr(cnt), _ptr(pos_q), None, 0, st())

        def face_args():
            return (_ptr(verts), N, _ptr(faces), F, _ptr(cluster), K, o, cell, scale, cap, _ptr(quad_q), _ptr(state), 0, st())

        def checked(fn, args):
            rc = fn(*args)
            assert rc == 0, rc

        passes = {"verts": {"combine": lambda: call("dmvs_mesh_cluster_verts_i64", *vert_args()),
                            "plain": lambda: checked(plain.dmvs_mesh_cluster_verts_i64, vert_args())},
                  "faces": {"combine": lambda: call("dmvs_mesh_cluster_quadrics_i64", *face_args()),
                            "plain": lambda: checked(plain.dmvs_mesh_cluster_quadrics_i64, face_args())}}
        ms, same = {}, {}
        for name, pair in passes.items():
            got, kept = {"combine": [], "plain": []}, {}
            for rep in range(a.reps + 1):
                for mode, fn in pair.items():
                    t = TB.timed(fn, 1)
                    if rep:                                               # (rep 0 is the warm-up of both)
                        got[mode].append(t)
                    kept[mode] = (cnt.clone(), pos_q.clone(), quad_q.clone())
            ms[name] = {k: round(float(np.median(v)), 3) for k, v in got.items()}
            same[name] = all(torch.equal(x, y) for x, y in zip(kept["combine"], kept["plain"]))
        passes["verts"]["combine"]()
        passes["faces"]["combine"]()

        def place():
            call("dmvs_mesh_cluster_place_f32", K, _ptr(cnt), _ptr(pos_q), None, _ptr(quad_q), _ptr(cells), o, cell, scale, 2.0 ** -10,
                 _lib.SIMPLIFY_QUADRIC, _ptr(new_verts), None, _ptr(state), st())

        def remap():
            call("dmvs_mesh_cluster_remap_i32", _ptr(verts), N, _ptr(faces), F, _ptr(cluster), K, _ptr(new_verts), _ptr(out_faces), _ptr(keep),
                 _ptr(state), 0, st())
        place()
        remap()
        ms["place"], ms["remap"] = round(TB.timed(place, a.reps), 3), round(TB.timed(remap, a.reps), 3)
        ms["torch_lattice_wall"] = wall_ms(lambda: MS._lattice(verts, cell, vol_origin), a.reps)
        ms["torch_repeats_wall"] = wall_ms(lambda: MS._survivors(out_faces, keep, K), a.reps)
        ms["simplify_wall"] = wall_ms(lambda: MS.simplify(ops, verts, None, faces, cell, origin=vol_origin), a.reps)
        row = {"cell_voxels": voxels, "cell": cell, "clusters": K, "scale": scale, "cap": cap, "ms": ms, "same_sums": same}
        if i == 0:
            hc, hp, hq, host_s = host_sums(verts, faces, cluster, K, origin, cell, scale, cap)
            row["host_numpy"] = {"s": round(host_s, 3), "what": "both summing passes with np.add.at, without the copies",
                                 "over_gpu": round(host_s * 1e3 / (ms["verts"]["combine"] + ms["faces"]["combine"]), 1),
                                 "same_integers": bool(np.array_equal(hc, cnt.cpu().numpy()) and np.array_equal(hp, pos_q.cpu().numpy())
                                                       and np.array_equal(hq, quad_q.cpu().numpy()))}
        for placement in ("quadric", "mean"):
            v, _, f, info = MS.simplify(ops, verts, None, faces, cell, origin=vol_origin, placement=placement)
            pts = ME.sample_surface(ops, v, f, h)[0]
            score = CE.evaluate(ops, pts, reference, 8 * h, [h])
            row[placement] = {"faces": info["faces"], "vertices": info["vertices"], "fallback_clusters": info["fallback_clusters"],
                              "flipped_faces": info["flipped_faces"], "duplicate_faces": info["duplicate_faces"],
                              "accuracy_voxels": score["accuracy"] / h, "completeness_voxels": score["completeness"] / h}
        per_cell[str(voxels)] = row
        del cnt, pos_q, quad_q, new_verts, out_faces, keep
    shown = [w for i, w in enumerate(sys.argv[1:]) if w != "--out" and (i == 0 or sys.argv[i] != "--out")]
    line = {"metric": "mesh simplification: vertex / face / cluster / remap passes, ms", "command": ("python tools/mesh_simplify_bench.py " + " ".join(shown)).strip(),
            "reps": a.reps, "voxels": a.dim ** 3, "voxel": h, "vertices": N, "faces": F, "cells": per_cell,
            "fidelity": "mesh_eval samples at spacing = one voxel of the simplified mesh against those of the original, mean distances in voxels"}
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
