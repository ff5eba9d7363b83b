"""Mesh simplification (csrc/mesh_simplify.hip, diffmvs_amd/mesh_simplify.py) against a numpy restatement of the contract in include/dmvs.h
at tolerance zero: the integer sums as integers, the placed vertices by their bit patterns, the remapped faces and every counter.  Every
kernel test runs on the host emulation here and on the MI355X under -m gpu."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT  # noqa: F401
from diffmvs_amd import _lib, cloud_grid as G, formats as IO, mesh as M, mesh_clean as MC, mesh_simplify as MS
from test_mesh_clean import uv_sphere


# ------------------------------------------------------------------------------------------ the contract, restated
def local(p, origin, cell):
    with np.errstate(all="ignore"):
        t = (np.asarray(p, np.float64) - np.asarray(origin, np.float64)) / cell
        return np.where(np.isfinite(t), t - (np.floor(t) + 0.5), 0.0)


def restate_lattice(verts, cell, origin=None):
    """-> (cluster [N] int32: the rank of the vertex's cell among the occupied cells in (z, y, x) order, -1 for a non-finite vertex; cells
    [K,3] int64; origin)"""
    v = np.asarray(verts, np.float32).astype(np.float64)
    ok = np.isfinite(v).all(1)
    if origin is None:
        origin = v[ok].min(0)
    c = np.floor((v[ok] - np.asarray(origin, np.float64)) / cell).astype(np.int64)
    assert c.min() >= 0
    zyx, inverse = np.unique(c[:, ::-1], axis=0, return_inverse=True)
    cluster = np.full(len(v), -1, np.int32)
    cluster[ok] = inverse.reshape(-1)
    return cluster, np.ascontiguousarray(zyx[:, ::-1]), tuple(float(o) for o in origin)


def face_tables(verts, faces, cluster):
    verts, faces, N = np.asarray(verts, np.float32), np.asarray(faces, np.int64).reshape(-1, 3), len(verts)
    inr = ((faces >= 0) & (faces < N)).all(1)
    fc = np.clip(faces, 0, max(N - 1, 0))
    kf = np.asarray(cluster, np.int64)[fc]
    return verts.astype(np.float64), fc, kf, inr & (kf >= 0).all(1)


def cross(P):
    with np.errstate(all="ignore"):
        a, b = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def restate_sums(verts, rgb, faces, cluster, K, origin, cell, scale, cap):
    """-> (cnt [K], pos_q [K,3], rgb_sum [K,3], quad_q [K,10] as int64, bad faces, flat faces)"""
    V, fc, kf, ok = face_tables(verts, faces, cluster)
    cluster = np.asarray(cluster, np.int64)
    has = cluster >= 0
    U = local(V, origin, cell)
    cnt = np.bincount(cluster[has], minlength=K).astype(np.int64)
    pos_q, rgb_sum, quad_q = np.zeros((K, 3), np.int64), np.zeros((K, 3), np.int64), np.zeros((K, 10), np.int64)
    np.add.at(pos_q, cluster[has], np.rint(U[has] * 2.0 ** 32).astype(np.int64))
    if rgb is not None:
        np.add.at(rgb_sum, cluster[has], np.asarray(rgb, np.int64)[has])
    with np.errstate(all="ignore"):
        c = cross(V[fc])
        l = np.sqrt((c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2])
        live = ok & (l > 0) & np.isfinite(l)
        n = c / l[:, None]
        w = np.minimum((0.5 * l) / (cell * cell), cap)
        for j in range(3):
            new = live.copy()
            for before in range(j):
                new &= kf[:, j] != kf[:, before]
            u = U[fc[:, j]]
            d = -((n[:, 0] * u[:, 0] + n[:, 1] * u[:, 1]) + n[:, 2] * u[:, 2])
            wx, wy, wz, wd = w * n[:, 0], w * n[:, 1], w * n[:, 2], w * d
            T = np.stack([wx * n[:, 0], wx * n[:, 1], wx * n[:, 2], wy * n[:, 1], wy * n[:, 2], wz * n[:, 2], wd * n[:, 0], wd * n[:, 1], wd * n[:, 2],
                          wd * d], 1)
            np.add.at(quad_q, kf[new, j], np.rint(T[new] * scale).astype(np.int64))
    return cnt, pos_q, rgb_sum, quad_q, int((~ok).sum()), int((ok & ~live).sum())


def restate_place(cnt, pos_q, rgb_sum, quad_q, cells, origin, cell, scale, reg, mean=False):
    """-> (verts [K,3] fp32, rgb [K,3] uint8, clusters with a quadric that fell back to the mean)"""
    with np.errstate(all="ignore"):
        q = quad_q.astype(np.float64) / scale
        n = cnt.astype(np.float64)
        m = np.where(cnt[:, None] > 0, (pos_q.astype(np.float64) / 2.0 ** 32) / n[:, None], 0.0)
        tr = (q[:, 0] + q[:, 3]) + q[:, 5]
        lam = reg * tr
        M00, M01, M02, M11, M12, M22 = q[:, 0] + lam, q[:, 1], q[:, 2], q[:, 3] + lam, q[:, 4], q[:, 5] + lam
        r0, r1, r2 = lam * m[:, 0] - q[:, 6], lam * m[:, 1] - q[:, 7], lam * m[:, 2] - q[:, 8]
        c00, c01, c02 = M11 * M22 - M12 * M12, M02 * M12 - M01 * M22, M01 * M12 - M02 * M11
        c11, c12, c22 = M00 * M22 - M02 * M02, M01 * M02 - M00 * M12, M00 * M11 - M01 * M01
        det = (M00 * c00 + M01 * c01) + M02 * c02
        x = np.stack([((c00 * r0 + c01 * r1) + c02 * r2) / det, ((c01 * r0 + c11 * r1) + c12 * r2) / det, ((c02 * r0 + c12 * r1) + c22 * r2) / det], 1)
        good = (tr > 0) & (det > 0) & np.isfinite(x).all(1)
        good &= np.abs(np.where(np.isfinite(x), x, 0.0)).max(1) <= 1.0
        fell = 0 if mean else int(((tr > 0) & ~good).sum())
        x = np.where((good & (not mean))[:, None], x, m)
        out = (np.asarray(origin, np.float64) + ((cells.astype(np.float64) + 0.5) + x) * cell).astype(np.float32)
    safe = np.maximum(cnt, 1)[:, None]
    rgb = np.where(cnt[:, None] > 0, (2 * rgb_sum + cnt[:, None]) // (2 * safe), 0).astype(np.uint8)
    return out, rgb, fell


def rotate(kf):
    first = np.where((kf[:, 0] <= kf[:, 1]) & (kf[:, 0] <= kf[:, 2]), 0, np.where(kf[:, 1] <= kf[:, 2], 1, 2))
    rows = np.arange(len(kf))
    return np.stack([kf[rows, first], kf[rows, (first + 1) % 3], kf[rows, (first + 2) % 3]], 1)


def restate_remap(verts, faces, cluster, new_verts):
    """-> (faces' [F,3] int32, keep [F] uint8, degenerate, flipped, bad)"""
    V, fc, kf, ok = face_tables(verts, faces, cluster)
    kf = np.where(ok[:, None], kf, -1)
    distinct = (kf[:, 0] != kf[:, 1]) & (kf[:, 0] != kf[:, 2]) & (kf[:, 1] != kf[:, 2])
    keep = ok & distinct
    flipped = 0
    if new_verts is not None:
        c, cn = cross(V[fc][keep]), cross(np.asarray(new_verts, np.float32).astype(np.float64)[kf[keep]])
        flipped = int((((c[:, 0] * cn[:, 0] + c[:, 1] * cn[:, 1]) + c[:, 2] * cn[:, 2]) < 0).sum())
    return rotate(kf).astype(np.int32), keep.astype(np.uint8), int((ok & ~distinct).sum()), flipped, int((~ok).sum())


def weights(ops, verts, n_faces, cell):
    """(scale, cap) as the issue states them: cap = min(1024, the bounding-box bound of mesh_clean.area_scale / cell^2)"""
    s, c = MC.area_scale(dev(ops, np.asarray(verts, np.float32)), n_faces)
    cap = min(1024.0, (c / s) / (cell * cell))
    return G.pow2_scale_below(cap, 3 * n_faces), cap


def restate_simplify(ops, verts, rgb, faces, cell, origin=None, mean=False, reg=2.0 ** -10):
    """the whole of mesh_simplify.simplify -> (verts', rgb', faces', info without cell / origin)"""
    cluster, cells, origin = restate_lattice(verts, cell, origin)
    K = len(cells)
    scale, cap = weights(ops, verts, len(faces), cell)
    cnt, pos_q, rgb_sum, quad_q, bad, flat = restate_sums(verts, rgb, faces, cluster, K, origin, cell, scale, cap)
    nv, nc, fell = restate_place(cnt, pos_q, rgb_sum, quad_q, cells, origin, cell, scale, reg, mean)
    fk, keep, degenerate, flipped, bad2 = restate_remap(verts, faces, cluster, nv)
    assert bad2 == bad
    kept = fk[keep != 0]
    _, firsts = np.unique(kept, axis=0, return_index=True)      # (the first of equal rows)
    kept = kept[np.sort(firsts)]
    used = np.zeros(K, bool)
    used[kept.reshape(-1)] = True
    new_index = np.cumsum(used) - 1
    info = {"clusters": K, "vertices": int(used.sum()), "faces": len(kept), "bad_faces": bad, "flat_faces": flat, "degenerate_faces": degenerate,
            "duplicate_faces": int((keep != 0).sum()) - len(kept), "flipped_faces": flipped, "fallback_clusters": fell, "scale": scale}
    return nv[used], None if rgb is None else nc[used], new_index[kept].astype(np.int32).reshape(-1, 3), info


# ------------------------------------------------------------------------------------------ meshes
def dev(ops, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(None)
def cube(n=24):
    """the unit cube, n x n quads per side, shared vertices along the edges: closed, normals outward"""
    index, verts, faces = {}, [], []

    def vid(p):
        if p not in index:
            index[p] = len(verts)
            verts.append(p)
        return index[p]

    for axis in range(3):
        for side in (0, n):
            for i in range(n):
                for j in range(n):
                    quad = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0, 0, 0]
                        p[axis], p[(axis + 1) % 3], p[(axis + 2) % 3] = side, i + di, j + dj
                        quad.append(vid(tuple(p)))
                    if side == 0:      # ((axis+1) x (axis+2) = +axis: the side at 0 is turned over)
                        quad = quad[::-1]
                    faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    return (np.array(verts, np.float64) / n).astype(np.float32), np.array(faces, np.int32)


def sheet(n=33, z=lambda x, y: 0.1 + 0.0 * x, reverse=False):
    """n x n vertices over the unit square at height z(x, y), normals up (down when reversed)"""
    g = np.arange(n) / (n - 1.0)
    x, y = np.meshgrid(g, g, indexing="ij")
    verts = np.stack([x, y, z(x, y)], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3).astype(np.int32)
    return verts, faces[:, ::-1].copy() if reverse else faces


def join(parts):
    verts, faces, off = [], [], 0
    for v, f in parts:
        verts.append(v)
        faces.append(f + off)
        off += len(v)
    return np.concatenate(verts), np.concatenate(faces).astype(np.int32)


def wedge():
    return join([sheet(), sheet(z=lambda x, y: 0.16 + 0.05 * x)])


def colours(n, seed=5):
    return np.random.RandomState(seed).randint(0, 256, (n, 3)).astype(np.uint8)


def cube_distance(p):
    """distance of points to the SURFACE of the unit cube"""
    p = np.asarray(p, np.float64)
    outside = np.linalg.norm(np.maximum(0.0, np.maximum(-p, p - 1.0)), axis=1)
    return np.where(outside > 0, outside, np.minimum(p, 1.0 - p).min(1))


def run_simplify(ops, verts, rgb, faces, cell, **kw):
    v, c, f, info = MS.simplify(ops, verts, rgb, faces, cell, **kw)
    assert v.dtype == torch.float32 and f.dtype == torch.int32 and (c is None or c.dtype == torch.uint8)
    assert info["vertices"] == int(v.shape[0]) and info["faces"] == int(f.shape[0]) and info["cell"] == cell
    return v.cpu().numpy(), None if c is None else c.cpu().numpy(), f.cpu().numpy(), info


def check_against_restatement(ops, verts, rgb, faces, cell, origin=None, **kw):
    got = run_simplify(ops, verts, rgb, faces, cell, origin=origin, **kw)
    want = restate_simplify(ops, verts, rgb, faces, cell, origin, mean=kw.get("placement") == "mean", reg=kw.get("reg", 2.0 ** -10))
    assert {k: got[3][k] for k in want[3]} == want[3]
    assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[2], want[2])
    assert (rgb is None and got[1] is None) or np.array_equal(got[1], want[1])
    return got


CUBE_CELLS = (0.25, 0.2, 1.0 / 6.0, 0.3)
CUBE_ORIGIN = (-0.013, -0.021, -0.017)


# ------------------------------------------------------------------------------------------ 1. the sums, as integers
@functools.lru_cache(None)
def soup():
    rs = np.random.RandomState(23)
    N, F = 3000, 2500
    verts = rs.uniform(-1.0, 1.0, (N, 3)).astype(np.float32)
    verts[1234] = (np.nan, 0.2, 0.3)
    faces = rs.randint(0, N, (F, 3)).astype(np.int32)
    faces[17], faces[900], faces[2499] = (5, -1, 9), (N, 3, 4), (1, 2, 2 ** 31 - 1)
    faces[40] = (1234, 7, 8)                       # a NaN vertex
    verts[2001] = verts[2000]
    faces[41] = (2000, 2001, 77)                   # zero area
    faces[42] = (300, 301, 300)                    # one vertex twice
    return verts, colours(N), faces


def test_sums_of_a_random_soup_equal_the_restatement(ops):
    verts, rgb, faces = soup()
    N, F, cell = len(verts), len(faces), 0.31
    cluster, cells, origin = restate_lattice(verts, cell)
    K = len(cells)
    got_cluster, got_cells, got_origin = MS._lattice(dev(ops, verts), cell)
    assert np.array_equal(got_cluster.cpu().numpy(), cluster) and np.array_equal(got_cells.cpu().numpy(), cells) and tuple(got_origin) == origin
    assert cluster[1234] == -1 and (np.delete(cluster, 1234) >= 0).all() and 100 < K < N
    scale, cap = weights(ops, verts, F, cell)
    assert np.frexp(scale)[0] == 0.5 and cap * scale * 3 * F < 2.0 ** 62
    cnt, pos_q, rgb_sum, quad_q, bad, flat = restate_sums(verts, rgb, faces, cluster, K, origin, cell, scale, cap)
    names_nan = ((faces == 1234).any(1) & ((faces >= 0) & (faces < N)).all(1)).sum()      # (the planted face and whatever the draw added)
    twice = (faces[:, 0] == faces[:, 1]) | (faces[:, 0] == faces[:, 2]) | (faces[:, 1] == faces[:, 2])
    assert bad == 3 + names_nan >= 4 and flat == 1 + twice.sum() >= 2 and cnt.sum() == N - 1 and np.abs(quad_q).max() > 2 ** 40
    for blocks in (1, 3, 0):      # one workgroup, several grid passes, the library's choice
        a = [t.cpu().numpy() for t in ops.mesh_cluster_verts(dev(ops, verts), dev(ops, rgb), dev(ops, cluster), K, origin, cell, blocks=blocks)]
        assert a[0].dtype == np.int32 and a[1].dtype == np.int64 and a[2].dtype == np.int64
        assert np.array_equal(a[0], cnt) and np.array_equal(a[1], pos_q) and np.array_equal(a[2], rgb_sum), blocks
        q, state = ops.mesh_cluster_quadrics(dev(ops, verts), dev(ops, faces), dev(ops, cluster), K, origin, cell, scale, cap, blocks=blocks)
        assert q.dtype == torch.int64 and np.array_equal(q.cpu().numpy(), quad_q) and state.cpu().tolist() == [bad, flat], blocks
    a = ops.mesh_cluster_verts(dev(ops, verts), None, dev(ops, cluster), K, origin, cell)
    assert a[2] is None and np.array_equal(a[0].cpu().numpy(), cnt) and np.array_equal(a[1].cpu().numpy(), pos_q)
    # the remap of the same soup, with and without the flip count
    nv = restate_place(cnt, pos_q, rgb_sum, quad_q, cells, origin, cell, scale, 2.0 ** -10)[0]
    fk, keep, degenerate, flipped, bad2 = restate_remap(verts, faces, cluster, nv)
    assert bad2 == bad and degenerate > 0 and flipped > 0 and keep.sum() > 2000
    for blocks in (1, 0):
        out, kp, st = ops.mesh_cluster_remap(dev(ops, verts), dev(ops, faces), dev(ops, cluster), K, new_verts=dev(ops, nv), blocks=blocks)
        assert np.array_equal(out.cpu().numpy(), fk) and np.array_equal(kp.cpu().numpy(), keep) and st.cpu().tolist() == [degenerate, flipped, bad2]
    out, kp, st = ops.mesh_cluster_remap(dev(ops, verts), dev(ops, faces), dev(ops, cluster), K)
    assert np.array_equal(out.cpu().numpy(), fk) and np.array_equal(kp.cpu().numpy(), keep) and st.cpu().tolist() == [degenerate, 0, bad2]


# ------------------------------------------------------------------------------------------ 2. runs of one cluster and their ends inside a wave
@functools.lru_cache(None)
def grid_case():
    n = 264
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    verts = np.stack([i, j, 3.0 * np.sin(i / 17.0) * np.cos(j / 23.0)], -1).reshape(-1, 3).astype(np.float32)
    idx = np.arange(n * n).reshape(n, n)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel(), idx[:-1, 1:].ravel()
    faces = np.stack([np.stack([a, b, c], 1), np.stack([a, c, d], 1)], 1).reshape(-1, 3).astype(np.int32)      # row order: a quad's two faces together
    cell, origin = 8.0, (-0.37, -0.41, -4.3)
    cluster, cells, origin = restate_lattice(verts, cell, origin)
    return verts, colours(len(verts)), faces, cell, origin, cluster, len(cells)


@functools.lru_cache(None)
def grid_sums(scale, cap):
    verts, rgb, faces, cell, origin, cluster, K = grid_case()
    return restate_sums(verts, rgb, faces, cluster, K, origin, cell, scale, cap)


def test_sums_with_long_runs_and_with_none_are_the_same_integers(ops):
    verts, rgb, faces, cell, origin, cluster, K = grid_case()
    F = len(faces)
    assert F == 138338 and 1000 < K < 2500
    scale, cap = weights(ops, verts, F, cell)
    cnt, pos_q, rgb_sum, quad_q, bad, flat = grid_sums(scale, cap)
    assert bad == 0 and flat == 0 and cnt.sum() == len(verts) and cnt.max() >= 64      # a cluster is about 8 x 8 vertices
    a = [t.cpu().numpy() for t in ops.mesh_cluster_verts(dev(ops, verts), dev(ops, rgb), dev(ops, cluster), K, origin, cell, blocks=3)]
    assert np.array_equal(a[0], cnt) and np.array_equal(a[1], pos_q) and np.array_equal(a[2], rgb_sum)
    shuffled = faces[np.random.RandomState(31).permutation(F)]
    for name, f, blocks in (("rows", faces, 3), ("rows", faces, 0), ("permuted", shuffled, 3)):      # 3 workgroups: 181 grid-stride passes
        q, state = ops.mesh_cluster_quadrics(dev(ops, verts), dev(ops, f), dev(ops, cluster), K, origin, cell, scale, cap, blocks=blocks)
        assert np.array_equal(q.cpu().numpy(), quad_q) and state.cpu().tolist() == [0, 0], (name, blocks)
    order = np.random.RandomState(32).permutation(len(verts))      # vertices without runs: the same sums per cluster
    a = [t.cpu().numpy() for t in ops.mesh_cluster_verts(dev(ops, verts[order]), dev(ops, rgb[order]), dev(ops, cluster[order]), K, origin, cell, blocks=3)]
    assert np.array_equal(a[0], cnt) and np.array_equal(a[1], pos_q) and np.array_equal(a[2], rgb_sum)


# ------------------------------------------------------------------------------------------ 3. placement, bit for bit
def test_placement_equals_the_restatement_bitwise(ops):
    cv, cf = cube()
    got = check_against_restatement(ops, cv, colours(len(cv)), cf, 0.25, origin=CUBE_ORIGIN)
    assert got[3]["fallback_clusters"] == 0 and got[3]["bad_faces"] == 0 and got[3]["flat_faces"] == 0
    check_against_restatement(ops, cv, colours(len(cv)), cf, 0.25, origin=CUBE_ORIGIN, placement="mean")
    check_against_restatement(ops, cv, None, cf, 0.2, origin=CUBE_ORIGIN, reg=2.0 ** -6)
    sv, sf = uv_sphere()
    got = check_against_restatement(ops, sv, colours(len(sv)), sf, 0.25)
    assert got[3]["fallback_clusters"] == 0 and got[3]["origin"] == [-1.0, -1.0, -1.0]
    wv, wf = wedge()
    got = check_against_restatement(ops, wv, colours(len(wv)), wf, 0.25, origin=(-0.01, -0.01, -0.01))
    assert got[3]["clusters"] == 25 and got[3]["fallback_clusters"] > 0      # the two planes meet far outside the cells
    print("wedge fallbacks", got[3]["fallback_clusters"])
    soup_v, soup_c, soup_f = soup()
    check_against_restatement(ops, soup_v, soup_c, soup_f, 0.31)


def test_a_given_origin_is_shifted_by_whole_cells(ops):
    cv, cf = cube()
    a = run_simplify(ops, cv, None, cf, 0.25, origin=(0.5, 0.25, 2.0))
    b = run_simplify(ops, cv, None, cf, 0.25, origin=(0.0, 0.0, 0.0))
    assert a[3]["origin"] == [0.0, 0.0, 0.0] and np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[2], b[2])
    with pytest.raises(ValueError, match="exceeds the 62-bit key"):
        MS.simplify(ops, cv, None, cf, 2.0 ** -22)
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="cell size"):
            MS.simplify(ops, cv, None, cf, bad)
    with pytest.raises(ValueError, match="placement"):
        MS.simplify(ops, cv, None, cf, 0.25, placement="median")
    with pytest.raises(ValueError, match="reg"):
        MS.simplify(ops, cv, None, cf, 0.25, reg=0.0)


# ------------------------------------------------------------------------------------------ 4. it is quadric placement
@pytest.mark.parametrize("cell", CUBE_CELLS)
def test_quadric_placement_keeps_the_cube_and_the_mean_does_not(ops, cell):
    cv, cf = cube()
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
    v, _, f, info = run_simplify(ops, cv, None, cf, cell, origin=CUBE_ORIGIN)
    far = cube_distance(v).max()
    to_corner = np.linalg.norm(v.astype(np.float64)[None] - corners[:, None], axis=2).min(1).max()
    vm, _, fm, _ = run_simplify(ops, cv, None, cf, cell, origin=CUBE_ORIGIN, placement="mean")
    far_mean = cube_distance(vm).max()
    print(f"cell {cell}: quadric {far:.3g} from the surface, corners within {to_corner:.3g}; mean {far_mean:.3g}; {info['faces']} faces")
    assert np.array_equal(f, fm) and info["faces"] < len(cf) // 8
    assert far <= 1e-3 and to_corner <= 5e-3 and far_mean >= 2e-2


# ------------------------------------------------------------------------------------------ 5. closed stays closed
def closed_surface(v, f, info):
    assert info["duplicate_faces"] == 0 and info["bad_faces"] == 0 and len(np.unique(f, axis=0)) == len(f)
    assert len(np.unique(f)) == len(v)      # every output vertex is used
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), 1)
    edges, counts = np.unique(e, axis=0, return_counts=True)
    assert (counts == 2).all(), np.bincount(counts)
    assert len(v) - len(edges) + len(f) == 2


@pytest.mark.parametrize("cell", CUBE_CELLS)
def test_the_simplified_cube_is_a_closed_surface(ops, cell):
    cv, cf = cube()
    v, _, f, info = run_simplify(ops, cv, None, cf, cell, origin=CUBE_ORIGIN)
    closed_surface(v, f, info)


@pytest.mark.parametrize("cell", (0.5, 0.25, 0.2, 0.125, 0.1))
def test_the_simplified_sphere_is_a_closed_surface(ops, cell):
    sv, sf = uv_sphere(32, 64)
    v, _, f, info = run_simplify(ops, sv, None, sf, cell)
    closed_surface(v, f, info)
    assert cell != 0.25 or (len(v), len(f)) == (269, 534)
    assert np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 1.0).max() < 0.5 * cell


# ------------------------------------------------------------------------------------------ 6. duplicates and orientation
def test_repeated_faces_go_and_opposite_ones_stay(ops):
    origin = (-0.01, -0.01, -0.01)
    low = sheet()
    verts, faces = join([low, sheet(z=lambda x, y: 0.14 + 0.0 * x)])
    alone = run_simplify(ops, low[0], None, low[1], 0.25, origin=origin)
    assert alone[3]["faces"] == 32 and alone[3]["duplicate_faces"] == 0 and alone[3]["clusters"] == 25
    v, _, f, info = run_simplify(ops, verts, None, faces, 0.25, origin=origin)
    assert info["faces"] == 32 and info["duplicate_faces"] == 32 and info["clusters"] == 25 and info["flipped_faces"] == 0
    assert np.array_equal(f, alone[2])      # the survivors are the first sheet's, in their order
    verts, faces = join([low, sheet(z=lambda x, y: 0.14 + 0.0 * x, reverse=True)])
    v, _, f, info = run_simplify(ops, verts, None, faces, 0.25, origin=origin)
    assert info["faces"] == 64 and info["duplicate_faces"] == 0 and np.array_equal(f[:32], alone[2])
    assert np.array_equal(np.unique(rotate(f[32:, ::-1].astype(np.int64)), axis=0), np.unique(alone[2], axis=0))      # the same triples, turned over


# ------------------------------------------------------------------------------------------ 7. cells below the shortest edge
@pytest.mark.parametrize("name", ("cube", "sphere"))
def test_tiny_cells_leave_the_mesh_as_it_is(ops, name):
    verts, faces, cell = (cube(4) + (0.2,)) if name == "cube" else (uv_sphere(8, 12) + (0.15,))
    v, _, f, info = run_simplify(ops, verts, None, faces, cell)
    cluster = restate_lattice(verts, cell)[0]
    assert info["clusters"] == info["vertices"] == len(verts) == len(np.unique(cluster)) and info["faces"] == len(faces)
    assert info["degenerate_faces"] == 0 and info["fallback_clusters"] == 0 and info["flipped_faces"] == 0
    assert np.array_equal(f, rotate(cluster.astype(np.int64)[faces]))      # every triple is a rotation of its input's
    assert np.abs(v.astype(np.float64)[cluster] - verts.astype(np.float64)).max() <= 2.0 ** -20 * cell


# ------------------------------------------------------------------------------------------ 8. a face budget
def test_simplify_to_faces_meets_the_budget(ops):
    sv, sf = uv_sphere()
    rgb = colours(len(sv))
    v, c, f, info = MS.simplify_to_faces(ops, sv, rgb, sf, 500)
    assert 0 < info["faces"] <= 500 and info["probes"] <= 16 and int(f.shape[0]) == info["faces"]
    print("target 500:", info["faces"], "faces at cell", info["cell"], "after", info["probes"], "probes")
    assert info["faces"] > 300      # (not just any cell that is coarse enough)
    v2, c2, f2, info2 = MS.simplify(ops, sv, rgb, sf, info["cell"])
    assert torch.equal(v, v2) and torch.equal(c, c2) and torch.equal(f, f2) and {k: info[k] for k in info2} == info2
    with pytest.raises(_lib.DmvsError, match="target_faces"):
        MS.simplify_to_faces(ops, sv, rgb, sf, -1)      # (no cell leaves fewer than no faces)


# ------------------------------------------------------------------------------------------ 9. files and wiring
def test_command_line_round_trip(ops, tmp_path, capsys):
    sv, sf = uv_sphere()
    rgb = colours(len(sv))
    src, out, out2 = (str(tmp_path / n) for n in ("in.ply", "out.ply", "budget.ply"))
    IO.write_ply(src, sv, rgb, faces=sf)
    res = MS.main(["--mesh", src, "--out", out, "--cell", "0.25", "--placement", "mean", "--reg", "0.001"], ops=ops)
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == {"mesh_simplify": res}
    want = run_simplify(ops, sv, rgb, sf, 0.25, placement="mean", reg=0.001)
    v, c, f = IO.read_ply_mesh(out)
    assert np.array_equal(bits(v), bits(want[0])) and np.array_equal(c, want[1]) and np.array_equal(f, want[2])
    assert res["ply"] == out and res["faces"] == 534 and res["faces_in"] == len(sf) and res["vertices_in"] == len(sv)
    res2 = MS.main(["--mesh", src, "--out", out2, "--target_faces", "500"], ops=ops)
    assert res2["faces"] <= 500 and res2["probes"] <= 16 and len(IO.read_ply_mesh(out2)[2]) == res2["faces"]
    with pytest.raises(SystemExit):
        MS.main(["--mesh", src, "--out", out], ops=ops)      # neither a cell nor a budget


def test_mesh_simplify_option_writes_what_simplify_makes_of_the_plain_mesh(ops, tmp_path):
    sys.path.insert(0, os.path.dirname(__file__))
    import fusion_scene
    root = fusion_scene.build_tree(str(tmp_path / "scan"), noise=0.02, outliers=0.02)
    plain, flagged = str(tmp_path / "plain.ply"), str(tmp_path / "flagged.ply")
    base = ["--outdir", root, "--testpath", root, "--dataset", "dtu", "--resolution", "24", "--trunc", "3", "--min_weight", "1"]
    a = M.main(base + ["--out", plain], ops=ops)[""]
    assert sorted(a) == ["bounds", "dims", "faces", "observed_voxels", "ply", "vertices", "views", "voxel"]      # the result line as it was
    verts, rgb, faces = IO.read_ply_mesh(plain)
    IO.write_ply(str(tmp_path / "rewritten.ply"), verts, rgb, faces=faces)                               # ... and the writer's bytes
    assert open(tmp_path / "rewritten.ply", "rb").read() == open(plain, "rb").read()
    b = M.main(base + ["--out", flagged, "--simplify", "2"], ops=ops)[""]
    v, c, f, info = MS.simplify(ops, verts, rgb, faces, 2.0 * a["voxel"], origin=a["bounds"][:3])
    IO.write_ply(str(tmp_path / "want.ply"), v.cpu().numpy(), c.cpu().numpy(), faces=f.cpu().numpy())
    assert open(flagged, "rb").read() == open(tmp_path / "want.ply", "rb").read()
    assert b["simplified"] == info and 0 < b["faces"] == info["faces"] < a["faces"] and b["vertices"] == info["vertices"] < a["vertices"]
    # after the cleaning, where both are asked for
    n = int(MC.component_table(ops, verts, faces, MC.components(ops, dev(ops, faces), len(verts))[0])["faces"].max())
    d = M.main(base + ["--out", flagged, "--min_component", str(n), "--simplify", "2"], ops=ops)[""]
    cv, cc, cf, _ = MC.clean(ops, verts, rgb, faces, min_faces=n)
    assert d["simplified"] == MS.simplify(ops, cv, cc, cf, 2.0 * a["voxel"], origin=a["bounds"][:3])[3] and d["cleaned"]["kept"] >= 1


# ------------------------------------------------------------------------------------------ 10. argument checks (CPU only)
def test_rejected_arguments_return_einval_before_any_launch():
    """the pointers are never dereferenced"""
    from diffmvs_amd.build import build_hip
    dll = _lib.Lib(build_hip()).dll
    p, odd, odd8 = C.c_void_p(4096), C.c_void_p(4098), C.c_void_p(4100)      # odd8: 4-byte but not 8-byte aligned
    o = (C.c_double * 3)(0.0, 0.0, 0.0)

    def verts(**kw):
        a = dict(verts=p, rgb=p, N=10, cluster=p, K=4, origin=o, cell=0.5, cnt=p, pos_q=p, rgb_sum=p, blocks=0)
        a.update(kw)
        return dll.dmvs_mesh_cluster_verts_i64(a["verts"], a["rgb"], a["N"], a["cluster"], a["K"], a["origin"], a["cell"], a["cnt"], a["pos_q"],
                                               a["rgb_sum"], a["blocks"], None)

    def quadrics(**kw):
        a = dict(verts=p, N=10, faces=p, F=5, cluster=p, K=4, origin=o, cell=0.5, scale=1024.0, cap=16.0, quad_q=p, state=p, blocks=0)
        a.update(kw)
        return dll.dmvs_mesh_cluster_quadrics_i64(a["verts"], a["N"], a["faces"], a["F"], a["cluster"], a["K"], a["origin"], a["cell"], a["scale"],
                                                  a["cap"], a["quad_q"], a["state"], a["blocks"], None)

    def place(**kw):
        a = dict(K=4, cnt=p, pos_q=p, rgb_sum=p, quad_q=p, cells=p, origin=o, cell=0.5, scale=1024.0, reg=2.0 ** -10, mode=0, out_verts=p, out_rgb=p,
                 state=p)
        a.update(kw)
        return dll.dmvs_mesh_cluster_place_f32(a["K"], a["cnt"], a["pos_q"], a["rgb_sum"], a["quad_q"], a["cells"], a["origin"], a["cell"], a["scale"],
                                               a["reg"], a["mode"], a["out_verts"], a["out_rgb"], a["state"], None)

    def remap(**kw):
        a = dict(verts=p, N=10, faces=p, F=5, cluster=p, K=4, new_verts=p, out_faces=p, keep=p, state=p, blocks=0)
        a.update(kw)
        return dll.dmvs_mesh_cluster_remap_i32(a["verts"], a["N"], a["faces"], a["F"], a["cluster"], a["K"], a["new_verts"], a["out_faces"], a["keep"],
                                               a["state"], a["blocks"], None)

    for fn in (verts, quadrics, place, remap):
        assert fn(K=-1) == -22 and fn(K=2 ** 31) == -22, fn.__name__
    for fn in (verts, quadrics, remap):
        assert fn(N=-1) == -22 and fn(N=2 ** 31) == -22 and fn(blocks=-1) == -22, fn.__name__
        assert fn(verts=odd) == -22 and fn(cluster=odd) == -22 and fn(cluster=None) == -22, fn.__name__
    for fn in (quadrics, remap):
        assert fn(F=-1) == -22 and fn(F=2 ** 31) == -22 and fn(faces=None) == -22 and fn(faces=odd) == -22 and fn(state=None) == -22, fn.__name__
        assert fn(state=odd8) == -22 and fn(state=None, F=0) == -22, fn.__name__      # the counters are always written
    for fn in (verts, quadrics, place):
        assert fn(origin=None) == -22 and fn(origin=(C.c_double * 3)(0.0, np.nan, 0.0)) == -22 and fn(origin=(C.c_double * 3)(np.inf, 0.0, 0.0)) == -22
        for cell in (0.0, -0.5, np.inf, np.nan):
            assert fn(cell=cell) == -22, (fn.__name__, cell)
    for fn in (quadrics, place):
        for scale in (0.0, -2.0, 3.0, 1000.0, np.inf, np.nan):
            assert fn(scale=scale) == -22, (fn.__name__, scale)
        assert fn(quad_q=None) == -22 and fn(quad_q=odd8) == -22, fn.__name__
    for name in ("verts", "cnt", "pos_q", "rgb_sum"):
        assert verts(**{name: None}) == -22, name
    assert verts(cnt=odd) == -22 and verts(pos_q=odd8) == -22 and verts(rgb_sum=odd8) == -22
    assert quadrics(verts=None) == -22
    assert quadrics(cap=-1.0) == -22 and quadrics(cap=np.nan) == -22 and quadrics(cap=np.inf) == -22 and quadrics(cap=2.0 ** 62) == -22
    assert quadrics(cap=2.0 ** 40, scale=2.0 ** 20) == -22      # 3 F cap scale >= 2^62: a sum could overflow
    for reg in (0.0, -1.0, np.inf, np.nan):
        assert place(reg=reg) == -22, reg
    assert place(mode=2) == -22 and place(mode=-1) == -22 and place(state=None) == -22 and place(state=odd8) == -22 and place(state=None, K=0) == -22
    for name in ("cnt", "pos_q", "cells", "out_verts"):
        assert place(**{name: None}) == -22, name
    assert place(rgb_sum=None) == -22 and place(out_rgb=None) == -22      # colours in and out go together
    assert place(cnt=odd) == -22 and place(out_verts=odd) == -22 and place(pos_q=odd8) == -22 and place(rgb_sum=odd8) == -22 and place(cells=odd8) == -22
    assert remap(out_faces=None) == -22 and remap(keep=None) == -22 and remap(out_faces=odd) == -22 and remap(new_verts=odd) == -22
    assert remap(verts=None) == -22      # the flip count needs the old positions
