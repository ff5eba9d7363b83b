"""Registration and cropping of point clouds (diffmvs_amd.cloud_register): dmvs_cloud_nn_index_f32, dmvs_cloud_pair_moments_f64 and
dmvs_cloud_crop_prism_f32 against fp64 numpy / scipy oracles written HERE (cKDTree, numpy.linalg.svd, matplotlib.path.Path), the closed
forms, ICP step by step and end to end against an fp64 restatement, and the path through cloud_eval.  Nothing is compared with the code
under test.  Every kernel test runs on the host emulation in the CPU suite and on the GPU under -m gpu (the `ops` fixture).

Bounds (derived, not tuned):
* fp32 distances: the kernel's operation order restated in numpy float32 -> bit equality.
* fixed-point sums: a term is rounded by at most 0.5 / scale, a sum of n terms by n * 0.5 / scale.
* a transform recovered from such sums: see `transform_tolerance`.
* ICP end to end: see test_icp_whole_run_against_the_fp64_restatement."""
import ctypes
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from diffmvs_amd import _lib
from diffmvs_amd import cloud_eval as CE
from diffmvs_amd import cloud_register as CR
from diffmvs_amd import formats as IO

cKDTree = pytest.importorskip("scipy.spatial").cKDTree
U24 = 2.0 ** -24
MAX_DIST = 20.0


def dev(ops, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)


def is_emu(ops):
    return ops.device.type == "cpu"


# ------------------------------------------------------------------------------------------ restatements of the kernels' arithmetic
def move_np(M, q):
    """fp32(((m0 x + m1 y) + m2 z) + m3) per row, fp64 products and sums in this order (numpy's elementwise operations do not contract)"""
    M = np.asarray(M, np.float64)
    x, y, z = (np.asarray(q[:, k], np.float64) for k in range(3))
    return np.stack([((M[r, 0] * x + M[r, 1] * y) + M[r, 2] * z) + M[r, 3] for r in range(3)], -1).astype(np.float32)


def dist_np(q, t):
    """the fp32 distance of the search: three differences, three squares, two sums, one root, each rounded to fp32"""
    d = q.astype(np.float32) - t.astype(np.float32)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(np.float32)


def rotation(axis, degrees):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = math.radians(degrees)
    return np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)


def similarity(R, t, s=1.0, about=(0, 0, 0)):
    """x -> s R (x - about) + about + t as a 4x4"""
    T, c = np.eye(4), np.asarray(about, np.float64)
    T[:3, :3] = s * R
    T[:3, 3] = c + np.asarray(t, np.float64) - s * R @ c
    return T


def surface(rs, n, offset=0.0):
    """the rippled surface of tests/test_cloud_eval.py (DTU-like coordinates, up to 10^3)"""
    x, y = rs.uniform(0, 1000, n), rs.uniform(0, 1000, n)
    z = 300 + 0.3 * x - 0.2 * y + 15 * np.sin(x / 40) * np.cos(y / 55)
    return (np.stack([x, y, z], -1) + offset).astype(np.float32)


_CASE = {}


def seeded_case():
    """2e4 targets on the surface, 2e4 queries on it with 0.5 noise, 500 of them displaced by up to 60 (test_cloud_eval.seeded_case's recipe)"""
    if not _CASE:
        rs = np.random.RandomState(20)
        target = surface(rs, 20000)
        query = surface(rs, 20000).astype(np.float64) + rs.normal(0, 0.5, (20000, 3))
        far = rs.choice(20000, 500, replace=False)
        v = rs.normal(size=(500, 3))
        query[far] += v / np.linalg.norm(v, axis=1, keepdims=True) * rs.uniform(0, 60, (500, 1))
        _CASE.update(query=query.astype(np.float32), target=target)
    return _CASE


def grid_args(g):
    return g["target"], g["keys"], g["start"], g["origin"], g["cell"], g["dims"]


def check_index_search(ops, q, t, max_dist, cell, transform=None, what=""):
    """the four properties of item 1 for one launch.  -> (dist, index) as numpy"""
    g = CE.build_grid(dev(ops, t), cell)
    qd = dev(ops, q)
    dist, index = ops.cloud_nn_index(qd, *grid_args(g), max_dist, transform=transform)
    dist, index = dist.cpu().numpy(), index.cpu().numpy()
    moved = q if transform is None else move_np(transform, q)
    ref = ops.cloud_nn_dist(dev(ops, moved), *grid_args(g), max_dist).cpu().numpy()
    assert dist.tobytes() == ref.tobytes(), f"{what}: dist differs from cloud_nn_dist"
    assert ops.cloud_nn_index(qd, *grid_args(g), max_dist, transform=transform, dist=False)[0] is None
    ts = g["target"].cpu().numpy()
    hit = index >= 0
    assert ((index == -1) == (dist == np.float32(max_dist))).all() and (index >= -1).all() and (index < max(1, len(ts))).all()
    assert dist_np(moved[hit], ts[index[hit]]).tobytes() == dist[hit].tobytes(), f"{what}: dist is not the distance to target[index]"
    if len(ts) >= 2 and len(q):
        d2, i2 = cKDTree(ts.astype(np.float64)).query(moved.astype(np.float64), k=2)
        decisive = (d2[:, 1] - d2[:, 0] > 8 * U24 * d2[:, 0]) & (np.abs(d2[:, 0] - max_dist) > 8 * U24 * max_dist)
        left_out = 1.0 - decisive.mean()
        print(f"{what}: {int((~decisive).sum())} of {len(q)} queries near-tied (left out), {int(hit.sum())} within max_dist")
        assert left_out <= 1e-3
        want = np.where(d2[:, 0] < max_dist, i2[:, 0], -1)
        assert (index[decisive] == want[decisive]).all(), f"{what}: index differs from cKDTree's at a decisive query"
    return dist, index


# ------------------------------------------------------------------------------------------ 1. index search
@pytest.mark.parametrize("cell", [1.25, 5.0, 20.0])
def test_index_search_matches_ckdtree_and_the_distance_kernel(ops, cell):
    c = seeded_case()
    n = 6000 if is_emu(ops) and cell == 20.0 else 20000          # (a 20-unit cell is brute force over ~8 points x 9 cells: keep the emulation quick)
    dist, index = check_index_search(ops, c["query"][:n], c["target"], MAX_DIST, cell, what=f"cell {cell}")
    assert (index == -1).sum() > 5 and (index >= 0).sum() > 0.9 * n


def test_index_search_edge_cases(ops):
    rs = np.random.RandomState(1)
    q = rs.uniform(-5, 5, (131, 3)).astype(np.float32)                      # not a multiple of 64
    dist, index = check_index_search(ops, q, np.zeros((0, 3), np.float32), 3.0, 1.0, what="empty target")
    assert (index == -1).all() and (dist == np.float32(3.0)).all()
    t1 = np.array([[0.25, -0.5, 1.0]], np.float32)
    for cell in (0.1, 3.0):
        dist, index = check_index_search(ops, q, t1, 6.0, cell, what=f"single target, cell {cell}")
        assert set(index.tolist()) <= {0, -1} and (index == 0).sum() > 10
        assert ((index == 0) == (dist_np(q, np.repeat(t1, len(q), 0)) < np.float32(6.0))).all()
    t = rs.uniform(-40, 40, (4099, 3)).astype(np.float32)                   # negative coordinates, duplicates of the queries
    q2 = np.concatenate([t[:500], rs.uniform(-45, 45, (801, 3)).astype(np.float32)])
    dist, index = check_index_search(ops, q2, t, 5.0, 2.0, what="negative coordinates")
    assert (dist[:500] == 0).all()
    d0, i0 = ops.cloud_nn_index(dev(ops, q[:0]), *grid_args(CE.build_grid(dev(ops, t), 2.0)), 5.0)
    assert d0.shape == (0,) and i0.shape == (0,) and i0.dtype == torch.int32


# ------------------------------------------------------------------------------------------ 2. the transform inside the kernel
def test_transform_in_the_kernel_is_the_fp64_product_rounded_once(ops):
    c = seeded_case()
    n = 5000 if is_emu(ops) else 20000
    M = similarity(rotation((0.3, -0.5, 0.8), 11.0), (7.0, -3.0, 2.5), s=1.07, about=(500, 500, 300))
    q0 = move_np(np.linalg.inv(M), c["query"][:n])                           # so that the moved queries land on the target again
    dist, index = check_index_search(ops, q0, c["target"], MAX_DIST, 5.0, transform=M, what="similarity")
    assert (index >= 0).mean() > 0.9
    g = CE.build_grid(dev(ops, c["target"]), 5.0)
    for form in (M[:3], torch.from_numpy(M)):                                # 3x4 and a 4x4 tensor are the same argument
        d2, i2 = ops.cloud_nn_index(dev(ops, q0), *grid_args(g), MAX_DIST, transform=form)
        assert d2.cpu().numpy().tobytes() == dist.tobytes() and (i2.cpu().numpy() == index).all()
    assert (CR.apply_transform(dev(ops, q0), M).cpu().numpy() == move_np(M, q0)).all()          # the host helper restates it too


# ------------------------------------------------------------------------------------------ 3. moments
def moments_np(src, M, tgt, index, valid, max_corr, cp, cq):
    """-> (19 sums as Python floats from long-double accumulation, counted mask)"""
    moved = src if M is None else move_np(M, src)
    ok = index >= 0
    if valid is not None:
        ok &= valid.astype(bool)
    j = np.where(ok, index, 0)
    ok &= dist_np(moved, tgt[j]) <= np.float32(max_corr)
    p = moved[ok].astype(np.longdouble) - np.asarray(cp, np.longdouble)
    t = tgt[index[ok]].astype(np.longdouble) - np.asarray(cq, np.longdouble)
    r = moved[ok].astype(np.longdouble) - tgt[index[ok]].astype(np.longdouble)
    sums = [float(ok.sum())] + list(p.sum(0)) + list(t.sum(0)) + list((p[:, :, None] * t[:, None, :]).sum(0).reshape(-1))
    sums += [(p * p).sum(), (t * t).sum(), (r * r).sum()]
    return [float(v) for v in sums], ok


def test_moments_are_exact_fixed_point_sums_independent_of_shape_and_order(ops):
    c = seeded_case()
    n = 6000 if is_emu(ops) else 20000
    rs = np.random.RandomState(31)
    M = similarity(rotation((1, 2, -1), 3.0), (0.4, -0.2, 0.3), about=(500, 500, 300))
    src = move_np(np.linalg.inv(M), c["query"][:n])                           # so that the moved source lands on the target
    g = CE.build_grid(dev(ops, c["target"]), 5.0)
    tgt = g["target"].cpu().numpy()
    index_t = ops.cloud_nn_index(dev(ops, src), *grid_args(g), MAX_DIST, transform=M, dist=False)[1]
    index = index_t.cpu().numpy()
    valid = (rs.uniform(size=n) < 0.8).astype(np.uint8)
    d_all = dist_np(move_np(M, src), tgt[np.maximum(index, 0)])
    at = np.flatnonzero((index >= 0) & (valid != 0) & (d_all > 0.5) & (d_all < 1.5))[0]
    max_corr = float(d_all[at])                                               # a pair EXACTLY at max_corr: it counts
    lo, hi = tgt.min(0).astype(np.float64), tgt.max(0).astype(np.float64)
    cp = cq = 0.5 * (lo + hi)
    bound = float((hi - lo).max()) * 0.5 + MAX_DIST
    s1, s2 = CR.moment_scales(n, bound, max_corr)
    assert n * bound * s1 < 2.0 ** 62 <= n * bound * 2 * s1 and math.log2(s2) == int(math.log2(s2))
    for vmask in (valid, None):
        for mc in (max_corr, MAX_DIST):
            want, ok = moments_np(src, M, tgt, index.copy(), vmask, mc, cp, cq)
            if vmask is not None and mc == max_corr:
                assert ok[at] and 0.02 * n < ok.sum() < 0.9 * n
            vt = None if vmask is None else dev(ops, vmask)
            runs = [ops.cloud_pair_moments(dev(ops, src), M, g["target"], index_t, vt, mc, cp, cq, bound, s1, s2, blocks=b).cpu().tolist() for b in (0, 1, 7, 0)]
            assert all(r == runs[0] for r in runs), "the sums depend on the launch shape or differ between two runs"
            got = runs[0]
            assert len(got) == _lib.CLOUD_MOMENTS and got[0] == int(want[0]) and got[19] == 0
            pairs = got[0]
            worst = 0.0
            for k in range(1, 19):
                scale = s1 if k < 7 else s2
                err = abs(got[k] / scale - want[k])
                worst = max(worst, err / (pairs * 0.5 / scale))
                assert err <= pairs * 0.5 / scale, (k, got[k] / scale, want[k])
            print(f"valid={'mask' if vmask is not None else 'all'} max_corr={mc:.4f}: {pairs} pairs, worst entry at {worst:.3f} of its bound, scales 2^{int(math.log2(s1))} / 2^{int(math.log2(s2))}")
            perm = rs.permutation(n)
            vp = None if vmask is None else dev(ops, vmask[perm])
            assert ops.cloud_pair_moments(dev(ops, src[perm]), M, g["target"], dev(ops, index[perm]), vp, mc, cp, cq, bound, s1, s2).cpu().tolist() == got
    # a pair beyond the coordinate bound is counted in out[19], never summed
    small = ops.cloud_pair_moments(dev(ops, src), M, g["target"], index_t, None, MAX_DIST, cp, cq, 100.0, s1, s2).cpu().tolist()
    assert small[19] > 0 and small[0] + small[19] == moments_np(src, M, tgt, index.copy(), None, MAX_DIST, cp, cq)[1].sum()
    assert ops.cloud_pair_moments(dev(ops, src[:0]), None, g["target"], index_t[:0], None, 1.0, cp, cq, bound, s1, s2).cpu().tolist() == [0] * 20


# ------------------------------------------------------------------------------------------ 4. closed forms
def umeyama_np(p, t, with_scale):
    """fp64 closed form on explicit pairs -> (4x4, singular values of the cross-covariance, variance of p)"""
    p, t = np.asarray(p, np.float64), np.asarray(t, np.float64)
    mp, mt = p.mean(0), t.mean(0)
    dp, dt = p - mp, t - mt
    U, D, Vt = np.linalg.svd(dt.T @ dp / len(p))
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1
    R = (U * S) @ Vt
    var = (dp * dp).sum() / len(p)
    s = (D * S).sum() / var if with_scale else 1.0
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = s * R, mt - s * R @ mp
    return T, D, var


def transform_tolerance(s1, s2, bound, D, var, scale, centroid_norm, with_scale, flipped=0, n=1):
    """how far a transform recovered from the fixed-point sums may lie from the fp64 closed form on the same pairs (+ `flipped` pairs that
    differ between the two pair sets).  -> (bound on the entries of sR, bound on the entries of t)

    Every sum of n terms is within n * 0.5 / scale of the exact sum, so after the division by n each mean is within e1 = 0.5 / s1 and each
    second moment within e2 = 0.5 / s2.  A covariance entry is cov = mean(p t) - mean(p) mean(t): its error is at most e2 + 2 B e1 (B bounds
    the centred coordinates), the Frobenius norm of the 3x3 error at most 3 times that.  A flipped pair changes a mean by at most 2 B / n
    and a second moment by at most 2 * 3 B^2 / n.  The rotation is the orthogonal polar factor of the covariance: first-order perturbation theory
    (Kenney & Laub 1991) gives |dR|_F <= 2 |dCov|_F / (sigma_2 + sigma_3) -- with the reflection guard the two smallest singular values that
    matter are D[1] and D[2] -- the scale c = tr(D S) / var moves by at most sqrt(3) |dCov|_F / var + c * dvar / var, and the translation
    t = mean_t - c R mean_p by the error of the means plus |d(cR)| times the centroid's norm.  A factor 4 covers the second-order terms and
    the fp64 rounding of two different SVD inputs."""
    e1, e2 = 0.5 / s1 + flipped * 2 * bound / n, 0.5 / s2 + flipped * 6 * bound * bound / n
    dcov = 3 * (e2 + 2 * bound * e1)
    dR = 2 * dcov / (D[1] + D[2])
    dc = (math.sqrt(3) * dcov / var + scale * (e2 * 3 + 2 * bound * e1 * 3) / var) if with_scale else 0.0
    dsR = 4 * (scale * dR + dc) + 1e-13
    return dsR, 4 * (2 * e1 + dsR * math.sqrt(3) * centroid_norm) + 1e-11


def exact_pairs(rs, n, T):
    p = (rs.uniform(-1, 1, (n, 3)) * np.array([300.0, 200.0, 80.0]) + np.array([500.0, 400.0, 600.0])).astype(np.float32)
    t = (p.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    return p, t


def moments_of_pairs(ops, p, t, with_centres=True):
    both = np.concatenate([p, t]).astype(np.float64)
    centre = 0.5 * (both.min(0) + both.max(0)) if with_centres else np.zeros(3)
    bound = float(np.abs(both - centre).max()) * 1.001
    s = CR.moment_scales(len(p), bound, 1e4)
    m = ops.cloud_pair_moments(dev(ops, p), None, dev(ops, t), torch.arange(len(p), dtype=torch.int32, device=ops.device), None, 1e4, centre, centre, bound, *s)
    return m.cpu().tolist(), s, centre, bound


@pytest.mark.parametrize("with_scale", [False, True])
def test_kabsch_recovers_the_closed_form_within_the_fixed_point_resolution(ops, with_scale):
    """exact correspondences target = fp32(s R p + t): kabsch() on the kernel's sums against numpy's closed form on the same pairs, within
    transform_tolerance (derivation there), and both close to the matrix that made the pairs (fp32 rounding of the targets only)"""
    rs = np.random.RandomState(41)
    n = 4000 if is_emu(ops) else 50000
    truth = similarity(rotation((0.2, 0.9, -0.4), 37.0), (12.0, -30.0, 7.0), s=1.13 if with_scale else 1.0, about=(500, 400, 600))
    p, t = exact_pairs(rs, n, truth)
    m, s, centre, bound = moments_of_pairs(ops, p, t)
    assert m[0] == n and m[19] == 0
    got = CR.kabsch(m, s, (centre, centre), with_scale=with_scale)
    want, D, var = umeyama_np(p, t, with_scale)
    scale = np.cbrt(np.linalg.det(want[:3, :3]))
    tol_R, tol_t = transform_tolerance(s[0], s[1], bound, D, var, scale, np.linalg.norm(p.astype(np.float64).mean(0)), with_scale)
    eR, et = np.abs(got[:3, :3] - want[:3, :3]).max(), np.abs(got[:3, 3] - want[:3, 3]).max()
    print(f"with_scale={with_scale}: |d sR| {eR:.3e} (bound {tol_R:.3e}), |d t| {et:.3e} (bound {tol_t:.3e}), scales 2^{int(math.log2(s[0]))} / 2^{int(math.log2(s[1]))}")
    assert eR <= tol_R and et <= tol_t and (got[3] == [0, 0, 0, 1]).all()
    assert np.abs(want - truth).max() < 1e-3                                   # the fp64 closed form itself finds the motion
    assert np.abs(CR.umeyama(p, t, with_scale=with_scale) - want).max() < 1e-9
    assert abs(np.linalg.det(got[:3, :3]) - scale ** 3) < 1e-6 * scale ** 3


def test_kabsch_mirrored_and_degenerate_input(ops):
    rs = np.random.RandomState(42)
    p = rs.uniform(-50, 50, (600, 3)).astype(np.float32)
    mirrored = (p * np.array([1, 1, -1], np.float32)).astype(np.float32)       # no rotation maps p onto its mirror image
    m, s, centre, _ = moments_of_pairs(ops, p, mirrored)
    T = CR.kabsch(m, s, (centre, centre))
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-9 and np.isfinite(T).all()
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-9
    assert abs(np.linalg.det(CR.umeyama(p, mirrored, with_scale=False)[:3, :3]) - 1.0) < 1e-9
    flat = p.copy()
    flat[:, 2] = 3.0                                                            # a planar configuration is NOT degenerate
    Tf = similarity(rotation((1, 1, 0), 20.0), (1, 2, 3))
    mf = moments_of_pairs(ops, flat, (flat.astype(np.float64) @ Tf[:3, :3].T + Tf[:3, 3]).astype(np.float32))
    assert np.abs(CR.kabsch(mf[0], mf[1], (mf[2], mf[2])) - Tf).max() < 1e-3
    line = (np.linspace(0, 1, 50)[:, None] * np.array([[3.0, 4.0, 5.0]])).astype(np.float32)
    ml = moments_of_pairs(ops, line, line)
    for bad in (lambda: CR.kabsch(ml[0], ml[1], (ml[2], ml[2])),                 # collinear
                lambda: CR.kabsch(moments_of_pairs(ops, p[:2], p[:2])[0], s, (centre, centre)),      # two pairs
                lambda: CR.kabsch([0] * 20, s, (centre, centre)),
                lambda: CR.umeyama(line, line), lambda: CR.umeyama(p[:2], p[:2]),
                lambda: CR.umeyama(np.repeat(p[:1], 9, 0), np.repeat(p[:1], 9, 0))):
        with pytest.raises(ValueError, match="pairs|degenerate"):
            bad()


# ------------------------------------------------------------------------------------------ 5. ICP
MOTIONS = [(2.0, (1.5, -1.0, 0.8), 5.0), (4.0, (3.0, -2.0, 1.5), 10.0), (8.0, (6.0, 5.0, -4.0), 20.0)]      # degrees, translation, max_corr
MAX_ITER = 80


def icp_scene(n_target, n_source, motion, scale=1.0):
    """item 5's scene -> (source fp32, target fp32, the true 4x4 source -> target)"""
    rs = np.random.RandomState(7)

    def z(x, y):
        return 30 * np.sin(x / 25) * np.cos(y / 30) + 8 * np.sin(x / 7 + y / 11) + 0.2 * x
    x, y = rs.uniform(0, 200, n_target), rs.uniform(0, 200, n_target)
    target = np.stack([x, y, z(x, y)], -1).astype(np.float32)
    x, y = rs.uniform(20, 180, n_source), rs.uniform(20, 180, n_source)
    s = np.stack([x, y, z(x, y)], -1) + rs.normal(0, 0.05, (n_source, 3))
    out = rs.choice(n_source, n_source // 50, replace=False)
    s[out] += rs.normal(0, 15, (len(out), 3))
    deg, tr, _ = motion
    truth = similarity(rotation((0.3, -0.5, 0.8), deg), tr, s=scale, about=(100, 100, 10))
    inv = np.linalg.inv(truth)
    return (s @ inv[:3, :3].T + inv[:3, 3]).astype(np.float32), target, truth


def scene_sizes(ops):
    return (40000, 4000) if is_emu(ops) else (150000, 12000)


class OracleICP:
    """the same algorithm in fp64 on a cKDTree; round32: the moved points are rounded to fp32 as the kernels' are"""

    def __init__(self, src, tgt, max_corr, round32):
        self.src, self.tgt, self.max_corr, self.round32 = src, tgt.astype(np.float64), float(max_corr), round32
        self.tree = cKDTree(self.tgt)

    def moved(self, T):
        return move_np(T, self.src).astype(np.float64) if self.round32 else self.src.astype(np.float64) @ T[:3, :3].T + T[:3, 3]

    def evaluate(self, T):
        m = self.moved(T)
        d, i = self.tree.query(m, k=2, workers=-1)
        ok = d[:, 0] <= self.max_corr
        return {"moved": m, "d": d, "i": i[:, 0], "ok": ok, "fitness": ok.mean(), "inlier_rmse": math.sqrt((d[ok, 0] ** 2).mean()) if ok.any() else 0.0}

    def update(self, ev, T, with_scale):
        return umeyama_np(ev["moved"][ev["ok"]], self.tgt[ev["i"][ev["ok"]]], with_scale)[0] @ T

    def run(self, with_scale=False, max_iter=MAX_ITER):
        T = np.eye(4)
        ev, it, converged, trail = self.evaluate(T), 0, False, [T]
        while it < max_iter:
            T = self.update(ev, T, with_scale)
            it += 1
            prev, ev = ev, self.evaluate(T)
            trail.append(T)
            if abs(prev["fitness"] - ev["fitness"]) < 1e-6 and abs(prev["inlier_rmse"] - ev["inlier_rmse"]) < 1e-6:
                converged = True
                break
        return {"T": T, "iterations": it, "converged": converged, "fitness": ev["fitness"], "inlier_rmse": ev["inlier_rmse"], "trail": trail, "last": ev}


def residual(T, truth, src):
    """RMS over the source points of |T x - truth x|"""
    s = src.astype(np.float64)
    return math.sqrt((((s @ T[:3, :3].T + T[:3, 3]) - (s @ truth[:3, :3].T + truth[:3, 3])) ** 2).sum(1).mean())


@pytest.mark.parametrize("case", [0, 1, 2])
def test_icp_one_step_against_the_fp64_restatement(ops, case):
    """from the same current transform (the oracle's after 0, 3 and its last update): the kernel's pairs are the oracle's except at
    near-ties (at most 0.1 %), and the next transform agrees within transform_tolerance with the differing pairs as `flipped`"""
    src, tgt, truth = icp_scene(*scene_sizes(ops), MOTIONS[case])
    max_corr = MOTIONS[case][2]
    oracle = OracleICP(src, tgt, max_corr, round32=True)
    run = oracle.run()
    assert run["converged"] and run["iterations"] < MAX_ITER
    g = CE.build_grid(dev(ops, tgt), 2.0)
    ts = g["target"].cpu().numpy()
    lo, hi = ts.min(0).astype(np.float64), ts.max(0).astype(np.float64)
    centre, bound = 0.5 * (lo + hi), float((hi - lo).max()) * 0.5 + max_corr * 1.001
    s = CR.moment_scales(len(src), bound, max_corr)
    o_sorted = OracleICP(src, ts, max_corr, round32=True)                    # (indices into the SORTED target, like the kernel's)
    for step in sorted({0, min(3, run["iterations"] - 1), run["iterations"] - 1}):
        T = run["trail"][step]
        ev = o_sorted.evaluate(T)
        index = ops.cloud_nn_index(dev(ops, src), *grid_args(g), max_corr, transform=T, dist=False)[1]
        m = ops.cloud_pair_moments(dev(ops, src), T, g["target"], index, None, max_corr, centre, centre, bound, *s).cpu().tolist()
        idx = index.cpu().numpy()
        want = np.where(ev["ok"], ev["i"], -1)
        differ = idx != want
        tied = (ev["d"][:, 1] - ev["d"][:, 0] <= 8 * U24 * ev["d"][:, 0]) | (np.abs(ev["d"][:, 0] - max_corr) <= 8 * U24 * max_corr)
        print(f"case {case} step {step}: {m[0]} pairs (oracle {int(ev['ok'].sum())}), {int(differ.sum())} differ, {int(tied.sum())} near-tied of {len(src)}")
        assert tied.mean() <= 1e-3 and not (differ & ~tied).any() and m[19] == 0
        got = CR.kabsch(m, s, (centre, centre)) @ T
        nxt = o_sorted.update(ev, T, False)
        ok = ev["ok"]
        _, D, var = umeyama_np(ev["moved"][ok], ts[ev["i"][ok]].astype(np.float64), False)
        tol_R, tol_t = transform_tolerance(s[0], s[1], bound, D, var, 1.0, np.linalg.norm(ev["moved"][ok].mean(0)), False,
                                           flipped=int(differ.sum()), n=int(ok.sum()))
        eR, et = np.abs(got[:3, :3] - nxt[:3, :3]).max(), np.abs(got[:3, 3] - nxt[:3, 3]).max()
        print(f"    next transform: |d R| {eR:.3e} (bound {tol_R:.3e}), |d t| {et:.3e} (bound {tol_t:.3e})")
        # the update is composed with T: the tolerance of the update carries over (|T| entries of the rotation part are <= 1, the
        # translation picks up |dR| times |t_T| which the centroid term of the bound already covers for this scene's 200-unit extent)
        assert eR <= tol_R and et <= tol_t + tol_R * math.sqrt(3) * np.linalg.norm(T[:3, 3])


@pytest.mark.parametrize("case", [0, 1, 2])
def test_icp_whole_run_against_the_fp64_restatement(ops, case):
    """The product and the fp64 oracle run the same algorithm from the identity with max_iter = 80; they differ only in arithmetic: the
    product rounds every moved coordinate to fp32 (one rounding, at most 2^-24 * 200 on this scene), takes fp32 distances and fixed-point
    sums.  So its RMS residual against the true motion may exceed the oracle's own residual (recomputed here) by at most
        margin = max(10 * 2^-24 * 200, 2 * |residual(oracle fp64) - residual(oracle with fp32-rounded moved points)|)
    -- ten roundings of a coordinate, or twice what that same rounding does to the oracle itself, whichever is larger.
    with_scale: the recovered scale deviates from 1 by at most the oracle's own deviation plus margin / 100 (a scale error ds moves the
    points of this 200-unit scene by up to 100 ds about its centre).  Two runs give bit-identical matrices.
    Measured, product = oracle to the printed digits in every case.  Emulation instance (40 000 x 4 000): 41 / 42 / 46 iterations, residual
    0.092812 / 0.089688 / 0.118418.  MI355X, full size (150 000 x 12 000): 40 / 44 / 36 iterations, residual 0.022392 / 0.039454 / 0.047931,
    near-tied share <= 8.3e-05, max |T64 - T32| <= 1e-7, margin 1.19e-4; with_scale 1.0298575 (oracle 1.0298575, truth 1.03) in 42."""
    src, tgt, truth = icp_scene(*scene_sizes(ops), MOTIONS[case])
    max_corr = MOTIONS[case][2]
    o64, o32 = OracleICP(src, tgt, max_corr, False).run(), OracleICP(src, tgt, max_corr, True).run()
    assert o64["converged"] and o32["converged"] and max(o64["iterations"], o32["iterations"]) < MAX_ITER
    r64, r32 = residual(o64["T"], truth, src), residual(o32["T"], truth, src)
    margin = max(10 * U24 * 200, 2 * abs(r64 - r32))
    d = o64["last"]["d"]
    print(f"case {case}: oracle fp64 {o64['iterations']} iterations, fitness {o64['fitness']:.6f}, rmse {o64['inlier_rmse']:.6f}, residual {r64:.6f}; "
          f"with fp32-rounded points {o32['iterations']} iterations, residual {r32:.6f}; near-tied share {float((d[:, 1] - d[:, 0] <= 8 * U24 * d[:, 0]).mean()):.2e}; "
          f"max |T64 - T32| {np.abs(o64['T'] - o32['T']).max():.2e}; margin {margin:.3e}")
    res = CR.icp(ops, src, tgt, max_corr=max_corr, max_iter=MAX_ITER)
    T = np.array(res["transformation"])
    r = residual(T, truth, src)
    print(f"    product: {res['iterations']} iterations, fitness {res['fitness']:.6f}, rmse {res['inlier_rmse']:.6f}, residual {r:.6f} (oracle {r64:.6f} + margin {margin:.3e})")
    assert res["converged"] and res["iterations"] < MAX_ITER and len(res["history"]) == res["iterations"] + 1
    assert res["fitness"] == res["pairs"] / len(src) and 0.9 < res["fitness"] <= 1.0
    assert r <= r64 + margin
    if case == 0:
        again = CR.icp(ops, src, tgt, max_corr=max_corr, max_iter=MAX_ITER)
        assert again["transformation"] == res["transformation"] and again["history"] == res["history"]
        cut = CR.icp(ops, src, tgt, max_corr=max_corr, max_iter=3)
        assert cut["iterations"] == 3 and not cut["converged"]
        # a similarity: the source shrunk by 3 % about the scene's centre on top of the motion
        src_s, _, truth_s = icp_scene(*scene_sizes(ops), MOTIONS[0], scale=1.03)
        os_ = OracleICP(src_s, tgt, max_corr, False).run(with_scale=True)
        os32 = OracleICP(src_s, tgt, max_corr, True).run(with_scale=True)
        assert os_["converged"] and os32["converged"]
        rs64, rs32 = residual(os_["T"], truth_s, src_s), residual(os32["T"], truth_s, src_s)
        margin_s = max(10 * U24 * 200, 2 * abs(rs64 - rs32))
        got = CR.icp(ops, src_s, tgt, max_corr=max_corr, max_iter=MAX_ITER, with_scale=True)
        Ts = np.array(got["transformation"])
        sc, sc_o = np.cbrt(np.linalg.det(Ts[:3, :3])), np.cbrt(np.linalg.det(os_["T"][:3, :3]))
        rs = residual(Ts, truth_s, src_s)
        print(f"    with_scale: product scale {sc:.7f} in {got['iterations']} iterations, residual {rs:.6f}; oracle scale {sc_o:.7f} in {os_['iterations']}, residual {rs64:.6f}; truth 1.03")
        assert got["converged"] and abs(sc / 1.03 - 1) <= abs(sc_o / 1.03 - 1) + margin_s / 100 and rs <= rs64 + margin_s
    with pytest.raises(ValueError, match="max_corr"):
        CR.icp(ops, src, tgt)


# ------------------------------------------------------------------------------------------ 6. crop
def star_polygon():
    """concave, 12 vertices: radii alternate between 40 and 17 about (5, -3)"""
    a = np.arange(12) * (2 * np.pi / 12) + 0.2
    r = np.where(np.arange(12) % 2 == 0, 40.0, 17.0)
    return np.stack([5 + r * np.cos(a), -3 + r * np.sin(a)], -1)


def crop_np(points, axis, lo, hi, poly):
    """the rule of include/dmvs.h, operation by operation, in fp64"""
    ui, vi = {0: (1, 2), 1: (0, 2), 2: (0, 1)}[axis]
    u, v, w = (points[:, k].astype(np.float64) for k in (ui, vi, axis))
    inside = np.zeros(len(points), bool)
    K = len(poly)
    with np.errstate(divide="ignore", invalid="ignore"):
        for i in range(K):
            j = (i - 1) % K
            cross = (poly[j, 0] - poly[i, 0]) * (v - poly[i, 1]) / (poly[j, 1] - poly[i, 1]) + poly[i, 0]
            inside ^= ((poly[i, 1] > v) != (poly[j, 1] > v)) & (u < cross)
    return inside & (w >= lo) & (w <= hi)


def edge_distance(uv, poly):
    d = np.full(len(uv), np.inf)
    for i in range(len(poly)):
        a, b = poly[i - 1], poly[i]
        t = np.clip(((uv - a) @ (b - a)) / ((b - a) @ (b - a)), 0, 1)
        d = np.minimum(d, np.linalg.norm(uv - (a + t[:, None] * (b - a)), axis=1))
    return d


@pytest.mark.parametrize("letter", ["X", "Y", "Z"])
def test_crop_matches_the_restated_rule_and_matplotlib(ops, letter):
    from matplotlib.path import Path
    rs = np.random.RandomState(51)
    poly = star_polygon()
    vol = CR.make_crop(letter, -7.5, 12.25, poly)
    axis = "XYZ".index(letter)
    ui, vi = {0: (1, 2), 1: (0, 2), 2: (0, 1)}[axis]
    n = 20011
    pts = np.empty((n, 3), np.float32)
    pts[:, ui], pts[:, vi], pts[:, axis] = rs.uniform(-45, 55, n), rs.uniform(-50, 45, n), rs.uniform(-12, 17, n)
    pts[:40, [ui, vi]] = poly[rs.randint(0, 12, 40)].astype(np.float32)            # points at (fp32-rounded) vertices
    pts[40:60, [ui, vi]] = np.float32(5.0), np.float32(-3.0)                       # inside, for the interval's ends:
    pts[40:50, axis], pts[50:60, axis] = np.float32(-7.5), np.float32(12.25)       # exactly at axis_min / axis_max -> inside
    pts[60:70, [ui, vi]], pts[60:70, axis] = (np.float32(5.0), np.float32(-3.0)), np.nextafter(np.float32(12.25), np.float32(100))
    got = CR.crop_mask(ops, pts, vol).cpu().numpy()
    assert got.dtype == np.uint8 and set(got.tolist()) <= {0, 1}
    want = crop_np(pts, axis, -7.5, 12.25, poly)
    assert (got.astype(bool) == want).all() and got[40:60].all() and not got[60:70].any() and 0.1 * n < want.sum() < 0.5 * n
    uv = pts[:, [ui, vi]].astype(np.float64)
    clear = edge_distance(uv, poly) > 1e-9 * 100
    mpl = Path(poly).contains_points(uv) & (pts[:, axis] >= -7.5) & (pts[:, axis] <= 12.25)
    print(f"axis {letter}: {int(want.sum())} of {n} inside, {int((~clear).sum())} within 1e-9 * extent of an edge")
    assert (got.astype(bool)[clear] == mpl[clear]).all() and clear.mean() > 0.99
    # the transform is applied first
    M = similarity(rotation((1, -2, 0.5), 25.0), (3.0, -4.0, 1.0), s=0.9)
    assert (CR.crop_mask(ops, pts, vol, transform=M).cpu().numpy().astype(bool) == crop_np(move_np(M, pts), axis, -7.5, 12.25, poly)).all()
    assert CR.crop_mask(ops, pts[:0], vol).shape == (0,)
    # bounding_polygon as 3-D points, infinite ends
    p3 = np.zeros((12, 3))
    p3[:, ui], p3[:, vi], p3[:, axis] = poly[:, 0], poly[:, 1], 99.0
    open_vol = CR.make_crop(axis, -math.inf, math.inf, p3)
    assert (CR.crop_mask(ops, pts, open_vol).cpu().numpy().astype(bool) == crop_np(pts, axis, -np.inf, np.inf, poly)).all()


def test_crop_refuses_too_many_vertices_and_readers_round_trip(ops, tmp_path):
    a = np.linspace(0, 2 * np.pi, 257, endpoint=False)
    big = np.stack([np.cos(a), np.sin(a)], -1)
    with pytest.raises(ValueError, match="vertices"):
        CR.make_crop("Z", 0, 1, big)
    pts = dev(ops, np.zeros((5, 3), np.float32))
    with pytest.raises(_lib.DmvsError, match="vertices"):
        ops.cloud_crop_prism(pts, dev(ops, big), 2, 0.0, 1.0)
    rc = ops.lib.dll.dmvs_cloud_crop_prism_f32(ctypes.c_void_p(pts.data_ptr()), 5, None, ctypes.c_void_p(dev(ops, big).data_ptr()), 257, 2, 0.0, 1.0,
                                               ctypes.c_void_p(pts.data_ptr()), None)
    assert rc == -22
    assert ops.cloud_crop_prism(pts, dev(ops, big[:256]), 2, 0.0, 1.0).cpu().tolist() == [1] * 5      # the maximum itself is served
    # the files of a Tanks&Temples scene
    poly = star_polygon()
    p3 = np.stack([poly[:, 0], np.full(12, 1.5), poly[:, 1]], -1)
    (tmp_path / "crop.json").write_text(json.dumps({"axis_max": 4.25, "axis_min": -1.5, "bounding_polygon": p3.tolist(), "class_name": "SelectionPolygonVolume",
                                                     "orthogonal_axis": "Y", "version_major": 1, "version_minor": 0}))
    vol = CR.load_crop_json(str(tmp_path / "crop.json"))
    assert vol["axis"] == 1 and vol["axis_min"] == -1.5 and vol["axis_max"] == 4.25 and (vol["polygon"] == poly).all()
    T = similarity(rotation((0.1, 0.2, 0.3), 123.0), (1e3, -2.5e-7, 1 / 3), s=math.pi)
    CR.save_transform(str(tmp_path / "T.txt"), T)
    assert (CR.load_transform(str(tmp_path / "T.txt")) == T).all()               # repr round-trips a double
    (tmp_path / "bad.txt").write_text("1 2 3\n")
    with pytest.raises(ValueError, match="4x4"):
        CR.load_transform(str(tmp_path / "bad.txt"))
    T2 = similarity(rotation((1, 0, 0), 10.0), (4, 5, 6))
    with open(tmp_path / "traj.log", "w") as f:
        for k, m in enumerate((T, T2)):
            f.write(f"{k} {k} {k + 1}\n" + "".join(" ".join(repr(float(v)) for v in row) + "\n" for row in m))
    log = CR.load_trajectory_log(str(tmp_path / "traj.log"))
    assert [b[0] for b in log] == [[0, 0, 1], [1, 1, 2]] and (log[0][1] == T).all() and (log[1][1] == T2).all()
    # corresponding camera centres give the initial guess
    centres = np.random.RandomState(3).uniform(-5, 5, (9, 3))
    assert np.abs(CR.umeyama(centres, centres @ T[:3, :3].T + T[:3, 3]) - T).max() < 1e-9


# ------------------------------------------------------------------------------------------ 7. through cloud_eval
EPS = 4.0 * U24
THRESHOLDS = [0.5, 1.0, 2.0, 20.0]


def nn_fp64(query, target, max_dist):
    """min(|q - nearest target|, max_dist) in fp64 (cKDTree on float64 copies)"""
    if len(target) == 0:
        return np.full(len(query), float(max_dist))
    return np.minimum(cKDTree(np.asarray(target, np.float64)).query(np.asarray(query, np.float64), workers=-1)[0], max_dist)


def metrics_fp64(d_pred, d_gt, max_dist, thresholds, valid_p=None, valid_g=None):
    out = {}
    for name, d, v in (("pred", d_pred, valid_p), ("gt", d_gt, valid_g)):
        d = d if v is None else d[v.astype(bool)]
        inr = d < max_dist
        out[name] = {"valid": int(len(d)), "in_range": int(inr.sum()), "mean": float(d[inr].mean()), "below": [int((d < t).sum()) for t in thresholds]}
    P = [b / out["pred"]["valid"] for b in out["pred"]["below"]]
    R = [b / out["gt"]["valid"] for b in out["gt"]["below"]]
    out.update(accuracy=out["pred"]["mean"], completeness=out["gt"]["mean"], precision=P, recall=R,
               fscore=[2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(P, R)])
    return out


def test_evaluate_without_the_new_arguments_is_unchanged(ops):
    """the bounds of tests/test_cloud_eval.py: counters exact (the seeded input keeps every distance away from the thresholds), means within
    4 * 2^-24 relative plus the fixed point's half unit"""
    c = seeded_case()
    n = 6000 if is_emu(ops) else 20000
    q, t = c["query"][:n], c["target"]
    want = metrics_fp64(nn_fp64(q, t, MAX_DIST), nn_fp64(t, q, MAX_DIST), MAX_DIST, THRESHOLDS)
    res = CE.evaluate(ops, q, t, MAX_DIST, THRESHOLDS)
    assert "transformation" not in res and "registration" not in res
    for side, key in (("pred", "accuracy"), ("gt", "completeness")):
        s, w = res[side], want[side]
        assert (s["valid"], s["in_range"], s["below"]) == (w["valid"], w["in_range"], w["below"])
        assert abs(res[key] - w["mean"]) <= EPS * w["mean"] + 0.5 / s["scale"]
    assert res["precision"] == want["precision"] and res["recall"] == want["recall"] and res["fscore"] == want["fscore"]
    ident = CE.evaluate(ops, q, t, MAX_DIST, THRESHOLDS, transform=np.eye(4))
    assert ident.pop("transformation") == np.eye(4).tolist() and json.dumps(ident) == json.dumps(res)


def registered_scores_check(res, plain, pred_displaced, pred, gt, max_corr, max_dist, thresholds, what):
    """item 7: the scores after registration differ from those of the undisplaced prediction by no more than the fp64 scipy pipeline
    (same ICP, same scoring) differs on the same inputs, plus the margin of the whole-run test.  For the mean distances the margin is a
    length; for the counted shares a point can change sides of a threshold only if its distance moves across it, so the margin there is
    the share of points whose fp64 distance lies within `margin` of the threshold (both clouds), on top of the oracle's own change."""
    o64, o32 = OracleICP(pred_displaced, gt, max_corr, False).run(), OracleICP(pred_displaced, gt, max_corr, True).run()
    assert o64["converged"] and o32["converged"]
    moved64 = pred_displaced.astype(np.float64) @ o64["T"][:3, :3].T + o64["T"][:3, 3]
    moved32 = move_np(o32["T"], pred_displaced).astype(np.float64)
    rms = math.sqrt(((moved64 - moved32) ** 2).sum(1).mean())
    margin = max(10 * U24 * 200, 2 * rms)
    ref = metrics_fp64(nn_fp64(pred, gt, max_dist), nn_fp64(gt, pred, max_dist), max_dist, thresholds)
    d_pg, d_gp = nn_fp64(moved64, gt, max_dist), nn_fp64(gt, moved64, max_dist)
    orc = metrics_fp64(d_pg, d_gp, max_dist, thresholds)
    for key in ("accuracy", "completeness"):
        print(f"{what} {key}: registered {res[key]:.6f}, undisplaced {plain[key]:.6f}; oracle registered {orc[key]:.6f}, undisplaced {ref[key]:.6f}; margin {margin:.2e}")
        assert abs(res[key] - plain[key]) <= abs(orc[key] - ref[key]) + margin + EPS * ref[key]
    for i, t in enumerate(thresholds):
        band = float((np.abs(d_pg - t) <= margin).mean() + (np.abs(d_gp - t) <= margin).mean())
        print(f"{what} fscore@{t}: registered {res['fscore'][i]:.6f}, undisplaced {plain['fscore'][i]:.6f}; oracle {orc['fscore'][i]:.6f} / {ref['fscore'][i]:.6f}; band {band:.2e}")
        assert abs(res["fscore"][i] - plain["fscore"][i]) <= abs(orc["fscore"][i] - ref["fscore"][i]) + 2 * band + 1e-12
    return orc


def test_evaluate_with_register_and_crop(ops):
    pred_displaced, gt, truth = icp_scene(*scene_sizes(ops), MOTIONS[0])
    pred = move_np(truth, pred_displaced)                                         # the prediction where it belongs
    max_corr, max_dist, thr = MOTIONS[0][2], 5.0, [0.1, 0.5, 2.0]
    plain = CE.evaluate(ops, pred, gt, max_dist, thr)
    reg = {"schedule": [(None, max_corr, MAX_ITER)]}
    res = CE.evaluate(ops, pred_displaced, gt, max_dist, thr, register=reg)
    assert res["registration"]["converged"] and res["transformation"] == res["registration"]["transformation"]
    registered_scores_check(res, plain, pred_displaced, pred, gt, max_corr, max_dist, thr, "icp scene")
    # a known transform alone: the prediction is moved exactly as move_np moves it
    moved = CE.evaluate(ops, pred_displaced, gt, max_dist, thr, transform=truth)
    want = CE.evaluate(ops, move_np(truth, pred_displaced), gt, max_dist, thr)
    moved.pop("transformation")
    assert json.dumps(moved) == json.dumps(want)
    # crop: the counters are the numpy mask's sums, the scores those of the masked clouds
    ring = np.stack([100 + 70 * np.cos(np.arange(7) * 0.9), 95 + np.array([60, 75, 50, 80, 55, 70, 65]) * np.sin(np.arange(7) * 0.9)], -1)
    vol = CR.make_crop("Z", -10.0, 35.0, ring)
    mp, mg = crop_np(pred, 2, -10.0, 35.0, ring), crop_np(gt, 2, -10.0, 35.0, ring)
    assert 0.1 < mp.mean() < 0.9 and 0.1 < mg.mean() < 0.9      # the volume cuts both clouds
    cropped = CE.evaluate(ops, pred_displaced, gt, max_dist, thr, transform=truth, crop=vol)
    assert cropped["pred"]["valid"] == int(mp.sum()) and cropped["gt"]["valid"] == int(mg.sum()) and cropped["pred"]["points"] == len(pred)
    w = metrics_fp64(nn_fp64(pred, gt, max_dist), nn_fp64(gt, pred, max_dist), max_dist, thr, mp, mg)
    for side in ("pred", "gt"):
        assert abs(cropped[side]["in_range"] - w[side]["in_range"]) <= 2 and abs(cropped[side]["mean"] - w[side]["mean"]) <= 1e-4 * w[side]["mean"] + 1e-6
    # register() in stages, only the source points inside the volume taking part
    staged = CR.register(ops, pred_displaced, gt, schedule=[(2.0, 2 * max_corr, 30), (None, max_corr, MAX_ITER)], crop=vol)
    assert [s["voxel"] for s in staged["stages"]] == [2.0, None] and staged["stages"][1]["source_points"] < len(pred) * 0.95
    # ... which is icp() stage by stage on the thinned clouds, the source cut by the numpy restatement of the volume at the stage's start
    T = np.eye(4)
    for voxel, corr, iters in [(2.0, 2 * max_corr, 30), (None, max_corr, MAX_ITER)]:
        s_pts = pred_displaced if voxel is None else CE.voxel_downsample(pred_displaced, voxel)[0].numpy()
        t_pts = gt if voxel is None else CE.voxel_downsample(gt, voxel)[0].numpy()
        s_pts = s_pts[crop_np(move_np(T, s_pts), 2, -10.0, 35.0, ring)]
        T = np.array(CR.icp(ops, s_pts, t_pts, init=T, max_corr=corr, max_iter=iters)["transformation"])
    assert staged["transformation"] == T.tolist() and staged["stages"][1]["source_points"] == len(s_pts)
    r_staged, r_start = residual(T, truth, pred_displaced), residual(np.eye(4), truth, pred_displaced)
    print(f"register(): two stages with crop, residual {r_staged:.5f} (identity start {r_start:.5f})")
    assert r_staged < r_start
    assert CR.tanks_schedule(0.01) == [(0.01, 0.8, 20), (0.005, 0.2, 20), (None, 0.02, 20)]
    with pytest.raises(ValueError, match="schedule"):
        CR.register(ops, pred, gt, schedule=[])


# ------------------------------------------------------------------------------------------ 8. entry-point validation (no device), end to end on the GPU
def test_invalid_arguments_are_rejected_before_any_launch():
    """every DMVS_EINVAL case of the three entry points returns -22; the device pointers below are never dereferenced"""
    from diffmvs_amd.build import build_hip
    lib = _lib.Lib(build_hip())
    p = ctypes.c_void_p(4096)
    D3, I3, D12 = ctypes.c_double * 3, ctypes.c_int32 * 3, ctypes.c_double * 12
    origin, dims, ident = D3(0.0, 0.0, 0.0), I3(8, 8, 8), D12(1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)

    def nn(query=p, Q=10, target=p, M=10, keys=p, start=p, C=5, origin=origin, h=1.0, dims=dims, max_dist=2.0, transform=ident, dist=p, index=p):
        return lib.dll.dmvs_cloud_nn_index_f32(query, Q, target, M, keys, start, C, origin, h, dims, max_dist, transform, dist, index, None, None)

    nan12 = D12(1, 0, 0, 0, 0, float("nan"), 0, 0, 0, 0, 1, 0)
    for kw in (dict(query=None), dict(index=None), dict(target=None), dict(keys=None), dict(start=None), dict(origin=None), dict(dims=None),
               dict(Q=-1), dict(M=-1), dict(C=-1), dict(C=11), dict(C=0), dict(M=0, C=5), dict(M=1 << 31, C=5),
               dict(h=0.0), dict(h=float("nan")), dict(max_dist=0.0), dict(max_dist=float("inf")), dict(dims=I3(8, 0, 8)),
               dict(h=1.0e-3, max_dist=2.0), dict(dims=I3(1 << 21, 1 << 21, 1 << 21)), dict(transform=nan12),
               dict(transform=D12(*([float("inf")] + [0] * 11)))):
        assert nn(**kw) == -22, kw
    assert nn(Q=0) == 0 and nn(Q=0, dist=None, transform=None) == 0 and nn(Q=0, M=0, C=0, target=None, keys=None, start=None) == 0

    def mom(source=p, N=1000, transform=None, target=p, M=1000, index=p, valid=None, max_corr=5.0, cp=origin, cq=origin, bound=100.0, s1=2.0 ** 30,
            s2=2.0 ** 20, blocks=0, out=p):
        return lib.dll.dmvs_cloud_pair_moments_f64(source, N, transform, target, M, index, valid, max_corr, cp, cq, bound, s1, s2, blocks, out, None)

    for kw in (dict(source=None), dict(index=None), dict(target=None), dict(out=None), dict(cp=None), dict(cq=None), dict(N=-1), dict(M=-1), dict(M=1 << 31),
               dict(blocks=-1), dict(max_corr=0.0), dict(max_corr=float("nan")), dict(max_corr=float("inf")), dict(bound=0.0), dict(bound=float("inf")),
               dict(cp=D3(0.0, float("nan"), 0.0)), dict(cq=D3(float("inf"), 0.0, 0.0)), dict(transform=nan12),
               dict(s1=3.0), dict(s2=3.0), dict(s1=0.0), dict(s2=-4.0), dict(s1=float("inf")), dict(s2=float("nan")),
               dict(s1=2.0 ** 46),                                                  # 1000 * 100 * 2^46 >= 2^62
               dict(s2=2.0 ** 38),                                                  # 1000 * 3 * 100^2 * 2^38 >= 2^62
               dict(max_corr=1.0e4, s2=2.0 ** 26)):                                 # 1000 * (1.001e4)^2 * 2^26 >= 2^62
        assert mom(**kw) == -22, kw
    assert mom(s1=2.0 ** -3, s2=2.0 ** -8, N=-1) == -22                       # (fractional powers of two are scales too)

    def crop(points=p, N=100, transform=None, polygon=p, K=12, axis=1, lo=-1.0, hi=1.0, inside=p):
        return lib.dll.dmvs_cloud_crop_prism_f32(points, N, transform, polygon, K, axis, lo, hi, inside, None)

    for kw in (dict(points=None), dict(inside=None), dict(polygon=None), dict(N=-1), dict(K=2), dict(K=257), dict(K=-1), dict(axis=3), dict(axis=-1),
               dict(lo=1.0, hi=-1.0), dict(lo=float("nan")), dict(hi=float("nan")), dict(transform=nan12)):
        assert crop(**kw) == -22, kw
    assert crop(N=0) == 0 and crop(N=0, points=None, inside=None, K=256, lo=-math.inf, hi=math.inf) == 0
    from conftest import emu_ops
    with pytest.raises(_lib.DmvsError, match="contiguous"):
        emu_ops().cloud_crop_prism(torch.zeros(4, 3), torch.zeros(5, 2), 0, 0.0, 1.0)          # the polygon is fp64
    with pytest.raises(_lib.DmvsError, match="3x4"):
        emu_ops().cloud_crop_prism(torch.zeros(4, 3), torch.zeros(5, 2, dtype=torch.float64), 0, 0.0, 1.0, transform=np.eye(3))
    with pytest.raises(_lib.DmvsError, match="one entry per source point"):
        emu_ops().cloud_pair_moments(torch.zeros(4, 3), None, torch.zeros(4, 3), torch.zeros(3, dtype=torch.int32), None, 1.0, (0, 0, 0), (0, 0, 0), 1.0, 1.0, 1.0)


@pytest.mark.gpu
def test_fused_scene_registers_and_scores_through_the_command_lines(tmp_path):
    """tests/fusion_scene.py's tree fused on the GPU, a displaced copy registered back by both command lines (child processes, each under
    its own time limit): the JSON lines are those of the in-process calls and obey item 7's bounds"""
    from conftest import hip_ops
    from test_cloud_eval import fused_scene
    ops = hip_ops()
    ply, gt = fused_scene(tmp_path, ops, 0.06)
    pred, colour = IO.read_ply(ply)
    centre = 0.5 * (gt.min(0) + gt.max(0)).astype(np.float64)
    extent = float((gt.max(0) - gt.min(0)).max())
    truth = similarity(rotation((0.3, -0.5, 0.8), 1.5), np.array([0.01, -0.008, 0.006]) * extent, about=centre)
    displaced = move_np(np.linalg.inv(truth), pred)
    IO.write_ply(str(tmp_path / "displaced.ply"), displaced, colour)
    IO.write_ply(str(tmp_path / "gt.ply"), gt, np.zeros((len(gt), 3), np.uint8))
    max_corr, max_dist, thr = 0.04 * extent, MAX_DIST, [1.0, 2.0, 5.0]
    cli = subprocess.run([sys.executable, "-m", "diffmvs_amd.cloud_register", "--pred", str(tmp_path / "displaced.ply"), "--gt", str(tmp_path / "gt.ply"),
                          "--max_corr", repr(max_corr), "--max_iter", str(MAX_ITER), "--out_transform", str(tmp_path / "T.txt"), "--out_ply", str(tmp_path / "aligned.ply")],
                         cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert cli.returncode == 0, cli.stderr[-2000:]
    line = json.loads(cli.stdout.strip().splitlines()[-1])
    here = CR.register(ops, displaced, gt, schedule=[(None, max_corr, MAX_ITER)])
    assert line == json.loads(json.dumps(here)) and line["converged"]
    T = CR.load_transform(str(tmp_path / "T.txt"))
    assert (T == np.array(here["transformation"])).all()
    assert (IO.read_ply(str(tmp_path / "aligned.ply"))[0] == move_np(T, displaced)).all()
    orc = OracleICP(displaced, gt, max_corr, False).run()
    r, r_o = residual(T, truth, displaced), residual(orc["T"], truth, displaced)
    print(f"fused scene ({len(pred)} x {len(gt)} points, extent {extent:.1f}): product residual {r:.6f} in {line['iterations']} iterations, oracle {r_o:.6f} in {orc['iterations']}")
    cli2 = subprocess.run([sys.executable, "-m", "diffmvs_amd.cloud_eval", "--pred", str(tmp_path / "displaced.ply"), "--gt", str(tmp_path / "gt.ply"), "--max_dist", "20",
                           "--thresholds", "1", "2", "5", "--register", repr(max_corr), "--register_max_iter", str(MAX_ITER)],
                          cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert cli2.returncode == 0, cli2.stderr[-2000:]
    res = json.loads(cli2.stdout.strip().splitlines()[-1])
    assert res["transformation"] == line["transformation"]
    plain = CE.evaluate(ops, pred, gt, max_dist, thr)
    registered_scores_check(res, plain, displaced, pred, gt, max_corr, max_dist, thr, "fused scene")
