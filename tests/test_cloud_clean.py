"""Cleaning of fused point clouds (diffmvs_amd.cloud_clean): dmvs_cloud_knn_f32 against a numpy brute-force restatement of its contract
written HERE, at tolerance zero -- the full [Q,M] matrix of fp32 squared distances in the kernel's operation order (numpy's elementwise
operations do not contract), the diagonal excluded in a self search, sorted; roots in fp64 summed in ascending order -- then the two
filters, the attributes, the files and the path through fusion and eval.  Nothing is compared with the code under test.  Every kernel
test runs on the host emulation in the CPU suite and on the GPU under -m gpu (the `ops` fixture)."""
import ctypes
import json
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, emu_ops, pin_ops
from diffmvs_amd import _lib, build as B, fusion, synth
from diffmvs_amd import cloud_clean as CC
from diffmvs_amd import cloud_grid as G
from diffmvs_amd import formats as IO

KS = [1, 7, 8, 9, 16, 17, 32]      # both sides of every template bound (8, 16, 32)
BLOCK = 256                        # DMVS_BLOCK


def dev(ops, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)


# ------------------------------------------------------------------------------------------ the contract, restated
def dist2_matrix(q, t):
    q, t = np.asarray(q, np.float32), np.asarray(t, np.float32)
    d = q[:, None, :] - t[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def brute(q, t, k, max_dist, self_search):
    """-> d2 [Q,k], found, kth, mean of include/dmvs.h, from all Q x M distances"""
    md = np.float32(max_dist)
    md2 = md * md
    with np.errstate(invalid="ignore", over="ignore"):
        d2 = dist2_matrix(q, t).reshape(len(q), len(t))
        if self_search:
            np.fill_diagonal(d2, np.inf)
        cand = d2 < md2                                              # (a NaN distance is no candidate)
    s = np.sort(np.where(cand, d2, np.float32(np.inf)), axis=1)
    s = np.concatenate([s, np.full((len(q), k), np.inf, np.float32)], 1)[:, :k]
    found = np.minimum(k, cand.sum(1)).astype(np.int32)
    live = np.arange(k)[None, :] < found[:, None]
    d2k = np.where(live, s, md2).astype(np.float32)
    kth = np.where(found == k, np.sqrt(d2k[:, k - 1]), md).astype(np.float32)
    S = np.zeros(len(q), np.float64)
    for j in range(k):                                               # ascending; adding 0.0 is exact
        S = S + np.where(live[:, j], np.sqrt(d2k[:, j].astype(np.float64)), 0.0)
    mean = np.where(found > 0, (S / np.maximum(found, 1).astype(np.float64)).astype(np.float32), md).astype(np.float32)
    return d2k, found, kth, mean


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_self(ops, pts, k, max_dist, cells):
    want = brute(pts, pts, k, max_dist, True)
    for cell in cells:
        r = CC.knn(ops, pts, k, max_dist, cell=cell, d2=True)
        got = [r[n].cpu().numpy() for n in ("d2", "found", "kth", "mean")]
        for name, g, w in zip(("d2", "found", "kth", "mean"), got, want):
            assert same_bits(g, w), (name, k, cell, np.argwhere(g != w)[:5])
    return want


# ------------------------------------------------------------------------------------------ 1. the kernel against brute force
_UNIT = np.random.default_rng(11).uniform(0.0, 1.0, (300, 3)).astype(np.float32)


@pytest.mark.parametrize("k", KS)
def test_random_cloud_equals_brute_force_at_two_cell_sizes(ops, k):
    """300 points of a unit cube, max_dist 0.3: with k = 32 part of the cloud finds fewer than k, with k = 1 everything is found"""
    _, found, _, _ = check_self(ops, _UNIT, k, 0.3, (0.05, 0.4))
    if k == 32:
        assert 0 < (found < k).sum() < len(found)
    if k == 1:
        assert (found == 1).all()


@pytest.mark.parametrize("k", [6, 8, 26])
def test_lattice_with_exact_ties_at_the_kth_place(ops, k):
    """an integer lattice 6x6x6: 6 neighbours at distance 1, 12 at sqrt 2, 8 at sqrt 3; k = 8 and 26 cut / end inside a shell of equal values"""
    g = np.stack(np.meshgrid(*[np.arange(6.0)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)
    check_self(ops, g, k, 2.5, (1.0, 0.7, 3.0))


def test_duplicates_are_neighbours_at_distance_zero(ops):
    """40 copies of one point and 5 others: d2 = 0 to the duplicates that are not the query itself, one cell holding more than k points"""
    rs = np.random.default_rng(5)
    pts = np.concatenate([np.tile(np.float32([[0.3, 0.4, 0.5]]), (40, 1)), rs.uniform(0, 1, (5, 3)).astype(np.float32)])
    for k in (8, 32):
        d2, found, _, mean = check_self(ops, pts, k, 2.0, (0.25, 1.0))
        assert (d2[:40, :min(k, 39)] == 0).all() and (found[:40] == k).all()
    assert (mean[:40] == 0).all() and (mean[40:] > 0).all()         # k = 32 of a copy's 39 twins; the others find the copies first


@pytest.mark.parametrize("n", [0, 1, 5])
def test_fewer_points_than_k(ops, n):
    pts = np.random.default_rng(n).uniform(0, 1, (n, 3)).astype(np.float32)
    d2, found, kth, mean = check_self(ops, pts, 8, 4.0, (0.5,))
    assert (found == max(0, n - 1)).all() and (kth == np.float32(4.0)).all() and (d2[:, max(0, n - 1):] == np.float32(16.0)).all()
    if n == 1:
        assert mean[0] == np.float32(4.0)


def test_a_point_farther_than_max_dist_finds_nothing(ops):
    pts = np.concatenate([_UNIT[:60], np.float32([[9.0, 9.0, 9.0]])])
    _, found, kth, mean = check_self(ops, pts, 4, 0.5, (0.1, 0.5))
    assert found[-1] == 0 and kth[-1] == mean[-1] == np.float32(0.5) and (found[:-1] > 0).all()


def test_more_than_one_workgroup_and_a_partial_last_one(ops):
    pts = np.random.default_rng(2).uniform(0, 1, (2 * BLOCK + 3, 3)).astype(np.float32)
    check_self(ops, pts, 8, 0.25, (0.1,))


def test_queries_that_are_not_the_target(ops):
    """self_index = NULL, a NaN and an infinite query, a query far outside the grid; and self_index given for some queries only"""
    rs = np.random.default_rng(3)
    t = rs.uniform(0, 1, (200, 3)).astype(np.float32)
    q = rs.uniform(-0.2, 1.2, (70, 3)).astype(np.float32)
    q[5, 1], q[6, 0], q[7] = np.nan, np.inf, (40.0, -3.0, 0.5)
    for cell in (0.08, 0.5):
        g = G.build_grid(dev(ops, t), cell)
        args = (g["target"], g["keys"], g["start"], g["origin"], g["cell"], g["dims"])
        ts = g["target"].cpu().numpy()
        for k in (3, 12):
            r = ops.cloud_knn(dev(ops, q), *args, 0.4, k, d2=True, work=True)
            for name, w in zip(("d2", "found", "kth", "mean"), brute(q, ts, k, 0.4, False)):
                assert same_bits(r[name].cpu().numpy(), w), (name, k, cell)
            assert r["found"][5] == r["found"][6] == r["found"][7] == 0
            wk = r["work"].cpu().numpy()
            assert (wk[5] == 0).all() and (wk[6] == 0).all() and (wk[r["found"].cpu().numpy() > 0] > 0).all()      # a non-finite query walks nothing
        # the sorted target as its own query: excluding position i for even i only
        me = np.where(np.arange(len(ts)) % 2 == 0, np.arange(len(ts)), -1).astype(np.int32)
        r = ops.cloud_knn(g["target"], *args, 0.4, 5, self_index=dev(ops, me), d2=True)
        with_self, without = brute(ts, ts, 5, 0.4, False), brute(ts, ts, 5, 0.4, True)
        for name, a, b in zip(("d2", "found", "kth", "mean"), with_self, without):
            assert same_bits(r[name].cpu().numpy(), np.where((me < 0).reshape([-1] + [1] * (a.ndim - 1)), a, b).astype(a.dtype)), name


def test_k1_without_self_exclusion_is_the_nearest_search(ops):
    rs = np.random.default_rng(4)
    t, q = rs.uniform(0, 1, (150, 3)).astype(np.float32), rs.uniform(0, 1, (90, 3)).astype(np.float32)
    g = G.build_grid(dev(ops, t), 0.1)
    args = (g["target"], g["keys"], g["start"], g["origin"], g["cell"], g["dims"])
    dist, index = ops.cloud_nn_index(dev(ops, q), *args, 0.12)
    r = ops.cloud_knn(dev(ops, q), *args, 0.12, 1)
    assert same_bits(r["kth"].cpu().numpy(), dist.cpu().numpy()) and same_bits(r["mean"].cpu().numpy(), dist.cpu().numpy())
    assert torch.equal(r["found"] == 1, index >= 0) and 0 < int((index < 0).sum()) < len(q)


# ------------------------------------------------------------------------------------------ 2. the entry point
def test_argument_checks_return_einval(ops):
    g = G.build_grid(dev(ops, _UNIT), 0.2)
    Q = len(_UNIT)
    out = {n: torch.full((Q,), 7, dtype=dt, device=ops.device) for n, dt in (("kth", torch.float32), ("mean", torch.float32), ("found", torch.int32))}
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(k, found=out["found"], max_dist=0.3, cell=0.2):
        return ops.lib.dll.dmvs_cloud_knn_f32(p(g["target"]), Q, p(g["target"]), Q, p(g["keys"]), p(g["start"]), g["keys"].numel(),
                                              (ctypes.c_double * 3)(*g["origin"]), cell, (ctypes.c_int32 * 3)(*g["dims"]), max_dist, None, k, None,
                                              p(out["kth"]), p(out["mean"]), p(found), None, ops.stream())
    assert _lib.CLOUD_MAX_K == 32
    assert call(0) == -22 and call(33) == -22 and call(-1) == -22 and call(8, found=None) == -22
    assert call(8, max_dist=float("nan")) == -22 and call(8, max_dist=0.0) == -22 and call(8, cell=0.0) == -22      # as the nearest searches
    if ops.device.type == "cuda":
        torch.cuda.synchronize()
    assert all(bool((t == 7).all()) for t in out.values())           # nothing was launched
    assert call(8) == 0 and call(32) == 0 and call(1) == 0
    with pytest.raises(_lib.DmvsError):
        ops.cloud_knn(g["target"], g["target"], g["keys"], g["start"], g["origin"], g["cell"], g["dims"], 0.3, 33)
    with pytest.raises(_lib.DmvsError):
        ops.cloud_knn(g["target"].double(), g["target"], g["keys"], g["start"], g["origin"], g["cell"], g["dims"], 0.3, 8)
    with pytest.raises(_lib.DmvsError):
        ops.cloud_knn(g["target"], g["target"], g["keys"], g["start"], g["origin"], g["cell"], g["dims"], 0.3, 8, self_index=torch.zeros(Q, dtype=torch.int64, device=ops.device))


# ------------------------------------------------------------------------------------------ 3. the two filters
_CLOUD500 = np.random.default_rng(21).uniform(0.0, 1.0, (500, 3)).astype(np.float32)
_CLOUD500[:12] *= np.float32(3.0)                                    # a few stragglers outside the cube


def restate_statistical(pts, k, std_ratio, max_dist):
    """the statistical filter of cloud_clean's docstring in Python integers -> (keep, mu, sd, threshold) in length units"""
    md = float(np.float32(max_dist))
    _, found, _, mean = brute(pts, pts, k, md, True)
    full = found == k
    e = 0
    while md * 2.0 ** (e + 1) <= 2.0 ** 30:
        e += 1
    while md * 2.0 ** e > 2.0 ** 30:
        e -= 1
    scale = 2.0 ** e
    q = [int(np.rint(np.float64(m) * scale)) for m in mean[full]]
    n, S1, S2 = len(q), sum(q), sum(v * v for v in q)
    mu, sd = S1 / n, math.sqrt(S2 * n - S1 * S1) / n
    bound = math.floor(mu + std_ratio * sd)
    keep = np.zeros(len(pts), bool)
    keep[np.nonzero(full)[0]] = np.array(q) <= bound
    return keep, full, mu / scale, sd / scale, bound / scale


def test_statistical_filter_equals_its_integer_restatement(ops):
    k, ratio, md = 8, 1.0, 0.6
    keep_w, full, mu, sd, thr = restate_statistical(_CLOUD500, k, ratio, md)
    assert 0 < (~full).sum() <= 12 and 0 < (full & ~keep_w).sum() < 250      # some isolated, some beyond the bound, most stay
    out = CC.clean(ops, _CLOUD500, knn=k, std_ratio=ratio, max_dist=md, cell=0.1)
    keep, info = out[3].cpu().numpy(), out[4]
    assert np.array_equal(keep, keep_w) and np.array_equal(out[0], _CLOUD500[keep_w])
    assert (info["mu"], info["sd"], info["threshold"]) == (mu, sd, thr) and info["max_dist"] == float(np.float32(md))
    assert info["removed"] == {"non_finite": 0, "isolated": int((~full).sum()), "statistical": int((full & ~keep_w).sum())}
    assert info["points"] == 500 and info["kept"] == int(keep_w.sum())
    # a permutation of the input, mapped back; a second cell size; the default cell
    perm = np.random.default_rng(0).permutation(500)
    o2 = CC.clean(ops, _CLOUD500[perm], knn=k, std_ratio=ratio, max_dist=md, cell=0.1)
    assert np.array_equal(o2[3].cpu().numpy(), keep_w[perm]) and {n: o2[4][n] for n in ("mu", "sd", "threshold")} == {n: info[n] for n in ("mu", "sd", "threshold")}
    for cell in (0.33, None):
        o3 = CC.clean(ops, _CLOUD500, knn=k, std_ratio=ratio, max_dist=md, cell=cell)
        assert np.array_equal(o3[3].cpu().numpy(), keep_w) and (o3[4]["mu"], o3[4]["sd"], o3[4]["threshold"]) == (mu, sd, thr)


def test_radius_filter_equals_the_brute_force_count(ops):
    n, r = 4, 0.15
    d2 = dist2_matrix(_CLOUD500, _CLOUD500)
    np.fill_diagonal(d2, np.inf)
    want = (d2 < np.float32(r) * np.float32(r)).sum(1) >= n
    assert 50 < want.sum() < 450
    for cell in (0.1, None):
        out = CC.clean(ops, _CLOUD500, min_neighbours=n, radius=r, cell=cell)
        assert np.array_equal(out[3].cpu().numpy(), want) and out[4]["removed"] == {"non_finite": 0, "radius": int((~want).sum())}


def plane_with_floaters():
    rng = np.random.default_rng(7)
    ij = np.stack(np.meshgrid(np.arange(40.), np.arange(40.), indexing="ij"), -1).reshape(1600, 2)
    xy = ij + rng.uniform(-.25, .25, (1600, 2))
    z = rng.uniform(-.05, .05, 1600)
    oxy = rng.uniform(0, 40, (80, 2))
    oz = rng.uniform(5, 40, 80)
    return np.concatenate([np.concatenate([xy, z[:, None]], 1), np.concatenate([oxy, oz[:, None]], 1)]).astype(np.float32)


def test_floaters_above_a_plane_go_and_the_plane_stays(ops):
    """1600 jittered lattice points in z = 0 and 80 points scattered 5 .. 40 above them.  A kd-tree run of the same rules on this scene
    (CPU) keeps 1600 / 1600 inliers and 0 / 80 outliers with knn = 8, std_ratio = 2, and 1575 inliers, 0 outliers with 4 neighbours
    inside 1.5."""
    pts = plane_with_floaters()
    keep = CC.clean(ops, pts, knn=8, std_ratio=2.0, max_dist=100.0)[3].cpu().numpy()
    print(f"statistical: {keep[:1600].sum()} / 1600 inliers, {keep[1600:].sum()} / 80 outliers stay")
    assert not keep[1600:].any() and keep[:1600].sum() >= 0.99 * 1600
    keep = CC.clean(ops, pts, min_neighbours=4, radius=1.5)[3].cpu().numpy()
    d2 = dist2_matrix(pts, pts)
    np.fill_diagonal(d2, np.inf)
    want = (d2 < np.float32(1.5) * np.float32(1.5)).sum(1) >= 4
    print(f"radius: {keep[:1600].sum()} / 1600 inliers, {keep[1600:].sum()} / 80 outliers stay")
    assert not keep[1600:].any() and np.array_equal(keep, want)


# ------------------------------------------------------------------------------------------ 4. attributes and files
def test_attributes_follow_and_stages_run_in_order(ops):
    rs = np.random.default_rng(9)
    pts = _CLOUD500.copy()
    pts[3, 1], pts[100, 2] = np.nan, np.inf
    pts[20:23] = np.float32([[5.0, 5.0, 5.0], [5.1, 5.0, 5.0], [5.0, 5.1, 5.0]])      # passes the radius filter, has too few neighbours for knn = 4
    rgb = rs.integers(0, 256, (500, 3)).astype(np.uint8)
    nrm = rs.normal(size=(500, 3)).astype(np.float32)
    xyz, c, m, keep, info = CC.clean(ops, pts, rgb, nrm, voxel=0.08, min_neighbours=2, radius=0.2, knn=4, std_ratio=1.5, max_dist=0.5)
    kp = keep.cpu().numpy()
    assert isinstance(xyz, np.ndarray) and same_bits(xyz, pts[kp]) and same_bits(c, rgb[kp]) and same_bits(m, nrm[kp]) and not kp[3] and not kp[100]
    assert list(info["removed"]) == ["non_finite", "voxel", "radius", "isolated", "statistical"] and info["removed"]["non_finite"] == 2
    assert all(v > 0 for v in info["removed"].values()) and info["kept"] == kp.sum() == 500 - sum(info["removed"].values())
    # each stage on the survivors of the one before
    s = np.isfinite(pts).all(1)
    idx = np.nonzero(s)[0][G.voxel_downsample(pts[s], 0.08)[1].numpy()]
    d2 = dist2_matrix(pts[idx], pts[idx])
    np.fill_diagonal(d2, np.inf)
    idx = idx[(d2 < np.float32(0.2) * np.float32(0.2)).sum(1) >= 2]
    idx = idx[restate_statistical(pts[idx], 4, 1.5, 0.5)[0]]
    assert np.array_equal(np.nonzero(kp)[0], idx)
    # tensors stay tensors; nothing asked for, nothing removed but the non-finite rows
    t = CC.clean(ops, dev(ops, pts), dev(ops, rgb))
    assert torch.is_tensor(t[0]) and torch.equal(t[0], dev(ops, pts[s])) and torch.equal(t[1], dev(ops, rgb[s])) and t[2] is None
    with pytest.raises(ValueError):
        CC.clean(ops, pts, min_neighbours=3)
    with pytest.raises(ValueError):
        CC.clean(ops, pts, knn=33)
    with pytest.raises(ValueError):
        CC.clean(ops, pts, rgb[:-1], knn=4)


def test_cli_round_trips_a_ply_with_normals(ops, tmp_path, capsys):
    pts = plane_with_floaters()
    rs = np.random.default_rng(1)
    rgb = rs.integers(0, 256, (len(pts), 3)).astype(np.uint8)
    nrm = rs.normal(size=(len(pts), 3)).astype(np.float32)
    src, dst, plain = (str(tmp_path / f) for f in ("in.ply", "out.ply", "plain.ply"))
    IO.write_ply(src, pts, rgb, nrm)
    res = CC.main(["--cloud", src, "--out", dst, "--knn", "8", "--std_ratio", "2", "--max_dist", "100", "--device", str(ops.device)])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
    keep = CC.clean(ops, pts, knn=8, std_ratio=2.0, max_dist=100.0)[3].cpu().numpy()
    x, c, m = IO.read_ply(dst, with_normals=True)
    assert same_bits(x, pts[keep]) and same_bits(c, rgb[keep]) and same_bits(m, nrm[keep])
    assert res["cloud_clean"]["kept"] == keep.sum() and res["cloud_clean"]["removed"]["statistical"] + res["cloud_clean"]["removed"]["isolated"] >= 80
    IO.write_ply(src, pts, rgb)                                       # without normals: none are written
    CC.main(["--cloud", src, "--out", plain, "--min_neighbours", "4", "--radius", "1.5", "--device", str(ops.device)])
    x, c, m = IO.read_ply(plain, with_normals=True)
    assert m is None and len(x) == len(c) < len(pts)


def test_filter_depth_cleans_the_cloud_it_writes(ops, tmp_path):
    sys.path.insert(0, os.path.dirname(__file__))
    import fusion_scene
    root = fusion_scene.build_tree(str(tmp_path / "scan"))
    kw = dict(geo_mask_thres=2, photo_thres=[0.3, 0.4, 0.5], method="casdiffmvs", dataset="dtu", ops=ops)
    masks = lambda: {f: open(os.path.join(root, "mask", f), "rb").read() for f in sorted(os.listdir(os.path.join(root, "mask")))}  # noqa: E731
    plain, tidy, again = (str(tmp_path / f) for f in ("plain.ply", "tidy.ply", "again.ply"))
    n0 = fusion.filter_depth(root, root, plain, normals=True, **kw)
    masks0 = masks()
    xyz, rgb, nrm = IO.read_ply(plain, with_normals=True)
    opts = dict(knn=6, std_ratio=1.0, min_neighbours=2, radius=4.0)
    want = CC.clean(ops, xyz, rgb, nrm, **opts)
    stats = {}
    n1 = fusion.filter_depth(root, root, tidy, normals=True, clean=opts, stats=stats, **kw)
    assert n1 == want[4]["kept"] and 0 < n1 < n0 == len(xyz) and stats["cloud_clean"] == want[4] and masks() == masks0
    got = IO.read_ply(tidy, with_normals=True)
    assert all(same_bits(g, w) for g, w in zip(got, want[:3]))
    assert fusion.filter_depth(root, root, again, normals=True, **kw) == n0 and open(again, "rb").read() == open(plain, "rb").read()


def test_eval_filter_with_and_without_the_cloud_options(tmp_path, monkeypatch, capsys):
    """without the new options eval --filter writes what fusion.filter_depth alone writes from the same tree; with them the cleaned cloud"""
    from PIL import Image
    from diffmvs_amd import eval as EV
    ops = emu_ops()
    pin_ops(monkeypatch, ops)
    root, H, W, V = tmp_path / "scene", 32, 64, 3
    sc = synth.synth_scene(H, W, n_views=V, n_src=V - 1, seed=2, grid_w=V)
    for d in ("images", "cams"):
        os.makedirs(root / d)
    with open(root / "pair.txt", "w") as f:
        f.write(f"{V}\n")
        for v in range(V):
            Image.fromarray((sc["images"][v].permute(1, 2, 0).numpy() * 255).astype("uint8")).save(str(root / "images" / f"{v:08d}.jpg"))
            cam = np.zeros((2, 4, 4), np.float32)
            cam[0], cam[1, :3, :3] = sc["E"][v].numpy(), sc["K"][v].numpy()
            IO.write_cam(str(root / "cams" / f"{v:08d}_cam.txt"), cam, 425.0, 935.0)
            f.write(f"{v}\n{V - 1} " + " ".join(f"{int(s)} 1.0" for s in sc["pairs"][v]) + "\n")
    base = ["--testpath", str(root), "--dataset", "general", "--method", "diffmvs", "--num_view", "2", "--numdepth_initial", "8", "--batch_size", "1",
            "--graphs", "0", "--noise_seed", "5", "--filter", "--geo_mask_thres", "1", "--geo_pixel_thres", "4", "--geo_depth_thres", "0.05",
            "--photo_thres", "0.0", "0.0", "0.0"]
    a = EV.main(base + ["--outdir", str(tmp_path / "a")], device=torch.device("cpu"))
    assert "cloud_clean" not in a
    kw = fusion.scene_protocol("general", "", str(tmp_path / "a"), 1, 4.0, 0.05, [0.0, 0.0, 0.0])
    direct = str(tmp_path / "direct.ply")
    kw["plyfilename"] = direct
    assert fusion.filter_depth(str(root), str(tmp_path / "a"), method="diffmvs", ops=ops, **kw) == a["fused_points"][""]
    assert open(a["ply"][""], "rb").read() == open(direct, "rb").read()
    b = EV.main(base + ["--outdir", str(tmp_path / "b"), "--cloud_knn", "6", "--cloud_std_ratio", "1.5", "--cloud_min_neighbours", "2", "--cloud_radius", "50",
                        "--cloud_voxel", "0.5"], device=torch.device("cpu"))
    xyz, rgb = IO.read_ply(a["ply"][""])
    want = CC.clean(ops, xyz, rgb, knn=6, std_ratio=1.5, min_neighbours=2, radius=50.0, voxel=0.5)
    got = IO.read_ply(b["ply"][""])
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1]) and b["cloud_clean"][""] == want[4] and b["fused_points"][""] == want[4]["kept"] > 0
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["cloud_clean"] == b["cloud_clean"] and "normals" not in b


# ------------------------------------------------------------------------------------------ 5. the list stays in registers
def test_no_instantiation_spills_its_list_to_scratch():
    """csrc/cloud_clean.hip alone through the compiler with the project's flags: the resource remarks of every cloud_knn instantiation
    report 0 bytes of scratch per lane (a run-time index into the list would put it there)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    err = subprocess.run([hipcc] + B.FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(B.CSRC, "cloud_clean.hip"), "-o", os.devnull],
                         capture_output=True, text=True, check=True, cwd=ROOT).stderr
    scratch = {}
    name = None
    for line in err.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name and "cloud_knn_kernel" in name:
            scratch[name] = int(m.group(1))
    assert len(scratch) == 3 and all("ILi%dE" % kb in " ".join(scratch) for kb in (8, 16, 32)), err[-2000:]
    assert all(v == 0 for v in scratch.values()), scratch
