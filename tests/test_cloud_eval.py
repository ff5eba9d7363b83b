"""Point-cloud scoring (diffmvs_amd.cloud_eval): the nearest-neighbour kernel (dmvs_cloud_nn_dist_f32) and the statistics kernel
(dmvs_cloud_stats_f32) against a brute-force fp64 nearest neighbour written here, the metrics built on them, read_ply, the voxel
thinning, the region of interest, and a fused synthetic scene end to end on the GPU.

The per-point bound |d - d_oracle| <= 4 * 2^-24 * d_oracle is derived, not tuned: three fp32 subtractions of one rounding each, three
products and two additions of non-negative terms, the error halved by the square root plus one rounding for the root: at most
3.5 * 2^-24 relative."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from diffmvs_amd import _lib
from diffmvs_amd import cloud_eval as CE
from diffmvs_amd import formats as IO

EPS = 4.0 * 2.0 ** -24
MAX_DIST = 20.0
THRESHOLDS = [0.5, 1.0, 2.0, 20.0]


# ------------------------------------------------------------------------------------------ the oracle (fp64, brute force)
def oracle_nn(query, target, max_dist, chunk=256):
    """min(|q - nearest target|, max_dist) in fp64 from chunked pairwise differences (no |a|^2 + |b|^2 - 2ab: that cancels)"""
    q, t = np.asarray(query, np.float64), np.asarray(target, np.float64)
    out = np.full(len(q), float(max_dist))
    if len(t) == 0:
        return out
    for i in range(0, len(q), chunk):
        d = q[i:i + chunk, None, :] - t[None, :, :]
        out[i:i + chunk] = np.minimum(np.sqrt((d * d).sum(-1).min(1)), max_dist)
    return out


def surface(rs, n, offset=0.0):
    """a tilted, rippled surface in DTU-like coordinates (up to 10^3)"""
    x, y = rs.uniform(0, 1000, n), rs.uniform(0, 1000, n)
    z = 300 + 0.3 * x - 0.2 * y + 15 * np.sin(x / 40) * np.cos(y / 55)
    return (np.stack([x, y, z], -1) + offset).astype(np.float32)


_CASE = {}


def seeded_case():
    """item 1's input: 2e4 targets on the surface, 2e4 queries on it with 0.5 noise, 500 of them displaced by up to 60"""
    if not _CASE:
        rs = np.random.RandomState(20)
        target = surface(rs, 20000)
        query = surface(rs, 20000).astype(np.float64) + rs.normal(0, 0.5, (20000, 3))
        far = rs.choice(20000, 500, replace=False)
        v = rs.normal(size=(500, 3))
        query[far] += v / np.linalg.norm(v, axis=1, keepdims=True) * rs.uniform(0, 60, (500, 1))
        query = query.astype(np.float32)
        _CASE.update(query=query, target=target, d_qt=oracle_nn(query, target, MAX_DIST), d_tq=oracle_nn(target, query, MAX_DIST))
    return _CASE


def assert_within_bound(got, want, what=""):
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want)
    worst = float((err / np.maximum(want, 1e-300)).max()) if len(want) else 0.0
    print(f"{what}: max relative error {worst / 2.0 ** -24:.2f} * 2^-24 over {len(want)} points")
    assert (err <= EPS * want).all(), (what, worst)


def dev(ops, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)


# ------------------------------------------------------------------------------------------ 1. per-point distances
def test_distances_match_the_oracle_at_every_point(ops):
    c = seeded_case()
    assert (c["d_qt"] >= MAX_DIST).sum() > 20 and (c["d_qt"] < MAX_DIST).sum() > 19000          # some beyond max_dist, most not
    stats = {}
    got = CE.nn_distance(ops, dev(ops, c["query"]), dev(ops, c["target"]), MAX_DIST, stats=stats)
    print(stats)
    assert_within_bound(got, c["d_qt"], "two passes, automatic cell")
    assert_within_bound(CE.nn_distance(ops, c["target"], c["query"], MAX_DIST), c["d_tq"], "reverse direction, numpy input")


# ------------------------------------------------------------------------------------------ 2. edge cases
def test_empty_and_single_target(ops):
    rs = np.random.RandomState(1)
    q = rs.uniform(-5, 5, (131, 3)).astype(np.float32)
    got = CE.nn_distance(ops, q, np.zeros((0, 3), np.float32), 3.0)
    assert got.shape == (131,) and (got.cpu().numpy() == np.float32(3.0)).all()
    t = np.array([[0.25, -0.5, 1.0]], np.float32)
    for cell in (None, 0.1, 3.0):
        assert_within_bound(CE.nn_distance(ops, q, t, 6.0, cell=cell), oracle_nn(q, t, 6.0), f"single target, cell {cell}")
    assert CE.nn_distance(ops, np.zeros((0, 3), np.float32), t, 1.0).shape == (0,)


def test_all_queries_beyond_max_dist_return_max_dist_exactly(ops):
    rs = np.random.RandomState(2)
    t = surface(rs, 3000)
    q = t[:777] + np.array([0, 0, 500], np.float32)
    for passes in (1, 2):
        got = CE.nn_distance(ops, q, t, MAX_DIST, cell=10.0, passes=passes).cpu().numpy()
        assert (got == np.float32(MAX_DIST)).all()


def test_duplicates_cell_faces_negative_and_offset_coordinates(ops):
    rs = np.random.RandomState(3)
    t = rs.uniform(-40, 40, (4099, 3)).astype(np.float32)                   # negative coordinates; M and Q not multiples of 64
    q = np.concatenate([t[:1000], rs.uniform(-45, 45, (1501, 3)).astype(np.float32)])
    got = CE.nn_distance(ops, q, t, 5.0, cell=2.0)
    assert (got[:1000].cpu().numpy() == 0).all()                            # duplicates: distance 0
    assert_within_bound(got, oracle_nn(q, t, 5.0), "negative coordinates")
    # queries exactly on cell faces: the grid origin is the targets' minimum corner, faces at origin + k * cell
    lo = t.min(0).astype(np.float64)
    faces = (lo + 2.0 * rs.randint(0, 40, (600, 3))).astype(np.float32)
    assert ((faces.astype(np.float64) - lo) / 2.0 == np.floor((faces.astype(np.float64) - lo) / 2.0)).all()
    assert_within_bound(CE.nn_distance(ops, faces, t, 5.0, cell=2.0, passes=1), oracle_nn(faces, t, 5.0), "queries on cell faces")
    # both clouds offset by 1e5: the grid origin follows the data
    rs = np.random.RandomState(4)
    t5, q5 = surface(rs, 3001, offset=1.0e5), surface(rs, 2003, offset=1.0e5)
    g = CE.build_grid(dev(ops, t5), 4.0)
    assert min(g["origin"]) > 9.0e4 and max(g["dims"]) < 400
    assert_within_bound(CE.nn_distance(ops, q5, t5, MAX_DIST, cell=4.0), oracle_nn(q5, t5, MAX_DIST), "offset 1e5")


@pytest.mark.parametrize("cell", [0.05, 0.4, 3.0, 8.0])
def test_cell_size_from_far_below_the_spacing_up_to_max_dist(ops, cell):
    rs = np.random.RandomState(5)
    t = (surface(rs, 2500) * 0.1).astype(np.float32)                        # 100 x 100 surface, spacing about 2
    q = (t[rs.randint(0, 2500, 1203)].astype(np.float64) + rs.normal(0, 1.5, (1203, 3))).astype(np.float32)
    want = oracle_nn(q, t, 8.0)
    for passes in (1, 2):
        assert_within_bound(CE.nn_distance(ops, q, t, 8.0, cell=cell, passes=passes), want, f"cell {cell}, passes {passes}")


# ------------------------------------------------------------------------------------------ 3. independence of the cell size
def test_result_does_not_depend_on_the_cell_size(ops):
    c = seeded_case()
    q, t = dev(ops, c["query"]), dev(ops, c["target"])
    res = {}
    for cell in (1.25, 5.0, 20.0):                                          # a factor of 16
        res[cell] = CE.nn_distance(ops, q, t, MAX_DIST, cell=cell, passes=1).cpu().numpy()
        assert_within_bound(res[cell], c["d_qt"], f"cell {cell}")
    res["auto"] = CE.nn_distance(ops, q, t, MAX_DIST).cpu().numpy()
    keys = list(res)
    for a in keys:
        for b in keys[keys.index(a) + 1:]:
            differ = res[a] != res[b]
            print(f"cell {a} vs {b}: {int(differ.sum())} points not bit-identical")
            # two cell sizes may differ only where two targets tie within the bound
            assert (np.abs(res[a].astype(np.float64) - res[b])[differ] <= 2 * EPS * c["d_qt"][differ]).all()
            assert int(differ.sum()) == 0


# ------------------------------------------------------------------------------------------ 4. statistics
def restated_stats(d, valid, max_dist, thresholds, scale):
    v = np.ones(len(d), bool) if valid is None else valid.astype(bool)
    inr = v & (d < np.float32(max_dist))
    terms = np.rint(d[inr].astype(np.float64) * scale).astype(np.uint64)
    return [int(v.sum()), int(inr.sum()), int(terms.sum(dtype=np.uint64))] + [int((v & (d < np.float32(t))).sum()) for t in thresholds]


def test_statistics_are_exact_integers_independent_of_launch_shape_and_order(ops):
    rs = np.random.RandomState(6)
    n = 100003
    d = np.minimum(rs.gamma(2.0, 3.0, n), MAX_DIST).astype(np.float32)
    valid = (rs.uniform(size=n) < 0.8).astype(np.uint8)
    scale = CE.fixed_scale(MAX_DIST, n)
    assert MAX_DIST * scale * n < 2.0 ** 62 <= MAX_DIST * 2 * scale * n and np.log2(scale) == int(np.log2(scale))
    for vmask in (valid, None):
        want = restated_stats(d, vmask, MAX_DIST, THRESHOLDS, scale)
        vt = None if vmask is None else dev(ops, vmask)
        got = [ops.cloud_stats(dev(ops, d), vt, MAX_DIST, THRESHOLDS, scale, blocks=b).cpu().tolist() for b in (0, 1, 7, 391)]
        assert all(g == want for g in got), (got, want)
        perm = rs.permutation(n)
        vp = None if vmask is None else dev(ops, vmask[perm])
        assert ops.cloud_stats(dev(ops, d[perm]), vp, MAX_DIST, THRESHOLDS, scale).cpu().tolist() == want
        inr = (np.ones(n, bool) if vmask is None else vmask.astype(bool)) & (d < MAX_DIST)
        mean = want[2] / scale / want[1]
        assert abs(mean - d[inr].astype(np.float64).mean()) <= 0.5 / scale
    s = CE.side_stats(ops, dev(ops, d), dev(ops, valid), MAX_DIST, THRESHOLDS)
    assert [s["valid"], s["in_range"], s["sum_fixed"]] + s["below"] == restated_stats(d, valid, MAX_DIST, THRESHOLDS, s["scale"])
    assert ops.cloud_stats(dev(ops, d[:0]), None, MAX_DIST, [], 1.0).cpu().tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------ 5. metrics
def oracle_metrics(d_pred, d_gt, max_dist, thresholds, valid_p=None, valid_g=None):
    """the same quantities from fp64 distances.  -> (metrics, points inside the either-side bands)"""
    out, band = {}, 0
    for name, d, v in (("pred", d_pred, valid_p), ("gt", d_gt, valid_g)):
        v = np.ones(len(d), bool) if v is None else v.astype(bool)
        d = d[v]
        for t in list(thresholds) + [max_dist]:
            band += int((np.abs(d - t) <= 1e-6 * t).sum()) - (int((d == max_dist).sum()) if t == max_dist else 0)      # the clamp itself is not a band
        inr = d < max_dist
        out[name] = {"valid": int(len(d)), "in_range": int(inr.sum()), "mean": float(d[inr].mean()), "below": [int((d < t).sum()) for t in thresholds]}
    return out, band


def assert_metrics_match(res, want, thresholds):
    for side, key in (("pred", "accuracy"), ("gt", "completeness")):
        s, w = res[side], want[side]
        assert (s["valid"], s["in_range"], s["below"]) == (w["valid"], w["in_range"], w["below"]), (side, s, w)
        assert s["out_of_range"] == w["valid"] - w["in_range"]
        print(f"{key}: {res[key]!r} (oracle {w['mean']!r}), scale 2^{int(np.log2(s['scale']))}")
        assert abs(res[key] - w["mean"]) <= EPS * w["mean"] + 0.5 / s["scale"]
    assert res["overall"] == 0.5 * (res["accuracy"] + res["completeness"])
    for i, _ in enumerate(thresholds):
        p, r = want["pred"]["below"][i] / want["pred"]["valid"], want["gt"]["below"][i] / want["gt"]["valid"]
        assert res["precision"][i] == p and res["recall"][i] == r
        assert res["fscore"][i] == (2 * p * r / (p + r) if p + r > 0 else 0.0)


def test_metrics_match_the_oracle(ops):
    c = seeded_case()
    want, band = oracle_metrics(c["d_qt"], c["d_tq"], MAX_DIST, THRESHOLDS[:3])
    assert band == 0, "the seeded input must keep every distance away from the thresholds and from max_dist"
    res = CE.evaluate(ops, c["query"], c["target"], MAX_DIST, THRESHOLDS)
    assert json.loads(json.dumps(res))["accuracy"] == res["accuracy"]
    want, _ = oracle_metrics(c["d_qt"], c["d_tq"], MAX_DIST, THRESHOLDS)
    assert_metrics_match(res, want, THRESHOLDS)
    assert res["pred"]["below"][3] == res["pred"]["in_range"]               # threshold 20 = max_dist
    # a cloud against itself: accuracy 0, completeness 0, F-score 1 everywhere
    same = CE.evaluate(ops, c["target"], c["target"], MAX_DIST, THRESHOLDS)
    assert same["accuracy"] == 0 and same["completeness"] == 0 and same["overall"] == 0 and same["fscore"] == [1.0] * 4


# ------------------------------------------------------------------------------------------ 6. read_ply
def test_read_ply_round_trips_write_ply_byte_for_byte(tmp_path):
    rs = np.random.RandomState(7)
    xyz, rgb = rs.normal(0, 300, (1234, 3)).astype(np.float32), rs.randint(0, 256, (1234, 3)).astype(np.uint8)
    IO.write_ply(str(tmp_path / "a.ply"), xyz, rgb)
    x, c = IO.read_ply(str(tmp_path / "a.ply"))
    assert x.dtype == np.float32 and c.dtype == np.uint8 and x.tobytes() == xyz.tobytes() and c.tobytes() == rgb.tobytes()
    IO.write_ply(str(tmp_path / "b.ply"), x, c)
    assert (tmp_path / "a.ply").read_bytes() == (tmp_path / "b.ply").read_bytes()


def test_read_ply_ascii_normals_faces_and_errors(tmp_path):
    p = tmp_path / "ascii.ply"
    p.write_text("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                 "element face 1\nproperty list uchar int vertex_indices\nend_header\n0 0 0\n1.5 -2 3e2\n4 5 6\n3 0 1 2\n")
    x, c = IO.read_ply(str(p))
    assert c is None and x.tolist() == [[0, 0, 0], [1.5, -2, 300], [4, 5, 6]]
    # binary: colour first, double normals between the coordinates' neighbours, a face element behind the vertices
    dt = np.dtype([("red", "u1"), ("green", "u1"), ("blue", "u1"), ("x", "<f4"), ("nx", "<f8"), ("y", "<f4"), ("z", "<f4"), ("ny", "<f8"), ("nz", "<f8")])
    v = np.zeros(5, dt)
    rs = np.random.RandomState(8)
    for k in ("x", "y", "z", "nx", "ny", "nz"):
        v[k] = rs.normal(size=5)
    for k in ("red", "green", "blue"):
        v[k] = rs.randint(0, 256, 5)
    head = ("ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty uchar red\nproperty uchar green\nproperty uchar blue\n"
            "property float x\nproperty double nx\nproperty float y\nproperty float z\nproperty double ny\nproperty double nz\n"
            "element face 2\nproperty list uchar int vertex_indices\nend_header\n").encode()
    faces = b"".join(bytes([3]) + np.array(f, "<i4").tobytes() for f in ([0, 1, 2], [2, 3, 4]))
    (tmp_path / "n.ply").write_bytes(head + v.tobytes() + faces)
    x, c = IO.read_ply(str(tmp_path / "n.ply"))
    assert (x == np.stack([v["x"], v["y"], v["z"]], -1)).all() and (c == np.stack([v["red"], v["green"], v["blue"]], -1)).all()
    # a face element IN FRONT of the vertices is stepped over
    head2 = head.replace(b"element face 2\nproperty list uchar int vertex_indices\n", b"").replace(
        b"element vertex 5", b"element face 2\nproperty list uchar int vertex_indices\nelement vertex 5")
    (tmp_path / "f.ply").write_bytes(head2 + faces + v.tobytes())
    assert (IO.read_ply(str(tmp_path / "f.ply"))[0] == x).all()
    (tmp_path / "t.ply").write_bytes(head + v.tobytes()[:-7])
    with pytest.raises(ValueError, match="truncated"):
        IO.read_ply(str(tmp_path / "t.ply"))
    (tmp_path / "be.ply").write_bytes(head.replace(b"binary_little_endian", b"binary_big_endian") + v.tobytes() + faces)
    with pytest.raises(ValueError, match="binary_big_endian"):
        IO.read_ply(str(tmp_path / "be.ply"))


# ------------------------------------------------------------------------------------------ 7. voxel_downsample
def test_voxel_downsample_keeps_the_lowest_index_of_every_voxel(ops):
    rs = np.random.RandomState(9)
    xyz = rs.uniform(-3, 7, (5000, 3)).astype(np.float32)
    voxel = 0.9
    cells = np.floor(xyz.astype(np.float64) / voxel).astype(np.int64)
    first = {}
    for i, c in enumerate(map(tuple, cells)):
        first.setdefault(c, i)
    want = np.array(sorted(first.values()))
    pts_cpu, idx_cpu = CE.voxel_downsample(xyz, voxel)
    pts_dev, idx_dev = CE.voxel_downsample(dev(ops, xyz), voxel)
    assert idx_cpu.tolist() == want.tolist() == idx_dev.cpu().tolist()
    assert (pts_cpu.numpy() == xyz[want]).all() and (pts_dev.cpu().numpy() == xyz[want]).all()
    assert len(set(map(tuple, cells[want]))) == len(want) == len(first)     # exactly one point per occupied voxel
    # appending points in voxels that are already occupied changes nothing
    extra = (xyz[rs.randint(0, 5000, 700)].astype(np.float64))
    extra = ((np.floor(extra / voxel) + rs.uniform(0.05, 0.95, extra.shape)) * voxel).astype(np.float32)
    assert set(map(tuple, np.floor(extra.astype(np.float64) / voxel).astype(np.int64))) <= set(first)
    assert CE.voxel_downsample(np.concatenate([xyz, extra]), voxel)[1].tolist() == want.tolist()
    assert CE.voxel_downsample(xyz[:0], voxel)[1].numel() == 0


# ------------------------------------------------------------------------------------------ 8. region of interest
def synthetic_roi(rs):
    mask = rs.uniform(size=(30, 26, 12)) < 0.6
    return {"mask": mask, "origin": np.array([100.0, 150.0, 280.0]), "resolution": 25.0, "plane": np.array([0.1, -0.05, 1.0, -420.0])}


def restated_roi(pred, gt, roi):
    u = (pred.astype(np.float64) - roi["origin"]) / roi["resolution"]
    v = (np.sign(u) * np.floor(np.abs(u) + 0.5)).astype(np.int64)            # MATLAB's round
    inside = ((v >= 0) & (v < np.array(roi["mask"].shape))).all(1)
    vp = np.zeros(len(pred), bool)
    vp[inside] = roi["mask"][v[inside, 0], v[inside, 1], v[inside, 2]]
    vg = gt.astype(np.float64) @ roi["plane"][:3] + roi["plane"][3] > 0
    return vp, vg


def test_roi_excludes_what_a_numpy_restatement_excludes(ops, tmp_path):
    c = seeded_case()
    r = synthetic_roi(np.random.RandomState(10))
    np.savez(str(tmp_path / "roi.npz"), **r)
    roi = CE.load_roi(str(tmp_path / "roi.npz"))
    vp, vg = restated_roi(c["query"], c["target"], r)
    assert 2000 < vp.sum() < 15000 and 2000 < vg.sum() < 18000               # the volume and the plane both cut the clouds
    assert (CE.roi_volume_mask(dev(ops, c["query"]), roi).cpu().numpy().astype(bool) == vp).all()
    assert (CE.roi_plane_mask(dev(ops, c["target"]), roi).cpu().numpy().astype(bool) == vg).all()
    want, band = oracle_metrics(c["d_qt"], c["d_tq"], MAX_DIST, THRESHOLDS[:3], vp, vg)
    assert band == 0
    res = CE.evaluate(ops, c["query"], c["target"], MAX_DIST, THRESHOLDS[:3], roi=roi)
    assert_metrics_match(res, want, THRESHOLDS[:3])
    no_plane = CE.make_roi(r["mask"], r["origin"], r["resolution"])
    assert CE.evaluate(ops, c["query"], c["target"], MAX_DIST, [1.0], roi=no_plane)["gt"]["valid"] == len(c["target"])


def test_dtu_mat_loader(tmp_path):
    sio = pytest.importorskip("scipy.io")
    r = synthetic_roi(np.random.RandomState(11))
    bb = np.stack([r["origin"], r["origin"] + r["resolution"] * np.array(r["mask"].shape)])
    sio.savemat(str(tmp_path / "ObsMask1_10.mat"), {"ObsMask": r["mask"].astype(np.uint8), "BB": bb, "Res": r["resolution"]})
    sio.savemat(str(tmp_path / "Plane1.mat"), {"P": r["plane"].reshape(4, 1)})
    roi = CE.load_dtu_roi(str(tmp_path / "ObsMask1_10.mat"), str(tmp_path / "Plane1.mat"))
    assert (roi["mask"] == r["mask"]).all() and (roi["origin"] == r["origin"]).all() and roi["resolution"] == 25.0
    assert (roi["plane"] == r["plane"]).all()


def test_only_the_mat_loader_imports_scipy():
    for base, _, files in os.walk(os.path.join(ROOT, "diffmvs_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(base, f)).read()
                assert ("scipy" in src) == (f == "cloud_eval.py"), f
    src = open(os.path.join(ROOT, "diffmvs_amd", "cloud_eval.py")).read()
    assert src.count("import") and all("scipy" not in ln for ln in src.splitlines() if ln.startswith(("import ", "from ")))
    out = subprocess.run([sys.executable, "-c", "import sys; import diffmvs_amd.cloud_eval; print('scipy' in sys.modules)"], cwd=ROOT,
                         capture_output=True, text=True)
    assert out.stdout.strip() == "False", out.stderr[-1000:]


# ------------------------------------------------------------------------------------------ 10. entry-point validation (no device)
def test_invalid_arguments_are_rejected_before_any_launch():
    """every DMVS_EINVAL case of include/dmvs.h returns -22; the device pointers below are never dereferenced"""
    from diffmvs_amd.build import build_hip
    lib = _lib.Lib(build_hip())
    p = ctypes.c_void_p(4096)
    origin, dims = (ctypes.c_double * 3)(0.0, 0.0, 0.0), (ctypes.c_int32 * 3)(8, 8, 8)

    def nn(query=p, Q=10, target=p, M=10, keys=p, start=p, C=5, origin=origin, h=1.0, dims=dims, max_dist=2.0, dist=p):
        return lib.dll.dmvs_cloud_nn_dist_f32(query, Q, target, M, keys, start, C, origin, h, dims, max_dist, dist, None, None)

    for kw in (dict(query=None), dict(dist=None), dict(target=None), dict(keys=None), dict(start=None), dict(origin=None), dict(dims=None),
               dict(Q=-1), dict(M=-1), dict(C=-1), dict(C=11), dict(C=0), dict(M=0, C=5),
               dict(h=0.0), dict(h=-1.0), dict(h=float("nan")), dict(h=float("inf")),
               dict(max_dist=0.0), dict(max_dist=-2.0), dict(max_dist=float("nan")), dict(max_dist=float("inf")),
               dict(origin=(ctypes.c_double * 3)(0.0, float("nan"), 0.0)), dict(dims=(ctypes.c_int32 * 3)(8, 0, 8)),
               dict(h=1.0e-3, max_dist=2.0),                                                      # 2000 rings > DMVS_CLOUD_MAX_RINGS
               dict(dims=(ctypes.c_int32 * 3)(1 << 21, 1 << 21, 1 << 21))):                       # 63 key bits
        assert nn(**kw) == -22, kw
    assert nn(Q=0) == 0 and nn(Q=0, M=0, C=0, target=None, keys=None, start=None) == 0          # nothing to do: no launch

    thr = (ctypes.c_float * 16)(*([1.0] * 16))

    def stats(dist=p, valid=None, N=1000, max_dist=20.0, thresholds=thr, T=3, scale=2.0 ** 40, blocks=0, out=p):
        return lib.dll.dmvs_cloud_stats_f32(dist, valid, N, max_dist, thresholds, T, scale, blocks, out, None)

    for kw in (dict(dist=None), dict(out=None), dict(thresholds=None), dict(N=-1), dict(T=-1), dict(T=17), dict(blocks=-1),
               dict(max_dist=0.0), dict(max_dist=float("nan")), dict(max_dist=float("inf")),
               dict(scale=0.0), dict(scale=-4.0), dict(scale=3.0), dict(scale=float("inf")), dict(scale=float("nan")),
               dict(scale=2.0 ** 48),                                                               # 20 * 2^48 * 1000 >= 2^62
               dict(thresholds=(ctypes.c_float * 16)(float("nan")))):
        assert stats(**kw) == -22, kw
    with pytest.raises(_lib.DmvsError, match="thresholds"):
        from conftest import emu_ops
        emu_ops().cloud_stats(torch.zeros(4), None, 1.0, [0.5] * 17, 1.0)
    with pytest.raises(_lib.DmvsError, match="contiguous"):
        emu_ops().cloud_stats(torch.zeros(4, dtype=torch.float64), None, 1.0, [0.5], 1.0)
    with pytest.raises(ValueError, match="rings"):
        CE.nn_distance(emu_ops(), np.zeros((3, 3), np.float32), np.ones((3, 3), np.float32), 20.0, cell=0.001, passes=1)


# ------------------------------------------------------------------------------------------ 9. end to end on the GPU
def fused_scene(tmp, ops, outliers):
    """tests/fusion_scene.py's tree fused by the consistency filter -> (ply file, ground-truth cloud from the noiseless depth maps)"""
    import fusion_scene
    from diffmvs_amd import fusion, synth
    root = fusion_scene.build_tree(str(tmp / f"scan{outliers}"), outliers=outliers)
    ply = str(tmp / f"fused{outliers}.ply")
    n = fusion.filter_depth(root, root, ply, geo_mask_thres=2, photo_thres=[0.3, 0.4, 0.5], method="casdiffmvs", dataset="dtu", ops=ops)
    assert n > 0
    H, W, V = fusion_scene.H, fusion_scene.W, fusion_scene.V
    depths = np.asarray(synth.synth_view_depths(H, W, V, seed=21), np.float64)
    gt = []
    for v in range(V):
        k, e, _, _ = IO.read_camera_parameters(os.path.join(root, f"cams/{v:08d}_cam.txt"))
        gt.append(fusion.unproject(depths[v], k, e, np.ones((H, W), bool)))
    return ply, np.concatenate(gt).astype(np.float32)


E2E_THRESHOLDS = [1.0, 2.0, 5.0]


@pytest.mark.gpu
def test_fused_scene_scores_match_the_oracle(tmp_path):
    from conftest import hip_ops
    ops = hip_ops()
    ply, gt = fused_scene(tmp_path, ops, 0.06)
    pred = IO.read_ply(ply)[0]
    d_pg, d_gp = oracle_nn(pred, gt, MAX_DIST), oracle_nn(gt, pred, MAX_DIST)
    want, band = oracle_metrics(d_pg, d_gp, MAX_DIST, E2E_THRESHOLDS)
    assert band == 0
    res = CE.evaluate(ops, pred, gt, MAX_DIST, E2E_THRESHOLDS)
    assert_metrics_match(res, want, E2E_THRESHOLDS)
    IO.write_ply(str(tmp_path / "gt.ply"), gt, np.zeros((len(gt), 3), np.uint8))
    cli = subprocess.run([sys.executable, "-m", "diffmvs_amd.cloud_eval", "--pred", ply, "--gt", str(tmp_path / "gt.ply"), "--max_dist", "20",
                          "--thresholds", "1", "2", "5", "--error_ply", str(tmp_path / "err.ply")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert cli.returncode == 0, cli.stderr[-2000:]
    assert json.loads(cli.stdout.strip().splitlines()[-1]) == json.loads(json.dumps(res))
    ex, ec = IO.read_ply(str(tmp_path / "err.ply"))
    assert (ex == pred).all() and ec.shape == (len(pred), 3)
    same = CE.evaluate(ops, gt, gt, MAX_DIST, E2E_THRESHOLDS)
    assert same["accuracy"] == 0 and same["completeness"] == 0 and same["fscore"] == [1.0, 1.0, 1.0]
    ply0, gt0 = fused_scene(tmp_path, ops, 0.0)
    clean = CE.evaluate(ops, IO.read_ply(ply0)[0], gt0, MAX_DIST, E2E_THRESHOLDS)
    for k in ("accuracy", "completeness", "overall", "precision", "recall", "fscore"):       # for the reader; not asserted
        print(f"{k}: outliers=0.06 {res[k]}   outliers=0 {clean[k]}")
    print("out of range (prediction):", res["pred"]["out_of_range"], "of", res["pred"]["valid"], "  outliers=0:", clean["pred"]["out_of_range"])


@pytest.mark.gpu
def test_eval_driver_reports_the_command_lines_numbers(tmp_path):
    from diffmvs_amd import colmap as CM
    from diffmvs_amd import eval as EV
    from diffmvs_amd import synth
    H, W, V, seed = 64, 96, 6, 2
    scene = synth.synth_scene(H, W, n_views=V, n_src=2, seed=seed, grid_w=3)
    ws, tree, out = tmp_path / "ws", tmp_path / "tree", tmp_path / "out"
    synth.export_colmap(scene, str(ws), seed=seed)
    from conftest import hip_ops
    CM.convert(str(ws), str(tree), num_src_images=4, ops=hip_ops(), copy_images=True)
    d0, a, c = synth.scene_plane(seed)
    xs, ys = np.meshgrid(np.linspace(-400, 400, 160), np.linspace(-300, 300, 120))
    gt = np.stack([xs.ravel(), ys.ravel(), d0 + a * xs.ravel() + c * ys.ravel()], -1).astype(np.float32)
    IO.write_ply(str(tmp_path / "gt.ply"), gt, np.zeros((len(gt), 3), np.uint8))
    base = ["--testpath", str(tree), "--dataset", "general", "--outdir", str(out), "--method", "diffmvs", "--num_view", "3",
            "--numdepth_initial", "16", "--noise_seed", "7", "--filter", "--geo_mask_thres", "1", "--geo_pixel_thres", "4",
            "--geo_depth_thres", "0.05", "--photo_thres", "0.0", "0.0", "0.0"]
    res = EV.main(base + ["--gt_ply", str(tmp_path / "gt{scene}.ply"), "--cloud_max_dist", "50", "--cloud_density", "2", "--cloud_thresholds", "5", "10"])
    assert res["fused_points"][""] > 0 and set(res["cloud_metrics"]) == {""}
    cli = CE.main(["--pred", res["ply"][""], "--gt", str(tmp_path / "gt.ply"), "--max_dist", "50", "--density", "2", "--thresholds", "5", "10"])
    assert json.loads(json.dumps(cli)) == json.loads(json.dumps(res["cloud_metrics"][""]))
    assert cli["pred"]["points"] <= cli["pred_points_read"] == res["fused_points"][""]
    plain = EV.main([x if x != str(out) else str(tmp_path / "out2") for x in base])
    assert "cloud_metrics" not in plain and set(plain) == set(res) - {"cloud_metrics"}
