"""COLMAP import (diffmvs_amd.colmap): model I/O, the view-selection kernel (dmvs_view_select_scores_f64) against an fp64 restatement
of the reference's calc_score (colmap_input.py:374-390), byte parity of the written tree with the reference's own output
(tests/golden/colmap.npz, tests/golden/make_golden_colmap.py), the error messages, and the synthetic scene end to end through
the converter and the evaluation driver on the GPU."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from diffmvs_amd import _lib
from diffmvs_amd import colmap as CM


# ------------------------------------------------------------------------------------------ the restatement (fp64, pair-major)
def restated_scores(model, theta0=5.0, sigma1=1.0, sigma2=10.0):
    """calc_score for every pair i < j in numpy fp64, with the module's two deviations (clamped cosine, zero-length ray -> 0);
    -> (score [N,N], shared [N,N]: the number of terms of each pair)"""
    extr = [CM.extrinsic(im) for im in model.images]
    C = CM.camera_centres(extr)
    row = {int(p): r for r, p in enumerate(model.points.ids)}
    N = len(model.images)
    S, shared = np.zeros((N, N)), np.zeros((N, N), np.int64)
    for i in range(N):
        ids_i = model.images[i].point3d_ids
        for j in range(i + 1, N):
            ids = ids_i[(ids_i != -1) & np.isin(ids_i, model.images[j].point3d_ids)]
            if ids.size == 0:
                continue
            p = model.points.xyz[[row[int(x)] for x in ids]]
            a, b = C[i] - p, C[j] - p
            na, nb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
            ok = (na > 0) & (nb > 0)
            with np.errstate(divide="ignore", invalid="ignore"):
                cos = np.clip((a * b).sum(1) / na / nb, -1.0, 1.0)
            th = (180 / np.pi) * np.arccos(cos)
            s = np.where(th <= theta0, sigma1, sigma2)
            S[i, j] = S[j, i] = float(np.where(ok, np.exp(-(th - theta0) * (th - theta0) / (2 * s ** 2)), 0.0).sum())
            shared[i, j] = shared[j, i] = ids.size
    return S, shared


def random_model(seed, N, P, max_track=40, scale=1.0, offset=0.0):
    """N images around a cloud of P points; every point is listed by 1..max_track images, some twice, plus -1 entries"""
    rs = np.random.RandomState(seed)
    xyz = rs.uniform(-1.5, 1.5, (P, 3)) * scale + offset
    ids = rs.permutation(P) * 5 + 2
    lists = [[] for _ in range(N)]
    for r in range(P):
        for i in rs.choice(N, min(N, rs.randint(1, max_track + 1)), replace=False):
            lists[i].append(int(ids[r]))
            if rs.uniform() < 0.05:
                lists[i].append(int(ids[r]))
    images = []
    for i in range(N):
        if not lists[i]:
            lists[i].append(int(ids[0]))
        lst = list(rs.permutation(lists[i])) + [-1] * rs.randint(0, 3)
        ang = rs.uniform(0, 2 * np.pi)
        c = np.array([6 * np.sin(ang), rs.uniform(-1, 1), 6 * np.cos(ang)]) * scale + offset
        q = rs.normal(size=4)
        q = q / np.linalg.norm(q)
        R = CM.quaternion_to_rotation_matrix(q)
        images.append(CM.Image(i + 1, tuple(map(float, q)), tuple(map(float, -R @ c)), 1, "im%d.jpg" % i, np.zeros((len(lst), 2)),
                               np.array(lst, np.int64)))
    toff = np.zeros(P + 1, np.int64)
    pts = CM.Points3D(ids.astype(np.int64), xyz, np.zeros((P, 3), np.uint8), np.zeros(P), toff, np.zeros((0, 2), np.int32))
    return CM.Model({1: CM.Camera(1, "PINHOLE", 64, 48, (50.0, 50.0, 32.0, 24.0))}, images, pts)


def kernel_scores(ops, model, **kw):
    extr = [CM.extrinsic(im) for im in model.images]
    return CM.view_scores(ops, model, CM.camera_centres(extr), CM._point_rows(model), **kw)


# ------------------------------------------------------------------------------------------ model I/O (CPU)
def _golden():
    return np.load(os.path.join(GOLDEN, "colmap.npz"))


def _write_golden_bins(z, name, d):
    os.makedirs(d, exist_ok=True)
    for f in ("cameras", "images", "points3D"):
        with open(os.path.join(d, f + ".bin"), "wb") as fh:
            fh.write(z[f"{name}.{f}.bin"].tobytes())


def _assert_models_equal(m, want):
    assert [[c.id, c.model, c.width, c.height, list(c.params)] for c in m.cameras.values()] == want["cameras"]
    got = [[im.id, list(im.qvec), list(im.tvec), im.camera_id, im.name, im.xys.tolist(), im.point3d_ids.tolist()] for im in m.images]
    assert got == want["images"]
    p = m.points
    assert [p.ids.tolist(), p.xyz.tolist(), p.rgb.tolist(), p.error.tolist(), p.track_offsets.tolist(), p.track.tolist()] == want["points"]


def test_golden_bin_bytes_parse_to_the_recorded_models(tmp_path):
    z = _golden()
    for name in json.loads(str(z["meta"]))["models"]:
        _write_golden_bins(z, name, tmp_path / name)
        _assert_models_equal(CM.read_model(str(tmp_path / name), ".bin"), json.loads(str(z[f"{name}.model"])))


def test_model_round_trips_through_bin_and_txt(tmp_path):
    z = _golden()
    _write_golden_bins(z, "a", tmp_path / "src")
    m = CM.read_model(str(tmp_path / "src"), ".bin")
    want = json.loads(str(z["a.model"]))
    for ext in (".bin", ".txt"):
        CM.write_model(m, str(tmp_path / ext[1:]), ext)
        _assert_models_equal(CM.read_model(str(tmp_path / ext[1:]), ext), want)
    for f in ("cameras", "images", "points3D"):       # the writer reproduces the bytes it was read from
        assert (tmp_path / "bin" / (f + ".bin")).read_bytes() == z[f"a.{f}.bin"].tobytes()


def test_model_folder_detection(tmp_path):
    z = _golden()
    _write_golden_bins(z, "b", tmp_path / "ws" / "sparse" / "0")
    assert CM.find_model(str(tmp_path / "ws")) == (str(tmp_path / "ws" / "sparse" / "0"), ".bin")
    CM.write_model(CM.read_model(str(tmp_path / "ws" / "sparse" / "0"), ".bin"), str(tmp_path / "ws" / "sparse"), ".txt")
    assert CM.find_model(str(tmp_path / "ws")) == (str(tmp_path / "ws" / "sparse"), ".txt")      # sparse/ before sparse/0/
    _write_golden_bins(z, "b", tmp_path / "ws" / "sparse")
    assert CM.find_model(str(tmp_path / "ws")) == (str(tmp_path / "ws" / "sparse"), ".bin")      # .bin before .txt
    with pytest.raises(CM.ColmapError, match="no COLMAP model"):
        CM.find_model(str(tmp_path))


# ------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("N,P,max_track", [(2, 30, 2), (5, 80, 5), (17, 120, 17), (64, 90, 40)])
def test_view_scores_match_the_restatement(ops, N, P, max_track):
    model = random_model(100 + N, N, P, max_track)
    got = kernel_scores(ops, model)
    want, shared = restated_scores(model)
    assert got.dtype == np.float64 and got.shape == (N, N)
    assert (got == got.T).all() and (np.diag(got) == 0).all()
    assert (np.abs(got - want) <= 1e-10 * np.maximum(1, shared)).all(), np.abs(got - want).max()


def test_view_scores_world_scale_coordinates(ops):
    """far from the origin, c - p cancels: fp64 throughout keeps the scores to the restatement's precision"""
    model = random_model(7, 9, 60, 9, scale=3.0, offset=1.0e5)
    want, shared = restated_scores(model, 4.0, 1.5, 8.0)
    got = kernel_scores(ops, model, theta0=4.0, sigma1=1.5, sigma2=8.0)
    assert (np.abs(got - want) <= 1e-10 * np.maximum(1, shared)).all(), np.abs(got - want).max()


def test_view_scores_degenerate_geometry(ops):
    """deviation 1: a point on the line through both centres (cosine rounds past +-1: the reference's nan) scores as theta = 0
    or 180; deviation 2: a point AT a camera centre contributes 0 (the reference divides by zero)"""
    model = random_model(3, 3, 10, 3)
    extr = [CM.extrinsic(im) for im in model.images]
    C = CM.camera_centres(extr)
    xyz = model.points.xyz.copy()
    xyz[0] = C[0] + 0.37 * (C[1] - C[0])          # between centres 0 and 1: theta ~ 180
    xyz[1] = C[0] + 2.5 * (C[1] - C[0])           # beyond centre 1: theta ~ 0
    xyz[2] = C[2]                                  # at centre 2
    pts = model.points._replace(xyz=xyz)
    ids = [int(x) for x in pts.ids[:3]]
    images = [im._replace(point3d_ids=np.array(ids, np.int64), xys=np.zeros((3, 2))) for im in model.images]
    model = model._replace(images=images, points=pts)
    got = kernel_scores(ops, model)
    want, shared = restated_scores(model)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    assert (np.abs(got - want) <= 1e-10 * np.maximum(1, shared)).all()
    # point 2 (at centre 2) adds nothing to pairs (0,2), (1,2): only points 0 and 1 can count there
    assert got[0, 1] > 0 and abs(got[0, 2] - want[0, 2]) <= 1e-10


def test_view_scores_limits(ops):
    lib = ops.lib
    p = None
    rc = lib.dll.dmvs_view_select_scores_f64(p, p, p, p, p, 0, 0, torch.zeros(1).data_ptr(), _lib.VIEW_SELECT_MAX_IMAGES + 1, 5.0, 1.0, 10.0,
                                             p, torch.zeros(1).data_ptr(), None)
    assert rc == -22
    one = torch.zeros(3, dtype=torch.float64)
    assert lib.dll.dmvs_view_select_scores_f64(p, p, p, p, p, 0, 0, one.data_ptr(), 1, 5.0, 0.0, 10.0, p, one.data_ptr(), None) == -22
    with pytest.raises(_lib.DmvsError, match="images"):
        z64, z32 = torch.zeros(1, dtype=torch.int64, device=ops.device), torch.zeros(0, dtype=torch.int32, device=ops.device)
        ops.view_scores(torch.zeros(0, 3, dtype=torch.float64, device=ops.device), z64, z32, z32,
                        torch.zeros(_lib.VIEW_SELECT_MAX_IMAGES + 1, 3, dtype=torch.float64, device=ops.device))
    # one image, no pairs: the 1x1 zero matrix
    out = ops.view_scores(torch.zeros(0, 3, dtype=torch.float64, device=ops.device), torch.zeros(1, dtype=torch.int64, device=ops.device),
                          torch.zeros(0, dtype=torch.int32, device=ops.device), torch.zeros(0, dtype=torch.int32, device=ops.device),
                          torch.zeros(1, 3, dtype=torch.float64, device=ops.device))
    assert out.shape == (1, 1) and float(out[0, 0]) == 0.0


@pytest.mark.gpu
def test_view_scores_are_bitwise_deterministic():
    """integer fixed-point accumulation: two runs and a run on the model with its points permuted give the same bits"""
    from conftest import hip_ops
    ops = hip_ops()
    model = random_model(11, 48, 400, 40)
    a, b = kernel_scores(ops, model), kernel_scores(ops, model)
    perm = np.random.RandomState(1).permutation(len(model.points.ids))
    p = model.points
    permuted = model._replace(points=p._replace(ids=p.ids[perm], xyz=p.xyz[perm]))
    c = kernel_scores(ops, permuted)
    assert a.tobytes() == b.tobytes() == c.tobytes()


# ------------------------------------------------------------------------------------------ byte parity with the reference
def _convert(ops, root, out, k):
    return CM.convert(str(root), str(out), num_src_images=k, ops=ops, copy_images=False)


def test_converted_tree_is_byte_identical_to_the_reference(ops, tmp_path, capsys):
    z = _golden()
    meta = json.loads(str(z["meta"]))
    for name in meta["models"]:
        m = json.loads(str(z[f"{name}.model"]))
        ws = tmp_path / name
        _write_golden_bins(z, name, ws / "sparse")
        for ext in (".bin", ".txt"):
            if ext == ".txt":
                model = CM.read_model(str(ws / "sparse"), ".bin")
                shutil.rmtree(ws / "sparse")
                CM.write_model(model, str(ws / "sparse"), ".txt")
            for k in meta["ks"]:
                out = tmp_path / f"out_{name}{ext}{k}"
                res = _convert(ops, ws, out, k)
                assert res["num_images"] == len(m["images"])
                assert (out / "pair.txt").read_text() == str(z[f"{name}.k{k}.pair"]), (name, ext, k)
                for i in range(len(m["images"])):
                    assert (out / "cams" / ("%08d_cam.txt" % i)).read_text() == str(z[f"{name}.k{k}.cam{i}"]), (name, ext, k, i)
    assert capsys.readouterr().err.count("SIMPLE_RADIAL cameras have non-zero distortion") == 4      # model a: once per convert(), 2 formats x 2 ks


def test_images_are_copied_or_reencoded(ops, tmp_path):
    from PIL import Image
    z = _golden()
    ws = tmp_path / "ws"
    _write_golden_bins(z, "b", ws / "sparse")
    names = [im[4] for im in json.loads(str(z["b.model"]))["images"]]
    os.makedirs(ws / "images")
    for i, n in enumerate(names):
        Image.fromarray(np.full((8, 12, 3), 40 * i, np.uint8)).save(str(ws / "images" / n))
    CM.convert(str(ws), str(tmp_path / "copy"), ops=ops)
    CM.convert(str(ws), str(tmp_path / "jpg"), ops=ops, convert_format=True)
    for i, n in enumerate(names):
        assert (tmp_path / "copy" / "images" / ("%08d.jpg" % i)).read_bytes() == (ws / "images" / n).read_bytes()
        im = Image.open(str(tmp_path / "jpg" / "images" / ("%08d.jpg" % i)))
        assert im.format == "JPEG" and im.size == (12, 8)


# ------------------------------------------------------------------------------------------ errors
def test_errors_say_what_is_wrong(ops, tmp_path):
    z = _golden()
    model = CM.read_model(*_golden_model_dir(z, tmp_path))
    imgs = list(model.images)
    imgs[2] = imgs[2]._replace(point3d_ids=np.full(len(imgs[2].point3d_ids), -1, np.int64))
    with pytest.raises(CM.ColmapError, match=r"image 'img_002.png' .* lists no valid 3-D point"):
        CM._point_rows(model._replace(images=imgs))
    imgs = list(model.images)
    ids = imgs[1].point3d_ids.copy()
    ids[5] = 999999
    imgs[1] = imgs[1]._replace(point3d_ids=ids)
    ws = tmp_path / "bad"
    CM.write_model(model._replace(images=imgs), str(ws / "sparse"), ".bin")
    with pytest.raises(CM.ColmapError, match="lists point3D_id 999999, which points3D does not contain"):
        CM.convert(str(ws), str(tmp_path / "o"), ops=ops, copy_images=False)
    cams = {1: model.cameras[1]._replace(model="EQUIRECTANGULAR")}
    CM.write_model(model._replace(cameras=cams), str(tmp_path / "cam"), ".txt")
    with pytest.raises(CM.ColmapError, match="unknown COLMAP camera model 'EQUIRECTANGULAR'"):
        CM.read_cameras_text(str(tmp_path / "cam" / "cameras.txt"))
    with pytest.raises(SystemExit, match="R2Former retrieval scoring is not part of diffmvs_amd"):
        CM.main(["--input_folder", str(ws), "--VGGT"])


def _golden_model_dir(z, tmp_path):
    _write_golden_bins(z, "b", tmp_path / "g")
    return str(tmp_path / "g"), ".bin"


# ------------------------------------------------------------------------------------------ end to end on the GPU
@pytest.mark.gpu
def test_synthetic_scene_through_colmap_and_the_eval_driver(tmp_path):
    from diffmvs_amd import eval as EV
    from diffmvs_amd import formats as IO
    from diffmvs_amd import synth
    H, W, V, seed = 64, 96, 6, 2
    scene = synth.synth_scene(H, W, n_views=V, n_src=2, seed=seed, grid_w=3)
    ws, tree = tmp_path / "ws", tmp_path / "tree"
    synth.export_colmap(scene, str(ws), seed=seed)
    r = subprocess.run([sys.executable, "-m", "diffmvs_amd.colmap", "--input_folder", str(ws), "--output_folder", str(tree),
                        "--num_src_images", "4"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["num_images"] == V
    d0, a, c = synth.scene_plane(seed)
    K = scene["K"][0].double().numpy()
    for v in range(V):
        k, e, dmin, dmax = IO.read_cam_file(str(tree / "cams" / ("%08d_cam.txt" % v)))
        E = scene["E"][v].double().numpy()
        assert np.allclose(k, K, rtol=1e-7, atol=0) and np.allclose(e[:3, :3], E[:3, :3], atol=2e-6) and np.allclose(e[:3, 3], E[:3, 3], atol=1e-4)
        # the plane's depth at the image centre lies inside the image's depth range
        R, t = E[:3, :3], E[:3, 3]
        o, d = -R.T @ t, R.T @ np.linalg.inv(K) @ np.array([W / 2.0, H / 2.0, 1.0])
        n = np.array([-a, -c, 1.0])
        z_centre = (d0 - n @ o) / (n @ d)
        assert dmin < z_centre < dmax, (v, dmin, z_centre, dmax)
    pairs = IO.read_pair_file_scored(str(tree / "pair.txt"), 0.01)
    assert len(pairs) == V and all(len(s) >= 2 for _, s in pairs)
    out = tmp_path / "out"
    res = EV.main(["--testpath", str(tree), "--dataset", "general", "--outdir", str(out), "--method", "diffmvs", "--num_view", "3",
                   "--numdepth_initial", "16", "--noise_seed", "7", "--filter", "--geo_mask_thres", "1", "--geo_pixel_thres", "4",
                   "--geo_depth_thres", "0.05", "--photo_thres", "0.0", "0.0", "0.0"])
    assert res["views"] == V
    for v in range(V):
        dm, _ = IO.read_pfm(str(out / "depth_est" / ("%08d.pfm" % v)))
        assert dm.shape == (H, W) and np.isfinite(dm).all()
    assert os.path.getsize(res["ply"][""]) > 0 and res["fused_points"][""] > 0
