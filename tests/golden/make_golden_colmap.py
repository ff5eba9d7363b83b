#!/usr/bin/env python3
"""DEV-ONLY fixture generator for the COLMAP import (diffmvs_amd.colmap).  Runs only where /root/reference is mounted.

Writes small binary COLMAP models with diffmvs_amd.colmap.write_model and runs the reference's own colmap_input.py on each
(as __main__, through runpy) with a stand-in cv2 module -- the only import it cannot satisfy here; the byte-copy leg of the
image step never touches it.  Recorded in colmap.npz, data only:
  <m>.cameras.bin / <m>.images.bin / <m>.points3D.bin   the input bytes (uint8)
  <m>.model                                            the same model as JSON (what the readers must parse the bytes into)
  <m>.k<K>.pair / <m>.k<K>.cam<i>                       the reference's pair.txt and cam files for --num_src_images K
The models cover PINHOLE and SIMPLE_RADIAL cameras, -1 entries, a point id listed twice by one image, points seen by one image
only, and an image order that differs from image_id order; their geometry gives no NaN score and no two different scores of
one row that print the same %f."""
import contextlib
import io
import json
import os
import runpy
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, ROOT)
from diffmvs_amd import colmap as CM  # noqa: E402

KS = (-1, 3)


def rot_to_quat(R):
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    x = np.copysign(np.sqrt(max(0.0, 1.0 + R[0, 0] - R[1, 1] - R[2, 2])) / 2.0, R[2, 1] - R[1, 2])
    y = np.copysign(np.sqrt(max(0.0, 1.0 - R[0, 0] + R[1, 1] - R[2, 2])) / 2.0, R[0, 2] - R[2, 0])
    z = np.copysign(np.sqrt(max(0.0, 1.0 - R[0, 0] - R[1, 1] + R[2, 2])) / 2.0, R[1, 0] - R[0, 1])
    q = np.array([w, x, y, z])
    return q / np.linalg.norm(q)


def look_at(c, target=np.zeros(3)):
    z = target - c
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z])        # world -> camera rotation


def make_model(seed, n_images, n_points, cams, radius, spread):
    rs = np.random.RandomState(seed)
    image_ids = rs.permutation(np.arange(1, n_images + 1) * 3 + 1)           # file order != image_id order
    xyz = rs.uniform(-spread, spread, (n_points, 3))
    point_ids = rs.permutation(np.arange(n_points) * 7 + 11)
    images, tracks = [], {int(p): [] for p in point_ids}
    for k in range(n_images):
        ang = 2 * np.pi * k / n_images * 0.35 + rs.uniform(-0.05, 0.05)
        c = np.array([radius * np.sin(ang), rs.uniform(-0.5, 0.5), -radius * np.cos(ang)])
        R = look_at(c, rs.uniform(-0.2, 0.2, 3))
        q = rot_to_quat(R)
        Rq = CM.quaternion_to_rotation_matrix(q)
        t = -Rq @ c
        seen = np.nonzero(rs.uniform(size=n_points) < 0.55)[0]
        ids = [int(point_ids[r]) for r in seen]
        if k == 1:
            ids.insert(3, ids[0])               # one point listed twice by one image
        for j in rs.choice(len(ids) + 1, 4):
            ids.insert(int(j), -1)              # keypoints without a 3-D point
        for j, pid in enumerate(ids):
            if pid != -1:
                tracks[pid].append((int(image_ids[k]), j))
        xys = rs.uniform(0, 640, (len(ids), 2))
        images.append(CM.Image(int(image_ids[k]), tuple(map(float, q)), tuple(map(float, t)), cams[k % len(cams)].id, "img_%03d.png" % k,
                               xys, np.array(ids, np.int64)))
    lens = [len(tracks[int(p)]) for p in point_ids]
    toff = np.zeros(n_points + 1, np.int64)
    np.cumsum(lens, out=toff[1:])
    track = np.array([t for p in point_ids for t in tracks[int(p)]], np.int32).reshape(-1, 2)
    pts = CM.Points3D(point_ids.astype(np.int64), xyz, rs.randint(0, 256, (n_points, 3)).astype(np.uint8), rs.uniform(0, 2, n_points),
                      toff, track)
    return CM.Model({c.id: c for c in cams}, images, pts)


def model_json(m):
    return json.dumps({"cameras": [[c.id, c.model, c.width, c.height, list(c.params)] for c in m.cameras.values()],
                       "images": [[im.id, list(im.qvec), list(im.tvec), im.camera_id, im.name, im.xys.tolist(), im.point3d_ids.tolist()]
                                  for im in m.images],
                       "points": [m.points.ids.tolist(), m.points.xyz.tolist(), m.points.rgb.tolist(), m.points.error.tolist(),
                                  m.points.track_offsets.tolist(), m.points.track.tolist()]})


def run_reference(model, k, tmp):
    root = os.path.join(tmp, "in")
    if not os.path.isdir(root):
        CM.write_model(model, os.path.join(root, "sparse"), ".bin")
        os.makedirs(os.path.join(root, "images"))
        for im in model.images:
            with open(os.path.join(root, "images", im.name), "wb") as f:
                f.write(b"not an image")
    out = os.path.join(tmp, "out%d" % k)
    sys.modules["cv2"] = types.ModuleType("cv2")
    argv = sys.argv
    sys.argv = ["colmap_input.py", "--input_folder", root, "--output_folder", out, "--num_src_images", str(k)]
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            runpy.run_path(os.path.join(REF, "colmap_input.py"), run_name="__main__")
    finally:
        sys.argv = argv
    pair = open(os.path.join(out, "pair.txt")).read()
    cams = [open(os.path.join(out, "cams", "%08d_cam.txt" % i)).read() for i in range(len(model.images))]
    return root, pair, cams


def check_scores(pair):
    """no nan, and within a row no two different scores that print alike"""
    lines = pair.splitlines()
    for ln in lines[2::2]:
        s = [float(x) for x in ln.split()[2::2]]
        assert all(np.isfinite(s)), ln
        assert len(set(s)) == len(s) or all(s.count(v) == 1 or v == 0.0 for v in s), ln


def main():
    models = {
        "a": make_model(5, 7, 48, [CM.Camera(1, "PINHOLE", 640, 480, (500.0, 510.0, 320.0, 240.0)),
                                   CM.Camera(2, "SIMPLE_RADIAL", 640, 480, (505.5, 321.0, 239.0, 0.012))], 6.0, 1.5),
        "b": make_model(9, 4, 30, [CM.Camera(1, "SIMPLE_RADIAL", 800, 600, (620.25, 400.0, 300.0, 0.0))], 9.0, 3.0),
    }
    out = {"meta": np.array(json.dumps({"models": sorted(models), "ks": list(KS)}))}
    for name, m in models.items():
        with tempfile.TemporaryDirectory() as tmp:
            for k in KS:
                root, pair, cams = run_reference(m, k, tmp)
                check_scores(pair)
                out[f"{name}.k{k}.pair"] = np.array(pair)
                for i, c in enumerate(cams):
                    out[f"{name}.k{k}.cam{i}"] = np.array(c)
            for f in ("cameras", "images", "points3D"):
                out[f"{name}.{f}.bin"] = np.frombuffer(open(os.path.join(root, "sparse", f + ".bin"), "rb").read(), np.uint8)
        out[f"{name}.model"] = np.array(model_json(m))
    path = os.path.join(HERE, "colmap.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
