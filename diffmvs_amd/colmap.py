"""COLMAP import: a sparse model + its undistorted images -> the scene tree of the 'general' dataset (images/%08d.jpg,
cams/%08d_cam.txt, pair.txt) that `python -m diffmvs_amd.eval --dataset general` reads.  The counterpart of the reference's
colmap_input.py (cited below as :<lines>), with the view-selection scores computed on the GPU (dmvs_view_select_scores_f64,
csrc/view_select.hip) instead of its O(N^2 L^2) Python pair loop.

    python -m diffmvs_amd.colmap --input_folder <colmap workspace> [--output_folder <out>] [--num_src_images K]
        [--theta0 5 --sigma1 1 --sigma2 10] [--convert_format]

The input folder holds images/ and a model in sparse/ or sparse/0/ (cameras, images, points3D as .bin, else .txt).  The cam
files and pair.txt are byte-identical to the reference's for the same model (tests/test_colmap.py), with two deliberate
deviations in the scores: a triangulation cosine that rounds past +-1 is clamped (the reference writes nan), and a point at a
camera centre contributes 0 (the reference divides by zero).  Where the reference crashes (an image without a valid 3-D point,
a point id missing from points3D, an unknown camera model) this module raises a ColmapError that says what is wrong; camera
distortion parameters are ignored as in the reference (the input is COLMAP's undistorted workspace), with one warning per
camera model that has non-zero ones.  --VGGT (R2Former retrieval scores) is not part of this project.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import struct
import sys
import time
from typing import Dict, List, NamedTuple, Tuple

import numpy as np


class ColmapError(ValueError):
    pass


# :43-56 model id -> (name, number of parameters), :282-294 parameter names
CAMERA_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
                 9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12)}
CAMERA_MODEL_IDS = {name: mid for mid, (name, _) in CAMERA_MODELS.items()}
PARAM_TYPE: Dict[str, List[str]] = {
    "SIMPLE_PINHOLE": ["f", "cx", "cy"],
    "PINHOLE": ["fx", "fy", "cx", "cy"],
    "SIMPLE_RADIAL": ["f", "cx", "cy", "k"],
    "SIMPLE_RADIAL_FISHEYE": ["f", "cx", "cy", "k"],
    "RADIAL": ["f", "cx", "cy", "k1", "k2"],
    "RADIAL_FISHEYE": ["f", "cx", "cy", "k1", "k2"],
    "OPENCV": ["fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2"],
    "OPENCV_FISHEYE": ["fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4"],
    "FULL_OPENCV": ["fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6"],
    "FOV": ["fx", "fy", "cx", "cy", "omega"],
    "THIN_PRISM_FISHEYE": ["fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "sx1", "sy1"],
}
_PINHOLE_PARAMS = {"f", "fx", "fy", "cx", "cy"}


class Camera(NamedTuple):
    id: int
    model: str
    width: int
    height: int
    params: Tuple[float, ...]


class Image(NamedTuple):
    id: int
    qvec: Tuple[float, float, float, float]
    tvec: Tuple[float, float, float]
    camera_id: int
    name: str
    xys: np.ndarray              # [n,2] fp64
    point3d_ids: np.ndarray      # [n] int64, -1 = no 3-D point


class Points3D(NamedTuple):
    """points3D as arrays: row r is point ids[r]; its track is track[track_offsets[r]:track_offsets[r+1]] = (image_id, point2d_idx)"""
    ids: np.ndarray              # [P] int64
    xyz: np.ndarray              # [P,3] fp64
    rgb: np.ndarray              # [P,3] uint8
    error: np.ndarray            # [P] fp64
    track_offsets: np.ndarray    # [P+1] int64
    track: np.ndarray            # [T,2] int32


class Model(NamedTuple):
    cameras: Dict[int, Camera]
    images: List[Image]          # in file order: the position is the image's index in the output tree
    points: Points3D


# ------------------------------------------------------------------------------------------ readers (:59-232)
def _camera_model_name(model_id: int) -> str:
    if model_id not in CAMERA_MODELS:
        raise ColmapError(f"unknown COLMAP camera model id {model_id} (known: {sorted(CAMERA_MODELS)})")
    return CAMERA_MODELS[model_id][0]


def read_cameras_binary(path: str) -> Dict[int, Camera]:
    with open(path, "rb") as f:
        buf = f.read()
    (n,), o, cams = struct.unpack_from("<Q", buf, 0), 8, {}
    for _ in range(n):
        cid, mid, w, h = struct.unpack_from("<iiQQ", buf, o)
        o += 24
        name = _camera_model_name(mid)
        k = CAMERA_MODELS[mid][1]
        cams[cid] = Camera(cid, name, w, h, struct.unpack_from("<%dd" % k, buf, o))
        o += 8 * k
    return cams


def read_cameras_text(path: str) -> Dict[int, Camera]:
    cams = {}
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line and line[0] != "#":
                e = line.split()
                if e[1] not in CAMERA_MODEL_IDS:
                    raise ColmapError(f"{path}: unknown COLMAP camera model {e[1]!r} (known: {sorted(CAMERA_MODEL_IDS)})")
                cams[int(e[0])] = Camera(int(e[0]), e[1], int(e[2]), int(e[3]), tuple(float(x) for x in e[4:]))
    return cams


_XY_ID = np.dtype([("x", "<f8"), ("y", "<f8"), ("id", "<i8")])


def read_images_binary(path: str) -> List[Image]:
    with open(path, "rb") as f:
        buf = f.read()
    (n,), o, images = struct.unpack_from("<Q", buf, 0), 8, []
    for _ in range(n):
        p = struct.unpack_from("<idddddddi", buf, o)
        o += 64
        end = buf.index(b"\x00", o)
        name = buf[o:end].decode("utf-8")
        o = end + 1
        (m,) = struct.unpack_from("<Q", buf, o)
        o += 8
        a = np.frombuffer(buf, _XY_ID, m, o)
        o += 24 * m
        images.append(Image(p[0], tuple(p[1:5]), tuple(p[5:8]), p[8], name, np.stack([a["x"], a["y"]], 1), a["id"].astype(np.int64)))
    return images


def read_images_text(path: str) -> List[Image]:
    images = []
    with open(path) as f:
        while True:
            line = f.readline()
            if not line:
                break
            line = line.strip()
            if line and line[0] != "#":
                e = line.split()
                pts = f.readline().split()
                xy = np.array([float(x) for i, x in enumerate(pts) if i % 3 != 2], np.float64).reshape(-1, 2)
                ids = np.array([int(x) for x in pts[2::3]], np.int64)
                images.append(Image(int(e[0]), tuple(float(x) for x in e[1:5]), tuple(float(x) for x in e[5:8]), int(e[8]), e[9], xy, ids))
    return images


_POINT_HEAD = np.dtype([("id", "<u8"), ("xyz", "<f8", 3), ("rgb", "u1", 3), ("error", "<f8"), ("len", "<u8")])      # 51 packed bytes


def read_points3d_binary(path: str) -> Points3D:
    with open(path, "rb") as f:
        buf = f.read()
    (n,) = struct.unpack_from("<Q", buf, 0)
    starts = np.zeros(n, np.int64)
    lens = np.zeros(n, np.int64)
    o, unpack = 8, struct.Struct("<Q").unpack_from
    for r in range(n):             # the records are variable-length: one pass for the offsets, then vectorised gathers
        starts[r] = o
        (L,) = unpack(buf, o + 43)
        lens[r] = L
        o += 51 + 8 * L
    raw = np.frombuffer(buf, np.uint8)
    head = raw[starts[:, None] + np.arange(51)].copy().view(_POINT_HEAD).reshape(n)
    toff = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=toff[1:])
    first = np.repeat(starts + 51, lens) + 8 * (np.arange(int(toff[-1])) - np.repeat(toff[:-1], lens))
    track = raw[first[:, None] + np.arange(8)].copy().view("<i4").reshape(-1, 2)
    return Points3D(head["id"].astype(np.int64), head["xyz"].astype(np.float64), head["rgb"].copy(), head["error"].astype(np.float64),
                    toff, track.astype(np.int32))


def read_points3d_text(path: str) -> Points3D:
    ids, xyz, rgb, err, lens, track = [], [], [], [], [], []
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line and line[0] != "#":
                e = line.split()
                ids.append(int(e[0]))
                xyz.append([float(x) for x in e[1:4]])
                rgb.append([int(x) for x in e[4:7]])
                err.append(float(e[7]))
                t = [int(x) for x in e[8:]]
                lens.append(len(t) // 2)
                track += t
    toff = np.zeros(len(ids) + 1, np.int64)
    np.cumsum(lens, out=toff[1:])
    return Points3D(np.array(ids, np.int64), np.array(xyz, np.float64).reshape(-1, 3), np.array(rgb, np.uint8).reshape(-1, 3),
                    np.array(err, np.float64), toff, np.array(track, np.int32).reshape(-1, 2))


def read_model(path: str, ext: str) -> Model:
    if ext == ".bin":
        return Model(read_cameras_binary(os.path.join(path, "cameras.bin")), read_images_binary(os.path.join(path, "images.bin")),
                     read_points3d_binary(os.path.join(path, "points3D.bin")))
    return Model(read_cameras_text(os.path.join(path, "cameras.txt")), read_images_text(os.path.join(path, "images.txt")),
                 read_points3d_text(os.path.join(path, "points3D.txt")))


def find_model(input_folder: str) -> Tuple[str, str]:
    """-> (model directory, extension): <input>/sparse/ before COLMAP's own <input>/sparse/0/, .bin before .txt"""
    for d in (os.path.join(input_folder, "sparse"), os.path.join(input_folder, "sparse", "0")):
        for ext in (".bin", ".txt"):
            if all(os.path.isfile(os.path.join(d, n + ext)) for n in ("cameras", "images", "points3D")):
                return d, ext
    raise ColmapError(f"no COLMAP model (cameras / images / points3D .bin or .txt) in {input_folder}/sparse or {input_folder}/sparse/0")


# ------------------------------------------------------------------------------------------ writers
def write_model(model: Model, path: str, ext: str = ".bin") -> None:
    os.makedirs(path, exist_ok=True)
    cams, images, pts = model
    if ext == ".bin":
        with open(os.path.join(path, "cameras.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(cams)))
            for c in cams.values():
                f.write(struct.pack("<iiQQ", c.id, CAMERA_MODEL_IDS[c.model], c.width, c.height))
                f.write(struct.pack("<%dd" % len(c.params), *c.params))
        with open(os.path.join(path, "images.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(images)))
            for im in images:
                f.write(struct.pack("<idddddddi", im.id, *im.qvec, *im.tvec, im.camera_id))
                f.write(im.name.encode("utf-8") + b"\x00")
                a = np.zeros(len(im.point3d_ids), _XY_ID)
                a["x"], a["y"], a["id"] = im.xys[:, 0], im.xys[:, 1], im.point3d_ids
                f.write(struct.pack("<Q", len(a)) + a.tobytes())
        with open(os.path.join(path, "points3D.bin"), "wb") as f:
            f.write(struct.pack("<Q", len(pts.ids)))
            for r in range(len(pts.ids)):
                t = pts.track[pts.track_offsets[r]:pts.track_offsets[r + 1]]
                f.write(struct.pack("<QdddBBBdQ", int(pts.ids[r]), *map(float, pts.xyz[r]), *map(int, pts.rgb[r]), float(pts.error[r]), len(t)))
                f.write(np.ascontiguousarray(t, "<i4").tobytes())
        return
    with open(os.path.join(path, "cameras.txt"), "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for c in cams.values():
            f.write(" ".join([str(c.id), c.model, str(c.width), str(c.height)] + [repr(float(x)) for x in c.params]) + "\n")
    with open(os.path.join(path, "images.txt"), "w") as f:
        f.write("# Image list with two lines of data per image:\n#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n"
                "#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        for im in images:
            f.write(" ".join([str(im.id)] + [repr(float(x)) for x in im.qvec + im.tvec] + [str(im.camera_id), im.name]) + "\n")
            f.write(" ".join("%r %r %d" % (float(x), float(y), int(i)) for (x, y), i in zip(im.xys, im.point3d_ids)) + "\n")
    with open(os.path.join(path, "points3D.txt"), "w") as f:
        f.write("# 3D point list with one line of data per point:\n"
                "#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for r in range(len(pts.ids)):
            t = pts.track[pts.track_offsets[r]:pts.track_offsets[r + 1]]
            f.write(" ".join([str(int(pts.ids[r]))] + [repr(float(x)) for x in pts.xyz[r]] + [str(int(x)) for x in pts.rgb[r]] +
                             [repr(float(pts.error[r]))] + [str(int(x)) for x in t.reshape(-1)]) + "\n")


# ------------------------------------------------------------------------------------------ cameras and depth ranges (:233-371)
def quaternion_to_rotation_matrix(qvec) -> np.ndarray:
    """:233-243, the same operation order (the cam files are pinned bit for bit)"""
    return np.array([
        [1 - 2 * qvec[2] ** 2 - 2 * qvec[3] ** 2,
         2 * qvec[1] * qvec[2] - 2 * qvec[0] * qvec[3],
         2 * qvec[3] * qvec[1] + 2 * qvec[0] * qvec[2]],
        [2 * qvec[1] * qvec[2] + 2 * qvec[0] * qvec[3],
         1 - 2 * qvec[1] ** 2 - 2 * qvec[3] ** 2,
         2 * qvec[2] * qvec[3] - 2 * qvec[0] * qvec[1]],
        [2 * qvec[3] * qvec[1] - 2 * qvec[0] * qvec[2],
         2 * qvec[2] * qvec[3] + 2 * qvec[0] * qvec[1],
         1 - 2 * qvec[1] ** 2 - 2 * qvec[2] ** 2]])


def intrinsics(cameras: Dict[int, Camera], warn=True) -> Dict[int, np.ndarray]:
    """:320-333: K per camera id from the parameter table ('f' -> fx = fy); distortion parameters are ignored"""
    out, warned = {}, set()
    for cid, cam in cameras.items():
        if cam.model not in PARAM_TYPE:
            raise ColmapError(f"camera {cid}: unknown COLMAP camera model {cam.model!r}")
        names = PARAM_TYPE[cam.model]
        p = dict(zip(names, cam.params))
        if warn and cam.model not in warned and any(v != 0 for k, v in p.items() if k not in _PINHOLE_PARAMS):
            warned.add(cam.model)
            print(f"[colmap] warning: {cam.model} cameras have non-zero distortion parameters, which are ignored: "
                  "convert the undistorted COLMAP workspace (colmap image_undistorter)", file=sys.stderr)
        if "f" in names:
            p["fx"] = p["f"]
            p["fy"] = p["f"]
        out[cid] = np.array([[p["fx"], 0, p["cx"]], [0, p["fy"], p["cy"]], [0, 0, 1]])
    return out


def extrinsic(im: Image) -> np.ndarray:
    """:336-343"""
    e = np.zeros((4, 4))
    e[:3, :3] = quaternion_to_rotation_matrix(im.qvec)
    e[:3, 3] = im.tvec
    e[3, 3] = 1
    return e


def _point_rows(model: Model) -> List[np.ndarray]:
    """per image: the points3D row of every listed point id other than -1 (duplicates kept), with the errors the reference crashes on"""
    pts = model.points
    order = np.argsort(pts.ids, kind="stable")
    sorted_ids = pts.ids[order]
    rows = []
    for im in model.images:
        ids = im.point3d_ids[im.point3d_ids != -1]
        if ids.size == 0:
            raise ColmapError(f"image {im.name!r} (image_id {im.id}) lists no valid 3-D point: its depth range is undefined "
                              "(remove it from the model or re-run the reconstruction)")
        if len(sorted_ids):
            k = np.minimum(np.searchsorted(sorted_ids, ids), len(sorted_ids) - 1)
            bad = sorted_ids[k] != ids
        else:
            k, bad = np.zeros(len(ids), np.int64), np.ones(len(ids), bool)
        if np.any(bad):
            raise ColmapError(f"image {im.name!r} (image_id {im.id}) lists point3D_id {int(ids[np.argmax(bad)])}, which points3D does not contain")
        rows.append(order[k])
    return rows


def depth_ranges(model: Model, extr: List[np.ndarray], rows: List[np.ndarray]) -> List[Tuple[float, float]]:
    """:346-360: z in camera space of every listed point (multiplicity included), sorted, [zs[int(n*.01)], zs[int(n*.99)]]"""
    out = []
    for e, r in zip(extr, rows):
        p = model.points.xyz[r]
        zs = np.sort(e[2, 0] * p[:, 0] + e[2, 1] * p[:, 1] + e[2, 2] * p[:, 2] + e[2, 3])
        n = len(zs)
        out.append((float(zs[int(n * .01)]), float(zs[int(n * .99)])))
    return out


def camera_centres(extr: List[np.ndarray]) -> np.ndarray:
    """:378-379 per image: -R^T t"""
    return np.array([-np.matmul(e[:3, :3].transpose(), e[:3, 3:4])[:, 0] for e in extr], np.float64).reshape(-1, 3)


def point_image_csr(rows: List[np.ndarray], n_points: int):
    """the point -> image CSR of dmvs_view_select_scores_f64 from the images' lists: per points3D row, the images (by position)
    that list it, ascending, and how often each lists it -> offsets [P+1] int64, images [E] int32, mult [E] int32"""
    N = len(rows)
    key = np.concatenate([r.astype(np.int64) * N + i for i, r in enumerate(rows)]) if rows else np.zeros(0, np.int64)
    uniq, mult = np.unique(key, return_counts=True)
    offsets = np.zeros(n_points + 1, np.int64)
    np.cumsum(np.bincount(uniq // N, minlength=n_points), out=offsets[1:])
    return offsets, (uniq % N).astype(np.int32), mult.astype(np.int32)


def view_scores(ops, model: Model, centres: np.ndarray, rows: List[np.ndarray], theta0=5.0, sigma1=1.0, sigma2=10.0) -> np.ndarray:
    """:374-411's score matrix [N,N] fp64 through the kernel.  Pair (i, j), i < j, counts a point once per entry in image i's list
    (the lower index), image j only has to contain it; deviations (clamped cosine, point at a camera centre) in the module docstring."""
    import torch
    offsets, imgs, mult = point_image_csr(rows, len(model.points.ids))
    dev = ops.device
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    s = ops.view_scores(t(model.points.xyz), t(offsets), t(imgs), t(mult), t(centres), theta0, sigma1, sigma2)
    return s.cpu().numpy()


def select_views(score: np.ndarray, num_src_images: int) -> List[List[Tuple[int, float]]]:
    """:404-411: the reference's own argsort call, so that exact ties order the same way; k < 0 -> every view (itself included)"""
    k = score.shape[0] if num_src_images < 0 else num_src_images
    return [[(int(j), score[i, j]) for j in np.argsort(score[i])[::-1][:k]] for i in range(score.shape[0])]


def write_cam(path: str, e: np.ndarray, K: np.ndarray, depth_range: Tuple[float, float]) -> None:
    """:421-436"""
    with open(path, "w") as f:
        f.write("extrinsic\n")
        for j in range(4):
            for k in range(4):
                f.write(str(e[j, k]) + " ")
            f.write("\n")
        f.write("\nintrinsic\n")
        for j in range(3):
            for k in range(3):
                f.write(str(K[j, k]) + " ")
            f.write("\n")
        f.write("\n%f %f \n" % (depth_range[0], depth_range[1]))


def write_pair(path: str, view_sel: List[List[Tuple[int, float]]]) -> None:
    """:438-444"""
    with open(path, "w") as f:
        f.write("%d\n" % len(view_sel))
        for i, sel in enumerate(view_sel):
            f.write("%d\n%d " % (i, len(sel)))
            for image_id, s in sel:
                f.write("%d %f " % (image_id, s))
            f.write("\n")


def convert(input_folder: str, output_folder: str = "", num_src_images: int = -1, theta0: float = 5.0, sigma1: float = 1.0,
            sigma2: float = 10.0, convert_format: bool = False, ops=None, copy_images: bool = True) -> dict:
    """colmap_input.py's __main__ without --VGGT: -> a summary {num_images, num_points, terms, seconds per phase}"""
    if not input_folder or not os.path.isdir(input_folder):
        raise ColmapError(f"invalid input folder {input_folder!r}")
    output_folder = output_folder or input_folder
    if ops is None:
        from .ops import Ops
        ops = Ops.for_device("cuda")
    t0 = time.perf_counter()
    model = read_model(*find_model(input_folder))
    t1 = time.perf_counter()
    K = intrinsics(model.cameras)
    for im in model.images:
        if im.camera_id not in K:
            raise ColmapError(f"image {im.name!r} (image_id {im.id}) uses camera {im.camera_id}, which cameras does not contain")
    extr = [extrinsic(im) for im in model.images]
    rows = _point_rows(model)
    ranges = depth_ranges(model, extr, rows)
    centres = camera_centres(extr)
    t2 = time.perf_counter()
    score = view_scores(ops, model, centres, rows, theta0, sigma1, sigma2)
    t3 = time.perf_counter()
    view_sel = select_views(score, num_src_images)
    cam_dir, img_dir = os.path.join(output_folder, "cams"), os.path.join(output_folder, "images")
    os.makedirs(cam_dir, exist_ok=True)
    os.makedirs(img_dir, exist_ok=True)
    for i, im in enumerate(model.images):
        write_cam(os.path.join(cam_dir, "%08d_cam.txt" % i), extr[i], K[im.camera_id], ranges[i])
    write_pair(os.path.join(output_folder, "pair.txt"), view_sel)
    t4 = time.perf_counter()
    if copy_images:      # :446-451 (--convert_format re-encodes through PIL at OpenCV's default JPEG quality, 95)
        for i, im in enumerate(model.images):
            src, dst = os.path.join(input_folder, "images", im.name), os.path.join(img_dir, "%08d.jpg" % i)
            if convert_format:
                from PIL import Image as PILImage
                PILImage.open(src).convert("RGB").save(dst, "JPEG", quality=95)
            else:
                shutil.copyfile(src, dst)
    t5 = time.perf_counter()
    return {"num_images": len(model.images), "num_points": len(model.points.ids), "read_s": t1 - t0, "cameras_s": t2 - t1,
            "scores_s": t3 - t2, "write_s": t4 - t3, "images_s": t5 - t4}


def main(argv=None) -> dict:
    ap = argparse.ArgumentParser(description="Convert a COLMAP sparse model into the 'general' scene tree of diffmvs_amd.eval")
    ap.add_argument("--input_folder", type=str, help="COLMAP workspace: images/ and sparse/ (or sparse/0/)")
    ap.add_argument("--output_folder", type=str, default="", help="output tree (default: the input folder)")
    ap.add_argument("--num_src_images", type=int, default=-1, help="views listed per image in pair.txt (< 0: all, itself included)")
    ap.add_argument("--theta0", type=float, default=5)
    ap.add_argument("--sigma1", type=float, default=1)
    ap.add_argument("--sigma2", type=float, default=10)
    ap.add_argument("--convert_format", action="store_true", default=False, help="re-encode the images as JPEG instead of copying them")
    ap.add_argument("--VGGT", action="store_true", default=False, help="not supported here (R2Former retrieval scores)")
    ap.add_argument("--checkpoint", type=str, default=None, help="not supported here (R2Former checkpoint)")
    a = ap.parse_args(argv)
    if a.VGGT or a.checkpoint:
        raise SystemExit("--VGGT / --checkpoint: R2Former retrieval scoring is not part of diffmvs_amd; "
                         "views are selected from the COLMAP points' triangulation angles")
    res = convert(a.input_folder, a.output_folder, a.num_src_images, a.theta0, a.sigma1, a.sigma2, a.convert_format)
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    try:
        main()
    except ColmapError as e:
        raise SystemExit(f"diffmvs_amd.colmap: {e}")
