"""dmvs_depth_normals_f32 / Ops.depth_normals / the normals of fusion.filter_depth: oriented normals from a plane fitted in inverse depth.
The kernel against a numpy fp64 restatement of include/dmvs.h (tolerance ZERO: integer sums, IEEE fp64 operations in a fixed order without
contraction, correctly rounded division and square root on both sides, one rounding to fp32), every slot hit on purpose, the truth on
analytic planes and across a depth step, independence of the view chunking and of the mask's form, the argument checks, the PLY with normals
and its readers, and the fusion and eval options.  Every `ops` test runs on the host emulation here and on the MI355X under -m gpu."""
import ctypes as C
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

from conftest import emu_ops, pin_ops
from diffmvs_amd import _lib, formats as IO, fusion, synth
from diffmvs_amd.ops import Ops

H0, W0 = 37, 53                                                      # two 32 x 8 tiles across and five down, both with a ragged remainder
K0 = np.array([[60.0, 0.3, 26.0], [0.0, 58.0, 18.0], [0.0, 0.0, 1.0]])


def restate(depth, valid, cams, r, rel_jump, min_pts):
    """include/dmvs.h, the normals contract, in numpy fp64 -> (out [B,H,W,4] fp32, counts [B,4] int64, slot [B,H,W])"""
    B, H, W = depth.shape
    out, counts, slots = np.zeros((B, H, W, 4), np.float32), np.zeros((B, 4), np.int64), np.zeros((B, H, W), np.int64)
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    for v in range(B):
        K, Kinv, R = (cams[v, 9 * i:9 * i + 9].reshape(3, 3) for i in range(3))
        d = depth[v]
        with np.errstate(all="ignore"):
            usable = np.isfinite(d) & (d > 0)
            if valid is not None:
                usable &= valid[v] != 0
            w = np.where(usable, 1.0 / d.astype(np.float64), 0.0)
            pad = np.zeros((H + 2 * r, W + 2 * r))
            pad[r:r + H, r:r + W] = w
            n, Sx, Sy, Sxx, Sxy, Syy = (np.zeros((H, W), np.int64) for _ in range(6))
            Tw, Tx, Ty = (np.zeros((H, W)) for _ in range(3))
            gate = rel_jump * w
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    wj = pad[r + dy:r + dy + H, r + dx:r + dx + W]           # 0 outside the image and where the tap is not usable
                    dl = wj - w
                    take = (wj > 0) & (np.abs(dl) <= gate)
                    n, Sx, Sy = n + take, Sx + take * dx, Sy + take * dy
                    Sxx, Sxy, Syy = Sxx + take * (dx * dx), Sxy + take * (dx * dy), Syy + take * (dy * dy)
                    Tw = np.where(take, Tw + dl, Tw)
                    Tx = np.where(take, Tx + float(dx) * dl, Tx)
                    Ty = np.where(take, Ty + float(dy) * dl, Ty)
            C00, C01, C02 = Syy * n - Sy * Sy, -(Sxy * n - Sx * Sy), Sxy * Sy - Syy * Sx
            C11, C12, C22 = Sxx * n - Sx * Sx, -(Sxx * Sy - Sxy * Sx), Sxx * Syy - Sxy * Sxy
            D = Sxx * C00 + Sxy * C01 + Sx * C02
            f = lambda q: q.astype(np.float64)  # noqa: E731
            a = ((f(C00) * Tx + f(C01) * Ty) + f(C02) * Tw) / f(D)
            b = ((f(C01) * Tx + f(C11) * Ty) + f(C12) * Tw) / f(D)
            c = ((f(C02) * Tx + f(C12) * Ty) + f(C22) * Tw) / f(D)
            wf = w + c
            c0 = (wf - a * xs) - b * ys
            g = [(K[0, i] * a + K[1, i] * b) + K[2, i] * c0 for i in range(3)]
            ln = np.sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2])
            ray = [(Kinv[i, 0] * xs + Kinv[i, 1] * ys) + Kinv[i, 2] for i in range(3)]
            rl = np.sqrt((ray[0] * ray[0] + ray[1] * ray[1]) + ray[2] * ray[2])
            slot = np.where(~usable, 0, np.where((n < min_pts) | (D == 0), 1, np.where(~(wf > 0) | ~np.isfinite(ln) | (ln == 0), 2, 3)))
            nc = [-g[i] / ln for i in range(3)]
            res = [(R[0, i] * nc[0] + R[1, i] * nc[1]) + R[2, i] * nc[2] for i in range(3)] + [wf / (ln * rl)]
            for i in range(4):
                out[v, ..., i] = np.where(slot == 3, res[i], 0.0).astype(np.float32)
        slots[v], counts[v] = slot, np.bincount(slot.ravel(), minlength=4)
    return out, counts, slots


def rig(V):
    """V cameras with the skewed K0, each turned about two axes and moved: E [V,4,4] world -> camera"""
    E = np.zeros((V, 4, 4))
    for v in range(V):
        ay, ax = 0.05 * (v - 1), 0.03 * v
        Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
        E[v] = np.eye(4)
        E[v, :3, :3] = Rx @ Ry
        E[v, :3, 3] = [-30.0 * (v - 1), 4.0 * v, 2.0 * v]
    return np.repeat(K0[None], V, 0), E


def dev(ops, a):
    return None if a is None else torch.from_numpy(np.array(a)).to(ops.device)


def run(ops, depth, valid, cams, r=2, rel_jump=0.02, min_pts=5):
    out, counts = ops.depth_normals(dev(ops, depth), dev(ops, valid), cams, None, r, rel_jump, min_pts)
    assert out.dtype == torch.float32 and tuple(out.shape) == depth.shape + (4,) and counts.dtype == torch.int64
    return out.cpu().numpy(), counts.cpu().numpy()


# ------------------------------------------------------------------------------------------ 1. the contract, tolerance zero
@functools.lru_cache(maxsize=None)
def exact_inputs():
    """B = 3, 37 x 53: a smooth surface plus noise, a constant patch (so that rel_jump = 0 still fits planes), a step, planted bad pixels and
    a random mask with holes"""
    rs = np.random.RandomState(5)
    ys, xs = np.meshgrid(np.arange(H0, dtype=np.float64), np.arange(W0, dtype=np.float64), indexing="ij")
    depth = np.stack([600.0 + 40.0 * v + (1.5 + v) * xs - 2.0 * ys + 6.0 * np.sin(xs / 5.0 + v) * np.cos(ys / 7.0) for v in range(3)])
    depth += rs.normal(0.0, 0.3, depth.shape)
    depth[:, 20:31, 8:24] = 640.0
    depth[:, :, 40:] += 70.0                                          # a 10 % step: gated at rel_jump = 0.02, not at 1e6
    depth = depth.astype(np.float32)
    for k, bad in enumerate((np.nan, np.inf, 0.0, -600.0)):
        depth[:, 3 + 7 * k, 5 + 9 * k] = bad
        depth[k % 3, 30, 30 + 3 * k] = bad
    depth[1, 24, 12] = np.nan                                         # ... and one inside the constant patch
    valid = (rs.rand(3, H0, W0) > 0.15).astype(np.uint8)
    K, E = rig(3)
    cams = Ops.normal_cams(K, E)
    for a in (depth, valid, cams):
        a.setflags(write=False)
    return depth, valid, cams


@functools.lru_cache(maxsize=None)
def exact_want(r, rel_jump, masked):
    depth, valid, cams = exact_inputs()
    want = restate(depth, valid if masked else None, cams, r, rel_jump, 5)
    for a in want:
        a.setflags(write=False)
    return want


@pytest.mark.parametrize("r", [1, 2, 4])
def test_normals_and_slots_equal_the_restatement(ops, r):
    depth, valid, cams = exact_inputs()
    for rel_jump in (0.02, 0.0, 1e6):
        for masked in (True, False):
            want, counts_w, _ = exact_want(r, rel_jump, masked)
            out, counts = run(ops, depth, valid if masked else None, cams, r, rel_jump)
            bad = np.argwhere((out != want).any(-1))
            assert np.array_equal(out, want), (r, rel_jump, masked, len(bad), bad[:4], [(out[tuple(i)], want[tuple(i)]) for i in bad[:2]])
            assert np.array_equal(counts, counts_w), (r, rel_jump, masked, counts - counts_w)
            assert (counts_w.sum(1) == H0 * W0).all() and (counts_w[:, 3] > (50 if rel_jump == 0.0 else 1000)).all()      # the case is not trivial
            assert (counts_w[:, 0] >= (200 if masked else 5)).all() and (rel_jump != 0.0 or (counts_w[:, 1] > 1000).all())


# ------------------------------------------------------------------------------------------ 2. every slot, on purpose
def test_every_slot_is_hit_on_purpose(ops):
    cams = Ops.normal_cams(*rig(1))
    depth = np.full((1, H0, W0), 600.0, np.float32)
    valid = np.ones((1, H0, W0), np.uint8)
    valid[0, 5, 7] = 0                                                # slot 0: a masked centre ...
    depth[0, 5, 20] = np.nan                                          # ... and a bad one
    valid[0, 10:21, 30:51] = 0
    valid[0, 15, 30:51] = 1                                           # slot 1: a single valid row (D == 0 with n = 5 >= min_pts)
    valid[0, 24:33, 36:45] = 0
    valid[0, 28, 40] = 1                                              # slot 1: an isolated pixel (n = 1 < min_pts)
    depth[0, 0:3, 0], depth[0, 0:3, 1], depth[0, 0:3, 2] = 1.0 / 0.01, 1.0, 1.0 / 3.0      # slot 2: inverse depths 0.01, 1, 3 from the corner
    want, counts_w, slot = restate(depth, valid, cams, 2, 1e6, 5)
    assert slot[0, 5, 7] == 0 and slot[0, 5, 20] == 0
    assert (slot[0, 15, 32:49] == 1).all() and slot[0, 28, 40] == 1
    assert slot[0, 0, 0] == 2                                         # the line through (0, 0.01), (1, 1), (2, 3) meets column 0 below zero
    assert slot[0, 34, 10] == 3
    out, counts = run(ops, depth, valid, cams, 2, 1e6)
    assert np.array_equal(out, want) and np.array_equal(counts, counts_w)
    assert (counts > 0).all() and counts.sum() == H0 * W0
    assert (out[slot != 3] == 0).all() and (np.abs(np.linalg.norm(out[slot == 3][:, :3].astype(np.float64), axis=1) - 1.0) < 2e-7).all()


# ------------------------------------------------------------------------------------------ 3. truth
def plane_case(slant_deg, tilt_deg=35.0, z0=600.0):
    """a plane through (0, 0, z0) of the camera frame whose normal makes `slant` with the optical axis, seen by camera 2 of rig(3):
    -> (depth [1,H,W] fp32 (<= 0 or inf behind its horizon), cams, the world normal, cos per pixel, the world points, the camera centre)"""
    K, E = rig(3)
    K, E = K[2], E[2]
    s, t = np.deg2rad(slant_deg), np.deg2rad(tilt_deg)
    n_c = np.array([np.sin(s) * np.cos(t), np.sin(s) * np.sin(t), -np.cos(s)])      # faces the camera
    ys, xs = np.meshgrid(np.arange(H0, dtype=np.float64), np.arange(W0, dtype=np.float64), indexing="ij")
    rays = np.linalg.inv(K) @ np.stack([xs.ravel(), ys.ravel(), np.ones(H0 * W0)])
    with np.errstate(all="ignore"):
        d = (n_c[2] * z0) / (n_c @ rays)
    Rm, tv = E[:3, :3], E[:3, 3]
    X = (Rm.T @ (rays * d - tv[:, None])).T.reshape(H0, W0, 3)
    cos = (-(n_c @ rays) / np.linalg.norm(rays, axis=0)).reshape(H0, W0)
    return d.reshape(1, H0, W0).astype(np.float32), Ops.normal_cams(K[None], E[None]), Rm.T @ n_c, cos, X, -Rm.T @ tv


def angle(a, b):
    """between unit-ish vectors [...,3] and one vector, accurate at small angles"""
    a = a.astype(np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=-1), a @ b)


@pytest.mark.parametrize("slant", [0, 30, 60, 80])
def test_truth_on_analytic_planes(ops, slant):
    depth, cams, N, cos, X, centre = plane_case(float(slant))
    for r in (1, 2, 4):
        out, counts = run(ops, depth, None, cams, r, 1.0)            # (at f = 60 a slanted plane's inverse depth changes by 3 .. 10 % per pixel)
        got = out[0].reshape(-1, 4)
        has = (got[:, :3] != 0).any(1)
        assert has.sum() == counts[0, 3] > (400 if slant == 80 else 0.95 * H0 * W0), (slant, r, counts)
        n = got[has, :3].astype(np.float64)
        err, cerr = angle(n, N), np.abs(got[has, 3] - cos.ravel()[has])
        unit = np.abs(np.linalg.norm(n, axis=1) - 1.0)
        print(f"slant {slant} r {r}: {has.sum()} normals, worst angle {err.max():.3g} rad, cos {cerr.max():.3g}, |N| - 1 {unit.max():.3g}")
        assert err.max() <= 2e-5 and cerr.max() <= 5e-6 and unit.max() <= 2e-7, (slant, r, err.max(), cerr.max(), unit.max())
        assert (np.einsum("ij,ij->i", n, centre - X.reshape(-1, 3)[has]) > 0).all()


def test_the_jump_gate_keeps_a_depth_step_sharp(ops):
    """600 | 660, fronto-parallel, an unrotated camera: with the gate every normal is (0, 0, -1) EXACTLY, right up to the edge (every
    difference of inverse depths inside a support is zero); without it the two columns at the edge are off by more than 0.5 rad"""
    depth = np.full((1, H0, W0), 600.0, np.float32)
    depth[:, :, 26:] = 660.0
    E = np.eye(4)[None]
    E[0, :3, 3] = [5.0, -3.0, 2.0]
    cams = Ops.normal_cams(K0[None], E)
    sharp, counts = run(ops, depth, None, cams, 2, 0.02)
    assert counts.tolist() == [[0, 0, 0, H0 * W0]]
    assert (sharp[0, ..., :3] == np.array([0.0, 0.0, -1.0], np.float32)).all()
    blurred, _ = run(ops, depth, None, cams, 2, 1.0)
    err = angle(blurred[0, ..., :3], np.array([0.0, 0.0, -1.0]))
    print(f"without the gate: {err[:, 25:27].min():.3f} .. {err[:, 25:27].max():.3f} rad at the edge, {err[:, :23].max():.3g} away from it")
    assert err[:, 25:27].min() > 0.5 and err[:, :24].max() == 0.0 and err[:, 28:].max() == 0.0


# ------------------------------------------------------------------------------------------ 4. independence
def test_bits_do_not_depend_on_the_view_chunk_or_the_masks_form(ops):
    assert _lib.NORMAL_VIEW_CHUNK == 8
    rs = np.random.RandomState(9)
    K, E = rig(9)
    cams = Ops.normal_cams(K, E)
    ys, xs = np.meshgrid(np.arange(H0, dtype=np.float64), np.arange(W0, dtype=np.float64), indexing="ij")
    depth = np.stack([500.0 + 30.0 * v + (v - 4.0) * xs + 1.5 * ys for v in range(9)]) + rs.normal(0.0, 0.5, (9, H0, W0))
    depth = depth.astype(np.float32)
    depth[:, 7, 9] = np.nan
    valid = (rs.rand(9, H0, W0) > 0.1).astype(np.uint8)
    together, counts = run(ops, depth, valid, cams)
    for v in range(9):
        one, c1 = run(ops, depth[v:v + 1], valid[v:v + 1], cams[v:v + 1])
        assert np.array_equal(together[v].view(np.uint32), one[0].view(np.uint32)) and np.array_equal(counts[v], c1[0]), v
    assert len({together[v].tobytes() for v in range(9)}) == 9          # (every view has its own camera and depth)
    ones, c_ones = run(ops, depth, np.ones_like(valid), cams)
    null, c_null = run(ops, depth, None, cams)
    assert np.array_equal(ones.view(np.uint32), null.view(np.uint32)) and np.array_equal(c_ones, c_null)
    as_bool = ops.depth_normals(dev(ops, depth), dev(ops, valid.astype(bool)), cams, None)[0].cpu().numpy()
    assert np.array_equal(as_bool.view(np.uint32), together.view(np.uint32))


# ------------------------------------------------------------------------------------------ 5. argument checks
def test_argument_checks_return_einval_and_touch_nothing(ops):
    d = ops.device
    B, H, W = 2, 8, 12
    depth = torch.full((B, H, W), 600.0, device=d)
    valid = torch.ones((B, H, W), dtype=torch.uint8, device=d)
    out = torch.full((B, H, W, 4), 7.0, device=d)
    counts = torch.full((B, 4), -1, dtype=torch.int64, device=d)
    table = Ops.normal_cams(*rig(B))
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    base = dict(depth=P(depth), valid=P(valid), cams=table, B=B, H=H, W=W, radius=2, rel_jump=0.02, min_pts=5, out=P(out), counts=P(counts))

    def call(**kw):
        a = {**base, **kw}
        cams = None if a["cams"] is None else np.ascontiguousarray(a["cams"], np.float64).ctypes.data_as(C.c_void_p)
        return ops.lib.dll.dmvs_depth_normals_f32(a["depth"], a["valid"], cams, a["B"], a["H"], a["W"], a["radius"], a["rel_jump"], a["min_pts"],
                                                  a["out"], a["counts"], None)

    def cam(col, value):
        t = table.copy()
        t[1, col] = value
        return t
    nan, inf = float("nan"), float("inf")
    for kw in (dict(B=-1), dict(H=-1), dict(W=-1), dict(H=1 << 16, W=1 << 15), dict(depth=None), dict(cams=None), dict(out=None), dict(counts=None),
               dict(radius=0), dict(radius=5), dict(radius=-1), dict(min_pts=2), dict(min_pts=26), dict(radius=1, min_pts=10),
               dict(rel_jump=-0.01), dict(rel_jump=nan), dict(rel_jump=inf), dict(cams=cam(0, nan)), dict(cams=cam(13, inf)), dict(cams=cam(26, -inf)),
               dict(out=C.c_void_p(out.data_ptr() + 8)), dict(out=C.c_void_p(out.data_ptr() + 4)), dict(counts=C.c_void_p(counts.data_ptr() + 4))):
        assert call(**kw) == -22, kw
    # nothing to do is not an error, and nothing at all was touched so far
    assert call(B=0) == 0 and call(H=0) == 0 and call(W=0) == 0
    assert bool((out == 7.0).all()) and bool((counts == -1).all())
    assert call(B=0, radius=9) == -22                                  # (a bad argument is one even without work)
    assert call(radius=4, min_pts=81) == 0 and call(radius=1, min_pts=9) == 0 and call(rel_jump=0.0) == 0 and call(valid=None) == 0      # the limits themselves
    assert counts.cpu().tolist() == [[0, 0, 0, H * W]] * 2 and bool((out[..., 2] < 0).all())
    # the binding's own checks
    for bad in (lambda: ops.depth_normals(depth.double(), None, table, None), lambda: ops.depth_normals(depth[0], None, table, None),
                lambda: ops.depth_normals(depth, valid[:1], table, None), lambda: ops.depth_normals(depth, valid.float(), table, None),
                lambda: ops.depth_normals(depth, None, table[:1], None), lambda: ops.depth_normals(depth, None, table, None, radius=5),
                lambda: ops.depth_normals(depth, None, np.zeros((B, 3, 3)), np.zeros((B, 4, 4))), lambda: ops.depth_normals(depth, None, table, None, min_pts=2)):
        with pytest.raises(_lib.DmvsError):
            bad()
    empty, c0 = ops.depth_normals(depth[:0], None, table[:0], None)
    assert tuple(empty.shape) == (0, H, W, 4) and tuple(c0.shape) == (0, 4)
    flat, c1 = ops.depth_normals(depth[:, :0], None, table, None)
    assert tuple(flat.shape) == (B, 0, W, 4) and c1.cpu().tolist() == [[0, 0, 0, 0]] * 2


# ------------------------------------------------------------------------------------------ 6. PLY
HEADER = ("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n%s"
          "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")


def test_ply_with_and_without_normals(tmp_path, monkeypatch, capsys):
    from diffmvs_amd import cloud_eval as CE, cloud_register as CR
    ops = emu_ops()
    pin_ops(monkeypatch, ops)
    rs = np.random.RandomState(3)
    n = 500
    xyz = rs.uniform(-50.0, 50.0, (n, 3)).astype(np.float32)
    rgb = rs.randint(0, 256, (n, 3)).astype(np.uint8)
    nrm = rs.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    nrm[7] = 0.0
    plain, with_n = str(tmp_path / "plain.ply"), str(tmp_path / "normals.ply")
    IO.write_ply(plain, xyz, rgb)
    rows = b"".join(xyz[i].astype("<f4").tobytes() + rgb[i].tobytes() for i in range(n))
    assert open(plain, "rb").read() == (HEADER % (n, "")).encode("ascii") + rows
    IO.write_ply(with_n, xyz, rgb, normals=nrm)
    rows = b"".join(xyz[i].astype("<f4").tobytes() + nrm[i].astype("<f4").tobytes() + rgb[i].tobytes() for i in range(n))
    assert open(with_n, "rb").read() == (HEADER % (n, "property float nx\nproperty float ny\nproperty float nz\n")).encode("ascii") + rows
    x, c, m = IO.read_ply(with_n, with_normals=True)
    assert np.array_equal(x, xyz) and np.array_equal(c, rgb) and m.dtype == np.float32 and np.array_equal(m, nrm)
    x0, c0 = IO.read_ply(with_n)
    assert np.array_equal(x0, xyz) and np.array_equal(c0, rgb)
    x1, c1, m1 = IO.read_ply(plain, with_normals=True)
    assert np.array_equal(x1, xyz) and np.array_equal(c1, rgb) and m1 is None
    with pytest.raises(ValueError):
        IO.write_ply(with_n, xyz, rgb, normals=nrm[:-1])
    # the readers of a fused cloud see the same points in both files
    a = CE.evaluate_files(ops, plain, plain, 20.0, [1.0])
    b = CE.evaluate_files(ops, with_n, plain, 20.0, [1.0])
    assert a == b and b["accuracy"] == 0 and b["pred"]["points"] == n
    reg = [CR.main(["--pred", f, "--gt", plain, "--max_corr", "5", "--max_iter", "3", "--out_transform", str(tmp_path / "T.txt"), "--out_ply", f + ".moved.ply"])
           for f in (plain, with_n)]
    assert reg[0] == reg[1] and open(plain + ".moved.ply", "rb").read() == open(with_n + ".moved.ply", "rb").read()


# ------------------------------------------------------------------------------------------ 7. fusion and eval
def test_fusion_writes_the_restatements_normals(ops, tmp_path):
    """tests/fusion_scene.py's tree without noise or outliers.  The restatement's own worst angle to the scene plane's normal on this tree,
    measured on the CPU: 1.62e-3 rad (the averaged depth mixes the reference view's depth with bilinear samples of the source views'); the
    bound below is twice that."""
    sys.path.insert(0, os.path.dirname(__file__))
    import fusion_scene
    root = fusion_scene.build_tree(str(tmp_path / "scan"), noise=0, outliers=0)
    Hf, Wf, V = fusion_scene.H, fusion_scene.W, fusion_scene.V
    kw = dict(geo_mask_thres=2, photo_thres=[0.3, 0.4, 0.5], method="casdiffmvs", dataset="dtu", ops=ops)
    masks = lambda: {f: open(os.path.join(root, "mask", f), "rb").read() for f in sorted(os.listdir(os.path.join(root, "mask")))}  # noqa: E731
    plain, with_n, cut = (str(tmp_path / f) for f in ("plain.ply", "normals.ply", "cut.ply"))
    n0 = fusion.filter_depth(root, root, plain, **kw)
    masks0 = masks()
    assert len(masks0) == 3 * V
    stats = {}
    assert fusion.filter_depth(root, root, with_n, normals=True, stats=stats, **kw) == n0 and masks() == masks0
    xyz0, rgb0 = IO.read_ply(plain)
    xyz, rgb, nrm = IO.read_ply(with_n, with_normals=True)
    assert np.array_equal(xyz, xyz0) and np.array_equal(rgb, rgb0) and nrm.shape == (n0, 3)
    # what the restatement gives on the same averaged depth, view by view
    pairs = IO.read_pair_file(os.path.join(root, "pair.txt"), "dtu")
    view = lambda v: (np.ascontiguousarray(IO.read_pfm(os.path.join(root, f"depth_est/{v:08d}.pfm"))[0]),) + \
        IO.read_camera_parameters(os.path.join(root, f"cams/{v:08d}_cam.txt"))  # noqa: E731
    want, slots = [], np.zeros(4, np.int64)
    for ref, srcs in pairs:
        rd, rk, re_, dmax, dmin = view(ref)
        confs = [np.ascontiguousarray(IO.read_pfm(os.path.join(root, f"conf{i}/{ref:08d}.pfm"))[0]) for i in range(3)]
        _, _, final, avg = fusion.fuse_view(ops, rd, rk, re_, dmax, dmin, confs, [view(s)[:3] for s in srcs], [0.3, 0.4, 0.5], 2, 1.0, 0.01, "casdiffmvs")
        o, c, _ = restate(avg.astype(np.float32)[None], final.astype(np.uint8)[None], Ops.normal_cams(rk[None], re_[None]), 2, 0.02, 5)
        want.append(o[0][final])
        slots += c[0]
    want = np.concatenate(want)
    assert np.array_equal(nrm, want[:, :3])
    has = (want[:, :3] != 0).any(1)
    assert stats == {"slots": slots.tolist(), "no_normal": int((~has).sum()), "dropped": 0} and slots.sum() == V * Hf * Wf and has.mean() > 0.9
    # the scene plane z = d0 + a x + c y of synth.synth_view_depths(seed = 21), seen from z < d0
    rsn = np.random.RandomState(1000003 * 21 + 17)
    rsn.uniform(560.0, 760.0)
    a, c = rsn.uniform(-0.25, 0.25, 2)
    N = np.array([a, c, -1.0]) / np.sqrt(a * a + c * c + 1.0)
    err = angle(want[has, :3], N)
    print(f"fused normals: worst angle to the plane's normal {err.max():.3g} rad, cos {want[has, 3].min():.4f} .. {want[has, 3].max():.4f}")
    assert err.max() <= 2 * 1.62e-3
    # max_view_angle between the smallest and the largest cosine: exactly the restatement's points stay, the masks are the reference's
    cos = want[:, 3].astype(np.float64)
    deg = float(np.rad2deg(np.arccos(0.5 * (cos[has].min() + cos[has].max()))))
    keep = has & (cos >= np.cos(np.deg2rad(np.float64(deg))))
    assert 0.1 * n0 < keep.sum() < 0.9 * has.sum()
    stats = {}
    assert fusion.filter_depth(root, root, cut, max_view_angle=deg, stats=stats, **kw) == keep.sum() and masks() == masks0
    xyz1, rgb1, nrm1 = IO.read_ply(cut, with_normals=True)
    assert np.array_equal(xyz1, xyz0[keep]) and np.array_equal(rgb1, rgb0[keep]) and np.array_equal(nrm1, want[keep, :3])
    assert stats == {"slots": slots.tolist(), "no_normal": 0, "dropped": int((~keep).sum())}
    assert open(plain, "rb").read() != open(with_n, "rb").read()
    assert fusion.filter_depth(root, root, cut, **kw) == n0 and open(cut, "rb").read() == open(plain, "rb").read()      # the defaults: the bytes of before


def test_eval_filter_normals_reports_the_slot_totals(tmp_path, monkeypatch, capsys):
    from PIL import Image
    from diffmvs_amd import eval as EV
    pin_ops(monkeypatch, emu_ops())
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
    res = EV.main(base + ["--outdir", str(tmp_path / "b"), "--normals", "--normal_radius", "1", "--normal_jump", "0.05", "--normal_min_pts", "4"],
                  device=torch.device("cpu"))
    st = res["normals"][""]
    assert sorted(st) == ["dropped", "no_normal", "slots"] and len(st["slots"]) == 4 and sum(st["slots"]) == V * H * W and st["dropped"] == 0
    xyz, _, nrm = IO.read_ply(res["ply"][""], with_normals=True)
    assert len(xyz) == res["fused_points"][""] > 0 and nrm.shape == xyz.shape and int((~(nrm != 0).any(1)).sum()) == st["no_normal"]
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["normals"] == res["normals"]
