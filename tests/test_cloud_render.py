"""dmvs_cloud_splat_zmin_f32 / dmvs_cloud_splat_sum_f32 / diffmvs_amd.cloud_render: depth maps rendered from a cloud.  The z-buffer, the slots,
the fixed-point sums and the resolved mean against a numpy fp64 restatement of include/dmvs.h (tolerance ZERO: every per-point operation is an
IEEE fp64 one, correctly rounded on both sides, without contraction; np.minimum into an fp32 buffer; np.rint = llrint), their independence of
the grid, of the order of the points and of the view chunking, the truth on an analytic plane, occlusion, the argument checks, and the command
line into the readers of a depth_gt/ tree.  Every `ops` test runs on the host emulation here and on the MI355X under -m gpu."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from conftest import emu_ops, hip_ops, pin_ops
from diffmvs_amd import _lib, cloud_render as R, formats as IO, synth
from diffmvs_amd.cloud_grid import pow2_scale_below

H0, W0 = 37, 53
K0 = np.array([[60.0, 0.0, 26.0], [0.0, 60.0, 18.0], [0.0, 0.0, 1.0]])


def restate(points, table, H, W, radius, r_min, r_max, tau=None, scale=None):
    """include/dmvs.h, the splat contract, in numpy fp64 -> (zbuf [V,H,W] fp32, counts [V,4] int64[, sum int64, cnt int32 with tau])"""
    X, Y, Z = (points[:, i].astype(np.float64) for i in range(3))
    fin = np.isfinite(X) & np.isfinite(Y) & np.isfinite(Z)
    V = table.shape[0]
    zbuf, counts = np.full((V, H, W), np.inf, np.float32), np.zeros((V, 4), np.int64)
    total, cnt = np.zeros((V, H, W), np.int64), np.zeros((V, H, W), np.int32)
    for k, q in enumerate(table):
        with np.errstate(all="ignore"):
            x = ((q[0] * X + q[1] * Y) + q[2] * Z) + q[3]
            y = ((q[4] * X + q[5] * Y) + q[6] * Z) + q[7]
            z = ((q[8] * X + q[9] * Y) + q[10] * Z) + q[11]
            inr = fin & (z > q[13]) & (z <= q[14])
            u, v = x / z, y / z
            raw = radius * q[12] / z
            r = np.fmin(np.fmax(raw, r_min), r_max)
            c0, c1 = np.fmax(np.ceil(u - r), 0.0), np.fmin(np.floor(u + r), float(W - 1))
            r0, r1 = np.fmax(np.ceil(v - r), 0.0), np.fmin(np.floor(v + r), float(H - 1))
            on = inr & np.isfinite(u) & np.isfinite(v) & (c0 <= c1) & (r0 <= r1)
            z32 = z.astype(np.float32)
        counts[k] = [(~fin).sum(), (fin & ~inr).sum(), (inr & ~on).sum(), (on & (raw > r_max)).sum()]
        idx = np.nonzero(on)[0]
        box = [(int(r0[i]), int(r1[i]) + 1, int(c0[i]), int(c1[i]) + 1) for i in idx]
        for i, (a, b, c, d) in zip(idx, box):
            np.minimum(zbuf[k, a:b, c:d], z32[i], out=zbuf[k, a:b, c:d])
        if tau is None:
            continue
        fixed = np.rint(z32[idx].astype(np.float64) * scale).astype(np.int64)
        for i, f, (a, b, c, d) in zip(idx, fixed, box):
            m = np.float64(z32[i]) <= zbuf[k, a:b, c:d].astype(np.float64) * (1.0 + tau)
            total[k, a:b, c:d][m] += f
            cnt[k, a:b, c:d][m] += 1
    return (zbuf, counts) if tau is None else (zbuf, counts, total, cnt)


def restate_mean(total, cnt, scale):
    with np.errstate(all="ignore"):
        return np.where(cnt > 0, (total.astype(np.float64) / cnt.astype(np.float64)) / scale, 0.0).astype(np.float32)


def rig(V):
    """V cameras 30 apart, each turned 0.05 rad per step, looking down +z: K0 at 53 x 37"""
    E = np.zeros((V, 4, 4))
    for v in range(V):
        a = 0.05 * (v - 1)
        E[v] = np.eye(4)
        E[v, :3, :3] = [[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]]
        E[v, :3, 3] = [-30.0 * (v - 1), 4.0 * (v - 1), 0.0]
    return np.repeat(K0[None], V, 0), E


# view 1 of rig(3) is the identity: u = 60 X / Z + 26, v = 60 Y / Z + 18; with radius 10 a point at Z = 600 has r = 1
PLANTED = np.array([[np.nan, 0.0, 600.0],          # slot 0
                    [0.0, 0.0, -600.0],            # behind the camera: slot 1
                    [0.0, 0.0, 5000.0],            # beyond far = 1000: slot 1
                    [10000.0, 0.0, 600.0],         # u = 1026: slot 2
                    [-263.0, 0.0, 600.0],          # u = -0.3: columns -1 .. 0 -> 0 (left border)
                    [263.0, 0.0, 600.0],           # u = 52.3: columns 52 .. 53 -> 52 (right border)
                    [0.0, -183.0, 600.0],          # v = -0.3 (top border)
                    [0.0, 183.0, 600.0],           # v = 36.3 (bottom border)
                    [0.0, 0.0, 60.0]], np.float32)  # radius * f / z = 10 > r_max = 4: slot 3, a 9 x 9 footprint
RADIUS, R_MIN, R_MAX, NEAR, FAR = 10.0, 0.5, 4.0, 1.0, 1000.0
TAU = 0.25                     # the slab is 800 deep: a quarter of the nearest depth puts several points into most pixels' means


@pytest.fixture(scope="module")
def exact_case():
    """V = 3, 37 x 53, N = 20 011 (79 workgroups with a ragged tail): a random slab that spills over every border, plus the planted points"""
    rs = np.random.RandomState(11)
    n = 20011 - len(PLANTED)
    pts = np.stack([rs.uniform(-420.0, 420.0, n), rs.uniform(-300.0, 300.0, n), rs.uniform(300.0, 1100.0, n)], 1).astype(np.float32)
    pts = np.concatenate([pts[:7000], PLANTED, pts[7000:]])
    K, E = rig(3)
    table = R.view_table(K, E, NEAR, FAR)
    scale = pow2_scale_below(FAR, len(pts))
    want = restate(pts, table, H0, W0, RADIUS, R_MIN, R_MAX, tau=TAU, scale=scale)
    for a in want:
        a.setflags(write=False)
    return pts, table, scale, want


def dev(ops, a):
    return torch.from_numpy(np.array(a)).to(ops.device)


def bits(t):
    return (t.cpu().numpy() if torch.is_tensor(t) else t).view(np.uint32)


def test_zmin_bits_and_slots_equal_the_restatement(ops, exact_case):
    pts, table, _, (zbuf_w, counts_w, _, _) = exact_case
    zbuf, counts = ops.cloud_splat_zmin(dev(ops, pts), table, (H0, W0), RADIUS, R_MIN, R_MAX)
    assert zbuf.dtype == torch.float32 and tuple(zbuf.shape) == (3, H0, W0) and counts.dtype == torch.int64
    assert np.array_equal(bits(zbuf), bits(zbuf_w)) and np.array_equal(counts.cpu().numpy(), counts_w), counts.cpu().numpy() - counts_w
    assert np.isfinite(zbuf_w).mean() > 0.5 and (counts_w[:, 1:3] > 100).all()           # the case is not trivial
    # the planted points alone, in the identity view: each in its slot, the border points on their border, the near one clamped to 9 x 9
    z1, c1 = ops.cloud_splat_zmin(dev(ops, PLANTED), table[1:2], (H0, W0), RADIUS, R_MIN, R_MAX)
    z1 = z1.cpu().numpy()[0]
    assert c1.cpu().tolist() == [[1, 2, 1, 1]]
    seen = np.isfinite(z1)
    assert seen.sum() == 4 * 3 + 81 and (z1[seen & (z1 > 100)] == 600.0).all()
    assert seen[17:20, 0].all() and not seen[17:20, 1].any() and seen[17:20, 52].all() and seen[0, 25:28].all() and seen[36, 25:28].all()
    assert (z1[14:23, 22:31] == 60.0).all() and not seen[13, 22:31].any()
    assert np.array_equal(bits(z1), bits(restate(PLANTED, table[1:2], H0, W0, RADIUS, R_MIN, R_MAX)[0][0]))
    # work: footprint pixels visited; without the pre-test every one of them is an atomic, with it no more than that
    _, _, wk = ops.cloud_splat_zmin(dev(ops, PLANTED), table[1:2], (H0, W0), RADIUS, R_MIN, R_MAX, pretest=False, work=True)
    assert wk.cpu().tolist() == [93, 93]
    z2, _, wk = ops.cloud_splat_zmin(dev(ops, PLANTED), table[1:2], (H0, W0), RADIUS, R_MIN, R_MAX, work=True)
    assert wk.cpu().tolist() == [93, 93] and np.array_equal(bits(z2[0]), bits(z1))       # (no two of these footprints overlap)


def test_sum_integers_and_the_mean_equal_the_restatement(ops, exact_case):
    pts, table, scale, (zbuf_w, _, total_w, cnt_w) = exact_case
    total, cnt = ops.cloud_splat_sum(dev(ops, pts), table, (H0, W0), RADIUS, R_MIN, R_MAX, dev(ops, zbuf_w), TAU, scale)
    assert total.dtype == torch.int64 and cnt.dtype == torch.int32
    assert np.array_equal(cnt.cpu().numpy(), cnt_w) and np.array_equal(total.cpu().numpy(), total_w)
    assert cnt_w.max() > 3 and ((cnt_w > 0) == np.isfinite(zbuf_w)).all()
    mean = R.resolve_mean(total, cnt, scale)
    assert mean.dtype == torch.float32 and np.array_equal(bits(mean), bits(restate_mean(total_w, cnt_w, scale)))
    # ... and through render_depth with the same range: the same maps in both modes
    K, E = rig(3)
    res = R.render_depth(ops, pts, K, E, (H0, W0), radius=RADIUS, r_min=R_MIN, r_max=R_MAX, depth_range=(NEAR, FAR), tau=TAU)
    assert np.array_equal(bits(res["depth"]), bits(mean)) and np.array_equal(res["count"].cpu().numpy(), cnt_w) and res["radius"] == RADIUS
    assert np.array_equal(res["mask"].cpu().numpy(), cnt_w > 0)
    near = R.render_depth(ops, pts, K, E, (H0, W0), radius=RADIUS, r_min=R_MIN, r_max=R_MAX, depth_range=(NEAR, FAR), mode="nearest")
    assert np.array_equal(bits(near["depth"]), bits(np.where(np.isinf(zbuf_w), np.float32(0), zbuf_w))) and "count" not in near


def test_bits_do_not_depend_on_grid_order_or_sorting(ops, exact_case):
    pts, table, scale, (zbuf_w, counts_w, total_w, cnt_w) = exact_case
    K, E = rig(3)
    perm = np.random.RandomState(12).permutation(len(pts))
    mean_w = restate_mean(total_w, cnt_w, scale)
    for mode, want in (("mean", mean_w), ("nearest", np.where(np.isinf(zbuf_w), np.float32(0), zbuf_w))):
        for cloud, sort, blocks in ((pts, False, 1), (pts, False, 7), (pts, False, 0), (pts[perm], False, 0), (pts, True, 0), (pts[perm], True, 7)):
            res = R.render_depth(ops, cloud, K, E, (H0, W0), radius=RADIUS, r_min=R_MIN, r_max=R_MAX, depth_range=(NEAR, FAR), mode=mode, tau=TAU,
                                 sort=sort, blocks=blocks)
            assert np.array_equal(bits(res["depth"]), bits(want)), (mode, sort, blocks)
            assert np.array_equal(res["counts"].cpu().numpy(), counts_w)
            assert mode == "nearest" or np.array_equal(res["count"].cpu().numpy(), cnt_w)
        res = R.render_depth(ops, pts[perm], K, E, (H0, W0), radius=RADIUS, r_min=R_MIN, r_max=R_MAX, depth_range=(NEAR, FAR), mode=mode, tau=TAU,
                             pretest=False)                    # every footprint pixel an atomic, no load in front of it
        assert np.array_equal(bits(res["depth"]), bits(want)) and np.array_equal(res["counts"].cpu().numpy(), counts_w), mode
    # more views than one launch carries (DMVS_SPLAT_VIEW_CHUNK = 8): eleven in one call against one call per view
    assert _lib.SPLAT_VIEW_CHUNK < 11
    K11, E11 = rig(11)
    kw = dict(radius=RADIUS, r_min=R_MIN, r_max=R_MAX, depth_range=(NEAR, FAR), tau=TAU)
    together = R.render_depth(ops, pts, K11, E11, (H0, W0), **kw)
    for v in range(11):
        one = R.render_depth(ops, pts, K11[v:v + 1], E11[v:v + 1], (H0, W0), **kw)
        assert np.array_equal(bits(together["depth"][v]), bits(one["depth"][0])) and torch.equal(together["count"][v], one["count"][0]), v
        assert torch.equal(together["counts"][v], one["counts"][0]), v
    assert np.array_equal(bits(together["depth"][:3]), bits(mean_w)) and int(together["mask"][10].sum()) > 0


# ------------------------------------------------------------------------------------------ a plane, and something in front of it
PH, PW, PV = 48, 64, 5


@pytest.fixture(scope="module")
def scene():
    sc = synth.synth_scene(PH, PW, n_views=PV, n_src=2, seed=3, grid_w=3)
    return sc, sc["K"].double().numpy(), sc["E"].double().numpy()


def lattice(spacing, x0, x1, y0, y1, lift=0.0, seed=0):
    """points of the plane of synth.scene_plane(3) (moved `lift` towards the cameras) on a jittered lattice (+- 0.3 spacing)"""
    d0, a, c = synth.scene_plane(3)
    rs = np.random.RandomState(seed)
    xs, ys = np.meshgrid(np.arange(x0, x1, spacing, dtype=np.float64), np.arange(y0, y1, spacing, dtype=np.float64), indexing="ij")
    x = xs.ravel() + rs.uniform(-0.3, 0.3, xs.size) * spacing
    y = ys.ravel() + rs.uniform(-0.3, 0.3, xs.size) * spacing
    return np.stack([x, y, d0 - lift + a * x + c * y], 1).astype(np.float32)


@pytest.fixture(scope="module")
def back_plane():
    pts = lattice(2.0, -450, 450, -350, 350)
    assert len(pts) == 157500
    return pts


def plane_depth(K, E, cols, rows):
    """camera-frame depth of the ray through pixel (col, row) where it meets the plane, analytically"""
    d0, a, c = synth.scene_plane(3)
    n = np.array([-a, -c, 1.0])
    Rm, t = E[:3, :3], E[:3, 3]
    o = -Rm.T @ t
    d = Rm.T @ (np.linalg.inv(K) @ np.stack([cols.ravel(), rows.ravel(), np.ones(cols.size)]))
    return ((d0 - n @ o) / (n @ d)).reshape(cols.shape)


def test_truth_on_a_plane(ops, scene, back_plane):
    """every pixel sees the plane within r pixels' worth of its slope (a splatted point lies within r of the centre in both directions), and
    the mean of the front points is much closer than their minimum"""
    _, K, E = scene
    res = {m: R.render_depth(ops, back_plane, K, E, (PH, PW), radius=2.0, r_min=0.5, r_max=4.0, mode=m) for m in ("mean", "nearest")}
    rows, cols = np.meshgrid(np.arange(0.0, PH), np.arange(0.0, PW), indexing="ij")
    mae = {m: [] for m in res}
    for v in range(PV):
        truth = plane_depth(K[v], E[v], cols, rows)
        r_used = max(0.5, min(4.0, 2.0 * K[v, 0, 0] / truth.min()))
        bound = r_used * (np.abs(np.diff(truth, axis=1)).max() + np.abs(np.diff(truth, axis=0)).max()) + 935.0 * 2.0 ** -23
        for m in res:
            d = res[m]["depth"][v].cpu().numpy().astype(np.float64)
            assert (d > 0).all(), (m, v)
            err = np.abs(d - truth)
            print(f"{m} view {v}: max error {err.max():.4f} (bound {bound:.4f}), mean {err.mean():.4f}")
            assert err.max() <= bound, (m, v, err.max(), bound)
            mae[m].append(err.mean())
    assert np.mean(mae["mean"]) < 0.5 * np.mean(mae["nearest"]), mae
    assert int(res["mean"]["counts"][:, :2].sum()) == 0 and int(res["mean"]["counts"][:, 2].min()) > 0


def test_occlusion(ops, scene, back_plane):
    _, K, E = scene
    kw = dict(r_min=0.5, r_max=4.0, depth_range=(100.0, 2000.0))
    for mode in ("mean", "nearest"):
        dense = lattice(2.0, -60, 400, -300, 300, lift=120.0, seed=1)
        alone = R.render_depth(ops, dense, K, E, (PH, PW), radius=2.0, mode=mode, **kw)["depth"].cpu().numpy()
        back = R.render_depth(ops, back_plane, K, E, (PH, PW), radius=2.0, mode=mode, **kw)["depth"].cpu().numpy()
        joint = R.render_depth(ops, np.concatenate([back_plane, dense]), K, E, (PH, PW), radius=2.0, mode=mode, **kw)["depth"].cpu().numpy()
        cov = alone > 0
        assert 0.5 < cov[0].mean() < 0.8
        assert np.array_equal(bits(joint)[cov], bits(alone)[cov]) and np.array_equal(bits(joint)[~cov], bits(back)[~cov])
    # a sparse occluder: with half-pixel splats the plane behind shows through; with its spacing as the world-space radius it does not
    sparse = lattice(14.0, -60, 400, -300, 300, lift=120.0, seed=2)
    both = np.concatenate([back_plane, sparse])
    foot = R.render_depth(ops, sparse, K, E, (PH, PW), radius=14.0, **kw)["depth"].cpu().numpy()
    inside = foot > 0
    thin = R.render_depth(ops, both, K, E, (PH, PW), radius=0.0, **kw)["depth"].cpu().numpy()
    wide = R.render_depth(ops, both, K, E, (PH, PW), radius=14.0, **kw)["depth"].cpu().numpy()
    shows_thin, shows_wide = (thin > foot + 60.0) & inside, (wide > foot + 60.0) & inside
    print(f"behind a sparse occluder: {shows_thin.sum() / inside.sum():.3f} of its pixels show the back plane at radius 0, {shows_wide.sum()} pixels at radius 14")
    assert inside.mean() > 0.4 and shows_thin.sum() > 0.5 * inside.sum() and shows_wide.sum() == 0


# ------------------------------------------------------------------------------------------ argument checks
def test_argument_checks_return_einval_and_touch_nothing(ops):
    d = ops.device
    pts = torch.rand(64, 3, device=d) + torch.tensor([0.0, 0.0, 500.0], device=d)
    K, E = rig(2)
    table = R.view_table(K, E, NEAR, FAR)
    H, W = 8, 12
    zbuf = torch.full((2, H, W), 7.0, device=d)
    counts = torch.full((2, 4), -1, dtype=torch.int64, device=d)
    total = torch.full((2, H, W), -1, dtype=torch.int64, device=d)
    cnt = torch.full((2, H, W), -1, dtype=torch.int32, device=d)
    scale = pow2_scale_below(FAR, 64)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    base = dict(points=P(pts), N=64, transform=None, views=table, V=2, H=H, W=W, radius=2.0, r_min=0.5, r_max=4.0, flags=0, blocks=0,
                zbuf=P(zbuf), counts=P(counts), work=None, tau=0.01, scale=scale, sum=P(total), cnt=P(cnt))

    def call(which, **kw):
        a = {**base, **kw}
        views = None if a["views"] is None else np.ascontiguousarray(a["views"], np.float64).ctypes.data_as(C.c_void_p)
        head = (a["points"], a["N"], a["transform"], views, a["V"], a["H"], a["W"], a["radius"], a["r_min"], a["r_max"])
        if which == "zmin":
            return ops.lib.dll.dmvs_cloud_splat_zmin_f32(*head, a["flags"], a["blocks"], a["zbuf"], a["counts"], a["work"], None)
        return ops.lib.dll.dmvs_cloud_splat_sum_f32(*head, a["tau"], a["scale"], a["blocks"], a["zbuf"], a["sum"], a["cnt"], None)

    def view(col, value):
        t = table.copy()
        t[1, col] = value
        return t
    nan, inf = float("nan"), float("inf")
    bad_T = (C.c_double * 12)(*([1.0] * 11 + [nan]))
    common = [dict(N=-1), dict(V=-1), dict(H=-1), dict(W=-1), dict(blocks=-1), dict(N=1 << 31), dict(H=1 << 16, W=1 << 16), dict(V=1 << 40),
              dict(points=None), dict(views=None), dict(zbuf=None), dict(points=C.c_void_p(pts.data_ptr() + 2)), dict(zbuf=C.c_void_p(zbuf.data_ptr() + 2)),
              dict(views=view(13, 0.0)), dict(views=view(13, -1.0)), dict(views=view(14, NEAR)), dict(views=view(14, inf)), dict(views=view(13, nan)),
              dict(views=view(14, nan)), dict(views=view(3, nan)), dict(views=view(9, inf)), dict(views=view(12, -1.0)), dict(views=view(12, nan)),
              dict(radius=-1.0), dict(radius=nan), dict(radius=inf), dict(r_min=-0.5), dict(r_min=nan), dict(r_max=0.25), dict(r_max=16.5),
              dict(r_max=nan), dict(transform=bad_T)]
    for kw in common + [dict(counts=None), dict(counts=C.c_void_p(counts.data_ptr() + 4)), dict(flags=2), dict(work=C.c_void_p(counts.data_ptr() + 4))]:
        assert call("zmin", **kw) == -22, kw
    for kw in common + [dict(tau=-0.1), dict(tau=nan), dict(tau=inf), dict(scale=3.0), dict(scale=0.0), dict(scale=nan), dict(scale=2.0 ** 60),
                        dict(sum=None), dict(cnt=None), dict(sum=C.c_void_p(total.data_ptr() + 4)), dict(cnt=C.c_void_p(cnt.data_ptr() + 2))]:
        assert call("sum", **kw) == -22, kw
    # nothing to do is not an error, and nothing at all was touched so far
    assert call("zmin", N=0) == 0 and call("zmin", V=0) == 0 and call("sum", N=0) == 0 and call("sum", V=0) == 0
    assert bool((zbuf == 7.0).all()) and bool((counts == -1).all()) and bool((total == -1).all()) and bool((cnt == -1).all())
    assert call("zmin", r_max=16.0) == 0 and bool((counts >= 0).all())                   # (the cap itself is allowed)
    # the binding's own checks
    for bad in (lambda: ops.cloud_splat_zmin(pts.double(), table, (H, W), 2.0, 0.5, 4.0), lambda: ops.cloud_splat_zmin(pts[:, :2], table, (H, W), 2.0, 0.5, 4.0),
                lambda: ops.cloud_splat_zmin(pts, table[:, :14], (H, W), 2.0, 0.5, 4.0), lambda: ops.cloud_splat_zmin(pts, table, (H, W), 2.0, 0.5, 4.0, zbuf=zbuf[:1]),
                lambda: ops.cloud_splat_sum(pts, table, (H, W), 2.0, 0.5, 4.0, None, 0.01, scale), lambda: ops.cloud_splat_zmin(pts, table, (H, W), 2.0, 0.5, 17.0)):
        with pytest.raises(_lib.DmvsError):
            bad()
    with pytest.raises(ValueError):
        R.render_depth(ops, pts, K, E, (H, W), mode="median")
    empty = R.render_depth(ops, np.zeros((0, 3), np.float32), K, E, (H, W))
    assert int(empty["mask"].sum()) == 0 and int(empty["counts"].sum()) == 0 and tuple(empty["depth"].shape) == (2, H, W)


# ------------------------------------------------------------------------------------------ command line
def write_tree(root, sc):
    from PIL import Image
    for d in ("images", "cams"):
        os.makedirs(os.path.join(root, d))
    with open(os.path.join(root, "pair.txt"), "w") as f:
        f.write(f"{PV}\n")
        for v in range(PV):
            Image.fromarray((sc["images"][v].permute(1, 2, 0).numpy() * 255).astype("uint8")).save(os.path.join(root, "images", f"{v:08d}.jpg"))
            cam = np.zeros((2, 4, 4), np.float32)
            cam[0], cam[1, :3, :3] = sc["E"][v].numpy(), sc["K"][v].numpy()
            IO.write_cam(os.path.join(root, "cams", f"{v:08d}_cam.txt"), cam, 425.0, 935.0)      # an INPUT camera file: depth_min first
            f.write(f"{v}\n2 " + " ".join(f"{int(s)} 1.0" for s in sc["pairs"][v]) + "\n")


def files(root):
    return {os.path.relpath(os.path.join(b, f), root): open(os.path.join(b, f), "rb").read() for b, _, fs in os.walk(root) for f in fs}


def round_trip(ops, tmp_path, sc, cloud, capsys):
    from PIL import Image
    from diffmvs_amd import depth_eval as DE, train_driver as TD
    from diffmvs_amd.cloud_register import save_transform
    tree = str(tmp_path / "tree")
    write_tree(tree, sc)
    cloud = np.round(cloud * 64.0) / 64.0                      # so that the quarter turn below moves it, and moves it back, exactly
    zero = np.zeros((len(cloud), 3), np.uint8)
    IO.write_ply(str(tmp_path / "gt.ply"), cloud.astype(np.float32), zero)
    res = R.main(["--cloud", str(tmp_path / "gt.ply"), "--tree", tree, "--radius", "2.0", "--r_max", "4"], ops=ops)
    assert list(res["scans"]) == [""] and len(res["scans"][""]["views"]) == PV
    record = json.load(open(os.path.join(tree, "render.json")))
    assert record["views"]["00000000"]["size"] == [32, 64] and record["views"]["00000000"]["covered"] > 0.9 and record["radius"] == 2.0
    # what the tree's readers see is what render_depth returns for load_view's cameras (general: 48 x 64 becomes 32 x 64)
    ds = IO.MVSDataset(tree, dataset="general")
    views = [ds.load_view("", v) for v in range(PV)]
    direct = R.render_depth(ops, cloud.astype(np.float32), np.stack([v[1] for v in views]), np.stack([v[2] for v in views]), (32, 64), radius=2.0,
                            r_max=4.0, depth_range=[(v[3], v[4]) for v in views])
    train = TD.TreeTrainSet(tree, [""], 3, numdepth=8, dataset="general")
    assert len(train) == PV
    for i in range(PV):
        s = train.get(i, None)
        ref = s["view_ids"][0]
        d, m = direct["depth"][ref].cpu(), direct["mask"][ref].cpu()
        assert torch.equal(s["depth"]["stage4"], d) and torch.equal(s["depth"]["stage1"], d[::8, ::8])
        assert torch.equal(s["mask"]["stage4"] > 0.5, m) and torch.equal(s["mask"]["stage1"] > 0.5, m[::8, ::8])
        assert np.array_equal(np.array(Image.open(os.path.join(tree, "mask", f"{ref:08d}.png"))), np.where(m.numpy(), 255, 0).astype(np.uint8))
    # depth_eval of an estimate that IS the ground truth: zero error over exactly the masked pixels
    os.makedirs(tmp_path / "est" / "depth_est")
    for v in range(PV):
        IO.save_pfm(str(tmp_path / "est" / "depth_est" / f"{v:08d}.pfm"), IO.read_pfm(os.path.join(tree, "depth_gt", f"{v:08d}.pfm"))[0])
    capsys.readouterr()
    score = DE.main(["--outdir", str(tmp_path / "est"), "--gtpath", tree], ops=ops)
    masked = int(direct["mask"].sum())
    assert score["overall"]["abs_err"] == 0.0 and score["overall"]["rmse"] == 0.0 and score["counters"]["views"] == PV
    assert score["counters"]["masked"] == score["counters"]["scored"] == masked > 0
    # a second run refuses, and changes nothing
    before = files(tree)
    with pytest.raises(SystemExit, match="--overwrite"):
        R.main(["--cloud", str(tmp_path / "gt.ply"), "--tree", tree, "--radius", "3.0"], ops=ops)
    assert files(tree) == before
    # the cloud in another frame, brought back by --transform T --invert, into another output tree: the same files
    T = np.array([[0.0, -1.0, 0.0, 64.0], [1.0, 0.0, 0.0, -32.0], [0.0, 0.0, 1.0, 16.0], [0.0, 0.0, 0.0, 1.0]])
    moved = cloud @ T[:3, :3].T + T[:3, 3]
    assert np.array_equal(moved.astype(np.float32).astype(np.float64), moved)
    IO.write_ply(str(tmp_path / "moved.ply"), moved.astype(np.float32), zero)
    save_transform(str(tmp_path / "T.txt"), T)
    R.main(["--cloud", str(tmp_path / "moved.ply"), "--tree", tree, "--out", str(tmp_path / "again"), "--transform", str(tmp_path / "T.txt"), "--invert",
            "--radius", "2.0", "--r_max", "4"], ops=ops)
    again = files(str(tmp_path / "again"))
    assert sorted(again) == sorted(k for k in before if k.startswith(("depth_gt", "mask", "render.json")))
    assert all(again[k] == before[k] for k in again if k != "render.json")
    assert json.load(open(tmp_path / "again" / "render.json"))["views"] == record["views"]


def test_command_line_per_scan_layout_and_overwrite(tmp_path):
    """--dataset tank --testlist: <tree>/<scan>/{images, cams_1, pair.txt} in, <out>/<scan>/{depth_gt, mask, render.json} out at the data set's
    fixed 1920 x 1056; --overwrite replaces the maps and leaves none of a view that pair.txt no longer lists"""
    from PIL import Image
    ops = emu_ops()
    sc = synth.synth_scene(PH, PW, n_views=2, n_src=1, seed=3, grid_w=2)
    tree, out = tmp_path / "tree", tmp_path / "out"
    for d in ("images", "cams_1"):
        os.makedirs(tree / "scan9" / d)
    for v in range(2):
        Image.fromarray((sc["images"][v].permute(1, 2, 0).numpy() * 255).astype("uint8")).save(str(tree / "scan9" / "images" / f"{v:08d}.jpg"))
        cam = np.zeros((2, 4, 4), np.float32)
        cam[0], cam[1, :3, :3] = sc["E"][v].numpy(), sc["K"][v].numpy()
        IO.write_cam(str(tree / "scan9" / "cams_1" / f"{v:08d}_cam.txt"), cam, 425.0, 935.0)
    (tree / "scan9" / "pair.txt").write_text("2\n0\n1 1 1.0\n1\n1 0 1.0\n")
    (tmp_path / "list.txt").write_text("scan9\n")
    cloud = lattice(4.0, -450, 450, -350, 350)
    IO.write_ply(str(tmp_path / "gt.ply"), cloud, np.zeros((len(cloud), 3), np.uint8))
    base = ["--cloud", str(tmp_path / "gt.ply"), "--tree", str(tree), "--out", str(out), "--dataset", "tank", "--radius", "4.0", "--r_max", "16"]
    with pytest.raises(SystemExit, match="--testlist"):
        R.main(base, ops=ops)
    res = R.main(base + ["--testlist", str(tmp_path / "list.txt")], ops=ops)
    assert list(res["scans"]) == ["scan9"] and sorted(res["scans"]["scan9"]["views"]) == ["00000000", "00000001"]
    assert sorted(os.listdir(out / "scan9")) == ["depth_gt", "mask", "render.json"] and sorted(os.listdir(out / "scan9" / "depth_gt")) == ["00000000.pfm", "00000001.pfm"]
    depth = IO.read_pfm(str(out / "scan9" / "depth_gt" / "00000001.pfm"))[0]
    mask = np.array(Image.open(str(out / "scan9" / "mask" / "00000001.png")))
    assert depth.shape == (1056, 1920) and mask.shape == (1056, 1920) and np.array_equal(mask > 0, depth > 0) and (depth > 0).mean() > 0.99
    # what load_view hands out for the scan is what was rendered
    ds = IO.MVSDataset(str(tree), dataset="tank", scan=["scan9"])
    _, k, e, d0, d1 = ds.load_view("scan9", 1)
    direct = R.render_depth(ops, cloud, k[None], e[None], (1056, 1920), radius=4.0, r_max=16.0, depth_range=(d0, d1))
    assert np.array_equal(bits(np.ascontiguousarray(depth)), bits(direct["depth"][0]))
    # view 1 leaves pair.txt: refused without --overwrite, and with it its maps are gone
    (tree / "scan9" / "pair.txt").write_text("1\n0\n1 1 1.0\n")
    with pytest.raises(SystemExit, match="--overwrite"):
        R.main(base + ["--testlist", str(tmp_path / "list.txt")], ops=ops)
    assert len(os.listdir(out / "scan9" / "depth_gt")) == 2
    R.main(base + ["--testlist", str(tmp_path / "list.txt"), "--overwrite"], ops=ops)
    assert os.listdir(out / "scan9" / "depth_gt") == ["00000000.pfm"] and os.listdir(out / "scan9" / "mask") == ["00000000.png"]
    assert list(json.load(open(out / "scan9" / "render.json"))["views"]) == ["00000000"]


def test_command_line_round_trip(tmp_path, monkeypatch, capsys, scene, back_plane):
    ops = emu_ops()
    pin_ops(monkeypatch, ops)
    round_trip(ops, tmp_path, scene[0], back_plane, capsys)


@pytest.mark.gpu
def test_command_line_round_trip_on_the_gpu(tmp_path, capsys, scene, back_plane):
    round_trip(hip_ops(), tmp_path, scene[0], back_plane, capsys)


@pytest.mark.gpu
def test_beyond_one_view_chunk_on_the_gpu():
    """300 000 points x 7 views at 96 x 128: three passes of 3 + 3 + 1 views against one pass of 7, bit for bit, in both modes"""
    ops = hip_ops()
    H, W = 96, 128
    sc = synth.synth_scene(H, W, n_views=7, n_src=2, seed=3, grid_w=3)
    rs = np.random.RandomState(5)
    d0, a, c = synth.scene_plane(3)
    x, y = rs.uniform(-450.0, 450.0, 300000), rs.uniform(-350.0, 350.0, 300000)
    pts = np.stack([x, y, d0 + a * x + c * y + rs.normal(0.0, 2.0, x.size)], 1).astype(np.float32)
    for mode in ("mean", "nearest"):
        a3 = R.render_depth(ops, pts, sc["K"], sc["E"], (H, W), radius=2.0, mode=mode, view_chunk=3)
        a7 = R.render_depth(ops, pts, sc["K"], sc["E"], (H, W), radius=2.0, mode=mode, view_chunk=7)
        assert torch.equal(a3["depth"].view(torch.int32), a7["depth"].view(torch.int32)) and torch.equal(a3["counts"], a7["counts"])
        assert mode == "nearest" or torch.equal(a3["count"], a7["count"])
        assert float(a7["mask"].float().mean()) > 0.99
