"""dmvs_depth_stats_f32 / diffmvs_amd.depth_eval: the integer rows of depth-map scoring against an fp64 numpy restatement (tolerance ZERO:
the kernel's subtract, divide and multiply are IEEE fp64 operations, correctly rounded on both sides, and llrint = np.rint round half to
even), their independence of the grid and of the load width, the metrics against the independent fp32 helpers of diffmvs_amd.formats, the
argument checks, and the command line on a small tree.  Every `ops` test runs on the host emulation here and on the MI355X under -m gpu."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import emu_ops, pin_ops
from diffmvs_amd import _lib, depth_eval as DE, formats as IO
from diffmvs_amd.cloud_grid import pow2_scale_below

THR = (2.0, 4.0, 8.0)
BIG = 935.0


def restate(est, gt, mask, thresholds, big, scale, band=(0.0, np.inf)):
    """include/dmvs.h, dmvs_depth_stats_f32, in numpy fp64: same casts, same operations, np.rint"""
    B = est.shape[0]
    mant, ex = math.frexp(big)
    scale_sq = scale / 2.0 ** (ex - 1 if mant == 0.5 else ex)
    rows = np.zeros((B, 7 + len(thresholds)), np.int64)
    for b in range(B):
        e32, g32 = est[b].reshape(-1), gt[b].reshape(-1)
        m = np.ones(e32.shape, bool) if mask is None else mask[b].reshape(-1) > np.float32(0.5)
        ok = np.isfinite(e32) & np.isfinite(g32) & (g32 > 0)
        with np.errstate(all="ignore"):
            e = e32.astype(np.float64) - g32.astype(np.float64)
            a = np.abs(e)
            s = m & ok & (a >= band[0]) & (a <= band[1])
            a, g, e = a[s], g32[s].astype(np.float64), e[s]
            rel, sq = a / g, e * e
        rows[b, 0], rows[b, 1], rows[b, 2] = m.sum(), s.sum(), (m & ~ok).sum()
        rows[b, 3] = (a > big).sum() + (rel > big).sum() + (sq > big * big).sum()
        rows[b, 4] = np.rint(np.minimum(a, big) * scale).astype(np.int64).sum()
        rows[b, 5] = np.rint(np.minimum(rel, big) * scale).astype(np.int64).sum()
        rows[b, 6] = np.rint(np.minimum(sq, big * big) * scale_sq).astype(np.int64).sum()
        for t, thr in enumerate(thresholds):
            rows[b, 7 + t] = (a < np.float64(np.float32(thr))).sum()
    return rows


def make_maps(B, H, W, seed, sigma=3.0):
    rs = np.random.RandomState(seed)
    gt = rs.uniform(425.0, 935.0, (B, H, W)).astype(np.float32)
    est = (gt + rs.normal(0.0, sigma, (B, H, W))).astype(np.float32)
    mask = (rs.rand(B, H, W) > 0.3).astype(np.float32)
    return est, gt, mask


def run(ops, est, gt, mask, scale, blocks=0, thresholds=THR, big=BIG, band=None):
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(ops.device)  # noqa: E731
    return ops.depth_stats(t(est), t(gt), t(mask), thresholds, big, scale, band=band, blocks=blocks).cpu().numpy()


def test_exact_integers_on_an_odd_shape_with_planted_exclusions(ops):
    """B = 3, 37 x 53 (odd: scalar head and tail, rows that start off a 16-byte line), holes in the mask, item 2 with an empty mask, and
    planted: a NaN and a +inf estimate and one gt = 0 at masked pixels (3 left out), one error beyond `big` (2 clamped terms: |e| and e^2).
    Every slot equals the fp64 restatement, tolerance zero, the relative-error slot included: hipcc's fp64 division is the correctly
    rounded one (no fast-math flag in the build), like the host's."""
    B, H, W = 3, 37, 53
    est, gt, mask = make_maps(B, H, W, 1)
    mask[2] = 0.0
    mask[0, 5, 7] = mask[0, 6, 8] = mask[1, 3, 3] = mask[1, 30, 50] = 1.0
    est[0, 5, 7], est[0, 6, 8], gt[1, 3, 3] = np.nan, np.inf, 0.0
    est[1, 30, 50] = gt[1, 30, 50] + np.float32(2000.0)
    scale = pow2_scale_below(BIG, H * W)
    got, want = run(ops, est, gt, mask, scale), restate(est, gt, mask, THR, BIG, scale)
    assert got.dtype == np.int64 and got.shape == (B, 10)
    assert np.array_equal(got, want), (got - want)
    assert got[:, 2].tolist() == [2, 1, 0] and got[:, 3].tolist() == [0, 2, 0]            # what was planted: left out, clamped terms
    assert got[2].tolist() == [0] * 10 and got[0, 1] == got[0, 0] - 2 and got[0, 1] > 0
    # ... and through the module: the same integers behind the two scale exponents, the counters carried into the summary
    t = lambda a: torch.from_numpy(a).to(ops.device)  # noqa: E731
    rows = DE.score(ops, t(est), t(gt), t(mask), THR, big=BIG)
    assert rows.device.type == ops.device.type and rows.dtype == torch.int64
    k, k_sq = DE.scale_exponents(BIG, H * W)
    assert 2.0 ** k == scale and k_sq == k - 10 and np.array_equal(rows.cpu().numpy(), np.concatenate([np.full((B, 1), k), np.full((B, 1), k_sq), want], 1))
    s = DE.summarise(rows, THR)
    assert (s["items"], s["empty_items"], s["left_out"], s["saturated"]) == (3, 1, 3, 2)
    per_item = [want[b, 4] / scale / want[b, 1] for b in range(2)]
    assert abs(s["abs_err"] - np.mean(per_item)) < 1e-12 and abs(s["pooled"]["abs_err"] - want[:2, 4].sum() / scale / want[:2, 1].sum()) < 1e-12
    assert abs(s["inlier_2"] - np.mean([want[b, 7] / want[b, 1] for b in range(2)])) < 1e-15
    assert abs(s["rmse"] - np.mean([math.sqrt(want[b, 6] / 2.0 ** k_sq / want[b, 1]) for b in range(2)])) < 1e-12
    # a band: only errors inside it are scored
    band = (1.0, 5.0)
    assert np.array_equal(run(ops, est, gt, mask, scale, band=band), restate(est, gt, mask, THR, BIG, scale, band))
    # no mask: every pixel
    assert np.array_equal(run(ops, est, gt, None, scale), restate(est, gt, None, THR, BIG, scale))


@pytest.fixture(scope="module")
def big_case():
    B, H, W = 2, 300, 301
    est, gt, mask = make_maps(B, H, W, 2)
    scale = pow2_scale_below(BIG, H * W)
    return est, gt, mask, scale, restate(est, gt, mask, THR, BIG, scale)


def test_past_one_workgroup_the_rows_do_not_depend_on_the_grid(ops, big_case):
    """B = 2, 300 x 301 = 90300 pixels per item (353 workgroups' worth one by one, 89 in quads): one workgroup per item, seven, and the
    library's choice give bit-identical rows, equal to numpy"""
    est, gt, mask, scale, want = big_case
    for blocks in (1, 7, 0):
        assert np.array_equal(run(ops, est, gt, mask, scale, blocks=blocks), want), blocks


def test_the_16_byte_path_and_the_scalar_path_give_the_same_rows(ops):
    """64 x 64 in whole allocations (aligned: float4 loads only) against the same values with est moved by ONE element inside its
    allocation while gt and mask stay put (the three no longer share a 16-byte phase: scalar loads), and with all three moved by one
    element (quads behind a scalar head)"""
    B, H, W = 2, 64, 64
    est, gt, mask = make_maps(B, H, W, 3)
    scale = pow2_scale_below(BIG, H * W)
    want = restate(est, gt, mask, THR, BIG, scale)
    dev = ops.device
    te, tg, tm = (torch.from_numpy(a).to(dev) for a in (est, gt, mask))
    assert te.data_ptr() % 16 == 0 and tg.data_ptr() % 16 == 0 and tm.data_ptr() % 16 == 0
    aligned = ops.depth_stats(te, tg, tm, THR, BIG, scale).cpu().numpy()

    def shifted(t):
        buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev)
        buf[1:1 + t.numel()] = t.reshape(-1)
        v = buf[1:1 + t.numel()].view(t.shape)
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        return v
    scalar = ops.depth_stats(shifted(te), tg, tm, THR, BIG, scale).cpu().numpy()
    headed = ops.depth_stats(shifted(te), shifted(tg), shifted(tm), THR, BIG, scale).cpu().numpy()
    assert np.array_equal(aligned, want) and np.array_equal(scalar, want) and np.array_equal(headed, want)


def test_metrics_against_the_independent_fp32_helpers(ops):
    """summarise(score(...)) against formats.abs_depth_error / abs_rel_error on the same tensors (no empty item, nothing non-finite).
    Bound, with u = 2^-24, n = H W pixels per item, B items, scale 2^k and emax the largest |est - gt|:
      this module: a term is rounded by at most 2^-(k+1), and so is every mean of terms (the fp64 ratios add ~2^-53 relative: nothing);
      the helper: its fp32 difference is off by at most u |e| (one rounding), its fp32 mean over up to n terms by at most n u times the
      mean of the magnitudes (the classical bound for ANY summation order, so it covers torch's blocked one), the division by the count and
      the mean over the B items by (B + 2) u more: (n + B + 3) u emax in all.  For the relative error the fp32 quotient adds one more
      rounding, and a term is at most emax / 425 (gt >= 425): (n + B + 4) u emax / 425."""
    B, H, W = 3, 37, 53
    est, gt, mask = make_maps(B, H, W, 4)
    te, tg, tm = (torch.from_numpy(a) for a in (est, gt, mask))
    k, _ = DE.scale_exponents(BIG, H * W)
    s = DE.summarise(DE.score(ops, te.to(ops.device), tg.to(ops.device), tm.to(ops.device), THR, big=BIG), THR)
    assert s["empty_items"] == 0 and s["left_out"] == 0 and s["saturated"] == 0
    yard_abs, yard_rel = float(IO.abs_depth_error(te, tg, tm > 0.5)), float(IO.abs_rel_error(te, tg, tm > 0.5))
    u, n = 2.0 ** -24, H * W
    emax = float((te.double() - tg.double()).abs().max())
    bound_abs = 2.0 ** -(k + 1) + (n + B + 3) * u * emax
    bound_rel = 2.0 ** -(k + 1) + (n + B + 4) * u * emax / 425.0
    print(f"abs_err {s['abs_err']!r} vs {yard_abs!r} (bound {bound_abs:.3e});  abs_rel {s['abs_rel']!r} vs {yard_rel!r} (bound {bound_rel:.3e})")
    assert abs(s["abs_err"] - yard_abs) <= bound_abs
    assert abs(s["abs_rel"] - yard_rel) <= bound_rel
    assert bound_abs < 0.05 * yard_abs and bound_rel < 0.05 * yard_rel                    # the bound still tells a wrong metric from a right one


def test_argument_checks_raise_before_any_launch(ops):
    dev = ops.device
    x = torch.ones(2, 8, 12, device=dev)
    scale = pow2_scale_below(BIG, 96)
    with pytest.raises(_lib.DmvsError):
        ops.depth_stats(x, x, None, list(range(1, 10)), BIG, scale)                       # 9 thresholds
    with pytest.raises(_lib.DmvsError):
        ops.depth_stats(x, torch.ones(2, 12, 8, device=dev), None, THR, BIG, scale)       # mismatched shapes
    with pytest.raises(_lib.DmvsError):
        ops.depth_stats(x, x, torch.ones(1, 8, 12, device=dev), THR, BIG, scale)
    with pytest.raises(_lib.DmvsError):
        ops.depth_stats(x.transpose(1, 2), x.transpose(1, 2), None, THR, BIG, scale)      # not contiguous
    with pytest.raises(_lib.DmvsError):
        ops.depth_stats(x.double(), x, None, THR, BIG, scale)                             # wrong dtype
    with pytest.raises(_lib.DmvsError):
        ops.depth_stats(x, x, x.to(torch.uint8), THR, BIG, scale)                         # the mask is fp32
    for kw in ({"big": 0.0}, {"big": float("inf")}, {"scale": 3.0}, {"scale": 2.0 ** 62}, {"band": (5.0, 1.0)}, {"band": (-1.0, 1.0)},
               {"band": (float("nan"), 1.0)}, {"blocks": -1}, {"thresholds": (float("nan"),)}):
        a = {"thresholds": THR, "big": BIG, "scale": scale, "band": None, "blocks": 0, **kw}
        with pytest.raises(_lib.DmvsError, match="-22"):                                  # DMVS_EINVAL from the library itself
            ops.depth_stats(x, x, None, a["thresholds"], a["big"], a["scale"], band=a["band"], blocks=a["blocks"])
    # the C entry point: NULL operands and misaligned pointers (never dereferenced)
    import ctypes as C
    f, p = ops.lib.dll.dmvs_depth_stats_f32, C.c_void_p(4096)
    thr = (C.c_float * 3)(*THR)
    inf = float("inf")
    assert f(None, p, None, 1, 96, thr, 3, 0.0, inf, BIG, scale, 0, p, None) == -22
    assert f(p, p, None, 1, 96, thr, 3, 0.0, inf, BIG, scale, 0, None, None) == -22
    assert f(C.c_void_p(4098), p, None, 1, 96, thr, 3, 0.0, inf, BIG, scale, 0, p, None) == -22
    assert f(p, p, None, -1, 96, thr, 3, 0.0, inf, BIG, scale, 0, p, None) == -22
    assert f(p, p, None, 65536, 96, thr, 3, 0.0, inf, BIG, scale, 0, p, None) == -22
    assert f(p, p, None, 1, 96, None, 3, 0.0, inf, BIG, scale, 0, p, None) == -22
    # nothing to score: zero rows, no launch
    assert tuple(ops.depth_stats(torch.ones(0, 8, 12, device=dev), torch.ones(0, 8, 12, device=dev), None, THR, BIG, scale).shape) == (0, 10)
    z = ops.depth_stats(torch.ones(2, 0, 12, device=dev), torch.ones(2, 0, 12, device=dev), None, THR, BIG, scale)
    assert tuple(z.shape) == (2, 10) and int(z.abs().sum()) == 0
    assert tuple(DE.score(ops, torch.ones(0, 8, 12), torch.ones(0, 8, 12), None, THR, big=BIG).shape) == (0, 12)
    assert DE.summarise(z.new_zeros(0, 12), THR)["abs_err"] is None


def test_summarise_is_a_function_of_the_integers_in_order():
    """no device: rows with different scales pool exactly; an empty item is counted, not averaged"""
    rows = [[4, 2, 10, 8, 0, 0, 24, 16, 64, 4, 6, 8],       # k = 4, k_sq = 2: 8 scored, sum |e| = 1.5, sum rel = 1, sum e^2 = 16
            [3, 1, 5, 0, 0, 0, 0, 0, 0, 0, 0, 0],           # nothing scored
            [3, 1, 4, 4, 1, 2, 8, 4, 8, 1, 2, 4]]           # k = 3, k_sq = 1: 4 scored, sum |e| = 1, sum rel = 0.5, sum e^2 = 4
    s = DE.summarise(rows, THR)
    assert s["abs_err"] == (1.5 / 8 + 1.0 / 4) / 2 and s["abs_rel"] == (1.0 / 8 + 0.5 / 4) / 2 and s["rmse"] == (math.sqrt(2.0) + 1.0) / 2
    assert s["inlier_2"] == (0.5 + 0.25) / 2 and s["inlier_8"] == 1.0
    assert s["pooled"] == {"abs_err": 2.5 / 12, "abs_rel": 1.5 / 12, "rmse": math.sqrt(20.0 / 12), "inlier_2": 5 / 12, "inlier_4": 8 / 12, "inlier_8": 1.0}
    assert (s["items"], s["empty_items"], s["masked"], s["scored"], s["left_out"], s["saturated"]) == (3, 1, 19, 12, 1, 2)
    assert DE.summarise(torch.tensor(rows), THR) == s


# ------------------------------------------------------------------------------------------ command line (host emulation)
def _tree(root, offset=3.0):
    """two views 32 x 64 under <root>/gt/{depth_gt, mask} and <root>/out/depth_est: estimate = ground truth + `offset` inside the mask (the
    left half), + 100 outside it; in view 1 the first three masked rows are off by 6 instead"""
    from PIL import Image
    H, W = 32, 64
    rs = np.random.RandomState(5)
    for d in ("gt/depth_gt", "gt/mask", "out/depth_est"):
        os.makedirs(os.path.join(root, d))
    m = np.zeros((H, W), np.uint8)
    m[:, :W // 2] = 255
    for v in range(2):
        gt = np.round(rs.uniform(500.0, 800.0, (H, W))).astype(np.float32)          # whole numbers: gt + 3 and gt + 6 are exact in fp32
        est = np.where(m > 0, gt + np.float32(offset), gt + np.float32(100.0)).astype(np.float32)
        if v == 1:
            est[:3, :W // 2] = gt[:3, :W // 2] + np.float32(6.0)
        IO.save_pfm(os.path.join(root, "gt/depth_gt", f"{v:08d}.pfm"), gt)
        IO.save_pfm(os.path.join(root, "out/depth_est", f"{v:08d}.pfm"), est)
        Image.fromarray(m).save(os.path.join(root, "gt/mask", f"{v:08d}.png"))
    IO.save_pfm(os.path.join(root, "out/depth_est", f"{2:08d}.pfm"), est)            # an estimate without ground truth: counted, not scored
    return H, W


def test_command_line_reports_the_planted_offset_and_inlier_shares(tmp_path, capsys):
    H, W = _tree(str(tmp_path))
    res = DE.main(["--outdir", str(tmp_path / "out"), "--gtpath", str(tmp_path / "gt"), "--thresholds", "2", "4", "8"], ops=emu_ops())
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed == res and set(res) == {"thresholds", "scenes", "overall", "counters"}
    n = H * W // 2
    o = res["overall"]
    # view 0: every masked pixel off by exactly 3; view 1: three rows (3 * 32 pixels) off by 6, the rest by 3
    share6 = 3 * (W // 2) / n
    assert o["abs_err"] == (3.0 + (3.0 + 3.0 * share6)) / 2 and o["pooled"]["abs_err"] == 3.0 + 3.0 * share6 / 2
    assert o["inlier_2"] == 0.0 and o["inlier_4"] == (1.0 + (1.0 - share6)) / 2 and o["inlier_8"] == 1.0
    assert res["scenes"][""] == o and res["counters"] == {"views": 2, "views_without_ground_truth": 1, "empty_items": 0, "masked": 2 * n,
                                                           "scored": 2 * n, "left_out": 0, "saturated": 0}


def test_command_line_subsamples_full_size_ground_truth(tmp_path):
    """ground truth at the image's size, estimate at half of it: the ground truth (and its mask) are taken at every second pixel"""
    H, W = _tree(str(tmp_path))
    for v in range(2):
        f = str(tmp_path / "out" / "depth_est" / f"{v:08d}.pfm")
        IO.save_pfm(f, np.ascontiguousarray(IO.read_pfm(f)[0][::2, ::2]))
    os.remove(str(tmp_path / "out" / "depth_est" / f"{2:08d}.pfm"))
    res = DE.main(["--outdir", str(tmp_path / "out"), "--gtpath", str(tmp_path / "gt")], ops=emu_ops())
    assert res["counters"]["scored"] == 2 * (H // 2) * (W // 4) and res["overall"]["inlier_8"] == 1.0
    assert res["overall"]["pooled"]["abs_err"] == 3.0 + 3.0 * (2 * (W // 4)) / (2 * (H // 2) * (W // 4))      # rows 0 and 2 of view 1 are off by 6


def _write_inputs(root, H, W, V, seed):
    """a `general` scene tree (images, cams, pair.txt) with depth_gt PFMs, written with this package's writers"""
    from PIL import Image
    from diffmvs_amd import synth
    sc = synth.synth_scene(H, W, n_views=V, n_src=V - 1, seed=seed, numdepth=8)
    depths = np.asarray(synth.synth_view_depths(H, W, V, seed=seed), np.float32)
    for d in ("images", "cams", "depth_gt"):
        os.makedirs(os.path.join(root, d))
    with open(os.path.join(root, "pair.txt"), "w") as f:
        f.write(f"{V}\n")
        for v in range(V):
            Image.fromarray((sc["images"][v].permute(1, 2, 0).numpy() * 255).astype("uint8")).save(os.path.join(root, "images", f"{v:08d}.jpg"))
            cam = np.zeros((2, 4, 4), np.float32)
            cam[0], cam[1, :3, :3] = sc["E"][v].numpy(), sc["K"][v].numpy()
            IO.write_cam(os.path.join(root, "cams", f"{v:08d}_cam.txt"), cam, 425.0, 935.0)       # an INPUT camera file: depth_min first
            IO.save_pfm(os.path.join(root, "depth_gt", f"{v:08d}.pfm"), depths[v])
            f.write(f"{v}\n{V - 1} " + " ".join(f"{int(s)} 1.0" for s in sc["pairs"][v]) + "\n")


def test_eval_gt_depth_adds_the_block_and_nothing_else(tmp_path, monkeypatch, capsys):
    """`eval --gt_depth <tree>` adds depth_metrics = what the command line reports for the same output tree, and writes no file; without the
    flag the result has exactly the keys it had before the flag existed"""
    from diffmvs_amd import eval as EV
    pin_ops(monkeypatch, emu_ops())
    root, H, W, V = tmp_path / "scene", 32, 64, 3
    _write_inputs(str(root), H, W, V, seed=2)
    base = ["--testpath", str(root), "--dataset", "general", "--method", "diffmvs", "--num_view", "2", "--numdepth_initial", "8", "--batch_size", "1",
            "--graphs", "0", "--noise_seed", "5"]
    plain = EV.main(base + ["--outdir", str(tmp_path / "a")], device=torch.device("cpu"))
    assert sorted(plain) == sorted(["rank", "scenes", "views", "avg_time_s", "first_call_s", "amortised_time_s", "errors", "feature_store_s", "hip_graphs"])
    scored = EV.main(base + ["--outdir", str(tmp_path / "b"), "--gt_depth", str(root)], device=torch.device("cpu"))
    assert sorted(scored) == sorted(list(plain) + ["depth_metrics"]) and scored["errors"] == plain["errors"]
    listing = lambda d: sorted(os.path.relpath(os.path.join(b, f), d) for b, _, fs in os.walk(d) for f in fs)  # noqa: E731
    assert listing(str(tmp_path / "a")) == listing(str(tmp_path / "b"))
    capsys.readouterr()
    cli = DE.main(["--outdir", str(tmp_path / "b"), "--gtpath", str(root)], ops=emu_ops())
    assert scored["depth_metrics"] == cli and cli["counters"]["views"] == V and cli["overall"]["abs_err"] > 0
    # the fp32 helpers eval already reports (same mask: the depth range of the camera file) agree to their own precision
    assert abs(cli["overall"]["abs_rel"] - plain["errors"][""]["abs_rel"]) < 1e-5 * plain["errors"][""]["abs_rel"] + 1e-7


def test_command_line_scene_layouts(tmp_path):
    """--dataset general is the single scene directly under the two roots; the other datasets keep one directory per scene of --testlist"""
    _tree(str(tmp_path / "scan7"))
    os.makedirs(tmp_path / "o"), os.makedirs(tmp_path / "g")
    os.rename(tmp_path / "scan7" / "out", tmp_path / "o" / "scan7"), os.rename(tmp_path / "scan7" / "gt", tmp_path / "g" / "scan7")
    (tmp_path / "list.txt").write_text("scan7\n\n")
    with pytest.raises(SystemExit, match="--testlist"):
        DE.main(["--outdir", str(tmp_path / "o"), "--gtpath", str(tmp_path / "g"), "--dataset", "dtu"], ops=emu_ops())
    res = DE.main(["--outdir", str(tmp_path / "o"), "--gtpath", str(tmp_path / "g"), "--dataset", "dtu", "--testlist", str(tmp_path / "list.txt")], ops=emu_ops())
    assert list(res["scenes"]) == ["scan7"] and res["counters"]["views"] == 2 and res["overall"]["inlier_8"] == 1.0
    flat = DE.main(["--outdir", str(tmp_path / "o" / "scan7"), "--gtpath", str(tmp_path / "g" / "scan7"), "--testlist", str(tmp_path / "list.txt")], ops=emu_ops())
    assert list(flat["scenes"]) == [""] and flat["overall"] == res["overall"]
