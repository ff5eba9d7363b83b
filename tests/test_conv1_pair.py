"""FeatureNet conv1.1 + conv1.2 in one kernel (csrc/conv1_pair.hip, Ops.conv1_pair): two 16 -> 16 3x3 layers with folded BN + ReLU, both in
split-bf16 arithmetic, against the two split launches it replaces (the same bits) and against torch in fp64.  Runs on the host emulation
and, with -m gpu, on the MI355X.

Shapes (the kernel's unit is a strip of S = 80 output columns x a segment of R = 64 output rows, its march 2 rows per step):
  (2, 24, 80)    exactly one strip, less than one segment
  (1, 40, 120)   1.5 strips: the partial strip's groups beyond the image are skipped, the intermediate is zero outside the image
  (3, 96, 200)   2.5 strips x 1.5 segments x an odd batch: the second segment's warm-up must reproduce what the segment above computed;
                 18 units on the emulation's 2 resident workgroups, the 4-row rings wrap 9 times per full segment
  (2, 37, 52)    W % 80 != 0 and W % 16 != 0, an odd height (the last step computes one row of its pair)"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from diffmvs_amd import ops as K
from diffmvs_amd import engine as E
from diffmvs_amd import synth

S, R = K.Ops.CONV1_PAIR_STRIP, K.Ops.CONV1_PAIR_SEGMENT
SHAPES = [(2, 24, S), (1, 40, 3 * S // 2), (3, 3 * R // 2, 5 * S // 2), (2, 37, 52)]


def rnd(*shape, seed=0, lo=-1.0, hi=1.0):
    rs = np.random.RandomState(seed + sum(shape))
    return torch.from_numpy(rs.uniform(lo, hi, shape).astype(np.float32))


def dev(ops, *ts):
    r = [None if t is None else t.to(ops.device).contiguous() for t in ts]
    return r if len(r) > 1 else r[0]


def _bn(c, seed):
    # a shift of the order of the activations: conv(zero padding) would NOT be zero after BN + ReLU
    return {"weight": rnd(c, seed=seed, lo=0.5, hi=1.5), "bias": rnd(c, seed=seed + 1, lo=0.2, hi=0.6),
            "running_mean": rnd(c, seed=seed + 2) * 0.2, "running_var": rnd(c, seed=seed + 3, lo=0.5, hi=1.5)}


_CASES = {}


def case(N, H, W):
    """inputs, weights and the fp64 reference of one shape, computed once and shared"""
    key = (N, H, W)
    if key not in _CASES:
        x = rnd(N, 16, H, W, seed=1, lo=0.0, hi=1.0)          # (a ReLU output, like conv1.0's)
        ws = [rnd(16, 16, 3, 3, seed=2) * 0.2, rnd(16, 16, 3, 3, seed=3) * 0.2]
        bns = [_bn(16, 10), _bn(16, 20)]
        r = x.double()
        for w, b in zip(ws, bns):
            r = F.relu(F.batch_norm(F.conv2d(r, w.double(), None, 1, 1), b["running_mean"].double(), b["running_var"].double(), b["weight"].double(),
                                    b["bias"].double(), False, 0.0, 1e-5))
        _CASES[key] = (x, ws, bns, r)
    return _CASES[key]


def packed(ops, ws, bns):
    d = lambda b: {k_: v.to(ops.device) for k_, v in b.items()}
    return [K.pack_conv2d(dev(ops, w), bn=d(b), stride=1, pad=1) for w, b in zip(ws, bns)]


def two_launches(o, pcs, x):
    return o.conv2d(pcs[1], o.conv2d(pcs[0], x, act=K.ACT_RELU), act=K.ACT_RELU)


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_pair_equals_the_two_split_launches_and_meets_the_split_bound(ops, N, H, W):
    """torch.equal with conv2d(pc2, conv2d(pc1, x)) under ARITH_SPLIT, the outermost two rows and columns by name; not the bits of the exact-fp32
    pair (the mode is really on); e = max |out - ref| / max |ref| against torch in fp64 inside the project's split bound (test_stem3.py) with
    e_f32 = the two exact-fp32 launches on the same inputs"""
    x, ws, bns, ref = case(N, H, W)
    pcs = packed(ops, ws, bns)
    so = ops.with_conv_arith(K.ARITH_SPLIT)
    xd = dev(ops, x)
    out = so.conv1_pair(*pcs, xd).cpu()
    assert out.shape == (N, 16, H, W) and torch.isfinite(out).all()
    two = two_launches(so, pcs, xd).cpu()
    f32 = two_launches(ops, pcs, xd).cpu()
    regions = {"top": (slice(0, 2), slice(None)), "bottom": (slice(-2, None), slice(None)), "left": (slice(None), slice(0, 2)),
               "right": (slice(None), slice(-2, None))}
    for name, (ry, rx) in regions.items():
        assert torch.equal(out[:, :, ry, rx], two[:, :, ry, rx]), name
    assert torch.equal(out, two), float((out - two).abs().max())
    assert not torch.equal(out, f32)
    scale = float(ref.abs().max())
    e_split, e_f32 = float((out.double() - ref).abs().max()) / scale, float((f32.double() - ref).abs().max()) / scale
    print("conv1 pair split vs fp64: %.2e   two exact-fp32 launches vs fp64: %.2e" % (e_split, e_f32))
    assert e_f32 < 1e-6 and e_split < 2e-6 and e_split < 4.0 * e_f32 + 2e-7, (e_split, e_f32)


def test_padding_would_not_be_zero_after_bn_relu():
    """the premise of the border assertions: with these BN shifts conv1.1 applied to padding is far from zero, so a kernel that pads conv1.2 with
    relu(bn1(conv(padding))) instead of zeros fails them"""
    b = _bn(16, 10)
    pad_value = F.relu(F.batch_norm(torch.zeros(1, 16, 1, 1), b["running_mean"], b["running_var"], b["weight"], b["bias"], False, 0.0, 1e-5))
    assert float(pad_value.min()) > 0.1


@pytest.mark.parametrize("N,H,W", [(3, 3 * R // 2, 5 * S // 2), (2, 37, 52)])
def test_pair_depends_only_on_the_position_in_the_image(ops, N, H, W):
    """an image gives the same bits alone and as an item of the batch; the grid forced to 1 and to 2 workgroups gives the same bits; so do two
    launches in a row"""
    x, ws, bns, _ = case(N, H, W)
    pcs = packed(ops, ws, bns)
    so = ops.with_conv_arith(K.ARITH_SPLIT)
    xd = dev(ops, x)
    whole = so.conv1_pair(*pcs, xd).cpu()
    assert torch.equal(so.conv1_pair(*pcs, xd).cpu(), whole)
    last = so.conv1_pair(*pcs, xd[N - 1:N].contiguous()).cpu()
    assert torch.equal(last, whole[N - 1:N])
    for grid in (1, 2):
        assert torch.equal(so.conv1_pair(*pcs, xd, tune=grid).cpu(), whole), grid


def test_pair_rejects_what_it_does_not_handle(ops):
    x, ws, bns, _ = case(2, 24, S)
    pcs = packed(ops, ws, bns)
    w1, w2 = K.split_weights(pcs[0]), K.split_weights(pcs[1])
    good = dev(ops, x)
    out = torch.empty_like(good)

    def entry(xp, w1p, w2p, yp, n, h, w):
        ops.lib.call("dmvs_featurenet_conv1_pair_f32", xp, w1p, None, None, w2p, None, None, yp, n, h, w, 0, ops.stream())

    entry(K._ptr(good), K._ptr(w1), K._ptr(w2), K._ptr(out), 2, 24, S)          # (the call form itself is accepted)
    bad_w = dev(ops, rnd(1, 16, 24, 62, seed=1))                                 # W % 4 != 0
    assert not ops.conv1_pair_supported(bad_w)
    with pytest.raises(K._lib.DmvsError):
        ops.conv1_pair(*pcs, bad_w)
    with pytest.raises(K._lib.DmvsError):
        entry(K._ptr(bad_w), K._ptr(w1), K._ptr(w2), K._ptr(out), 1, 24, 62)
    flat = dev(ops, rnd(16 * 24 * S + 4, seed=2))
    view = flat[1:1 + 16 * 24 * S].view(1, 16, 24, S)                            # 4 bytes off a 16-byte boundary
    assert not ops.conv1_pair_supported(view)
    with pytest.raises(K._lib.DmvsError):
        ops.conv1_pair(*pcs, view)
    with pytest.raises(K._lib.DmvsError):
        entry(K._ptr(view), K._ptr(w1), K._ptr(w2), K._ptr(out), 1, 24, S)
    with pytest.raises(K._lib.DmvsError):                                        # wrong channel count
        ops.conv1_pair(*pcs, dev(ops, rnd(1, 8, 24, S, seed=1)))
    pc8 = K.pack_conv2d(dev(ops, rnd(16, 8, 3, 3, seed=5)), stride=1, pad=1)
    with pytest.raises(K._lib.DmvsError):
        ops.conv1_pair(pc8, pcs[1], good)
    for args in ((None, K._ptr(w1), K._ptr(w2), K._ptr(out)), (K._ptr(good), None, K._ptr(w2), K._ptr(out)),
                 (K._ptr(good), K._ptr(w1), None, K._ptr(out)), (K._ptr(good), K._ptr(w1), K._ptr(w2), None)):
        with pytest.raises(K._lib.DmvsError):
            entry(*args, 2, 24, S)
    with pytest.raises(K._lib.DmvsError):                                        # 16 * H * W >= 2^31
        entry(K._ptr(good), K._ptr(w1), K._ptr(w2), K._ptr(out), 1, 16384, 8192)


def _feature_weights(ops, seed=5):
    from models import CasDiffMVS
    model = CasDiffMVS(synth.make_args("diffmvs", numdepth_initial=8), test=True).eval()
    sd = synth.synth_state_dict(model.state_dict(), seed)
    return E.pack_feature({k: v.to(ops.device) for k, v in sd.items()})


def test_run_feature_switch_and_fallback(ops, monkeypatch):
    """run_feature takes the pair kernel under conv_arith = "split" where it applies, and the two launches otherwise: DMVS_CONV1_PAIR=0, the
    fp32 arithmetic and a width the kernel does not take (c1 rows that are no 16-byte multiples) -- and the features are the same bits"""
    f = _feature_weights(ops)
    so = ops.with_conv_arith(K.ARITH_SPLIT)
    calls = []
    real = K.Ops.conv1_pair
    monkeypatch.setattr(K.Ops, "conv1_pair", lambda self, *a, **kw: (calls.append(1), real(self, *a, **kw))[1])

    def feats(o, x):
        return {k: v.cpu() for k, v in E.run_feature(o, f, x).items()}

    x = dev(ops, rnd(1, 3, 48, 2 * S, seed=1))         # c1 is 24 x S: one strip
    monkeypatch.setenv("DMVS_CONV1_PAIR", "1")
    on = feats(so, x)
    assert len(calls) == 1
    monkeypatch.setenv("DMVS_CONV1_PAIR", "0")
    off = feats(so, x)
    assert len(calls) == 1
    assert on.keys() == off.keys() and all(torch.equal(on[k], off[k]) for k in on)
    monkeypatch.setenv("DMVS_CONV1_PAIR", "1")
    feats(ops, x)                                       # fp32 arithmetic: untouched
    assert len(calls) == 1
    xb = dev(ops, rnd(1, 3, 48, 2 * S + 4, seed=1))     # c1 rows of S + 2 floats: unsupported, the two launches
    feats(so, xb)
    assert len(calls) == 1


def test_model_forward_with_and_without_the_pair(ops, monkeypatch):
    """the whole forward (64 x 160, B = 1, 3 views, conv_arith = "split") with DMVS_CONV1_PAIR = 1 and = 0: the same depth maps bit for bit"""
    from models import CasDiffMVS
    args = synth.make_args("diffmvs", numdepth_initial=8, conv_arith="split")
    model = CasDiffMVS(args, test=True).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 7), strict=True)
    if ops.device.type != "cpu":
        model = model.to(ops.device)
    imgs, proj, dv = synth.synth_inputs(64, 2 * S, 2, B=1, seed=3)
    eng = model.engine(ops)
    assert eng.conv_arith == "split"
    calls = []
    real = K.Ops.conv1_pair
    monkeypatch.setattr(K.Ops, "conv1_pair", lambda self, *a, **kw: (calls.append(1), real(self, *a, **kw))[1])
    outs = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("DMVS_CONV1_PAIR", knob)
        with torch.no_grad():
            outs[knob] = eng.forward(imgs, proj, dv, noise_fn=synth.NoiseSource(11))["depth"][-1].cpu()
    assert len(calls) >= 1
    assert torch.isfinite(outs["1"]).all() and torch.equal(outs["1"], outs["0"])
