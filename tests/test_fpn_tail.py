"""FeatureNet's FPN tail for stage 2 in one kernel (csrc/fpn_tail.hip, Ops.fpn_tail): inner1 (1x1, 32 -> 64, bias, exact fp32) + the nearest-x2
upsampled c3 + out2 (3x3, 64 -> 32, zero padding, split-bf16, channel-last output), against the two launches it replaces (the same bits) and
against torch in fp64.  Runs on the host emulation and, with -m gpu, on the MI355X.

Shapes of c2 (N, H, W) (the kernel's unit is a strip of S = 32 output columns x a segment of R = 64 output rows, its march 2 rows per step):
  (2, 24, S)            exactly one strip, less than one segment
  (1, 40, 3S/2)         1.5 strips: the partial strip's columns beyond the image are not stored, the sum is zero outside the image
  (3, 3R/2, 5S/2)       2.5 strips x 1.5 segments x an odd batch: the second segment's warm-up must reproduce the rows above; 18 units on the
                        emulation's 2 resident workgroups, the 4-row ring wraps 17 times per full segment
  (2, 38, 56)           W % S != 0, W % 16 != 0 and H / 2 odd"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from diffmvs_amd import ops as K
from diffmvs_amd import engine as E
from diffmvs_amd import synth

S, R = K.Ops.FPN_TAIL_STRIP, K.Ops.FPN_TAIL_SEGMENT
SHAPES = [(2, 24, S), (1, 40, 3 * S // 2), (3, 3 * R // 2, 5 * S // 2), (2, 38, 56)]


def rnd(*shape, seed=0, lo=-1.0, hi=1.0):
    rs = np.random.RandomState(seed + sum(shape))
    return torch.from_numpy(rs.uniform(lo, hi, shape).astype(np.float32))


def dev(ops, *ts):
    r = [None if t is None else t.to(ops.device).contiguous() for t in ts]
    return r if len(r) > 1 else r[0]


def _bias():
    # of the order of the activations: inner1 applied to out2's padding would NOT be zero
    return rnd(64, seed=11, lo=0.2, hi=0.6)


_CASES = {}


def case(N, H, W):
    """inputs, weights and the fp64 reference of one shape, computed once and shared"""
    key = (N, H, W)
    if key not in _CASES:
        c2 = rnd(N, 32, H, W, seed=1, lo=0.0, hi=1.0)                # (ReLU outputs, like conv2.2's and conv3.2's)
        c3 = rnd(N, 64, H // 2, W // 2, seed=2, lo=0.0, hi=1.0)
        w1, b1 = rnd(64, 32, 1, 1, seed=3) * 0.2, _bias()
        w2 = (rnd(32, 64, 3, 3, seed=4) * 0.1)[K.g4_channels(32)].contiguous()      # an output-channel permutation, as pack_feature(g4=True) does
        intra = F.conv2d(c2.double(), w1.double(), b1.double()) + F.interpolate(c3.double(), scale_factor=2, mode="nearest")
        ref = F.conv2d(intra, w2.double(), padding=1).permute(0, 2, 3, 1).contiguous()
        _CASES[key] = (c2, c3, w1, b1, w2, ref)
    return _CASES[key]


def packed(ops, w1, b1, w2):
    return K.pack_conv2d(dev(ops, w1), dev(ops, b1)), K.pack_conv2d(dev(ops, w2), pad=1)


def two_launches(o, pcs, c2, c3):
    return o.conv2d(pcs[1], o.conv2d(pcs[0], c2, residual=c3, res_mode=K.IN_UPSAMPLE2), out_layout=K.LAYOUT_NHWC)


@pytest.mark.parametrize("N,H,W", SHAPES)
def test_tail_equals_the_two_launches_and_meets_the_split_bound(ops, N, H, W):
    """torch.equal with conv2d(out2, conv2d(inner1, c2, residual=c3, res_mode=IN_UPSAMPLE2), out_layout=NHWC) under ARITH_SPLIT, the outermost two
    rows and columns by name; not the bits of the exact-fp32 launches (the mode is really on); e = max |out - ref| / max |ref| against torch in
    fp64 inside the project's split bound (test_conv1_pair.py, test_stem3.py) with e_f32 = the two exact-fp32 launches on the same inputs (no
    absolute cap on e_f32 is set here: test_conv2d_split_bf16_arithmetic holds the 64-channel layers to theirs)"""
    c2, c3, w1, b1, w2, ref = case(N, H, W)
    pcs = packed(ops, w1, b1, w2)
    so = ops.with_conv_arith(K.ARITH_SPLIT)
    c2d, c3d = dev(ops, c2, c3)
    out = so.fpn_tail(*pcs, c2d, c3d).cpu()
    assert out.shape == (N, H, W, 32) and torch.isfinite(out).all()
    two = two_launches(so, pcs, c2d, c3d).cpu()
    f32 = two_launches(ops, pcs, c2d, c3d).cpu()
    regions = {"top": (slice(0, 2), slice(None)), "bottom": (slice(-2, None), slice(None)), "left": (slice(None), slice(0, 2)),
               "right": (slice(None), slice(-2, None))}
    for name, (ry, rx) in regions.items():
        assert torch.equal(out[:, ry, rx], two[:, ry, rx]), name
    assert torch.equal(out, two), float((out - two).abs().max())
    assert not torch.equal(out, f32)
    scale = float(ref.abs().max())
    e_split, e_f32 = float((out.double() - ref).abs().max()) / scale, float((f32.double() - ref).abs().max()) / scale
    print("fpn tail split vs fp64: %.2e   two exact-fp32 launches vs fp64: %.2e" % (e_split, e_f32))
    assert e_split < 4.0 * e_f32 + 2e-7, (e_split, e_f32)


def test_padding_would_not_be_zero_after_the_bias():
    """the premise of the border assertions: inner1 applied to zero padding is its bias, far from zero, so a kernel that pads out2 with
    bias + 0 instead of zeros fails them"""
    assert float(F.conv2d(torch.zeros(1, 32, 1, 1), torch.zeros(64, 32, 1, 1), _bias()).min()) > 0.1


@pytest.mark.parametrize("N,H,W", [(3, 3 * R // 2, 5 * S // 2), (2, 38, 56)])
def test_tail_depends_only_on_the_position_in_the_image(ops, N, H, W):
    """an image gives the same bits alone and as an item of the batch; the grid forced to 1 and to 2 workgroups gives the same bits; so do two
    launches in a row"""
    c2, c3, w1, b1, w2, _ = case(N, H, W)
    pcs = packed(ops, w1, b1, w2)
    so = ops.with_conv_arith(K.ARITH_SPLIT)
    c2d, c3d = dev(ops, c2, c3)
    whole = so.fpn_tail(*pcs, c2d, c3d).cpu()
    assert torch.equal(so.fpn_tail(*pcs, c2d, c3d).cpu(), whole)
    last = so.fpn_tail(*pcs, c2d[N - 1:N].contiguous(), c3d[N - 1:N].contiguous()).cpu()
    assert torch.equal(last, whole[N - 1:N])
    for grid in (1, 2):
        assert torch.equal(so.fpn_tail(*pcs, c2d, c3d, tune=grid).cpu(), whole), grid


def _entry(ops, c2p, c3p, w1p, b1p, w2p, yp, n, h, w, tune=0):
    ops.lib.call("dmvs_featurenet_fpn_tail_f32", c2p, c3p, w1p, b1p, w2p, yp, n, h, w, tune, ops.stream())


@pytest.mark.parametrize("N,H,W", [(1, 40, 3 * S // 2), (2, 38, 56)])
def test_tail_stays_inside_its_tensors(ops, N, H, W):
    """c2, c3 and the output as 16-byte aligned views inside larger flat buffers whose surroundings are NaN (inputs) or a sentinel (output): the
    result is finite and equal to the plain-tensor result, the sentinels are untouched -- a staged piece that strays outside a tensor would
    bring a NaN in"""
    c2, c3, w1, b1, w2, _ = case(N, H, W)
    pcs = packed(ops, w1, b1, w2)
    so = ops.with_conv_arith(K.ARITH_SPLIT)
    plain = so.fpn_tail(*pcs, *dev(ops, c2, c3)).cpu()
    G = 64      # guard floats on either side (a multiple of 4: the views stay 16-byte aligned)

    def banded(t, fill):
        flat = torch.full((t.numel() + 2 * G,), fill, dtype=torch.float32, device=ops.device)
        view = flat[G:G + t.numel()].view(t.shape)
        assert view.data_ptr() % 16 == 0
        return flat, view

    f2, v2 = banded(c2, float("nan"))
    f3, v3 = banded(c3, float("nan"))
    v2.copy_(dev(ops, c2))
    v3.copy_(dev(ops, c3))
    fo, vo = banded(plain, -12345.0)
    via_ops = so.fpn_tail(*pcs, v2, v3).cpu()
    assert torch.isfinite(via_ops).all() and torch.equal(via_ops, plain)
    _entry(ops, K._ptr(v2), K._ptr(v3), K._ptr(pcs[0].weight), K._ptr(pcs[0].shift), K._ptr(K.split_weights(pcs[1])), K._ptr(vo), N, H, W)
    fo = fo.cpu()
    assert torch.isfinite(fo).all() and torch.equal(fo[G:-G].view(plain.shape), plain)
    assert bool((fo[:G] == -12345.0).all()) and bool((fo[-G:] == -12345.0).all())


def test_tail_rejects_what_it_does_not_handle(ops):
    c2, c3, w1, b1, w2, _ = case(2, 24, S)
    pcs = packed(ops, w1, b1, w2)
    w1p, b1p, w2p = K._ptr(pcs[0].weight), K._ptr(pcs[0].shift), K._ptr(K.split_weights(pcs[1]))
    g2, g3 = dev(ops, c2, c3)
    out = torch.empty(2, 24, S, 32, device=ops.device)
    _entry(ops, K._ptr(g2), K._ptr(g3), w1p, b1p, w2p, K._ptr(out), 2, 24, S)          # (the call form itself is accepted)

    def rejected(a2, a3, n, h, w):
        assert not ops.fpn_tail_supported(a2, a3)
        with pytest.raises(K._lib.DmvsError):
            ops.fpn_tail(*pcs, a2, a3)
        with pytest.raises(K._lib.DmvsError):
            _entry(ops, K._ptr(a2), K._ptr(a3), w1p, b1p, w2p, K._ptr(out), n, h, w)

    rejected(dev(ops, rnd(1, 32, 23, S, seed=1)), dev(ops, rnd(1, 64, 11, S // 2, seed=1)), 1, 23, S)               # odd H
    rejected(dev(ops, rnd(1, 32, 24, S - 4, seed=1)), dev(ops, rnd(1, 64, 12, S // 2 - 2, seed=1)), 1, 24, S - 4)   # W % 8 != 0
    flat = dev(ops, rnd(32 * 24 * S + 4, seed=2))
    view = flat[1:1 + 32 * 24 * S].view(1, 32, 24, S)                                                              # 4 bytes off a 16-byte boundary
    rejected(view, g3[:1].contiguous(), 1, 24, S)
    flat3 = dev(ops, rnd(64 * 12 * (S // 2) + 4, seed=3))
    rejected(g2[:1].contiguous(), flat3[1:1 + 64 * 12 * (S // 2)].view(1, 64, 12, S // 2), 1, 24, S)
    for a2, a3 in ((dev(ops, rnd(1, 16, 24, S, seed=1)), g3[:1].contiguous()), (g2[:1].contiguous(), dev(ops, rnd(1, 32, 12, S // 2, seed=1)))):
        assert not ops.fpn_tail_supported(a2, a3)                                                                   # wrong channel counts
        with pytest.raises(K._lib.DmvsError):
            ops.fpn_tail(*pcs, a2, a3)
    pc_other = K.pack_conv2d(dev(ops, rnd(64, 16, 1, 1, seed=5)), dev(ops, _bias()))
    with pytest.raises(K._lib.DmvsError):
        ops.fpn_tail(pc_other, pcs[1], g2, g3)
    with pytest.raises(K._lib.DmvsError):
        ops.fpn_tail(pcs[0], pcs[0], g2, g3)
    ptrs = [K._ptr(g2), K._ptr(g3), w1p, b1p, w2p, K._ptr(out)]
    for missing in (0, 1, 2, 4, 5):                                                                                # null pointers (the bias may be null)
        with pytest.raises(K._lib.DmvsError):
            _entry(ops, *[None if i == missing else p for i, p in enumerate(ptrs)], 2, 24, S)
    with pytest.raises(K._lib.DmvsError):                                                                          # 64 * H * W >= 2^31
        _entry(ops, *ptrs, 1, 8192, 4096)

    class Big:      # a plane too large for 32-bit offsets, by its shape alone
        dtype = torch.float32

        def __init__(self, shape):
            self.shape = shape

        def dim(self):
            return 4

        def is_contiguous(self):
            return True

        def data_ptr(self):
            return 0

    assert not ops.fpn_tail_supported(Big((1, 32, 8192, 4096)), Big((1, 64, 4096, 2048)))


def _feature_weights(ops, variant="diffmvs", seed=5):
    from models import CasDiffMVS
    model = CasDiffMVS(synth.make_args(variant, numdepth_initial=8), test=True).eval()
    sd = synth.synth_state_dict(model.state_dict(), seed)
    return E.pack_feature({k: v.to(ops.device) for k, v in sd.items()}, g4=True)


def test_run_feature_switch_and_fallback(ops, monkeypatch):
    """run_feature takes the kernel once under conv_arith = "split" where it applies, and the two launches otherwise: DMVS_FPN_TAIL=0, the fp32
    arithmetic, a pack with an out3 (CasDiffMVS: the sum has a second reader), layout = NCHW and a width the kernel does not take (c3 rows that
    are no 16-byte multiples) -- and the features are the same bits on and off"""
    f = _feature_weights(ops)
    assert "out3" not in f
    so = ops.with_conv_arith(K.ARITH_SPLIT)
    calls = []
    real = K.Ops.fpn_tail
    monkeypatch.setattr(K.Ops, "fpn_tail", lambda self, *a, **kw: (calls.append(1), real(self, *a, **kw))[1])

    def feats(o, x, ff=f, **kw):
        return {k: v.cpu() for k, v in E.run_feature(o, ff, x, **kw).items()}

    x = dev(ops, rnd(1, 3, 96, 4 * S, seed=1))         # c2 is 24 x S: one strip
    monkeypatch.setenv("DMVS_FPN_TAIL", "1")
    on = feats(so, x)
    assert len(calls) == 1
    monkeypatch.setenv("DMVS_FPN_TAIL", "0")
    off = feats(so, x)
    assert len(calls) == 1
    assert on.keys() == off.keys() and all(torch.equal(on[k], off[k]) for k in on)
    monkeypatch.setenv("DMVS_FPN_TAIL", "1")
    feats(ops, x)                                       # fp32 arithmetic: untouched
    assert len(calls) == 1
    feats(so, x, layout=K.LAYOUT_NCHW)                  # planar features: the two launches
    assert len(calls) == 1
    fc = _feature_weights(ops, "casdiffmvs")
    assert "out3" in fc
    feats(so, x, ff=fc)                                 # the sum feeds inner2 as well: the two launches
    assert len(calls) == 1
    xb = dev(ops, rnd(1, 3, 96, 4 * S + 16, seed=1))    # c2 rows of S + 4 floats: unsupported, the two launches
    feats(so, xb)
    assert len(calls) == 1


def test_model_forward_with_and_without_the_tail(ops, monkeypatch):
    """the whole forward (64 x 160, B = 1, 3 views, conv_arith = "split") with DMVS_FPN_TAIL = 1 and = 0: the same depth maps bit for bit"""
    from models import CasDiffMVS
    args = synth.make_args("diffmvs", numdepth_initial=8, conv_arith="split")
    model = CasDiffMVS(args, test=True).eval()
    model.load_state_dict(synth.synth_state_dict(model.state_dict(), 7), strict=True)
    if ops.device.type != "cpu":
        model = model.to(ops.device)
    imgs, proj, dv = synth.synth_inputs(64, 160, 2, B=1, seed=3)
    eng = model.engine(ops)
    assert eng.conv_arith == "split"
    calls = []
    real = K.Ops.fpn_tail
    monkeypatch.setattr(K.Ops, "fpn_tail", lambda self, *a, **kw: (calls.append(1), real(self, *a, **kw))[1])
    outs = {}
    for knob in ("1", "0"):
        monkeypatch.setenv("DMVS_FPN_TAIL", knob)
        with torch.no_grad():
            outs[knob] = eng.forward(imgs, proj, dv, noise_fn=synth.NoiseSource(11))["depth"][-1].cpu()
    assert len(calls) >= 1
    assert torch.isfinite(outs["1"]).all() and torch.equal(outs["1"], outs["0"])
