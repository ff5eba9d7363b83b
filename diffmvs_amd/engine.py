"""Inference engine: the DiffMVS / CasDiffMVS depth-estimation forward as a sequence of
libdmvs_hip.so kernel launches on one HIP stream.

It consumes the reference's flat checkpoint layout and the constructor
namespace, packs the weights once into kernel layout (eval-BN folded into per-channel
scale/shift, weight-standardised convs standardised, time-embedding scale/shift tables
evaluated -- all parameter-only constant folding), and then `forward` issues only kernel
launches plus torch memory plumbing (allocation, cat of the input images).  Nothing in
here computes on the CPU and nothing falls back to ATen operators for the hot path.

Reference call graph followed (models/diffusion.py:139-295):
  FeatureNet x V, ContextNet -> InitialCost (stage 1) -> [DiffusionUpdateBlockDepth (stage 2, 3)].
"""
from __future__ import annotations

import math
import os
from typing import Callable, Dict, List, Optional

import torch
import torch.nn.functional as F

from . import ops as K
from .ops import Ops, PackedConv, pack_conv2d, pack_conv3d

_RATIOS = [4, 2, 1]                      # depth_interals_ratio default (diffusion.py:15)
_MULTS = [(1,), (1, 2), (1, 2, 4)]       # unet_dim_mults (diffusion.py:33)


def _bn(sd, p):
    return {k: sd[f"{p}.{k}"] for k in ("weight", "bias", "running_mean", "running_var")}


def _cw(sd, p, **kw):
    """module.Conv2d / ConvBnReLU / ConvBn wrapper -> packed conv with eval-BN folded (module.py:24-58, :279-301)."""
    return pack_conv2d(sd[p + ".conv.weight"], sd.get(p + ".conv.bias"),
                       bn=_bn(sd, p + ".bn") if (p + ".bn.weight") in sd else None, **kw)


def pack_feature(sd, p="feature", g4=False, feat_dtype=torch.float32):
    """FeatureNet weights (models/module.py:357-420).  g4: the output convolutions emit their channels in the
    group-interleaved NHWC-g4 order the quad-per-pixel warp kernels read (an output-channel permutation of the weights:
    free at run time; identity for 16-bit feature storage)."""
    order = (lambda w: w[K.g4_channels(w.shape[0], feat_dtype).to(w.device)].contiguous()) if g4 else (lambda w: w)
    f = {"conv0.0": _cw(sd, p + ".conv0.0", pad=1), "conv0.1": _cw(sd, p + ".conv0.1", pad=1)}
    for i in (1, 2, 3):
        f[f"conv{i}.0"] = _cw(sd, f"{p}.conv{i}.0", stride=2, pad=2)
        f[f"conv{i}.1"], f[f"conv{i}.2"] = _cw(sd, f"{p}.conv{i}.1", pad=1), _cw(sd, f"{p}.conv{i}.2", pad=1)
    f["out1"] = pack_conv2d(order(sd[p + ".out1.weight"]))
    f["inner1"] = pack_conv2d(sd[p + ".inner1.weight"], sd[p + ".inner1.bias"])
    f["out2"] = pack_conv2d(order(sd[p + ".out2.weight"]), pad=1)
    if (p + ".out3.weight") in sd:
        f["inner2"] = pack_conv2d(sd[p + ".inner2.weight"], sd[p + ".inner2.bias"])
        f["out3"] = pack_conv2d(order(sd[p + ".out3.weight"]), pad=1)
    return f


# On: 1.12 against 0.69 + 0.58 ms per 96-image launch (profiles/stem3_kernel_stats_*.csv); the step 0.5-1.2 ms shorter in three interleaved
# sessions, in one of them every fused run ahead of every other run (profiles/stem3_step_ab.json); DMVS_STEM_FUSE=0 turns it off
STEM_FUSE_DEFAULT = "1"


def stem3_applies(o: Ops, x):
    """conv1.0 runs inside the stem kernel (Ops.featurenet_stem3) under conv_arith = "split" -- the kernel computes conv0.1 and conv1.0 in split
    arithmetic only -- wherever its geometry applies; DMVS_STEM_FUSE=0 is the A/B knob: the stem and conv1.0 as two launches"""
    return (o.conv_arith == K.ARITH_SPLIT and os.environ.get("DMVS_STEM_FUSE", STEM_FUSE_DEFAULT) != "0" and
            o.featurenet_stem3_supported(x))


CONV1_PAIR_DEFAULT = "1"


def conv1_pair_applies(o: Ops, c1):
    """conv1.1 + conv1.2 run as one kernel (Ops.conv1_pair) under conv_arith = "split" -- the kernel computes in split arithmetic only, and
    gives the two launches' bits -- wherever its geometry applies and the map is at least one strip wide (a narrower map leaves most of a
    workgroup's statically assigned 16-column groups empty; the two launches' 16 x 16 tiles fit it better); DMVS_CONV1_PAIR=0 is the A/B knob:
    the two launches"""
    return (o.conv_arith == K.ARITH_SPLIT and os.environ.get("DMVS_CONV1_PAIR", CONV1_PAIR_DEFAULT) != "0" and
            o.conv1_pair_supported(c1) and c1.shape[3] >= K.Ops.CONV1_PAIR_STRIP)


# On: 3.72 against 4.52 ms per 576 images for the two launches (tools/conv_bench.py row); the step 0.6-0.9 ms shorter in three interleaved rounds,
# every fused run ahead of every other run (profiles/fpn_tail_step_ab.json); DMVS_FPN_TAIL=0 turns it off
FPN_TAIL_DEFAULT = "1"


def fpn_tail_applies(o: Ops, f, c2, c3, layout, feat_dtype):
    """inner1 + the upsample-add + out2 run as one kernel (Ops.fpn_tail) under conv_arith = "split" -- out2 computes in split arithmetic only
    there, and the kernel gives the two launches' bits -- for channel-last fp32 features, when the sum has no other reader (no out3: DiffMVS)
    and the geometry applies; DMVS_FPN_TAIL=0 is the A/B knob: the two launches"""
    return (o.conv_arith == K.ARITH_SPLIT and layout == K.LAYOUT_NHWC and feat_dtype == torch.float32 and "out3" not in f and
            os.environ.get("DMVS_FPN_TAIL", FPN_TAIL_DEFAULT) != "0" and o.fpn_tail_supported(c2, c3))


def run_feature(o: Ops, f, x, layout=K.LAYOUT_NHWC, feat_dtype=torch.float32):
    """x [N,3,H,W] -> {'stage1': [N,H/8,W/8,48], 'stage2': [N,H/4,W/4,32], ('stage3': [N,H/2,W/2,16])} (NHWC by
    default: the layout the warp kernels read; feat_dtype bf16 / fp16 = reduced-precision feature storage, rounded in the
    output convolutions' epilogue)."""
    R = K.ACT_RELU
    if stem3_applies(o, x):
        c1 = o.featurenet_stem3(f["conv0.0"], f["conv0.1"], f["conv1.0"], x)      # conv0.0 + conv0.1 + conv1.0: c0 has no other reader, it stays in LDS
    else:
        c0 = o.featurenet_stem(f["conv0.0"], f["conv0.1"], x)      # conv0.0 + conv0.1 fused: the 8-channel intermediate stays in LDS
        c1 = o.conv2d(f["conv1.0"], c0, act=R)
    if conv1_pair_applies(o, c1):
        c1 = o.conv1_pair(f["conv1.1"], f["conv1.2"], c1)      # conv1.1 + conv1.2: the map between them has no other reader, it stays in LDS
    else:
        c1 = o.conv2d(f["conv1.2"], o.conv2d(f["conv1.1"], c1, act=R), act=R)
    c2 = o.conv2d(f["conv2.2"], o.conv2d(f["conv2.1"], o.conv2d(f["conv2.0"], c1, act=R), act=R), act=R)
    c3 = o.conv2d(f["conv3.2"], o.conv2d(f["conv3.1"], o.conv2d(f["conv3.0"], c2, act=R), act=R), act=R)
    out = {"stage1": o.conv2d(f["out1"], c3, out_layout=layout, out_dtype=feat_dtype)}
    if fpn_tail_applies(o, f, c2, c3, layout, feat_dtype):
        out["stage2"] = o.fpn_tail(f["inner1"], f["out2"], c2, c3)      # inner1 + upsample-add + out2: the sum has no other reader, it stays in LDS
        return out
    intra = o.conv2d(f["inner1"], c2, residual=c3, res_mode=K.IN_UPSAMPLE2)
    out["stage2"] = o.conv2d(f["out2"], intra, out_layout=layout, out_dtype=feat_dtype)
    if "out3" in f:
        intra = o.conv2d(f["inner2"], c1, residual=intra, res_mode=K.IN_UPSAMPLE2)
        out["stage3"] = o.conv2d(f["out3"], intra, out_layout=layout, out_dtype=feat_dtype)
    return out


def pack_context_trunk(sd, p="context"):
    """ContextNet body (models/module.py:321-343)."""
    c = {"conv1": _cw(sd, p + ".conv1", pad=1)}
    for li in (1, 2, 3):
        for bi in (0, 1):
            q = f"{p}.layer{li}.{bi}"
            c[f"{li}.{bi}.conv1"] = _cw(sd, q + ".conv1", stride=(2 if bi == 0 else 1), pad=1)
            c[f"{li}.{bi}.conv2"] = _cw(sd, q + ".conv2", pad=1)
            if bi == 0:
                c[f"{li}.{bi}.down"] = _cw(sd, q + ".downsample", stride=2, pad=1)
    return c


def run_context_trunk(o: Ops, c, x):
    """-> {0: 1/8-resolution map (48 ch), 1: 1/4 (32 ch), 2: 1/2 (16 ch)}: the inputs of output1/2/3."""
    R = K.ACT_RELU
    x = o.conv2d(c["conv1"], x, act=R)
    taps = {}
    for li in (1, 2, 3):
        y = o.conv2d(c[f"{li}.0.conv1"], x, act=R)
        xd = o.conv2d(c[f"{li}.0.down"], x)
        x = o.conv2d(c[f"{li}.0.conv2"], y, residual=xd, act=R)       # relu(x + y), module.py:315-319
        y = o.conv2d(c[f"{li}.1.conv1"], x, act=R)
        x = o.conv2d(c[f"{li}.1.conv2"], y, residual=x, act=R)
        taps[3 - li] = x
    return taps


def pack_pvw(sd, p):
    """PixelViewWeight (models/module.py:450-463)."""
    return (pack_conv3d(sd[p + ".conv.0.conv.weight"], bn=_bn(sd, p + ".conv.0.bn")),
            pack_conv3d(sd[p + ".conv.1.weight"], sd[p + ".conv.1.bias"]))


def run_pvw(o: Ops, pk, cor):
    """cor [N,G,D,H,W] -> [N,H,W] = max_d sigmoid(conv1(relu(bn(conv0))))."""
    N, _, D, H, W = cor.shape
    x = o.conv3d(pk[1], o.conv3d(pk[0], cor, act=K.ACT_RELU))
    return o.sigmoid_max_d(x.view(N, D, H, W))


def pack_costreg(sd, p):
    """CostRegNet_small (models/module.py:422-448)."""
    reg = {}
    for i, st in ((0, 1), (1, 1), (2, 2), (3, 1), (4, 2), (5, 1)):
        reg[i] = pack_conv3d(sd[f"{p}.conv{i}.conv.weight"], bn=_bn(sd, f"{p}.conv{i}.bn"), stride=st)
    for i in (6, 7):
        reg[i] = pack_conv3d(sd[f"{p}.conv{i}.conv.weight"], bn=_bn(sd, f"{p}.conv{i}.bn"), stride=2, transposed=True)
    reg["prob"] = pack_conv3d(sd[p + ".prob.weight"])
    return reg


def run_costreg(o: Ops, reg, x):
    R = K.ACT_RELU
    c1 = o.conv3d(reg[1], o.conv3d(reg[0], x, act=R), act=R)
    c3 = o.conv3d(reg[3], o.conv3d(reg[2], c1, act=R), act=R)
    x = o.conv3d(reg[5], o.conv3d(reg[4], c3, act=R), act=R)
    x = o.conv3d(reg[6], x, act=R, residual=c3)
    x = o.conv3d(reg[7], x, act=R, residual=c1)
    return o.conv3d(reg["prob"], x)


def pack_mask(sd, p):
    """mask head: Conv3x3 -> ReLU -> Conv1x1 (module.py:481-485, update.py:335-339)."""
    return (pack_conv2d(sd[p + ".0.weight"], sd[p + ".0.bias"], pad=1), pack_conv2d(sd[p + ".2.weight"], sd[p + ".2.bias"]))


def run_mask(o: Ops, pk, context, post_scale=0.25):
    return o.conv2d(pk[1], o.conv2d(pk[0], context, act=K.ACT_RELU), post_scale=post_scale)


def mask_head_fuses(pk, up_ratio) -> bool:
    """the head's 1x1 layer runs inside the convex-upsampling kernel (Ops.mask_upsample4: DiffMVS, ratio 4, 64 -> 144 channels); DMVS_MASK_FUSE=0
    keeps the two launches (A/B runs and the bit-identity test)"""
    return up_ratio == 4 and pk[1].cin == 64 and pk[1].cout == 144 and pk[1].scale is None and os.environ.get("DMVS_MASK_FUSE", "1") != "0"


def pack_gru(sd, p):
    """SepConvGRU (models/module.py:152-179)."""
    g = {}
    for n, pad in (("1", (0, 2)), ("2", (2, 0))):
        for gate in "zrq":
            g[gate + n] = pack_conv2d(sd[f"{p}.conv{gate}{n}.weight"], sd[f"{p}.conv{gate}{n}.bias"], pad=pad)
        # z and r read the same input: ONE convolution with the two weight sets stacked along cout ([z | r])
        g["zr" + n] = pack_conv2d(torch.cat([sd[f"{p}.convz{n}.weight"], sd[f"{p}.convr{n}.weight"]], 0),
                                  torch.cat([sd[f"{p}.convz{n}.bias"], sd[f"{p}.convr{n}.bias"]], 0), pad=pad)
    return g


def run_gru(o: Ops, g, h, x):
    hd = h.shape[1]
    merged = os.environ.get("DMVS_GRU_MERGE", "1") != "0"      # A/B knob: 0 = z and r as two launches
    for n in ("1", "2"):     # horizontal then vertical pass (module.py:164-177)
        if merged:
            # [B, 2*hd, H, W] = [z | r * h]: the r half of sigmoid([convz | convr]([h, x])) is multiplied by h in the epilogue (out_mul), so
            # the candidate convolution reads a plain concatenated input instead of gating its staged tile in LDS per chunk
            zr = o.conv2d(g["zr" + n], h, x, act=K.ACT_SIGMOID, out_mul=h, out_mul_c0=hd)
            h = o.conv2d(g["q" + n], zr[:, hd:], x, in0_cstride=2 * hd, act=K.ACT_TANH, gru_z=zr[:, :hd], gru_h=h, gate_cstride=2 * hd)
        else:
            z = o.conv2d(g["z" + n], h, x, act=K.ACT_SIGMOID)
            r = o.conv2d(g["r" + n], h, x, act=K.ACT_SIGMOID)
            h = o.conv2d(g["q" + n], h, x, mul0=r, act=K.ACT_TANH, gru_z=z, gru_h=h)
    return h


def pack_encoder(sd, p):
    """ConditionEncoder (models/update.py:276-297)."""
    return {n: pack_conv2d(sd[f"{p}.{n}.weight"], sd[f"{p}.{n}.bias"], pad=1)
            for n in ("convc1", "convc2", "convd1", "convd2", "output")}


def run_encoder(o: Ops, enc, cost, samples, out=None, out_cstride=None, out_coffset=0):
    """-> relu(output(cat(c_feat, d_feat))): the first out_chs-1 channels of the encoder result."""
    R = K.ACT_RELU
    cf = o.conv2d(enc["convc2"], o.conv2d(enc["convc1"], cost, act=R), act=R)
    df = o.conv2d(enc["convd2"], o.conv2d(enc["convd1"], samples, act=R), act=R)
    return o.conv2d(enc["output"], cf, df, act=R, out=out, out_cstride=out_cstride, out_coffset=out_coffset)


class GnArena:
    """GroupNorm statistics scratch: [slot][B*4*2] doubles, zeroed with one memset per forward; the
    producing conv's epilogue accumulates into a slot, groupnorm_apply consumes it.
    One buffer PER BATCH SIZE, kept for the life of the engine (16 KB x B): a captured HIP graph holds the raw pointer of
    the buffer it was captured with in its memset / atomics / reads, so a buffer must never go back to the allocator
    while a graph of that batch size may still be replayed (an eval run whose last batch is smaller alternates sizes)."""
    SLOTS = 256

    def __init__(self, ops: Ops):
        self.ops, self.bufs, self.buf, self.next = ops, {}, None, 0

    def reset(self, B):
        self.buf = self.bufs.get(B)
        if self.buf is None:
            self.buf = self.bufs[B] = torch.zeros(self.SLOTS, B * 8, dtype=torch.float64, device=self.ops.device)
        else:
            self.buf.zero_()
        self.next = 0

    def slot(self):
        if self.next >= self.SLOTS:
            raise RuntimeError("GroupNorm statistics arena exhausted")
        s = self.buf[self.next]
        self.next += 1
        return s


def run_resblock(o: Ops, arena: GnArena, rb, x0, x1=None, scale_shift=None):
    """ResnetBlock (update.py:147-159): two WS-conv/GroupNorm/SiLU blocks + residual."""
    st1, st2 = arena.slot(), arena.slot()
    h = o.conv2d(rb["c1"], x0, x1, gn_stats=st1)
    h = o.groupnorm_apply(h, rb["g1"][0], rb["g1"][1], 4, st1, scale_shift=scale_shift, out=h)
    h2 = o.conv2d(rb["c2"], h, gn_stats=st2)
    if rb["res"] is not None:
        res = o.conv2d(rb["res"], x0, x1)
    else:
        assert x1 is None
        res = x0
    return o.groupnorm_apply(h2, rb["g2"][0], rb["g2"][1], 4, st2, residual=res, out=h2)


def run_unet(o: Ops, arena: GnArena, ub, E, ctx_part, hidden, ss_of):
    """Unet.forward (update.py:245-274).  The Unet input is cat(relu(context), encoder output) (update.py:497-498); its
    7x7 init_conv is linear in the input channels, so the context half -- the same tensor in every GRU iteration and DDIM
    step of the stage -- is convolved ONCE per stage (ctx_part = init_conv[:, :cd](context) + bias) and each iteration adds
    the encoder half's convolution to it: E [B,cd,H,W], hidden [B,hd,h,w]; ss_of(rb) -> [B,2*dim_out] | None."""
    x = o.conv2d(ub.init_enc, E, residual=ctx_part)
    r = x
    skips = []
    L = len(ub.mults)
    for i, (blk, ds) in enumerate(ub.downs):
        x = run_resblock(o, arena, blk, x, None, ss_of(blk))
        skips.append(x)
        x = o.conv2d(ds, x, in_mode=(K.IN_UNSHUFFLE2 if i < L - 1 else K.IN_PLAIN))
    hidden = run_gru(o, ub.gru, hidden, x)
    x = run_resblock(o, arena, ub.mid, hidden, None, None)      # mid has no time MLP
    for i, (blk, us) in enumerate(ub.ups):
        x = run_resblock(o, arena, blk, x, skips.pop(), ss_of(blk))
        x = o.conv2d(us, x, in_mode=(K.IN_UPSAMPLE2 if i < L - 1 else K.IN_PLAIN))
    x = run_resblock(o, arena, ub.final, x, r, ss_of(ub.final))
    delta = o.conv2d(ub.final_conv, x)
    conf = o.conv2d(ub.conf, x, act=K.ACT_SIGMOID)
    return hidden, delta, conf


class _UpdateBlock:
    """Packed weights of one DiffusionUpdateBlockDepth (reference models/update.py:299-391)."""

    def __init__(self, sd: Dict[str, torch.Tensor], p: str, args, stage: int, up_ratio: int):
        self.p = p
        self.stage = stage
        self.iters = args.stage_iters[stage]
        self.cd = args.context_dim[stage]
        self.hd = args.hidden_dim[stage]
        self.n = args.CostNum[stage]
        self.dim = args.unet_dim[stage]
        self.mults = _MULTS[stage]
        self.timesteps = args.timesteps[stage]
        st = args.sampling_timesteps[stage]
        self.sampling_timesteps = self.timesteps if st is None else st
        self.eta = args.ddim_eta[stage]
        self.scale = args.scale[stage]
        self.up_ratio = up_ratio
        c2 = lambda name, **kw: pack_conv2d(sd[f"{p}.{name}.weight"], sd.get(f"{p}.{name}.bias"), **kw)  # noqa: E731
        self.enc = pack_encoder(sd, p + ".encoder")
        self.mask = pack_mask(sd, p + ".mask")
        self.fused_up = mask_head_fuses(self.mask, up_ratio)      # the mask never leaves registers: see Engine.forward
        u = p + ".unet"
        wi, bi = sd[f"{p}.unet.init_conv.weight"], sd.get(f"{p}.unet.init_conv.bias")
        self.init_ctx = pack_conv2d(wi[:, :self.cd], bi, pad=3)        # input channels = cat(relu(context), encoder output)
        self.init_enc = pack_conv2d(wi[:, self.cd:], None, pad=3)
        L = len(self.mults)
        self.downs = []
        for i in range(L):
            blk = self._resblock(sd, f"{u}.downs.{i}.0")
            if i < L - 1:
                ds = pack_conv2d(sd[f"{u}.downs.{i}.1.1.weight"], sd[f"{u}.downs.{i}.1.1.bias"])
            else:
                ds = pack_conv2d(sd[f"{u}.downs.{i}.1.weight"], sd[f"{u}.downs.{i}.1.bias"], pad=1)
            self.downs.append((blk, ds))
        self.gru = pack_gru(sd, u + ".gru")
        self.mid = self._resblock(sd, f"{u}.mid")
        self.ups = []
        for i in range(L):
            blk = self._resblock(sd, f"{u}.ups.{i}.0")
            if i < L - 1:
                us = pack_conv2d(sd[f"{u}.ups.{i}.1.1.weight"], sd[f"{u}.ups.{i}.1.1.bias"], pad=1)
            else:
                us = pack_conv2d(sd[f"{u}.ups.{i}.1.weight"], sd[f"{u}.ups.{i}.1.bias"], pad=1)
            self.ups.append((blk, us))
        self.final = self._resblock(sd, f"{u}.final_res_block")
        self.final_conv, self.conf = c2("unet.final_conv"), c2("unet.conf")
        self.acp = sd[f"{p}.alphas_cumprod"].float()
        self.sqrt_recip_acp = sd[f"{p}.sqrt_recip_alphas_cumprod"].float()
        self.sqrt_recipm1_acp = sd[f"{p}.sqrt_recipm1_alphas_cumprod"].float()
        # DDIM schedule (update.py:469-471) and the time-conditioned scale/shift of every ResnetBlock,
        # evaluated once: they depend on parameters and the integer time step only.
        times = torch.linspace(-1, self.timesteps - 1, steps=self.sampling_timesteps + 1)
        times = list(reversed(times.int().tolist()))
        self.time_pairs = list(zip(times[:-1], times[1:]))
        self.ss_tables = {t: self._scale_shift_table(sd, u, t) for t, _ in self.time_pairs}

    @staticmethod
    def _resblock(sd, p):
        rb = {
            "p": p,
            "c1": pack_conv2d(sd[p + ".block1.proj.weight"], sd[p + ".block1.proj.bias"], pad=1, standardize=True),
            "c2": pack_conv2d(sd[p + ".block2.proj.weight"], sd[p + ".block2.proj.bias"], pad=1, standardize=True),
            "g1": (sd[p + ".block1.norm.weight"].float().contiguous(), sd[p + ".block1.norm.bias"].float().contiguous()),
            "g2": (sd[p + ".block2.norm.weight"].float().contiguous(), sd[p + ".block2.norm.bias"].float().contiguous()),
            "res": None,
            "has_mlp": (p + ".mlp.1.weight") in sd,
        }
        if (p + ".res_conv.weight") in sd:
            rb["res"] = pack_conv2d(sd[p + ".res_conv.weight"], sd[p + ".res_conv.bias"])
        return rb

    def _scale_shift_table(self, sd, u, t: int):
        """SinusoidalPosEmb -> Linear -> GELU -> Linear (update.py:50-62, :204-211), then each block's
        SiLU -> Linear (update.py:138-153).  Returns {block prefix: [1, 2*dim_out]}."""
        dev = sd[u + ".time_mlp.1.weight"].device
        half = self.dim // 2
        k = math.log(10000) / (half - 1)
        freqs = torch.exp(torch.arange(half, device=dev) * -k)
        e = torch.tensor([float(t)], device=dev)[:, None] * freqs[None, :]
        e = torch.cat((e.sin(), e.cos()), -1)
        e = F.gelu(F.linear(e, sd[u + ".time_mlp.1.weight"], sd[u + ".time_mlp.1.bias"]))
        te = F.linear(e, sd[u + ".time_mlp.3.weight"], sd[u + ".time_mlp.3.bias"])
        table = {}
        blocks = [b for b, _ in self.downs] + [self.mid] + [b for b, _ in self.ups] + [self.final]
        for rb in blocks:
            if rb["has_mlp"]:
                pp = rb["p"]
                table[pp] = F.linear(F.silu(te), sd[pp + ".mlp.1.weight"], sd[pp + ".mlp.1.bias"]).float().contiguous()
        return table


class SceneFeatureStore:
    """FeatureNet outputs of every image of a scene, computed ONCE: {stage: [N,h,w,C]} in the layout the warp kernels read.
    The reference's harness (test.py:92-127) -- and a per-sample forward here -- runs FeatureNet on all V images of every reference
    view, so an image that is a source view of ~V-1 neighbours is pushed through the network ~V times per scene; 288 GB of HBM hold
    every view's features of any scene (DTU, 49 views at 1600x1152: 2.4 GB), so the scene loop keeps them resident and each
    reference view only gathers its rows.  `gather` returns the view-major [V*B,h,w,C] stack Engine.forward(feats=...) consumes:
    plain device copies of rows, bit-identical to what a per-sample forward computes."""

    def __init__(self, engine: "Engine", images: torch.Tensor, chunk: int = 64):
        o = engine.ops
        images = images.to(o.device).float().contiguous()
        parts = [run_feature(o, engine.feat, images[i:i + chunk], feat_dtype=engine.feat_dtype) for i in range(0, images.shape[0], chunk)]
        self.feats = {k: (parts[0][k] if len(parts) == 1 else torch.cat([p[k] for p in parts], 0)) for k in parts[0]}
        self.n_views = images.shape[0]

    def gather(self, view_ids: torch.Tensor, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        """view_ids [B,V] (column 0 = the reference view) -> {stage: [V*B,h,w,C]}, row v*B + b = features of view_ids[b, v].
        out: buffers to gather INTO (the static inputs of a captured graph: one copy instead of gather + copy)"""
        idx = view_ids.to(next(iter(self.feats.values())).device).long().t().reshape(-1)
        if out is not None:
            for k, f in self.feats.items():
                torch.index_select(f, 0, idx, out=out[k])
            return out
        return {k: f.index_select(0, idx) for k, f in self.feats.items()}


class GraphedForward:
    """One HIP graph of the whole eval forward for fixed input shapes: ~350 kernel launches replayed by a single
    hipGraphLaunch.  Small batches are launch-bound in eager mode (the reference's own harness runs batch 1,
    test.py:101-127); at the bench's batch 16 the GPU is busy either way.  Inputs are copied into static buffers (skipped when
    the caller passes the same tensors again); the returned tensors are the graph's static outputs and are OVERWRITTEN by
    the next call.  The diffusion noise must come from the device (default torch.randn, whose generator torch keeps
    graph-safe) or from a source that returns the same device tensors every call."""

    def __init__(self, engine, imgs, proj, dv, noise_fn, test, feats=None):
        self.s_imgs = [i.detach().clone() for i in imgs]
        self.s_proj = {k: v.detach().clone() for k, v in proj.items()}
        self.s_dv = dv.detach().clone()
        self.s_feats = None if feats is None else {k: v.detach().clone() for k, v in feats.items()}      # (scene mode: gathered rows of the store)
        side = torch.cuda.Stream(device=engine.ops.device)
        side.wait_stream(torch.cuda.current_stream(engine.ops.device))
        with torch.cuda.stream(side):                  # warm-up outside the capture: weight-side caches, allocator pools
            for _ in range(2):
                self._rewind(noise_fn)
                engine.forward(self.s_imgs, self.s_proj, self.s_dv, noise_fn=noise_fn, test=test, feats=self.s_feats)
        torch.cuda.current_stream(engine.ops.device).wait_stream(side)
        self._rewind(noise_fn)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.out = engine.forward(self.s_imgs, self.s_proj, self.s_dv, noise_fn=noise_fn, test=test, feats=self.s_feats)

    @staticmethod
    def _rewind(noise_fn):
        if hasattr(noise_fn, "rewind"):           # a source of fixed device tensors: every pass must see them in the same order
            noise_fn.rewind()

    @staticmethod
    def _refresh(dst, src):
        if src.data_ptr() != dst.data_ptr():
            dst.copy_(src, non_blocking=True)

    def __call__(self, imgs, proj, dv, feats=None):
        for d, s in zip(self.s_imgs, imgs):
            self._refresh(d, s)
        if self.s_feats is not None:
            for k, d in self.s_feats.items():
                self._refresh(d, feats[k])
        for k, d in self.s_proj.items():
            self._refresh(d, proj[k])
        self._refresh(self.s_dv, dv)
        self.graph.replay()
        return self.out


class Engine:
    def __init__(self, sd: Dict[str, torch.Tensor], args, ops: Ops):
        self.ops = self.base_ops = ops       # (self.ops may become a copy bound to another conv arithmetic, see conv_arith)
        self._graphs = {}
        self.args = args
        self.arena = GnArena(ops)
        self._ss_cache = {}
        dev = ops.device
        sd = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in sd.items()}
        self.cas = args.stage_iters[2] != 0
        self.up_ratio = 2 if self.cas else 4
        self.G = args.cost_dim_stage[0]
        self.G_cost = args.cost_dim_stage[1]
        # feature storage precision: args.precision / DMVS_PRECISION in {"fp32", "bf16", "fp16"} (BASELINE.json configs[2] /
        # [4]).  The image features FeatureNet hands to the warp kernels are stored in 16 bits (half the bytes of the path's
        # dominant gather traffic); projection, hypotheses, correlation, every convolution and all accumulators stay fp32
        prec = getattr(args, "precision", None) or os.environ.get("DMVS_PRECISION") or "fp32"      # an explicit args value wins
        if prec not in K.FEATURE_DTYPES:
            raise K._lib.DmvsError(f"precision '{prec}': expected one of {sorted(K.FEATURE_DTYPES)}")
        self.precision, self.feat_dtype = prec, K.FEATURE_DTYPES[prec]
        # matrix arithmetic of the 2-D convolutions: args.conv_arith / DMVS_CONV_ARITH in {"split", "fp32", "bf16"}.
        #   "split" (the default, round 6): fp32 ACCURACY on the bf16 matrix cores -- every fp32 operand of a multi-tap convolution is split into
        #       three bf16 values and a product is the sum of its six partial products down to 2^-18 (fp32 accumulation); against fp64 it is as
        #       close as the exact-fp32 kernels (tests/test_ops.py::test_conv2d_split_bf16_arithmetic, measured on the MI355X).  Honoured where it
        #       is faster (csrc/conv2d_tiled.h: conv_split_honoured); the other layers, the FeatureNet stem, the 1x1 layers, the 3-D convolutions,
        #       the warps and every epilogue compute in exact fp32.
        #   "fp32": exact fp32 products everywhere (v_mfma_f32_16x16x4_f32: bitwise a k-ordered fma chain).
        #   "bf16": inputs and weights of every multi-tap convolution with a planar output ROUNDED to bf16 as they enter the matrix cores (fp32
        #       accumulation) -- the arithmetic of BASELINE.json's bf16 configuration, a reduced-precision mode.
        # The reference's eps switch for non-fp32 activations (update.py:87,102) does not apply: activations are fp32 here.
        arith = getattr(args, "conv_arith", None) or os.environ.get("DMVS_CONV_ARITH") or "split"   # an explicit args value wins
        if arith not in K.CONV_ARITH:
            raise K._lib.DmvsError(f"conv_arith '{arith}': expected one of {sorted(K.CONV_ARITH)}")
        self.conv_arith = arith
        if K.CONV_ARITH[arith] != self.ops.conv_arith:
            self.ops = self.ops.with_conv_arith(K.CONV_ARITH[arith])
        self.feat = pack_feature(sd, "feature", g4=True, feat_dtype=self.feat_dtype)      # (the quad warp kernels' channel order)
        self.ctx = pack_context_trunk(sd, "context")
        # ContextNet output heads split into their hidden | context halves (diffusion.py:223-231): the
        # context half is written straight into the Unet input buffer, the hidden half feeds hidden_init
        self.ctx_out = {}
        for s in range(3):
            name = f"context.output{s + 1}"
            if name + ".weight" not in sd:
                continue
            w, b = sd[name + ".weight"], sd[name + ".bias"]
            hd = args.hidden_dim[s]
            hid = pack_conv2d(w[:hd].contiguous(), b[:hd].contiguous(), pad=1) if hd > 0 else None
            self.ctx_out[s] = (hid, pack_conv2d(w[hd:].contiguous(), b[hd:].contiguous(), pad=1))
        # ---- InitialCost (models/module.py:465-573)
        self.pvw = pack_pvw(sd, "depthnet.pixel_view_weight")
        self.reg = pack_costreg(sd, "depthnet.cost_regularization")
        self.mask = pack_mask(sd, "depthnet.mask")
        # ---- hidden_init (models/diffusion.py:53-58, :91-101)
        self.hidden_init = {1: [_cw(sd, "hidden_init.0.0", stride=2, pad=1), pack_conv2d(sd["hidden_init.0.1.weight"], pad=1)]}
        if self.cas:
            self.hidden_init[2] = [_cw(sd, "hidden_init.1.0", stride=2, pad=1), _cw(sd, "hidden_init.1.1", stride=2, pad=1),
                                   pack_conv2d(sd["hidden_init.1.2.weight"], pad=1)]
        # ---- update blocks
        self.ub = {1: _UpdateBlock(sd, "update_block_depth2", args, 1, self.up_ratio)}
        if self.cas:
            self.ub[2] = _UpdateBlock(sd, "update_block_depth3", args, 2, self.up_ratio)

    def _ss_of(self, ss, B):
        """time-conditioned scale/shift rows of one DDIM step, expanded to the batch once and cached"""
        def get(rb):
            if ss is None or rb["p"] not in ss:
                return None
            key = (id(ss), rb["p"], B)
            if key not in self._ss_cache:
                self._ss_cache[key] = ss[rb["p"]].expand(B, -1).contiguous()
            return self._ss_cache[key]
        return get

    # ------------------------------------------------------------------ stage 1
    def initial_cost(self, ref, src, rt, context, disp_min, disp_max, D):
        """InitialCost.forward eval branch (module.py:487-573) on NHWC features."""
        o = self.ops
        B, H, W, _ = ref.shape
        S = src.shape[0]
        cor = o.warp_corr_init_quad(ref, src, rt, disp_min, disp_max, D, self.G)        # [B,S,G,D,H,W]
        vw = run_pvw(o, self.pvw, cor.view(B * S, self.G, D, H, W)).view(B, S, H, W)
        agg = o.view_aggregate(cor, vw)
        logits = run_costreg(o, self.reg, agg)                                          # [B,1,D,H,W]
        nd, depth, conf = o.depth_regress(logits.view(B, D, H, W), disp_min, disp_max)
        mask = run_mask(o, self.mask, context)
        return mask, nd, depth, vw, conf

    # ------------------------------------------------------------------ stages 2, 3
    def update_block(self, ub: _UpdateBlock, feats_ref, feats_src, rt, inv_depth, hidden, context, view_w, vw_shift,
                     disp_min, disp_max, interval, noise_fn):
        """DiffusionUpdateBlockDepth.forward eval branch (update.py:466-521).
        context: [B,cd,H,W] = relu(context half of the ContextNet head); the encoder output lives in its own [B,cd,H,W] tensor
        (run_unet: the Unet's input concatenation is never materialised)."""
        o = self.ops
        a = self.args
        B, _, H, W = inv_depth.shape
        cd, n = ub.cd, ub.n
        noise = noise_fn((B, 1, H, W), o.device).float().contiguous()
        # (fused_up: only the head's 3x3 layer runs here; its 1x1 layer is evaluated inside the upsampling kernel at the end of the stage)
        mask = o.conv2d(ub.mask[0], context, act=K.ACT_RELU) if ub.fused_up else run_mask(o, ub.mask, context)
        ctx_part = o.conv2d(ub.init_ctx, context)             # the context half of the Unet's 7x7 init_conv, once per stage
        E = o.empty(B, cd, H, W)                              # encoder output (cd - 1 channels) + current inverse depth
        img, img_scale = noise, float(ub.scale)
        inv_list: List[torch.Tensor] = []
        conf_list: List[torch.Tensor] = []
        cur_hidden = hidden
        for time, time_next in ub.time_pairs:
            ss_of = self._ss_of(ub.ss_tables[time], B)
            inv_list, conf_list = [], []
            delta, new = o.delta_update(inv_depth, img, None, img_scale, new2=E, new2_cstride=cd, new2_coffset=cd - 1)
            img, img_scale = delta, 1.0
            cur_hidden, confidence = hidden, None
            for it in range(ub.iters):
                cost, samples = o.getcost_quad(feats_ref, feats_src, rt, new, confidence, view_w, disp_min, disp_max, n,
                                               interval, a.min_radius, a.max_radius, vw_shift, G=self.G_cost)
                run_encoder(o, ub.enc, cost, samples, out=E, out_cstride=cd, out_coffset=0)
                cur_hidden, upd, conf = run_unet(o, self.arena, ub, E, ctx_part, cur_hidden, ss_of)
                confidence = conf.view(B, H, W)
                delta, new = o.delta_update(inv_depth, delta, upd, 1.0, new2=E, new2_cstride=cd, new2_coffset=cd - 1)
                conf_list.append(confidence)
                inv_list.append(new)
            if time_next < 0:
                continue
            # multi-step DDIM update (update.py:504-519); not exercised by the shipped configs
            # (sampling_timesteps = 1), kept as plain device tensor arithmetic.
            pred_noise = (ub.sqrt_recip_acp[time] * img - delta) / ub.sqrt_recipm1_acp[time]
            alpha, alpha_next = ub.acp[time], ub.acp[time_next]
            sigma = ub.eta * ((1 - alpha / alpha_next) * (1 - alpha_next) / (1 - alpha)).sqrt()
            c = (1 - alpha_next - sigma ** 2).sqrt()
            fresh = (ub.scale * noise_fn((B, 1, H, W), o.device)).float()
            img = (delta * alpha_next.sqrt() + c * pred_noise + sigma * fresh).contiguous()
        return mask, cur_hidden, inv_list, conf_list

    # ------------------------------------------------------------------ whole forward
    @torch.no_grad()
    def forward_graphed(self, imgs, proj_matrices, depth_values, noise_fn: Optional[Callable] = None, test: bool = True, feats=None):
        """forward() through a captured HIP graph (one per input geometry); see GraphedForward for the contract"""
        dev = self.ops.device
        imgs = [i.to(dev).float() for i in imgs]
        proj = {k: v.to(dev).float().contiguous() for k, v in proj_matrices.items()}
        dv = depth_values.to(dev).float()
        nrows = None if feats is None else next(iter(feats.values())).shape[0]
        key = (len(imgs), tuple(imgs[0].shape), tuple(dv.shape), bool(test), id(noise_fn), nrows)
        g = self._graphs.get(key)
        if g is None:
            g = self._graphs[key] = GraphedForward(self, imgs, proj, dv, noise_fn, test, feats)
        return g(imgs, proj, dv, feats)

    @torch.no_grad()
    def forward(self, imgs, proj_matrices, depth_values, noise_fn: Optional[Callable] = None, test: bool = True, feats=None):
        """CasDiffMVS.forward in eval mode (models/diffusion.py:139-295).  test=True: the final iterate of each
        refinement stage and its confidence at full resolution (test.py); test=False: every iterate in "depth" and
        the Unet confidences in "conf" (diffusion.py:264-270, what train.py's validation loop feeds the loss).
        feats: {stage: [V*B,h,w,C]} from SceneFeatureStore.gather -- the image features are taken from the scene's store instead of
        running FeatureNet on `imgs` (of which only imgs[0], the reference views ContextNet reads, is then used)."""
        o, a = self.ops, self.args
        if noise_fn is None:
            noise_fn = lambda shape, device: torch.randn(shape, device=device)  # noqa: E731
        B = imgs[0].shape[0]
        V = len(imgs)
        Hi, Wi = int(imgs[0].shape[-2]), int(imgs[0].shape[-1])
        if Hi % 32 or Wi % 32 or Hi < 32 or Wi < 32:
            # FeatureNet halves the image three times and CostRegNet_small the stage-1 volume twice: the reference's own skip connections
            # (module.py:444-445, `conv3 + conv6(x)`) only line up -- and this engine's kernels only stay inside their tensors -- on multiples of
            # 32 (its datasets crop to that, datasets/mvs.py); found by running the host emulation under ASan on a 72 x 104 input, round 6
            raise K._lib.DmvsError(f"image size {Hi}x{Wi}: height and width must be multiples of 32")
        if feats is not None:      # rows gathered from a scene's store: validate before any launch reads them
            H, W = imgs[0].shape[-2:]
            V = next(iter(feats.values())).shape[0] // max(B, 1)
            for s in range(3):
                if a.stage_iters[s] == 0:
                    continue
                f = feats.get(f"stage{s + 1}")
                Cs = (48, 32, 16)[s]                      # FeatureNet's output widths (module.py:357-420)
                want = (V * B, H >> (3 - s), W >> (3 - s), Cs)
                if f is None or f.dim() != 4 or tuple(f.shape) != want or f.dtype != self.feat_dtype or f.device != o.device or V < 2:
                    raise K._lib.DmvsError(f"feats['stage{s + 1}']: expected a {self.feat_dtype} tensor [V*B={want[0]},{want[1]},{want[2]},{Cs}] on {o.device} "
                                           f"(SceneFeatureStore.gather of view ids [B,V], V >= 2), got "
                                           f"{None if f is None else (tuple(f.shape), f.dtype, str(f.device))}")
                # the warp kernels index the composed projections with S = V - 1 taken from the FEATURE rows: a camera tensor with fewer
                # views would be read out of bounds
                pm = proj_matrices.get(f"stage{s + 1}")
                if pm is None or pm.dim() != 5 or tuple(pm.shape[:2]) != (B, V):
                    raise K._lib.DmvsError(f"proj_matrices['stage{s + 1}']: expected [B={B},V={V},2,4,4] to match the gathered feature rows, got "
                                           f"{None if pm is None else tuple(pm.shape)}")
        self.arena.reset(B)
        dv = depth_values.to(o.device).float()
        depth_max_, depth_min_ = 1.0 / dv[:, 0], 1.0 / dv[:, -1]
        disp_min, disp_max = (1.0 / depth_max_).contiguous(), (1.0 / depth_min_).contiguous()   # module.py:222-223
        interval = 1.0 / depth_values.size(1)

        if feats is None:
            views = [im.to(o.device).float().contiguous() for im in imgs]       # V x [B,3,H,W]: FeatureNet's stem reads them in place
            feats = run_feature(o, self.feat, views, feat_dtype=self.feat_dtype)
        else:
            views = [imgs[0].to(o.device).float().contiguous()]
        trunk = run_context_trunk(o, self.ctx, views[0])
        depths, confs_full, confs_seq = [], [], []
        view_w = None
        for s in range(3):
            if a.stage_iters[s] == 0:
                continue
            name = f"stage{s + 1}"
            fs = feats[name]
            h, w, C = fs.shape[1], fs.shape[2], fs.shape[3]
            ref, src = fs[:B], fs[B:].view(V - 1, B, h, w, C)
            rt = o.compose_proj(proj_matrices[name].to(o.device).float().contiguous())
            hid_pc, ctx_pc = self.ctx_out[s]
            if s == 0:
                context = o.conv2d(ctx_pc, trunk[0], act=K.ACT_RELU)
                mask, nd, init_depth, view_w, conf = self.initial_cost(ref, src, rt, context, disp_min, disp_max,
                                                                       a.numdepth_initial)
                depths.append(init_depth)
                confs_full.append(o.upsample_nearest(conf.view(B, h, w), 8))
                _, depth_up = o.convex_upsample(nd, mask, disp_min, disp_max, 2, want_inv=False)
                depths.append(depth_up)
            else:
                ub = self.ub[s]
                cd = ub.cd
                inv_cur = o.depth_convert(depths[-1].view(B, 1, h, w), disp_min, disp_max, K._lib.EW_DEPTH_TO_DISP)
                hidden = o.conv2d(hid_pc, trunk[s])
                hi = self.hidden_init[s]
                for pc in hi[:-1]:
                    hidden = o.conv2d(pc, hidden, act=K.ACT_RELU)
                hidden = o.conv2d(hi[-1], hidden, act=K.ACT_TANH)
                context = o.conv2d(ctx_pc, trunk[s], act=K.ACT_RELU)
                mask, hidden, inv_seq, conf_seq = self.update_block(
                    ub, ref, src, rt, inv_cur, hidden, context, view_w, s, disp_min, disp_max,
                    interval * _RATIOS[s], noise_fn)
                if test:
                    depths.append(o.depth_convert(inv_seq[-1], disp_min, disp_max, K._lib.EW_DISP_TO_DEPTH).view(B, h, w))
                    confs_full.append(o.upsample_nearest(conf_seq[-1], 2 ** (3 - s)))
                else:
                    for inv_i in inv_seq:
                        depths.append(o.depth_convert(inv_i, disp_min, disp_max, K._lib.EW_DISP_TO_DEPTH).view(B, h, w))
                    confs_seq.extend(conf_seq)
                if ub.fused_up:
                    _, depth_up = o.mask_upsample4(ub.mask[1], mask, inv_seq[-1], disp_min, disp_max, post_scale=0.25)
                else:
                    _, depth_up = o.convex_upsample(inv_seq[-1], mask, disp_min, disp_max, self.up_ratio, want_inv=False)
                depths.append(depth_up)
        return {"depth": depths, "conf": confs_seq, "photometric_confidence": confs_full}
