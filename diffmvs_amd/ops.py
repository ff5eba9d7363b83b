"""Tensor-level wrappers around the C ABI (include/dmvs.h).

torch is used here for device memory and the stream handle only; every arithmetic
operation on the hot path is a kernel of libdmvs_hip.so.  `Ops` is bound to one library and
one device; the product constructs it with `Ops.for_device(cuda_device)` which loads the
gfx950 library and refuses anything else.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._lib import (ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_SILU, ACT_TANH, ARITH_BF16, ARITH_F32, ARITH_SPLIT, DTYPE_BF16, DTYPE_F16, DTYPE_F32, IN_PLAIN,  # noqa: F401
                   IN_UNSHUFFLE2, IN_UPSAMPLE2, IN_ZEROINSERT2, LAYOUT_NCHW, LAYOUT_NHWC, LAYOUT_NHWC_BF16, LAYOUT_NHWC_F16)

# matrix arithmetic of the multi-tap 2-D convolutions: "fp32" (exact, the reference's) | "bf16" (bf16 products, fp32 accumulation)
CONV_ARITH = {"fp32": ARITH_F32, "bf16": ARITH_BF16, "split": ARITH_SPLIT}
# reduced-precision FEATURE storage (BASELINE.json's bf16 / fp16 configurations): torch dtype <-> C-ABI codes
FEATURE_DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
_DTYPE_CODE = {torch.float32: DTYPE_F32, torch.bfloat16: DTYPE_BF16, torch.float16: DTYPE_F16}
_NHWC_LAYOUT = {torch.float32: LAYOUT_NHWC, torch.bfloat16: LAYOUT_NHWC_BF16, torch.float16: LAYOUT_NHWC_F16}


def _round_up(x: int, m: int) -> int:
    return (x + m - 1) // m * m


@dataclass
class PackedConv:
    """Weights in kernel layout [cin][k...][cout_pad] + folded per-channel epilogue."""
    weight: torch.Tensor
    scale: Optional[torch.Tensor]
    shift: Optional[torch.Tensor]
    cin: int
    cout: int
    cout_pad: int
    k: tuple
    stride: int = 1
    pad: tuple = (0, 0)
    transposed: bool = False
    wsplit: Optional[torch.Tensor] = None      # (conv2d, ARITH_SPLIT) the weights as bf16 triples in the matrix cores' operand order: split_weights()


def split_weights(pc: "PackedConv") -> torch.Tensor:
    """dmvs_conv2d_desc.weight_split (include/dmvs.h): [ceil(cin/8)][ceil(T/4)][3 planes hi, mid, lo][4][cout_pad][8] bf16, element
    (c, g, p, q, co, j) = part p of the weight of input channel 8c + j, tap 4g + q, output channel co; hi = bf16(w), mid = bf16(w - hi),
    lo = bf16(w - hi - mid), round to nearest even; zero beyond cin / the taps.  Built once per packed layer, cached on it."""
    if pc.wsplit is None:
        kh, kw = pc.k
        T, cp = kh * kw, pc.cout_pad
        NG, NC = (T + 3) // 4, (pc.cin + 7) // 8
        w = torch.zeros(NC * 8, NG * 4, cp, dtype=torch.float32, device=pc.weight.device)
        w[:pc.cin, :T] = pc.weight.reshape(pc.cin, T, cp)
        hi = w.to(torch.bfloat16)
        r1 = w - hi.float()
        mid = r1.to(torch.bfloat16)
        lo = (r1 - mid.float()).to(torch.bfloat16)
        planes = torch.stack([hi, mid, lo]).view(3, NC, 8, NG, 4, cp)          # [p, c, j, g, q, co]
        pc.wsplit = planes.permute(1, 3, 0, 4, 5, 2).contiguous()              # [c, g, p, q, co, j]
    return pc.wsplit


def _pad_cout(cout: int) -> int:
    return 8 if cout <= 8 else _round_up(cout, 16)


def fold_bn(bn: dict, eps: float = 1e-5):
    """eval BatchNorm -> (scale, shift).  reference models/module.py:46,90 (torch default eps)."""
    scale = bn["weight"] * torch.rsqrt(bn["running_var"] + eps)
    shift = bn["bias"] - bn["running_mean"] * scale
    return scale, shift


def pack_conv2d(w: torch.Tensor, bias=None, bn: Optional[dict] = None, stride=1, pad=(0, 0),
                standardize=False) -> PackedConv:
    """w: [cout, cin, kh, kw] (torch layout).  standardize: WeightStandardizedConv2d,
    reference models/update.py:86-94 (fp32 eps 1e-5) applied once at pack time."""
    w = w.detach().float()
    if standardize:
        mean = w.mean(dim=(1, 2, 3), keepdim=True)
        var = w.var(dim=(1, 2, 3), unbiased=False, keepdim=True)
        w = (w - mean) * torch.rsqrt(var + 1e-5)
    cout, cin, kh, kw = w.shape
    cp = _pad_cout(cout)
    if cp == cout:                  # the usual case: no padding columns, one permuting copy
        wk = w.permute(1, 2, 3, 0).contiguous()
    else:
        wk = torch.zeros(cin, kh, kw, cp, dtype=torch.float32, device=w.device)
        wk[..., :cout] = w.permute(1, 2, 3, 0)
    scale = shift = None
    if bn is not None:
        scale, shift = fold_bn(bn)
        if bias is not None:
            shift = shift + bias.detach().float() * scale
    elif bias is not None:
        shift = bias.detach().float()
    pad = (pad, pad) if isinstance(pad, int) else tuple(pad)
    return PackedConv(wk.contiguous(), None if scale is None else scale.contiguous().float(),
                      None if shift is None else shift.contiguous().float(), cin, cout, cp, (kh, kw), stride, pad)


def pack_conv3d(w: torch.Tensor, bias=None, bn: Optional[dict] = None, stride=1, transposed=False) -> PackedConv:
    """w: Conv3d [cout,cin,3,3,3] or ConvTranspose3d [cin,cout,3,3,3] (reference module.py:88,130)."""
    w = w.detach().float()
    if transposed:
        cin, cout = w.shape[0], w.shape[1]
        wk_src = w.permute(0, 2, 3, 4, 1)          # [cin,kd,kh,kw,cout]
    else:
        cout, cin = w.shape[0], w.shape[1]
        wk_src = w.permute(1, 2, 3, 4, 0)
    cp = _pad_cout(cout)
    if cp == cout:
        wk = wk_src.reshape(cin, 27, cout).contiguous()
    else:
        wk = torch.zeros(cin, 27, cp, dtype=torch.float32, device=w.device)
        wk[..., :cout] = wk_src.reshape(cin, 27, cout)
    scale = shift = None
    if bn is not None:
        scale, shift = fold_bn(bn)
    elif bias is not None:
        shift = bias.detach().float()
    return PackedConv(wk.contiguous(), None if scale is None else scale.contiguous(),
                      None if shift is None else shift.contiguous(), cin, cout, cp, (3, 3, 3), stride, (1, 1),
                      transposed)


def g4_channels(C: int, dtype=torch.float32) -> torch.Tensor:
    """Channel order of the GROUP-INTERLEAVED channel-last feature layout "NHWC-g4" the quad-per-pixel warp kernels read
    (include/dmvs.h): position p of a texel holds channel  c(p) = ((p // 4) % 4) * (C // 4) + (p // 16) * 4 + p % 4,
    i.e. x_g4 = x_nhwc[..., g4_channels(C)].  The engine folds this permutation into the weights of FeatureNet's output
    convolutions; tests and the module-level GetCost use it on plain tensors.  16-bit features are read in plain NHWC
    order (a group's channels already form one 8 / 16 / 24-byte run per lane): identity."""
    p = torch.arange(C)
    if dtype != torch.float32:
        return p
    return ((p // 4) % 4) * (C // 4) + (p // 16) * 4 + p % 4


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


MAX_WINDOW_VIEWS = 16      # include/dmvs.h: DMVS_GETCOST_MAX_WINDOW_VIEWS
RASTER_QUEUE_ENTRIES = 1 << 20      # mesh_raster_zid: the default queue of large (face, view) pairs holds at most this many (8 MiB)

# Kernels that write parameters / buffers through raw pointers (dmvs_adamw_step_f32, the running statistics of
# dmvs_batchnorm_train_fwd_f32) do not bump torch's per-tensor version counters, so every cache of packed weights
# (models.module.HipModule.packed, CasDiffMVS.engine) also keys on this process-wide generation.
_weights_generation = [0]


def weights_generation() -> int:
    return _weights_generation[0]


def bump_weights_generation() -> None:
    _weights_generation[0] += 1


BWD_INTERLEAVED_DEFAULT = 1      # round-6 A/B (profiles/r6_bwd_interleave_ab.json): getcost_bwd 33.3 -> 9.9 ms per cfg4 step, 31.3 -> 40.3 samples/s


def _env_tune():
    """A/B knobs of the kernels' `tune` arguments (include/dmvs.h), read ONCE per binding in the Python layer -- the C library
    itself reads no environment variable -- and Ops.for_device keeps ONE binding per (library, device) for the life of the process: changing
    a variable after the first forward has no effect (A/B tools pass tune= per call, mutate ops.tune, or construct a fresh Ops).
    All default to 0 = the library's measured-best path:
      DMVS_CONV_WX=1|2, DMVS_CONV_MT=1|2|4, DMVS_CONV_WALK=0, DMVS_CONV_LEAN=0, DMVS_CONV_V16=0, DMVS_CONV1X1_PX4=0, DMVS_CONV_TALL=0|1, DMVS_CONV_XCD=1..7   (dmvs_conv2d_desc.tune)
      DMVS_CONV3D_V16=0, DMVS_CONV3D_S2=direct, DMVS_CONV3D_PAIR=0, DMVS_CONV3D_XCD=1..4   (dmvs_conv3d_desc.tune)      DMVS_STEM_V16=0, DMVS_STEM_XCD=1..4, DMVS_STEM_EXACT=1      DMVS_PLANE_SWEEP=quad"""
    e = os.environ.get
    t2 = _lib.tune_tile_wx(int(e("DMVS_CONV_WX", "0"))) | _lib.tune_tile_mt(int(e("DMVS_CONV_MT", "0")))
    t2 |= _lib.TUNE_NO_WALK if e("DMVS_CONV_WALK") == "0" else 0
    t2 |= _lib.TUNE_PIECES4 if e("DMVS_CONV_V16") == "0" else 0
    t2 |= _lib.TUNE_NO_LEAN if e("DMVS_CONV_LEAN") == "0" else 0
    t2 |= _lib.TUNE_1X1_TILED if e("DMVS_CONV1X1_PX4") == "0" else 0
    t2 |= {"0": _lib.TUNE_NO_TALL, "1": _lib.TUNE_TALL}.get(e("DMVS_CONV_TALL"), 0)
    t2 |= _lib.TUNE_SPLIT_ALL if e("DMVS_CONV_SPLIT_ALL") == "1" else 0
    t2 |= _lib.tune_xcd_group(int(e("DMVS_CONV_XCD", "0")))      # round 6: which tiles share an XCD's L2 (include/dmvs.h DMVS_TUNE_XCD_GROUP)
    t3 = (_lib.TUNE3D_PIECES4 if e("DMVS_CONV3D_V16") == "0" else 0) | (_lib.TUNE3D_S2_DIRECT if e("DMVS_CONV3D_S2") == "direct" else 0)
    t3 |= _lib.TUNE3D_NO_PAIR if e("DMVS_CONV3D_PAIR") == "0" else 0
    t3 |= _lib.tune3d_xcd_group(int(e("DMVS_CONV3D_XCD", "0")))
    return {"conv2d": t2, "conv3d": t3, "stem": (_lib.TUNE_PIECES4 if e("DMVS_STEM_V16") == "0" else 0) | _lib.tune_xcd_group(int(e("DMVS_STEM_XCD", "0"))) | (_lib.TUNE_STEM_EXACT if e("DMVS_STEM_EXACT") == "1" else 0),
            "sweep": _lib.TUNE_SWEEP_GLOBAL if e("DMVS_PLANE_SWEEP") == "quad" else 0,
            # training: GetCost backward through the per-pixel gather kernel only (no tile pre-pass / LDS-window worklist): DMVS_GETCOST_BWD=gather
            "bwd_gather": e("DMVS_GETCOST_BWD") == "gather",
            # training: channel -> lane mapping of the per-pixel scatter kernels (include/dmvs.h DMVS_TUNE_BWD_INTERLEAVED): DMVS_BWD_INTERLEAVED=0|1
            "bwd_il": e("DMVS_BWD_INTERLEAVED", "%d" % BWD_INTERLEAVED_DEFAULT) == "1"}


class Ops:
    _bindings = {}      # (library path, device) -> the one Ops of the process for it (for_device)

    def __init__(self, lib: _lib.Lib, device):
        self.lib = lib
        self.device = torch.device(device)
        self.tune = _env_tune()
        # optional per-entry-point HIP-event timing on the launch stream (bench.py roofline leg):
        # {"dmvs_getcost_f32": [(start_event, end_event), ...]}
        self.timers = None
        self.conv_arith = ARITH_F32      # matrix arithmetic of the multi-tap 2-D convolutions (with_conv_arith)
        # debugging aid (tools/determinism.py, tests): a float every freshly allocated kernel output is filled with before the launch, so
        # that a kernel that leaves part of its output unwritten -- or reads scratch it never wrote -- shows up as NaN instead of whatever the
        # allocator handed back.  None (the product default): plain torch.empty
        self.debug_fill = None
        # measurement hook (bench.py's untimed probe legs): called as hook(descriptor, tensors) right BEFORE every GetCost launch, on the
        # launch stream.  None in the product.
        self.getcost_hook = None

    def with_conv_arith(self, arith: int) -> "Ops":
        """a binding of the same library whose conv2d() computes in `arith` (ARITH_F32 | ARITH_BF16) by default"""
        import copy
        o = copy.copy(self)
        o.conv_arith = arith
        return o

    def _call(self, name, *args):
        if self.timers is not None and name in self.timers:
            st, en = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            st.record()
            self.lib.call(name, *args)
            en.record()
            self.timers[name].append((st, en))
        else:
            self.lib.call(name, *args)

    @classmethod
    def for_device(cls, device) -> "Ops":
        device = torch.device(device)
        if device.type != "cuda":
            raise _lib.DmvsError(
                f"diffmvs_amd runs on MI355X only (got device '{device}'); there is no CPU path. "
                "Move the model and inputs to a HIP device.")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        lib = _lib.hip_lib()
        # ONE binding per (library, device): the engine, the training forward and the Trainer then share its per-binding state
        # (timers, conv_arith, the GetCost path probe) instead of each building a throw-away Ops per call
        key = (lib.path, device.index)
        o = cls._bindings.get(key)
        if o is None:
            o = cls._bindings[key] = cls(lib, device)
        return o

    # ------------------------------------------------------------------ plumbing
    def stream(self):
        if self.device.type == "cuda":
            return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        return None

    def empty(self, *shape, dtype=torch.float32):
        t = torch.empty(*shape, dtype=dtype, device=self.device)
        if self.debug_fill is not None and t.is_floating_point():      # tools/determinism.py: every kernel output starts as NaN / garbage
            t.fill_(self.debug_fill)
        return t

    def empty_like(self, x):
        t = torch.empty_like(x)
        if self.debug_fill is not None and t.is_floating_point():
            t.fill_(self.debug_fill)
        return t

    def _chk_feat(self, *ts):
        dt = ts[0].dtype
        for t in ts:
            if t.dtype not in _DTYPE_CODE or t.dtype != dt or not t.is_contiguous() or t.device != self.device:
                raise _lib.DmvsError(f"expected contiguous fp32 / bf16 / fp16 feature tensors of one dtype on {self.device}, got "
                                     f"{t.dtype} contiguous={t.is_contiguous()} on {t.device}")
        return _DTYPE_CODE[dt]

    def _chk(self, *ts):
        for t in ts:
            if t is None:
                continue
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device:
                raise _lib.DmvsError(f"expected contiguous fp32 tensor on {self.device}, got {t.dtype} "
                                     f"contiguous={t.is_contiguous()} on {t.device}")

    def _chk_typed(self, what, *pairs):
        for t, dt in pairs:
            if t is not None and (t.dtype != dt or not t.is_contiguous() or t.device != self.device):
                raise _lib.DmvsError(f"{what}: expected a contiguous {dt} tensor on {self.device}, got {t.dtype} on {t.device}")

    # ------------------------------------------------------------------ conv2d
    def conv2d(self, pc: PackedConv, x0, x1=None, *, mul0=None, in_mode=IN_PLAIN, act=ACT_NONE, residual=None,
               res_mode=IN_PLAIN, res_after_act=False, post_scale=1.0, gru_z=None, gru_h=None, out=None,
               out_layout=LAYOUT_NCHW, out_cstride=None, out_coffset=0, gn_stats=None, gn_groups=4, out_dtype=torch.float32,
               gate_cstride=0, arith=None, tune=None, out_mul=None, out_mul_c0=0, in0_cstride=0):
        """gn_stats: zeroed float64 [B*gn_groups*2] tensor that receives the GroupNorm statistics of
        the (pre-activation) output, for a following groupnorm_apply().  out_dtype (channel-last outputs only): bf16 / fp16
        feature storage, rounded to nearest even in the epilogue.  arith: ARITH_F32 | ARITH_BF16 (default: this binding's
        conv_arith) -- bf16 rounds inputs and weights as they enter the matrix cores (fp32 accumulation, fp32 tensors); layers
        with one tap and channel-last outputs always compute in fp32."""
        if in0_cstride:       # x0 is a channel slice of a contiguous [B,in0_cstride,H,W] tensor (the r * h half of the merged gate conv's output)
            if (x0.dtype != torch.float32 or x0.device != self.device or x0.stride(1) != x0.shape[2] * x0.shape[3] or
                    x0.stride(0) != in0_cstride * x0.shape[2] * x0.shape[3] or x0.stride(3) != 1 or in_mode != IN_PLAIN):
                raise _lib.DmvsError("in0_cstride: x0 must be a channel slice of a contiguous [B,in0_cstride,H,W] tensor, plain input mode")
        self._chk(out_mul)
        if gate_cstride:      # mul0 / gru_z are channel slices of one [B,gate_cstride,H,W] tensor (merged z|r gate convolution)
            self._chk(*(() if in0_cstride else (x0,)), x1, residual, gru_h)
            for t in (mul0, gru_z):
                if t is not None and (t.dtype != torch.float32 or t.device != self.device or t.stride(1) != t.shape[2] * t.shape[3] or
                                      t.stride(0) != gate_cstride * t.shape[2] * t.shape[3] or t.stride(3) != 1):
                    raise _lib.DmvsError("gate_cstride: mul0 / gru_z must be channel slices of a contiguous [B,gate_cstride,H,W] tensor")
        else:
            self._chk(*(() if in0_cstride else (x0,)), x1, mul0, residual, gru_z, gru_h)
        if out_dtype != torch.float32:
            if out_layout != LAYOUT_NHWC or out is not None:
                raise _lib.DmvsError("16-bit outputs are channel-last feature tensors allocated by conv2d")
            out_layout = _NHWC_LAYOUT[out_dtype]
        else:
            self._chk(out)
        if gn_stats is not None and (gn_stats.dtype != torch.float64 or gn_stats.numel() < x0.shape[0] * gn_groups * 2):
            raise _lib.DmvsError("gn_stats must be float64 with B*groups*2 elements")
        B = x0.shape[0]
        if in_mode == IN_PLAIN:
            c0, Hin, Win = x0.shape[1], x0.shape[2], x0.shape[3]
        elif in_mode in (IN_UPSAMPLE2, IN_ZEROINSERT2):
            c0, Hin, Win = x0.shape[1], x0.shape[2] * 2, x0.shape[3] * 2
        else:
            c0, Hin, Win = x0.shape[1] * 4, x0.shape[2] // 2, x0.shape[3] // 2
        c1 = 0 if x1 is None else x1.shape[1]
        assert c0 + c1 == pc.cin, (c0, c1, pc.cin)
        kh, kw = pc.k
        Hout = (Hin + 2 * pc.pad[0] - kh) // pc.stride + 1
        Wout = (Win + 2 * pc.pad[1] - kw) // pc.stride + 1
        if out_cstride is None:
            out_cstride = pc.cout
        if out is None:
            shape = (B, out_cstride, Hout, Wout) if out_layout == LAYOUT_NCHW else (B, Hout, Wout, out_cstride)
            out = self.empty(*shape, dtype=out_dtype)
        arith = self.conv_arith if arith is None else arith
        wsplit = split_weights(pc) if (arith == ARITH_SPLIT and kh * kw > 1 and out_layout in (LAYOUT_NCHW, LAYOUT_NHWC)) else None
        d = _lib.Conv2dDesc(
            weight_split=_ptr(wsplit),
            in0=_ptr(x0), in1=_ptr(x1), mul0=_ptr(mul0), weight=_ptr(pc.weight), scale=_ptr(pc.scale),
            shift=_ptr(pc.shift), residual=_ptr(residual), gru_z=_ptr(gru_z), gru_h=_ptr(gru_h), out=_ptr(out),
            gn_stats=_ptr(gn_stats), gn_groups=(gn_groups if gn_stats is not None else 0), B=B, c0=c0, c1=c1, Hin=Hin, Win=Win, Hout=Hout, Wout=Wout, cout=pc.cout, cout_pad=pc.cout_pad,
            kh=kh, kw=kw, stride=pc.stride, pad_h=pc.pad[0], pad_w=pc.pad[1], in_mode=in_mode, act=act,
            res_mode=res_mode, res_after_act=int(res_after_act), out_layout=out_layout, out_cstride=out_cstride,
            out_coffset=out_coffset, post_scale=post_scale, gate_cstride=gate_cstride,
            arith=arith, tune=(self.tune["conv2d"] if tune is None else tune),
            out_mul=_ptr(out_mul), out_mul_c0=out_mul_c0, in0_cstride=in0_cstride)
        self._call("dmvs_conv2d_f32", C.byref(d), self.stream())
        if self.timers is not None and "dmvs_conv2d_f32" in self.timers:      # bench: MFMA roofline over every conv launch
            self.timers.setdefault("_conv2d_flops", []).append(2.0 * B * Hout * Wout * pc.cout * pc.cin * kh * kw)
            self.timers.setdefault("_conv2d_shape", []).append((B, pc.cin, pc.cout, kh, kw, pc.stride, Hout, Wout, in_mode, int(mul0 is not None)))
            # algorithmic bytes: every operand tensor read once, the output written once (SURVEY 8d's convention)
            nb = sum(t.numel() * t.element_size() for t in (x0, x1, mul0, residual, gru_z, gru_h, out_mul) if t is not None)
            self.timers.setdefault("_conv2d_bytes", []).append(nb + B * Hout * Wout * pc.cout * out.element_size())
        return out

    def featurenet_stem(self, pc0: PackedConv, pc1: PackedConv, x, tune=None):
        """relu(bn(conv0.1(relu(bn(conv0.0(x)))))) of FeatureNet in one kernel: x [N,3,H,W] -> [N,8,H,W].
        x may be a LIST of V tensors [B,3,H,W] (the views of a batch): one launch per view into consecutive slices of one
        [V*B,8,H,W] output -- the view stack is never concatenated"""
        if isinstance(x, (list, tuple)):
            self._chk(*x)
            Bv, cin, H, W = x[0].shape
            y = self.empty(len(x) * Bv, 8, H, W)
            for v, xv in enumerate(x):
                self._stem_launch(pc0, pc1, xv, y[v * Bv:(v + 1) * Bv], tune)
            return y
        self._chk(x)
        N, cin, H, W = x.shape
        y = self.empty(N, 8, H, W)
        self._stem_launch(pc0, pc1, x, y, tune)
        return y

    def _stem_launch(self, pc0: PackedConv, pc1: PackedConv, x, y, tune=None):
        N, cin, H, W = x.shape
        if not (cin == 3 and pc0.cin == 3 and pc0.cout == 8 and pc1.cin == 8 and pc1.cout == 8 and pc0.k == (3, 3) and
                pc1.k == (3, 3) and pc0.stride == 1 and pc1.stride == 1 and pc0.pad == (1, 1) and pc1.pad == (1, 1) and
                pc0.cout_pad == 8 and pc1.cout_pad == 8):
            raise _lib.DmvsError("featurenet_stem: expects the 3->8->8 3x3 stem of FeatureNet")
        tune = self.tune["stem"] if tune is None else tune
        if self.conv_arith != ARITH_SPLIT:      # conv0.1 in split-bf16 arithmetic (the library's default) only under conv_arith = "split"
            tune |= _lib.TUNE_STEM_EXACT
        self._call("dmvs_featurenet_stem_f32", _ptr(x), _ptr(pc0.weight), _ptr(pc0.scale), _ptr(pc0.shift), _ptr(pc1.weight),
                   _ptr(pc1.scale), _ptr(pc1.shift), _ptr(y), N, H, W, tune, self.stream())

    @staticmethod
    def featurenet_stem3_supported(x):
        """geometry of dmvs_featurenet_stem3_f32: even H, rows of whole 16-byte pieces on 16-byte aligned tensors"""
        xs = x if isinstance(x, (list, tuple)) else [x]
        H, W = xs[0].shape[2], xs[0].shape[3]
        return H % 2 == 0 and W % 4 == 0 and 3 * H * W < 2 ** 31 and all(t.data_ptr() % 16 == 0 for t in xs)

    def featurenet_stem3(self, pc0: PackedConv, pc1: PackedConv, pc2: PackedConv, x, tune=None):
        """relu(bn(conv1.0(relu(bn(conv0.1(relu(bn(conv0.0(x))))))))) of FeatureNet in one kernel: x [N,3,H,W] -> [N,16,H/2,W/2]; conv0.1 and
        conv1.0 in split-bf16 arithmetic.  x may be a LIST of V tensors [B,3,H,W] like featurenet_stem's: one launch per view into consecutive
        slices of one [V*B,16,H/2,W/2] output"""
        xs = x if isinstance(x, (list, tuple)) else [x]
        self._chk(*xs)
        Bv, cin, H, W = xs[0].shape
        if not (cin == 3 and pc0.cin == 3 and pc0.cout == 8 and pc1.cin == 8 and pc1.cout == 8 and pc0.k == (3, 3) and
                pc1.k == (3, 3) and pc0.stride == 1 and pc1.stride == 1 and pc0.pad == (1, 1) and pc1.pad == (1, 1) and
                pc0.cout_pad == 8 and pc1.cout_pad == 8 and pc2.cin == 8 and pc2.cout == 16 and pc2.cout_pad == 16 and pc2.k == (5, 5) and
                pc2.stride == 2 and pc2.pad == (2, 2)):
            raise _lib.DmvsError("featurenet_stem3: expects the 3->8->8 3x3 stem of FeatureNet and its 8->16 5x5 stride-2 conv1.0")
        if not self.featurenet_stem3_supported(xs) or any(t.shape != xs[0].shape for t in xs):
            raise _lib.DmvsError(f"featurenet_stem3: needs even H, W % 4 == 0 and 16-byte aligned views of one shape, got {tuple(xs[0].shape)}")
        y = self.empty(len(xs) * Bv, 16, H // 2, W // 2)
        for v, xv in enumerate(xs):
            self._call("dmvs_featurenet_stem3_f32", _ptr(xv), _ptr(pc0.weight), _ptr(pc0.scale), _ptr(pc0.shift), _ptr(pc1.weight),
                       _ptr(pc1.scale), _ptr(pc1.shift), _ptr(pc2.weight), _ptr(pc2.scale), _ptr(pc2.shift), _ptr(y[v * Bv:(v + 1) * Bv]),
                       Bv, H, W, 0 if tune is None else tune, self.stream())
        return y

    CONV1_PAIR_STRIP, CONV1_PAIR_SEGMENT = 80, 64      # csrc/conv1_pair.hip: a work unit's output columns / rows (US, UR)

    @staticmethod
    def conv1_pair_supported(x):
        """geometry of dmvs_featurenet_conv1_pair_f32: 16 channels, rows of whole 16-byte pieces on a 16-byte aligned tensor"""
        return (x.dim() == 4 and x.shape[1] == 16 and x.shape[3] % 4 == 0 and 16 * x.shape[2] * x.shape[3] < 2 ** 31 and
                x.data_ptr() % 16 == 0)

    def conv1_pair(self, pc1: PackedConv, pc2: PackedConv, x, tune=0):
        """relu(bn(conv1.2(relu(bn(conv1.1(x)))))) of FeatureNet in one kernel: x [N,16,H,W] -> [N,16,H,W], both layers in split-bf16
        arithmetic: the bits of conv2d(pc2, conv2d(pc1, x, act=ACT_RELU), act=ACT_RELU) under ARITH_SPLIT.  tune: 1 .. 65535 forces the grid."""
        self._chk(x)
        for pc in (pc1, pc2):
            if not (pc.cin == 16 and pc.cout == 16 and pc.cout_pad == 16 and pc.k == (3, 3) and pc.stride == 1 and pc.pad == (1, 1)):
                raise _lib.DmvsError("conv1_pair: expects the two 16->16 3x3 stride-1 layers of FeatureNet's conv1")
        if not self.conv1_pair_supported(x):
            raise _lib.DmvsError(f"conv1_pair: needs 16 channels, W % 4 == 0 and a 16-byte aligned tensor, got {tuple(x.shape)}")
        N, _, H, W = x.shape
        y = self.empty(N, 16, H, W)
        self._call("dmvs_featurenet_conv1_pair_f32", _ptr(x), _ptr(split_weights(pc1)), _ptr(pc1.scale), _ptr(pc1.shift),
                   _ptr(split_weights(pc2)), _ptr(pc2.scale), _ptr(pc2.shift), _ptr(y), N, H, W, tune, self.stream())
        return y

    FPN_TAIL_STRIP, FPN_TAIL_SEGMENT = 32, 64      # csrc/fpn_tail.hip: a work unit's output columns / rows (US, UR)

    @staticmethod
    def fpn_tail_supported(c2, c3):
        """geometry of dmvs_featurenet_fpn_tail_f32: 32 and 64 channels, c3 at half the resolution, even H, c3 rows of whole 16-byte pieces
        (W % 8 == 0) on 16-byte aligned contiguous fp32 tensors, 32-bit offsets inside an image"""
        if not (c2.dim() == 4 and c3.dim() == 4 and c2.dtype == torch.float32 and c3.dtype == torch.float32):
            return False
        N, C, H, W = c2.shape
        return (C == 32 and H % 2 == 0 and W % 8 == 0 and H > 0 and W > 0 and tuple(c3.shape) == (N, 64, H // 2, W // 2) and
                64 * H * W < 2 ** 31 and c2.is_contiguous() and c3.is_contiguous() and c2.data_ptr() % 16 == 0 and c3.data_ptr() % 16 == 0)

    def fpn_tail(self, pc_inner: PackedConv, pc_out: PackedConv, c2, c3, tune=0):
        """out2(inner1(c2) + nearest_up2(c3)) of FeatureNet in one kernel: c2 [N,32,H,W], c3 [N,64,H/2,W/2] -> [N,H,W,32] channel-last fp32, the
        1x1 in exact fp32 and the 3x3 in split-bf16 arithmetic: the bits of conv2d(pc_out, conv2d(pc_inner, c2, residual=c3,
        res_mode=IN_UPSAMPLE2), out_layout=LAYOUT_NHWC) under ARITH_SPLIT.  tune: 1 .. 65535 forces the grid."""
        self._chk(c2, c3)
        if not (pc_inner.cin == 32 and pc_inner.cout == 64 and pc_inner.cout_pad == 64 and pc_inner.k == (1, 1) and pc_inner.stride == 1 and
                pc_inner.pad == (0, 0) and pc_inner.scale is None and pc_out.cin == 64 and pc_out.cout == 32 and pc_out.cout_pad == 32 and
                pc_out.k == (3, 3) and pc_out.stride == 1 and pc_out.pad == (1, 1) and pc_out.scale is None and pc_out.shift is None):
            raise _lib.DmvsError("fpn_tail: expects FeatureNet's inner1 (32->64 1x1, bias) and out2 (64->32 3x3, no bias)")
        if not self.fpn_tail_supported(c2, c3):
            raise _lib.DmvsError(f"fpn_tail: needs c2 [N,32,H,W] and c3 [N,64,H/2,W/2] with even H, W % 8 == 0, contiguous and 16-byte aligned, "
                                 f"got {tuple(c2.shape)} and {tuple(c3.shape)}")
        N, _, H, W = c2.shape
        y = self.empty(N, H, W, 32)
        self._call("dmvs_featurenet_fpn_tail_f32", _ptr(c2), _ptr(c3), _ptr(pc_inner.weight), _ptr(pc_inner.shift), _ptr(split_weights(pc_out)),
                   _ptr(y), N, H, W, tune, self.stream())
        return y

    def conv2d_wgrad(self, pc: PackedConv, x0, grad_out, x1=None, *, mul0=None, in_mode=IN_PLAIN, want_bias=False, tune=None,
                     into_gw=None, into_gb=None):
        """Weight gradient of conv2d(pc, x0, x1, mul0=..., in_mode=...) in torch layout [cout, cin, kh, kw]
        (and the bias gradient [cout] when want_bias) -> gw | (gw, gb).  into_gw (/ into_gb): ADD the gradient to these running
        gradients (contiguous fp32 tensors of the right shapes, e.g. views of the trainer's flat bucket) instead of returning new tensors."""
        self._chk(x0, x1, mul0, grad_out, into_gw, into_gb)
        B = x0.shape[0]
        if in_mode == IN_PLAIN:
            c0, Hin, Win = x0.shape[1], x0.shape[2], x0.shape[3]
        elif in_mode in (IN_UPSAMPLE2, IN_ZEROINSERT2):
            c0, Hin, Win = x0.shape[1], x0.shape[2] * 2, x0.shape[3] * 2
        else:
            c0, Hin, Win = x0.shape[1] * 4, x0.shape[2] // 2, x0.shape[3] // 2
        c1 = 0 if x1 is None else x1.shape[1]
        kh, kw = pc.k
        Hout, Wout = grad_out.shape[2], grad_out.shape[3]
        acc = into_gw is not None
        if acc and (tuple(into_gw.shape) != (pc.cout, pc.cin, kh, kw) or (want_bias and (into_gb is None or tuple(into_gb.shape) != (pc.cout,)))):
            raise _lib.DmvsError("conv2d_wgrad: into_gw / into_gb do not have the gradient's shape")
        gw = into_gw if acc else self.empty(pc.cout, pc.cin, kh, kw)
        gb = (into_gb if acc else self.empty(pc.cout)) if want_bias else None
        d = _lib.Conv2dDesc(
            in0=_ptr(x0), in1=_ptr(x1), mul0=_ptr(mul0), weight=None, scale=None, shift=None, residual=None, gru_z=None,
            gru_h=None, out=None, gn_stats=None, gn_groups=0, B=B, c0=c0, c1=c1, Hin=Hin, Win=Win, Hout=Hout, Wout=Wout,
            cout=pc.cout, cout_pad=pc.cout_pad, kh=kh, kw=kw, stride=pc.stride, pad_h=pc.pad[0], pad_w=pc.pad[1],
            in_mode=in_mode, act=ACT_NONE, res_mode=IN_PLAIN, res_after_act=0, out_layout=LAYOUT_NCHW,
            out_cstride=pc.cout, out_coffset=0, post_scale=1.0, gate_cstride=0, arith=ARITH_F32,
            tune=((self.tune["conv2d"] & _lib.TUNE_PIECES4) if tune is None else tune) | (_lib.TUNE_WGRAD_ACCUMULATE if acc else 0))
        nbytes = C.c_int64(0)
        self._call("dmvs_conv2d_wgrad_workspace_f32", C.byref(d), C.byref(nbytes))
        ws = self.empty(nbytes.value // 4)
        self._call("dmvs_conv2d_wgrad_f32", C.byref(d), _ptr(grad_out), _ptr(gw), _ptr(gb), _ptr(ws), nbytes.value, self.stream())
        if self.timers is not None and "dmvs_conv2d_wgrad_f32" in self.timers:      # bench cfg4: MFMA roofline over every weight-gradient launch
            self.timers.setdefault("_wgrad_flops", []).append(2.0 * B * Hout * Wout * pc.cout * pc.cin * kh * kw)
        return (gw, gb) if want_bias else gw

    # ------------------------------------------------------------------ conv3d
    def conv3d(self, pc: PackedConv, x, *, act=ACT_NONE, residual=None, out=None, tune=None):
        self._chk(x, residual, out)
        B, cin, Din, Hin, Win = x.shape
        assert cin == pc.cin
        if pc.transposed:
            Dout, Hout, Wout = 2 * Din, 2 * Hin, 2 * Win
        else:
            s = pc.stride
            Dout, Hout, Wout = (Din - 1) // s + 1, (Hin - 1) // s + 1, (Win - 1) // s + 1
        if out is None:
            out = self.empty(B, pc.cout, Dout, Hout, Wout)
        d = _lib.Conv3dDesc(in_=_ptr(x), weight=_ptr(pc.weight), scale=_ptr(pc.scale), shift=_ptr(pc.shift),
                            residual=_ptr(residual), out=_ptr(out), B=B, cin=cin, cout=pc.cout, cout_pad=pc.cout_pad,
                            Din=Din, Hin=Hin, Win=Win, Dout=Dout, Hout=Hout, Wout=Wout, stride=pc.stride,
                            transposed=int(pc.transposed), act=act, tune=(self.tune["conv3d"] if tune is None else tune))
        self._call("dmvs_conv3d_f32", C.byref(d), self.stream())
        return out

    def conv3d_wgrad(self, x, grad_out, cout, stride, want_bias=False):
        """gw of a (non-transposed) 3x3x3 conv: x [B,cin,D,H,W], grad_out [B,cout,Do,Ho,Wo] -> [cout,cin,3,3,3] (, gb [cout])"""
        self._chk(x, grad_out)
        B, cin, Din, Hin, Win = x.shape
        Dout, Hout, Wout = grad_out.shape[2:]
        gw = self.empty(cout, cin, 3, 3, 3)
        gb = self.empty(cout) if want_bias else None
        d = _lib.Conv3dDesc(in_=_ptr(x), weight=None, scale=None, shift=None, residual=None, out=None, B=B, cin=cin,
                            cout=cout, cout_pad=_pad_cout(cout), Din=Din, Hin=Hin, Win=Win, Dout=Dout, Hout=Hout, Wout=Wout,
                            stride=stride, transposed=0, act=ACT_NONE)
        nbytes = C.c_int64(0)
        self._call("dmvs_conv3d_wgrad_workspace_f32", C.byref(d), C.byref(nbytes))
        ws = self.empty(nbytes.value // 4)
        self._call("dmvs_conv3d_wgrad_f32", C.byref(d), _ptr(grad_out), _ptr(gw), _ptr(gb), _ptr(ws), nbytes.value, self.stream())
        return (gw, gb) if want_bias else gw

    # ------------------------------------------------------------------ geometry / cost volumes
    def compose_proj(self, proj):
        """proj [B,V,2,4,4] -> [B,S,12] (rot row-major, trans)."""
        self._chk(proj)
        B, V = proj.shape[0], proj.shape[1]
        out = self.empty(B, V - 1, 12)
        self._call("dmvs_compose_proj_f32", _ptr(proj), _ptr(out), B, V, self.stream())
        return out

    def warp_corr_init_quad(self, ref, src, rt, disp_min, disp_max, D, G=4, tune=None, plain=False):
        """quad-per-pixel plane sweep: ref [B,H,W,C], src [S,B,Hs,Ws,C] in the NHWC-g4 channel order (fp32) or plain NHWC
        (bf16 / fp16 feature storage; fp32 with plain=True: the training graph's features) -> [B,S,G,D,H,W] fp32"""
        self._chk(rt, disp_min, disp_max)
        fdt = self._chk_feat(ref, src)
        if plain and fdt == DTYPE_F32:
            fdt = _lib.DTYPE_F32_PLAIN
        B, H, W, Cc = ref.shape
        S, _, Hs, Ws, _ = src.shape
        out = self.empty(B, S, G, D, H, W)
        self._call("dmvs_warp_corr_init_quad_f32", _ptr(ref), _ptr(src), _ptr(rt), _ptr(disp_min), _ptr(disp_max), _ptr(out),
                   B, S, Cc, G, D, H, W, Hs, Ws, fdt, self.tune["sweep"] if tune is None else tune, self.stream())
        if self.timers is not None and "dmvs_warp_corr_init_quad_f32" in self.timers:
            self.timers.setdefault("_warp_init_bytes", []).append(B * H * W * (ref.element_size() * (Cc + S * Cc) + 4 * S * G * D))
        return out

    def getcost_quad(self, ref, src, rt, inv_depth, confidence, view_w, disp_min, disp_max, n, interval, min_radius,
                     max_radius, vw_shift, out_cost=None, cost_cstride=None, cost_coffset=0, out_samples=None,
                     samp_cstride=None, samp_coffset=0, G=4, plain=False):
        """quad-per-pixel GetCost, one launch for any geometry; ref / src in the NHWC-g4 channel order (fp32) or plain NHWC
        (bf16 / fp16 feature storage; fp32 with plain=True: the training graph's features)"""
        self._chk(rt, inv_depth, confidence, view_w, disp_min, disp_max, out_cost, out_samples)
        fdt = self._chk_feat(ref, src)
        if plain and fdt == DTYPE_F32:
            fdt = _lib.DTYPE_F32_PLAIN
        B, H, W, Cc = ref.shape
        S = src.shape[0]
        if out_cost is None:
            cost_cstride = G * n
            out_cost = self.empty(B, G * n, H, W)
        if out_samples is None:
            samp_cstride = n
            out_samples = self.empty(B, n, H, W)
        d = _lib.GetCostDesc(ref=_ptr(ref), src=_ptr(src), rt=_ptr(rt), inv_depth=_ptr(inv_depth),
                             confidence=_ptr(confidence), view_w=_ptr(view_w), disp_min=_ptr(disp_min),
                             disp_max=_ptr(disp_max), out_cost=_ptr(out_cost), out_samples=_ptr(out_samples),
                             worklist=None, B=B, S=S, C=Cc, G=G, n=n, H=H, W=W, vw_shift=vw_shift, cost_cstride=cost_cstride,
                             cost_coffset=cost_coffset, samp_cstride=samp_cstride, samp_coffset=samp_coffset,
                             interval=interval, min_radius=min_radius, max_radius=max_radius, feat_dtype=fdt)
        if self.getcost_hook is not None:
            self.getcost_hook(d, {"ref": ref, "src": src, "rt": rt, "inv_depth": inv_depth, "confidence": confidence, "view_w": view_w,
                                  "disp_min": disp_min, "disp_max": disp_max, "out_cost": out_cost, "out_samples": out_samples})
        self._call("dmvs_getcost_quad_f32", C.byref(d), self.stream())
        if self.timers is not None and "dmvs_getcost_quad_f32" in self.timers:      # bench: algorithmic bytes of this launch
            es = ref.element_size()
            self.timers.setdefault("_getcost_bytes", []).append(B * H * W * (es * (Cc + S * Cc) + 4 * (n + S + G * n)))
        return out_cost, out_samples

    def warp_volume(self, src, rt, depth):
        """differentiable_warping: src [B,C,Hs,Ws], rt [B,12], depth [B,D,H,W] -> [B,C,D,H,W]."""
        self._chk(src, rt, depth)
        B, Cc, Hs, Ws = src.shape
        D, H, W = depth.shape[1:]
        out = self.empty(B, Cc, D, H, W)
        self._call("dmvs_warp_volume_f32", _ptr(src), _ptr(rt), _ptr(depth), _ptr(out), B, Cc, D, H, W, Hs, Ws,
                   self.stream())
        return out

    # ------------------------------------------------------------------ backward (training step)
    def warp_corr_init_bwd(self, ref, src, rt, disp_min, disp_max, gcor, gsrc=None, gather=True):
        """-> gref [B,H,W,C], gsrc [S,B,Hs,Ws,C] (accumulated into `gsrc` if given).  gather=False selects the LDS-window
        kernel (C = 48); measured slower than the per-pixel kernel at training sizes (10.9 vs 8.4 ms at cfg4: only ~10^3
        long-running tile x view workgroups), so it is not the default."""
        self._chk(ref, src, rt, disp_min, disp_max, gcor, gsrc)
        B, H, W, Cc = ref.shape
        S, _, Hs, Ws, _ = src.shape
        G, D = gcor.shape[2], gcor.shape[3]
        gref = self.empty_like(ref)
        if gsrc is None:
            gsrc = torch.zeros_like(src)
        mode = (_lib.BWD_GATHER_INTERLEAVED if self.tune.get("bwd_il") else 1) if gather else 0
        self._call("dmvs_warp_corr_init_bwd_f32", _ptr(ref), _ptr(src), _ptr(rt), _ptr(disp_min), _ptr(disp_max), _ptr(gcor),
                   _ptr(gref), _ptr(gsrc), B, S, Cc, G, D, H, W, Hs, Ws, mode, self.stream())
        return gref, gsrc

    def getcost_bwd(self, ref, src, rt, inv_depth, confidence, view_w, disp_min, disp_max, n, interval, min_radius,
                    max_radius, vw_shift, gcost, gsrc=None, G=4, gather=None, worklist=None):
        """-> gref [B,H,W,C], gsrc [S,B,H,W,C] (accumulated into `gsrc` if given).  `worklist`: caller-owned int32 scratch of
        4 + 66 * ntiles entries (16x16 tiles; layout in csrc/warp_tile.h) used instead of the internal one, so that the caller can
        read the tile dispatch back; ignored on the paths that take none (gather, C = 48, S > MAX_WINDOW_VIEWS)."""
        gather = self.tune.get("bwd_gather", False) if gather is None else gather
        self._chk(ref, src, rt, inv_depth, confidence, view_w, disp_min, disp_max, gcost, gsrc)
        B, H, W, Cc = ref.shape
        S = src.shape[0]
        gref = self.empty_like(ref)
        if gsrc is None:
            gsrc = torch.zeros_like(src)
        ntiles = B * ((H + 15) // 16) * ((W + 15) // 16)
        if gather or Cc == 48 or S > MAX_WINDOW_VIEWS:
            wl = None
        elif worklist is not None:
            if worklist.dtype != torch.int32 or worklist.device != self.device or not worklist.is_contiguous() \
                    or worklist.numel() < 4 + 66 * ntiles:
                raise ValueError(f"worklist: contiguous int32 of at least {4 + 66 * ntiles} entries on {self.device}")
            wl = worklist
        else:
            wl = torch.empty(4 + 66 * ntiles, dtype=torch.int32, device=self.device)
        d = _lib.GetCostDesc(ref=_ptr(ref), src=_ptr(src), rt=_ptr(rt), inv_depth=_ptr(inv_depth),
                             confidence=_ptr(confidence), view_w=_ptr(view_w), disp_min=_ptr(disp_min),
                             disp_max=_ptr(disp_max), out_cost=None, out_samples=None, worklist=_ptr(wl), B=B, S=S, C=Cc, G=G, n=n,
                             H=H, W=W, vw_shift=vw_shift, cost_cstride=G * n, cost_coffset=0, samp_cstride=n, samp_coffset=0,
                             interval=interval, min_radius=min_radius, max_radius=max_radius,
                             tune=(_lib.TUNE_BWD_INTERLEAVED if self.tune.get("bwd_il") else 0))
        self._call("dmvs_getcost_bwd_f32", C.byref(d), _ptr(gcost), _ptr(gref), _ptr(gsrc), self.stream())
        if self.timers is not None and "dmvs_getcost_bwd_f32" in self.timers:
            # bench cfg4, algorithmic bytes: read ref + src + grad_cost, write grad_ref, read-modify-write grad_src (the scatter target)
            self.timers.setdefault("_getcost_bwd_bytes", []).append(4.0 * B * H * W * (Cc + S * Cc + G * n + Cc + 2 * S * Cc))
        return gref, gsrc

    def view_aggregate_bwd(self, cor, w, out, gout):
        self._chk(cor, w, out, gout)
        B, S, G, D, H, W = cor.shape
        gcor, gw = self.empty_like(cor), self.empty_like(w)
        self._call("dmvs_view_aggregate_bwd_f32", _ptr(cor), _ptr(w), _ptr(out), _ptr(gout), _ptr(gcor), _ptr(gw), B, S,
                   G * D, H * W, self.stream())
        return gcor, gw

    def view_aggregate(self, cor, w):
        """cor [B,S,G,D,H,W], w [B,S,H,W] -> [B,G,D,H,W]."""
        self._chk(cor, w)
        B, S, G, D, H, W = cor.shape
        out = self.empty(B, G, D, H, W)
        self._call("dmvs_view_aggregate_f32", _ptr(cor), _ptr(w), _ptr(out), B, S, G * D, H * W, self.stream())
        return out

    def sigmoid_max_d(self, x):
        """x [N,D,H,W] -> [N,H,W]."""
        self._chk(x)
        N, D, H, W = x.shape
        out = self.empty(N, H, W)
        self._call("dmvs_sigmoid_max_d_f32", _ptr(x), _ptr(out), N, D, H * W, self.stream())
        return out

    def depth_regress(self, logits, disp_min, disp_max):
        """logits [B,D,H,W] -> norm_depth [B,1,H,W], depth [B,H,W], conf [B,1,H,W]."""
        self._chk(logits, disp_min, disp_max)
        B, D, H, W = logits.shape
        nd, depth, conf = self.empty(B, 1, H, W), self.empty(B, H, W), self.empty(B, 1, H, W)
        self._call("dmvs_depth_regress_f32", _ptr(logits), _ptr(disp_min), _ptr(disp_max), _ptr(nd), _ptr(depth),
                      _ptr(conf), B, D, H * W, self.stream())
        return nd, depth, conf

    def convex_upsample(self, inv, mask, disp_min, disp_max, ratio, want_inv=True):
        """inv [B,1,H,W] or [B,H,W]; mask [B,9*r*r,H,W] -> (inv_up [B,rH,rW] | None, depth_up [B,rH,rW])."""
        self._chk(inv, mask, disp_min, disp_max)
        B, H, W = inv.shape[0], inv.shape[-2], inv.shape[-1]
        assert mask.shape[1] == 9 * ratio * ratio
        out_inv = self.empty(B, H * ratio, W * ratio) if want_inv else None
        out_depth = self.empty(B, H * ratio, W * ratio)
        self._call("dmvs_convex_upsample_f32", _ptr(inv), _ptr(mask), _ptr(disp_min), _ptr(disp_max), _ptr(out_inv),
                      _ptr(out_depth), B, H, W, ratio, self.stream())
        return out_inv, out_depth

    def mask_upsample4(self, pc: PackedConv, x, inv, disp_min, disp_max, post_scale=0.25, want_inv=False):
        """post_scale * conv1x1(pc, x) -> softmax over the 9 taps -> convex x4 upsampling of inv -> metric depth, in one launch (the
        144-channel mask is never materialised): x [B,64,H,W], inv [B,1,H,W] or [B,H,W] -> (inv_up | None, depth_up [B,4H,4W]).
        Bit-identical to convex_upsample(inv, conv2d(pc, x, post_scale=post_scale), ..., 4)."""
        self._chk(x, inv, disp_min, disp_max)
        B, cin, H, W = x.shape
        if pc.k != (1, 1) or pc.cin != cin or pc.cout != 144 or pc.scale is not None:
            raise _lib.DmvsError("mask_upsample4: expects the 64 -> 144 1x1 layer of the DiffMVS mask head")
        out_inv = self.empty(B, H * 4, W * 4) if want_inv else None
        out_depth = self.empty(B, H * 4, W * 4)
        self._call("dmvs_mask_upsample4_f32", _ptr(x), _ptr(pc.weight), _ptr(pc.shift), post_scale, _ptr(inv), _ptr(disp_min), _ptr(disp_max),
                   _ptr(out_inv), _ptr(out_depth), B, cin, pc.cout_pad, H, W, self.stream())
        return out_inv, out_depth

    def groupnorm_silu(self, x, gamma, beta, groups, scale_shift=None, residual=None, out=None, eps=1e-5):
        self._chk(x, gamma, beta, scale_shift, residual, out)
        B, Cc, H, W = x.shape
        if out is None:
            out = self.empty(B, Cc, H, W)
        stats = torch.empty(B * groups * 2, dtype=torch.float64, device=self.device)
        self._call("dmvs_groupnorm_silu_f32", _ptr(x), _ptr(gamma), _ptr(beta), _ptr(scale_shift), _ptr(residual),
                      _ptr(out), _ptr(stats), B, Cc, H * W, groups, eps, self.stream())
        return out

    def groupnorm_silu_train(self, x, gamma, beta, groups, scale_shift=None, eps=1e-5):
        """forward that also returns the statistics buffer the backward needs"""
        self._chk(x, gamma, beta, scale_shift)
        B, Cc, H, W = x.shape
        out = self.empty(B, Cc, H, W)
        stats = torch.empty(B * groups * 2, dtype=torch.float64, device=self.device)
        self._call("dmvs_groupnorm_silu_f32", _ptr(x), _ptr(gamma), _ptr(beta), _ptr(scale_shift), None, _ptr(out), _ptr(stats), B, Cc,
                   H * W, groups, eps, self.stream())
        return out, stats

    def groupnorm_silu_bwd(self, x, dy, gamma, beta, groups, stats, scale_shift=None, eps=1e-5):
        self._chk(x, dy, gamma, beta, scale_shift)
        B, Cc, H, W = x.shape
        dx = self.empty_like(x)
        dgamma, dbeta = self.empty(Cc), self.empty(Cc)
        dss = self.empty(B, 2 * Cc) if scale_shift is not None else None
        n = C.c_int64(0)
        self._call("dmvs_groupnorm_silu_bwd_workspace_f32", B, Cc, H * W, C.byref(n))
        ws = self.empty(max(n.value // 4, 1))
        self._call("dmvs_groupnorm_silu_bwd_f32", _ptr(x), _ptr(dy), _ptr(gamma), _ptr(beta), _ptr(scale_shift), _ptr(stats), _ptr(dx),
                   _ptr(dgamma), _ptr(dbeta), _ptr(dss), _ptr(ws), n.value, B, Cc, H * W, groups, eps, self.stream())
        return dx, dgamma, dbeta, dss

    def groupnorm_apply(self, x, gamma, beta, groups, stats, scale_shift=None, residual=None, out=None, eps=1e-5):
        """normalise + scale/shift + SiLU (+ residual) with statistics accumulated by conv2d(gn_stats=...)."""
        self._chk(x, gamma, beta, scale_shift, residual, out)
        B, Cc, H, W = x.shape
        if out is None:
            out = self.empty(B, Cc, H, W)
        self._call("dmvs_groupnorm_apply_f32", _ptr(x), _ptr(gamma), _ptr(beta), _ptr(scale_shift), _ptr(residual),
                   _ptr(out), _ptr(stats), B, Cc, H * W, groups, eps, self.stream())
        return out

    def delta_update(self, inv, delta_in, update, delta_in_scale=1.0, new2=None, new2_cstride=0, new2_coffset=0):
        """-> (delta_out, new_inv), also mirrors new_inv into channel new2_coffset of new2."""
        self._chk(inv, delta_in, update, new2)
        B = inv.shape[0]
        HW = inv.numel() // B
        delta_out = self.empty_like(inv)
        new_inv = self.empty_like(inv)
        self._call("dmvs_delta_update_f32", _ptr(inv), _ptr(delta_in), _ptr(update), delta_in_scale,
                      _ptr(delta_out), _ptr(new_inv), _ptr(new2), new2_cstride, new2_coffset, B, HW, self.stream())
        return delta_out, new_inv

    def depth_convert(self, x, disp_min, disp_max, mode):
        self._chk(x, disp_min, disp_max)
        B = x.shape[0]
        out = self.empty_like(x)
        self._call("dmvs_depth_convert_f32", _ptr(x), _ptr(disp_min), _ptr(disp_max), _ptr(out), mode, B,
                      x.numel() // B, self.stream())
        return out

    def act_slice(self, x, act, c_from, c_count, out=None, out_cstride=None, out_coffset=0):
        self._chk(x, out)
        B, Ct, H, W = x.shape
        if out is None:
            out_cstride = c_count
            out = self.empty(B, c_count, H, W)
        self._call("dmvs_act_slice_f32", _ptr(x), _ptr(out), act, B, c_count, H * W, Ct, c_from, out_cstride,
                      out_coffset, self.stream())
        return out

    def upsample_nearest(self, x, factor):
        """x [..., H, W] -> [..., fH, fW]."""
        self._chk(x)
        H, W = x.shape[-2], x.shape[-1]
        N = x.numel() // (H * W)
        out = self.empty(*x.shape[:-2], H * factor, W * factor)
        self._call("dmvs_upsample_nearest_f32", _ptr(x), _ptr(out), N, H, W, factor, self.stream())
        return out

    def nchw_to_nhwc(self, x):
        self._chk(x)
        B, Cc, H, W = x.shape
        out = self.empty(B, H, W, Cc)
        self._call("dmvs_nchw_to_nhwc_f32", _ptr(x), _ptr(out), B, Cc, H * W, self.stream())
        return out

    # ------------------------------------------------------------------ training-mode BatchNorm
    def _bn_ws(self, B, Cc, S, views):
        n = C.c_int64(0)
        self._call("dmvs_batchnorm_workspace_f32", B, Cc, S, views, C.byref(n))
        return self.empty(max(n.value // 4, 1)), n.value

    def batchnorm_train_fwd(self, x, gamma, beta, running_mean, running_var, momentum=0.1, eps=1e-5, act=ACT_NONE, views=1,
                            view_major=True):
        """x [B,C,*spatial] -> y, save_mean [views,C], save_rstd [views,C]; running stats updated in place (once per view)"""
        self._chk(x, gamma, beta, running_mean, running_var)
        B, Cc = x.shape[0], x.shape[1]
        S = x.numel() // (B * Cc)
        y = self.empty_like(x)
        mean, rstd = self.empty(views, Cc), self.empty(views, Cc)
        ws, nb = self._bn_ws(B, Cc, S, views)
        bump_weights_generation()         # running_mean / running_var are rewritten in place
        self._call("dmvs_batchnorm_train_fwd_f32", _ptr(x), _ptr(gamma), _ptr(beta), _ptr(running_mean), _ptr(running_var), _ptr(y),
                   _ptr(mean), _ptr(rstd), _ptr(ws), nb, B, Cc, S, views, int(view_major), momentum, eps, act, self.stream())
        return y, mean, rstd

    def batchnorm_train_bwd(self, x, dy, gamma, beta, mean, rstd, act=ACT_NONE, views=1, view_major=True):
        self._chk(x, dy, gamma, beta, mean, rstd)
        B, Cc = x.shape[0], x.shape[1]
        S = x.numel() // (B * Cc)
        dx = self.empty_like(x)
        dgamma, dbeta = self.empty(Cc), self.empty(Cc)
        ws, nb = self._bn_ws(B, Cc, S, views)
        self._call("dmvs_batchnorm_train_bwd_f32", _ptr(x), _ptr(dy), _ptr(gamma), _ptr(beta), _ptr(mean), _ptr(rstd), _ptr(dx),
                   _ptr(dgamma), _ptr(dbeta), _ptr(ws), nb, B, Cc, S, views, int(view_major), act, self.stream())
        return dx, dgamma, dbeta

    # ------------------------------------------------------------------ training-step tail
    def sumsq(self, g, out=None):
        """sum of squares of a flat fp32 tensor -> device double scalar"""
        self._chk(g)
        if out is None:
            out = self.empty(1, dtype=torch.float64)
        self._call("dmvs_sumsq_f32", _ptr(g), g.numel(), _ptr(out), self.stream())
        return out

    def adamw_step(self, p, g, m, v, lr, beta1, beta2, eps, wd, step, grad_scale=1.0, sumsq=None, max_norm=0.0):
        self._chk(p, g, m, v)
        bump_weights_generation()         # parameters are rewritten in place
        self._call("dmvs_adamw_step_f32", _ptr(p), _ptr(g), _ptr(m), _ptr(v), p.numel(), lr, beta1, beta2, eps, wd, step,
                   grad_scale, _ptr(sumsq), max_norm, self.stream())

    # ------------------------------------------------------------------ COLMAP import: view selection
    def view_scores(self, xyz, offsets, images, mult, centres, theta0=5.0, sigma1=1.0, sigma2=10.0):
        """dmvs_view_select_scores_f64: the [N,N] fp64 pair scores of colmap_input.py:374-390 from a point -> image CSR (include/dmvs.h).
        xyz [P,3] / centres [N,3] fp64, offsets [P+1] int64, images / mult [E] int32, all on this binding's device."""
        self._chk_typed("view_scores", (xyz, torch.float64), (centres, torch.float64), (offsets, torch.int64), (images, torch.int32), (mult, torch.int32))
        N, P = int(centres.shape[0]), int(xyz.shape[0])
        if not 1 <= N <= _lib.VIEW_SELECT_MAX_IMAGES:
            raise _lib.DmvsError(f"view_scores: {N} images; the score matrix supports 1..{_lib.VIEW_SELECT_MAX_IMAGES}")
        if offsets.numel() != P + 1 or images.numel() != mult.numel():
            raise _lib.DmvsError("view_scores: offsets must have P+1 entries and images / mult one per CSR entry")
        if images.numel():            # the fixed-point range: every image's total multiplicity stays below 2^23
            per_image = torch.zeros(N, dtype=torch.int64, device=self.device).index_add_(0, images.long().clamp(0, N - 1), mult.long())
            if int(per_image.max()) >= _lib.VIEW_SELECT_MAX_LIST:
                raise _lib.DmvsError(f"view_scores: an image lists {int(per_image.max())} points; at most {_lib.VIEW_SELECT_MAX_LIST - 1} are supported")
        L = offsets[1:] - offsets[:-1]
        pair_off = torch.zeros(P + 1, dtype=torch.int64, device=self.device)
        torch.cumsum(L * (L - 1) // 2, 0, out=pair_off[1:])
        terms = int(pair_off[-1]) if P else 0
        ws = torch.empty(max(1, N * (N - 1) // 2), dtype=torch.int64, device=self.device)
        out = self.empty(N, N, dtype=torch.float64)
        self._call("dmvs_view_select_scores_f64", _ptr(xyz), _ptr(offsets), _ptr(images), _ptr(mult), _ptr(pair_off), P, terms, _ptr(centres), N,
                   float(theta0), float(sigma1), float(sigma2), _ptr(ws), _ptr(out), self.stream())
        return out

    # ------------------------------------------------------------------ point-cloud scoring (diffmvs_amd/cloud_eval.py)
    def _cloud_nn(self, what, query, target, cell_keys, cell_start, origin, h, dims, max_dist, transform, want_dist, want_index, work):
        """the checks and the call both grid searches share -> (dist or None, index or None, work or None)"""
        self._chk_typed(what, (query, torch.float32), (target, torch.float32), (cell_keys, torch.int64), (cell_start, torch.int64))
        Q, M, Cn = int(query.shape[0]), int(target.shape[0]), int(cell_keys.numel())
        if query.dim() != 2 or query.shape[1] != 3 or target.dim() != 2 or target.shape[1] != 3:
            raise _lib.DmvsError(f"{what}: query and target must be [N,3]")
        if cell_start.numel() != Cn + 1 or Cn > M or (M > 0 and Cn < 1):
            raise _lib.DmvsError(f"{what}: cell_start must have one entry more than cell_keys, and every target a cell")
        dist = self.empty(Q) if want_dist else None
        index = torch.empty(Q, dtype=torch.int32, device=self.device) if want_index else None
        wk = torch.empty(Q, 2, dtype=torch.int32, device=self.device) if work else None
        grid = (_ptr(query), Q, _ptr(target), M, _ptr(cell_keys), _ptr(cell_start), Cn, (C.c_double * 3)(*[float(v) for v in origin]), float(h),
                (C.c_int32 * 3)(*[int(v) for v in dims]), float(max_dist))
        if want_index:
            self._call("dmvs_cloud_nn_index_f32", *grid, self._transform_arg(transform), _ptr(dist), _ptr(index), _ptr(wk), self.stream())
        else:
            self._call("dmvs_cloud_nn_dist_f32", *grid, _ptr(dist), _ptr(wk), self.stream())
        return dist, index, wk

    def cloud_nn_dist(self, query, target, cell_keys, cell_start, origin, h, dims, max_dist, work=False):
        """dmvs_cloud_nn_dist_f32: min(|q - nearest target|, max_dist) per query (include/dmvs.h).  query [Q,3] / target [M,3] fp32 with the
        targets sorted by cell key, cell_keys [C] / cell_start [C+1] int64, origin 3 floats, dims 3 ints.
        -> dist [Q] fp32, or (dist, work [Q,2] int32: rings walked, targets tested) with work=True."""
        dist, _, wk = self._cloud_nn("cloud_nn_dist", query, target, cell_keys, cell_start, origin, h, dims, max_dist, None, True, False, work)
        return (dist, wk) if work else dist

    def cloud_stats(self, dist, valid, max_dist, thresholds, scale, blocks=0):
        """dmvs_cloud_stats_f32 -> [3 + T] int64 on the device: valid points, those with d < max_dist, their fixed-point sum
        (rint(d * scale) per term), and per threshold the valid points with d < threshold (include/dmvs.h)."""
        self._chk_typed("cloud_stats", (dist, torch.float32), (valid, torch.uint8))
        T = len(thresholds)
        if T > _lib.CLOUD_MAX_THRESHOLDS:
            raise _lib.DmvsError(f"cloud_stats: {T} thresholds; at most {_lib.CLOUD_MAX_THRESHOLDS} are supported")
        if valid is not None and valid.numel() != dist.numel():
            raise _lib.DmvsError("cloud_stats: the validity mask must have one entry per distance")
        out = torch.empty(3 + T, dtype=torch.int64, device=self.device)
        thr = (C.c_float * max(1, T))(*[float(t) for t in thresholds])
        self._call("dmvs_cloud_stats_f32", _ptr(dist), _ptr(valid), dist.numel(), float(max_dist), thr, T, float(scale), int(blocks),
                   _ptr(out), self.stream())
        return out

    # ------------------------------------------------------------------ registration and cropping (diffmvs_amd/cloud_register.py)
    @staticmethod
    def _transform_arg(transform):
        """None or anything shaped [3,4] / [4,4] -> a host array of 12 doubles (row-major [sR | t]) or None"""
        if transform is None:
            return None
        import numpy as np
        m = np.asarray(transform.detach().cpu().numpy() if torch.is_tensor(transform) else transform, np.float64)
        if m.shape not in ((3, 4), (4, 4)):
            raise _lib.DmvsError(f"a transform is a 3x4 or 4x4 matrix, got {m.shape}")
        return (C.c_double * 12)(*[float(v) for v in m[:3].reshape(-1)])

    def cloud_nn_index(self, query, target, cell_keys, cell_start, origin, h, dims, max_dist, transform=None, dist=True, work=False):
        """dmvs_cloud_nn_index_f32: cloud_nn_dist on the query moved by `transform`, plus the position of the nearest target in the
        sorted target array (-1 where nothing is closer than max_dist).  -> (dist [Q] fp32 or None, index [Q] int32[, work [Q,2]])."""
        d, index, wk = self._cloud_nn("cloud_nn_index", query, target, cell_keys, cell_start, origin, h, dims, max_dist, transform, dist, True, work)
        return (d, index, wk) if work else (d, index)

    def cloud_pair_moments(self, source, transform, target, index, valid, max_corr, center_p, center_q, bound, scale_linear, scale_quadratic,
                           blocks=0):
        """dmvs_cloud_pair_moments_f64 -> [20] int64 on the device: the fixed-point sums of one ICP step (include/dmvs.h)"""
        self._chk_typed("cloud_pair_moments", (source, torch.float32), (target, torch.float32), (index, torch.int32), (valid, torch.uint8))
        N = int(source.shape[0])
        if source.dim() != 2 or source.shape[1] != 3 or target.dim() != 2 or target.shape[1] != 3:
            raise _lib.DmvsError("cloud_pair_moments: source and target must be [N,3]")
        if index.numel() != N or (valid is not None and valid.numel() != N):
            raise _lib.DmvsError("cloud_pair_moments: index (and the validity mask) must have one entry per source point")
        out = torch.empty(_lib.CLOUD_MOMENTS, dtype=torch.int64, device=self.device)
        cp = (C.c_double * 3)(*[float(v) for v in center_p])
        cq = (C.c_double * 3)(*[float(v) for v in center_q])
        self._call("dmvs_cloud_pair_moments_f64", _ptr(source), N, self._transform_arg(transform), _ptr(target), int(target.shape[0]), _ptr(index),
                   _ptr(valid), float(max_corr), cp, cq, float(bound), float(scale_linear), float(scale_quadratic), int(blocks), _ptr(out),
                   self.stream())
        return out

    def cloud_crop_prism(self, points, polygon, axis, axis_min, axis_max, transform=None):
        """dmvs_cloud_crop_prism_f32 -> uint8 [N]: 1 where the (moved) point lies inside the polygon prism.  polygon [K,2] fp64 on this
        binding's device, axis 0 / 1 / 2 (include/dmvs.h)."""
        self._chk_typed("cloud_crop_prism", (points, torch.float32), (polygon, torch.float64))
        if points.dim() != 2 or points.shape[1] != 3 or polygon.dim() != 2 or polygon.shape[1] != 2:
            raise _lib.DmvsError("cloud_crop_prism: points must be [N,3] and the polygon [K,2]")
        K = int(polygon.shape[0])
        if not 3 <= K <= _lib.CLOUD_MAX_POLYGON:
            raise _lib.DmvsError(f"cloud_crop_prism: a polygon of {K} vertices; 3..{_lib.CLOUD_MAX_POLYGON} are supported")
        out = torch.empty(points.shape[0], dtype=torch.uint8, device=self.device)
        self._call("dmvs_cloud_crop_prism_f32", _ptr(points), int(points.shape[0]), self._transform_arg(transform), _ptr(polygon), K, int(axis),
                   float(axis_min), float(axis_max), _ptr(out), self.stream())
        return out

    # ------------------------------------------------------------------ point-cloud cleaning (diffmvs_amd/cloud_clean.py)
    def cloud_knn(self, query, target, cell_keys, cell_start, origin, h, dims, max_dist, k, self_index=None, d2=False, work=False):
        """dmvs_cloud_knn_f32: the k nearest targets of every query closer than max_dist, over the grid operands of cloud_nn_dist
        (include/dmvs.h).  self_index: None or [Q] int32, the sorted-target position query i must not match (-1: none).
        -> {"mean" [Q] fp32, "kth" [Q] fp32, "found" [Q] int32[, "d2" [Q,k] fp32 ascending, padded with max_dist^2][, "work" [Q,2] int32]}."""
        self._chk_typed("cloud_knn", (query, torch.float32), (target, torch.float32), (cell_keys, torch.int64), (cell_start, torch.int64),
                        (self_index, torch.int32))
        Q, M, Cn, k = int(query.shape[0]), int(target.shape[0]), int(cell_keys.numel()), int(k)
        if query.dim() != 2 or query.shape[1] != 3 or target.dim() != 2 or target.shape[1] != 3:
            raise _lib.DmvsError("cloud_knn: query and target must be [N,3]")
        if cell_start.numel() != Cn + 1 or Cn > M or (M > 0 and Cn < 1):
            raise _lib.DmvsError("cloud_knn: cell_start must have one entry more than cell_keys, and every target a cell")
        if not 1 <= k <= _lib.CLOUD_MAX_K:
            raise _lib.DmvsError(f"cloud_knn: k = {k}; 1..{_lib.CLOUD_MAX_K} are supported")
        if self_index is not None and self_index.numel() != Q:
            raise _lib.DmvsError("cloud_knn: self_index must have one entry per query")
        out = {"mean": self.empty(Q), "kth": self.empty(Q), "found": torch.empty(Q, dtype=torch.int32, device=self.device)}
        if d2:
            out["d2"] = self.empty(Q, k)
        if work:
            out["work"] = torch.empty(Q, 2, dtype=torch.int32, device=self.device)
        self._call("dmvs_cloud_knn_f32", _ptr(query), Q, _ptr(target), M, _ptr(cell_keys), _ptr(cell_start), Cn,
                   (C.c_double * 3)(*[float(v) for v in origin]), float(h), (C.c_int32 * 3)(*[int(v) for v in dims]), float(max_dist),
                   _ptr(self_index), k, _ptr(out.get("d2")), _ptr(out["kth"]), _ptr(out["mean"]), _ptr(out["found"]), _ptr(out.get("work")),
                   self.stream())
        return out

    # ------------------------------------------------------------------ depth-map scoring (diffmvs_amd/depth_eval.py)
    def depth_stats(self, est, gt, mask, thresholds, big, scale, band=None, blocks=0):
        """dmvs_depth_stats_f32 -> [B, 7 + T] int64 on the device, one row per batch item: masked pixels, scored pixels, pixels left out
        (non-finite est / gt or gt <= 0), clamped terms, the fixed-point sums of |e|, |e| / gt and e^2, and per threshold the scored pixels
        with |e| < threshold (include/dmvs.h).  est, gt [B,H,W] fp32; mask None or [B,H,W] fp32 (> 0.5 = in); band None or (lo, hi)."""
        self._chk_typed("depth_stats", (est, torch.float32), (gt, torch.float32), (mask, torch.float32))
        T = len(thresholds)
        if T > _lib.DEPTH_MAX_THRESHOLDS:
            raise _lib.DmvsError(f"depth_stats: {T} thresholds; at most {_lib.DEPTH_MAX_THRESHOLDS} are supported")
        if est.dim() != 3 or gt.shape != est.shape or (mask is not None and mask.shape != est.shape):
            raise _lib.DmvsError(f"depth_stats: est, gt and the mask must share one [B,H,W] shape, got {tuple(est.shape)}, {tuple(gt.shape)}"
                                 + (f", {tuple(mask.shape)}" if mask is not None else ""))
        B, HW = int(est.shape[0]), int(est.shape[1] * est.shape[2])
        out = torch.empty(B, _lib.DEPTH_SLOTS + T, dtype=torch.int64, device=self.device)
        thr = (C.c_float * max(1, T))(*[float(t) for t in thresholds])
        lo, hi = (0.0, float("inf")) if band is None else (float(band[0]), float(band[1]))
        self._call("dmvs_depth_stats_f32", _ptr(est), _ptr(gt), _ptr(mask), B, HW, thr, T, lo, hi, float(big), float(scale), int(blocks),
                   _ptr(out), self.stream())
        return out

    # ------------------------------------------------------------------ depth maps from a cloud (diffmvs_amd/cloud_render.py)
    def _splat_args(self, what, points, views, size, zbuf):
        """the checks both splat passes share -> (N, V, H, W, the HOST view table)"""
        import numpy as np
        self._chk_typed(what, (points, torch.float32), (zbuf, torch.float32))
        if points.dim() != 2 or points.shape[1] != 3:
            raise _lib.DmvsError(f"{what}: points must be [N,3], got {tuple(points.shape)}")
        v = np.ascontiguousarray(views.detach().cpu().numpy() if torch.is_tensor(views) else views, dtype=np.float64)
        if v.ndim != 2 or v.shape[1] != _lib.SPLAT_VIEW_DOUBLES:
            raise _lib.DmvsError(f"{what}: views must be [V,{_lib.SPLAT_VIEW_DOUBLES}] (two rows of P, row 2 of E, f, near, far), got {v.shape}")
        H, W = int(size[0]), int(size[1])
        V = int(v.shape[0])
        if zbuf is not None and tuple(zbuf.shape) != (V, H, W):
            raise _lib.DmvsError(f"{what}: the z-buffer must be [V,H,W] = {(V, H, W)}, got {tuple(zbuf.shape)}")
        return int(points.shape[0]), V, H, W, v

    def cloud_splat_zmin(self, points, views, size, radius, r_min, r_max, zbuf=None, transform=None, pretest=True, work=False, blocks=0):
        """dmvs_cloud_splat_zmin_f32 (include/dmvs.h): the nearest depth per pixel of every point's footprint.  points [N,3] fp32; views
        [V,15] fp64 on the host (cloud_render.view_table); size (H, W); zbuf: None (a fresh [V,H,W] fp32 buffer of +inf) or one to go on with.
        -> (zbuf, counts [V,4] int64: non-finite, outside the depth range, off the image, radius clamped[, work [2] int64: footprint
        pixels visited, atomics issued])"""
        N, V, H, W, v = self._splat_args("cloud_splat_zmin", points, views, size, zbuf)
        if zbuf is None:
            zbuf = torch.full((V, H, W), float("inf"), dtype=torch.float32, device=self.device)
        fresh = torch.empty if N > 0 and V > 0 else torch.zeros      # (the library zeroes both, unless there is nothing to do)
        counts = fresh((V, _lib.SPLAT_SLOTS), dtype=torch.int64, device=self.device)
        wk = fresh((2,), dtype=torch.int64, device=self.device) if work else None
        self._call("dmvs_cloud_splat_zmin_f32", _ptr(points), N, self._transform_arg(transform), v.ctypes.data_as(C.c_void_p), V, H, W, float(radius),
                   float(r_min), float(r_max), 0 if pretest else _lib.SPLAT_NO_PRETEST, int(blocks), _ptr(zbuf), _ptr(counts), _ptr(wk), self.stream())
        return (zbuf, counts, wk) if work else (zbuf, counts)

    def cloud_splat_sum(self, points, views, size, radius, r_min, r_max, zbuf, tau, scale, transform=None, blocks=0):
        """dmvs_cloud_splat_sum_f32 (include/dmvs.h): over the finished z-buffer of cloud_splat_zmin (same points, views and radii), the
        fixed-point sum and the count of the depths within (1 + tau) of each pixel's nearest.  -> (sum [V,H,W] int64, cnt [V,H,W] int32)"""
        N, V, H, W, v = self._splat_args("cloud_splat_sum", points, views, size, zbuf)
        if zbuf is None:
            raise _lib.DmvsError("cloud_splat_sum: needs the z-buffer of cloud_splat_zmin")
        fresh = torch.empty if N > 0 and V > 0 and H * W > 0 else torch.zeros      # (the library zeroes both, unless there is nothing to do)
        total = fresh((V, H, W), dtype=torch.int64, device=self.device)
        cnt = fresh((V, H, W), dtype=torch.int32, device=self.device)
        self._call("dmvs_cloud_splat_sum_f32", _ptr(points), N, self._transform_arg(transform), v.ctypes.data_as(C.c_void_p), V, H, W, float(radius),
                   float(r_min), float(r_max), float(tau), float(scale), int(blocks), _ptr(zbuf), _ptr(total), _ptr(cnt), self.stream())
        return total, cnt

    # ------------------------------------------------------------------ oriented normals of a depth map (diffmvs_amd/fusion.py)
    @staticmethod
    def normal_cams(K, E):
        """K [B,3,3], E [B,4,4] (world -> camera) -> the HOST [B,27] fp64 table of dmvs_depth_normals_f32: K | inv(K), formed here in
        fp64 | R = E[:3,:3], each row-major"""
        import numpy as np
        K, E = (np.asarray(m.detach().cpu().numpy() if torch.is_tensor(m) else m, np.float64) for m in (K, E))
        if K.ndim != 3 or K.shape[1:] != (3, 3) or E.shape != (K.shape[0], 4, 4):
            raise _lib.DmvsError(f"depth_normals: K must be [B,3,3] and E [B,4,4], got {K.shape} and {E.shape}")
        B = K.shape[0]
        if not (np.isfinite(K).all() and np.isfinite(E).all()):
            raise _lib.DmvsError("depth_normals: a camera matrix with a non-finite entry")
        try:
            Kinv = np.linalg.inv(K) if B else K
        except np.linalg.LinAlgError as e:
            raise _lib.DmvsError("depth_normals: a singular intrinsic matrix") from e
        return np.ascontiguousarray(np.concatenate([K.reshape(B, 9), Kinv.reshape(B, 9), E[:, :3, :3].reshape(B, 9)], 1))

    def depth_normals(self, depth, valid, K, E, radius=2, rel_jump=0.02, min_pts=5):
        """dmvs_depth_normals_f32 (include/dmvs.h): a plane fitted in inverse depth to every pixel's (2 radius + 1)^2 window.  depth [B,H,W]
        fp32; valid None or [B,H,W] uint8 / bool; K [B,3,3], E [B,4,4] on the host (or a ready normal_cams table [B,27]).
        -> (out [B,H,W,4] fp32: the world normal and the cosine to the viewing ray, zeros where there is none; counts [B,4] int64: centre
        not usable, support degenerate, fit rejected, normals written)"""
        import numpy as np
        if valid is not None and valid.dtype == torch.bool:
            valid = valid.view(torch.uint8)
        self._chk_typed("depth_normals", (depth, torch.float32), (valid, torch.uint8))
        if depth.dim() != 3 or (valid is not None and valid.shape != depth.shape):
            raise _lib.DmvsError(f"depth_normals: depth (and the mask) must be [B,H,W], got {tuple(depth.shape)}"
                                 + (f" and {tuple(valid.shape)}" if valid is not None else ""))
        B, H, W = (int(s) for s in depth.shape)
        cams = np.ascontiguousarray(K, np.float64) if E is None else self.normal_cams(K, E)
        if cams.shape != (B, _lib.NORMAL_CAM_DOUBLES):
            raise _lib.DmvsError(f"depth_normals: {B} depth maps need a [{B},{_lib.NORMAL_CAM_DOUBLES}] camera table, got {cams.shape}")
        if not 1 <= int(radius) <= _lib.NORMAL_MAX_RADIUS:
            raise _lib.DmvsError(f"depth_normals: radius {radius}; 1..{_lib.NORMAL_MAX_RADIUS} are supported")
        fresh = torch.empty if B * H * W > 0 else torch.zeros      # (the library writes both, unless there is nothing to do)
        out = fresh((B, H, W, 4), dtype=torch.float32, device=self.device)
        counts = fresh((B, _lib.NORMAL_SLOTS), dtype=torch.int64, device=self.device)
        self._call("dmvs_depth_normals_f32", _ptr(depth), _ptr(valid), cams.ctypes.data_as(C.c_void_p), B, H, W, int(radius), float(rel_jump),
                   int(min_pts), _ptr(out), _ptr(counts), self.stream())
        return out, counts

    # ------------------------------------------------------------------ a surface from depth maps (diffmvs_amd/mesh.py)
    def tsdf_volume(self, dims, origin, h, colour=True) -> "TsdfVolume":
        """a zeroed volume of dmvs_tsdf_integrate_f32 (include/dmvs.h): dims (nx, ny, nz), origin (three doubles), voxel side h"""
        import numpy as np
        nx, ny, nz = (int(d) for d in dims)
        if min(nx, ny, nz) < 0 or nx * ny * nz >= 2 ** 31:
            raise _lib.DmvsError(f"tsdf_volume: dims {(nx, ny, nz)}; the volume must have fewer than 2^31 voxels")
        origin = np.ascontiguousarray(origin, np.float64).reshape(-1)
        if origin.shape != (3,) or not np.isfinite(origin).all() or not (float(h) > 0.0 and np.isfinite(h)):
            raise _lib.DmvsError(f"tsdf_volume: the origin must be three finite numbers and the voxel side positive, got {origin} and {h}")
        z = lambda *s, dt: torch.zeros(*s, dtype=dt, device=self.device)       # noqa: E731
        return TsdfVolume((nx, ny, nz), origin, float(h), z(nz, ny, nx, dt=torch.int32), z(nz, ny, nx, dt=torch.int32),
                          z(nz, ny, nx, 4, dt=torch.int32) if colour else None)

    def _tsdf_vol(self, what, vol):
        self._chk_typed(what, (vol.S, torch.int32), (vol.Wt, torch.int32), (vol.C, torch.int32))
        nx, ny, nz = vol.dims
        if tuple(vol.S.shape) != (nz, ny, nx) or vol.Wt.shape != vol.S.shape or (vol.C is not None and tuple(vol.C.shape) != (nz, ny, nx, 4)):
            raise _lib.DmvsError(f"{what}: S, Wt (and C) must be [nz,ny,nx](,4) = {(nz, ny, nx)}, got {tuple(vol.S.shape)}, {tuple(vol.Wt.shape)}"
                                 + (f", {tuple(vol.C.shape)}" if vol.C is not None else ""))
        return nx, ny, nz, vol.origin.ctypes.data_as(C.c_void_p)

    def tsdf_integrate(self, vol, depth, valid, rgb, views, tau, cull=True):
        """dmvs_tsdf_integrate_f32 (include/dmvs.h): ADDS the truncated signed distances of V depth maps to the volume.  depth [V,H,W] fp32;
        valid None or [V,H,W] uint8 / bool; rgb None or [V,H,W,3] uint8 (the volume then needs its colour sums); views [V,12] fp64 on the
        host (mesh.tsdf_views); tau: the truncation distance.  cull=False: DMVS_TSDF_NO_CULL (the same bits).  -> vol"""
        import numpy as np
        if valid is not None and valid.dtype == torch.bool:
            valid = valid.view(torch.uint8)
        self._chk_typed("tsdf_integrate", (depth, torch.float32), (valid, torch.uint8), (rgb, torch.uint8))
        nx, ny, nz, origin = self._tsdf_vol("tsdf_integrate", vol)
        if depth.dim() != 3 or (valid is not None and valid.shape != depth.shape) or (rgb is not None and tuple(rgb.shape) != tuple(depth.shape) + (3,)):
            raise _lib.DmvsError(f"tsdf_integrate: depth (and the mask) must be [V,H,W] and rgb [V,H,W,3], got {tuple(depth.shape)}"
                                 + (f", {tuple(valid.shape)}" if valid is not None else "") + (f", {tuple(rgb.shape)}" if rgb is not None else ""))
        V, H, W = (int(s) for s in depth.shape)
        v = np.ascontiguousarray(views.detach().cpu().numpy() if torch.is_tensor(views) else views, dtype=np.float64)
        if v.shape != (V, _lib.TSDF_VIEW_DOUBLES):
            raise _lib.DmvsError(f"tsdf_integrate: {V} depth maps need a [{V},{_lib.TSDF_VIEW_DOUBLES}] view table (two rows of P, row 2 of E), got {v.shape}")
        if rgb is not None and vol.C is None:
            raise _lib.DmvsError("tsdf_integrate: colours need a volume made with colour=True")
        if vol.views + V > _lib.TSDF_MAX_VIEWS:
            raise _lib.DmvsError(f"tsdf_integrate: {vol.views} + {V} views; a volume takes at most {_lib.TSDF_MAX_VIEWS} (its sums are 32-bit)")
        self._call("dmvs_tsdf_integrate_f32", _ptr(depth), _ptr(valid), _ptr(rgb), v.ctypes.data_as(C.c_void_p), V, H, W, nx, ny, nz, origin,
                   float(vol.h), float(tau), 0 if cull else _lib.TSDF_NO_CULL, _ptr(vol.S), _ptr(vol.Wt), _ptr(vol.C), self.stream())
        vol.views += V
        return vol

    def tsdf_extract(self, vol, min_weight=1):
        """dmvs_tsdf_flags_u8 / _vertices_f32 / _faces_i32 (include/dmvs.h): the surface-nets mesh of the volume's zero set over the voxels
        with Wt >= min_weight.  -> (verts [N,3] fp32, rgb [N,3] uint8 (zeros without colour sums), faces [F,3] int32)"""
        nx, ny, nz, origin = self._tsdf_vol("tsdf_extract", vol)
        dev, n = self.device, nx * ny * nz
        cell = torch.empty((nz, ny, nx), dtype=torch.uint8, device=dev)
        quad = torch.empty((nz, ny, nx), dtype=torch.uint8, device=dev)
        self._call("dmvs_tsdf_flags_u8", _ptr(vol.S), _ptr(vol.Wt), nx, ny, nz, int(min_weight), _ptr(cell), _ptr(quad), self.stream())
        N = Q = 0
        if n > 0:
            cell_cum = torch.cumsum(cell.reshape(-1), 0, dtype=torch.int32)      # (N <= n < 2^31)
            quad_cum = torch.cumsum(((quad & 1) + ((quad >> 1) & 1) + (quad >> 2)).reshape(-1), 0, dtype=torch.int64)
            N, Q = int(cell_cum[-1]), int(quad_cum[-1])
            if Q > _lib.TSDF_MAX_QUADS:
                raise _lib.DmvsError(f"tsdf_extract: {Q} quads; at most {_lib.TSDF_MAX_QUADS} are supported (int32 face tables): use a coarser volume")
            quad_cum = quad_cum.to(torch.int32)
        verts = torch.empty((N, 3), dtype=torch.float32, device=dev)
        rgb = torch.empty((N, 3), dtype=torch.uint8, device=dev)
        faces = torch.empty((2 * Q, 3), dtype=torch.int32, device=dev)
        if N > 0:
            self._call("dmvs_tsdf_vertices_f32", _ptr(vol.S), _ptr(vol.Wt), _ptr(vol.C), nx, ny, nz, origin, float(vol.h), _ptr(cell), _ptr(cell_cum), N,
                       _ptr(verts), _ptr(rgb), self.stream())
        if Q > 0:
            self._call("dmvs_tsdf_faces_i32", _ptr(vol.S), nx, ny, nz, _ptr(quad), _ptr(quad_cum), _ptr(cell_cum), Q, _ptr(faces), self.stream())
        return verts, rgb, faces

    # ------------------------------------------------------------------ triangle meshes into the views (diffmvs_amd/mesh_render.py)
    def _raster_args(self, what, verts, faces, views):
        """the checks both raster passes share -> (N, F, V, the HOST view table)"""
        import numpy as np
        self._chk_typed(what, (verts, torch.float32), (faces, torch.int32))
        if verts.dim() != 2 or verts.shape[1] != 3 or faces.dim() != 2 or faces.shape[1] != 3:
            raise _lib.DmvsError(f"{what}: verts must be [N,3] and faces [F,3], got {tuple(verts.shape)} and {tuple(faces.shape)}")
        v = np.ascontiguousarray(views.detach().cpu().numpy() if torch.is_tensor(views) else views, dtype=np.float64)
        if v.ndim != 2 or v.shape[1] != _lib.RASTER_VIEW_DOUBLES:
            raise _lib.DmvsError(f"{what}: views must be [V,{_lib.RASTER_VIEW_DOUBLES}] (two rows of P, E[:3], near, far), got {v.shape}")
        return int(verts.shape[0]), int(faces.shape[0]), int(v.shape[0]), v

    def mesh_raster_zid(self, verts, faces, views, size, cull=None, transform=None, zid=None, queue_cap=None, blocks=0, work=False):
        """dmvs_mesh_raster_fill_u64 / dmvs_mesh_raster_zid_u64 (include/dmvs.h): per pixel the smallest (depth bits << 32 | face) of the
        faces that cover it.  verts [N,3] fp32, faces [F,3] int32; views [V,22] fp64 on the host (mesh_render.view_table); size (H, W);
        cull None | "neg" | "pos"; zid: None (a fresh [V,H,W] buffer of all ones) or one to go on with, int64 holding the uint64 keys;
        queue_cap: entries of the wave pass's queue, None = one per (face, view) of a launch up to RASTER_QUEUE_ENTRIES, 0 = no wave pass.
        -> (zid, counts [V,8] int64[, work [3] int64: covered pixels, atomics issued, faces that fell back])"""
        N, F, V, v = self._raster_args("mesh_raster_zid", verts, faces, views)
        H, W = int(size[0]), int(size[1])
        if cull not in (None, "neg", "pos"):
            raise _lib.DmvsError(f"mesh_raster_zid: cull must be None, 'neg' or 'pos', got {cull!r}")
        flags = {None: 0, "neg": _lib.RASTER_CULL_NEG, "pos": _lib.RASTER_CULL_POS}[cull]
        if zid is None:
            zid = torch.empty((V, H, W), dtype=torch.int64, device=self.device)
            self._call("dmvs_mesh_raster_fill_u64", _ptr(zid), zid.numel(), self.stream())
        elif zid.dtype != torch.int64 or tuple(zid.shape) != (V, H, W) or not zid.is_contiguous() or zid.device != self.device:
            raise _lib.DmvsError(f"mesh_raster_zid: zid must be a contiguous int64 [V,H,W] = {(V, H, W)} on {self.device}")
        if queue_cap is None:
            queue_cap = min(F * min(V, _lib.SPLAT_VIEW_CHUNK), RASTER_QUEUE_ENTRIES)
        queue = torch.empty(1 + int(queue_cap), dtype=torch.int64, device=self.device) if queue_cap > 0 else None
        counts = torch.empty((V, _lib.RASTER_SLOTS), dtype=torch.int64, device=self.device)
        wk = torch.empty((3,), dtype=torch.int64, device=self.device) if work else None
        self._call("dmvs_mesh_raster_zid_u64", _ptr(verts), N, _ptr(faces), F, self._transform_arg(transform), v.ctypes.data_as(C.c_void_p), V, H, W,
                   flags, int(blocks), _ptr(zid), _ptr(counts), _ptr(wk), _ptr(queue), int(queue_cap), self.stream())
        return (zid, counts, wk) if work else (zid, counts)

    def mesh_raster_resolve(self, zid, verts, faces, views, transform=None, vrgb=None, normals=False):
        """dmvs_mesh_raster_resolve_f32 (include/dmvs.h) over the finished zid of mesh_raster_zid (same mesh, transform and views).
        -> (depth [V,H,W] fp32, 0 where nothing was drawn; face [V,H,W] int32, -1 there; normal [V,H,W,3] fp32 or None: the winning
        face's unit normal in the world frame, turned to the camera; rgb [V,H,W,3] uint8 or None: vrgb [N,3] uint8 interpolated)"""
        N, F, V, v = self._raster_args("mesh_raster_resolve", verts, faces, views)
        self._chk_typed("mesh_raster_resolve", (zid, torch.int64), (vrgb, torch.uint8))
        if zid.dim() != 3 or zid.shape[0] != V or (vrgb is not None and tuple(vrgb.shape) != (N, 3)):
            raise _lib.DmvsError(f"mesh_raster_resolve: zid must be [V,H,W] with V = {V} and vrgb [N,3], got {tuple(zid.shape)}"
                                 + (f" and {tuple(vrgb.shape)}" if vrgb is not None else ""))
        H, W = int(zid.shape[1]), int(zid.shape[2])
        depth = torch.empty((V, H, W), dtype=torch.float32, device=self.device)
        face = torch.empty((V, H, W), dtype=torch.int32, device=self.device)
        normal = torch.empty((V, H, W, 3), dtype=torch.float32, device=self.device) if normals else None
        rgb = torch.empty((V, H, W, 3), dtype=torch.uint8, device=self.device) if vrgb is not None else None
        self._call("dmvs_mesh_raster_resolve_f32", _ptr(zid), _ptr(verts), N, _ptr(faces), F, self._transform_arg(transform),
                   v.ctypes.data_as(C.c_void_p), V, H, W, _ptr(vrgb), _ptr(depth), _ptr(face), _ptr(normal), _ptr(rgb), self.stream())
        return depth, face, normal, rgb

    # ------------------------------------------------------------------ cleaning and scoring a mesh (diffmvs_amd/mesh_clean.py, mesh_eval.py)
    def _mesh_args(self, what, verts, faces):
        self._chk_typed(what, (verts, torch.float32), (faces, torch.int32))
        if (verts is not None and (verts.dim() != 2 or verts.shape[1] != 3)) or faces.dim() != 2 or faces.shape[1] != 3:
            raise _lib.DmvsError(f"{what}: verts must be [N,3] and faces [F,3], got {None if verts is None else tuple(verts.shape)} and {tuple(faces.shape)}")

    def mesh_label_round(self, faces, label, state=None, blocks=0):
        """dmvs_mesh_label_round_i32 (include/dmvs.h): one hook + shortcut round on label [N] int32 (label[v] = v before the first), in
        place.  state: None or an int32 [2] to write.  -> state (device): atomics issued (0: the labels are final), out-of-range faces"""
        self._mesh_args("mesh_label_round", None, faces)
        self._chk_typed("mesh_label_round", (label, torch.int32), (state, torch.int32))
        if label.dim() != 1 or (state is not None and tuple(state.shape) != (2,)):
            raise _lib.DmvsError(f"mesh_label_round: label must be [N] and state [2], got {tuple(label.shape)}"
                                 + (f" and {tuple(state.shape)}" if state is not None else ""))
        if state is None:
            state = torch.empty((2,), dtype=torch.int32, device=self.device)
        self._call("dmvs_mesh_label_round_i32", _ptr(faces), int(faces.shape[0]), int(label.shape[0]), _ptr(label), _ptr(state), int(blocks), self.stream())
        return state

    def mesh_face_tally(self, verts, faces, label, scale, cap, blocks=0):
        """dmvs_mesh_face_tally_i64 (include/dmvs.h): label [N] int32 (mesh_label_round's fixpoint); scale: a power of two; cap: the bound of
        one face's scaled area.  -> (area_q [F] int64, comp_faces [N] int32, comp_area [N] int64; the sums sit at the components' roots)"""
        self._mesh_args("mesh_face_tally", verts, faces)
        self._chk_typed("mesh_face_tally", (label, torch.int32))
        N, F = int(verts.shape[0]), int(faces.shape[0])
        if tuple(label.shape) != (N,):
            raise _lib.DmvsError(f"mesh_face_tally: label must be [N] = [{N}], got {tuple(label.shape)}")
        fresh = torch.empty if N > 0 else torch.zeros      # (with no vertices the library touches nothing: every face is out of range)
        area_q = fresh((F,), dtype=torch.int64, device=self.device)
        comp_faces = torch.empty((N,), dtype=torch.int32, device=self.device)
        comp_area = torch.empty((N,), dtype=torch.int64, device=self.device)
        self._call("dmvs_mesh_face_tally_i64", _ptr(verts), N, _ptr(faces), F, _ptr(label), float(scale), float(cap), _ptr(area_q), _ptr(comp_faces),
                   _ptr(comp_area), int(blocks), self.stream())
        return area_q, comp_faces, comp_area

    def mesh_sample(self, verts, faces, area_cum, a0, M, blocks=0):
        """dmvs_mesh_sample_f32 (include/dmvs.h): M samples, one per a0 units of the running area sums area_cum [F] int64 (inclusive), at the
        R2 sequence's coordinates inside their faces.  The caller keeps M a0 <= area_cum[-1].  -> (points [M,3] fp32, face_of [M] int32)"""
        self._mesh_args("mesh_sample", verts, faces)
        self._chk_typed("mesh_sample", (area_cum, torch.int64))
        N, F, M = int(verts.shape[0]), int(faces.shape[0]), int(M)
        if tuple(area_cum.shape) != (F,):
            raise _lib.DmvsError(f"mesh_sample: area_cum must be [F] = [{F}], got {tuple(area_cum.shape)}")
        if not 0 <= M <= 2 ** 31 - 1 or not 1 <= int(a0) < 2 ** 63:
            raise _lib.DmvsError(f"mesh_sample: M = {M} and a0 = {a0}; 0 <= M < 2^31 and 1 <= a0 < 2^63")
        if M > 0 and (N == 0 or F == 0):
            raise _lib.DmvsError(f"mesh_sample: {M} samples of a mesh with {N} vertices and {F} faces")
        points = torch.empty((M, 3), dtype=torch.float32, device=self.device)
        face_of = torch.empty((M,), dtype=torch.int32, device=self.device)
        self._call("dmvs_mesh_sample_f32", _ptr(verts), N, _ptr(faces), F, _ptr(area_cum), int(a0), M, _ptr(points), _ptr(face_of), int(blocks), self.stream())
        return points, face_of

    # ------------------------------------------------------------------ simplifying a mesh (diffmvs_amd/mesh_simplify.py)
    def _cluster_args(self, what, verts, faces, cluster, K, origin):
        """the checks the clustering passes share -> (N, K, the HOST origin)"""
        if faces is not None:
            self._mesh_args(what, verts, faces)
        self._chk_typed(what, (verts, torch.float32), (cluster, torch.int32))
        N = int(verts.shape[0])
        if verts.dim() != 2 or verts.shape[1] != 3 or tuple(cluster.shape) != (N,):
            raise _lib.DmvsError(f"{what}: verts must be [N,3] and cluster [N], got {tuple(verts.shape)} and {tuple(cluster.shape)}")
        if not 0 <= int(K) <= 2 ** 31 - 1:
            raise _lib.DmvsError(f"{what}: {K} clusters; 0 .. 2^31 - 1 are supported")
        return N, int(K), None if origin is None else (C.c_double * 3)(*[float(v) for v in origin])

    def mesh_cluster_verts(self, verts, rgb, cluster, K, origin, cell, blocks=0):
        """dmvs_mesh_cluster_verts_i64 (include/dmvs.h): cluster [N] int32 (outside [0, K): none); origin: three doubles; rgb [N,3] uint8 or
        None.  -> (cnt [K] int32, pos_q [K,3] int64, rgb_sum [K,3] int64 or None)"""
        N, K, o = self._cluster_args("mesh_cluster_verts", verts, None, cluster, K, origin)
        self._chk_typed("mesh_cluster_verts", (rgb, torch.uint8))
        if rgb is not None and tuple(rgb.shape) != (N, 3):
            raise _lib.DmvsError(f"mesh_cluster_verts: rgb must be [N,3] = [{N},3], got {tuple(rgb.shape)}")
        cnt = torch.empty((K,), dtype=torch.int32, device=self.device)
        pos_q = torch.empty((K, 3), dtype=torch.int64, device=self.device)
        rgb_sum = torch.empty((K, 3), dtype=torch.int64, device=self.device) if rgb is not None else None
        self._call("dmvs_mesh_cluster_verts_i64", _ptr(verts), _ptr(rgb), N, _ptr(cluster), K, o, float(cell), _ptr(cnt), _ptr(pos_q), _ptr(rgb_sum),
                   int(blocks), self.stream())
        return cnt, pos_q, rgb_sum

    def mesh_cluster_quadrics(self, verts, faces, cluster, K, origin, cell, scale, cap, blocks=0):
        """dmvs_mesh_cluster_quadrics_i64 (include/dmvs.h): scale: a power of two; cap: the bound of one face's weight.
        -> (quad_q [K,10] int64, state [2] int64 (device): bad faces, flat faces)"""
        N, K, o = self._cluster_args("mesh_cluster_quadrics", verts, faces, cluster, K, origin)
        quad_q = torch.empty((K, 10), dtype=torch.int64, device=self.device)
        state = torch.empty((2,), dtype=torch.int64, device=self.device)
        self._call("dmvs_mesh_cluster_quadrics_i64", _ptr(verts), N, _ptr(faces), int(faces.shape[0]), _ptr(cluster), K, o, float(cell), float(scale),
                   float(cap), _ptr(quad_q), _ptr(state), int(blocks), self.stream())
        return quad_q, state

    def mesh_cluster_place(self, cnt, pos_q, rgb_sum, quad_q, cells, origin, cell, scale, reg, mean=False):
        """dmvs_mesh_cluster_place_f32 (include/dmvs.h): the sums of the two passes above, cells [K,3] int64: the clusters' lattice cells;
        mean: every cluster at the mean of its vertices.  -> (verts [K,3] fp32, rgb [K,3] uint8 or None, state [1] int64 (device): clusters
        that have a quadric and fell back to the mean)"""
        self._chk_typed("mesh_cluster_place", (cnt, torch.int32), (pos_q, torch.int64), (rgb_sum, torch.int64), (quad_q, torch.int64), (cells, torch.int64))
        K = int(cnt.shape[0])
        if tuple(cnt.shape) != (K,) or tuple(pos_q.shape) != (K, 3) or tuple(quad_q.shape) != (K, 10) or tuple(cells.shape) != (K, 3) or (
                rgb_sum is not None and tuple(rgb_sum.shape) != (K, 3)):
            raise _lib.DmvsError(f"mesh_cluster_place: cnt [K], pos_q [K,3], rgb_sum [K,3], quad_q [K,10] and cells [K,3] with K = {K} are expected")
        out = torch.empty((K, 3), dtype=torch.float32, device=self.device)
        out_rgb = torch.empty((K, 3), dtype=torch.uint8, device=self.device) if rgb_sum is not None else None
        state = torch.empty((1,), dtype=torch.int64, device=self.device)
        self._call("dmvs_mesh_cluster_place_f32", K, _ptr(cnt), _ptr(pos_q), _ptr(rgb_sum), _ptr(quad_q), _ptr(cells),
                   (C.c_double * 3)(*[float(v) for v in origin]), float(cell), float(scale), float(reg),
                   _lib.SIMPLIFY_MEAN if mean else _lib.SIMPLIFY_QUADRIC, _ptr(out), _ptr(out_rgb), _ptr(state), self.stream())
        return out, out_rgb, state

    def mesh_cluster_remap(self, verts, faces, cluster, K, new_verts=None, blocks=0):
        """dmvs_mesh_cluster_remap_i32 (include/dmvs.h): new_verts [K,3] fp32 or None (flipped faces are then not counted).
        -> (faces' [F,3] int32: the corners' clusters, the smallest first, (-1, -1, -1) for a bad face; keep [F] uint8; state [3] int64
        (device): degenerate, flipped, bad)"""
        N, K, _ = self._cluster_args("mesh_cluster_remap", verts, faces, cluster, K, None)
        self._chk_typed("mesh_cluster_remap", (new_verts, torch.float32))
        if new_verts is not None and tuple(new_verts.shape) != (K, 3):
            raise _lib.DmvsError(f"mesh_cluster_remap: new_verts must be [K,3] = [{K},3], got {tuple(new_verts.shape)}")
        F = int(faces.shape[0])
        out = torch.empty((F, 3), dtype=torch.int32, device=self.device)
        keep = torch.empty((F,), dtype=torch.uint8, device=self.device)
        state = torch.empty((3,), dtype=torch.int64, device=self.device)
        self._call("dmvs_mesh_cluster_remap_i32", _ptr(verts), N, _ptr(faces), F, _ptr(cluster), K, _ptr(new_verts), _ptr(out), _ptr(keep), _ptr(state),
                   int(blocks), self.stream())
        return out, keep, state


class TsdfVolume:
    """The caller-owned state of dmvs_tsdf_integrate_f32 (include/dmvs.h), made zeroed by Ops.tsdf_volume: dims (nx, ny, nz), origin (HOST,
    three doubles), h, S and Wt [nz,ny,nx] int32, C [nz,ny,nx,4] int32 holding the uint32 colour sums (torch has no arithmetic on uint32;
    they stay below 2^24) or None, and `views`, how many views went in so far."""

    def __init__(self, dims, origin, h, S, Wt, C):
        self.dims, self.origin, self.h, self.S, self.Wt, self.C, self.views = tuple(dims), origin, h, S, Wt, C, 0
