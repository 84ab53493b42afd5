"""Autograd ops of the CostRegNet training path on the hand-written HIP kernels (reference:
models/module.py:80-160 Conv3d / Deconv3d + BatchNorm3d(train) + ReLU, :305-315 the U-Net wiring).

* :class:`Conv3dK3` — ``nn.Conv3d(k=3, p=1, stride 1|2, bias=False)`` / ``nn.ConvTranspose3d(k=3, s=2, p=1, op=1, bias=False)``:
  forward and data gradient on the inference kernels (``cds_conv3d_k3_f32`` / ``cds_deconv3d_k3s2_f32``: the data gradient
  of a stride-2 convolution is the transposed convolution with the same weights and vice versa, a stride-1 convolution's is
  the convolution with flipped, transposed weights), weight gradient on ``cds_conv3d_wgrad_f32``.
* :class:`BnRelu3d` — BatchNorm3d with batch statistics + ReLU + optional residual, fused forward (``cds_bn3d_stats_f32`` ->
  ``cds_bn3d_norm_f32``) and closed-form backward (``cds_bn3d_bwd_reduce_f32`` -> ``cds_bn3d_bwd_norm_f32``); running
  statistics are updated like ``nn.BatchNorm3d`` (momentum 0.1, unbiased variance).

All kernels are fp32; under bf16 autocast the Functions cast their inputs up (the reference trains in fp32).

:func:`conv_arithmetic` (``"f32"`` default, or ``"split_f16"``; process default ``CDS_TRAIN_CONV``) selects the arithmetic of the
CostRegNet convolutions conv0 .. conv11 in all three passes: ``"split_f16"`` runs them on the f16 matrix cores in the split-f16 form
of the inference path (csrc/train3d_sf16.hip), with the operand bounds kept on the device (no host read: the step stays capturable).
The mode is read when :class:`Conv3dK3` runs forward and kept for its backward."""
from __future__ import annotations

import os
import warnings
from typing import Optional

import torch

from . import _lib, _scratch, ops
from ._lib import check
from .model import COSTREG_KERNELS, costreg_unet

Tensor = torch.Tensor


def _dev(t: Tensor) -> int:
    return ops._dev(t, "tensor")


_CONV = {"kind": "f32"}
CONV_KINDS = ("f32", "split_f16")


def set_conv_arithmetic(kind: str) -> None:
    if kind not in CONV_KINDS:
        raise ValueError(f"conv arithmetic {kind!r}: expected 'f32' or 'split_f16'")
    _CONV["kind"] = kind


def get_conv_arithmetic() -> str:
    return _CONV["kind"]


_env_kind = os.environ.get("CDS_TRAIN_CONV", "f32")
if _env_kind in CONV_KINDS:
    set_conv_arithmetic(_env_kind)
else:                                     # the same values as conv_arithmetic(); a bad one must not make the package unimportable
    warnings.warn(f"CDS_TRAIN_CONV={_env_kind!r}: expected 'f32' or 'split_f16'; using 'f32'")


class conv_arithmetic:
    """``with conv_arithmetic("split_f16"): loss = model(...)`` - the mode applies to the forward passes run inside (and to their
    backward passes, wherever those run)."""

    def __init__(self, kind: str):
        if kind not in CONV_KINDS:
            raise ValueError(f"conv arithmetic {kind!r}: expected 'f32' or 'split_f16'")
        self.kind = kind

    def __enter__(self):
        self.prev = _CONV["kind"]
        set_conv_arithmetic(self.kind)
        return self

    def __exit__(self, *exc):
        _CONV["kind"] = self.prev
        return False


def _sf16_eligible(x: Tensor, weight: Tensor, stride: int, transposed: bool) -> bool:
    """The split-f16 kernels take 8..64 channels in multiples of 8 (every CostRegNet layer but prob) and, for the stride-2 pairs, even
    sizes (the data gradient of a stride-2 convolution is the transposed one: 2 D must give back D)."""
    a, b = weight.shape[:2]
    if a % 8 or b % 8 or not (8 <= a <= 64 and 8 <= b <= 64):
        return False
    return not (stride == 2 and not transposed and any(d % 2 for d in x.shape[2:]))


def absmax_bound(x: Tensor, slot: Optional[Tensor] = None) -> Tensor:
    """An upper bound of max |x| in a device slot (one launch; `slot` must hold 0 or a smaller bound): the operand bound of a tensor no
    kernel of the mode produced."""
    if slot is None:
        slot = _scratch.zeros((1,), torch.float32, x.device)
    x = x.contiguous()
    check(_lib.load().cds_absmax_bound_f32(_dev(x), x.numel(), slot.data_ptr(), ops._stream(x)), "cds_absmax_bound_f32")
    return slot


def sf16_pack_conv3d(w: Tensor, mode: int, dgrad: bool):
    """(forward pack, data-gradient pack | None, 1 / s_w [1]) of a 3x3x3 weight in one launch, all on the device (mode as pack_conv3d)."""
    a, b = w.shape[:2]
    w = w.detach().float().contiguous()
    mf, cf = (b, a) if mode == 2 else (a, b)

    def size(m, c):
        return (c // 8) * 28 * 2 * ((m + 15) // 16 * 16) * 8

    f = torch.empty((size(mf, cf),), dtype=torch.float16, device=w.device)
    d = torch.empty((size(cf, mf),), dtype=torch.float16, device=w.device) if dgrad else None
    winv = torch.empty((1,), dtype=torch.float32, device=w.device)
    check(_lib.load().cds_sf16_pack_conv3d_f32(_dev(w), f.data_ptr(), d.data_ptr() if dgrad else None, winv.data_ptr(), a, b, mode,
                                               ops._stream(w)), "cds_sf16_pack_conv3d_f32")
    return f, d, winv


def conv3d_sf16(x: Tensor, pack: Tensor, winv: Tensor, x_bound: Tensor, cout: int, mode: int) -> Tensor:
    """y = conv(x) on the split-f16 kernel; mode 0 / 1: k3 convolution stride 1 / 2, mode 2: transposed k3 s2."""
    B, C, D, H, W = x.shape
    if mode == 0:
        shp = (D, H, W)
    elif mode == 1:
        shp = ((D - 1) // 2 + 1, (H - 1) // 2 + 1, (W - 1) // 2 + 1)
    else:
        shp = (2 * D, 2 * H, 2 * W)
    y = torch.empty((B, cout) + shp, dtype=torch.float32, device=x.device)
    check(_lib.load().cds_conv3d_k3_sf16_f32(_dev(x), pack.data_ptr(), winv.data_ptr(), x_bound.data_ptr(), y.data_ptr(), B, C, cout,
                                             D, H, W, mode, ops._stream(x)), "cds_conv3d_k3_sf16_f32")
    return y


def conv3d_wgrad_sf16(g: Tensor, xin: Tensor, g_bound: Tensor, x_bound: Tensor, stride: int) -> Tensor:
    """conv3d_wgrad on the f16 matrix cores.  Always on the CURRENT stream: the side stream of conv3d_wgrad runs next to ATen kernels,
    and those may use packed-fp32 instructions, which a 16x16x32 f16 MFMA on the same SIMD corrupts (profiles/r06_packed_fp32_hazard.md)."""
    B, Ca, Do, Ho, Wo = g.shape
    Bx, Cb, Di, Hi, Wi = xin.shape
    if Bx != B:
        raise ValueError("conv3d_wgrad_sf16: batch mismatch")
    dw = _scratch.zeros((Ca, Cb, 3, 3, 3), torch.float32, g.device)      # the step's zero arena (no fill launch per layer)
    check(_lib.load().cds_conv3d_wgrad_sf16_f32(_dev(g), _dev(xin), g_bound.data_ptr(), x_bound.data_ptr(), dw.data_ptr(), B, Ca, Cb,
                                                Do, Ho, Wo, Di, Hi, Wi, stride, ops._stream(g)), "cds_conv3d_wgrad_sf16_f32")
    return dw


def conv3d_wgrad(g: Tensor, xin: Tensor, stride: int) -> Tensor:
    """dw[a][b][kz][ky][kx] = sum_{batch, o} g[:, a][o] * xin[:, b][stride * o - 1 + k]  ->  [Ca,Cb,3,3,3]."""
    B, Ca, Do, Ho, Wo = g.shape
    Bx, Cb, Di, Hi, Wi = xin.shape
    if Bx != B:
        raise ValueError("conv3d_wgrad: batch mismatch")
    dw = _scratch.zeros((Ca, Cb, 3, 3, 3), torch.float32, g.device)
    _scratch.audit_note(dw)
    side = _scratch.side_stream(g.device)
    if side is None:
        check(_lib.load().cds_conv3d_wgrad_f32(_dev(g), _dev(xin), dw.data_ptr(), B, Ca, Cb, Do, Ho, Wo, Di, Hi, Wi, stride,
                                               ops._stream(g)), "cds_conv3d_wgrad_f32")
        return dw
    with torch.cuda.stream(side):                                # a leaf of the backward pass: overlaps with the data-gradient chain
        check(_lib.load().cds_conv3d_wgrad_f32(_dev(g), _dev(xin), dw.data_ptr(), B, Ca, Cb, Do, Ho, Wo, Di, Hi, Wi, stride,
                                               side.cuda_stream), "cds_conv3d_wgrad_f32")
    g.record_stream(side)
    xin.record_stream(side)
    return dw


def _per_item(fn, x: Tensor) -> Tensor:
    """fn on every batch item (the inference kernels take one item per call); a batch of one is not copied again."""
    if x.shape[0] == 1:
        return fn(x[0]).unsqueeze(0)
    return torch.stack([fn(x[b]) for b in range(x.shape[0])])


def pack_conv3d(w: Tensor, mode: int, dgrad: bool):
    """(forward layout, data-gradient layout | None) of a 3x3x3 weight in one launch (cds_pack_conv3d_f32; mode 0 / 1: Conv3d stride
    1 / 2, mode 2: ConvTranspose3d)."""
    a, b = w.shape[:2]
    w = w.detach().float().contiguous()
    cin, cout = (a, b) if mode == 2 else (b, a)
    f = torch.empty((cin, 27, cout), dtype=torch.float32, device=w.device)
    d = torch.empty((cout, 27, cin), dtype=torch.float32, device=w.device) if dgrad else None
    check(_lib.load().cds_pack_conv3d_f32(_dev(w), f.data_ptr(), d.data_ptr() if dgrad else None, a, b, mode, ops._stream(w)),
          "cds_pack_conv3d_f32")
    return f, d


class Conv3dK3(torch.autograd.Function):
    """x [B,Cin,D,H,W], weight (Conv3d: [Cout,Cin,3,3,3]; ConvTranspose3d: [Cin,Cout,3,3,3]) -> y."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, x, weight, stride: int, transposed: bool, x_bound: Optional[Tensor] = None, dy_bound: Optional[Tensor] = None):
        """x_bound: a device upper bound of max |x| (split-f16 mode; None = measured here); dy_bound: the slot the producer of this
        layer's output gradient fills in the backward (None = measured there)."""
        x = x.contiguous()
        ctx.save_for_backward(x, weight)
        ctx.stride, ctx.transposed = stride, transposed
        ctx.sf16 = get_conv_arithmetic() == "split_f16" and _sf16_eligible(x, weight, stride, transposed)
        if ctx.sf16:
            mode = 2 if transposed else (0 if stride == 1 else 1)
            if x_bound is None:
                x_bound = absmax_bound(x)
            wpk, ctx.dgrad_pack, ctx.w_inv = sf16_pack_conv3d(weight, mode, ctx.needs_input_grad[0])
            ctx.x_bound, ctx.dy_bound = x_bound, dy_bound
            return conv3d_sf16(x, wpk, ctx.w_inv, x_bound, weight.shape[1] if transposed else weight.shape[0], mode)
        wpk, ctx.dgrad_pack = pack_conv3d(weight, 2 if transposed else (0 if stride == 1 else 1), ctx.needs_input_grad[0])
        if transposed:
            return _per_item(lambda xb: ops.deconv3d_k3s2(xb, wpk, None, relu=False), x)
        return _per_item(lambda xb: ops.conv3d_k3(xb, wpk, None, stride=stride, relu=False), x)

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous().float()
        w = weight.detach().float()
        B = x.shape[0]
        dx = dw = None
        if ctx.sf16:
            return Conv3dK3._backward_sf16(ctx, x, w, dy) + (None, None, None, None)
        if ctx.transposed:                                   # y = convT(x, w[Cin,Cout]):  dx = conv_s2(dy, w as [Cout'=Cin][Cin'=Cout])
            cin, cout = w.shape[:2]
            if ctx.needs_input_grad[0]:
                dx = _per_item(lambda gb: ops.conv3d_k3(gb, ctx.dgrad_pack, None, stride=2, relu=False), dy)
            if ctx.needs_input_grad[1]:
                dw = conv3d_wgrad(x, dy, 2)                  # [Cin,Cout,3,3,3]
        else:
            cout, cin = w.shape[:2]
            if ctx.needs_input_grad[0]:
                if ctx.stride == 1:                          # dx = conv(dy, flipped taps, channels swapped)
                    dx = _per_item(lambda gb: ops.conv3d_k3(gb, ctx.dgrad_pack, None, relu=False), dy)
                else:                                        # dx = convT(dy, w)
                    dx = _per_item(lambda gb: ops.deconv3d_k3s2(gb, ctx.dgrad_pack, None, relu=False), dy)
            if ctx.needs_input_grad[1]:
                dw = conv3d_wgrad(dy, x, ctx.stride)         # [Cout,Cin,3,3,3]
        return dx, dw, None, None, None, None

    @staticmethod
    def _backward_sf16(ctx, x, w, dy):
        dyb = ctx.dy_bound if ctx.dy_bound is not None else absmax_bound(dy)
        dx = dw = None
        a, b = w.shape[:2]
        if ctx.transposed:                                   # dx = conv_s2(dy), dw from (g = x, xin = dy)
            if ctx.needs_input_grad[0]:
                dx = conv3d_sf16(dy, ctx.dgrad_pack, ctx.w_inv, dyb, a, 1)
            if ctx.needs_input_grad[1]:
                dw = conv3d_wgrad_sf16(x, dy, ctx.x_bound, dyb, 2)
        else:
            if ctx.needs_input_grad[0]:                      # stride 1: flipped, transposed taps; stride 2: the transposed convolution
                dx = conv3d_sf16(dy, ctx.dgrad_pack, ctx.w_inv, dyb, b, 0 if ctx.stride == 1 else 2)
            if ctx.needs_input_grad[1]:
                dw = conv3d_wgrad_sf16(dy, x, dyb, ctx.x_bound, ctx.stride)
        return dx, dw


class BnRelu3d(torch.autograd.Function):
    """out = [skip +] relu?(batchnorm_train(y; gamma, beta)).  running_mean / running_var are updated in place."""

    @staticmethod
    @torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
    def forward(ctx, y, gamma, beta, skip, running_mean, running_var, momentum: float, eps: float, relu: bool,
                out_bound: Optional[Tensor] = None, dy_bound: Optional[Tensor] = None):
        """out_bound / dy_bound: zeroed device slots raised to max |out| here / max |dy| in the backward (split-f16 mode), or None."""
        y = y.contiguous()
        B, C = y.shape[:2]
        V = y[0, 0].numel()
        n = B * V
        lib = _lib.load()
        sums = _scratch.zeros((C, 2), torch.float64, y.device)
        check(lib.cds_bn3d_stats_f32(_dev(y), sums.data_ptr(), B, C, V, ops._stream(y)), "cds_bn3d_stats_f32")
        # statistics pass, then ONE launch for the per-channel step (fp64: scale / shift, the saved mean / invstd, the
        # running-statistics update) + normalisation + ReLU + residual
        ss = torch.empty((2, C), dtype=torch.float32, device=y.device)
        mi = torch.empty((2, C), dtype=torch.float64, device=y.device)
        scale, shift, mean, invstd = ss[0], ss[1], mi[0], mi[1]
        g32, b32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
        track = running_mean is not None
        out = torch.empty_like(y)
        skip_c = skip.contiguous() if skip is not None else None
        args = (_dev(y), sums.data_ptr(), _dev(g32), _dev(b32), float(n), float(eps), float(momentum),
                _dev(running_mean) if track else None, _dev(running_var) if track else None,
                _dev(skip_c) if skip_c is not None else None, out.data_ptr(), scale.data_ptr(), shift.data_ptr(),
                mean.data_ptr(), invstd.data_ptr(), B, C, V, 1 if relu else 0)
        if out_bound is not None:
            check(lib.cds_bn3d_norm_bound_f32(*args, out_bound.data_ptr(), ops._stream(y)), "cds_bn3d_norm_bound_f32")
        else:
            check(lib.cds_bn3d_norm_f32(*args, ops._stream(y)), "cds_bn3d_norm_f32")
        ctx.save_for_backward(y, scale, shift, mean, invstd, gamma)
        ctx.dy_bound = dy_bound
        ctx.relu, ctx.has_skip, ctx.n = relu, skip is not None, n
        return out

    @staticmethod
    @torch.amp.custom_bwd(device_type="cuda")
    def backward(ctx, dout):
        y, scale, shift, mean, invstd, gamma = ctx.saved_tensors
        dout = dout.contiguous().float()
        B, C = y.shape[:2]
        V = y[0, 0].numel()
        n = ctx.n
        lib = _lib.load()
        sums = _scratch.zeros((C, 2), torch.float64, y.device)
        check(lib.cds_bn3d_bwd_reduce_f32(_dev(dout), _dev(y), scale.data_ptr(), shift.data_ptr(), sums.data_ptr(), B, C, V,
                                          1 if ctx.relu else 0, ops._stream(y)), "cds_bn3d_bwd_reduce_f32")
        gb = torch.empty((2, C), dtype=torch.float32, device=y.device)
        dgamma, dbeta = gb[0], gb[1]
        dy = torch.empty_like(y)
        args = (_dev(dout), _dev(y), scale.data_ptr(), shift.data_ptr(), sums.data_ptr(), mean.data_ptr(), invstd.data_ptr(), float(n),
                dy.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), B, C, V, 1 if ctx.relu else 0)
        if ctx.dy_bound is not None:
            check(lib.cds_bn3d_bwd_norm_bound_f32(*args, ctx.dy_bound.data_ptr(), ops._stream(y)), "cds_bn3d_bwd_norm_bound_f32")
        else:
            check(lib.cds_bn3d_bwd_norm_f32(*args, ops._stream(y)), "cds_bn3d_bwd_norm_f32")
        return (dy, dgamma.to(gamma.dtype), dbeta.to(gamma.dtype), dout if ctx.has_skip else None,
                None, None, None, None, None, None, None)


def bn_momentum_and_count(bn) -> float:
    """The momentum of this training-mode call of a BatchNorm module, counting the call in num_batches_tracked (nn.BatchNorm semantics:
    momentum None = cumulative moving average)."""
    momentum = bn.momentum
    if bn.num_batches_tracked is not None:
        if momentum is None:
            bn.num_batches_tracked += 1
            momentum = 1.0 / float(bn.num_batches_tracked)
        else:
            _scratch.bump(bn.num_batches_tracked, 1)
    return 0.0 if momentum is None else float(momentum)


def conv_bn_relu3d(unit, x: Tensor, skip: Optional[Tensor] = None, bounds=None) -> Tensor:
    """One ConvBn3d holder (model.py) in its module mode: training -> batch statistics (and running-stat update),
    eval -> running statistics; Conv3d / ConvTranspose3d + BatchNorm3d + ReLU (+ skip), all on the HIP kernels.
    bounds (split-f16 mode): (x_bound, out slot, dy slot) - the device bound of x, and zeroed slots for the bound of the output (the
    BatchNorm pass raises it) and of the convolution's output gradient (the BatchNorm backward raises it)."""
    x_bound, out_slot, dy_slot = bounds if bounds is not None else (None, None, None)
    bn = unit.bn
    if not bn.training:
        out_slot = dy_slot = None
    y = Conv3dK3.apply(x, unit.conv.weight, unit.stride, unit.transposed, x_bound, dy_slot)
    if bn.training:
        momentum = bn_momentum_and_count(bn)
        return BnRelu3d.apply(y, bn.weight, bn.bias, skip, bn.running_mean, bn.running_var, float(momentum), bn.eps, True, out_slot,
                              dy_slot)
    out = torch.relu(torch.nn.functional.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps))
    return out if skip is None else skip + out


class _TrainLayers:
    """costreg_unet on the autograd ops, batched planar volumes [B,C,D,h,w].  Split-f16 mode keeps one zeroed slot array per call:
    [0] the cost volume's bound (one absmax launch), then per layer (output bound, output-gradient bound); the BatchNorm passes raise
    them, the convolutions read them."""

    def __init__(self, cr, x: Tensor):
        self.cr = cr
        self.slots = None
        if get_conv_arithmetic() == "split_f16":
            self.slots = _scratch.zeros((1 + 2 * len(COSTREG_KERNELS),), torch.float32, x.device)
            self.in_bound, self.used = self.slots[0:1], 1
            absmax_bound(x, self.in_bound)

    def _unit(self, name: str, x: Tensor, skip: Optional[Tensor] = None) -> Tensor:
        unit = getattr(self.cr, name)                              # the holder knows its own stride and direction
        if self.slots is None:
            return conv_bn_relu3d(unit, x, skip)
        out_slot, dy_slot = self.slots[self.used:self.used + 1], self.slots[self.used + 1:self.used + 2]
        self.used += 2
        y = conv_bn_relu3d(unit, x, skip, (self.in_bound, out_slot, dy_slot))
        self.in_bound = out_slot if unit.bn.training else None     # a BatchNorm in eval mode publishes no bound: the next layer measures
        return y

    def conv(self, name: str, x: Tensor, stride: int) -> Tensor:
        return self._unit(name, x)

    deconv = _unit

    def tail(self, x: Tensor, skip: Tensor, refresh) -> Tensor:
        return Conv3dK3.apply(self._unit("conv11", x, skip), self.cr.prob.weight, 1, False)


def cost_regularization(cr, x: Tensor) -> Tensor:
    """models/module.py:305-315 on the HIP training ops.  x [B,C,D,h,w] -> [B,1,D,h,w]."""
    if x.shape[2] % 8 or x.shape[3] % 8 or x.shape[4] % 8:
        raise ValueError(f"CostRegNet needs D,h,w divisible by 8, got {tuple(x.shape[2:])}")
    return costreg_unet(_TrainLayers(cr, x), x)
