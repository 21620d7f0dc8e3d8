"""torch-tensor front end of the HIP kernels (include/dlmcq.h).

Everything here is plumbing: shape bookkeeping, output allocation and the current-stream handle.
The arithmetic happens in libdlmcq.so; tensors that are not on the GPU are refused (no fallback).
Two wrappers of pure data movement, patch_rows_quant and assemble_tokens, restate in torch ops the inputs their kernels do not read in
place (a channels_last image batch, misaligned views): the graph's own ops, the same values.
"""
import collections
import ctypes
import math

import torch

from ... import _native as N
from ..._native import (CODES_I8, CODES_NONE, CODES_P4, FORM_EMULATE, FORM_QBASE, FORM_ROOTQ_ACT,
                        FORM_SYMMETRIC, FORM_ZEROPOINT, MINMAX_ABSMAX, MINMAX_MINMAX, MINMAX_NEGMIN,
                        Y_CODES, Y_DEQUANT)

__all__ = ["fake_quant", "dequant_codes", "dequant", "minmax", "observe_qparams", "qparams_from_minmax",
           "span_scale", "lsq_init", "l2norm_step", "adaround_weight", "adaround_weight_backward", "quantize_weight_krsc", "conv2d_i8", "global_avgpool", "avgpool_quant", "gate_quant", "swish_quant", "hardswish_quant", "squeeze_gate", "squeeze_gate_torch", "squeeze_gate_supported", "gelu_quant", "layernorm_quant", "LAYERNORM_MAX_C", "patch_rows_quant", "patch_rows_view", "patch_rows_torch", "PATCH_MAX_STRIP", "assemble_tokens", "tokens_view", "attention_quant", "attention_views", "ATTENTION_DIMS", "conv2d_i8_gap", "gap_head_supported", "gap_head_profitable", "pack_int4", "unpack_int4", "fake_quant_backward", "Segment", "FqMultiPlan", "fake_quant_multi", "fake_quant_multi_backward", "rootq_weight", "geometry", "channel_shape",
           "PROFILE"]


class _Profile:
    """Optional HIP-event timing of the fake-quant launches (bench.py turns it on).  Events are
    recorded on the stream the kernel is launched on, which is torch's current stream."""

    def __init__(self):
        self.enabled = False
        self.records = []  # (tag, algorithmic_bytes, start_event, stop_event, integer operations = 2 x MACs or 0)

    def reset(self):
        self.records = []

    def launch(self, tag, nbytes, fn, ops=0):
        if not self.enabled:
            return fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        self.records.append((tag, nbytes, a, b, ops))
        return r


PROFILE = _Profile()


def _f32c(t, like):
    """A contiguous fp32 tensor on `like`'s device (scale / offset operands)."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        return torch.full((1,), float(t), dtype=torch.float32, device=like.device)
    if t.dtype != torch.float32 or t.device != like.device:
        t = t.to(device=like.device, dtype=torch.float32)
    return t.contiguous()


def geometry(x, scale, ch_axis=None):
    """(outer, channels, inner) of contiguous `x` for a scale of shape [], [1] or [1,..,C,..,1]."""
    n = x.numel()
    if scale.numel() == 1:
        return 1, 1, n
    if ch_axis is None:
        if scale.dim() != x.dim():
            raise ValueError(f"per-channel scale {tuple(scale.shape)} must have the rank of x {tuple(x.shape)}")
        axes = [i for i, s in enumerate(scale.shape) if s != 1]
        if len(axes) != 1:
            raise ValueError(f"scale {tuple(scale.shape)} is not a single-axis broadcast")
        ch_axis = axes[0]
    c = x.shape[ch_axis]
    if scale.numel() != c:
        raise ValueError(f"scale has {scale.numel()} entries, axis {ch_axis} of x has {c}")
    outer = math.prod(x.shape[:ch_axis])
    inner = math.prod(x.shape[ch_axis + 1:])
    return outer, c, inner


def channel_shape(x, ch_axis):
    shape = [1] * x.dim()
    shape[ch_axis] = x.shape[ch_axis]
    return shape


def _dense(x):
    """x as it lies in memory when that is one dense block (NCHW-contiguous or channels_last): per-tensor
    kernels are layout-blind, so a channels_last activation needs no copy."""
    if x.is_contiguous():
        return x
    if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last):
        return x
    return x.contiguous()


def fake_quant(x, scale, offset, lo, hi, form, g=0.0, y_kind=Y_DEQUANT, codes=None, want_y=True,
               out=None, ch_axis=None):
    """One-pass fake-quantisation.  Returns y, or (y, codes) when `codes` is "i8" / "p4"
    (y is None when want_y is False)."""
    N.require_gpu(x)
    per_tensor = (not isinstance(scale, torch.Tensor)) or scale.numel() == 1
    x = _dense(x) if per_tensor else x.contiguous()
    if x.dtype != torch.float32:
        raise TypeError(f"fake_quant computes in fp32; got {x.dtype}")
    scale, offset = _f32c(scale, x), _f32c(offset, x)
    outer, ch, inner = geometry(x, scale, ch_axis)
    if offset is not None and offset.numel() != scale.numel():
        if offset.numel() == 1:
            offset = offset.reshape(1).expand(scale.numel()).contiguous()
        else:
            raise ValueError("offset must have one entry per scale entry")
    y = None
    if want_y:
        y = out if out is not None else torch.empty_like(x)   # preserves x's memory format
        if not (y.dtype == torch.float32 and y.shape == x.shape and y.stride() == x.stride()):
            raise ValueError("out must be an fp32 tensor with x's shape and memory layout")
    cbuf, ckind = None, CODES_NONE
    n = x.numel()
    if codes == "i8":
        cbuf = torch.empty_like(x, dtype=torch.int8 if lo < 0 else torch.uint8)   # same memory layout as x
        ckind = CODES_I8
    elif codes == "p4":
        cbuf = torch.empty((n + 1) // 2, dtype=torch.uint8, device=x.device)
        ckind = CODES_P4
    elif codes is not None:
        raise ValueError("codes must be None, 'i8' or 'p4'")
    nbytes = n * (4 + (4 if want_y else 0)) + (n if ckind == CODES_I8 else (n + 1) // 2 if ckind == CODES_P4 else 0)
    PROFILE.launch(
        "fq_channel" if ch > 1 else "fq_tensor", nbytes,
        lambda: N.check(N.lib.dlmcq_fake_quant_f32(
            N.ptr(x), N.ptr(y), N.ptr(cbuf), N.ptr(scale), N.ptr(offset), outer, ch, inner, int(lo), int(hi),
            int(form), int(y_kind), ckind, float(g), N.stream_ptr())))
    return y if cbuf is None else (y, cbuf)


def dequant_codes(codes, shape, scale, offset, form, kind, signed, g=0.0, ch_axis=None):
    """Integer codes (int8/uint8 tensor of `shape`, or packed nibbles) -> fp32."""
    N.require_gpu(codes)
    y = torch.empty(shape, dtype=torch.float32, device=codes.device)
    scale, offset = _f32c(scale, y), _f32c(offset, y)
    outer, ch, inner = geometry(y, scale, ch_axis)
    ckind = CODES_I8 if kind == "i8" else CODES_P4
    N.check(N.lib.dlmcq_dequant_codes_f32(N.ptr(codes.contiguous()), N.ptr(y), N.ptr(scale), N.ptr(offset), outer, ch,
                                          inner, int(form), ckind, int(bool(signed)), float(g), N.stream_ptr()))
    return y


def dequant(q, scale, offset, ch_axis=None):
    """Reference `dequantize` on fp32 codes: q*s + o."""
    N.require_gpu(q)
    q = q.contiguous()
    y = torch.empty_like(q)
    scale, offset = _f32c(scale, q), _f32c(offset, q)
    outer, ch, inner = geometry(q, scale, ch_axis)
    if offset is not None and offset.numel() != scale.numel():
        offset = offset.reshape(1).expand(scale.numel()).contiguous()
    N.check(N.lib.dlmcq_dequant_f32(N.ptr(q), N.ptr(y), N.ptr(scale), N.ptr(offset), outer, ch, inner, N.stream_ptr()))
    return y


def _obs_geometry(x, ch_axis):
    if ch_axis is None:
        return 1, 1, x.numel()
    return math.prod(x.shape[:ch_axis]), x.shape[ch_axis], math.prod(x.shape[ch_axis + 1:])


def _scratch(nbytes, device):
    return torch.empty(max(int(nbytes), 4) // 4 + 1, dtype=torch.float32, device=device)


def minmax(x, ch_axis=None, mode=MINMAX_MINMAX):
    """(max, min) of x - per tensor (0-dim results) or per channel ([C] results) - in one read.
    mode ABSMAX returns (max|x|, None); NEGMIN returns (max, -min)."""
    N.require_gpu(x)
    x = _dense(x) if ch_axis is None else x.contiguous()     # (min / max of a whole tensor do not depend on the order it is read in)
    outer, ch, inner = _obs_geometry(x, ch_axis)
    vmax = torch.empty(ch, dtype=torch.float32, device=x.device)
    vmin = torch.empty(ch, dtype=torch.float32, device=x.device) if mode != MINMAX_ABSMAX else None
    nb = N.lib.dlmcq_minmax_scratch_bytes(outer, ch, inner)
    sc = _scratch(nb, x.device)
    PROFILE.launch("observer", x.numel() * 4, lambda: N.check(N.lib.dlmcq_minmax_f32(
        N.ptr(x), N.ptr(vmax), N.ptr(vmin), outer, ch, inner, int(mode), N.ptr(sc), sc.numel() * 4, N.stream_ptr())))
    if ch_axis is None:
        return vmax.reshape(()), (None if vmin is None else vmin.reshape(()))
    return vmax, vmin


def minmax_hint(x):
    """The observer partials a producing launch left on tensor `x` (conv2d_i8(..., observe=True)), if `x` is still what that launch wrote."""
    h = getattr(x, "_dlmcq_mm", None)
    return (h[0], h[1]) if h is not None and h[2] == x._version else None


def minmax_from_partials(partials, count, mode=MINMAX_MINMAX):
    """(max, min) - 0-dim tensors - of the tensor whose per-workgroup observer partials a producing launch wrote (three planes of
    `count` floats: dlmcq_conv2d_i8_nhwc_fused_observed); dlmcq_minmax_finalize_f32.  mode as in `minmax`."""
    vmax = torch.empty(1, dtype=torch.float32, device=partials.device)
    vmin = torch.empty(1, dtype=torch.float32, device=partials.device) if mode != MINMAX_ABSMAX else None
    PROFILE.launch("observer", count * 12, lambda: N.check(N.lib.dlmcq_minmax_finalize_f32(
        N.ptr(partials), int(count), int(count), N.ptr(vmax), N.ptr(vmin), int(mode), N.stream_ptr())))
    return vmax.reshape(()), (None if vmin is None else vmin.reshape(()))


def observe_qparams(x, n_bits, signed, ch_axis=None, allow_offset=True, scale_eps=0.0):
    """Observer + the scale/offset arithmetic of ops.py:20-34 / :121-140, entirely on device.
    Returns (scale, offset): 0-dim tensors per tensor, [1,..,C,..,1] per channel."""
    N.require_gpu(x)
    # per tensor the observer is layout-blind: a channels_last activation (the int8 path's layout) is read in place - round 2
    # copied it to NCHW first, 26 of the 55 ms of a calibrating ResNet-50 forward at batch 512 (tools/first_batch_probe.py)
    x = _dense(x) if ch_axis is None else x.contiguous()
    outer, ch, inner = _obs_geometry(x, ch_axis)
    scale = torch.empty(ch, dtype=torch.float32, device=x.device)
    offset = torch.empty(ch, dtype=torch.float32, device=x.device)
    nb = N.lib.dlmcq_minmax_scratch_bytes(outer, ch, inner)
    sc = _scratch(nb, x.device)
    PROFILE.launch("observer", x.numel() * 4, lambda: N.check(N.lib.dlmcq_observe_qparams_f32(
        N.ptr(x), N.ptr(scale), N.ptr(offset), outer, ch, inner, int(n_bits), int(bool(signed)),
        int(bool(allow_offset)), float(scale_eps), N.ptr(sc), sc.numel() * 4, N.stream_ptr())))
    if ch_axis is None:
        return scale.reshape(()), offset.reshape(())
    shape = channel_shape(x, ch_axis)
    return scale.reshape(shape), offset.reshape(shape)


def qparams_from_minmax(vmax, vmin, n_bits, signed, allow_offset=True, min_is_negated=False, scale_eps=0.0):
    """The arithmetic tail alone (after a cross-rank all-reduce of [max | -min])."""
    N.require_gpu(vmax)
    vmax = vmax.contiguous()
    vmin = None if vmin is None else vmin.contiguous()
    ch = vmax.numel()
    scale = torch.empty(ch, dtype=torch.float32, device=vmax.device)
    offset = torch.empty(ch, dtype=torch.float32, device=vmax.device)
    N.check(N.lib.dlmcq_qparams_from_minmax(N.ptr(vmax), N.ptr(vmin), N.ptr(scale), N.ptr(offset), ch, int(n_bits),
                                            int(bool(signed)), int(bool(allow_offset)), int(bool(min_is_negated)),
                                            float(scale_eps), N.stream_ptr()))
    return scale, offset


def span_scale(vmax, neg_vmin, span):
    """(max - min) / span with a true IEEE division, from the [max | -min] pair of `minmax(NEGMIN)`."""
    N.require_gpu(vmax, neg_vmin)
    vmax, neg_vmin = vmax.contiguous(), neg_vmin.contiguous()
    scale = torch.empty(vmax.numel(), dtype=torch.float32, device=vmax.device)
    N.check(N.lib.dlmcq_span_scale_f32(N.ptr(vmax), N.ptr(neg_vmin), N.ptr(scale), vmax.numel(), float(span), 1,
                                       N.stream_ptr()))
    return scale


def lsq_init(x, qmax):
    """LSQ's first-call scale 2 * mean|x| / sqrt(Qp) (modules/base.py:84-85,118-121) as one read of `x` on the device
    (dlmcq_lsq_init_f32: deterministic double-precision sum, the reference's fp32 chain and a true division).  Returns [1] fp32."""
    import math
    N.require_gpu(x)
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.float()
    if not (x.is_contiguous() or (x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last))):
        x = x.contiguous()       # (an element-order-free reduction: any dense layout is read in place)
    scale = torch.empty(1, dtype=torch.float32, device=x.device)
    nb = N.lib.dlmcq_lsq_init_scratch_bytes(x.numel())
    scr = _scratch(nb, x.device)
    N.check(N.lib.dlmcq_lsq_init_f32(N.ptr(x), N.ptr(scale), x.numel(), float(torch.tensor(math.sqrt(qmax), dtype=torch.float32)),
                                     N.ptr(scr), scr.numel() * 4, N.stream_ptr()))
    return scale


def l2norm_step(x, scale, offset, lo, hi, ch_axis=None):
    """One fused iteration of the l2norm refinement: returns the new scale, shaped like `scale`."""
    N.require_gpu(x)
    x = x.detach().contiguous()
    sc, off = _f32c(scale.detach(), x), _f32c(offset, x)
    outer, ch, inner = geometry(x, sc, ch_axis)
    if off is not None and off.numel() != sc.numel():
        off = off.reshape(1).expand(sc.numel()).contiguous()
    new = torch.empty(ch, dtype=torch.float32, device=x.device)
    nb = N.lib.dlmcq_l2norm_scratch_bytes(outer, ch, inner)
    scr = _scratch(nb, x.device)
    N.check(N.lib.dlmcq_l2norm_step_f32(N.ptr(x), N.ptr(sc), N.ptr(off), N.ptr(new), outer, ch, inner, int(lo), int(hi),
                                        N.ptr(scr), scr.numel() * 4, N.stream_ptr()))
    return new.reshape(scale.shape)


def l2norm_refine(x, scale, offset, lo, hi, ch_axis=None, eps=1e-5, batch=8):
    """The whole l2norm refinement loop (ops.py:71-83 / :198-215) on the device: `batch` iterations per host check, each
    of them a no-op once the convergence flag is set.  Returns the converged scale, shaped like `scale`."""
    N.require_gpu(x)
    x = x.detach().contiguous()
    sc0 = _f32c(scale.detach(), x)
    outer, ch, inner = geometry(x, sc0, ch_axis)
    sc = sc0.reshape(-1).clone()
    off = _f32c(offset, x)
    if off is not None and off.numel() != sc.numel():
        off = off.reshape(1).expand(sc.numel()).contiguous()
    state = torch.zeros(3, dtype=torch.float32, device=x.device)
    nb = N.lib.dlmcq_l2norm_scratch_bytes(outer, ch, inner)
    scr = _scratch(nb, x.device)
    while True:
        N.check(N.lib.dlmcq_l2norm_iterate_f32(N.ptr(x), N.ptr(sc), N.ptr(off), N.ptr(state), outer, ch, inner, int(lo), int(hi),
                                               int(batch), float(eps), N.ptr(scr), scr.numel() * 4, N.stream_ptr()))
        if float(state[0]) != 0.0:          # one sync per `batch` iterations
            break
    return sc.reshape(scale.shape)


class OutputAwareState:
    """Device-side state of an output-aware refinement (l2norm_output / l2norm_output_channel)."""

    def __init__(self, scale):
        flat = scale.detach().to(torch.float32).reshape(-1)
        self.scale = flat.clone()
        self.best = torch.cat([flat, flat]).contiguous()           # [best | staging]
        self.state = torch.tensor([0.0, 0.0, float("inf")], dtype=torch.float32, device=scale.device)

    def done(self):
        return float(self.state[0]) != 0.0

    def iterations(self):
        return int(self.state[1])


def l2out_update(out, out_q, st, per_channel, eps=1e-5):
    """One fused output-aware step on (out, out_q) [batch, channels, ...]: sums, new scale, best-scale bookkeeping and the
    convergence flag, all on the device (dlmcq_l2out_update_f32)."""
    N.require_gpu(out, out_q)
    out, out_q = out.detach().contiguous(), out_q.detach().contiguous()
    b, c = out.shape[0], out.shape[1]
    inner = out.numel() // (b * c)
    mse_div = float(out.numel() // c)                    # l2_loss: sum over axis 1, mean over the rest
    nb = N.lib.dlmcq_l2out_scratch_bytes(b, c, inner)
    scr = _scratch(nb, out.device)
    N.check(N.lib.dlmcq_l2out_update_f32(N.ptr(out), N.ptr(out_q), N.ptr(st.scale), N.ptr(st.best), N.ptr(st.state), b, c, inner,
                                         int(bool(per_channel)), mse_div, float(eps), N.ptr(scr), scr.numel() * 4, N.stream_ptr()))


def l2loss_tensor(x, vmax, vmin, n_bits):
    """quantize_l2loss_tensor's 80-candidate search in one read of x (dlmcq_l2loss_tensor_f32) -> (scale, zero point)."""
    N.require_gpu(x)
    x = x.detach().contiguous()
    shape1 = x.shape[1] if x.dim() >= 2 else x.numel()
    loss_div = float(x.numel() // shape1)
    scale = torch.empty(1, dtype=torch.float32, device=x.device)
    offset = torch.empty(1, dtype=torch.float32, device=x.device)
    nb = N.lib.dlmcq_l2loss_scratch_bytes(x.numel())
    scr = _scratch(nb, x.device)
    N.check(N.lib.dlmcq_l2loss_tensor_f32(N.ptr(x), N.ptr(_f32c(vmax, x).reshape(-1)), N.ptr(None if vmin is None else _f32c(vmin, x).reshape(-1)),
                                          N.ptr(scale), N.ptr(offset), x.numel(), int(n_bits), loss_div, N.ptr(scr), scr.numel() * 4,
                                          N.stream_ptr()))
    return scale.reshape(()), offset.reshape(())


def l2loss_rows(rows, scale, offset, n_bits):
    """quantize_l2loss_channel's per-row search (dlmcq_l2loss_rows_f32).  rows [C, L]; scale / offset [C, 1] from the
    min/max observer; returns the searched (scale, zero point), same shapes."""
    N.require_gpu(rows)
    rows = rows.detach().contiguous()
    sc = _f32c(scale.detach(), rows).reshape(-1).clone()
    off = _f32c(offset.detach(), rows).reshape(-1).clone()
    N.check(N.lib.dlmcq_l2loss_rows_f32(N.ptr(rows), N.ptr(sc), N.ptr(off), rows.shape[0], rows.shape[1], int(n_bits), N.stream_ptr()))
    return sc.reshape(scale.shape), off.reshape(offset.shape)


def adaround_weight(w, alpha, scale, lo, hi, training):
    """Fused AdaRound weight forward; `scale` is the per-output-channel [K,1,..] scale."""
    N.require_gpu(w, alpha)
    w, alpha = w.detach().contiguous(), alpha.detach().contiguous()
    sc = _f32c(scale.detach(), w).reshape(-1)
    K_, inner = w.shape[0], w.numel() // max(w.shape[0], 1)
    y = torch.empty_like(w)
    N.check(N.lib.dlmcq_adaround_weight_f32(N.ptr(w), N.ptr(alpha), N.ptr(sc), N.ptr(y), K_, inner, int(lo), int(hi),
                                            int(bool(training)), N.stream_ptr()))
    return y


def adaround_weight_backward(w, alpha, scale, gy, lo, hi, want_alpha=True, want_scale=True):
    """(g_alpha like w, g_scale shaped like `scale`) of the training-mode AdaRound forward."""
    N.require_gpu(w, alpha, gy)
    w, alpha, gy = w.detach().contiguous(), alpha.detach().contiguous(), gy.contiguous()
    sc = _f32c(scale.detach(), w).reshape(-1)
    K_, inner = w.shape[0], w.numel() // max(w.shape[0], 1)
    ga = torch.empty_like(w) if want_alpha else None
    gs = torch.empty(K_, dtype=torch.float32, device=w.device) if want_scale else None
    N.check(N.lib.dlmcq_adaround_weight_bwd_f32(N.ptr(w), N.ptr(alpha), N.ptr(sc), N.ptr(gy), N.ptr(ga), N.ptr(gs), K_, inner,
                                                int(lo), int(hi), N.stream_ptr()))
    return ga, (None if gs is None else gs.reshape(scale.shape))


def quantize_weight_krsc(w, scale, lo, hi):
    """fp32 KCRS (or [K, C]) weights -> (int8 codes in KRSC order, int32 per-output-channel code sums)."""
    N.require_gpu(w)
    w = w.detach().contiguous()
    K = w.shape[0]
    C = w.shape[1]
    R, S = (w.shape[2], w.shape[3]) if w.dim() == 4 else (1, 1)
    scale = _f32c(scale.detach(), w).reshape(-1)
    if scale.numel() == 1:
        scale = scale.expand(K).contiguous()
    wq = torch.empty((K, R, S, C), dtype=torch.int8, device=w.device)
    wsum = torch.empty(K, dtype=torch.int32, device=w.device)
    N.check(N.lib.dlmcq_quantize_weight_krsc_i8(N.ptr(w), N.ptr(wq), N.ptr(wsum), N.ptr(scale), K, C, R, S, int(lo), int(hi),
                                                N.stream_ptr()))
    return wq, wsum


class EmitCodes:
    """The consumer's activation quantiser, for a producer that emits its codes directly (conv2d_i8 `emit=`)."""

    def __init__(self, scale, zero_point, lo, hi, form, g=0.0, shift128=False):
        self.scale, self.zero_point, self.lo, self.hi, self.form, self.g = scale, zero_point, int(lo), int(hi), int(form), float(g)
        # shift128 (unsigned byte ranges only): the codes are stored as int8 `code - 128` (DLMCQ_EMIT_SHIFT128) - what the matrix
        # cores multiply anyway; the consumer passes them as signed codes with the zero point `zp - 128` (same integers, same results)
        self.shift128 = bool(shift128)
        if self.shift128 and not (0 <= self.lo and self.hi <= 255):
            raise ValueError("EmitCodes: shift128 needs an unsigned byte range")

    @property
    def dtype(self):
        return torch.uint8 if self.lo >= 0 and not self.shift128 else torch.int8

    @property
    def form_arg(self):
        """The `q_form` argument of the entry points that accept the shifted emission."""
        return self.form | (N.EMIT_SHIFT128 if self.shift128 else 0)


def _act(relu, act):
    """The activation argument of the fused entry points (DLMCQ_ACT_*): `act` when given (N.ACT_NONE / ACT_RELU / ACT_RELU6),
    else ReLU or nothing as `relu` says."""
    if act is None:
        return int(bool(relu))
    if act not in (N.ACT_NONE, N.ACT_RELU, N.ACT_RELU6):
        raise ValueError(f"unknown activation {act!r} (dlmc._native.ACT_NONE / ACT_RELU / ACT_RELU6)")
    return int(act)


# ---- operand marshalling shared by the int8 convolution wrappers below (tensors -> the positional arguments of include/dlmcq.h)
def _flat(t, like, k=None):
    """A scale / zero point / offset operand as a flat contiguous fp32 tensor on `like`'s device: None stays None, a tensor is detached,
    a Python number becomes one entry.  With `k`, a single entry is broadcast to `k` entries (a copy; [k] entries pass as they are)."""
    if t is None:
        return None
    t = _f32c(t.detach() if isinstance(t, torch.Tensor) else t, like).reshape(-1)
    return t.expand(k).contiguous() if k is not None and t.numel() == 1 else t


def _bias_c(bias):
    return None if bias is None else bias.detach().contiguous()


def _nhwc(t):
    """4-D `t` in channels_last memory (a copy only when it is not already)."""
    return t if t.is_contiguous(memory_format=torch.channels_last) else t.contiguous(memory_format=torch.channels_last)


def _out_hw(h, w, r, s, stride=1, padding=0, dilation=1):
    """Output (P, Q) of an r x s convolution (or pooling window) over h x w."""
    return (h + 2 * padding - dilation * (r - 1) - 1) // stride + 1, (w + 2 * padding - dilation * (s - 1) - 1) // stride + 1


def _quantiser(emit, alloc, like, shifted, what):
    """The consumer's quantiser `emit` (EmitCodes or None) as the seven values every fused entry point ends with: (codes tensor,
    q_scale, q_zp, lo, hi, form, g), the codes allocated by `alloc(dtype)`.  `shifted`: whether the entry point takes the shifted
    emission (EmitCodes.shift128, carried in the form); where it does not, asking for it is an error."""
    if emit is None:
        return None, None, None, 0, 0, 0, 0.0
    if emit.shift128 and not shifted:
        raise ValueError(f"{what}: this entry point does not emit shifted codes (EmitCodes.shift128)")
    return (alloc(emit.dtype), _flat(emit.scale, like), _flat(emit.zero_point, like), emit.lo, emit.hi,
            emit.form_arg if shifted else emit.form, emit.g)


def _q_args(q, flags=0):
    """_quantiser's values as call arguments, `flags` (DLMCQ_FORCE_TILED, DLMCQ_ROUTE_ONLY, ...) or-ed into the form."""
    codes, q_scale, q_zp, lo, hi, form, g = q
    return N.ptr(codes), N.ptr(q_scale), N.ptr(q_zp), lo, hi, form | flags, g


def _emit_launch(name, tag, like, shape_or_alloc, emit, want_out, nbytes, issue, ops=0, shifted=False):
    """The tail of the wrappers that return `(out or None, codes or None)` of one launch: fp32 `out` unless `want_out=False`, and with
    `emit=EmitCodes(...)` the consumer's activation codes of the same values, each of `shape_or_alloc` (a shape on `like`'s device, or
    `alloc(dtype)`); `issue(out, codes, *tail)` calls the entry point with the two pointers and `tail` = _q_args' six quantiser values
    and the stream, and is recorded as PROFILE launch `tag` of `nbytes` bytes and `ops` operations.  `shifted`: as _quantiser says.
    (A wrapper with a check of its own behind "nothing to produce" makes that one itself too, where it stands: the order decides what
    a call with two faults is told.)"""
    if not want_out and emit is None:
        raise ValueError(f"{name}: nothing to produce (want_out=False without emit)")
    alloc = shape_or_alloc if callable(shape_or_alloc) else lambda dtype: torch.empty(tuple(shape_or_alloc), dtype=dtype, device=like.device)
    out = alloc(torch.float32) if want_out else None
    q = _quantiser(emit, alloc, like, shifted, name)
    args = (N.ptr(out), *_q_args(q), N.stream_ptr())
    PROFILE.launch(tag, nbytes, lambda: N.check(issue(*args)), ops)
    return out, q[0]


def _as_chunk_major(out):
    """A channels_last fp32 (N, K, P, Q) tensor the kernel wrote chunk-major: the same memory, read as [K / 64][M][64]."""
    n, k, p, q = out.shape
    return ChunkMajor(out.permute(0, 2, 3, 1).reshape(k // 64, n * p * q, 64), out.shape)


# One convolution operand, marshalled: `codes` in the kernel's layout, `keep` the small tensors made for the call (alive until it is
# issued), `shape` of the output, and the two argument runs in the order of include/dlmcq.h as a SECOND operand has them - `ptrs`
# (x, w, bias, wsum, in_scale, in_zero_point, w_scale) and `geom` (H, W, C, R, S, stride, pad, dilation, x_is_unsigned)
_Operand = collections.namedtuple("_Operand", "codes keep shape ptrs geom")


def _operand(t):
    """The operand dict `t` (codes, wq, wsum, bias, in_scale, in_zp, w_scale, optional stride / padding / dilation; codes (N, C, H, W),
    or (N, C) for a linear layer) as an _Operand.  A one-entry `w_scale` is broadcast to [K]."""
    codes, wq = t["codes"], t["wq"]
    N.require_gpu(codes, wq)
    K_, R, S, _ = wq.shape
    st, pd, dl = int(t.get("stride", 1)), int(t.get("padding", 0)), int(t.get("dilation", 1))
    if codes.dim() == 2:
        codes = codes.contiguous()
        (n, c), h, w_ = codes.shape, 1, 1
        shape = (n, K_)
    else:
        codes = _nhwc(codes)
        n, c, h, w_ = codes.shape
        shape = (n, K_) + _out_hw(h, w_, R, S, st, pd, dl)
    bias, si, zp, ws = _bias_c(t["bias"]), _flat(t["in_scale"], codes), _flat(t["in_zp"], codes), _flat(t["w_scale"], codes, K_)
    ptrs = (N.ptr(codes), N.ptr(wq), N.ptr(bias), N.ptr(t["wsum"]), N.ptr(si), N.ptr(zp), N.ptr(ws))
    return _Operand(codes, (bias, si, zp, ws), shape, ptrs, (h, w_, c, R, S, st, pd, dl, int(codes.dtype == torch.uint8)))


def _head(o, out):
    """The eight pointers every entry point starts with: a first operand's, the fp32 output (or None) after the weights."""
    x, w, *rest = o.ptrs
    return (x, w, N.ptr(out), *rest)


def conv2d_i8(codes, wq, wsum, bias, in_scale, in_zp, w_scale, stride=1, padding=0, dilation=1,
              residual=None, relu=False, emit=None, want_out=True, w_offset=None, force_tiled=False, pipelined=False, observe=False,
              out_chunk_major=False, act=None, in_offset=None, tap_sums=None, out_channels=None):
    """Fused int8 conv / linear on the matrix cores.  `codes`: uint8/int8 activation codes, logically
    (N, C, H, W) in channels_last memory, or (N, C) for a linear layer.  Returns fp32 (N, K, P, Q) in
    channels_last memory (or (N, K)).  The operands are marshalled by `_operand`: scales and zero point as `_flat` takes them, a
    one-entry `w_scale` broadcast to [K], codes in another layout copied.

    Epilogue options (dlmcq_conv2d_i8_nhwc_fused): `residual` (fp32, the output's shape and layout) is added,
    `relu` applied (or the activation `act` names: `act=N.ACT_RELU6` is F.relu6), and with `emit=EmitCodes(...)` the consumer's
    activation codes of the result are written as well; the return value is then `(out, out_codes)`, `out` being None when `want_out=False`.
    `w_offset` ([K] fp32): asymmetric per-channel weights w' = qw * s_w[k] + w_offset[k] (dlmcq_conv2d_i8_nhwc_asym).
    `force_tiled` (DLMCQ_FORCE_TILED): the generic tiled kernel even where the library's dispatch would pick a specialised one -
    the same results bit for bit; tests compare the two on one tensor, tools time them on one box.  `pipelined` (DLMCQ_PIPELINED, opt-in):
    the persistent, software-pipelined halo-tile 3x3 kernel where it applies (same bytes; measured slower than the plain one).
    `observe` (dlmcq_conv2d_i8_nhwc_fused_observed; needs the fp32 output): the launch also leaves the observer partials of its output -
    `out._dlmcq_mm = (partials, count, version)` when the kernel that ran has the observing epilogue; `minmax_from_partials` reduces them.
    `residual` may be a ChunkMajor and `out_chunk_major` asks for the fp32 output as one (the block tensors between chain kernels): the
    block-end kernel (csrc/conv_pwr_i8.hip) takes them so; where the library's dispatch hands the call to another kernel a ChunkMajor
    residual is converted first (a copy) and the output comes back as an ordinary tensor.
    `in_offset` (fp32 device scalar o) with `tap_sums` (fp32 [R * S, K]): a float activation offset (dlmcq_conv2d_i8_nhwc_xoff) - `bias`
    must already hold o * tap_sums.sum(0); border pixels lose o * (their out-of-bounds taps' sums).  Not with `observe`.
    `out_channels=k` (dlmcq_conv2d_i8_nhwc_narrow; convolutions only): the weights' K rows are a layer's k real output channels zero-padded
    to a multiple of 64 (K - 64 < k <= K, k % 4 == 0).  The fp32 output is then (N, k, P, Q), dense channels_last, and `residual` has that
    shape, while the emitted codes stay (N, K, P, Q) - what a consumer's K step wants.  Always the tiled kernel.  Not with `observe`,
    `in_offset`, `out_chunk_major`, a ChunkMajor residual or `pipelined`."""
    if (in_offset is None) != (tap_sums is None):
        raise ValueError("conv2d_i8: in_offset and tap_sums go together")
    narrow = out_channels is not None
    padres = isinstance(residual, PadShortcut)
    if padres and not narrow:
        raise ValueError("conv2d_i8: a PadShortcut residual goes with the narrow path only - pass out_channels (K for an unpadded layer)")
    if narrow and (observe or in_offset is not None or out_chunk_major or pipelined or isinstance(residual, ChunkMajor)):
        raise ValueError("conv2d_i8: out_channels (narrow fp32 rows) goes with none of observe, in_offset, out_chunk_major, a ChunkMajor "
                         "residual and pipelined")
    o = _operand(dict(codes=codes, wq=wq, wsum=wsum, bias=bias, in_scale=in_scale, in_zp=in_zp, w_scale=w_scale, stride=stride,
                      padding=padding, dilation=dilation))
    codes, shape = o.codes, o.shape      # (codes: the device / dtype anchor for the small parameter tensors)
    linear = codes.dim() == 2
    (n, K), (h, w_, c, R, S, st, pd, dl, uns) = shape[:2], o.geom
    geo = (n, h, w_, c, K, R, S, st, pd, dl, uns)
    if narrow and linear:
        raise ValueError("conv2d_i8: out_channels is for convolutions (4-D codes)")
    fshape = (n, int(out_channels)) + tuple(shape[2:]) if narrow else shape      # the fp32 tensors' shape (`out`, `residual`)

    def alloc(dtype, shape=shape):
        if linear:
            return torch.empty(shape, dtype=dtype, device=codes.device)
        return torch.empty(shape, dtype=dtype, device=codes.device, memory_format=torch.channels_last)
    act = _act(relu, act)
    fused = (residual is not None or act or emit is not None or w_offset is not None or (observe and want_out) or in_offset is not None
             or narrow)
    if in_offset is not None and observe:
        raise ValueError("conv2d_i8: the offset entry point has no observing form")
    if not want_out and emit is None:
        raise ValueError("conv2d_i8: nothing to produce (want_out=False without emit)")
    out = alloc(torch.float32, fshape) if want_out else None
    head = _head(o, out)
    out_elems, f_elems = math.prod(shape), math.prod(fshape)
    ops = 2 * out_elems * c * R * S
    if not fused:
        if force_tiled:
            raise ValueError("conv2d_i8: force_tiled needs an epilogue (the plain fp32 entry point always runs the tiled kernel)")
        PROFILE.launch("conv_i8", codes.numel() + out_elems * 4 + wq.numel(),
                       lambda: N.check(N.lib.dlmcq_conv2d_i8_nhwc_f32(*head, *geo, N.stream_ptr())), ops)
        return out
    icm = isinstance(residual, ChunkMajor)
    ocm = bool(out_chunk_major) and out is not None and not linear
    pad_args = None
    if padres:
        src = residual.src
        N.require_gpu(src)
        if residual.shape_for(int(out_channels)) != fshape:
            raise ValueError(f"conv2d_i8: the pad shortcut gives {residual.shape_for(int(out_channels))}, the layer's fp32 output is {fshape}")
        pad_args = (N.ptr(src), src.shape[2], src.shape[3], src.shape[1], residual.stride, residual.lo)
        residual_elems = f_elems // int(out_channels) * src.shape[1]     # (what the kernel reads of it)
    elif residual is not None:
        if tuple(residual.shape) != fshape or residual.dtype != torch.float32:
            raise ValueError("conv2d_i8: residual must be fp32 of the output's shape")
        if icm:
            residual = residual.buf
        N.require_gpu(residual)
        if not icm:
            residual = residual.contiguous() if linear else _nhwc(residual)
    q = _quantiser(emit, alloc, codes, True, "conv2d_i8")
    nbytes = (codes.numel() + wq.numel() + f_elems * 4 * (out is not None) + out_elems * (emit is not None) +
              4 * (residual_elems if padres else f_elems * (residual is not None)))
    flags = (N.FORCE_TILED if force_tiled else 0) | (N.PIPELINED if pipelined else 0)
    # the entry point: head, [w_offset], geometry, the epilogue, [what only this entry point takes]
    w_off, trailer, observing = (), (), False
    if in_offset is not None or w_offset is not None or narrow:
        w_offset = _flat(w_offset, codes)
        w_off = (N.ptr(w_offset),)
    if padres:
        fn, trailer = N.lib.dlmcq_conv2d_i8_nhwc_padres, (int(out_channels),)
    elif narrow:
        fn, trailer = N.lib.dlmcq_conv2d_i8_nhwc_narrow, (int(out_channels),)
    elif in_offset is not None:
        fn = N.lib.dlmcq_conv2d_i8_nhwc_xoff
        in_offset, tap_sums = _flat(in_offset, codes), _flat(tap_sums, codes)
        trailer = (N.ptr(in_offset), N.ptr(tap_sums))
    elif w_offset is not None:
        fn = N.lib.dlmcq_conv2d_i8_nhwc_asym
    elif observe and out is not None:
        fn, observing = N.lib.dlmcq_conv2d_i8_nhwc_fused_observed, True
        cap = int(N.lib.dlmcq_conv2d_i8_observed_partials(out_elems // K, K))
        partials = torch.empty(3 * cap, dtype=torch.float32, device=codes.device)
        count = ctypes.c_int64(0)
        trailer = (N.ptr(partials), 3 * cap, ctypes.byref(count))
    else:
        fn = N.lib.dlmcq_conv2d_i8_nhwc_fused

    def call(extra=0):      # (`residual` as it is when the call is made: a ChunkMajor one may be converted below)
        res_args = pad_args if padres else (N.ptr(residual),)
        return fn(*head, *w_off, *geo, *res_args, act, *_q_args(q, flags | extra), *trailer, N.stream_ptr())
    cm_bits = 0
    if icm or ocm:
        # chunk-major block tensors: only where the block-end kernel takes the call, with one layout for its fp32 tensors (the
        # library's own dispatch answers: DLMCQ_ROUTE_ONLY).  Otherwise: the ordinary layout, the residual converted
        if (not w_off and not observing and (residual is None or out is None or icm == ocm)
                and N.route(call(N.ROUTE_ONLY)) == N.ROUTE_PWR):
            cm_bits = (N.FP32_IN_CHUNK_MAJOR if icm else 0) | (N.FP32_OUT_CHUNK_MAJOR if ocm else 0)
        else:
            if icm:
                residual = ChunkMajor(residual, shape).to_nhwc()
            ocm = False
    # (the profile tag - which kernel of the library takes the launch - is asked of the library itself: the same call with
    #  DLMCQ_ROUTE_ONLY runs the dispatch code and launches nothing; only when bench.py's per-kernel events are on)
    tag = N.ROUTE_TAG[N.route(call(N.ROUTE_ONLY))] if PROFILE.enabled else "conv_i8"
    PROFILE.launch(tag, nbytes, lambda: N.check(call(cm_bits)), ops)
    if observing and count.value > 0:
        out._dlmcq_mm = (partials, int(count.value), out._version)      # (an in-place write to `out` later invalidates it: the version is checked)
    if ocm:
        out = _as_chunk_major(out)
    return (out, q[0]) if emit is not None else out


def conv2d_dw_i8(codes, wq, bias, in_scale, in_zp, w_scale, w_offset=None, stride=1, padding=0, relu=False, emit=None, want_out=True,
                 force_tiled=False, act=None, in_offset=None, tap_sums=None):
    """Depthwise convolution on activation codes (dlmcq_conv2d_dw_i8_nhwc).  codes: (N, C, H, W) uint8/int8 channels_last,
    C % 4 == 0; wq: int8 [R, S, C] (tap-major); per-channel w_scale / w_offset / bias [C] (passed as given: no broadcast).  Returns fp32 (N, C, P, Q)
    channels_last, or `(out, codes)` with `emit`.  `relu` / `act` as in conv2d_i8.  `in_offset` / `tap_sums` ([R * S, C]): a float
    activation offset, as in conv2d_i8 (dlmcq_conv2d_dw_i8_nhwc_xoff: 3 x 3 layers, C % 16 == 0)."""
    if (in_offset is None) != (tap_sums is None):
        raise ValueError("conv2d_dw_i8: in_offset and tap_sums go together")
    N.require_gpu(codes, wq)
    n, c, h, w_ = codes.shape
    codes = _nhwc(codes)
    R, S, _ = wq.shape
    P, Q = _out_hw(h, w_, R, S, stride, padding)
    if not want_out and emit is None:
        raise ValueError("conv2d_dw_i8: nothing to produce (want_out=False without emit)")

    def alloc(dtype):
        return torch.empty((n, c, P, Q), dtype=dtype, device=codes.device, memory_format=torch.channels_last)
    q = _quantiser(emit, alloc, codes, False, "conv2d_dw_i8")
    out = alloc(torch.float32) if want_out else None
    small = (_bias_c(bias), _flat(in_scale, codes), _flat(in_zp, codes), _flat(w_scale, codes), _flat(w_offset, codes))
    fn, trailer = N.lib.dlmcq_conv2d_dw_i8_nhwc, ()
    if in_offset is not None:
        in_offset, tap_sums = _flat(in_offset, codes), _flat(tap_sums, codes)
        fn, trailer = N.lib.dlmcq_conv2d_dw_i8_nhwc_xoff, (N.ptr(in_offset), N.ptr(tap_sums))
    args = (N.ptr(codes), N.ptr(wq), N.ptr(out), *map(N.ptr, small), n, h, w_, c, R, S, int(stride), int(padding),
            int(codes.dtype == torch.uint8), _act(relu, act))
    flags = N.FORCE_TILED if force_tiled else 0

    def call(extra=0):
        return fn(*args, *_q_args(q, flags | extra), *trailer, N.stream_ptr())
    oe = n * c * P * Q
    # (the profile tag - conv_dw: the vector kernels, conv_dwm: the matrix-core kernel - from the library's own dispatch, DLMCQ_ROUTE_ONLY)
    tag = N.ROUTE_TAG[N.route(call(N.ROUTE_ONLY))] if PROFILE.enabled else "conv_dw"
    PROFILE.launch(tag, codes.numel() + wq.numel() + oe * (4 * want_out + (emit is not None)), lambda: N.check(call()), 2 * oe * R * S)
    return (out, q[0]) if emit is not None else out


DW5_MAX_C = 2048      # channels dlmcq_conv2d_dw5_i8_nhwc's LDS table holds


def dw5_supported(c, stride, padding, kernel_size):
    """Whether dlmcq_conv2d_dw5_i8_nhwc takes a depthwise layer of c channels: 5 x 5, padding 2, stride 1 or 2,
    c % 16 == 0, c <= 2048 - the entry point's own geometry rules (csrc/conv_dw5_i8.hip)."""
    return int(kernel_size) == 5 and int(padding) == 2 and int(stride) in (1, 2) and c % 16 == 0 and 16 <= c <= DW5_MAX_C


def dw5_profitable(c, h, w, stride):
    """Whether the 5 x 5 kernel was measured faster than the generic one (dlmcq_conv2d_dw_i8_nhwc's route) on a supported layer of c padded
    channels and an h x w input (tools/dw5_ab.py, profiles/dw5_ab.json).  No shape of the sweep was slower - the
    narrowest margin, 1152 channels at 7 x 7, is 1.8 times - so every supported layer is taken."""
    return True


def conv2d_dw5_i8(codes, wq, bias, in_scale, in_zp, w_scale, w_offset=None, stride=1, relu=False, emit=None, want_out=True, act=None):
    """Depthwise 5 x 5 convolution with padding 2 on activation codes, on the integer dot-product kernel (dlmcq_conv2d_dw5_i8_nhwc):
    conv2d_dw_i8's arguments without `padding`, and bit for bit its result on wq [5, 5, C] for an integer input zero point.  C % 16 == 0,
    C <= 2048, stride 1 or 2 (K.dw5_supported); no float activation offset."""
    N.require_gpu(codes, wq)
    n, c, h, w_ = codes.shape
    codes = _nhwc(codes)
    if tuple(wq.shape[:2]) != (5, 5):
        raise ValueError(f"conv2d_dw5_i8: weights [5, 5, C], not {tuple(wq.shape)}")
    P, Q = _out_hw(h, w_, 5, 5, stride, 2)
    if not want_out and emit is None:
        raise ValueError("conv2d_dw5_i8: nothing to produce (want_out=False without emit)")

    def alloc(dtype):
        return torch.empty((n, c, P, Q), dtype=dtype, device=codes.device, memory_format=torch.channels_last)
    q = _quantiser(emit, alloc, codes, False, "conv2d_dw5_i8")
    out = alloc(torch.float32) if want_out else None
    small = (_bias_c(bias), _flat(in_scale, codes), _flat(in_zp, codes), _flat(w_scale, codes), _flat(w_offset, codes))
    args = (N.ptr(codes), N.ptr(wq), N.ptr(out), *map(N.ptr, small), n, h, w_, c, int(stride), 2, int(codes.dtype == torch.uint8), _act(relu, act))
    oe = n * c * P * Q
    PROFILE.launch("conv_dw5", codes.numel() + wq.numel() + oe * (4 * want_out + (emit is not None)),
                   lambda: N.check(N.lib.dlmcq_conv2d_dw5_i8_nhwc(*args, *_q_args(q, 0), N.stream_ptr())), 2 * oe * 25)
    return (out, q[0]) if emit is not None else out


DWPW_WIDTHS = (128, 192, 512)      # pointwise output widths dlmcq_conv2d_dwpw_i8_nhwc is built for


def dwpw_supported(c, k, h, w, stride, padding, ksize):
    """Whether dlmcq_conv2d_dwpw_i8_nhwc takes a depthwise layer (c channels, ksize x ksize, stride, padding, input h x w) followed
    by a pointwise layer to k channels."""
    return ksize == 3 and stride == 1 and padding == 1 and c % 64 == 0 and k in DWPW_WIDTHS and w <= 61 and h >= 1


def dwpw_table(wq, bias, in_scale, in_zp, w_scale, w_offset, x_unsigned=True):
    """The depthwise layer's constants in the fused kernel's layout (dlmcq_dwpw_pack_table): int32 [C / 64, 64, 8]."""
    N.require_gpu(wq)
    r, s_, c = wq.shape
    if (r, s_) != (3, 3) or c % 64:
        raise ValueError("dwpw_table: 3 x 3 weights [3, 3, C], C % 64 == 0")
    table = torch.empty((c // 64, 64, 8), dtype=torch.int32, device=wq.device)
    small = (_bias_c(bias), _flat(in_scale, wq), _flat(in_zp, wq), _flat(w_scale, wq), _flat(w_offset, wq))
    N.check(N.lib.dlmcq_dwpw_pack_table(N.ptr(wq), *map(N.ptr, small), c, int(bool(x_unsigned)), N.ptr(table), N.stream_ptr()))
    return table


def conv2d_dwpw_i8(codes, table, dw_asym, dw_bias, dw_relu, in_zp, emit, pw, relu=True, emit2=None):
    """Depthwise 3x3 / 1 / 1 (+ ReLU + quantiser `emit`) and the pointwise 1x1 convolution `pw` on its codes (+ ReLU + the consumer's
    quantiser `emit2`) in one kernel (dlmcq_conv2d_dwpw_i8_nhwc).  codes: (N, C, H, W) uint8 / int8 channels_last; table:
    dwpw_table(...) of the depthwise layer; pw: dict with wq [K, 1, 1, C], wsum, bias, w_scale, optional w_offset and in_scale (the
    scale the pointwise layer dequantises its input with).  Returns the codes (N, K, H, W)."""
    N.require_gpu(codes, table, pw["wq"])
    codes = _nhwc(codes)
    n, c, h, w_ = codes.shape
    k = pw["wq"].shape[0]
    if tuple(pw["wq"].shape[1:]) != (1, 1, c) or emit is None or emit2 is None or tuple(table.shape) != (c // 64, 64, 8):
        raise ValueError("conv2d_dwpw_i8: a pointwise layer [K, 1, 1, C] on the depthwise layer's codes, both quantisers given")
    q1 = _quantiser(emit, lambda dtype: None, codes, False, "conv2d_dwpw_i8")      # (the depthwise layer's codes stay in LDS)
    q2 = _quantiser(emit2, lambda dtype: torch.empty((n, k, h, w_), dtype=dtype, device=codes.device, memory_format=torch.channels_last),
                    codes, False, "conv2d_dwpw_i8")
    zx, b = _flat(in_zp, codes), _bias_c(pw["bias"])
    scales = (_flat(pw["in_scale"], codes), _flat(pw["w_scale"], codes, k), _flat(pw.get("w_offset"), codes, k))
    m = n * h * w_
    nbytes = codes.numel() + table.numel() * 4 + pw["wq"].numel() + m * k
    PROFILE.launch("conv_dwpw", nbytes, lambda: N.check(N.lib.dlmcq_conv2d_dwpw_i8_nhwc(
        N.ptr(codes), N.ptr(table), int(bool(dw_asym)), int(bool(dw_bias)), int(bool(dw_relu)), N.ptr(zx), n, h, w_, c,
        int(codes.dtype == torch.uint8), *_q_args(q1)[1:], N.ptr(pw["wq"]), N.ptr(b), N.ptr(pw["wsum"]), *map(N.ptr, scales), k,
        int(bool(relu)), *_q_args(q2), N.stream_ptr())), 2 * m * c * (9 + k))
    return q2[0]


def conv2d_i8_dual(a, b, relu=False, emit=None, want_out=True, force_tiled=False, out_chunk_major=False):
    """conv(a) + conv(b) in one kernel (dlmcq_conv2d_i8_nhwc_dual).  `a`, `b`: dicts with codes, wq, wsum, bias,
    in_scale, in_zp, w_scale and optional stride / padding / dilation (`_operand`); both must produce the same output shape.
    Returns fp32 (N, K, P, Q) channels_last, or `(out, codes)` with `emit` (see conv2d_i8; `force_tiled`, `out_chunk_major` as there)."""
    for t in (a, b):
        if t["codes"].dim() != 4:
            raise ValueError("conv2d_i8_dual takes 4-D activation codes")
    oa, ob = _operand(a), _operand(b)
    if oa.shape != ob.shape:
        raise ValueError(f"conv2d_i8_dual: the two convolutions give {oa.shape} and {ob.shape}")
    if not want_out and emit is None:
        raise ValueError("conv2d_i8_dual: nothing to produce (want_out=False without emit)")
    shape = oa.shape
    n, K_ = shape[:2]

    def alloc(dtype):
        return torch.empty(shape, dtype=dtype, device=oa.codes.device, memory_format=torch.channels_last)
    out = alloc(torch.float32) if want_out else None
    q = _quantiser(emit, alloc, oa.codes, True, "conv2d_i8_dual")
    h, w_, ch, R, S, st, pd, dl, uns = oa.geom
    _, _, ch2, R2, S2, st2, _, _, _ = ob.geom
    oe = math.prod(shape)
    def touched(c, r, s_, stride):     # a strided 1x1 convolution reads only the pixels it samples
        return c.numel() // (stride * stride) if r == 1 and s_ == 1 else c.numel()
    nbytes = touched(oa.codes, R, S, st) + touched(ob.codes, R2, S2, st2) + a["wq"].numel() + b["wq"].numel() + oe * (4 * want_out + (emit is not None))
    args = (*_head(oa, out), n, h, w_, ch, K_, R, S, st, pd, dl, uns, *ob.ptrs, *ob.geom, int(bool(relu)))
    flags = N.FORCE_TILED if force_tiled else 0

    def call(extra=0):
        return N.lib.dlmcq_conv2d_i8_nhwc_dual(*args, *_q_args(q, flags | extra), N.stream_ptr())
    # (the profile tag from the library's own dispatch: conv_pwr = csrc/conv_pwr_i8.hip's dual form, conv_i8 = the tiled dual kernel)
    ocm = bool(out_chunk_major) and out is not None and N.route(call(N.ROUTE_ONLY)) == N.ROUTE_PWR
    tag = N.ROUTE_TAG[N.route(call(N.ROUTE_ONLY))] if PROFILE.enabled else "conv_i8"
    PROFILE.launch(tag, nbytes, lambda: N.check(call(N.FP32_OUT_CHUNK_MAJOR if ocm else 0)), 2 * oe * (ch * R * S + ch2 * R2 * S2))
    if ocm:
        out = _as_chunk_major(out)
    return (out, q[0]) if emit is not None else out


CHAIN_SHAPES = {(64, 64), (64, 128), (128, 128), (128, 256), (256, 256)}   # (C, K2) pairs dlmcq_conv2d_i8_nhwc_chain is built for
CHAIN_ONE_LAYOUT = {(128, 128)}    # ... and those whose two fp32 tensors must share one layout (row-major or ChunkMajor, not one of each)
DUAL_CHAIN_SHAPES = {(64, 64, 64), (128, 256, 128)}   # (C, C2, K3) triples dlmcq_conv2d_i8_nhwc_dual_chain is built for
RECOMPUTE_CHAIN_SHAPES = {(64, 64, 64, 64)}   # (C, Ca, Cb, K2) dlmcq_conv2d_i8_nhwc_recompute_chain is built for: ResNet-50's stage 1


def _chain_fits(k, m):
    """What every chain kernel asks of its block tensor [m, k]: whole 64-channel chunks, 32-bit byte offsets."""
    return k % 64 == 0 and m * k * 4 <= 0x7fff0000


def chain_supported(c, k, k2, m):
    """Whether dlmcq_conv2d_i8_nhwc_chain takes a block end [m, c] -> [m, k] followed by a reduction to k2."""
    return (c, k2) in CHAIN_SHAPES and _chain_fits(k, m)


def dual_chain_supported(c, c2, k, k3, m):
    return (c, c2, k3) in DUAL_CHAIN_SHAPES and _chain_fits(k, m)


def recompute_chain_supported(c, ca, cb, k, k2, m):
    return (c, ca, cb, k2) in RECOMPUTE_CHAIN_SHAPES and _chain_fits(k, m)


def chunk_major(wq):
    """Weight codes [K2, 1, 1, K] (KRSC) of a 1x1 layer -> [K / 64, K2, 64]: the layout the chain kernels take for their second layer
    under DLMCQ_W2_CHUNK_MAJOR (a chunk of 64 input columns = one contiguous K2 x 64 byte block)."""
    k2, r, s_, k = wq.shape
    if (r, s_) != (1, 1) or k % 64:
        raise ValueError("chunk_major: a 1x1 layer with K % 64 = 0")
    return wq.reshape(k2, k // 64, 64).permute(1, 0, 2).contiguous()


class ChunkMajor:
    """An fp32 block tensor [N, K, H, W] kept CHUNK-MAJOR between two kernels that walk it chunk by chunk (DLMCQ_FP32_CHUNK_MAJOR):
    `buf` is [K / 64, N * H * W, 64] - every 64-channel chunk one plane of M rows x 256 bytes - so that the pieces neighbouring workgroups
    touch at the same time are neighbours in memory (HBM serves that at 5.9 - 6.0 TB/s, the row-major tensor's 256-byte pieces K * 4 bytes
    apart at 4.6 - 5.8: tools/probes/stream_pattern_probe.hip).  Deliberately NOT a tensor: only the chain / block-end wrappers below take
    it, anything else fails loudly; `.to_nhwc()` gives the ordinary channels_last tensor (same values)."""

    def __init__(self, buf, shape):
        self.buf, self.shape = buf, tuple(shape)
        self.dtype, self.device = buf.dtype, buf.device

    @staticmethod
    def empty(n, k, h, w, device):
        if k % 64:
            raise ValueError("ChunkMajor: K % 64 = 0")
        return ChunkMajor(torch.empty((k // 64, n * h * w, 64), dtype=torch.float32, device=device), (n, k, h, w))

    @staticmethod
    def from_nhwc(t):
        n, k, h, w = t.shape
        if k % 64 or t.dtype != torch.float32:
            raise ValueError("ChunkMajor: an fp32 tensor with K % 64 = 0")
        rows = t.permute(0, 2, 3, 1).reshape(n * h * w, k // 64, 64)
        return ChunkMajor(rows.permute(1, 0, 2).contiguous(), (n, k, h, w))

    def to_nhwc(self):
        n, k, h, w = self.shape
        rows = self.buf.permute(1, 0, 2).reshape(n, h, w, k)
        return rows.permute(0, 3, 1, 2).contiguous(memory_format=torch.channels_last)

    def dim(self):
        return 4

    def numel(self):
        return self.buf.numel()

    def window(self, n, p0, p1, q0, q1):
        """[1, K, p1 - p0, q1 - q0] of image n as an ordinary tensor (tests and tools look at windows of full-size tensors)."""
        nn, k, h, w = self.shape
        rows = self.buf.view(k // 64, nn, h, w, 64)[:, n, p0:p1, q0:q1, :]
        return rows.permute(1, 2, 0, 3).reshape(1, p1 - p0, q1 - q0, k).permute(0, 3, 1, 2).contiguous()

    def record_stream(self, s):
        self.buf.record_stream(s)


class DeferredBlock(ChunkMajor):
    """An fp32 block tensor [N, K, H, W] that is NOT stored: the output relu?(conv1x1(pa) + conv1x1(pb)) of a convolution-shortcut block,
    carried as the two operand dicts it is made of (as conv2d_i8_dual takes them; `pb` may carry a stride).  A reader that can make
    the values itself takes the operands (conv2d_i8_recompute_chain, via fuse.ChainInt8Layer); for anyone else it is a ChunkMajor whose
    `buf` appears on first use - one conv2d_i8_dual launch, the bits the block's own kernel would have stored - and is kept."""

    def __init__(self, pa, pb, relu, shape):
        self.pa, self.pb, self.relu, self.shape = pa, pb, bool(relu), tuple(shape)
        self.dtype, self.device, self._buf = torch.float32, pa["codes"].device, None

    @property
    def buf(self):
        if self._buf is None:
            self._buf = ChunkMajor.from_nhwc(conv2d_i8_dual(self.pa, self.pb, relu=self.relu, emit=None, want_out=True)).buf
        return self._buf

    def numel(self):
        return math.prod(self.shape)

    def record_stream(self, s):
        for t in (self.pa["codes"], self.pb["codes"], self._buf):
            if t is not None:
                t.record_stream(s)


class PadShortcut:
    """The parameter-free "option A" shortcut of He et al. 2016, section 4.2 - `F.pad(src[:, :, ::stride, ::stride], (0, 0, 0, 0, lo, hi))`,
    subsample and zero-pad the channels - as the SOURCE tensor and two numbers instead of the padded tensor: `conv2d_i8(residual=
    PadShortcut(src, stride, lo), out_channels=k)` reads `src` in place (dlmcq_conv2d_i8_nhwc_padres), `hi` being whatever is left of k.
    `src`: fp32 (N, Cs, Hs, Ws), dense in channels_last memory (rows of Cs floats, no gaps), Cs % 4 == 0, lo % 4 == 0.  Deliberately NOT a
    tensor (as ChunkMajor is not): only conv2d_i8's narrow path takes it, anything else fails loudly; `.materialise(k)` gives the tensor."""

    def __init__(self, src, stride=1, lo=0):
        if not isinstance(src, torch.Tensor) or src.dim() != 4 or src.dtype != torch.float32:
            raise ValueError("PadShortcut: the source is an fp32 (N, C, H, W) tensor")
        if not src.permute(0, 2, 3, 1).is_contiguous():
            raise ValueError("PadShortcut: the source must be dense in channels_last memory (a slice or a view with gaps is not)")
        self.src, self.stride, self.lo = src, int(stride), int(lo)
        if self.stride < 1 or self.lo < 0 or self.lo % 4 or src.shape[1] % 4 or src.shape[1] < 4:
            raise ValueError("PadShortcut: stride >= 1, lo >= 0, lo % 4 == 0 and source channels % 4 == 0")
        self.dtype, self.device = src.dtype, src.device

    def shape_for(self, k):
        """Shape of the padded shortcut at `k` channels, or None when source and leading pad do not fit into k."""
        n, c, h, w = self.src.shape
        s = self.stride
        return (n, k, (h + s - 1) // s, (w + s - 1) // s) if self.lo + c <= k else None

    def materialise(self, k):
        """The shortcut as the tensor the model's own `F.pad(x[:, :, ::s, ::s], ...)` builds: fp32 (N, k, P, Q), channels_last."""
        sub = self.src[:, :, ::self.stride, ::self.stride]
        return torch.nn.functional.pad(sub, (0, 0, 0, 0, self.lo, k - self.lo - sub.shape[1])).contiguous(memory_format=torch.channels_last)

    def record_stream(self, s):
        self.src.record_stream(s)


def _second_weights(b):
    """(pointer tensor, form flag) of a chain kernel's second layer: its chunk-major copy when the operand dict carries one."""
    wc = b.get("wq_chunk")
    if wc is None:
        return b["wq"], 0
    k2, _, _, k = b["wq"].shape
    if tuple(wc.shape) != (k // 64, k2, 64) or wc.dtype != torch.int8 or not wc.is_contiguous():
        raise ValueError("wq_chunk must be chunk_major(wq)")
    return wc, N.W2_CHUNK_MAJOR


def _chain(entry, o, mid, b, relu, emit, want_out, want_codes, ocm, relu2, emit2, flags, rows_per_tile, nbytes, ops):
    """What the three chain wrappers share (`entry`: "chain", "dual_chain" or "recompute_chain").  `o`: the block end's _Operand; `mid`: the entry point's arguments between the eight leading
    pointers and `relu` (the problem, the shortcut's operands); `b`: the second layer (wq, wsum, bias, w_scale, optional wq_chunk);
    `ocm`: the fp32 output as a ChunkMajor; `flags`: layout bits for the second form besides the two this function adds; `nbytes`, `ops`:
    the launch's algorithmic bytes and operations, the wrapper's to state.  Returns (out or None, codes or None, codes2)."""
    c, what = o.codes, "conv2d_i8_" + entry
    (n, K_), (h, w_), K2 = o.shape[:2], o.geom[:2], b["wq"].shape[0]

    def alloc(k, dtype):
        return torch.empty((n, k, h, w_), dtype=dtype, device=c.device, memory_format=torch.channels_last)
    out = (ChunkMajor.empty(n, K_, h, w_, c.device) if ocm else alloc(K_, torch.float32)) if want_out else None
    q = _quantiser(emit, lambda dtype: alloc(K_, dtype) if want_codes else None, c, False, what)
    q2 = _quantiser(emit2, lambda dtype: alloc(K2, dtype), c, True, what)
    b2, ws2 = _bias_c(b["bias"]), _flat(b["w_scale"], c, K2)
    w2t, w2flag = _second_weights(b)
    flags |= w2flag | (N.FP32_OUT_CHUNK_MAJOR if ocm else 0)
    PROFILE.launch("conv_chain", nbytes, lambda: N.check(getattr(N.lib, "dlmcq_conv2d_i8_nhwc_" + entry)(
        *_head(o, out.buf if ocm else out), *mid, int(bool(relu)), *_q_args(q), N.ptr(w2t), N.ptr(b2), N.ptr(b["wsum"]), N.ptr(ws2), K2,
        int(bool(relu2)), *_q_args(q2, flags), int(rows_per_tile), N.stream_ptr())), ops)
    return out, q[0], q2[0]


def conv2d_i8_chain(a, b, residual, relu=True, emit=None, want_out=True, want_codes=False, relu2=True, emit2=None,
                    rows_per_tile=0, out_chunk_major=False):
    """A block's last 1x1 convolution (+ residual, ReLU, the consumer's quantiser `emit`) and the next block's first 1x1
    convolution (+ ReLU, its consumer's quantiser `emit2`) in one kernel (dlmcq_conv2d_i8_nhwc_chain).  `a`: dict with
    codes, wq, wsum, bias, in_scale, in_zp, w_scale of the first layer; `b`: wq, wsum, bias, w_scale of the second (its
    input quantiser is `emit`).  Returns (out or None, codes or None, codes2).  `residual` may be a ChunkMajor; `out_chunk_major`
    asks for the fp32 output as one (the 128 -> K -> 128 instantiation keeps both fp32 tensors of a call in ONE layout: there a
    residual in the other layout is converted first - a copy; plans avoid it)."""
    c = a["codes"]
    icm, ocm = isinstance(residual, ChunkMajor), bool(out_chunk_major) and want_out
    if want_out and icm != ocm and (c.shape[1], b["wq"].shape[0]) in CHAIN_ONE_LAYOUT:
        residual = residual.to_nhwc() if icm else ChunkMajor.from_nhwc(residual)
        icm = ocm
    res_cm, residual = (residual, residual.buf) if icm else (None, residual)
    N.require_gpu(b["wq"], residual)
    o = _operand(a)
    (n, K_), (h, w_, ch, R, S, _, _, _, uns) = o.shape[:2], o.geom
    K2, R2, S2, C2 = b["wq"].shape
    if (R, S, R2, S2) != (1, 1, 1, 1) or C2 != K_ or emit is None or emit2 is None:
        raise ValueError("conv2d_i8_chain: two 1x1 convolutions, the second reading the first's codes")
    if tuple(res_cm.shape if icm else residual.shape) != (n, K_, h, w_) or residual.dtype != torch.float32:
        raise ValueError("conv2d_i8_chain: residual must be fp32 of the first output's shape")
    if not icm:
        residual = _nhwc(residual)
    m = n * h * w_
    nbytes = o.codes.numel() + a["wq"].numel() + b["wq"].numel() + m * K_ * (4 + 4 * want_out + want_codes) + m * K2
    return _chain("chain", o, (m, ch, K_, uns, N.ptr(residual)), b, relu, emit, want_out, want_codes, ocm, relu2, emit2,
                  N.FP32_IN_CHUNK_MAJOR if icm else 0, rows_per_tile, nbytes, 2 * m * K_ * (ch + K2))


def conv2d_i8_dual_chain(a, b, c3, relu=True, emit=None, want_out=True, want_codes=False, relu3=True, emit3=None, rows_per_tile=0,
                         out_chunk_major=False):
    """conv1x1(a) + conv1x1(b, strided) (+ ReLU, the consumer's quantiser `emit`) and the next 1x1 convolution `c3` on the
    codes, in one kernel (dlmcq_conv2d_i8_nhwc_dual_chain).  `a`, `b`: operand dicts as for conv2d_i8_dual (`b` may carry a
    stride); `c3`: wq, wsum, bias, w_scale.  Returns (out or None, codes or None, codes3)."""
    N.require_gpu(c3["wq"])
    oa, ob = _operand(a), _operand(b)
    (n, K_), (h, w_, ch, _, _, st, pd, _, uns) = oa.shape[:2], oa.geom
    h2, w2, ch2, _, _, st2, pd2, _, uns2 = ob.geom
    K3 = c3["wq"].shape[0]
    if (tuple(a["wq"].shape[1:3]), tuple(b["wq"].shape[1:3]), tuple(c3["wq"].shape[1:3])) != ((1, 1),) * 3 or st != 1 or pd or pd2 \
            or b["wq"].shape[0] != K_ or c3["wq"].shape[3] != K_ or emit is None or emit3 is None:
        raise ValueError("conv2d_i8_dual_chain: three unpadded 1x1 convolutions, the third reading the codes of the sum of the first two")
    m = n * h * w_
    nbytes = oa.codes.numel() + ob.codes.numel() // (st2 * st2) + a["wq"].numel() + b["wq"].numel() + c3["wq"].numel() + \
        m * K_ * (4 * want_out + want_codes) + m * K3
    return _chain("dual_chain", oa, (n, h, w_, ch, K_, uns, *ob.ptrs, h2, w2, ch2, st2, uns2), c3, relu, emit, want_out,
                  want_codes, bool(out_chunk_major) and want_out, relu3, emit3, 0, rows_per_tile, nbytes, 2 * m * K_ * (ch + ch2 + K3))


def conv2d_i8_recompute_chain(a, b, pa, pb, relu_shortcut=True, relu=True, emit=None, want_out=True, want_codes=False, relu2=True,
                              emit2=None, rows_per_tile=0, out_chunk_major=False):
    """conv2d_i8_chain whose shortcut is not an fp32 tensor but the PREVIOUS block's two operands `pa` (unit stride) and `pb` (may carry a
    stride) - operand dicts as conv2d_i8_dual_chain takes them as `a` and `b`: the shortcut relu?(conv1x1(pa) + conv1x1(pb)) is
    recomputed chunk by chunk, bit for bit what conv2d_i8_dual_chain(pa, pb, ..., want_out=True) stores
    (dlmcq_conv2d_i8_nhwc_recompute_chain).  `a`, `b` and the rest as in conv2d_i8_chain.  Returns (out or None, codes or None, codes2)."""
    N.require_gpu(b["wq"])
    o, oa, ob = _operand(a), _operand(pa), _operand(pb)
    (n, K_), (h, w_, ch, R, S, st, pd, _, uns) = o.shape[:2], o.geom
    _, _, cha, Ra, Sa, sta, pda, _, unsa = oa.geom
    hb, wb_, chb, Rb, Sb, stb, pdb, _, unsb = ob.geom
    K2, R2, S2, C2 = b["wq"].shape
    if (R, S, R2, S2, Ra, Sa, Rb, Sb) != (1,) * 8 or (st, sta) != (1, 1) or pd or pda or pdb or C2 != K_ or emit is None or emit2 is None:
        raise ValueError("conv2d_i8_recompute_chain: unpadded 1x1 convolutions, the second reading the first's codes")
    if oa.shape != o.shape or ob.shape != o.shape:
        raise ValueError(f"conv2d_i8_recompute_chain: the block gives {o.shape}, its recomputed shortcut {oa.shape} and {ob.shape}")
    m = n * h * w_
    # algorithmic bytes: the launch's real operands - three code tensors (the strided one where it is sampled) and four weight tensors in,
    # no fp32 in; ops: the MACs it executes, the two recomputed reductions included
    nbytes = o.codes.numel() + oa.codes.numel() + ob.codes.numel() // (stb * stb) + a["wq"].numel() + pa["wq"].numel() + pb["wq"].numel() + \
        b["wq"].numel() + m * K_ * (4 * want_out + want_codes) + m * K2
    mid = (n, h, w_, ch, K_, uns, *oa.ptrs, cha, unsa, *ob.ptrs, hb, wb_, chb, stb, unsb, int(bool(relu_shortcut)))
    return _chain("recompute_chain", o, mid, b, relu, emit, want_out, want_codes, bool(out_chunk_major) and want_out, relu2, emit2,
                  0, rows_per_tile, nbytes, 2 * m * K_ * (ch + cha + chb + K2))


def quantize_pad_nhwc4(x, scale, zero_point, lo, hi, form, pad, g=0.0, shift128=False, pad_code0=False):
    """Image batch (N, C <= 4, H, W) fp32, any memory format -> activation codes in a zero-point-padded NHWC
    buffer, 4 bytes per pixel: uint8/int8 tensor (N, H + 2 pad, W + 2 pad, 4) (a view of a slightly larger
    allocation: the stem kernel over-reads up to 32 bytes).  `shift128` (unsigned ranges): the buffer holds int8 `code - 128`
    (DLMCQ_EMIT_SHIFT128); the first-layer kernels then take it as signed codes with the zero point `zp - 128`.  `pad_code0`
    (DLMCQ_PAD_CODE0): the border holds code 0, not the code of x' = 0 - a float-offset quantiser's padding (conv2d_i8_stem `in_offset`)."""
    N.require_gpu(x)
    if x.dim() != 4 or x.shape[1] > 4 or x.dtype != torch.float32:
        raise ValueError("quantize_pad_nhwc4 takes an fp32 (N, C <= 4, H, W) tensor")
    n, c, h, w = x.shape
    hp, wp = h + 2 * pad, w + 2 * pad
    if shift128 and not (0 <= lo and hi <= 255):
        raise ValueError("quantize_pad_nhwc4: shift128 needs an unsigned byte range")
    flat = torch.empty(n * hp * wp * 4 + 32, dtype=torch.uint8 if lo >= 0 and not shift128 else torch.int8, device=x.device)
    scale = _f32c(scale.detach(), x).reshape(-1)
    zero_point = None if zero_point is None else _f32c(zero_point, x).reshape(-1)
    PROFILE.launch("fq_image", x.numel() * 4 + n * hp * wp * 4, lambda: N.check(N.lib.dlmcq_quantize_pad_nhwc4(
        N.ptr(x), N.ptr(flat), N.ptr(scale), N.ptr(zero_point), n, c, h, w, *x.stride(), int(pad), int(lo), int(hi),
        int(form) | (N.EMIT_SHIFT128 if shift128 else 0) | (N.PAD_CODE0 if pad_code0 else 0), float(g), N.stream_ptr())))
    return flat[:n * hp * wp * 4].view(n, hp, wp, 4)


def quantize_weight_stem(w, scale, lo, hi):
    """fp32 KCRS weights of a C <= 4 layer -> (int8 [K, R, 8, 4] zero-filled, int32 per-channel code sums)."""
    N.require_gpu(w)
    w = w.detach().contiguous()
    K_, C, R, S = w.shape
    scale = _f32c(scale.detach(), w).reshape(-1)
    if scale.numel() == 1:
        scale = scale.expand(K_).contiguous()
    wq = torch.empty((K_, R, 8, 4), dtype=torch.int8, device=w.device)
    wsum = torch.empty(K_, dtype=torch.int32, device=w.device)
    N.check(N.lib.dlmcq_quantize_weight_stem_i8(N.ptr(w), N.ptr(wq), N.ptr(wsum), N.ptr(scale), K_, C, R, S, int(lo), int(hi),
                                                N.stream_ptr()))
    return wq, wsum


def conv2d_i8_stem(xpad, wq, wsum, bias, in_scale, in_zp, w_scale, S, stride=1, relu=False, emit=None, want_out=True, pool=False,
                   w_offset=None, channels=4, act=None, in_offset=None, tap_sums=None, pad=0):
    """The first-layer convolution on padded NHWC4 codes (quantize_pad_nhwc4 / quantize_weight_stem).  Returns fp32
    (N, K, P, Q) channels_last, or `(out, codes)` with `emit` (see conv2d_i8).  `pool=True` (K <= 64): followed by
    MaxPool2d(3, 2, 1) in the same kernel - the results are the pooled tensors.  `w_offset` ([K] fp32, with the image's real
    channel count `channels`): asymmetric per-channel weights (dlmcq_conv2d_i8_stem_asym; not with `pool`).  `relu` / `act` as in
    conv2d_i8 (the pooling kernel: ReLU only).  `in_offset` / `tap_sums` ([R * S, K]) with `pad` (the buffer's padding, filled with
    code 0: quantize_pad_nhwc4(pad_code0=True)): a float activation offset, as in conv2d_i8 (dlmcq_conv2d_i8_stem_xoff; R = 3 or 7)."""
    if (in_offset is None) != (tap_sums is None) or (in_offset is not None and pool):
        raise ValueError("conv2d_i8_stem: in_offset needs tap_sums and no pool")
    act = _act(relu, act)
    N.require_gpu(xpad, wq)
    n, hp, wp, _ = xpad.shape
    K_, R = wq.shape[0], wq.shape[1]
    P0, Q0 = P, Q = _out_hw(hp, wp, R, S, stride)       # the convolution's own output: what the operation count is of
    if pool:
        if K_ > 64:
            raise ValueError("conv2d_i8_stem(pool=True) handles at most 64 output channels")
        P, Q = _out_hw(P, Q, 3, 3, 2, 1)
    if not want_out and emit is None:
        raise ValueError("conv2d_i8_stem: nothing to produce (want_out=False without emit)")

    def alloc(dtype):
        return torch.empty((n, K_, P, Q), dtype=dtype, device=xpad.device, memory_format=torch.channels_last)
    q = _quantiser(emit, alloc, xpad, False, "conv2d_i8_stem")
    out = alloc(torch.float32) if want_out else None
    bias, in_scale, in_zp, w_scale = _bias_c(bias), _flat(in_scale, xpad), _flat(in_zp, xpad), _flat(w_scale, xpad, K_)
    w_offset, in_offset, tap_sums = _flat(w_offset, xpad), _flat(in_offset, xpad), _flat(tap_sums, xpad)
    # the entry point by (in_offset, w_offset, pool), with what it takes beyond the plain one: [w_offset, C] before the geometry, [pad]
    # inside it, [in_offset, tap_sums] at the end.  (The plain kernels' operation count is of the 3 channels of an image.)
    w_off, pad_arg, trailer, cin = (N.ptr(w_offset), int(channels)), (), (), int(channels)
    if in_offset is not None:
        fn, pad_arg, trailer = N.lib.dlmcq_conv2d_i8_stem_xoff, (int(pad),), (N.ptr(in_offset), N.ptr(tap_sums))
    elif w_offset is not None:
        if pool:
            raise ValueError("conv2d_i8_stem: the pooling kernel has no weight-offset term")
        fn = N.lib.dlmcq_conv2d_i8_stem_asym
    else:
        fn, w_off, cin = (N.lib.dlmcq_conv2d_i8_stem_pool_fused if pool else N.lib.dlmcq_conv2d_i8_stem_fused), (), 3
    args = (N.ptr(xpad), N.ptr(wq), N.ptr(out), N.ptr(bias), N.ptr(wsum), N.ptr(in_scale), N.ptr(in_zp), N.ptr(w_scale), *w_off,
            n, hp, wp, K_, R, int(S), int(stride), *pad_arg, int(xpad.dtype == torch.uint8), act, *_q_args(q), *trailer)
    PROFILE.launch("conv_stem", xpad.numel() + wq.numel() + n * K_ * P * Q * (4 * want_out + (emit is not None)),
                   lambda: N.check(fn(*args, N.stream_ptr())), 2 * n * K_ * P0 * Q0 * R * S * cin)
    return (out, q[0]) if emit is not None else out


def maxpool_codes(codes, kernel, stride, padding):
    """nn.MaxPool2d on channels_last activation codes (uint8 / int8), C % 4 == 0."""
    N.require_gpu(codes)
    n, c, h, w = codes.shape
    if not codes.is_contiguous(memory_format=torch.channels_last):
        codes = codes.contiguous(memory_format=torch.channels_last)
    P, Q = (h + 2 * padding - kernel) // stride + 1, (w + 2 * padding - kernel) // stride + 1
    y = torch.empty((n, c, P, Q), dtype=codes.dtype, device=codes.device, memory_format=torch.channels_last)
    PROFILE.launch("pool_codes", codes.numel() + y.numel(), lambda: N.check(N.lib.dlmcq_maxpool_codes_nhwc(
        N.ptr(codes), N.ptr(y), n, h, w, c, int(kernel), int(stride), int(padding), int(codes.dtype == torch.uint8),
        N.stream_ptr())))
    return y


GAP_HEAD_MAX_HW, GAP_HEAD_MAX_C = 64, 2048    # dlmcq_conv2d_i8_nhwc_gap: the image fits one 64-row tile, the slice's weights stay in LDS (DLMCQ_GAP_MAX_C)


def gap_head_supported(c, k, h, w, ksize=1, stride=1, padding=0, asym=False):
    """Whether dlmcq_conv2d_i8_nhwc_gap takes a layer of c -> k channels (ksize x ksize, stride, padding; `asym`: per-channel weight
    offsets) on an h x w map followed by a global average pool."""
    return (ksize == 1 and stride == 1 and padding == 0 and not asym and c >= 64 and c % 64 == 0 and c <= GAP_HEAD_MAX_C and k >= 64 and
            k % 64 == 0 and h >= 1 and w >= 1 and h * w <= GAP_HEAD_MAX_HW)


# (C, K) of the layers on which the fused head was MEASURED slower than the layer's ordinary launch + the pool kernel (7 x 7 maps, batch
# 512 / 1024: ResNet-50 233 against 98 + 35 us, MobileNetV2 178 against 92 + 45, MobileOne-S1 213 against 105 + 41; DESIGN.md 5.14,
# profiles/gap_head_ab.json).  fuse_inference(gap_head=True) runs these as two launches; the kernel stays reachable through
# conv2d_i8_gap and gap_head="fused"
GAP_HEAD_MEASURED_SLOWER = {(512, 2048), (320, 1280), (512, 1280)}


def gap_head_profitable(c, k):
    """Whether fuse_inference(gap_head=True) routes a gap_head_supported layer of c -> k channels to the fused head: not where it was
    measured slower than the two launches it replaces (GAP_HEAD_MEASURED_SLOWER)."""
    return (c, k) not in GAP_HEAD_MEASURED_SLOWER


def global_avgpool(x, emit=None, want_out=True):
    """Global average pool of an fp32 (N, C, H, W) map in channels_last memory (copied when it is not), C % 4 == 0, by
    dlmcq_gap_nhwc_f32: a sequential fp32 sum over the pixels in row order and a true division (include/dlmcq.h: NOT torch.mean's
    summation order).  Returns fp32 (N, C); with `emit=EmitCodes(...)` `(pooled, codes)` - the consumer's activation codes (N, C) of
    the pooled values - `pooled` being None when `want_out=False`."""
    N.require_gpu(x)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError("global_avgpool: an fp32 (N, C, H, W) tensor")
    x = _nhwc(x)
    n, c, h, w_ = x.shape
    out, codes = _emit_launch("global_avgpool", "gap", x, (n, c), emit, want_out, x.numel() * 4 + n * c * (4 * want_out + (emit is not None)),
                              lambda op, cp, *tail: N.lib.dlmcq_gap_nhwc_f32(N.ptr(x), op, cp, n, h * w_, c, *tail), shifted=True)
    return (out, codes) if emit is not None else out


def _nhwc_rows(x):
    """Floats per pixel if 4-D `x` can be read in place as NHWC rows - channels_last memory, or a channel slice `t[:, :c]` of a
    channels_last tensor (rows wider than the data, a multiple of 4 floats, 16-byte aligned) - else None."""
    n, c, h, w = x.shape
    xs = x.stride(3)
    ok = (h > 1 and w > 1 and x.stride(1) == 1 and xs >= c and xs % 4 == 0 and x.stride(2) == w * xs and
          (n == 1 or x.stride(0) == h * w * xs) and x.data_ptr() % 16 == 0)
    return xs if ok else None


def _fp32_map(name, x):
    """The shape (n, c, h, w) of `x`, which has to be an fp32 4-D tensor."""
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"{name}: an fp32 (N, C, H, W) tensor")
    return tuple(x.shape)


def _map_codes(name, x, p, q_, emit, want_out, c_pad, pad_code, tag, read, issue):
    """avgpool_quant, gate_quant and swish_quant (csrc/map_codes.h) behind their own checks: fp32 map `x` (_fp32_map) to `(out or None,
    codes or None)`, both channels_last with `p` x `q_` pixels.  `x` is read in place when it is channels_last or a channel slice of a
    channels_last tensor, else copied to channels_last.  `out`: fp32, C channels, unless `want_out=False`; `codes`: with
    `emit=EmitCodes(...)` the consumer's activation codes of the same values, `c_pad` channels wide (default C), channels C .. c_pad - 1
    holding the byte `pad_code` (the consumer's zero point; code 0 under a float activation offset; either minus 128 with
    `emit.shift128`).  `tag`, `read`: profile tag and bytes read; `issue(x, out, codes, x_stride, c_pad, pad_code, *quantiser, stream)`
    calls the entry point with the marshalled arguments all three take."""
    if not want_out and emit is None:
        raise ValueError(f"{name}: nothing to produce (want_out=False without emit)")
    n, c = x.shape[:2]
    c_pad = c if c_pad is None else int(c_pad)
    if c_pad != c and emit is None:
        raise ValueError(f"{name}: c_pad pads the code rows (emit=None writes none)")
    xs = _nhwc_rows(x)
    if xs is None:
        x, xs = _nhwc(x), c

    def alloc(dtype):      # (fp32: the map, C channels; else the code rows)
        return torch.empty((n, c if dtype == torch.float32 else c_pad, p, q_), dtype=dtype, device=x.device, memory_format=torch.channels_last)
    return _emit_launch(name, tag, x, alloc, emit, want_out, read + n * p * q_ * (c * 4 * want_out + c_pad * (emit is not None)),
                        lambda op, cp, *tail: issue(N.ptr(x), op, cp, xs, c_pad, int(pad_code), *tail), shifted=True)


def avgpool_quant(x, window, emit=None, want_out=True, c_pad=None, pad_code=0):
    """nn.AvgPool2d(window, window) (no padding, floor) of an fp32 (N, C, H, W) map, C % 4 == 0, by dlmcq_avgpool_nhwc_f32: a
    sequential fp32 sum from +0 in row-major window order and a true division (torch's own loop: the pooled values are bit-identical to
    F.avg_pool2d(x, window)).  Returns `(pooled or None, codes or None)`: fp32 (N, C, H // window, W // window) and the consumer's
    activation codes of the pooled values; the inputs read in place, `emit`, `want_out`, `c_pad` and `pad_code` as _map_codes says."""
    N.require_gpu(x)
    n, c, h, w_ = _fp32_map("avgpool_quant", x)
    s = int(window)
    p, q_ = (h // s, w_ // s) if s > 0 else (0, 0)
    return _map_codes("avgpool_quant", x, p, q_, emit, want_out, c_pad, pad_code, "avgpool", n * p * q_ * c * 4 * s * s,
                      lambda xp, op, cp, xs, cpad, pad, *tail: N.lib.dlmcq_avgpool_nhwc_f32(xp, op, cp, n, h, w_, c, xs, s, cpad, pad, *tail))


def gate_quant(x, gate, act=None, emit=None, want_out=True, c_pad=None, pad_code=0):
    """A squeeze-excite channel gate `x * gate` of an fp32 (N, C, H, W) map, C % 4 == 0, (+ `act`: N.ACT_NONE / ACT_RELU / ACT_RELU6) by
    dlmcq_gate_nhwc_f32: one IEEE multiply per element, then torch's relu / relu6 - the values of `act(x * gate.view(N, C, 1, 1))`, bit
    for bit.  `gate`: any fp32 tensor of N * C elements shaped (N, C, 1, 1) or (N, C), made dense.  Returns `(out or None, codes or
    None)`: fp32 (N, C, H, W) and the consumer's activation codes of the gated values; the inputs read in place, `emit`, `want_out`,
    `c_pad` and `pad_code` as _map_codes says."""
    N.require_gpu(x, gate)
    n, c, h, w_ = _fp32_map("gate_quant", x)
    if gate.dtype != torch.float32 or tuple(gate.shape) not in ((n, c, 1, 1), (n, c)):
        raise ValueError(f"gate_quant: an fp32 gate of shape ({n}, {c}, 1, 1) or ({n}, {c}), not {gate.dtype} {tuple(gate.shape)}")
    gate = gate.detach().reshape(n, c).contiguous()
    return _map_codes("gate_quant", x, h, w_, emit, want_out, c_pad, pad_code, "gate", n * h * w_ * c * 4 + n * c * 4,
                      lambda xp, op, cp, xs, cpad, pad, *tail: N.lib.dlmcq_gate_nhwc_f32(xp, N.ptr(gate), op, cp, n, h, w_, c, xs, cpad, pad,
                                                                                         _act(False, act), *tail))


def swish_quant(x, emit=None, want_out=True, c_pad=None, pad_code=0):
    """Swish / SiLU `x * sigmoid(x)` of an fp32 (N, C, H, W) map, C % 4 == 0, by dlmcq_swish_nhwc_f32: e = expf(-x), d = 1 + e, s = 1 / d,
    v = x * s, each step rounded to fp32 - the operation sequence of `x * torch.sigmoid(x)`.  Returns `(out or None, codes or None)`:
    fp32 (N, C, H, W) and the consumer's activation codes of the activated values; the inputs read in place, `emit`, `want_out`, `c_pad`
    and `pad_code` as _map_codes says."""
    N.require_gpu(x)
    n, c, h, w_ = _fp32_map("swish_quant", x)
    return _map_codes("swish_quant", x, h, w_, emit, want_out, c_pad, pad_code, "swish", n * h * w_ * c * 4,
                      lambda xp, op, cp, xs, cpad, pad, *tail: N.lib.dlmcq_swish_nhwc_f32(xp, op, cp, n, h, w_, c, xs, cpad, pad, *tail))


HARDSWISH_ORDERS = {"mul_first": N.HSWISH_MUL_FIRST, "gate_first": N.HSWISH_GATE_FIRST}


def hardswish_quant(x, order="mul_first", emit=None, want_out=True, c_pad=None, pad_code=0):
    """Hard swish `x * relu6(x + 3) / 6` of an fp32 (N, C, H, W) map, C % 4 == 0, by dlmcq_hardswish_nhwc_f32: t = x + 3, r = relu6(t),
    c = fl32(1 / 6), then `order="mul_first"`: v = (x * r) * c - nn.Hardswish, F.hardswish, `x * F.relu6(x + 3) / 6` - or
    `order="gate_first"`: v = x * (r * c) - `x * (F.relu6(x + 3) / 6)`, `x * F.hardsigmoid(x)` - each step rounded to fp32.  Returns
    `(out or None, codes or None)`: fp32 (N, C, H, W) and the consumer's activation codes of the activated values; the inputs read in
    place, `emit`, `want_out`, `c_pad` and `pad_code` as _map_codes says."""
    N.require_gpu(x)
    n, c, h, w_ = _fp32_map("hardswish_quant", x)
    if order not in HARDSWISH_ORDERS:
        raise ValueError(f"hardswish_quant: order is 'mul_first' or 'gate_first', not {order!r}")
    o = HARDSWISH_ORDERS[order]
    return _map_codes("hardswish_quant", x, h, w_, emit, want_out, c_pad, pad_code, "hardswish", n * h * w_ * c * 4,
                      lambda xp, op, cp, xs, cpad, pad, *tail: N.lib.dlmcq_hardswish_nhwc_f32(xp, op, cp, n, h, w_, c, xs, cpad, pad, *tail[:-1],
                                                                                              o, tail[-1]))


SQUEEZE_ACTS = {None: N.SQUEEZE_NONE, "none": N.SQUEEZE_NONE, "relu": N.SQUEEZE_RELU, "swish": N.SQUEEZE_SWISH}
GATE_FNS = {None: N.GATE_NONE, "none": N.GATE_NONE, "sigmoid": N.GATE_SIGMOID, "hardsigmoid": N.GATE_HARDSIGMOID}

# the two layers of a squeeze path, checked: layer 1 (wq [R, C], wsum [R], bias, in_scale, in_zp, w_scale), layer 2 (wq [C, R], wsum [C],
# bias, w_scale) - the small tensors flat fp32 on the codes' device, a one-entry weight scale broadcast
_Squeeze = collections.namedtuple("_Squeeze", "n c r w1 wsum1 b1 s1 zp1 ws1 w2 wsum2 b2 ws2 act fn")


def _squeeze_operands(name, codes, l1, inner_act, emit, l2, gate_fn, want_gate, want_hidden):
    """squeeze_gate's and squeeze_gate_torch's shared argument checks, in the order that decides what a call with two faults is told:
    the two names, nothing to produce, the quantiser, the codes, layer 1, layer 2 - all before anything needs the GPU."""
    if inner_act not in SQUEEZE_ACTS:
        raise ValueError(f"{name}: inner_act is None, 'relu' or 'swish', not {inner_act!r}")
    if gate_fn not in GATE_FNS:
        raise ValueError(f"{name}: gate_fn is None, 'sigmoid' or 'hardsigmoid', not {gate_fn!r}")
    if not (want_gate or want_hidden):
        raise ValueError(f"{name}: nothing to produce (neither the gate nor the hidden values)")
    if emit is None:
        raise ValueError(f"{name}: the second layer's activation quantiser (emit=EmitCodes(...)) is required")
    if emit.shift128:
        raise ValueError(f"{name}: the hidden codes are plain codes (EmitCodes.shift128 is refused)")
    if emit.lo < 0 and emit.hi > 127:
        raise ValueError(f"{name}: the hidden codes are uint8 or int8 bytes, the range {emit.lo} .. {emit.hi} is neither")
    if codes.dim() != 2 or codes.dtype not in (torch.uint8, torch.int8):
        raise ValueError(f"{name}: activation codes (N, C), uint8 or int8, not {codes.dtype} {tuple(codes.shape)}")
    n, c = codes.shape
    w1, w2 = l1["wq"], l2["wq"]
    w1 = w1.reshape(w1.shape[0], -1) if w1.dim() == 4 and w1.shape[1:3] == (1, 1) else w1
    w2 = w2.reshape(w2.shape[0], -1) if w2.dim() == 4 and w2.shape[1:3] == (1, 1) else w2
    if w1.dim() != 2 or w1.dtype != torch.int8 or w1.shape[1] != c or w1.shape[0] < 1:
        raise ValueError(f"{name}: layer 1's weight codes are int8 [R, {c}], not {w1.dtype} {tuple(w1.shape)}")
    r = w1.shape[0]
    if w2.dim() != 2 or w2.dtype != torch.int8 or tuple(w2.shape) != (c, r):
        raise ValueError(f"{name}: layer 2's weight codes are int8 [{c}, {r}], not {w2.dtype} {tuple(w2.shape)}")
    for what, t, k in (("layer 1's wsum", l1["wsum"], r), ("layer 2's wsum", l2["wsum"], c)):
        if t.dtype != torch.int32 or t.numel() != k:
            raise ValueError(f"{name}: {what} is int32 [{k}], not {t.dtype} {tuple(t.shape)}")
    for what, t, k in (("layer 1's bias", l1.get("bias"), r), ("layer 2's bias", l2.get("bias"), c)):
        if t is not None and (t.dtype != torch.float32 or t.numel() != k):
            raise ValueError(f"{name}: {what} is fp32 [{k}] or None, not {t.dtype} {tuple(t.shape)}")
    for what, t, k in (("layer 1's w_scale", l1["w_scale"], r), ("layer 2's w_scale", l2["w_scale"], c)):
        if isinstance(t, torch.Tensor) and t.numel() not in (1, k):
            raise ValueError(f"{name}: {what} has 1 or {k} entries, not {t.numel()}")
    N.require_gpu(codes, w1, w2)
    codes = codes.contiguous()
    return codes, _Squeeze(n, c, r, w1.contiguous(), l1["wsum"].reshape(-1).contiguous(), _bias_c(l1.get("bias")), _flat(l1["in_scale"], codes),
                           _flat(l1.get("in_zp"), codes), _flat(l1["w_scale"], codes, r), w2.contiguous(), l2["wsum"].reshape(-1).contiguous(),
                           _bias_c(l2.get("bias")), _flat(l2["w_scale"], codes, c), SQUEEZE_ACTS[inner_act], GATE_FNS[gate_fn])


def _pad_cols(t, width, fill):
    """2-D `t` with its rows widened to `width` columns of `fill` (a Python number or a one-entry tensor): a copy, or `t` as it is."""
    n, c = t.shape
    if c == width:
        return t
    out = torch.empty((n, width), dtype=t.dtype, device=t.device)
    out[:, :c] = t
    out[:, c:] = fill
    return out


def squeeze_gate_supported(c, r):
    """Whether dlmcq_squeeze_gate_i8 takes a squeeze path of `c` channels and `r` hidden units (padded to a multiple of 4)."""
    return c % 4 == 0 and 4 <= c <= N.SQUEEZE_MAX_C and 1 <= (r + 3) // 4 * 4 <= N.SQUEEZE_MAX_R


def squeeze_gate_torch(codes, l1, inner_act, emit, l2, gate_fn, want_gate=True, want_hidden=False):
    """squeeze_gate restated with the wrappers that were there before it - what squeeze_gate runs for widths its kernel does not take,
    and the yardstick its tests compare it with bit for bit: the codes padded with their zero point and the weights with 0 to a multiple
    of 64 (integer sums do not change), conv2d_i8, the activation in torch, fake_quant to the hidden codes, conv2d_i8, torch.sigmoid or
    F.relu6(v + 3) / 6.  Returns `(gate or None, hidden or None)`, hidden (N, R)."""
    codes, q = _squeeze_operands("squeeze_gate_torch", codes, l1, inner_act, emit, l2, gate_fn, want_gate, want_hidden)
    c64, r64 = (q.c + 63) // 64 * 64, (q.r + 63) // 64 * 64
    zp1 = 0 if q.zp1 is None else q.zp1.to(codes.dtype)
    w1 = _pad_cols(q.w1, c64, 0).reshape(q.r, 1, 1, c64)
    h = conv2d_i8(_pad_cols(codes, c64, zp1), w1, q.wsum1, q.b1, q.s1, q.zp1, q.ws1)
    if q.act == N.SQUEEZE_RELU:
        h = torch.relu(h)
    elif q.act == N.SQUEEZE_SWISH:
        h = h * torch.sigmoid(h)
    hidden = h if want_hidden else None
    if not want_gate:
        return None, hidden
    hq = fake_quant(h, emit.scale, emit.zero_point, emit.lo, emit.hi, emit.form, g=emit.g, codes="i8", want_y=False)[1]
    s_h, zp2 = _flat(emit.scale, codes), _flat(emit.zero_point, codes)
    if emit.form == FORM_QBASE:
        sg = s_h * emit.g
        s_h = (s_h - sg) + sg
    w2 = _pad_cols(q.w2, r64, 0).reshape(q.c, 1, 1, r64)
    v = conv2d_i8(_pad_cols(hq, r64, 0 if zp2 is None else zp2.to(hq.dtype)), w2, q.wsum2, q.b2, s_h, zp2, q.ws2)
    if q.fn == N.GATE_SIGMOID:
        v = torch.sigmoid(v)
    elif q.fn == N.GATE_HARDSIGMOID:
        v = torch.nn.functional.relu6(v + 3) / 6
    return v, hidden


def squeeze_gate(codes, l1, inner_act, emit, l2, gate_fn, want_gate=True, want_hidden=False):
    """The squeeze path of a squeeze-excite block from its pooled activation codes (N, C) - global_avgpool's - to the fp32 gate (N, C), by
    dlmcq_squeeze_gate_i8 in one launch: int8 layer 1 (`l1`: wq int8 [R, C], wsum, bias or None, in_scale, in_zp, w_scale), `inner_act`
    (None, "relu", "swish"), the hidden quantiser `emit` (EmitCodes, plain codes), int8 layer 2 (`l2`: wq int8 [C, R], wsum, bias or None,
    w_scale; its input scale and zero point are the quantiser's), `gate_fn` (None, "sigmoid", "hardsigmoid").  The operands are marshalled
    as conv2d_i8 marshals its own; a hidden width that is no multiple of 4 is zero-padded here, per call (a plan pads once).  Returns
    `(gate or None, hidden or None)`: `hidden` (N, R) the fp32 values behind `inner_act`, for tests and calibration.  Widths the kernel
    does not take (C % 4, C > 2048, R > 512) run squeeze_gate_torch: the same values from the tiled kernels."""
    codes, q = _squeeze_operands("squeeze_gate", codes, l1, inner_act, emit, l2, gate_fn, want_gate, want_hidden)
    if not squeeze_gate_supported(q.c, q.r):
        return squeeze_gate_torch(codes, l1, inner_act, emit, l2, gate_fn, want_gate, want_hidden)
    n, c, r = q.n, q.c, q.r
    r4 = (r + 3) // 4 * 4
    w1, wsum1, b1, ws1, w2 = q.w1, q.wsum1, q.b1, q.ws1, q.w2
    if r4 != r:
        pad = lambda t, fill: torch.cat([t.reshape(-1), torch.full((r4 - r,), fill, dtype=t.dtype, device=t.device)])  # noqa: E731
        w1 = torch.cat([w1, torch.zeros((r4 - r, c), dtype=torch.int8, device=w1.device)])
        wsum1, ws1, b1 = pad(wsum1, 0), pad(ws1, 1.0), (None if b1 is None else pad(b1, 0.0))
        w2 = _pad_cols(w2, r4, 0)
    gate = torch.empty((n, c), dtype=torch.float32, device=codes.device) if want_gate else None
    hidden = torch.empty((n, r4), dtype=torch.float32, device=codes.device) if want_hidden else None
    qs, qz = _flat(emit.scale, codes), _flat(emit.zero_point, codes)
    nbytes = n * c + w1.numel() + w2.numel() + 4 * n * c * want_gate + 4 * n * r4 * want_hidden
    PROFILE.launch("squeeze", nbytes, lambda: N.check(N.lib.dlmcq_squeeze_gate_i8(
        N.ptr(codes), N.ptr(w1), N.ptr(wsum1), N.ptr(b1), N.ptr(q.s1), N.ptr(q.zp1), N.ptr(ws1), q.act, N.ptr(w2), N.ptr(q.wsum2), N.ptr(q.b2),
        N.ptr(q.ws2), q.fn, N.ptr(gate), N.ptr(hidden), n, c, r4, int(codes.dtype == torch.uint8), N.ptr(qs), N.ptr(qz), emit.lo, emit.hi,
        emit.form, emit.g, N.stream_ptr())), 2 * n * (c * r4) * 2)
    return gate, (hidden if hidden is None or r4 == r else hidden[:, :r])


def gelu_quant(x, emit=None, want_out=True, c_pad=None, pad_code=0):
    """GELU in its erf form (nn.GELU() / F.gelu(x), approximate="none") by dlmcq_gelu_nhwc_f32: z = x * fl32(1 / sqrt(2)), e = erff(z),
    f = 1 + e, h = x * 0.5, v = h * f, each step rounded to fp32 - the operation order of torch's device kernel.  `x`: an fp32 4-D
    tensor is an (N, C, H, W) map, C % 4 == 0, handled as swish_quant handles it (read in place when channels_last or a channel slice
    of a channels_last tensor); an fp32 tensor of any other rank is dense rows [..., C], C % 4 == 0 (copied when not contiguous), passed
    as N = rows, H = W = 1.  Returns `(out or None, codes or None)` in the input's shape (code rows `c_pad` wide); `emit`, `want_out`,
    `c_pad` and `pad_code` as _map_codes says."""
    N.require_gpu(x)
    if x.dtype != torch.float32 or x.dim() < 1:
        raise ValueError("gelu_quant: an fp32 (N, C, H, W) map or fp32 rows [..., C]")
    lead = None
    if x.dim() != 4:
        lead, x = tuple(x.shape[:-1]), x.reshape(-1, x.shape[-1]).contiguous()
        x = x.view(x.shape[0], x.shape[1], 1, 1)
    n, c, h, w_ = x.shape
    out, codes = _map_codes("gelu_quant", x, h, w_, emit, want_out, c_pad, pad_code, "gelu", n * h * w_ * c * 4,
                            lambda xp, op, cp, xs, cpad, pad, *tail: N.lib.dlmcq_gelu_nhwc_f32(xp, op, cp, n, h, w_, c, xs, cpad, pad, *tail))
    if lead is not None:
        out = None if out is None else out.reshape(*lead, c)
        codes = None if codes is None else codes.reshape(*lead, codes.shape[1])
    return out, codes


LAYERNORM_MAX_C = 2048    # dlmcq_layernorm_rows_f32: a row lives in one wave's registers (8 quads of 4 floats per lane)


def layernorm_quant(x, weight, bias, eps, emit=None, want_out=True):
    """nn.LayerNorm((C,)) of dense fp32 rows `x` [..., C], C % 4 == 0, 4 <= C <= LAYERNORM_MAX_C, by dlmcq_layernorm_rows_f32: a two-pass
    mean / biased variance in a fixed summation order (include/dlmcq.h), r = 1 / sqrt(var + eps), v = ((x - mean) * r) * weight + bias,
    each step rounded to fp32.  `weight`, `bias`: fp32 [C] or None.  Returns `(out or None, codes or None)` in the input's shape: fp32
    unless `want_out=False`, and with `emit=EmitCodes(...)` the consumer's activation codes of the same values (plain codes: the
    readers are Linear layers; EmitCodes.shift128 is an error)."""
    N.require_gpu(x)
    if x.dtype != torch.float32 or x.dim() < 1:
        raise ValueError("layernorm_quant: fp32 rows [..., C]")
    if not want_out and emit is None:
        raise ValueError("layernorm_quant: nothing to produce (want_out=False without emit)")
    c = x.shape[-1]
    for name, t in (("weight", weight), ("bias", bias)):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (c,)):
            raise ValueError(f"layernorm_quant: an fp32 {name} of shape ({c},), not {t.dtype} {tuple(t.shape)}")
    shape = tuple(x.shape)
    x = x.detach().reshape(-1, c).contiguous()
    m = x.shape[0]
    weight, bias = _bias_c(weight), _bias_c(bias)
    nbytes = m * c * (4 + 4 * want_out + (emit is not None)) + 4 * c * ((weight is not None) + (bias is not None))
    return _emit_launch("layernorm_quant", "layernorm", x, shape, emit, want_out, nbytes, lambda op, cp, *tail: N.lib.dlmcq_layernorm_rows_f32(
        N.ptr(x), N.ptr(weight), N.ptr(bias), op, cp, m, c, float(eps), *tail))


PATCH_MAX_STRIP = 65536      # dlmcq_patch_rows_f32: elements of one (image, patch row) strip, whose codes are staged in LDS


def patch_rows_torch(img, p):
    """The patch rows [B, gh * gw, p * p * C] of an image batch (B, C, gh * p, gw * p) in torch ops: the graph's own reshape, permute
    and reshape ('b c (h p1) (w p2) -> b (h w) (p1 p2 c)')."""
    b, c, h, w = img.shape
    gh, gw = h // p, w // p
    return img.reshape(b, c, gh, p, gw, p).permute(0, 2, 4, 3, 5, 1).reshape(b, gh * gw, p * p * c)


def patch_rows_view(img, p):
    """Whether dlmcq_patch_rows_f32 reads the image batch `img` (B, C, H, W) in place for patches of p x p pixels: an fp32 device
    tensor, p % 4 == 0, H and W multiples of p, unit stride along a line, every other stride a non-negative multiple of 4 elements,
    a strip's gw * p * p * C elements within PATCH_MAX_STRIP, 16-byte aligned."""
    if not (isinstance(p, int) and p >= 4 and p % 4 == 0 and img.dim() == 4 and img.dtype == torch.float32 and img.is_cuda):
        return False
    b, c, h, w = img.shape
    if c < 1 or h < p or w < p or h % p or w % p or w * p * c > PATCH_MAX_STRIP:
        return False
    sb, sc, sh, sw = img.stride()
    return sw == 1 and not any(s < 0 or s % 4 for s in (sb, sc, sh)) and img.data_ptr() % 16 == 0


def patch_rows_quant(img, p, emit=None, want_out=True):
    """The patch rows of a vision transformer, `img.reshape(B, C, gh, p, gw, p).permute(0, 2, 4, 3, 5, 1).reshape(B, gh * gw, p * p * C)`
    of an image batch (B, C, gh * p, gw * p), by dlmcq_patch_rows_f32: one read of the image, read in place through its strides.
    Returns `(rows or None, codes or None)`, both [B, gh * gw, p * p * C]: fp32 unless `want_out=False`, and with `emit=EmitCodes(...)`
    the activation codes of the embedding that reads the rows - K.fake_quant of the rows, bit for bit (plain codes: the reader is a
    Linear layer; EmitCodes.shift128 is an error).  An input the kernel does not take (patch_rows_view: not fp32, not on the device, a
    stride along the lines other than 1 - a channels_last batch -, strides or a base that are not aligned, a strip too long for the
    LDS) takes the torch restatement: patch_rows_torch, then K.fake_quant - the unfused graph's values."""
    if img.dim() != 4 or not isinstance(p, int) or p < 1 or img.shape[2] % p or img.shape[3] % p:
        raise ValueError(f"patch_rows_quant: an image batch (B, C, gh * p, gw * p), not {tuple(img.shape)} with p = {p!r}")
    if not want_out and emit is None:
        raise ValueError("patch_rows_quant: nothing to produce (want_out=False without emit)")
    if emit is not None and emit.shift128:
        raise ValueError("patch_rows_quant: this entry point does not emit shifted codes (EmitCodes.shift128)")
    img = img.detach()
    b, c, h, w = img.shape
    gh, gw = h // p, w // p
    if not patch_rows_view(img, p):
        rows = patch_rows_torch(img, p)
        codes = None
        if emit is not None:
            codes = fake_quant(rows.contiguous(), emit.scale, emit.zero_point, emit.lo, emit.hi, emit.form, g=emit.g, codes="i8",
                               want_y=False)[1]
        return (rows if want_out else None), codes
    return _emit_launch("patch_rows_quant", "patch_rows", img, (b, gh * gw, p * p * c), emit, want_out,
                        img.numel() * (4 + 4 * want_out + (emit is not None)), lambda op, cp, *tail: N.lib.dlmcq_patch_rows_f32(
                            N.ptr(img), op, cp, b, c, gh, gw, p, *img.stride()[:3], *tail))


def tokens_view(e, cls, pos):
    """Whether dlmcq_tokens_assemble_f32 takes the embedded patches `e` [B, T, C], the class token `cls` [1, 1, C] and the position
    embedding `pos` [1, T + 1, C]: fp32 device tensors, T >= 1, C % 4 == 0; `e` with unit stride in C, a row stride that is a multiple
    of 4 elements and rows b * T + i one stride apart (a dense tensor, or a column slice of one), 16-byte aligned."""
    ts = (e, cls, pos)
    if not all(isinstance(t, torch.Tensor) and t.dim() == 3 and t.dtype == torch.float32 and t.is_cuda for t in ts):
        return False
    b, t, c = e.shape
    if t < 1 or c < 4 or c % 4 or tuple(cls.shape) != (1, 1, c) or tuple(pos.shape) != (1, t + 1, c):
        return False
    sb, st, sc = e.stride()
    if sc != 1 or st < c or st % 4 or (b > 1 and sb != t * st) or e.data_ptr() % 16:
        return False
    return all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in (cls, pos))


def assemble_tokens(e, cls, pos):
    """`torch.cat((cls.expand(B, -1, -1), e), 1) + pos` - a transformer's token tensor [B, T + 1, C] from the embedded patches `e`
    [B, T, C], the class token `cls` [1, 1, C] and the position embedding `pos` [1, T + 1, C] - by dlmcq_tokens_assemble_f32: one IEEE
    add per element in one pass, the bits of torch's concatenation and add.  fp32.  Inputs the kernel does not take (tokens_view: not
    fp32, not on the device, other shapes, C % 4 != 0, rows of `e` that are not one stride apart or not aligned) take that torch
    expression itself."""
    if not tokens_view(e, cls, pos):
        return torch.cat((cls.expand(e.shape[0], -1, -1), e), dim=1) + pos
    e, cls, pos = e.detach(), cls.detach(), pos.detach()
    b, t, c = e.shape
    out = torch.empty((b, t + 1, c), dtype=torch.float32, device=e.device)
    PROFILE.launch("tokens", 4 * c * (b * t + (t + 1) + 1 + b * (t + 1)),
                   lambda: N.check(N.lib.dlmcq_tokens_assemble_f32(N.ptr(e), N.ptr(cls), N.ptr(pos), N.ptr(out), b, t, c, e.stride(1),
                                                                   (t + 1) * c, c, N.stream_ptr())))
    return out


ATTENTION_DIMS = (32, 64)    # dlmcq_attention_f32: the head dimensions the kernel is built for


def attention_views(q, k, v):
    """Whether dlmcq_attention_f32 reads `q` [B, H, Tq, D] and `k`, `v` [B, H, Tk, D] in place: fp32, D in ATTENTION_DIMS, Tk >= 1, unit
    stride in D, every other stride a multiple of 4 elements and a token's row not overlapping the next, 16-byte aligned."""
    if not (q.dim() == k.dim() == v.dim() == 4 and q.dtype == k.dtype == v.dtype == torch.float32):
        return False
    b, h, tq, d = q.shape
    if d not in ATTENTION_DIMS or tuple(k.shape) != tuple(v.shape) or tuple(k.shape[:2]) != (b, h) or k.shape[3] != d or k.shape[2] < 1:
        return False
    for t in (q, k, v):
        sb, sh, st, sd = t.stride()
        if sd != 1 or any(s < 0 or s % 4 for s in (sb, sh, st)) or st < d or t.data_ptr() % 16:
            return False
    return True


def attention_quant(q, k, v, scale, emit=None, want_out=True, merged=True):
    """softmax(scale * q k^T) v of fp32 views `q` [B, H, Tq, D], `k`, `v` [B, H, Tk, D] (attention_views: read in place, the three
    slices of one packed projection included) by dlmcq_attention_f32: one flash forward on the f32 matrix cores - k-ordered fmaf
    chains, an online softmax over key blocks of 32 with the accurate expf, a true division at the end (include/dlmcq.h states the
    order and the bound); no mask, no dropout.  `merged`: the result as [B, Tq, H * D], the merge-heads permute + reshape a free view;
    else [B, H, Tq, D].  Returns `(out or None, codes or None)`: fp32 unless `want_out=False`, and with `emit=EmitCodes(...)` the
    consumer's activation codes of the same values (plain codes: the reader is a Linear layer; EmitCodes.shift128 is an error)."""
    N.require_gpu(q, k, v)
    if not attention_views(q, k, v):
        raise ValueError("attention_quant: fp32 views q [B, H, Tq, D], k, v [B, H, Tk, D], D in (32, 64), unit stride in D, strides "
                         "multiples of 4 elements, 16-byte aligned")
    if not want_out and emit is None:
        raise ValueError("attention_quant: nothing to produce (want_out=False without emit)")
    scale = float(scale)
    if not math.isfinite(scale):
        raise ValueError(f"attention_quant: a finite scale, not {scale}")
    q, k, v = q.detach(), k.detach(), v.detach()
    b, h, tq, d = q.shape
    tk = k.shape[2]
    shape = (b, tq, h * d) if merged else (b, h, tq, d)
    o_strides = (tq * h * d, d, h * d) if merged else (h * tq * d, tq * d, d)
    nbytes = 4 * b * h * d * (tq + 2 * tk) + b * h * tq * d * (4 * want_out + (emit is not None))
    return _emit_launch("attention_quant", "attention", q, shape, emit, want_out, nbytes, lambda op, cp, *tail: N.lib.dlmcq_attention_f32(
        N.ptr(q), N.ptr(k), N.ptr(v), op, cp, b, h, tq, tk, d, *q.stride()[:3], *k.stride()[:3], *v.stride()[:3], *o_strides, scale, *tail),
        ops=4 * b * h * tq * tk * d)


def conv2d_i8_gap(codes, wq, wsum, bias, in_scale, in_zp, w_scale, residual=None, act=None, emit=None, want_out=True):
    """A 1 x 1 / stride 1 / unpadded int8 convolution (+ fp32 `residual` of its output's shape) (+ `act`: N.ACT_NONE / ACT_RELU /
    ACT_RELU6) and the global average pool of the result in ONE launch (dlmcq_conv2d_i8_nhwc_gap): the (N, K, H, W) map is never
    written.  Operands as conv2d_i8 takes them (codes (N, C, H, W), wq [K, 1, 1, C]); `gap_head_supported` says which shapes the
    kernel is built for.  Returns fp32 (N, K) - conv2d_i8(..., want_out=True) followed by global_avgpool, bit for bit - or
    `(pooled or None, codes)` with `emit`."""
    o = _operand(dict(codes=codes, wq=wq, wsum=wsum, bias=bias, in_scale=in_scale, in_zp=in_zp, w_scale=w_scale))
    codes = o.codes
    if codes.dim() != 4 or tuple(wq.shape[1:3]) != (1, 1):
        raise ValueError("conv2d_i8_gap: 4-D activation codes and a 1 x 1 layer [K, 1, 1, C]")
    if not want_out and emit is None:
        raise ValueError("conv2d_i8_gap: nothing to produce (want_out=False without emit)")
    (n, K_), (h, w_, c, _, _, _, _, _, uns) = o.shape[:2], o.geom
    if residual is not None:
        if tuple(residual.shape) != tuple(o.shape) or residual.dtype != torch.float32:
            raise ValueError("conv2d_i8_gap: residual must be fp32 of the convolution output's shape")
        N.require_gpu(residual)
        residual = _nhwc(residual)

    def alloc(dtype):
        return torch.empty((n, K_), dtype=dtype, device=codes.device)
    out = alloc(torch.float32) if want_out else None
    q = _quantiser(emit, alloc, codes, True, "conv2d_i8_gap")
    m = n * h * w_
    nbytes = codes.numel() + wq.numel() + m * K_ * 4 * (residual is not None) + n * K_ * (4 * want_out + (emit is not None))

    def call(extra=0):
        return N.lib.dlmcq_conv2d_i8_nhwc_gap(*_head(o, out), n, h, w_, c, K_, uns, N.ptr(residual), _act(False, act), *_q_args(q, extra),
                                              N.stream_ptr())
    tag = N.ROUTE_TAG[N.route(call(N.ROUTE_ONLY))] if PROFILE.enabled else "conv_gap"
    PROFILE.launch(tag, nbytes, lambda: N.check(call()), 2 * m * K_ * c)
    return (out, q[0]) if emit is not None else out


def pack_int4(codes):
    N.require_gpu(codes)
    codes = codes.contiguous().view(torch.int8)
    n = codes.numel()
    packed = torch.empty((n + 1) // 2, dtype=torch.uint8, device=codes.device)
    N.check(N.lib.dlmcq_pack_int4(N.ptr(codes), N.ptr(packed), n, N.stream_ptr()))
    return packed


def unpack_int4(packed, n, signed, out=None):
    """Packed 4-bit codes (element 2i in the low nibble) -> one byte per code (dlmcq_unpack_int4).  `out`: an int8 / uint8 buffer
    of >= n elements to expand into (the frozen plan expands all its 4-bit weights into one scratch buffer per step)."""
    N.require_gpu(packed)
    if out is None:
        codes = torch.empty(n, dtype=torch.int8, device=packed.device)
    else:
        N.require_gpu(out)
        if out.numel() < n or out.element_size() != 1 or not out.is_contiguous():
            raise ValueError("unpack_int4: out must be a contiguous byte tensor of at least n elements")
        codes = out.view(torch.int8)
    PROFILE.launch("unpack_int4", (n + 1) // 2 + n,
                   lambda: N.check(N.lib.dlmcq_unpack_int4(N.ptr(packed.contiguous()), N.ptr(codes), n, int(bool(signed)), N.stream_ptr())))
    return codes if signed else codes.view(torch.uint8)


def fake_quant_backward(x, gy, scale, offset, lo, hi, g, ch_axis=None, want_gx=True, want_gscale=True, form=None):
    """Backward of FORM_QBASE (default), FORM_ZEROPOINT, FORM_SYMMETRIC or FORM_ROOTQ_ACT: (gx, gscale[C]) - gx bit-exact
    with autograd, gscale a deterministic tree sum."""
    N.require_gpu(x, gy)
    x, gy = x.contiguous(), gy.contiguous()
    scale, offset = _f32c(scale, x), _f32c(offset, x)
    outer, ch, inner = geometry(x, scale, ch_axis)
    if offset is not None and offset.numel() != scale.numel():
        offset = offset.reshape(1).expand(scale.numel()).contiguous()
    gx = torch.empty_like(x) if want_gx else None
    gs = torch.empty(ch, dtype=torch.float32, device=x.device) if want_gscale else None
    nb = N.lib.dlmcq_fq_bwd_scratch_bytes(outer, ch, inner)
    sc = _scratch(nb, x.device)
    # algorithmic bytes: x and gy read, gx written (12 per element; 8 when only the scale gradient is wanted)
    PROFILE.launch("fq_bwd", x.numel() * (8 + 4 * bool(want_gx)), lambda: N.check(N.lib.dlmcq_fake_quant_bwd_form_f32(
        N.ptr(x), N.ptr(gy), N.ptr(gx), N.ptr(gs), N.ptr(scale), N.ptr(offset), outer, ch, inner, int(lo), int(hi),
        int(N.FORM_QBASE if form is None else form), float(g), N.ptr(sc), sc.numel() * 4, N.stream_ptr())))
    return gx, gs


# ------------------------------------------------------ many tensors, one launch (csrc/fake_quant_multi.hip)
_MULTI_FORMS = (FORM_QBASE, FORM_ZEROPOINT, FORM_SYMMETRIC)


class Segment:
    """One tensor with its quantiser, as `fake_quant_multi` takes it: per tensor (a one-element scale) or per channel on axis 0.
    Nothing is copied - the launches read `x` and `scale` where they lie - so `x` must be fp32 and contiguous already."""
    __slots__ = ("x", "scale", "offset", "lo", "hi", "form", "g", "channels", "inner")

    def __init__(self, x, scale, offset, lo, hi, form, g=0.0):
        if x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError("fake_quant_multi: a segment is fp32 and contiguous")
        if int(form) not in _MULTI_FORMS:
            raise ValueError("fake_quant_multi: forms QBASE, ZEROPOINT and SYMMETRIC only")
        scale, offset = _f32c(scale.detach(), x), _f32c(offset, x)
        outer, ch, inner = geometry(x, scale)
        if ch > 1 and outer != 1:
            raise ValueError("fake_quant_multi: per-channel segments have their channel on axis 0")
        if offset is not None and offset.numel() != scale.numel():
            if offset.numel() != 1:
                raise ValueError("offset must have one entry per scale entry")
            offset = offset.reshape(1).expand(scale.numel()).contiguous()
        self.x, self.scale, self.offset = x.detach(), scale, None if form == FORM_SYMMETRIC else offset
        self.lo, self.hi, self.form, self.g = int(lo), int(hi), int(form), float(g)
        self.channels, self.inner = ch, (inner if ch > 1 else x.numel())

    def fill(self, rec):
        """The caller's fields of one dlmcq_fq_segment (the pointers of the outputs stay 0)."""
        rec.x, rec.scale = self.x.data_ptr(), self.scale.data_ptr()
        rec.offset = 0 if self.offset is None else self.offset.data_ptr()
        rec.y = rec.gy = rec.gx = rec.gscale = 0
        rec.n, rec.channels, rec.inner = self.x.numel(), self.channels, self.inner
        rec.lo, rec.hi, rec.ste_g, rec.form = self.lo, self.hi, self.g, self.form


def _prepare(table, nseg):
    f, b, z, sc = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_size_t(0)
    rc = N.lib.dlmcq_fq_multi_prepare(ctypes.byref(table), nseg, ctypes.byref(f), ctypes.byref(b), ctypes.byref(z), ctypes.byref(sc))
    return rc, f.value, b.value, z.value, sc.value


def segment_refusal(seg):
    """None when the library takes `seg` in a segment table, else why not (dlmcq_fq_multi_prepare's verdict; host only)."""
    table = (N.FqSegment * 1)()
    seg.fill(table[0])
    rc = _prepare(table, 1)[0]
    return None if rc == 0 else N.lib.dlmcq_strerror(rc).decode()


def _carve(sizes, device, pad=4):
    """One fp32 arena and a view of sizes[i] elements per entry, each starting on a 16-byte boundary."""
    offs, total = [], 0
    for n in sizes:
        offs.append(total)
        total += (n + pad - 1) // pad * pad
    arena = torch.empty(max(total, pad), dtype=torch.float32, device=device)
    return arena, [arena[o:o + n] for o, n in zip(offs, sizes)]


def _aligned(t):
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class FqMultiPlan:
    """A list of segments as device tables: the forward table is built and uploaded once (weights, scales and the outputs - an
    arena this object owns unless `out` names them - keep their addresses across steps), the backward's per call (gy and gx are
    new tensors every step)."""

    def __init__(self, segments, out=None, forward=True):
        self.segments = list(segments)
        self.nseg = len(self.segments)
        N.require_gpu(*[s.x for s in self.segments])
        self.device = self.segments[0].x.device if self.segments else torch.device("cuda")
        self.numel = sum(s.x.numel() for s in self.segments)
        self._host = (N.FqSegment * max(self.nseg, 1))()
        for s, rec in zip(self.segments, self._host):
            s.fill(rec)
        self.arena, self.ys, self._fwd_table, self._bwd_table, self.fwd_workgroups = None, None, None, None, 0
        if not forward:
            return
        if out is None:
            self.arena, flat = _carve([s.x.numel() for s in self.segments], self.device)
            self.ys = [y.view(s.x.shape) for y, s in zip(flat, self.segments)]
        else:
            self.ys = list(out)
            for y, s in zip(self.ys, self.segments):
                if not (y.dtype == torch.float32 and y.shape == s.x.shape and y.is_contiguous() and y.device == s.x.device):
                    raise ValueError("out must hold contiguous fp32 tensors of the segments' shapes")
        for y, rec in zip(self.ys, self._host):
            rec.y = y.data_ptr()
        rc, self.fwd_workgroups = _prepare(self._host, self.nseg)[:2]
        N.check(rc)
        self._fwd_table = self._upload(self._host)

    def _upload(self, table):
        """The table on the device, through a pinned staging buffer: a copy from pageable memory would make the host wait for
        everything queued on the stream - in the middle of a backward pass.  (The pinned allocator keeps the buffer until the
        copy has run.)"""
        host = torch.empty(ctypes.sizeof(table) // 8, dtype=torch.int64, pin_memory=True)
        ctypes.memmove(host.data_ptr(), table, ctypes.sizeof(table))
        return host.to(self.device, non_blocking=True)

    def forward(self):
        """One launch; returns the outputs (the same storage every call)."""
        if self.arena is not None:
            torch.autograd.graph.increment_version(self.arena)   # a graph that still holds last step's outputs must say so
        if self.fwd_workgroups:
            PROFILE.launch("fq_multi", 8 * self.numel, lambda: N.check(N.lib.dlmcq_fake_quant_multi_f32(
                N.ptr(self._fwd_table), self.nseg, self.fwd_workgroups, N.stream_ptr())))
        return [y.detach() for y in self.ys]

    def backward(self, gys, want_gx=True, want_gscale=True, gx_out=None, gscale_out=None, scratch=None):
        """One backward launch and one finalize.  `gys[i]` None: segment i takes no part.  Returns (gxs, gscales), with None
        where nothing was wanted or computed; gscales are [channels]."""
        wx = list(want_gx) if isinstance(want_gx, (list, tuple)) else [bool(want_gx)] * self.nseg
        ws = list(want_gscale) if isinstance(want_gscale, (list, tuple)) else [bool(want_gscale)] * self.nseg
        live = [g is not None and (a or b) for g, a, b in zip(gys, wx, ws)]
        gys = [_aligned(g) if l else None for g, l in zip(gys, live)]
        for g, s, l in zip(gys, self.segments, live):
            if l and (g.dtype != torch.float32 or g.shape != s.x.shape):
                raise ValueError("fake_quant_multi_backward: gy must be fp32 with the segment's shape")
        gxs, gss = [None] * self.nseg, [None] * self.nseg
        if gx_out is None:
            idx = [i for i in range(self.nseg) if live[i] and wx[i]]
            flat = _carve([self.segments[i].x.numel() for i in idx], self.device)[1]
            for i, t in zip(idx, flat):
                gxs[i] = t.view(self.segments[i].x.shape)
        else:
            gxs = [t if (l and w) else None for t, l, w in zip(gx_out, live, wx)]
        if gscale_out is None:
            idx = [i for i in range(self.nseg) if live[i] and ws[i]]
            flat = _carve([self.segments[i].channels for i in idx], self.device, pad=1)[1]
            for i, t in zip(idx, flat):
                gss[i] = t
        else:
            gss = [t if (l and w) else None for t, l, w in zip(gscale_out, live, ws)]
        table = (N.FqSegment * max(self.nseg, 1))()
        ctypes.memmove(table, self._host, ctypes.sizeof(table))
        nbytes = 0
        for rec, g, gx, gs, s in zip(table, gys, gxs, gss, self.segments):
            rec.y = 0
            rec.gy = 0 if g is None else g.data_ptr()
            rec.gx = 0 if gx is None else gx.data_ptr()
            rec.gscale = 0 if gs is None else gs.data_ptr()
            if g is not None:
                nbytes += s.x.numel() * (12 if gx is not None else 8)
        rc, _, bwd, fin, need = _prepare(table, self.nseg)
        N.check(rc)
        if bwd or fin:
            sc = scratch if scratch is not None else _scratch(need, self.device)
            raw = bytes(table)      # in the steady state the allocator hands out last step's addresses: the same table
            if self._bwd_table is None or self._bwd_table[0] != raw:
                self._bwd_table = (raw, self._upload(table))
            dev = self._bwd_table[1]
            PROFILE.launch("fq_multi_bwd", nbytes, lambda: N.check(N.lib.dlmcq_fake_quant_multi_bwd_f32(
                N.ptr(dev), self.nseg, bwd, fin, N.ptr(sc), sc.numel() * 4, N.stream_ptr())))
        return gxs, gss


def fake_quant_multi(segments, out=None):
    """Fake-quantise every tensor of `segments` in ONE launch; the outputs (dequantised fp32) are the bits of `fake_quant` on each."""
    return FqMultiPlan(segments, out=out).forward()


def fake_quant_multi_backward(segments, gys, want_gx=True, want_gscale=True, gx_out=None, gscale_out=None, scratch=None):
    """The backward of every segment in one launch plus one finalize: ([gx], [gscale]), the bits of `fake_quant_backward` on each."""
    return FqMultiPlan(segments, forward=False).backward(gys, want_gx, want_gscale, gx_out, gscale_out, scratch)


def rootq_weight(w, upper, lower, lo, hi):
    """RootQ weight forward; `upper`/`lower` are 0-dim (or 1-element) device tensors."""
    N.require_gpu(w)
    w = w.contiguous()
    bounds = torch.stack([upper.detach().reshape(()).float(), lower.detach().reshape(()).float()]).to(w.device)
    y = torch.empty_like(w)
    N.check(N.lib.dlmcq_rootq_weight_f32(N.ptr(w), N.ptr(y), N.ptr(bounds), w.numel(), int(lo), int(hi), N.stream_ptr()))
    return y


def rootq_weight_backward(w, gy, upper, lower, alpha, lo, hi, want_gw=True):
    """Backward of rootq_weight: (gw or None, g_upper, g_lower, g_alpha) - 0-dim tensors for the three scalars."""
    N.require_gpu(w, gy)
    w, gy = w.contiguous(), gy.contiguous()
    bounds = torch.stack([upper.detach().reshape(()).float(), lower.detach().reshape(()).float()]).to(w.device)
    al = alpha.detach().reshape(1).float().to(w.device)
    gw = torch.empty_like(w) if want_gw else None
    out = torch.empty(3, dtype=torch.float32, device=w.device)
    sc = _scratch(N.lib.dlmcq_rootq_bwd_scratch_bytes(w.numel()), w.device)
    N.check(N.lib.dlmcq_rootq_weight_bwd_f32(N.ptr(w), N.ptr(gy), N.ptr(gw), N.ptr(out), N.ptr(bounds), N.ptr(al), w.numel(), int(lo),
                                             int(hi), N.ptr(sc), sc.numel() * 4, N.stream_ptr()))
    return gw, out[0], out[1], out[2]

