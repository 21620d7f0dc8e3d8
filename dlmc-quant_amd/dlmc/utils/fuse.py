"""Frozen-network execution plan: fold what FOLLOWS each quantised layer into that layer's int8 kernel.

In the reference every wrapper is an island (`modules/conv.py:13-19`, `FSPTQuant/base.py:95-159`): it reads an
fp32 activation, fake-quantises it, convolves, and writes an fp32 activation which a ReLU module re-reads and
re-writes, a residual add re-reads and re-writes, and the next wrapper re-reads to quantise again.  Once the
scales are frozen (after calibration / PTQ - the state `post_training_quantization.py:77` evaluates in) none of
those trips through HBM is needed: the value that leaves the matrix-core accumulator can be dequantised, added to
the shortcut, rectified and turned into the NEXT layer's activation code while it is still in a register
(`dlmcq_conv2d_i8_nhwc_fused`).  Arithmetic and order are those of the separate kernels, so the codes - and hence
every downstream value - are bit-identical to the unfused wrappers; only the memory traffic changes.

    model = ...; quantize_model(model, cfg, logger, "FSPTQ"); model(calib_batch)      # calibrated, on the GPU
    fused = fuse_inference(model)            # torch.fx GraphModule over the same parameters
    y = fused(x)                             # == model(x) bit for bit (up to the sign of zero)

`torch.fx` is used once, as a dataflow reader (which ReLU / add / wrapper consumes which tensor); execution is the
explicit HIP launches of the plan, and the result can be captured with `dlmc.utils.graph.GraphedForward`.
The plan snapshots weights and scales: re-fuse after changing them.
"""
import collections
import functools
import math
import os
import operator

import torch
import torch.fx as fx
import torch.nn.functional as F
from torch import nn

from .. import _native as N
from ..quantization.scalar import kernels as K
from ..quantization.scalar._wrapper import int8_kind, ste_scale_value
from ..quantization.scalar.FSPTQuant.base import FSPTQBase
from ..quantization.scalar.modules.base import QBase
from ..quantization.scalar.RootQ.base import RootQBase

__all__ = ["fuse_inference", "StreamedPlan", "Int8Layer", "DualInt8Layer", "StemLayer", "GapLayer", "GapHeadLayer", "AvgPoolLayer", "GateLayer", "SqueezeLayer", "SwishLayer", "HardswishLayer", "LayerNormLayer", "GeluLayer", "AttentionLayer", "FusionReport"]


# ---------------------------------------------------------------------------------- frozen quantiser specs
class _ActSpec:
    """One wrapper's frozen activation quantiser, as a producer has to evaluate it."""

    def __init__(self, scale, zp, lo, hi, form, needs_g, xoff=False):
        self.scale, self.zp, self.lo, self.hi, self.form, self.needs_g = scale, zp, int(lo), int(hi), form, needs_g
        # xoff (fuse_inference(act_offsets=True)): `zp` is a QBase FLOAT offset o (x^ = q * s^ + o), not an integer zero point.  It is
        # what quantises and emits this tensor's codes (q = R(clamp((x - o) / s^))); the consumer's kernel sees zero point 0, o * (weight
        # sums) folded into its bias and, for padded layers, the border term of the *_xoff entry points
        self.xoff = bool(xoff)
        self.key = (form, self.lo, self.hi, float(scale.reshape(-1)[0]), 0.0 if zp is None else float(zp.reshape(-1)[0]),
                    needs_g)
        # what a PRODUCER is told: a zero point of 0 (every post-ReLU tensor) goes as "none" - the kernels' plain-quantiser paths
        # (csrc/conv_epilogue.h epi_plain) key on the null pointer (read once, when the plan is built)
        self.zp_emit = None if self.key[4] == 0.0 else zp

    def g(self, numel):
        return 1 / math.sqrt(numel * self.hi) if self.needs_g else 0.0

    def emit(self, numel):
        return K.EmitCodes(self.scale, self.zp_emit, self.lo, self.hi, self.form, self.g(numel))


def _byte_range(lo, hi):
    return (0 <= lo and hi <= 255) or (-128 <= lo and hi <= 127)


def _ceil64(n):
    return (n + 63) // 64 * 64


def plan_kind(mod):
    """Which kernel of the frozen plan runs `mod`: "gemm" = conv_i8.hip (dense conv / linear; channel counts that are no
    multiple of 64 are zero-padded when the plan is built), "stem" = conv_stem_i8.hip (<= 4 input channels), "dw" =
    conv_dw_i8.hip (depthwise), or None."""
    k = int8_kind(mod)
    if k is not None:
        return k
    w = mod.weight
    sq = lambda t: len(set(t)) == 1  # noqa: E731
    if w.dim() != 4 or mod.padding_mode != "zeros" or isinstance(mod.padding, str) or not (sq(mod.stride) and sq(mod.padding)):
        return None
    if tuple(mod.dilation) != (1, 1):
        return None
    if mod.groups == 1 and w.shape[1] % 4 == 0 and w.shape[1] > 4:
        return "gemm"
    if mod.groups == w.shape[0] and w.shape[1] == 1 and w.shape[0] % 4 == 0 and w.shape[2] <= 7 and w.shape[3] <= 7:
        return "dw"
    return None


class _LayerSpec(collections.namedtuple("_LayerSpec", "act w_scale w_lo w_hi kind w_off w_codes", defaults=(None, None))):
    """The frozen quantisers of one layer that can run on an int8 kernel: `act` (_ActSpec), the weight scale and code range, `kind`
    (plan_kind).  `w_off`, `w_codes`: None for symmetric per-tensor / per-channel weights quantised by quantize_weight_krsc; asymmetric
    (offset = channel minimum, ops.py:129-136) or QBase per-channel weights carry their float offsets [K] and a function returning the
    module's own integer codes [K, C, R, S]."""

    @property
    def symmetric(self):
        """Symmetric weights: no offset term (the dual, pooling first-layer and fused-head kernels have none)."""
        return self.w_off is None

    def with_codes(self, fn):
        """The same quantisers, the weight codes coming from `fn()` (an integer checkpoint) instead of the fp32 weights."""
        return self._replace(w_codes=fn)


def _border_term(act, mod):
    """A float activation offset in front of a padded convolution: the layer needs the border term of the *_xoff entry points (which
    have no narrow, dual or pad-shortcut form)."""
    return bool(act.xoff and mod.weight.dim() == 4 and int(mod.padding[0]) > 0)


def _zp_fill(act):
    """The code that pads an activation's channels for the kernels: its zero point; a float offset has none and pads with code 0."""
    return 0 if (act.xoff or act.zp is None) else int(float(act.zp.reshape(-1)[0]))


def _takes_shifted(spec, mod, dwpw=False):
    """Whether plan convolution `mod` (its spec; None: not a plan layer of its own) reads an unsigned-byte quantiser's codes re-centred
    (`code - 128`, see _PlanLayer.__init__) as they are: a matrix-core layer without channel padding."""
    if spec is None or mod is None or mod.weight.dim() != 4:
        return False
    if spec.kind == "dw":      # the matrix-core depthwise kernel (csrc/conv_dwm_i8.hip) multiplies signed bytes: no re-centring of its fragments
        # (not with `dwpw`: the fused unit's kernel emits plain codes only)
        return not dwpw and mod.kernel_size == (3, 3) and mod.stride == (1, 1) and mod.padding == (1, 1) and mod.weight.shape[0] % 64 == 0
    return spec.kind == "gemm" and mod.groups == 1 and mod.weight.shape[1] % 64 == 0


def _emits_shifted(emit, readers, dwpw=False):
    """Whether a producer hands quantiser `emit`'s codes over re-centred: an unsigned-byte quantiser whose every reader - (spec, module),
    (None, None) for an operand of a dual node - takes them so."""
    return bool(emit is not None and 0 <= emit.lo and emit.hi <= 255 and readers and all(_takes_shifted(s, m, dwpw) for s, m in readers))


def _frozen_spec(mod, act_offsets=False):
    """The _LayerSpec of `mod` if it can run on an int8 kernel with frozen scales, else None."""
    kind = plan_kind(mod)
    if kind is None:
        return None
    if isinstance(mod, FSPTQBase):
        return _fsptq_spec(mod, kind)
    return _qbase_spec(mod, kind, act_offsets) if isinstance(mod, QBase) else None


def _xoff_kernel_exists(mod, kind):
    """Whether a layer whose input quantiser has a float offset has a kernel with the border term (include/dlmcq.h, the *_xoff entry
    points).  Unpadded layers need none (the folded bias is the whole term); padded depthwise layers need a 3 x 3 filter (the vector
    kernels, <= 2048 channels once padded to 64), padded first layers a 3 x 3 or 7 x 7 one.  Anything else keeps its fp32 path."""
    w = mod.weight
    if w.dim() != 4 or int(mod.padding[0]) == 0 or kind == "gemm":
        return True
    if kind == "dw":
        return tuple(w.shape[2:]) == (3, 3) and _ceil64(w.shape[0]) <= 2048
    return w.shape[2] in (3, 7)          # "stem"


def _takes_dw5(spec, mod):
    """Whether a planned layer runs on the 5 x 5 depthwise kernel under fuse_inference(dw5=True): a depthwise 5 x 5 filter with padding 2
    and stride 1 or 2 in both axes, at most 2048 channels once padded to 64, an input quantiser without a float offset (that kernel has no
    border term: such a padded 5 x 5 layer is not planned at all, _xoff_kernel_exists), and no shape measured slower (K.dw5_profitable)."""
    w = mod.weight
    if spec.kind != "dw" or spec.act.xoff or w.dim() != 4 or tuple(w.shape[2:]) != (5, 5):
        return False
    if len(set(mod.stride)) != 1 or len(set(mod.padding)) != 1 or tuple(getattr(mod, "dilation", (1, 1))) != (1, 1):
        return False
    return K.dw5_supported(_ceil64(w.shape[0]), mod.stride[0], mod.padding[0], 5)


def _fsptq_spec(mod, kind):
    if not (mod.act_quant and mod.wt_quant) or mod.in_scale.numel() != 1:
        return None
    if mod.qconfig["weight"].get("recon_type") in ("adaround", "dist_recon"):
        return None
    if not (mod._init.ready(mod, "in_init_state") and mod._init.ready(mod, "wt_init_state")):
        raise RuntimeError("fuse_inference: run a calibration forward first (scales are not initialised)")
    if not (_byte_range(mod.in_min_val, mod.in_max_val) and -128 <= mod.wt_min_val and mod.wt_max_val <= 127):
        return None
    zp = mod.in_offset.detach().to(torch.float32).reshape(-1)[:1].clone()
    z = float(zp[0])
    if z != round(z) or not (mod.in_min_val <= z <= mod.in_max_val):
        return None
    act = _ActSpec(mod.in_scale.detach().reshape(-1)[:1].clone(), zp, mod.in_min_val, mod.in_max_val, N.FORM_ZEROPOINT, False)
    return _LayerSpec(act, mod.wt_scale.detach().clone(), mod.wt_min_val, mod.wt_max_val, kind)


def _qbase_spec(mod, kind, act_offsets):
    cfg = mod.qconfig
    if not (cfg["input"]["enable"] and cfg["weight"]["enable"]):
        return None
    k = mod.weight.shape[0]
    per_channel = mod.wt_scale.numel() != 1
    if mod.in_scale.numel() != 1 or (per_channel and (mod.wt_scale.numel() != k or mod.wt_scale.shape[0] != k)):
        return None
    if not (mod._init.ready(mod, "in_init_state") and mod._init.ready(mod, "wt_init_state")):
        raise RuntimeError("fuse_inference: run a calibration forward first (scales are not initialised)")
    lo, hi = mod.wt_min_val, mod.wt_max_val
    if not (_byte_range(mod.in_min_val, mod.in_max_val) and _byte_range(lo, hi)):
        return None
    xoff = float(mod.in_offset.abs().max()) != 0
    if xoff and not (act_offsets and mod.in_offset.numel() == 1 and _xoff_kernel_exists(mod, kind)):
        return None                  # a float activation offset has no integer zero point (padding must be a code): act_offsets=True
    asym = mod.wt_offset is not None and float(mod.wt_offset.abs().max()) != 0
    act = _ActSpec(mod.in_scale.detach().reshape(-1)[:1].clone(),
                   mod.in_offset.detach().to(torch.float32).reshape(-1)[:1].clone() if xoff else None, mod.in_min_val, mod.in_max_val,
                   N.FORM_QBASE, True, xoff=xoff)
    g_w = 1 / math.sqrt(mod.weight.numel() * hi)
    s_hat = ste_scale_value(mod.wt_scale, g_w).clone()
    if not (per_channel or asym or hi > 127 or kind == "dw"):
        return _LayerSpec(act, s_hat, lo, hi, kind)
    w_off = mod.wt_offset.detach().to(torch.float32).reshape(-1).clone() if asym else None

    def codes(mod=mod, g_w=g_w, lo=lo, hi=hi):      # the module's own weight quantiser (form QBASE), as integers
        off = mod.wt_offset if mod.wt_offset is not None else None
        return K.fake_quant(mod.weight.detach(), mod.wt_scale.detach(), off, lo, hi, N.FORM_QBASE, g=g_w, codes="i8",
                            want_y=False)[1]
    return _LayerSpec(act, s_hat, lo, hi, kind, w_off, codes)


# -------------------------------------------------------------------------------------------- plan nodes
class _PlanLayer(nn.Module):
    """Common part of the plan nodes: frozen quantiser constants, the consumer's emit spec, pooling on codes."""

    def __init__(self, layer, spec, **decided):
        super().__init__()
        self._structure(layer, spec, **decided)
        self.w_lo, self.w_hi, self._w_codes = spec.w_lo, spec.w_hi, spec.w_codes
        w_scale = spec.w_scale.detach().to(torch.float32).reshape(-1)
        w_scale = w_scale.expand(self.k) if w_scale.numel() == 1 else w_scale
        self.register_buffer("w_scale", self._padk(w_scale, 1.0), persistent=False)
        self.register_buffer("bias_pad", None if layer.bias is None or self.k_pad == self.k else self._padk(layer.bias.detach().float(), 0.0),
                             persistent=False)
        # the zero point the KERNELS see: a float offset (act.xoff) is none - its codes pad with code 0 and its term is in the bias / border
        self._kzp = None if self.act.xoff else self.act.zp
        self._zp_fill = _zp_fill(self.act)   # (read once: no host sync in forward)
        # A producer may hand an unsigned-byte quantiser's codes over as int8 `code - 128` (EmitCodes.shift128: what the matrix
        # cores multiply anyway, so the consumer's kernel need not re-centre every operand byte it reads); this node then runs
        # with the zero point `zp - 128` - the same integers.  `emit_shift`: this node emits ITS consumers' codes that way.
        zs = None
        if self.act.lo >= 0:
            zs = (torch.zeros(1, device=w_scale.device) if self._kzp is None else self._kzp.detach().float().reshape(-1)[:1]) - 128.0
        self.register_buffer("zp_shift", zs, persistent=False)
        self._deq = {}     # QBase dequantises with s^ = grad_scale(s, g(numel)): one tiny tensor per input size
        for name in ("bias_fold", "x_off", "tap_sums"):
            self.register_buffer(name, None, persistent=False)
        self.xoff_padded = False     # the border term runs in the kernel (the *_xoff entry points)

    def _structure(self, layer, spec, relu=False, emit=None, want_out=True, pool=None, relu6=False, narrow=False, pad_shortcut=None,
                   emit_shift=False, dw5=False):
        """What the plan's passes read off a node - the layer's shape and quantisers, and what the main pass decided for it
        (_Decision.options).  The whole of a `dry_run="chains"` stand-in; needs no GPU."""
        self.layer, self.act, self.kind = layer, spec.act, spec.kind
        self.relu, self.emit, self.want_out, self.pool = bool(relu), emit, bool(want_out), pool
        # ReLU6 fused into the epilogue (DLMCQ_ACT_RELU6).  `relu` keeps meaning ReLU alone: the chain / dual / block-end decisions and
        # the kernels that know no upper bound read it, and they leave ReLU6 layers alone
        self.relu6 = bool(relu6)
        w = layer.weight
        conv, k = w.dim() == 4, w.shape[0]
        # channel counts that are no multiple of 64 (the K step of the matrix-core kernel) are zero-padded: padded output
        # channels have zero weights and bias, so their value is 0 and their code is the consumer's code of 0
        self.k, self.k_pad = k, (_ceil64(k) if self.kind in ("gemm", "dw") and conv else k)
        self.c = k if self.kind == "dw" else w.shape[1]       # (depthwise: one input channel per output channel)
        if self.kind != "stem":
            self.c_pad = _ceil64(self.c) if conv else self.c
        w_off = spec.w_off
        if w_off is not None:
            w_off = self._padk((w_off.expand(k) if w_off.numel() == 1 else w_off).to(spec.w_scale.device), 0.0)
        self.register_buffer("w_off", w_off, persistent=False)
        # narrow fp32 rows (fuse_inference(narrow_rows=True); Int8Layer only): a channel-padded layer reads its fp32 shortcut and writes its
        # fp32 output k wide - dense, no slice on the way out - while its codes stay k_pad wide (dlmcq_conv2d_i8_nhwc_narrow)
        self.narrow = bool(narrow)
        # a pad shortcut (fuse_inference(pad_shortcuts=True); Int8Layer only): (stride, leading zero channels) of an option-A shortcut
        # `F.pad(x[:, :, ::s, ::s], (0, 0, 0, 0, lo, hi))` - the node's second argument is then the SOURCE x, read in place by the
        # epilogue (K.PadShortcut, dlmcq_conv2d_i8_nhwc_padres: the narrow path, at k == k_pad too)
        self.pad_shortcut = pad_shortcut
        self.emit_shift = bool(emit_shift)      # (see __init__; stand-ins: False - the chain pass clears it anyway)
        # the 5 x 5 integer dot-product kernel (fuse_inference(dw5=True); DwInt8Layer only): K.conv2d_dw5_i8 instead of K.conv2d_dw_i8
        self.dw5 = bool(dw5)

    def _fold_offset(self, tap):
        """A float activation offset o (act.xoff): `tap` [k_pad, R, S] (float64, on the device) = per output channel and tap the sum of the
        dequantised weights over the REAL input channels.  o * SUM_{taps} tap goes into the bias (float64, rounded once); a padded layer
        keeps the fp32 taps [R * S, k_pad] for its border term."""
        o = self.act.zp.detach().to(torch.float64).reshape(-1)[:1].to(tap.device)
        b = torch.zeros(self.k_pad, dtype=torch.float64, device=tap.device)
        if self.layer.bias is not None:
            b[:self.k] = self.layer.bias.detach().to(torch.float64).reshape(-1)
        self.register_buffer("bias_fold", (b + o * tap.sum(dim=(1, 2))).to(torch.float32).contiguous(), persistent=False)
        self.register_buffer("x_off", self.act.zp.detach().to(torch.float32).reshape(-1)[:1].to(tap.device).contiguous(), persistent=False)
        lay = self.layer
        self.xoff_padded = _border_term(self.act, lay)
        if self.xoff_padded:
            self.register_buffer("tap_sums", tap.permute(1, 2, 0).reshape(-1, tap.shape[0]).to(torch.float32).contiguous(), persistent=False)

    def _xoff_kw(self):
        return dict(in_offset=self.x_off, tap_sums=self.tap_sums) if self.xoff_padded else {}

    def _padk(self, v, fill):
        v = v.detach().reshape(-1)
        if self.k_pad == v.numel():
            return v.contiguous()
        return torch.cat([v, torch.full((self.k_pad - v.numel(),), fill, dtype=v.dtype, device=v.device)]).contiguous()

    def _bias(self):
        if self.bias_fold is not None:
            return self.bias_fold
        return self.layer.bias if self.bias_pad is None else self.bias_pad

    def _in_scale(self, numel):
        if not self.act.needs_g:
            return self.act.scale
        s = self._deq.get(numel)
        if s is None:
            s = self._deq[numel] = ste_scale_value(self.act.scale, self.act.g(numel)).contiguous()
        return s

    def _emit_for(self, n, k, p, q):
        """The consumer's quantiser; its g (QBase) is taken over ITS input = this node's (pooled) output."""
        if self.emit is None:
            return None
        if self.pool is not None:
            kk, ss, pp = self.pool
            p, q = (p + 2 * pp - kk) // ss + 1, (q + 2 * pp - kk) // ss + 1
        e = self.emit.emit(n * k * p * q)
        e.shift128 = self.emit_shift
        return e

    def _zp(self, codes):
        """The zero point that goes with `codes`: int8 codes of an unsigned quantiser are shifted codes (see __init__)."""
        return self.zp_shift if (codes.dtype == torch.int8 and self.act.lo >= 0) else self._kzp

    def _act_arg(self):
        """The layer's activation as the kernels' `act` argument (DLMCQ_ACT_*)."""
        return N.ACT_RELU6 if self.relu6 else (N.ACT_RELU if self.relu else N.ACT_NONE)

    def _finish(self, out, codes):
        if self.pool is not None:
            codes = K.maxpool_codes(codes, *self.pool)
        if out is not None and self.k_pad != self.k and not self.narrow:
            out = out[:, :self.k]          # fp32 leaves the plan: drop the padding channels (codes stay padded for plan consumers)
        return out, codes


def _pad_channels(codes, c_pad, fill):
    """Activation codes (N, C, H, W) channels_last -> (N, c_pad, H, W), the new channels holding `fill` (the code of 0)."""
    n, c, h, w = codes.shape
    if c == c_pad:
        return codes
    out = torch.full((n, c_pad, h, w), fill, dtype=codes.dtype, device=codes.device).contiguous(memory_format=torch.channels_last)
    out[:, :c] = codes
    return out


def _weight_codes(node):
    """Integer weight codes [K, C, R, S] (int16) of a plan node whose spec carries its own quantiser, with codes above 127
    re-centred (qw - 128, offset + 128 * s: the matrix cores multiply signed bytes)."""
    q = node._w_codes().to(torch.int16)
    if q.dim() == 2:
        q = q[:, :, None, None]
    if node.w_hi > 127:
        q = q - 128
        shift = 128.0 * node.w_scale[:node.k]
        base = node.w_off[:node.k] if node.w_off is not None else torch.zeros_like(shift)
        node.w_off = node._padk(base + shift, 0.0)
    return q


class Int8Layer(_PlanLayer):
    """One quantised conv / linear of the frozen plan (input channels % 64 == 0).  Input: the producer's codes
    (uint8/int8) or an fp32 tensor (quantised here, one pass).  Output: `(fp32 or None, consumer codes or None)`."""

    def __init__(self, layer, spec, **kw):
        super().__init__(layer, spec, **kw)
        w = layer.weight.detach()
        c = self.c
        if self._w_codes is None and self.c_pad == c and self.k_pad == self.k:
            wq, wsum = K.quantize_weight_krsc(w, self.w_scale, self.w_lo, self.w_hi)
        else:
            if self._w_codes is not None:
                q = _weight_codes(self)                                            # [K, C, R, S] int16
            else:
                q4 = w if w.dim() == 4 else w[:, :, None, None]
                q = K.quantize_weight_krsc(q4, self.w_scale[:self.k], self.w_lo, self.w_hi)[0].permute(0, 3, 1, 2).to(torch.int16)
            full = torch.zeros((self.k_pad, self.c_pad) + tuple(q.shape[2:]), dtype=torch.int16, device=q.device)
            full[:self.k, :c] = q
            wq = full.permute(0, 2, 3, 1).contiguous().to(torch.int8)                # KRSC
            wsum = full.sum(dim=(1, 2, 3)).to(torch.int32).contiguous()
        self.register_buffer("wq", wq, persistent=False)
        self.register_buffer("wsum", wsum, persistent=False)
        if self.act.xoff:
            q = wq.reshape(self.k_pad, -1, self.c_pad)[:, :, :c].to(torch.float64)               # [K, R * S, real C]
            tap = q.sum(dim=2) * self.w_scale.to(torch.float64)[:, None]
            if self.w_off is not None:
                tap = tap + c * self.w_off.to(torch.float64)[:, None]
            r, s_ = (w.shape[2], w.shape[3]) if w.dim() == 4 else (1, 1)
            self._fold_offset(tap.reshape(self.k_pad, r, s_))

    def _codes(self, x):
        """The activation codes of `x` (already codes, or fp32 quantised here in one pass), channel-padded for the kernel."""
        act = self.act
        if x.dtype not in (torch.uint8, torch.int8):
            N.require_gpu(x)
            if x.dim() == 4 and not x.is_contiguous(memory_format=torch.channels_last):
                x = x.contiguous(memory_format=torch.channels_last)
            x = K.fake_quant(x, act.scale, act.zp, act.lo, act.hi, act.form, g=act.g(x.numel()), codes="i8", want_y=False)[1]
        c_pad = getattr(self, "c_pad", x.shape[1])
        if x.dim() == 4 and x.shape[1] != c_pad:
            x = _pad_channels(x, c_pad, self._zp_fill)
        elif act.xoff and x.dim() == 4 and self.c != c_pad and self.w_off is not None:
            # a producer's padded output channels carry ITS code of 0, which is no zero point under a float offset; the asymmetric-weight
            # term sums the codes of every channel, so they must hold code 0 (the value the tap sums assume) - in place, for every taker alike
            x[:, self.c:] = -128 if (x.dtype == torch.int8 and act.lo >= 0) else 0
        return x

    def _real_numel(self, codes):
        """Elements of the layer's real (unpadded) input: QBase's grad_scale factor is defined on it."""
        return codes.numel() // codes.shape[1] * self.c if codes.dim() == 4 else codes.numel()

    def _conv_kw(self):
        lay = self.layer
        return {} if lay.weight.dim() == 2 else dict(stride=lay.stride[0], padding=lay.padding[0], dilation=lay.dilation[0])

    def _out_hw(self, codes):
        lay = self.layer
        if lay.weight.dim() == 2:
            return 1, 1
        st, pd, dl = lay.stride[0], lay.padding[0], lay.dilation[0]
        r, s = lay.weight.shape[2], lay.weight.shape[3]
        return (codes.shape[2] + 2 * pd - dl * (r - 1) - 1) // st + 1, (codes.shape[3] + 2 * pd - dl * (s - 1) - 1) // st + 1

    def operand(self, x, codes=None):
        """This layer as an operand dict of the kernel wrappers (conv2d_i8_dual / _chain / _dual_chain); `codes`: _codes(x), when made already."""
        codes = self._codes(x) if codes is None else codes
        return dict(codes=codes, wq=self.wq, wsum=self.wsum, bias=self._bias(), in_scale=self._in_scale(self._real_numel(codes)),
                    in_zp=self._zp(codes), w_scale=self.w_scale, **self._conv_kw())

    def forward(self, x, residual=None):
        lay, act = self.layer, self.act
        linear = lay.weight.dim() == 2
        lead = None
        if linear and x.dim() != 2:
            lead = x.shape[:-1]
            x = x.reshape(-1, x.shape[-1])
            if residual is not None:
                residual = residual.reshape(-1, residual.shape[-1])
        codes = self._codes(x)
        numel = self._real_numel(codes)
        emit = self._emit_for(codes.shape[0], lay.weight.shape[0], *self._out_hw(codes))
        kw = self._conv_kw()
        if self.w_off is not None:
            kw["w_offset"] = self.w_off
        kw.update(self._xoff_kw())
        if self.narrow or self.pad_shortcut is not None:
            kw["out_channels"] = self.k
        if self.pad_shortcut is not None:
            # (a plan node's output is dense channels_last already: no copy; only an NCHW-contiguous network input is converted)
            residual = K.PadShortcut(K._nhwc(residual), *self.pad_shortcut)
        if self.relu or self.relu6 or residual is not None or emit is not None or self.w_off is not None or self.xoff_padded:
            res = K.conv2d_i8(codes, self.wq, self.wsum, self._bias(), self._in_scale(numel), self._zp(codes), self.w_scale,
                              residual=residual, act=self._act_arg(), emit=emit, want_out=self.want_out,
                              out_chunk_major=getattr(self, "out_cm", False), **kw)
            out, out_codes = res if emit is not None else (res, None)
        else:
            out, out_codes = K.conv2d_i8(codes, self.wq, self.wsum, self._bias(), self._in_scale(numel), self._zp(codes), self.w_scale, **kw), None
        if lead is not None:
            out = None if out is None else out.reshape(*lead, out.shape[-1])
            out_codes = None if out_codes is None else out_codes.reshape(*lead, out_codes.shape[-1])
        return self._finish(out, out_codes)


class DwInt8Layer(Int8Layer):
    """A depthwise convolution of the frozen plan (csrc/conv_dw_i8.hip; `dw5`: csrc/conv_dw5_i8.hip): codes in, codes (and / or fp32) out."""

    def __init__(self, layer, spec, **kw):
        _PlanLayer.__init__(self, layer, spec, **kw)
        w = layer.weight.detach()
        if self._w_codes is not None:
            q = _weight_codes(self)                                                # [C, 1, R, S]
        else:
            q = K.quantize_weight_krsc(w, self.w_scale[:self.k], self.w_lo, self.w_hi)[0].permute(0, 3, 1, 2).to(torch.int16)
        full = torch.zeros((self.k_pad,) + tuple(q.shape[2:]), dtype=torch.int16, device=q.device)
        full[:self.k] = q[:, 0]
        self.register_buffer("wq", full.permute(1, 2, 0).contiguous().to(torch.int8), persistent=False)   # [R, S, C]
        if self.act.xoff:
            tap = full.to(torch.float64) * self.w_scale.to(torch.float64)[:, None, None]             # one real input channel per output channel
            if self.w_off is not None:
                tap = tap + self.w_off.to(torch.float64)[:, None, None]
                tap[self.k:] = 0.0
            self._fold_offset(tap)

    def forward(self, x):
        lay, act = self.layer, self.act
        codes = self._codes(x)
        numel = self._real_numel(codes)
        emit = self._emit_for(codes.shape[0], self.k, *self._out_hw(codes))
        if self.dw5:      # (5 x 5 / padding 2 / no float offset: decided by the main pass)
            res = K.conv2d_dw5_i8(codes, self.wq, self._bias(), self._in_scale(numel), self._zp(codes), self.w_scale, self.w_off,
                                  stride=lay.stride[0], act=self._act_arg(), emit=emit, want_out=self.want_out)
        else:
            res = K.conv2d_dw_i8(codes, self.wq, self._bias(), self._in_scale(numel), self._zp(codes), self.w_scale, self.w_off,
                                 stride=lay.stride[0], padding=lay.padding[0], act=self._act_arg(), emit=emit, want_out=self.want_out,
                                 **self._xoff_kw())
        out, out_codes = res if emit is not None else (res, None)
        return self._finish(out, out_codes)


class DualInt8Layer(nn.Module):
    """`conv_a(x) + conv_b(y)` -> (ReLU) -> codes as ONE kernel: the last convolution of a residual block's first
    unit and the convolution on its shortcut.  Neither addend is written to memory."""

    def __init__(self, a, b):
        super().__init__()
        self.a, self.b = a, b          # `a` carries the epilogue options (relu / emit / want_out / pool)

    def forward(self, x, y):
        a = self.a
        oa, ob = a.operand(x), self.b.operand(y)
        emit = a._emit_for(oa["codes"].shape[0], a.layer.weight.shape[0], *a._out_hw(oa["codes"]))
        res = K.conv2d_i8_dual(oa, ob, relu=a.relu, emit=emit, want_out=a.want_out, out_chunk_major=getattr(self, "out_cm", False))
        out, out_codes = res if emit is not None else (res, None)
        return a._finish(out, out_codes)


class ChainInt8Layer(nn.Module):
    """A residual block's last 1x1 convolution (+ shortcut, ReLU) and the next block's first 1x1 convolution as ONE kernel
    (csrc/conv_chain_i8.hip): the activation codes between them stay in LDS.  The shortcut is an fp32 tensor, or - `short`,
    the first block of a stage - a second 1x1 convolution reduced into the same tile.  Returns
    `(fp32 or None, codes or None, codes2)`; shapes the kernel is not built for run the plan nodes one after the other."""

    def __init__(self, a, b, want_codes, short=None, main=None):
        super().__init__()
        # `a` carries the epilogue options; with a convolution shortcut, `main` / `short` are the unit-stride and the (possibly)
        # strided operand of the sum (fp32 addition commutes: which of the two the dual plan node called `a` does not matter)
        self.a, self.b, self.want_codes, self.short, self.main = a, b, bool(want_codes), short, (main if main is not None else a)
        self.swapped = short is not None and self.main is not a       # main reads the plan node's SECOND input
        self._w2cm = None      # the second layer's weight codes chunk-major (K.chunk_major), made at the first forward
        self.out_cm = False    # the fp32 block output as a K.ChunkMajor (set by _block_layout_pass where only chain kernels read it)
        # _recompute_pass.  `defer_out` (a convolution-shortcut chain): the fp32 block output is not stored but handed on as a
        # K.DeferredBlock - the two operands it is made of; `recompute` (the chain that alone reads it, as its shortcut): given such a
        # value, the kernel recomputes it chunk by chunk (K.conv2d_i8_recompute_chain).  Any other reader of a DeferredBlock gets the
        # tensor, materialised by one dual launch: same bits
        self.defer_out = False
        self.recompute = False

    def forward(self, x, y):
        a, b, sc, mn = self.a, self.b, self.short, self.main
        if self.swapped:
            x, y = y, x
        codes = mn._codes(x)
        n, c, h, w = codes.shape
        nxt = dict(wq=b.wq, wsum=b.wsum, bias=b._bias(), w_scale=b.w_scale)
        if not getattr(b, "_packed4", False):     # (4-bit weights live packed and are expanded per forward: they stay KRSC)
            if self._w2cm is None or self._w2cm.device != b.wq.device:
                self._w2cm = K.chunk_major(b.wq)  # the plan's weights are frozen: made once
            nxt["wq_chunk"] = self._w2cm
        kw = dict(relu=a.relu, emit=a._emit_for(n, a.k, h, w), want_out=a.want_out, want_codes=self.want_codes, emit2=b._emit_for(n, b.k, h, w),
                  out_chunk_major=self.out_cm)
        if sc is None:
            if (self.recompute and isinstance(y, K.DeferredBlock) and y._buf is None and
                    K.recompute_chain_supported(c, y.pa["codes"].shape[1], y.pb["codes"].shape[1], a.k, b.k, n * h * w)):
                return K.conv2d_i8_recompute_chain(a.operand(x, codes), nxt, y.pa, y.pb, relu_shortcut=y.relu, relu2=b.relu, **kw)
            if not K.chain_supported(c, a.k, b.k, n * h * w):
                if isinstance(y, K.ChunkMajor):      # (the plan nodes one after the other know row-major tensors only)
                    y = y.to_nhwc()
                out, mid = a(x, y)
                return out, (mid if self.want_codes else None), b(mid)[1]
            return K.conv2d_i8_chain(a.operand(x, codes), nxt, y, relu2=b.relu, **kw)
        if not K.dual_chain_supported(c, sc.c, a.k, b.k, n * h * w):
            out, mid = DualInt8Layer(a, sc if mn is a else mn)(*((x, y) if mn is a else (y, x)))
            return out, (mid if self.want_codes else None), b(mid)[1]      # (row-major: every reader takes that)
        kw["emit3"] = kw.pop("emit2")
        oa, ob = mn.operand(x), sc.operand(y)
        if self.defer_out and a.want_out:
            _, mid, codes3 = K.conv2d_i8_dual_chain(oa, ob, nxt, relu3=b.relu, **dict(kw, want_out=False))
            return K.DeferredBlock(oa, ob, a.relu, (n, a.k, h, w)), mid, codes3
        return K.conv2d_i8_dual_chain(oa, ob, nxt, relu3=b.relu, **kw)


class DwPwInt8Layer(nn.Module):
    """A depthwise 3x3 / stride 1 / pad 1 layer and the pointwise layer that alone reads its codes as ONE kernel
    (csrc/conv_dwpw_i8.hip: the MobileOne / MobileNet unit; the wide code tensor between them stays in LDS).  Returns
    `(None, codes)` like a codes-only Int8Layer; inputs the kernel is not built for run the two plan nodes one after the other."""

    def __init__(self, dw, pw):
        super().__init__()
        self.dw, self.pw = dw, pw
        self._tables = {}      # (elements of the input, unsigned?) -> the depthwise constants in the kernel's layout (QBase: s^ depends on numel)

    def forward(self, x):
        dw, pw = self.dw, self.pw
        codes = dw._codes(x)
        n, c, h, w = codes.shape
        lay = dw.layer
        if not K.dwpw_supported(c, pw.k_pad, h, w, lay.stride[0], lay.padding[0], lay.weight.shape[2]) or pw.c_pad != c:
            return pw(dw(x)[1])
        numel = dw._real_numel(codes)
        key = (numel, codes.dtype == torch.uint8, dw.wq.data_ptr())
        table = self._tables.get(key)
        if table is None:
            self._tables.clear()
            table = self._tables[key] = K.dwpw_table(dw.wq, dw._bias(), dw._in_scale(numel), dw._zp(codes), dw.w_scale, dw.w_off,
                                                     x_unsigned=codes.dtype == torch.uint8)
        emit = dw._emit_for(n, dw.k, h, w)                          # the depthwise output's quantiser = the pointwise layer's input quantiser
        emit2 = pw._emit_for(n, pw.layer.weight.shape[0], h, w)
        op = dict(wq=pw.wq, wsum=pw.wsum, bias=pw._bias(), w_scale=pw.w_scale, w_offset=pw.w_off, in_scale=pw._in_scale(n * h * w * pw.c))
        out = K.conv2d_dwpw_i8(codes, table, dw.w_off is not None, dw._bias() is not None, dw.relu, dw._zp(codes), emit, op, relu=pw.relu, emit2=emit2)
        return pw._finish(None, out)


# ------------------------------------------------------------------------- graph surgery of the passes
def _outputs_read(node):
    """{i: the `node[i]` getitem} over the readers of plan node `node`; None if anything else reads it (or two read one output)."""
    gets = {u.args[1]: u for u in node.users if u.op == "call_function" and u.target is operator.getitem}
    return gets if len(gets) == len(node.users) else None


def _sole_user(node):
    """The one reader of graph node `node`; None if it has none or several (or is no graph node: a Python scalar argument)."""
    return next(iter(node.users)) if isinstance(node, fx.Node) and len(node.users) == 1 else None


def _call_plan_module(gm, after, name, module, args, outputs=(0, 1)):
    """Add `module` to the plan as `name`, called with `args` behind node `after`.  Returns the call and {i: its `[i]` getitem}, made
    in the order of `outputs`."""
    gm.add_module(name, module)
    with gm.graph.inserting_after(after):
        node = gm.graph.call_module(name, args=args)
    with gm.graph.inserting_after(node):
        return node, {i: gm.graph.call_function(operator.getitem, (node, i)) for i in outputs}


def _settle(gm, changed=True):
    """The end of a rewriting pass: drop what nothing reads any more, check the graph, regenerate its code."""
    if changed:
        gm.graph.eliminate_dead_code()
        gm.graph.lint()
        gm.recompile()


def _dwpw_pass(gm, report):
    """Depthwise 3x3 -> pointwise 1x1 (a MobileOne / MobileNet unit): replace the two plan nodes by one DwPwInt8Layer where the pointwise
    layer is the only reader of the depthwise layer's codes and both emit codes only."""
    graph = gm.graph
    modules = dict(gm.named_modules())
    count = 0
    for nd in list(graph.nodes):
        dw = modules.get(nd.target) if nd.op == "call_module" else None
        if type(dw) is not DwInt8Layer or len(nd.args) != 1:
            continue
        lay = dw.layer
        if dw.relu6 or dw.act.xoff:          # (the fused unit's kernel: ReLU only, no float activation offset)
            continue
        if not (tuple(lay.weight.shape[2:]) == (3, 3) and lay.stride[0] == 1 and lay.padding[0] == 1 and lay.dilation[0] == 1 and dw.pool is None and
                dw.emit is not None and not dw.want_out and (dw.emit.lo, dw.emit.hi) == (0, 255) and not dw.emit_shift and dw.k_pad % 64 == 0):
            continue
        gets = _outputs_read(nd)
        if gets is None or 1 not in gets or (0 in gets and gets[0].users):
            continue
        g1 = gets[1]
        if len(g1.users) != 1:
            continue
        npw = next(iter(g1.users))
        pw = modules.get(npw.target) if npw.op == "call_module" else None
        # (nor a pointwise layer whose input quantiser has a float offset: the unit's kernel takes the depthwise output's quantiser
        #  zero point as the pointwise operand's integer zero point)
        if type(pw) is not Int8Layer or npw.args != (g1,) or pw.relu6 or pw.act.xoff:
            continue
        pl = pw.layer
        if not (pl.weight.dim() == 4 and tuple(pl.weight.shape[2:]) == (1, 1) and pl.stride[0] == 1 and pl.padding[0] == 0 and pw.pool is None and
                pw.emit is not None and not pw.want_out and not pw.emit_shift and pw.c_pad == dw.k_pad and pw.k_pad in K.DWPW_WIDTHS):
            continue
        pgets = _outputs_read(npw)
        if pgets is None or (0 in pgets and pgets[0].users):
            continue
        _, outs = _call_plan_module(gm, npw, f"_int8_dwpw_{count}", DwPwInt8Layer(dw, pw), nd.args, outputs=(1,))
        count += 1
        if 1 in pgets:
            pgets[1].replace_all_uses_with(outs[1])
        for n in list(pgets.values()) + [npw] + list(gets.values()) + [nd]:
            graph.erase_node(n)
    report.dwpw = count
    _settle(gm, count)


def _pointwise(plan):
    """A plan node the chain kernel can take as either half: a plain 1x1 / stride 1 / unpadded int8 convolution."""
    lay = plan.layer
    return (_is_int8(plan) and lay.weight.dim() == 4 and tuple(lay.weight.shape[2:]) == (1, 1) and lay.stride[0] == 1 and
            lay.padding[0] == 0 and plan.w_off is None and plan.pool is None and plan.k_pad == plan.k and plan.c_pad == plan.c and
            not plan.act.needs_g and not plan.relu6 and          # (the chain kernel: ReLU only)
            plan.pad_shortcut is None)                           # (a pad shortcut: the tiled kernel's PADRES epilogue alone reads one)


def _chain_pass(gm, report):
    """Block end -> next block's first 1x1: replace the two plan nodes by one ChainInt8Layer where the second reads nothing
    but the first's codes (other readers of those codes - a stage's downsample convolution - keep getting them)."""
    graph = gm.graph
    modules = dict(gm.named_modules())
    count = 0
    for na in list(graph.nodes):
        if na.op != "call_module" or len(na.args) != 2 or not isinstance(modules.get(na.target), (Int8Layer, DualInt8Layer)):
            continue
        a, main, short = modules[na.target], None, None
        if isinstance(a, DualInt8Layer):      # the first block of a stage: its shortcut is a (possibly strided) 1x1 convolution
            a, other = a.a, a.b
            main, short = (a, other) if _pointwise(a) else (other, a)
            lay = short.layer
            if not (_pointwise(main) and _is_int8(short) and lay.weight.dim() == 4 and tuple(lay.weight.shape[2:]) == (1, 1) and
                    lay.padding[0] == 0 and short.w_off is None and short.pool is None and short.k_pad == short.k and
                    short.c_pad == short.c and not short.act.needs_g and a.pool is None and a.w_off is None):
                continue
        elif not _pointwise(a):
            continue
        if not (a.emit is not None and (a.emit.lo, a.emit.hi) == (0, 255) and not a.emit.needs_g):
            continue
        mc = (main if main is not None else a).c       # channels of the unit-stride operand
        gets = _outputs_read(na)
        if gets is None or 1 not in gets:
            continue
        g1 = gets[1]
        nb = next((u for u in g1.users if u.op == "call_module" and u.args == (g1,) and isinstance(modules.get(u.target), Int8Layer) and
                   _pointwise(modules[u.target]) and modules[u.target].emit is not None and not modules[u.target].want_out and
                   not modules[u.target].emit.needs_g and modules[u.target].c == a.k and
                   ((mc, modules[u.target].k) in K.CHAIN_SHAPES if short is None else
                    (mc, short.c, modules[u.target].k) in K.DUAL_CHAIN_SHAPES)), None)
        if nb is None:
            continue
        b = modules[nb.target]
        bgets = _outputs_read(nb)
        if bgets is None or (0 in bgets and bgets[0].users):
            continue
        a.emit_shift = False        # the chain kernel's second GEMM reads those codes in place, as unsigned bytes
        _, outs = _call_plan_module(gm, na, f"_int8_chain_{count}", ChainInt8Layer(a, b, want_codes=len(g1.users) > 1, short=short, main=main),
                                    na.args, outputs=(2, 1, 0))
        count += 1
        if 0 in gets:
            gets[0].replace_all_uses_with(outs[0])
        for u in list(g1.users):
            if u is not nb:
                u.replace_input_with(g1, outs[1])
        if 1 in bgets:
            bgets[1].replace_all_uses_with(outs[2])
        for n in list(bgets.values()) + [nb] + list(gets.values()) + [na]:
            graph.erase_node(n)
    report.chained = count
    _settle(gm, count)


# (C, Ca, Cb, K2) of the pairs _recompute_pass rewrites: the shapes whose pair won when measured (LABNOTES 17), among those the kernel is
# built for (K.RECOMPUTE_CHAIN_SHAPES)
RECOMPUTE_ENABLED = {(64, 64, 64, 64)}
# fuse_inference(recompute_shortcuts=None) takes its default from the environment, so that one tree runs an unchanged benchmark both ways
RECOMPUTE_DEFAULT = os.environ.get("DLMCQ_RECOMPUTE_SHORTCUTS", "1") not in ("0", "", "off", "false")


def _plain_emit(e):
    """The quantiser the chain kernels' compile-time-flag forms know: unsigned byte, zero point 0, no g."""
    return e is not None and (e.lo, e.hi) == (0, 255) and not e.needs_g and e.zp_emit is None


def _recompute_pass(gm, report, enabled):
    """The fp32 output of a stage's first block (a convolution-shortcut chain) read by nothing but the next chain, as its shortcut, exists
    only for transport - 1 KB per pixel written and read back at K = 256, computed from 128 B of codes.  Where the shape is enabled the
    first launch hands on a K.DeferredBlock - its two operands - instead of the tensor, and the second recomputes the tensor chunk
    by chunk from them (csrc/conv_chain_i8.hip, the CA / CB form): bit-identical.  The graph keeps its edges: only the two modules are marked.  Anything else - another reader of the tensor, a quantiser the kernel's
    compile-time forms do not know, a second layer without ReLU, a shape outside `enabled` - keeps the graph as it is."""
    graph = gm.graph
    modules = dict(gm.named_modules())
    count = 0
    for n0 in list(graph.nodes):
        m0 = modules.get(n0.target) if n0.op == "call_module" else None
        if not isinstance(m0, ChainInt8Layer) or m0.short is None or m0.defer_out or len(n0.args) != 2:
            continue
        outs = [u for u in n0.users if u.op == "call_function" and u.target is operator.getitem and u.args[1] == 0]
        if len(outs) != 1 or len(outs[0].users) != 1:
            continue
        o = outs[0]
        n1 = next(iter(o.users))
        m1 = modules.get(n1.target) if n1.op == "call_module" else None
        if not (isinstance(m1, ChainInt8Layer) and m1.short is None and not m1.recompute and len(n1.args) == 2 and not n1.kwargs and
                n1.args[1] is o and n1.args[0] is not o):
            continue
        if (m1.main.c, m0.main.c, m0.short.c, m1.b.k) not in enabled or m0.a.k != m1.a.k:
            continue
        if not (m1.a.relu and _plain_emit(m1.a.emit) and _plain_emit(m1.b.emit) and m0.a.pool is None and m1.a.pool is None):
            continue
        m0.defer_out = m1.recompute = True
        count += 1
    report.recomputed = count


def _block_end_like(m):
    """A plan layer the library's block-end kernel (csrc/conv_pwr_i8.hip) can take: the only kernel besides the chain kernels that
    knows chunk-major block tensors.  (Whether it DOES take a call is the library's decision per call - K.conv2d_i8 asks and falls
    back to the ordinary layout.)"""
    return (_is_int8(m) and _pointwise(m) and m.c in (256, 512) and m.k % 128 == 0 and m.k_pad == m.k and m.c_pad == m.c and m.relu
            and m.w_off is None and m.pool is None and m.layer.stride[0] == 1 and not m.act.needs_g and
            (m.emit is None or ((m.emit.lo, m.emit.hi) == (0, 255) and not m.emit.needs_g)))


def _block_layout_pass(gm, report):
    """The fp32 block tensor between two kernels that walk it chunk by chunk - written by a chain kernel or the block-end kernel, read
    as the shortcut by another of them, by nothing else - goes CHUNK-MAJOR (K.ChunkMajor, DLMCQ_FP32_*_CHUNK_MAJOR): HBM serves planes in
    which neighbouring workgroups' pieces are neighbours faster than 256-byte pieces of K * 4-byte rows (chain launches -11 ... -18 % at
    14^2 / 56^2, tools/chain_ab.py --abcm).  A private layout of the plan: same values.  Calls that keep their two fp32 tensors in one
    layout (K.CHAIN_ONE_LAYOUT; the block-end kernel) get both or neither."""
    graph = gm.graph
    modules = dict(gm.named_modules())

    def mod(node):
        return modules.get(node.target) if node.op == "call_module" else None

    def writer(m):      # can write its fp32 output chunk-major
        if isinstance(m, ChainInt8Layer):
            return m.a.k % 64 == 0
        if isinstance(m, DualInt8Layer):     # (the 256-deep addend read row by row, the 512-deep one sampled: conv_pwr_applies)
            one = lambda t: _is_int8(t) and t.layer.weight.dim() == 4 and tuple(t.layer.weight.shape[2:]) == (1, 1)
            dense, other = (m.a, m.b) if m.a.c == 256 else (m.b, m.a)
            return (one(m.a) and one(m.b) and (dense.c, other.c) == (256, 512) and dense.layer.stride[0] == 1 and m.a.relu and m.a.k % 128 == 0
                    and m.a.k_pad == m.a.k and m.a.w_off is None and m.b.w_off is None and m.a.pool is None and m.a.emit is not None)
        return isinstance(m, Int8Layer) and _block_end_like(m)

    def reader(node, o):   # reads `o` as its fp32 shortcut, chunk-major if offered
        m = mod(node)
        if len(node.args) != 2 or node.args[1] is not o or node.args[0] is o:
            return False
        if isinstance(m, ChainInt8Layer):
            return m.short is None
        return isinstance(m, Int8Layer) and _block_end_like(m)

    def one_layout(m):
        if isinstance(m, ChainInt8Layer):
            return m.short is None and (m.main.c, m.b.k) in K.CHAIN_ONE_LAYOUT
        return True         # (the block-end kernel)
    nodes = [n for n in graph.nodes if isinstance(mod(n), (ChainInt8Layer, DualInt8Layer, Int8Layer))]
    out_node, src, cm = {}, {}, {}     # node -> getitem of its fp32 output; node -> the node whose output is its shortcut; node -> output chunk-major?
    for nd in nodes:
        for u in nd.users:
            if u.op == "call_function" and u.target is operator.getitem and u.args[1] == 0 and u.users:
                out_node[nd] = u
    for nd, o in out_node.items():
        cm[nd] = writer(mod(nd)) and all(reader(r, o) for r in o.users)
        if cm[nd]:
            for r in o.users:
                src[r] = nd
    changed = True
    while changed:                   # one layout per call where the kernel has a single set of offsets
        changed = False
        for nd in nodes:
            m = mod(nd)
            has_shortcut = len(nd.args) == 2 and not isinstance(m, DualInt8Layer) and not (isinstance(m, ChainInt8Layer) and m.short is not None)
            if nd not in out_node or not has_shortcut or not one_layout(m):
                continue
            icm, ocm = cm.get(src.get(nd), False), cm.get(nd, False)
            if icm and not ocm:
                cm[src[nd]] = False
                changed = True
            elif ocm and not icm:
                cm[nd] = False
                changed = True
    count = 0
    for nd, flag in cm.items():
        mod(nd).out_cm = bool(flag)
        count += bool(flag)
    report.chunk_major = count


class GapLayer(nn.Module):
    """Global average pool of an fp32 map (csrc/gap.hip) straight to the classifier's activation codes [N, C] (and / or fp32): the
    pool, the flatten and the consumer's quantise pass as one read of the map.  Returns `(fp32 or None, codes)`."""

    def __init__(self, emit, want_out):
        super().__init__()
        self.emit, self.want_out = emit, bool(want_out)

    def forward(self, x):
        n, c = x.shape[0], x.shape[1]
        return K.global_avgpool(x, emit=self.emit.emit(n * c), want_out=self.want_out)


class GapHeadLayer(nn.Module):
    """The network's head as ONE kernel (csrc/conv_gap_i8.hip): the last 1x1 convolution (+ fp32 shortcut) (+ ReLU / ReLU6), pooled
    over its <= 64 pixels into the classifier's codes - its fp32 map is never written.  `a`: the convolution's plan node (it carries
    the activation); maps the kernel is not built for (more than 64 pixels) run the plan node and the pool kernel one after the other.
    Returns `(fp32 [N, K] or None, codes [N, K])` - the same bits either way."""

    def __init__(self, a, emit, want_out):
        super().__init__()
        self.a, self.emit, self.want_out = a, emit, bool(want_out)

    def forward(self, x, residual=None):
        a = self.a
        codes = a._codes(x)
        n, c, h, w = codes.shape
        emit = self.emit.emit(n * a.k)
        if not K.gap_head_supported(c, a.k, h, w):
            return K.global_avgpool(a(codes, residual)[0], emit=emit, want_out=self.want_out)
        return K.conv2d_i8_gap(codes, a.wq, a.wsum, a._bias(), a._in_scale(a._real_numel(codes)), a._zp(codes), a.w_scale,
                               residual=residual, act=a._act_arg(), emit=emit, want_out=self.want_out)


class _MapCodesLayer(nn.Module):
    """What the plan nodes that read an fp32 map once and hand its readers activation codes share (AvgPoolLayer, GateLayer, SwishLayer,
    HardswishLayer; csrc/map_codes.h).  `emit`: the readers' activation quantiser (_ActSpec); `want_out`: whether anyone reads the fp32 values; the code
    rows are `c_pad` wide with `pad_code` behind the `c` real channels - what Int8Layer._codes / _pad_channels build from the fp32
    tensor; `shift`: the codes are stored as `code - 128`."""

    def __init__(self, emit, want_out, c, c_pad, pad_code, shift):
        super().__init__()
        self.emit, self.want_out = emit, bool(want_out)
        self.c, self.c_pad, self.pad_code, self.emit_shift = int(c), int(c_pad), int(pad_code), bool(shift)

    def _to_codes(self, numel):
        """The keyword arguments every K.*_quant wrapper ends with; `numel`: the consumer's real input (a QBase consumer's g)."""
        e = self.emit.emit(numel)
        e.shift128 = self.emit_shift
        return dict(emit=e, want_out=self.want_out, c_pad=self.c_pad, pad_code=self.pad_code)

    def _torch_codes(self, v):
        """`(v or None, codes)` of fp32 values `v` computed with torch, quantised with K.fake_quant: the values of the unfused graph."""
        a = self.emit
        t = v.contiguous(memory_format=torch.channels_last) if v.dim() == 4 else v.contiguous()
        codes = K.fake_quant(t, a.scale, a.zp, a.lo, a.hi, a.form, g=a.g(v.numel()), codes="i8", want_y=False)[1]
        if self.emit_shift:
            codes = (codes.view(torch.uint8) ^ 0x80).view(torch.int8)
        if codes.dim() == 4 and codes.shape[1] < self.c_pad:
            codes = _pad_channels(codes, self.c_pad, self.pad_code)
        return (v if self.want_out else None), codes

    def _torch_rows(self, v):
        """_torch_codes of dense rows [..., C] of any rank (no channel axis to pad: the readers are Linear layers), in `v`'s shape."""
        _, codes = self._torch_codes(v.reshape(-1, v.shape[-1]))
        return (v if self.want_out else None), codes.reshape(v.shape)


class AvgPoolLayer(_MapCodesLayer):
    """A windowed average pool (nn.AvgPool2d(s, s) / F.avg_pool2d(x, s): window = stride, no padding, floor) of an fp32 map straight to
    the activation codes of the plan layers that read it (csrc/avgpool.hip) - the shortcut of a ResNet-C / -D block: the pool, the pooled
    fp32 tensor and the consumer's quantise pass as one read of the map.  Returns `(fp32 or None, codes)`."""

    def __init__(self, window, emit, want_out, c, c_pad, pad_code, shift=False):
        super().__init__(emit, want_out, c, c_pad, pad_code, shift)
        self.window = int(window)

    def forward(self, x):
        n, c, h, w = x.shape
        s = self.window
        return K.avgpool_quant(x, s, **self._to_codes(n * c * (h // s) * (w // s)))      # (the pooled tensor)


_AVGPOOL_NAMES = ("input", "kernel_size", "stride", "padding", "ceil_mode", "count_include_pad", "divisor_override")


def _avgpool_window(node, modules):
    """(input node, s) if `node` is an average pool the plan runs - nn.AvgPool2d or F.avg_pool2d in any argument spelling, the kernel a
    Python int or an equal pair in 2 .. 8, the stride None or equal to the kernel, padding 0, ceil_mode False, divisor_override None -
    else None (a kernel size read from the tensor, as in F.avg_pool2d(x, x.size(3)), is a graph node, not an int)."""
    if node.op == "call_module":
        m = modules.get(node.target)
        if type(m) is not nn.AvgPool2d or len(node.args) != 1 or node.kwargs:
            return None
        given = dict(input=node.args[0], kernel_size=m.kernel_size, stride=m.stride, padding=m.padding, ceil_mode=m.ceil_mode,
                     divisor_override=m.divisor_override)
    elif node.op == "call_function" and node.target in (F.avg_pool2d, torch._C._nn.avg_pool2d):
        if len(node.args) > len(_AVGPOOL_NAMES) or not set(node.kwargs) <= set(_AVGPOOL_NAMES[len(node.args):]):
            return None
        given = dict(zip(_AVGPOOL_NAMES, node.args), **node.kwargs)
    else:
        return None

    def one(v):      # an int, or a pair of equal ints
        if isinstance(v, (tuple, list)) and len(v) in (1, 2) and len(set(v)) == 1:
            v = v[0]
        return v if isinstance(v, int) and not isinstance(v, bool) else None
    x, k = given.get("input"), one(given.get("kernel_size"))
    stride, pad = given.get("stride"), given.get("padding", 0)
    if not isinstance(x, fx.Node) or k is None or not 2 <= k <= 8:
        return None
    if not (stride is None or (isinstance(stride, (tuple, list)) and len(stride) == 0) or one(stride) == k):
        return None
    if one(pad) != 0 or given.get("ceil_mode", False) is not False or given.get("divisor_override") is not None:
        return None
    return x, k


_CodeReaders = collections.namedtuple("_CodeReaders", "emit takers want_out c c_pad pad_code shift")


def _decided(r):
    """What a _CodeReaders (or a record built on it) decides for the plan node, as a _MapCodesLayer's constructor arguments."""
    return dict(emit=r.emit, want_out=r.want_out, c=r.c, c_pad=r.c_pad, pad_code=r.pad_code, shift=r.shift)


def _splice_map_node(gm, last, name, module, args, takers, erase, outputs=2):
    """Put `module` into the plan as `name`, called with `args`, in place of fp32 node `last`: `takers` read its codes (output 1),
    everyone else its fp32 map (output 0) - or, with `outputs=1`, the one tensor it returns; then `erase` the nodes it replaces, in
    that order."""
    call, outs = _call_plan_module(gm, last, name, module, args, (0, 1) if outputs == 2 else ())
    for u in list(last.users):
        u.replace_input_with(last, (outs[1] if u in takers else outs[0]) if outs else call)
    for n in erase:
        gm.graph.erase_node(n)


class _DryNode(nn.Module):
    """fuse_inference(dry_run=...): a plan node that holds nothing (a main-pass node, a head, an average pool, a gate).  It cannot be run."""

    def __init__(self, *args, **kwargs):
        super().__init__()

    def forward(self, *args):
        raise RuntimeError("fuse_inference(dry_run=...) builds the plan's structure only")


@functools.lru_cache(maxsize=None)
def _dry(cls, init=None):
    """The dry-run stand-in of plan node class `cls`: the subclass `_Dry<cls>` that is built like it (or by `init`), carries the same
    decision in the same attributes and cannot be run.  (An average pool's and a gate's stand-in is the attribute-less _DryNode: the
    recorded plans of tests/golden/plans/ print them so.)"""
    if cls in (AvgPoolLayer, GateLayer):
        return _DryNode
    body = dict(forward=_DryNode.forward, __doc__=f"fuse_inference(dry_run=...): a {cls.__name__}'s decision.  It cannot be run.")
    return type("_Dry" + cls.__name__, (cls,), dict(body, __init__=init) if init else body)


# What a matcher of _run_node_pass decides: the plan node's module is `cls(**ctor)`; it is called with `args` in place of fp32 node
# `last`; `takers` read its codes; it replaces the nodes `erase` (erased in that order).
_Splice = collections.namedtuple("_Splice", "cls ctor last args takers erase")


def _run_node_pass(gm, report, kind, field, match, dry_run, outputs=2, left=None):
    """One pass that puts code-emitting nodes behind the main pass's plan.  `match(node, modules)` reads the graph and changes nothing:
    a _Splice (taken), a str (a candidate left alone: why - collected in `left`, else `report.patch_embed_left`) or None.  Every node of the graph
    as the pass found it is asked in turn; a taken one becomes plan node `_int8_<kind>_<i>` - the module, or under `dry_run` its
    stand-in (_dry) - of `outputs` outputs; `modules` (name -> module) is kept current for the matcher; `report.<field>` counts."""
    modules = dict(gm.named_modules())
    count = 0
    for node in list(gm.graph.nodes):
        d = match(node, modules)
        if isinstance(d, str):
            (report.patch_embed_left if left is None else left).append((node.name, d))
        if not isinstance(d, _Splice):
            continue
        name = f"_int8_{kind}_{count}"
        modules[name] = (_dry(d.cls) if dry_run else d.cls)(**d.ctor)
        _splice_map_node(gm, d.last, name, modules[name], d.args, d.takers, d.erase, outputs)
        count += 1
    setattr(report, field, count)
    _settle(gm, count)


def _code_readers(planned, t, dw=False, dwpw=False, linear=False):
    """Who takes fp32 node `t` as codes from a stand-alone quantising node (the average-pool, gate and swish passes): "gemm" plan
    convolutions that read it through their activation argument - as their own node or as an operand of a dual node - with input
    channels % 4 == 0, all sharing one activation quantiser and one channel count; with `dw` (the swish pass: MBConv's expansion swish is
    read by the depthwise layer) "dw" plan convolutions too, which take channel-padded codes as the main pass hands them over (`dwpw`:
    fuse_inference's flag, under which a depthwise layer reads no shifted codes); with `linear` (the LayerNorm and GELU passes) "gemm"
    plan layers with a 2-D weight - Linear layers, which read rows [..., C] - too: they take plain codes of their in-features (a multiple
    of 64: no padding, never shifted), and either every taker is one or none is.  Returns a _CodeReaders (that quantiser, the takers,
    whether anyone else reads `t` as fp32, channels, code-row width, pad code, shifted emission), or None where no such reader exists or
    they disagree."""
    def reader(u):
        """(activation spec, convolution) with which plan node `u` reads `t` as codes, else None."""
        d = planned.get(u)
        if d is None or d.spec.kind not in (("gemm", "dw") if dw else ("gemm",)):
            return None
        if d.spec.kind == "dw":
            ok = not d.dual and u.args[0] is t and t not in u.args[1:] and d.mod.weight.dim() == 4
            return (d.spec.act, d.mod) if ok else None
        if d.dual:
            ops = [(d.dual_inputs[i], (d.mod, d.dual_mod)[i]) for i in (0, 1) if u.args[i] is t]
            if not ops or len({a.key for a, _ in ops}) != 1:
                return None
        elif u.args[0] is t and t not in u.args[1:]:
            ops = [(d.spec.act, d.mod)]
        else:
            return None
        a, m = ops[0]
        if linear and not d.dual and m.weight.dim() == 2:
            return a, m
        return (a, m) if m.weight.dim() == 4 and m.groups == 1 and all(mm.weight.shape[1] == m.weight.shape[1] for _, mm in ops) else None

    readers = {u: reader(u) for u in t.users}
    takers = [u for u, r in readers.items() if r is not None]
    if not takers or len({readers[u][0].key for u in takers}) != 1:      # (the max-pool rule: one quantiser for all code readers)
        return None
    def width(m):      # input channels of reader `m` (depthwise: one per output channel)
        return int(m.weight.shape[0] if m.weight.dim() == 4 and m.groups != 1 else m.weight.shape[1])
    if len({readers[u][1].weight.dim() for u in takers}) != 1:      # (`linear`: rows or a map, not both)
        return None
    emit, conv = readers[takers[0]]
    c = width(conv)
    if c % 4 or c < 4 or any(width(readers[u][1]) != c for u in takers):
        return None
    # shifted codes (`code - 128`) where every taker is a plan convolution on its own node that reads them as they are (a dual node
    # is never handed shifted codes by the main pass either)
    shift = _emits_shifted(emit, [(None, None) if planned[u].dual else (planned[u].spec, planned[u].mod) for u in takers], dwpw)
    return _CodeReaders(emit, takers, len(takers) != len(readers), c, _ceil64(c), _zp_fill(emit) - (128 if shift else 0), shift)


def _avgpool_pass(gm, report, planned, dry_run):
    """Windowed average pools (fuse_inference(avg_pools=True)): `AvgPool2d(s, s) -> plan convolution` becomes a node that hands the
    convolution its activation codes (AvgPoolLayer).  `planned`: plan node -> what the main pass decided for it (_Decision); whatever that is for
    the convolution behind the pool (dual operand, own node, narrow, chain) stays - only its input changes, from fp32 to codes."""
    def match(pool, modules):
        win = _avgpool_window(pool, modules)
        taken = _code_readers(planned, pool) if win is not None else None
        if taken is None:
            return None
        x, s = win
        return _Splice(AvgPoolLayer, dict(_decided(taken), window=s), pool, (x,), taken.takers, [pool])
    _run_node_pass(gm, report, "avgpool", "avg_pools", match, dry_run)


class GateLayer(_MapCodesLayer):
    """A squeeze-excite channel gate `x * g` (x fp32 (N, C, H, W), g (N, C, 1, 1)) (+ ReLU / ReLU6) straight to the activation codes of
    the plan layers that read the gated map (csrc/gate.hip): the multiply, the activation, the gated fp32 tensor and the consumer's
    quantise pass as one read of the map.  `act`: DLMCQ_ACT_*.  A `g`
    of any other shape at run time (a per-tensor or spatial gate the trace could not tell apart) is multiplied, activated and quantised
    with torch and K.fake_quant: the values of the unfused graph.  Returns `(fp32 or None, codes)`."""

    def __init__(self, emit, want_out, act, c, c_pad, pad_code, shift=False):
        super().__init__(emit, want_out, c, c_pad, pad_code, shift)
        self.act = int(act)

    def forward(self, x, g):
        if x.dim() != 4 or x.dtype != torch.float32 or g.dtype != torch.float32 or tuple(g.shape) != (x.shape[0], x.shape[1], 1, 1) or x.shape[1] != self.c:
            return self._unfused(x, g)
        return K.gate_quant(x, g, act=self.act, **self._to_codes(x.numel()))      # (the gated tensor)

    def _unfused(self, x, g):
        v = x * g
        return self._torch_codes(F.relu6(v) if self.act == N.ACT_RELU6 else (torch.relu(v) if self.act == N.ACT_RELU else v))


_MUL_FNS = (operator.mul, torch.mul)


def _is_call(node, fns, method):
    """`node` calls one of the functions `fns` or the tensor method `method`, without keyword arguments."""
    if not isinstance(node, fx.Node) or node.kwargs:
        return False
    return (node.op == "call_function" and node.target in fns) or (node.op == "call_method" and node.target == method)


def _is_mul(node):
    """An out-of-place multiply of two graph values: `a * b`, torch.mul(a, b), a.mul(b)."""
    return _is_call(node, _MUL_FNS, "mul") and len(node.args) == 2 and all(isinstance(a, fx.Node) for a in node.args)


def _squeezed_from(g, modules, limit=16):
    """The input of the global average pool (a spelling _pool_dims knows) that `g` derives from, walking back through first arguments
    only (a multiply on the way - a swish - through either operand), at most `limit` nodes; None if none is reached."""
    stack, seen = [g], 0
    while stack and seen < limit:
        n = stack.pop()
        seen += 1
        if _pool_dims(n, modules) is not None:
            src = n.args[0] if n.args else n.kwargs.get("input")
            return src if isinstance(src, fx.Node) else None
        if n.op not in ("call_function", "call_method", "call_module") or not n.args:
            continue
        nxt = list(n.args) if _is_mul(n) else [n.args[0]]
        stack.extend(a for a in reversed(nxt) if isinstance(a, fx.Node))
    return None


def _gate_pass(gm, report, planned, dry_run, relu6):
    """Squeeze-excite gates (fuse_inference(gates=True)): `x * gate(pool(x))` (+ ReLU / ReLU6) `-> plan convolution` becomes a node
    that hands the convolution its activation codes (GateLayer).  The squeeze path - pool, two small layers, the gate function - stays
    as it is.  `planned`: plan node -> what the main pass decided for it (_Decision); whatever that is for the convolution behind the
    gate stays - only its input changes, from fp32 to codes."""
    def match(mul, modules):
        if not _is_mul(mul) or mul.args[0] is mul.args[1] or _swish_of(mul, modules) is not None:      # (x * sigmoid(x): no gate)
            return None
        if _hardswish_multiply(mul, modules):      # (x * hardsigmoid(x), x * relu6(x + 3): no gate either)
            return None
        a, b = mul.args
        # exactly one operand derives from a global average pool, and that pool reads the other operand
        gated = [(x, g) for x, g in ((a, b), (b, a)) if _squeezed_from(g, modules) is x]
        if len(gated) != 1:
            return None
        act, last = N.ACT_NONE, mul
        nxt = _sole_user(mul)
        if nxt is not None and (_is_relu(nxt, modules) or (relu6 and _is_relu6(nxt, modules))):
            act, last = (N.ACT_RELU if _is_relu(nxt, modules) else N.ACT_RELU6), nxt
        taken = _code_readers(planned, last)
        if taken is None:
            return None
        return _Splice(GateLayer, dict(_decided(taken), act=act), last, gated[0], taken.takers, [last, mul] if last is not mul else [mul])
    _run_node_pass(gm, report, "gate", "gates", match, dry_run)


class SwishLayer(_MapCodesLayer):
    """Swish / SiLU `x * sigmoid(x)` of an fp32 (N, C, H, W) map straight to the activation codes of the plan layers that read the
    activated map (csrc/swish.hip): the sigmoid, the multiply, the activated fp32 tensor and the consumer's quantise pass as one read
    of the map.  `emit`: None where nobody takes codes (the map is then activated in one pass instead of two, and always written); `c`,
    `c_pad`: None where no reader fixes them.  An input that at run time is no 4-D fp32 map of `c` channels (a multiple of 4) is
    activated and quantised with torch and K.fake_quant: the values of the unfused graph.  Returns `(fp32 or None, codes or None)`."""

    def __init__(self, emit, want_out, c, c_pad, pad_code, shift=False):
        super().__init__(emit, want_out or emit is None, c or 0, c_pad or 0, pad_code, shift)
        self.c, self.c_pad = (None if c is None else self.c), (None if c_pad is None else self.c_pad)

    def forward(self, x):
        if x.dim() != 4 or x.dtype != torch.float32 or x.shape[1] != (x.shape[1] if self.c is None else self.c) or x.shape[1] % 4 or not x.is_cuda:
            return self._unfused(x)
        if self.emit is None:
            return K.swish_quant(x)
        return K.swish_quant(x, **self._to_codes(x.numel()))      # (the activated tensor)

    def _unfused(self, x):
        v = x * torch.sigmoid(x)
        return (v, None) if self.emit is None else self._torch_codes(v)


_SIGMOID_FNS = (torch.sigmoid, F.sigmoid)
_SILU_FNS = (F.silu,)


def _swish_of(node, modules):
    """(x, the nodes that compute it) if `node` is swish of graph value x in a spelling the plan takes - `x * torch.sigmoid(x)` with
    either operand first, x.sigmoid(), torch.mul / x.mul(...), the sigmoid read by that multiply alone; nn.SiLU; F.silu(x), not in place
    (an nn.SiLU(inplace=True) only where nothing else reads x) - else None.  A user module whose body is one of these is traced into
    it.  A gate `x * sigmoid(f(pool(x)))` is none of them: the sigmoid's argument must BE the other operand."""
    if node.op == "call_module":
        m = modules.get(node.target)
        x = node.args[0] if len(node.args) == 1 and not node.kwargs else None
        ok = type(m) is nn.SiLU and isinstance(x, fx.Node) and (not m.inplace or len(x.users) == 1)
        return (x, [node]) if ok else None
    if node.op == "call_function" and node.target in _SILU_FNS:
        ok = len(node.args) == 1 and isinstance(node.args[0], fx.Node) and set(node.kwargs) <= {"inplace"} and not node.kwargs.get("inplace", False)
        return (node.args[0], [node]) if ok else None
    if not _is_mul(node) or node.args[0] is node.args[1]:
        return None
    for x, s in (node.args, node.args[::-1]):
        sig = ((s.op == "call_function" and s.target in _SIGMOID_FNS) or (s.op == "call_method" and s.target == "sigmoid"))
        if sig and not s.kwargs and len(s.args) == 1 and s.args[0] is x and len(s.users) == 1:
            return x, [node, s]
    return None


def _is_map(x, planned, modules, limit=8):
    """Whether graph value `x` is known to be a 4-D (N, C, H, W) tensor: the fp32 output of a plan convolution or of a plan node of the
    average-pool / gate / swish passes, a 2-D convolution, batch norm or pool module's, or a sum with one (at most `limit` nodes back).
    The swish on the (N, mid) vector of a squeeze path is none and stays in torch."""
    stack, seen = [x], 0
    while stack and seen < limit:
        n = stack.pop()
        seen += 1
        if n.op == "call_function" and n.target is operator.getitem and isinstance(n.args[0], fx.Node) and n.args[1] == 0:
            d = planned.get(n.args[0])
            if d is not None:
                if d.mod.weight.dim() == 4:
                    return True
            elif n.args[0].op == "call_module" and isinstance(modules.get(n.args[0].target), _MapCodesLayer):
                return True
        elif n.op == "call_module":
            if isinstance(modules.get(n.target), (nn.Conv2d, nn.BatchNorm2d, nn.MaxPool2d, nn.AvgPool2d, nn.AdaptiveAvgPool2d)):
                return True
        elif _is_add(n):
            stack.extend(n.args)
    return False


def _swish_pass(gm, report, planned, dry_run, dwpw):
    """Swish activations (fuse_inference(swish=True)): `x * sigmoid(x)` / SiLU of a 4-D map becomes a node (SwishLayer) that hands the
    plan convolutions behind it - depthwise ones included - their activation codes and every other reader (a squeeze-excite pool, the
    gate node, a shortcut add) the activated fp32 map from the same launch.  `planned`: plan node -> what the main pass decided for it
    (_Decision); whatever that is for the convolution behind the swish stays - only its input changes, from fp32 to codes."""
    def match(node, modules):
        found = _swish_of(node, modules)
        if found is None:
            return None
        x, nodes = found
        taken = _code_readers(planned, node, dw=True, dwpw=dwpw)
        if taken is None:      # nobody takes codes: one pass over the map instead of two, where it is known to be a map (which an
            #                    earlier swish node's fp32 output is: `modules` holds the nodes of this pass too)
            if not _is_map(x, planned, modules):
                return None
            taken = _CodeReaders(None, (), True, None, None, 0, False)
        return _Splice(SwishLayer, _decided(taken), node, (x,), taken.takers, nodes)
    _run_node_pass(gm, report, "swish", "swishes", match, dry_run)


# ------------------------------------------------------------------ hard swish x * relu6(x + 3) / 6
# The spellings _hardswish_of takes -> the order of csrc/hardswish.hip's two multiplies that computes the spelling's own values, and the
# spelling again in torch (HardswishLayer._unfused).  "mul_*": (x * r) / 6 or (x * r) * (1 / 6); "gate_*": x * (r / 6) or x * (r * (1 / 6)),
# r = relu6(x + 3); "hardsigmoid": x * hardsigmoid(x).
_HARDSWISH_ORDER = {"hardswish": "mul_first", "mul_div": "mul_first", "mul_mul": "mul_first",
                    "gate_div": "gate_first", "gate_mul": "gate_first", "hardsigmoid": "gate_first"}
_HARDSWISH_TORCH = {"hardswish": F.hardswish,
                    "mul_div": lambda x: x * F.relu6(x + 3.0) / 6.0,
                    "mul_mul": lambda x: x * F.relu6(x + 3.0) * (1.0 / 6.0),
                    "gate_div": lambda x: x * (F.relu6(x + 3.0) / 6.0),
                    "gate_mul": lambda x: x * (F.relu6(x + 3.0) * (1.0 / 6.0)),
                    "hardsigmoid": lambda x: x * F.hardsigmoid(x)}
# What _hardswish_pass decides for one node: the graph value it activates, the spelling it replaces, the kernel's order, the nodes it
# replaces (names).
_HardswishDecision = collections.namedtuple("_HardswishDecision", "x spelling order chain")


class HardswishLayer(_MapCodesLayer):
    """Hard swish `x * relu6(x + 3) / 6` of an fp32 (N, C, H, W) map straight to the activation codes of the plan layers that read the
    activated map (csrc/hardswish.hip): the add, the clamp, the multiplies, the activated fp32 tensor and the consumer's quantise pass
    as one read of the map.  `order`: "mul_first" ((x * r) * fl32(1 / 6): nn.Hardswish's) or "gate_first" (x * (r * fl32(1 / 6)):
    x * hardsigmoid(x)'s) - the order of the spelling the node replaces; `decision`: the pass's record (_HardswishDecision), None for a
    node built by hand, which then restates nn.Hardswish or x * hardsigmoid(x).  `emit`: None where nobody takes codes (the map is then
    activated in one pass, and always written); `c`, `c_pad`: None where no reader fixes them.  An input that at run time is no 4-D fp32
    device map of `c` channels (a multiple of 4) is activated with the torch ops of the spelling that was matched and quantised with
    K.fake_quant: the values of the unfused graph.  Returns `(fp32 or None, codes or None)`."""

    def __init__(self, emit, want_out, c, c_pad, pad_code, shift=False, order="mul_first", decision=None):
        super().__init__(emit, want_out or emit is None, c or 0, c_pad or 0, pad_code, shift)
        self.c, self.c_pad = (None if c is None else self.c), (None if c_pad is None else self.c_pad)
        if order not in K.HARDSWISH_ORDERS:
            raise ValueError(f"HardswishLayer: order is 'mul_first' or 'gate_first', not {order!r}")
        if decision is not None and _HARDSWISH_ORDER[decision.spelling] != order:
            raise ValueError(f"HardswishLayer: the spelling {decision.spelling!r} is computed {_HARDSWISH_ORDER[decision.spelling]}, not {order}")
        self.order = order
        self.spelling = decision.spelling if decision is not None else ("hardswish" if order == "mul_first" else "hardsigmoid")
        if decision is not None:
            self.decision = decision

    def forward(self, x):
        if x.dim() != 4 or x.dtype != torch.float32 or x.shape[1] != (x.shape[1] if self.c is None else self.c) or x.shape[1] % 4 or not x.is_cuda:
            return self._unfused(x)
        if self.emit is None:
            return K.hardswish_quant(x, self.order)
        return K.hardswish_quant(x, self.order, **self._to_codes(x.numel()))      # (the activated tensor)

    def _unfused(self, x):
        v = _HARDSWISH_TORCH[self.spelling](x)
        return (v, None) if self.emit is None else self._torch_codes(v)


def _is_number(v, k):
    return isinstance(v, (int, float)) and not isinstance(v, bool) and float(v) == k


def _relu6_of_plus3(r6, modules):
    """(x, [r6, add]) if `r6` is relu6(x + 3) - a ReLU6 in a spelling _is_relu6 knows, of `x + 3` / `3 + x` / torch.add / x.add with the
    addend exactly 3, that sum read by the ReLU6 alone - else None."""
    if not isinstance(r6, fx.Node) or not _is_relu6(r6, modules) or not r6.args:
        return None
    add = r6.args[0]
    if not (_is_call(add, (operator.add, torch.add), "add") and len(add.args) == 2 and len(add.users) == 1):
        return None
    for x, k in (add.args, add.args[::-1]):
        if isinstance(x, fx.Node) and _is_number(k, 3.0):
            return x, [r6, add]
    return None


def _sixth_of(node, src):
    """"div" if `node` is `src / 6`, "mul" if it is `src * (1 / 6)` (either operand first) - the divisor exactly 6, the factor exactly the
    double 1 / 6 - else None."""
    if _is_call(node, _DIV_FNS, "div") and len(node.args) == 2 and node.args[0] is src and _is_number(node.args[1], 6.0):
        return "div"
    if _is_call(node, _MUL_FNS, "mul") and len(node.args) == 2:
        if any(a is src and _is_number(b, 1.0 / 6.0) for a, b in (node.args, node.args[::-1])):
            return "mul"
    return None


def _hardswish_of(node, modules):
    """(x, the nodes that compute it, the spelling) if `node` is the hard swish of graph value x in a spelling the plan takes, else None:
    nn.Hardswish (an inplace one only where nothing else reads x); F.hardswish(x), not in place; `(x * r) / 6` and `x * (r / 6)` with
    r = relu6(x + 3) spelled out - the addend exactly 3, the ReLU6 any spelling _is_relu6 knows, the divisor exactly 6 or the factor
    exactly 1 / 6, the multiplies with either operand first, each intermediate read by the next node alone; `x * F.hardsigmoid(x)` /
    `x * nn.Hardsigmoid()(x)`, not in place, the gate read by that multiply alone.  A user module whose body is one of these is traced
    into it.  `x * hardsigmoid(y)`, a squeeze-excite gate `x * hardsigmoid(f(pool(x)))`, `+ 2` and `/ 5` are none of them."""
    if node.op == "call_module":
        m = modules.get(node.target)
        x = node.args[0] if len(node.args) == 1 and not node.kwargs else None
        ok = type(m) is nn.Hardswish and isinstance(x, fx.Node) and (not m.inplace or len(x.users) == 1)
        return (x, [node], "hardswish") if ok else None
    if node.op == "call_function" and node.target is F.hardswish:
        ok = len(node.args) == 1 and isinstance(node.args[0], fx.Node) and set(node.kwargs) <= {"inplace"} and not node.kwargs.get("inplace", False)
        return (node.args[0], [node], "hardswish") if ok else None
    if not isinstance(node, fx.Node) or node.kwargs or len(node.args) != 2:
        return None
    # (x * r) / 6, (x * r) * (1 / 6): `node` scales the product
    for mul in node.args:
        if _is_mul(mul) and mul.args[0] is not mul.args[1] and len(mul.users) == 1 and _sixth_of(node, mul) is not None:
            for x, r in (mul.args, mul.args[::-1]):
                found = _relu6_of_plus3(r, modules) if len(r.users) == 1 else None
                if found is not None and found[0] is x:
                    return x, [node, mul] + found[1], "mul_" + _sixth_of(node, mul)
    if not _is_mul(node) or node.args[0] is node.args[1]:
        return None
    # x * (r / 6), x * (r * (1 / 6)), x * hardsigmoid(x): `node` multiplies x by its gate
    for x, g in (node.args, node.args[::-1]):
        if len(g.users) != 1:
            continue
        if g.op == "call_module":
            m = modules.get(g.target)
            if type(m) is nn.Hardsigmoid and not m.inplace and len(g.args) == 1 and not g.kwargs and g.args[0] is x:
                return x, [node, g], "hardsigmoid"
        elif g.op == "call_function" and g.target is F.hardsigmoid:
            if len(g.args) == 1 and g.args[0] is x and set(g.kwargs) <= {"inplace"} and not g.kwargs.get("inplace", False):
                return x, [node, g], "hardsigmoid"
        elif not g.kwargs and len(g.args) == 2:
            for r in g.args:
                found = _relu6_of_plus3(r, modules) if isinstance(r, fx.Node) and len(r.users) == 1 and _sixth_of(g, r) is not None else None
                if found is not None and found[0] is x:
                    return x, [node, g] + found[1], "gate_" + _sixth_of(g, r)
    return None


def _hardswish_multiply(mul, modules):
    """Whether multiply `mul` is part of a hard swish _hardswish_of takes: its last node, or the product `x * r` its scaling reads."""
    if _hardswish_of(mul, modules) is not None:
        return True
    nxt = _sole_user(mul)
    found = _hardswish_of(nxt, modules) if nxt is not None else None
    return found is not None and mul in found[1]


def _hardswish_pass(gm, report, planned, dry_run, dwpw):
    """Hard-swish activations (fuse_inference(hardswish=True)): nn.Hardswish / `x * relu6(x + 3) / 6` / `x * hardsigmoid(x)` of a 4-D map
    becomes a node (HardswishLayer) that hands the plan convolutions behind it - depthwise ones included - their activation codes and
    every other reader (a squeeze-excite pool, the gate node, a shortcut add) the activated fp32 map from the same launch, computed in
    the order of the spelling it replaces.  Readers and the no-taker case: _swish_pass's.  `planned`: plan node -> what the main pass
    decided for it (_Decision); whatever that is for the convolution behind the hard swish stays - only its input changes."""
    def match(node, modules):
        found = _hardswish_of(node, modules)
        if found is None:
            return None
        x, nodes, spelling = found
        taken = _code_readers(planned, node, dw=True, dwpw=dwpw)
        if taken is None:      # nobody takes codes: one pass over the map instead of four, where it is known to be a map
            if not _is_map(x, planned, modules):
                return None
            taken = _CodeReaders(None, (), True, None, None, 0, False)
        order = _HARDSWISH_ORDER[spelling]
        dec = _HardswishDecision(x.name, spelling, order, tuple(n.name for n in nodes))
        return _Splice(HardswishLayer, dict(_decided(taken), order=order, decision=dec), node, (x,), taken.takers, nodes)
    _run_node_pass(gm, report, "hardswish", "hardswishes", match, dry_run)


class LayerNormLayer(_MapCodesLayer):
    """nn.LayerNorm((C,)) of fp32 rows [..., C] straight to the activation codes of the Linear plan layers that read the normalised
    rows (csrc/layernorm.hip): the normalisation, the normalised fp32 tensor and the consumer's quantise pass as one read of the rows.
    `norm`: the nn.LayerNorm, whose parameters and eps are read at every call; `emit`: the readers' activation quantiser; `want_out`:
    whether anyone reads the fp32 values; `c` = the readers' in-features.  An input that at run time is no fp32 device tensor of width
    `c` (or parameters that are not fp32) is normalised with F.layer_norm and quantised with K.fake_quant: the values of the unfused
    graph.  Returns `(fp32 or None, codes)`."""

    def __init__(self, norm, emit, want_out, c):
        super().__init__(emit, want_out, c, c, 0, False)
        self.norm = norm

    def forward(self, x):
        m = self.norm
        fp32 = all(p is None or p.dtype == torch.float32 for p in (m.weight, m.bias))
        if not (x.is_cuda and x.dtype == torch.float32 and x.dim() >= 1 and x.shape[-1] == self.c and fp32):
            return self._torch_rows(F.layer_norm(x, m.normalized_shape, m.weight, m.bias, m.eps))
        return K.layernorm_quant(x, m.weight, m.bias, m.eps, emit=self.emit.emit(x.numel()), want_out=self.want_out)


def _layernorm_pass(gm, report, planned, dry_run):
    """LayerNorms (fuse_inference(layer_norms=True)): `nn.LayerNorm((C,)) -> Linear plan layers` becomes a node that hands the Linear
    layers their activation codes (LayerNormLayer) and anyone else the normalised fp32 rows from the same launch.  Taken: an nn.LayerNorm
    called with one positional argument, normalising the last dimension only, C % 4 == 0, 4 <= C <= K.LAYERNORM_MAX_C, a finite eps > 0,
    with at least one taker, every taker a Linear of C in-features.  `planned`: plan node -> what the main pass decided for it
    (_Decision); whatever that is for the Linear behind the LayerNorm stays - only its input changes, from fp32 to codes."""
    def match(node, modules):
        m = modules.get(node.target) if node.op == "call_module" else None
        if type(m) is not nn.LayerNorm or len(node.args) != 1 or node.kwargs or not isinstance(node.args[0], fx.Node):
            return None
        shape = tuple(m.normalized_shape)
        if len(shape) != 1 or shape[0] % 4 or not 4 <= shape[0] <= K.LAYERNORM_MAX_C or not (m.eps > 0 and math.isfinite(m.eps)):
            return None
        taken = _code_readers(planned, node, linear=True)
        if taken is None or taken.c != shape[0] or any(planned[u].mod.weight.dim() != 2 for u in taken.takers):
            return None
        ctor = dict(norm=m, emit=taken.emit, want_out=taken.want_out, c=taken.c)
        return _Splice(LayerNormLayer, ctor, node, (node.args[0],), taken.takers, [node])
    _run_node_pass(gm, report, "layernorm", "layer_norms", match, dry_run)


class AttentionLayer(_MapCodesLayer):
    """softmax(scale * q k^T) v of fp32 views [B, H, T, D] as one flash-forward launch (csrc/attention.hip), and - `merged` - the
    merge-heads `permute(0, 2, 1, 3)` + reshape behind it as a free view: the node returns [B, Tq, H * D] and hands the Linear plan
    layer that reads it (`to_out`) its activation codes from the same launch.  `emit`: the reader's activation quantiser or None (an
    fp32-only node); `want_out`: whether anyone reads the fp32 values; `c`: the reader's in-features; `scale`: the Python float of the
    graph's multiply, or None (F.scaled_dot_product_attention's default, D ** -0.5); `sdpa`: None, or the keyword arguments of the
    graph's F.scaled_dot_product_attention call; `flatten`: the tail is `flatten(2)`, else the reshape's three shape arguments arrive
    at run time (graph values, checked there).  Not merged: [B, H, Tq, D], fp32 only.  The torch restatement - the graph's own ops,
    then K.fake_quant - runs for anything that is not three fp32 device views the kernel reads in place (K.attention_views) with
    D in K.ATTENTION_DIMS, a merged width other than H * D or `c`.  Returns `(fp32 or None, codes or None)`."""

    def __init__(self, emit, want_out, c, scale, merged, sdpa=None, flatten=False):
        super().__init__(emit, want_out, c, c, 0, False)
        self.scale, self.merged, self.flatten = (None if scale is None else float(scale)), bool(merged), bool(flatten)
        self.sdpa = None if sdpa is None else dict(sdpa)

    def _torch(self, q, k, v, shape):
        """The unfused graph: the products and the softmax as they were spelled, the tail, the reader's quantise pass."""
        if self.sdpa is not None:
            o = F.scaled_dot_product_attention(q, k, v, **self.sdpa)
        else:
            o = torch.matmul(torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * self.scale, dim=-1), v)
        if self.merged:
            o = o.permute(0, 2, 1, 3)
            o = o.flatten(2) if self.flatten else o.reshape(*shape)
        return self._torch_rows(o) if self.emit is not None else (o, None)

    def forward(self, q, k, v, *shape):
        ok = q.is_cuda and K.attention_views(q, k, v)
        if ok and self.merged:
            b, h, tq, d = q.shape
            want = [b, tq, h * d]
            if not self.flatten:      # (a reshape to three dimensions, at most one of them -1: the merged heads or something else)
                dims = [int(x) for x in shape]
                free = [i for i, x in enumerate(dims) if x == -1]
                if len(free) == 1 and all(x == y for i, (x, y) in enumerate(zip(dims, want)) if i != free[0]):
                    dims = want
                ok = dims == want
            ok = ok and (self.emit is None or h * d == self.c)
        if not ok:
            return self._torch(q, k, v, shape)
        scale = q.shape[-1] ** -0.5 if self.scale is None else self.scale
        emit = None if self.emit is None else self.emit.emit(q.numel())
        return K.attention_quant(q, k, v, scale, emit=emit, want_out=self.want_out, merged=self.merged)


_MATMUL_FNS = (torch.matmul, operator.matmul)
_SDPA_NAMES = ("query", "key", "value", "attn_mask", "dropout_p", "is_causal", "scale")


def _softmax_of(node, modules):
    """The graph value x if `node` is a softmax of x over its last axis of four (`-1` or `3`) in a spelling the plan takes -
    torch.softmax, F.softmax, the method, an nn.Softmax module; no dtype argument - else None."""
    if not isinstance(node, fx.Node):
        return None
    if node.op == "call_module":
        m = modules.get(node.target)
        ok = type(m) is nn.Softmax and len(node.args) == 1 and not node.kwargs
        x, dim = (node.args[0], m.dim) if ok else (None, None)
    elif (node.op == "call_function" and node.target in (torch.softmax, F.softmax)) or (node.op == "call_method" and node.target == "softmax"):
        if not 1 <= len(node.args) <= 2 or not set(node.kwargs) <= {"dim", "dtype", "_stacklevel"} or (len(node.args) == 2 and "dim" in node.kwargs):
            return None
        if node.kwargs.get("dtype") is not None:
            return None
        x, dim = node.args[0], (node.args[1] if len(node.args) == 2 else node.kwargs.get("dim"))
    else:
        return None
    return x if isinstance(x, fx.Node) and isinstance(dim, int) and not isinstance(dim, bool) and dim in (-1, 3) else None


def _attention_core(node, modules):
    """(q, k, v, scale, sdpa keyword arguments or None, the nodes it is made of) if `node` is the last node of an attention core the
    plan takes - `matmul(softmax(matmul(q, k.transpose(-1, -2)) * c, dim=-1), v)`, c a Python float on either side, every
    intermediate read once; or F.scaled_dot_product_attention(q, k, v) without mask, dropout or causal flag, `scale` None or a float -
    else None."""
    if node.op == "call_function" and node.target is F.scaled_dot_product_attention:
        if len(node.args) > len(_SDPA_NAMES) or not set(node.kwargs) <= set(_SDPA_NAMES[len(node.args):]):
            return None
        given = dict(zip(_SDPA_NAMES, node.args), **node.kwargs)
        q, k, v, scale = given.get("query"), given.get("key"), given.get("value"), given.get("scale")
        if not all(isinstance(t, fx.Node) for t in (q, k, v)) or given.get("attn_mask") is not None:
            return None
        p, causal = given.get("dropout_p", 0.0), given.get("is_causal", False)
        if isinstance(p, bool) or not isinstance(p, (int, float)) or p != 0 or causal is not False:
            return None
        if not (scale is None or (isinstance(scale, float) and math.isfinite(scale))):
            return None
        return q, k, v, scale, ({} if scale is None else {"scale": scale}), [node]
    if not _is_call(node, _MATMUL_FNS, "matmul") or len(node.args) != 2:
        return None
    attn, v = node.args
    scores = _softmax_of(attn, modules)
    if scores is None or not isinstance(v, fx.Node) or _sole_user(attn) is None or _sole_user(scores) is None:
        return None
    if not _is_call(scores, _MUL_FNS, "mul") or len(scores.args) != 2:
        return None
    dots, c = scores.args if isinstance(scores.args[0], fx.Node) else scores.args[::-1]
    if not isinstance(c, float) or not math.isfinite(c) or _sole_user(dots) is None:
        return None
    if not _is_call(dots, _MATMUL_FNS, "matmul") or len(dots.args) != 2:
        return None
    q, kt = dots.args
    if not isinstance(q, fx.Node) or _sole_user(kt) is None or not _is_call(kt, (torch.transpose,), "transpose") or len(kt.args) != 3:
        return None
    k, d0, d1 = kt.args
    if not isinstance(k, fx.Node) or {d0, d1} not in ({-1, -2}, {2, 3}, {-1, 2}, {-2, 3}) or isinstance(d0, bool) or isinstance(d1, bool):
        return None
    return q, k, v, c, None, [node, attn, scores, dots, kt]


def _static_head_dim(node):
    """D where the graph spells it as a Python int: `node` [B, H, T, D] is - through getitem's on leading axes and permutes that keep
    the last axis last - a reshape / view whose last size is an int.  Else None (decided at run time)."""
    for _ in range(4):
        if not isinstance(node, fx.Node) or node.kwargs:
            return None
        if node.op == "call_function" and node.target is operator.getitem and isinstance(node.args[1], int):
            node = node.args[0]
        elif node.op == "call_method" and node.target == "permute":
            dims = node.args[1:]
            dims = tuple(dims[0]) if len(dims) == 1 and isinstance(dims[0], (tuple, list)) else dims
            if not dims or dims[-1] not in (-1, len(dims) - 1):
                return None
            node = node.args[0]
        elif node.op == "call_method" and node.target in ("reshape", "view"):
            sizes = node.args[1:]
            sizes = tuple(sizes[0]) if len(sizes) == 1 and isinstance(sizes[0], (tuple, list)) else sizes
            last = sizes[-1] if sizes else None
            return last if isinstance(last, int) and not isinstance(last, bool) and last > 0 else None
        else:
            return None
    return None


def _merge_heads_tail(node):
    """(permute node, reshape node, its shape arguments or None for flatten(2)) if the sole reader of `node` [B, H, T, D] is
    `permute(0, 2, 1, 3)` / `transpose(1, 2)` whose sole reader reshapes to rank 3 - `reshape` / `view` with three sizes (Python
    ints or graph values) or `flatten(2)` - else None."""
    perm = _sole_user(node)
    shape = _sole_user(perm)
    if shape is None or perm.kwargs or perm.op != "call_method" or not perm.args or perm.args[0] is not node:
        return None
    dims = perm.args[1:]
    if len(dims) == 1 and isinstance(dims[0], (tuple, list)):
        dims = tuple(dims[0])
    if not ((perm.target == "permute" and tuple(dims) == (0, 2, 1, 3)) or (perm.target == "transpose" and tuple(sorted(dims)) == (1, 2))):
        return None
    if shape.kwargs or not shape.args or shape.args[0] is not perm:
        return None
    if (shape.op == "call_method" and shape.target == "flatten") or (shape.op == "call_function" and shape.target is torch.flatten):
        return (perm, shape, None) if tuple(shape.args[1:]) in ((2,), (2, -1), (2, 3)) else None
    if shape.op != "call_method" or shape.target not in ("reshape", "view"):
        return None
    sizes = shape.args[1:]
    if len(sizes) == 1 and isinstance(sizes[0], (tuple, list)):
        sizes = tuple(sizes[0])
    ok = len(sizes) == 3 and all(isinstance(x, fx.Node) or (isinstance(x, int) and not isinstance(x, bool)) for x in sizes)
    return (perm, shape, tuple(sizes)) if ok else None


def _attention_pass(gm, report, planned, dry_run):
    """Attention (fuse_inference(attention=True)): the core `softmax(q k^T * c) v` (_attention_core) becomes one node (AttentionLayer,
    csrc/attention.hip).  With the merge-heads tail behind it (_merge_heads_tail) the node stands where the reshape stood, returns
    [B, Tq, H * D], and the Linear plan layers reading it - one quantiser, as for a LayerNorm - take its codes; anyone else reads the
    fp32 values of the same launch.  Without the tail it stands where the second product stood and returns fp32 [B, H, Tq, D].
    `planned`: plan node -> what the main pass decided for it (_Decision), which stays - only the reader's input changes."""
    def match(node, modules):
        core = _attention_core(node, modules) if node.op in ("call_function", "call_method") else None
        if core is None:
            return None
        q, k, v, scale, sdpa, made_of = core
        if _static_head_dim(q) not in (None,) + K.ATTENTION_DIMS:      # (a head dimension the kernel is not built for, spelled as an int)
            return None
        perm, shape, sizes = _merge_heads_tail(node) or (None, None, ())
        taken = _code_readers(planned, shape, linear=True) if shape is not None else None
        if taken is None or any(planned[u].mod.weight.dim() != 2 for u in taken.takers):      # nobody takes codes: an fp32-only node
            taken = _CodeReaders(None, [], True, 0, 0, 0, False)
        ctor = dict(emit=taken.emit, want_out=taken.want_out, c=taken.c, scale=scale, merged=shape is not None, sdpa=sdpa,
                    flatten=sizes is None)
        if shape is None:
            return _Splice(AttentionLayer, ctor, node, (q, k, v), [], made_of)
        return _Splice(AttentionLayer, ctor, shape, (q, k, v) + (sizes or ()), taken.takers, [shape, perm] + made_of)
    _run_node_pass(gm, report, "attention", "attentions", match, dry_run)


_GELU_ALPHA = 0.70710678118654752440      # 1 / sqrt(2): as a Python scalar torch multiplies an fp32 tensor by its fp32 rounding


class GeluLayer(_MapCodesLayer):
    """GELU in its erf form (approximate="none") straight to the activation codes of the plan layers that read the activated tensor
    (csrc/gelu.hip): the activation, the activated fp32 tensor and the consumer's quantise pass as one read.  `rows`: the readers are
    Linear layers - the input is rows [..., c] of any rank; else plan convolutions - the input is an (N, c, H, W) map and the code rows
    are `c_pad` wide, as a SwishLayer's.  An input that at run time is no fp32 device tensor of that form takes the same five steps in
    torch ops and K.fake_quant.  Returns `(fp32 or None, codes)`."""

    def __init__(self, emit, want_out, c, c_pad, pad_code, shift=False, rows=False):
        super().__init__(emit, want_out, c, c_pad, pad_code, shift)
        self.rows = bool(rows)

    @staticmethod
    def _gelu(x):
        """csrc/gelu.hip's five steps in torch ops (each one rounded to the tensor's dtype)."""
        return (x * 0.5) * (1.0 + torch.erf(x * _GELU_ALPHA))

    def forward(self, x):
        device_fp32 = x.is_cuda and x.dtype == torch.float32
        if self.rows:
            if not (device_fp32 and x.dim() >= 1 and x.shape[-1] == self.c):
                return self._torch_rows(self._gelu(x))
            out, codes = K.gelu_quant(x.reshape(-1, self.c), **self._to_codes(x.numel()))
            return (None if out is None else out.reshape(x.shape)), codes.reshape(x.shape)
        if not (device_fp32 and x.dim() == 4 and x.shape[1] == self.c):
            return self._torch_codes(self._gelu(x))
        return K.gelu_quant(x, **self._to_codes(x.numel()))


def _gelu_of(node, modules):
    """The graph value x if `node` is the erf-form GELU of x in a spelling the plan takes - nn.GELU() / nn.GELU(approximate="none") called
    with one positional argument, F.gelu(x) / F.gelu(x, approximate="none") (positional too) - else None.  The tanh form is none of them.
    A user module whose body is one of these is traced into it."""
    if node.op == "call_module":
        m = modules.get(node.target)
        x = node.args[0] if len(node.args) == 1 and not node.kwargs else None
        return x if type(m) is nn.GELU and m.approximate == "none" and isinstance(x, fx.Node) else None
    if node.op == "call_function" and node.target in (F.gelu, torch._C._nn.gelu):
        if not 1 <= len(node.args) <= 2 or not set(node.kwargs) <= {"approximate"} or (len(node.args) == 2 and node.kwargs):
            return None
        approximate = node.args[1] if len(node.args) == 2 else node.kwargs.get("approximate", "none")
        return node.args[0] if approximate == "none" and isinstance(node.args[0], fx.Node) else None
    return None


def _gelu_pass(gm, report, planned, dry_run, dwpw):
    """GELUs (fuse_inference(gelu=True)): `GELU -> plan layers` becomes a node that hands the plan layers behind it their activation codes
    (GeluLayer) and anyone else the activated fp32 tensor from the same launch.  The takers are Linear plan layers (rows) or 4-D "gemm"
    plan convolutions (a map: the channel-padded code rows of the average-pool rule), never both; a GELU nobody takes as codes is left
    alone.  `planned`: plan node -> what the main pass decided for it (_Decision); whatever that is for the layer behind the GELU stays
    - only its input changes, from fp32 to codes."""
    def match(node, modules):
        x = _gelu_of(node, modules)
        taken = _code_readers(planned, node, dwpw=dwpw, linear=True) if x is not None else None
        if taken is None:
            return None
        rows = planned[taken.takers[0]].mod.weight.dim() == 2
        return _Splice(GeluLayer, dict(_decided(taken), rows=rows), node, (x,), taken.takers, [node])
    _run_node_pass(gm, report, "gelu", "gelus", match, dry_run)


_PatchRows = collections.namedtuple("_PatchRows", "src chain c g1 g2 p emit takers want_out")
_TokenAssemble = collections.namedtuple("_TokenAssemble", "x cls pos rows c chain")


class PatchRowsLayer(_MapCodesLayer):
    """A vision transformer's patch rows - `img.reshape(-1, C, g1, p, g2, p).permute(0, 2, 4, 3, 5, 1).reshape(-1, g1 * g2, p * p * C)` -
    straight to the activation codes of the Linear plan layer that embeds them (csrc/patch_rows.hip): the strided copy, the fp32 rows
    and the consumer's quantise pass as one read of the image.  `decision`: the pass's record (_PatchRows: channels, grid, patch size,
    the readers' activation quantiser, whether anyone reads the fp32 rows).  An input that at run time is no (B, C, g1 * p, g2 * p)
    batch takes the graph's own three ops and K.fake_quant; one of that shape which the kernel does not read in place (not fp32, not on
    the device, channels_last, misaligned) takes K.patch_rows_quant's torch restatement: the unfused graph's values either way.
    Returns `(fp32 or None, codes)`."""

    def __init__(self, decision):
        d = decision
        k = d.p * d.p * d.c
        super().__init__(d.emit, d.want_out, k, k, 0, False)
        self.channels, self.grid, self.patch, self.tokens = int(d.c), (int(d.g1), int(d.g2)), int(d.p), int(d.g1 * d.g2)
        self.decision = d._replace(src=d.src.name, chain=tuple(n.name for n in d.chain), takers=tuple(n.name for n in d.takers))

    def forward(self, img):
        (g1, g2), p, c = self.grid, self.patch, self.channels
        if img.dim() != 4 or tuple(img.shape[1:]) != (c, g1 * p, g2 * p):
            return self._torch_rows(img.reshape(-1, c, g1, p, g2, p).permute(0, 2, 4, 3, 5, 1).reshape(-1, g1 * g2, p * p * c))
        return K.patch_rows_quant(img, p, emit=self.emit.emit(img.numel()), want_out=self.want_out)


class TokenAssembleLayer(nn.Module):
    """`torch.cat((cls.expand(B, -1, -1), x), dim=1) + pos` - the class token in front of the embedded patches, the position embedding
    added - as one launch (csrc/tokens.hip): fp32 [B, T + 1, C], the bits of the two torch ops.  The node is called with the graph's
    own `cls` and `pos` parameters, which are therefore read at every call; `decision`: the pass's record (_TokenAssemble; `rows`: the
    static n of a `pos[:, :n]` slice, or None; `c`: the width).  Inputs the kernel does not take run the torch expression itself
    (K.assemble_tokens)."""

    def __init__(self, decision):
        super().__init__()
        d = decision
        self.rows, self.c = (None if d.rows is None else int(d.rows)), int(d.c)
        self.decision = d._replace(x=d.x.name, cls=d.cls.name, pos=d.pos.name, chain=tuple(n.name for n in d.chain))

    def forward(self, x, cls, pos):
        return K.assemble_tokens(x, cls, pos if self.rows is None else pos[:, :self.rows])


def _static_sizes(node, methods):
    """The sizes of `node` = x.reshape(...) / x.view(...) / x.permute(...) (one of `methods`; spelled one by one or as one tuple) if
    every one of them is a Python int, else None."""
    if not isinstance(node, fx.Node) or node.op != "call_method" or node.target not in methods or node.kwargs or len(node.args) < 2:
        return None
    sizes = node.args[1:]
    if len(sizes) == 1 and isinstance(sizes[0], (tuple, list)):
        sizes = tuple(sizes[0])
    return tuple(sizes) if all(isinstance(s, int) and not isinstance(s, bool) for s in sizes) and isinstance(node.args[0], fx.Node) else None


def _patch_rows_of(planned, last):
    """What `last` is to the patch-embedding pass: None (no candidate: not a reshape to three sizes of a six-axis permute of a reshape
    to six sizes), a str (a candidate left alone: why), or the _PatchRows decision."""
    s3 = _static_sizes(last, ("reshape", "view"))
    perm = last.args[0] if s3 is not None else None
    order = _static_sizes(perm, ("permute",))
    first = perm.args[0] if order is not None else None
    s6 = _static_sizes(first, ("reshape", "view"))
    if s3 is None or order is None or s6 is None or len(s3) != 3 or len(order) != 6 or len(s6) != 6:
        return None
    if order != (0, 2, 4, 3, 5, 1):
        return f"a permute {order}, not (0, 2, 4, 3, 5, 1)"
    if _sole_user(first) is None or _sole_user(perm) is None:
        return "an intermediate of the rearrangement has a second reader"
    lead, c, g1, p, g2, p2 = s6
    if lead != -1 or s3[0] != -1 or min(c, g1, p, g2) < 1 or p != p2 or s3[1:] != (g1 * g2, p * p * c):
        return f"sizes {s6} -> {s3} are not (-1, C, g1, p, g2, p) -> (-1, g1 * g2, p * p * C)"
    if p % 4:
        return f"patch size {p} is no multiple of 4"
    if g2 * p * p * c > K.PATCH_MAX_STRIP:
        return f"a strip of {g2 * p * p * c} elements does not fit the kernel's LDS"
    taken = _code_readers(planned, last, linear=True)
    if taken is None or any(planned[u].mod.weight.dim() != 2 for u in taken.takers):
        return "no Linear plan layer (or no single quantiser) takes the rows as codes"
    if taken.c != p * p * c:
        return f"the Linear behind the rows has {taken.c} in-features, the rows {p * p * c}"
    return _PatchRows(first.args[0], (last, perm, first), c, g1, g2, p, taken.emit, tuple(taken.takers), taken.want_out)


def _fetch_attr(gm, node):
    """The tensor behind get_attr node `node`, else None."""
    if not isinstance(node, fx.Node) or node.op != "get_attr":
        return None
    obj = gm
    for part in str(node.target).split("."):
        obj = getattr(obj, part, None)
    return obj if isinstance(obj, torch.Tensor) else None


def _static_tokens(gm, planned, x):
    """T where the graph says how many rows per image `x` [B, T, C] has - `x` is the fp32 output of a Linear plan layer (or that
    layer's wrapper) fed by a PatchRowsLayer node or by a reshape / view to three static sizes - else None (checked at run time)."""
    if x.op == "call_function" and x.target is operator.getitem and x.args[0] in planned:
        x = x.args[0]
    if x.op != "call_module" or len(x.args) != 1 or not isinstance(x.args[0], fx.Node):
        return None
    src = x.args[0]
    if src.op == "call_function" and src.target is operator.getitem and src.args[0].op == "call_module":
        m = dict(gm.named_modules()).get(src.args[0].target)
        return m.tokens if isinstance(m, PatchRowsLayer) else None
    s3 = _static_sizes(src, ("reshape", "view"))
    return s3[1] if s3 is not None and len(s3) == 3 and s3[1] > 0 else None


def _token_assemble_of(gm, planned, add):
    """What `add` is to the patch-embedding pass: None (no candidate: not an add of a torch.cat whose first part is an expanded
    parameter), a str (a candidate left alone: why), or the _TokenAssemble decision."""
    if not _is_add(add):
        return None
    for cat, pos in (add.args, add.args[::-1]):
        if cat.op == "call_function" and cat.target in (torch.cat, torch.concat, torch.concatenate) and cat.args:
            break
    else:
        return None
    parts = cat.args[0]
    given = dict(zip(("dim",), cat.args[1:]), **cat.kwargs)
    if not (isinstance(parts, (tuple, list)) and len(parts) == 2 and all(isinstance(t, fx.Node) for t in parts)) or len(cat.args) > 2:
        return None
    expand, x = parts
    if not _is_call(expand, (), "expand") or _fetch_attr(gm, expand.args[0]) is None:
        return None
    if set(given) != {"dim"} or given["dim"] != 1 or isinstance(given["dim"], bool):
        return "the concatenation is not along dim 1"
    sizes = expand.args[1:]
    if len(sizes) == 1 and isinstance(sizes[0], (tuple, list)):
        sizes = tuple(sizes[0])
    if len(sizes) != 3 or tuple(sizes[1:]) != (-1, -1):
        return "the class token is not expanded along the batch alone"
    if _sole_user(expand) is None or _sole_user(cat) is None:
        return "an intermediate (the expanded class token, the concatenation) has a second reader"
    if _inplace_add(add) and add.args[0] is not cat:
        return "an in-place add into the position embedding"
    rows, sliced = None, pos
    if pos.op == "call_function" and pos.target is operator.getitem and len(pos.args) == 2:      # pos[:, :n], n a Python int
        idx = pos.args[1]
        ok = (isinstance(idx, tuple) and len(idx) == 2 and all(isinstance(s, slice) for s in idx) and idx[0] == slice(None) and
              idx[1].start is None and idx[1].step is None and isinstance(idx[1].stop, int) and not isinstance(idx[1].stop, bool))
        if not ok or _sole_user(pos) is None:
            return "the position embedding is sliced in another way than [:, :n] with a static n"
        rows, pos = idx[1].stop, pos.args[0]
    cls_t, pos_t = _fetch_attr(gm, expand.args[0]), _fetch_attr(gm, pos)
    if pos_t is None:
        return "the position embedding is not a parameter of the model"
    if cls_t.dim() != 3 or tuple(cls_t.shape[:2]) != (1, 1) or cls_t.shape[2] % 4 or cls_t.shape[2] < 4:
        return f"a class token of shape {tuple(cls_t.shape)}, not [1, 1, C] with C % 4 == 0"
    c = int(cls_t.shape[2])
    if pos_t.dim() != 3 or pos_t.shape[0] != 1 or pos_t.shape[2] != c or (rows is not None and not 2 <= rows <= pos_t.shape[1]):
        return f"a position embedding of shape {tuple(pos_t.shape)}" + ("" if rows is None else f"[:, :{rows}]") + f", not [1, T + 1, {c}]"
    length = int(pos_t.shape[1]) if rows is None else rows
    tokens = _static_tokens(gm, planned, x)
    if length < 2 or (tokens is not None and tokens + 1 != length):
        return f"a position embedding of {length} rows for {'?' if tokens is None else tokens} + 1 tokens"
    return _TokenAssemble(x, expand.args[0], pos, rows, c, (add, cat, expand) if rows is None else (add, sliced, cat, expand))


def _patch_embed_pass(gm, report, planned, dry_run):
    """The front of a vision transformer (fuse_inference(patch_embed=True)).  The rearrangement into patch rows in front of a Linear
    plan layer becomes a node that hands that layer its activation codes from one read of the image (PatchRowsLayer; _patch_rows_of
    says what is taken), and `cat((cls.expand(B, -1, -1), x), dim=1) + pos` one launch (TokenAssembleLayer; _token_assemble_of).
    `planned`: plan node -> what the main pass decided for it (_Decision), which stays - only the embedding's input changes, from fp32
    to codes.  A candidate that is left alone keeps its nodes, and `report.patch_embed_left` says why."""
    def rows(node, modules):
        d = _patch_rows_of(planned, node)
        return _Splice(PatchRowsLayer, dict(decision=d), node, (d.src,), d.takers, d.chain) if isinstance(d, _PatchRows) else d

    def tokens(node, modules):
        d = _token_assemble_of(gm, planned, node)
        return _Splice(TokenAssembleLayer, dict(decision=d), node, (d.x, d.cls, d.pos), (), d.chain) if isinstance(d, _TokenAssemble) else d
    _run_node_pass(gm, report, "patch_rows", "patch_rows", rows, dry_run)
    _run_node_pass(gm, report, "tokens", "token_assemblies", tokens, dry_run, outputs=1)


def _pool_dims(node, modules):
    """Rank of the result (4: keeps [N, C, 1, 1]; 2: [N, C]) if `node` is a global average pool in a spelling the plan folds -
    nn.AdaptiveAvgPool2d(1 | (1, 1)), F.adaptive_avg_pool2d(x, 1 | (1, 1)), x.mean((2, 3)) / torch.mean(x, (2, 3)) / [2, 3] / dim=,
    keepdim either way - else None."""
    one = lambda v: v == 1 or (isinstance(v, (tuple, list)) and tuple(v) == (1, 1))  # noqa: E731
    if node.op == "call_module":
        m = modules.get(node.target)
        return 4 if type(m) is nn.AdaptiveAvgPool2d and one(m.output_size) and len(node.args) == 1 and not node.kwargs else None
    if node.op == "call_function" and node.target is F.adaptive_avg_pool2d:
        given = dict(zip(("input", "output_size"), node.args), **node.kwargs)
        return 4 if set(given) == {"input", "output_size"} and isinstance(given["input"], fx.Node) and one(given["output_size"]) else None
    if (node.op == "call_method" and node.target == "mean") or (node.op == "call_function" and node.target is torch.mean):
        given = dict(zip(("input", "dim", "keepdim"), node.args), **node.kwargs)
        if not set(given) <= {"input", "dim", "keepdim"} or not isinstance(given.get("input"), fx.Node):
            return None
        dim, keep = given.get("dim"), given.get("keepdim", False)
        if not (isinstance(dim, (tuple, list)) and sorted(dim) in ([2, 3], [-2, -1]) and isinstance(keep, bool)):
            return None
        return 4 if keep else 2
    return None


def _batch_size_of(node, dim=0):
    """Whether `node` is `t.size(0)` / `t.shape[0]` of some tensor `t` (the first argument of a `.view(N, -1)`); `dim`: another axis."""
    if not isinstance(node, fx.Node):
        return False
    if node.op == "call_method" and node.target == "size":
        return len(node.args) == 2 and node.args[1] == dim and not node.kwargs
    if node.op == "call_function" and node.target is operator.getitem and node.args[1] == dim:
        src = node.args[0]
        return (isinstance(src, fx.Node) and ((src.op == "call_function" and src.target is getattr and src.args[1] == "shape") or
                                              (src.op == "call_method" and src.target == "size" and len(src.args) == 1)))
    return False


def _flatten_rank(node, src, rank):
    """Rank after `node` if it is one of the reshapes that follow a global pool - torch.flatten(x, 1) / x.flatten(1), x.view(N, -1) /
    x.reshape(N, -1) with N = t.size(0) / t.shape[0] (not an int literal), x.squeeze() / x.squeeze(d) over a pooled axis - applied to `src`; else None."""
    fn, meth = node.op == "call_function", node.op == "call_method"
    if not (fn or meth) or not node.args or node.args[0] is not src:
        return None
    if (fn and node.target is torch.flatten) or (meth and node.target == "flatten"):
        given = dict(zip(("input", "start_dim", "end_dim"), node.args), **node.kwargs)
        return 2 if given.get("start_dim") == 1 and given.get("end_dim", -1) in (-1, rank - 1) and set(given) <= {"input", "start_dim", "end_dim"} else None
    if meth and node.target in ("view", "reshape") and not node.kwargs:
        shape = node.args[1:]
        if len(shape) == 1 and isinstance(shape[0], (tuple, list)):
            shape = tuple(shape[0])
        return 2 if len(shape) == 2 and shape[1] == -1 and _batch_size_of(shape[0]) else None     # (an int literal is [N, C] only at that batch size)
    if (fn and node.target is torch.squeeze) or (meth and node.target == "squeeze"):
        given = dict(zip(("input", "dim"), node.args), **node.kwargs)
        if set(given) == {"input"}:
            return 2
        d = given.get("dim")
        if set(given) != {"input", "dim"} or not isinstance(d, int) or isinstance(d, bool):
            return None
        d = d if d >= 0 else rank + d
        return rank - 1 if 2 <= d < rank else None
    return None


def _gap_pass(gm, report, mode, planned, dry_run):
    """Global-average-pool heads (fuse_inference(gap_head=...)): `pool -> flatten -> quantised Linear` becomes a node that hands the
    Linear its activation codes [N, C].  `planned`: plan node -> what the main pass decided for it (_Decision)."""
    graph = gm.graph
    modules = dict(gm.named_modules())
    count = 0

    def aux(n, inside):      # a batch-size read (x.size(0), x.shape[0] and their pieces) used by the chain's nodes only
        if not ((n.op == "call_method" and n.target == "size") or (n.op == "call_function" and n.target in (getattr, operator.getitem))):
            return False
        return bool(n.users) and all(u in inside or aux(u, inside) for u in n.users)

    def real_users(n, inside):
        return [u for u in n.users if not aux(u, inside)]

    for pool in list(graph.nodes):
        rank = _pool_dims(pool, modules)
        if rank is None:
            continue
        x = pool.args[0] if pool.args else pool.kwargs["input"]
        # ---- pool -> reshapes -> [N, C], each link the only reader of the one before ----
        chain, last = [pool], pool
        while True:
            nxt = [u for u in last.users if _flatten_rank(u, last, rank) is not None]
            if len(nxt) != 1 or len(real_users(last, set(chain) | set(nxt))) != 1:
                break
            rank = _flatten_rank(nxt[0], last, rank)
            chain.append(nxt[0])
            last = nxt[0]
        if rank != 2:
            continue
        inside = set(chain)
        if any(real_users(n, inside) != [c] for n, c in zip(chain[:-1], chain[1:])):
            continue
        # ---- the readers: plan-eligible linear layers, through their activation argument, take codes ----
        def linear_act(u):
            d = planned.get(u)
            if d is None or d.dual or d.spec.kind != "gemm" or u.args[0] is not last or last in u.args[1:]:
                return None
            w = d.mod.weight
            return d.spec.act if w.dim() == 2 and w.shape[1] % 64 == 0 else None
        users = real_users(last, inside)
        acts = {u: linear_act(u) for u in users}
        keys = [a.key for a in acts.values() if a is not None]
        if not keys:
            continue
        key = max(set(keys), key=keys.count)
        takers = [u for u, a in acts.items() if a is not None and a.key == key]
        emit = acts[takers[0]]
        want_out = len(takers) != len(users)
        # ---- the producer: a plan convolution read by the pool alone becomes the fused head (True: where profitable; "fused": always) ----
        prod = x.args[0] if x.op == "call_function" and x.target is operator.getitem and x.args[1] == 0 else None
        d = planned.get(prod)
        fused = False
        if mode in (True, "fused") and d is not None and real_users(x, inside) == [pool]:
            w = d.mod.weight
            gets = _outputs_read(prod)
            fused = (d.spec.kind == "gemm" and not d.dual and d.pool is None and d.emit is None and w.dim() == 4 and d.pad_shortcut is None and
                     gets is not None and all(g is x or not real_users(g, inside) for g in gets.values()) and d.spec.symmetric and
                     K.gap_head_supported(_ceil64(w.shape[1]), w.shape[0], 1, 1, w.shape[2], d.mod.stride[0], d.mod.padding[0]) and
                     w.shape[2] == w.shape[3] and (mode == "fused" or K.gap_head_profitable(_ceil64(w.shape[1]), w.shape[0])))
        name = f"_int8_gap_{count}"
        count += 1
        if dry_run:
            module = _DryNode()
        else:
            module = GapHeadLayer(modules[prod.target], emit, want_out) if fused else GapLayer(emit, want_out)
        _, outs = _call_plan_module(gm, last, name, module, tuple(prod.args) if fused else (x,))
        for u in users:
            u.replace_input_with(last, outs[1] if u in takers else outs[0])
        def erase_tree(n):     # `n` and what hangs on it: by now the chain's reshapes and their batch-size reads only
            for u in list(n.users):
                erase_tree(u)
            if n in live:
                live.discard(n)
                graph.erase_node(n)
        live = set(graph.nodes)
        erase_tree(pool)
        if fused:
            erase_tree(prod)
            report.fp32_outputs -= 1
        report.gap_heads.append((name, "fused" if fused else "separate"))
    _settle(gm, count)


# ------------------------------------------------------------------ the squeeze path of a squeeze-excite block
# What _squeeze_pass decides for one node: graph names, widths, the two activations' names, whether the gate keeps (N, C, 1, 1), the two
# layers' module names and input quantisers (_ActSpec), which of them the main pass had planned, and the nodes the node replaces.
_SqueezeDecision = collections.namedtuple("_SqueezeDecision", "pool x c r r4 inner gate_fn rank4 layer1 layer2 q1 q2 planned chain")


def _squeeze_weights(mod, spec):
    """A squeeze layer's integer weight codes [K, C] (int16) and its weight scales [K] from its frozen spec (symmetric weights)."""
    w = mod.weight.detach()
    k = w.shape[0]
    ws = spec.w_scale.detach().to(torch.float32).reshape(-1)
    ws = (ws.expand(k) if ws.numel() == 1 else ws).contiguous()
    if spec.w_codes is not None:
        q = spec.w_codes()
    else:
        q = K.quantize_weight_krsc(w if w.dim() == 4 else w[:, :, None, None], ws, spec.w_lo, spec.w_hi)[0]
    return q.reshape(k, -1).to(torch.int16), ws


class SqueezeLayer(nn.Module):
    """The squeeze path of a squeeze-excite block - global average pool, (flatten), a quantised Linear / 1x1 convolution, none | ReLU |
    swish, a second such layer, (view), sigmoid | hard sigmoid - as two launches: K.global_avgpool hands layer 1 its activation codes
    (N, C), K.squeeze_gate (csrc/squeeze_i8.hip) takes them to the fp32 gate.  `decision`: the pass's record (_SqueezeDecision);
    `layers`: (module 1, its _LayerSpec, module 2, its _LayerSpec); `weights=False` (a dry run) quantises nothing.  The hidden width is
    zero-padded to a multiple of 4 here, once.  An input that at run time is no channels_last fp32 (N, C, H, W) device map of the planned
    width is converted and runs `restated`: the same values from the kernels that were there before.  Returns the gate, (N, C, 1, 1) or
    (N, C) as the graph had it."""

    def __init__(self, decision, layers, weights=True):
        super().__init__()
        d = decision
        self.c, self.r, self.r4, self.inner, self.gate_fn, self.rank4 = int(d.c), int(d.r), int(d.r4), d.inner, d.gate_fn, bool(d.rank4)
        mod1, spec1, mod2, spec2 = layers
        self.act1, self.act2 = spec1.act, spec2.act
        self.decision = d
        self._deq = {}
        if not weights:
            return
        (q1, ws1), (q2, ws2) = _squeeze_weights(mod1, spec1), _squeeze_weights(mod2, spec2)
        dev, c, r, r4 = q1.device, self.c, self.r, self.r4
        w1, w2 = torch.zeros((r4, c), dtype=torch.int16, device=dev), torch.zeros((c, r4), dtype=torch.int16, device=dev)
        w1[:r], w2[:, :r] = q1, q2

        def padded(v, fill):
            out = torch.full((r4,), fill, dtype=torch.float32, device=dev)
            out[:r] = v.detach().to(torch.float32).reshape(-1)
            return out
        for name, t in (("w1", w1.to(torch.int8)), ("wsum1", w1.sum(dim=1).to(torch.int32)), ("ws1", padded(ws1, 1.0)),
                        ("b1", None if mod1.bias is None else padded(mod1.bias, 0.0)), ("w2", w2.to(torch.int8)),
                        ("wsum2", w2.sum(dim=1).to(torch.int32)), ("ws2", ws2),
                        ("b2", None if mod2.bias is None else mod2.bias.detach().to(torch.float32).reshape(-1).clone())):
            self.register_buffer(name, None if t is None else t.contiguous(), persistent=False)

    def _in_scale(self, numel):
        """Layer 1's dequantising scale: QBase's is grad_scale(s, g) with g taken over the layer's input (as _PlanLayer._in_scale)."""
        if not self.act1.needs_g:
            return self.act1.scale
        s = self._deq.get(numel)
        if s is None:
            s = self._deq[numel] = ste_scale_value(self.act1.scale, self.act1.g(numel)).contiguous()
        return s

    def _operands(self, n):
        """K.squeeze_gate's arguments behind the codes for a batch of `n` images."""
        l1 = dict(wq=self.w1, wsum=self.wsum1, bias=self.b1, in_scale=self._in_scale(n * self.c), in_zp=self.act1.zp, w_scale=self.ws1)
        return l1, self.inner, self.act2.emit(n * self.r), dict(wq=self.w2, wsum=self.wsum2, bias=self.b2, w_scale=self.ws2), self.gate_fn

    def _run(self, x, fn):
        n = x.shape[0]
        codes = K.global_avgpool(x, emit=self.act1.emit(n * self.c), want_out=False)[1]
        gate = fn(codes, *self._operands(n))[0]
        return gate.view(n, self.c, 1, 1) if self.rank4 else gate

    def restated(self, x):
        """The node's value from the wrappers that were there before it (K.squeeze_gate_torch), for any (N, C, H, W) input."""
        if x.dim() != 4 or x.shape[1] != self.c:
            raise ValueError(f"SqueezeLayer: a (N, {self.c}, H, W) map, not {tuple(x.shape)}")
        return self._run(x.to(torch.float32).contiguous(memory_format=torch.channels_last), K.squeeze_gate_torch)

    def forward(self, x):
        # (NHWC rows: channels_last memory, or the channel slice a channel-padded plan layer returns as its fp32 output)
        if x.dim() != 4 or x.dtype != torch.float32 or not x.is_cuda or x.shape[1] != self.c or not (
                x.is_contiguous(memory_format=torch.channels_last) or K._nhwc_rows(x) is not None):
            return self.restated(x)
        return self._run(x, K.squeeze_gate)


def _squeeze_layer_shape_ok(mod):
    """A Linear, or an unpadded 1x1 / stride 1 convolution without groups or dilation."""
    w = mod.weight
    if w.dim() == 2:
        return True
    return (w.dim() == 4 and tuple(w.shape[2:]) == (1, 1) and tuple(mod.stride) == (1, 1) and tuple(mod.padding) == (0, 0) and
            mod.groups == 1 and tuple(mod.dilation) == (1, 1) and mod.padding_mode == "zeros")


def _squeeze_refusal(mod, spec, weight_blob, pack_int4):
    """Why a squeeze layer with frozen spec `spec` (None: it has none) stays as it is, or None."""
    if isinstance(mod, FSPTQBase) and mod.qconfig["weight"].get("recon_type") in ("adaround", "dist_recon"):
        return "AdaRound / dist_recon weights"
    if isinstance(mod, QBase) and float(mod.in_offset.abs().max()) != 0:
        return "a float activation offset"
    if spec is None:
        return "no frozen int8 quantisers (a disabled quantiser, a non-integer zero point or a range beyond a byte)"
    if not spec.symmetric:
        return "asymmetric weights"
    if spec.w_hi > 127 or spec.w_lo < -128:
        return "weights with an offset (codes beyond int8 are re-centred)"
    if weight_blob is not None:
        return "a plan built from an integer checkpoint (weight_blob)"
    if pack_int4 and -8 <= spec.w_lo and spec.w_hi <= 15:
        return "4-bit weights, which the plan stores packed (pack_int4)"
    return None


_DIV_FNS = (operator.truediv, torch.div, torch.true_divide)


def _squeeze_gate_fn(node, src, modules):
    """(name, nodes) if `node` starts the gate function of `src` in a spelling the plan takes - torch.sigmoid / F.sigmoid / .sigmoid() /
    nn.Sigmoid; nn.Hardsigmoid, F.hardsigmoid; `relu6(src + 3) / 6` spelled out, each node read by the next alone - else None."""
    if not isinstance(node, fx.Node):
        return None
    one = len(node.args) == 1 and node.args[0] is src
    if node.op == "call_module":
        m = modules.get(node.target)
        name = "sigmoid" if type(m) is nn.Sigmoid else ("hardsigmoid" if type(m) is nn.Hardsigmoid else None)
        return (name, [node]) if name and one and not node.kwargs else None
    if _is_call(node, _SIGMOID_FNS, "sigmoid") and one:
        return "sigmoid", [node]
    if node.op == "call_function" and node.target is F.hardsigmoid:
        return ("hardsigmoid", [node]) if one and set(node.kwargs) <= {"inplace"} else None
    num = lambda v, k: isinstance(v, (int, float)) and not isinstance(v, bool) and float(v) == k  # noqa: E731
    if not (_is_call(node, (operator.add, torch.add), "add") and len(node.args) == 2 and
            ((node.args[0] is src and num(node.args[1], 3.0)) or (node.args[1] is src and num(node.args[0], 3.0)))):
        return None
    r6 = _sole_user(node)
    if r6 is None or not _is_relu6(r6, modules) or r6.args[0] is not node:
        return None
    div = _sole_user(r6)
    if not (_is_call(div, _DIV_FNS, "div") and len(div.args) == 2 and div.args[0] is r6 and num(div.args[1], 6.0)):
        return None
    return "hardsigmoid", [node, r6, div]


def _squeeze_pass(gm, report, planned, dry_run, weight_blob, pack_int4):
    """Squeeze paths (fuse_inference(squeezes=True)): `pool(x) -> (flatten) -> layer -> none | ReLU | swish -> layer -> (view) -> sigmoid
    | hard sigmoid`, every node read by the next alone, becomes one SqueezeLayer node called with `x`.  A layer is a QBase / FSPTQ Linear
    or unpadded 1x1 / stride 1 convolution still in the graph (its frozen quantisers read with kind "gemm": this kernel pads nothing to
    64), or the plan node the main pass made of one (with the ReLU it absorbed and the codes it hands the second layer).  `planned`:
    plan node -> _Decision; absorbed plan nodes leave it and the report's counts, absorbed wrappers leave `report.skipped`.  A candidate
    the kernel or the pass does not take stays as it is, with the reason in `report.squeeze_left`."""
    absorbed = []

    def layer(node, modules):
        """(module, spec or None, ReLU absorbed, output node, [the nodes], _Decision or None) of a squeeze layer at `node`, else None."""
        d = planned.get(node)
        if d is not None:
            gets = _outputs_read(node)
            if (d.dual or d.residual is not None or d.pool is not None or d.relu6 or d.narrow or d.pad_shortcut is not None or
                    d.spec.kind != "gemm" or gets is None or len(gets) != 1 or not _squeeze_layer_shape_ok(d.mod)):
                return None
            (i, out), = gets.items()
            if (i == 1) != (d.emit is not None and not d.want_out):
                return None
            return d.mod, d.spec, d.relu, out, [node, out], d
        if not isinstance(node, fx.Node) or node.op != "call_module" or len(node.args) != 1 or node.kwargs:
            return None
        mod = modules.get(node.target)
        if not isinstance(mod, (QBase, FSPTQBase)) or not hasattr(mod, "weight") or not _squeeze_layer_shape_ok(mod):
            return None
        spec = _fsptq_spec(mod, "gemm") if isinstance(mod, FSPTQBase) else _qbase_spec(mod, "gemm", False)
        return mod, spec, False, node, [node], None

    def match(pool, modules):
        rank = _pool_dims(pool, modules)
        x = (pool.args[0] if pool.args else pool.kwargs.get("input")) if rank is not None else None
        if not isinstance(x, fx.Node):
            return None
        chain, cur = [pool], pool
        nxt = _sole_user(cur)
        if (nxt is not None and nxt.target in ("flatten", "view", "reshape", torch.flatten) and _flatten_rank(nxt, cur, rank) == 2):
            chain, cur, rank = chain + [nxt], nxt, 2
            nxt = _sole_user(cur)
        l1 = layer(nxt, modules)
        if l1 is None or (l1[0].weight.dim() == 2) != (rank == 2):
            return None
        mod1, spec1, relu1, cur, nodes1, d1 = l1
        chain += nodes1
        inner, users = ("relu" if relu1 else None), list(cur.users)
        if d1 is None or d1.emit is None:      # (else: the plan node hands the second layer its codes itself)
            mul = next((u for u in users if _is_mul(u)), None)
            sw = _swish_of(mul, modules) if len(users) == 2 and mul is not None else None
            if sw is not None and sw[0] is cur and len(sw[1]) == 2 and set(sw[1]) == set(users) and inner is None:
                inner, cur = "swish", mul
                chain += sw[1][::-1]
            elif len(users) == 1 and inner is None and _is_relu(users[0], modules) and users[0].args[0] is cur:
                inner, cur = "relu", users[0]
                chain.append(cur)
            elif len(users) != 1:
                return None
        nxt = _sole_user(cur)
        l2 = layer(nxt, modules)
        if l2 is None or l2[2] or (l2[5] is not None and l2[5].emit is not None) or l2[0].weight.dim() != mod1.weight.dim():
            return None
        mod2, spec2, _, cur, nodes2, d2 = l2
        chain += nodes2
        r, c = int(mod1.weight.shape[0]), int(mod1.weight.shape[1])
        if tuple(mod2.weight.shape[:2]) != (c, r):
            return None
        rank4 = rank == 4
        nxt = _sole_user(cur)
        if nxt is not None and not rank4 and nxt.op == "call_method" and nxt.target in ("view", "reshape") and not nxt.kwargs and nxt.args[0] is cur:
            shape = nxt.args[1:]
            shape = tuple(shape[0]) if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else shape
            if (len(shape) == 4 and _batch_size_of(shape[0]) and (shape[1] == c or _batch_size_of(shape[1], 1)) and shape[2] == 1 and shape[3] == 1):
                chain, cur, rank4 = chain + [nxt], nxt, True
                nxt = _sole_user(cur)
        fn = _squeeze_gate_fn(nxt, cur, modules)
        if fn is None:
            return None
        chain += fn[1]
        # ---- a candidate: taken unless a quantiser or a width refuses
        for mod, spec in ((mod1, spec1), (mod2, spec2)):
            why = _squeeze_refusal(mod, spec, weight_blob, pack_int4)
            if why is not None:
                return why
        if d1 is not None and d1.emit is not None and d1.emit.key != spec2.act.key:
            return "the first layer emits another quantiser's codes than the second layer reads"
        if not K.squeeze_gate_supported(c, r):
            return f"widths beyond the kernel's limits ({c} channels, {r} hidden units)"
        names = tuple(d.node.target if d is not None else n[0].target for d, n in ((d1, nodes1), (d2, nodes2)))
        dec = _SqueezeDecision(pool.name, x.name, c, r, (r + 3) // 4 * 4, inner, fn[0], rank4, names[0], names[1], spec1.act, spec2.act,
                               (d1 is not None, d2 is not None), tuple(n.name for n in chain))
        absorbed.extend([(nodes1[0], d1, names[0]), (nodes2[0], d2, names[1])])
        return _Splice(SqueezeLayer, dict(decision=dec, layers=(mod1, spec1, mod2, spec2), weights=not dry_run), chain[-1], (x,), (), chain[::-1])

    _run_node_pass(gm, report, "squeeze", "squeezes", match, dry_run, outputs=1, left=report.squeeze_left)
    for node, d, name in absorbed:
        if d is None:
            if name in report.skipped:
                report.skipped.remove(name)
            continue
        planned.pop(node, None)
        report.layers -= 1
        report.relu -= d.relu
        report.emit -= d.emit is not None
        report.fp32_outputs -= d.want_out


class StemLayer(_PlanLayer):
    """The network's first convolution (<= 4 input channels) of the frozen plan: the image is quantised into a
    zero-point-padded NHWC4 code buffer and convolved on the matrix cores (csrc/conv_stem_i8.hip)."""

    def __init__(self, layer, spec, **kw):
        super().__init__(layer, spec, **kw)
        if self._w_codes is None:
            wq, wsum = K.quantize_weight_stem(layer.weight, self.w_scale, self.w_lo, self.w_hi)
        else:     # the module's own integer codes (asymmetric / per-channel QBase weights) in the stem kernel's [K, R, 8 taps, 4] layout
            q = _weight_codes(self)                                                # [K, C, R, S] int16, re-centred
            k, c, r, s_ = q.shape
            full = torch.zeros((k, r, 8, 4), dtype=torch.int16, device=q.device)
            full[:, :, :s_, :c] = q.permute(0, 2, 3, 1)
            wq, wsum = full.to(torch.int8).contiguous(), q.sum(dim=(1, 2, 3)).to(torch.int32).contiguous()
        self.register_buffer("wq", wq, persistent=False)
        self.register_buffer("wsum", wsum, persistent=False)
        if self.act.xoff:
            _, _, r, s_ = layer.weight.shape
            tap = wq[:, :, :s_, :self.c].to(torch.float64).sum(dim=3) * self.w_scale.to(torch.float64)[:, None, None]   # [K, R, S]
            if self.w_off is not None:
                tap = tap + self.c * self.w_off.to(torch.float64)[:, None, None]
            self._fold_offset(tap)

    def forward(self, x):
        lay, act = self.layer, self.act
        numel = x.numel()
        pad, st = lay.padding[0], lay.stride[0]
        k, _, r, s = lay.weight.shape
        emit = self._emit_for(x.shape[0], k, (x.shape[2] + 2 * pad - r) // st + 1, (x.shape[3] + 2 * pad - s) // st + 1)
        in_kernel = self.pool == (3, 2, 1) and k <= 64 and self.w_off is None and not self.relu6 and not act.xoff   # conv + ReLU + MaxPool2d(3, 2, 1) + quantiser: one kernel
        # an unsigned image quantiser's codes go into the padded buffer re-centred (`code - 128`: what the matrix cores multiply),
        # so the first-layer kernels need not xor every operand fragment they read; the zero point moves with them
        shifted = act.lo >= 0
        # (a float offset pads with code 0 - its zero has no code - and the kernel takes the difference as its border term)
        xpad = K.quantize_pad_nhwc4(x, act.scale, act.zp, act.lo, act.hi, act.form, pad, g=act.g(numel), shift128=shifted, pad_code0=act.xoff)
        xkw = dict(self._xoff_kw(), pad=pad) if self.xoff_padded else {}
        res = K.conv2d_i8_stem(xpad, self.wq, self.wsum, self._bias() if act.xoff else lay.bias, self._in_scale(numel),
                               self.zp_shift if shifted else self._kzp, self.w_scale, s, stride=st, act=self._act_arg(), emit=emit,
                               want_out=self.want_out, pool=in_kernel, w_offset=self.w_off, channels=self.c, **xkw)
        out, out_codes = res if emit is not None else (res, None)
        return (out, out_codes) if in_kernel else self._finish(out, out_codes)


def _structure_only(self, layer, spec, **decided):
    nn.Module.__init__(self)
    self._structure(layer, spec, **decided)


# fuse_inference(dry_run="chains"): an Int8Layer's structure - what the chain-level passes decide on - without its weight codes
# (quantising them needs the GPU)
_DryInt8Layer = _dry(Int8Layer, _structure_only)


def _is_int8(m):
    """A plain Int8Layer plan node (no subclass with a kernel family of its own), or its dry-run stand-in."""
    return type(m) in (Int8Layer, _DryInt8Layer)


class FusionReport:
    """What the pass did, for logs and tests."""

    def __init__(self):
        self.layers = self.relu = self.residual = self.emit = self.fp32_outputs = self.stem = self.pooled = self.dual = 0
        self.relu6 = 0        # ReLU6 (nn.ReLU6, nn.Hardtanh(0, 6), F.relu6, F.hardtanh(x, 0, 6)) fused; `relu` counts ReLU alone
        self.chained = 0      # block end + next block's 1x1 pairs running as one kernel
        self.recomputed = 0   # projection-block fp32 outputs dropped, their reader recomputing them from the block's operands (_recompute_pass)
        self.chunk_major = 0  # fp32 block outputs kept chunk-major between two kernels that walk them chunk by chunk (_block_layout_pass)
        self.dwpw = 0         # depthwise 3x3 + pointwise 1x1 units running as one kernel
        self.act_offset = 0   # planned layers whose input quantiser has a float offset (fuse_inference(act_offsets=True))
        self.narrow = 0       # channel-padded layers reading / writing their fp32 tensors at the real width (fuse_inference(narrow_rows=True))
        self.pad_shortcuts = 0   # option-A shortcuts (subsample + zero-pad) read in place by the layer's epilogue (fuse_inference(pad_shortcuts=True))
        self.avg_pools = 0    # windowed average pools handing the plan layers behind them their codes (fuse_inference(avg_pools=True))
        self.gates = 0        # squeeze-excite gates (x * g, + ReLU / ReLU6) handing the plan layers behind them their codes (fuse_inference(gates=True))
        self.dw5 = 0          # 5x5 depthwise layers on the integer dot-product kernel, csrc/conv_dw5_i8.hip (fuse_inference(dw5=True))
        self.squeezes = 0     # squeeze paths (pool, two small layers, gate function) running as two launches (fuse_inference(squeezes=True))
        self.squeeze_left = []   # (pool node, why): squeeze paths the squeeze pass recognised and left as they are
        self.swishes = 0      # swish / SiLU activations of 4-D maps handing the plan layers behind them their codes (fuse_inference(swish=True))
        self.hardswishes = 0  # hard-swish activations of 4-D maps handing the plan layers behind them their codes (fuse_inference(hardswish=True))
        self.layer_norms = 0  # LayerNorms handing the Linear plan layers behind them their codes (fuse_inference(layer_norms=True))
        self.gelus = 0        # erf-form GELUs handing the plan layers behind them their codes (fuse_inference(gelu=True))
        self.attentions = 0   # attention cores running as one flash-forward launch, codes to the projection (fuse_inference(attention=True))
        self.patch_rows = 0   # patch rearrangements handing the embedding its codes from one read of the image (fuse_inference(patch_embed=True))
        self.token_assemblies = 0   # class-token concatenations + position embeddings running as one launch (fuse_inference(patch_embed=True))
        self.patch_embed_left = []  # (graph node, why): candidates of the patch-embedding pass that were left as they are
        self.gap_heads = []   # (plan node, "fused" | "separate"): global-average-pool heads handing the classifier its codes (gap_head=...)
        self.skipped = []

    def count(self, d):
        """One plan node of the main pass (its _Decision)."""
        self.layers += 1 + d.dual
        self.dual += d.dual
        self.stem += d.spec.kind == "stem"
        self.pooled += d.pool is not None
        self.relu += d.relu
        self.relu6 += d.relu6
        self.act_offset += d.spec.act.xoff + (d.dual and d.dual_spec.act.xoff)
        self.residual += d.residual is not None
        self.narrow += d.narrow
        self.dw5 += d.dw5
        self.pad_shortcuts += d.pad_shortcut is not None
        self.emit += d.emit is not None
        self.fp32_outputs += d.want_out

    def __repr__(self):
        return (f"FusionReport(int8 layers={self.layers}, relu fused={self.relu}, relu6 fused={self.relu6}, residual fused={self.residual}, "
                f"code-emitting={self.emit}, fp32 outputs kept={self.fp32_outputs}, stem layers={self.stem}, "
                f"pools on codes={self.pooled}, dual (conv + shortcut conv) kernels={self.dual}, chained pairs={self.chained} (fp32 outputs chunk-major: {self.chunk_major}), "
                f"depthwise + pointwise units={self.dwpw}, " + (f"gap heads={self.gap_heads}, " if self.gap_heads else "") +
                (f"recomputed shortcuts={self.recomputed}, " if self.recomputed else "") +
                (f"narrow fp32 rows={self.narrow}, " if self.narrow else "") +
                (f"pad shortcuts={self.pad_shortcuts}, " if self.pad_shortcuts else "") +
                (f"average pools on the plan={self.avg_pools}, " if self.avg_pools else "") +
                (f"gates on the plan={self.gates}, " if self.gates else "") +
                (f"squeezes on the plan={self.squeezes}, " if self.squeezes else "") +
                (f"swishes on the plan={self.swishes}, " if self.swishes else "") +
                (f"hard swishes on the plan={self.hardswishes}, " if self.hardswishes else "") +
                (f"layer norms on the plan={self.layer_norms}, " if self.layer_norms else "") +
                (f"gelus on the plan={self.gelus}, " if self.gelus else "") +
                (f"attentions on the plan={self.attentions}, " if self.attentions else "") +
                (f"patch rows on the plan={self.patch_rows}, " if self.patch_rows else "") +
                (f"token assemblies on the plan={self.token_assemblies}, " if self.token_assemblies else "") +
                (f"patch embedding left alone={self.patch_embed_left}, " if self.patch_embed_left else "") +
                (f"5x5 depthwise on the dot-product kernel={self.dw5}, " if self.dw5 else "") +
                f"not eligible={self.skipped})")


class _Tracer(fx.Tracer):
    def is_leaf_module(self, m, qualname):
        return isinstance(m, (QBase, FSPTQBase, RootQBase)) or super().is_leaf_module(m, qualname)


_ADD_FNS = (operator.add, operator.iadd, torch.add)
_RELU_FNS = (F.relu, torch.relu, torch.relu_, F.relu_)


def _is_add(node):
    if node.kwargs:
        return False
    if node.op == "call_function" and node.target in _ADD_FNS:
        return len(node.args) == 2 and all(isinstance(a, fx.Node) for a in node.args)
    if node.op == "call_method" and node.target in ("add", "add_"):
        return len(node.args) == 2 and all(isinstance(a, fx.Node) for a in node.args)
    return False


def _inplace_add(node):
    return (node.op == "call_method" and node.target == "add_") or (node.op == "call_function" and node.target is operator.iadd)


def _is_relu(node, modules):
    if node.op == "call_module":
        return type(modules.get(node.target)) is nn.ReLU
    if node.op == "call_function":
        return node.target in _RELU_FNS
    return node.op == "call_method" and node.target in ("relu", "relu_")


def _is_relu6(node, modules):
    """ReLU6 in the forms the plan fuses: nn.ReLU6, nn.Hardtanh(0, 6), F.relu6 (inplace or not), F.hardtanh(x, 0, 6).  Its own
    predicate - _is_relu is shared with EagerFused, whose kernels know ReLU alone."""
    if node.op == "call_module":
        m = modules.get(node.target)
        return isinstance(m, nn.Hardtanh) and type(m) in (nn.ReLU6, nn.Hardtanh) and m.min_val == 0.0 and m.max_val == 6.0
    if node.op != "call_function":
        return False
    if node.target is F.relu6:
        return len(node.args) == 1 and set(node.kwargs) <= {"inplace"}
    if node.target in (F.hardtanh, F.hardtanh_):
        names = ("min_val", "max_val", "inplace") if node.target is F.hardtanh else ("min_val", "max_val")
        if len(node.args) > 1 + len(names) or not set(node.kwargs) <= set(names):
            return False
        given = dict(zip(names, node.args[1:]), **node.kwargs)
        lo, hi = given.get("min_val", -1.0), given.get("max_val", 1.0)
        return (isinstance(lo, (int, float)) and isinstance(hi, (int, float)) and not isinstance(lo, bool) and not isinstance(hi, bool)
                and float(lo) == 0.0 and float(hi) == 6.0)
    return False


_PAD_FNS = tuple({F.pad, torch._C._nn.pad})
_PadShortcut = collections.namedtuple("_PadShortcut", "source stride lo hi nodes")


def _pad_shortcut(node):
    """`node` as an option-A shortcut (He et al. 2016, section 4.2: subsample, zero-pad the channels) - `F.pad(t, (0, 0, 0, 0, lo, hi))`,
    constant mode, value 0, of `t = x[:, :, ::s, ::s]` or of x itself - as _PadShortcut(x, s, lo, hi, the nodes to erase), each node the
    only reader of the one before; None for anything else."""
    if node.op != "call_function" or node.target not in _PAD_FNS or len(node.users) != 1:
        return None
    names = ("input", "pad", "mode", "value")
    if len(node.args) > len(names) or not set(node.kwargs) <= set(names[len(node.args):]):
        return None
    given = dict(zip(names, node.args), **node.kwargs)
    t, pad, mode, value = given.get("input"), given.get("pad"), given.get("mode", "constant"), given.get("value", None)
    if not isinstance(t, fx.Node) or not isinstance(pad, (tuple, list)) or len(pad) != 6 or mode != "constant":
        return None
    if not all(isinstance(v, int) and not isinstance(v, bool) for v in pad) or tuple(pad[:4]) != (0, 0, 0, 0) or pad[4] < 0 or pad[5] < 0:
        return None
    if not (value is None or (isinstance(value, (int, float)) and not isinstance(value, bool) and float(value) == 0.0)):
        return None
    # (`t[i]` with an integer i is a plan node's output, not a subscript of a tensor)
    if not (t.op == "call_function" and t.target is operator.getitem and len(t.args) == 2 and not isinstance(t.args[1], int)):
        return _PadShortcut(t, 1, int(pad[4]), int(pad[5]), [node])          # F.pad alone: stride 1
    if len(t.users) != 1 or t.kwargs or not isinstance(t.args[0], fx.Node) or not isinstance(t.args[1], tuple):
        return None
    idx = t.args[1]
    full = slice(None, None, None)
    if len(idx) != 4 or idx[0] != full or idx[1] != full or not all(isinstance(i, slice) for i in idx):
        return None
    s = idx[2].step
    if (idx[2].start, idx[2].stop, idx[3].start, idx[3].stop) != (None,) * 4 or not isinstance(s, int) or isinstance(s, bool) or s < 1 or idx[3].step != s:
        return None
    return _PadShortcut(t.args[0], s, int(pad[4]), int(pad[5]), [node, t])


def _pool_params(node, modules):
    """(kernel, stride, padding) if `node` is an nn.MaxPool2d the code-domain pool reproduces."""
    if node.op != "call_module" or type(modules.get(node.target)) is not nn.MaxPool2d:
        return None
    m = modules[node.target]
    one = lambda v: v[0] if isinstance(v, (tuple, list)) and len(set(v)) == 1 else (v if isinstance(v, int) else None)  # noqa: E731
    k, s, p, d = one(m.kernel_size), one(m.stride if m.stride is not None else m.kernel_size), one(m.padding), one(m.dilation)
    if None in (k, s, p, d) or d != 1 or m.ceil_mode or m.return_indices:
        return None
    return k, s, p


class PackedWeights4(nn.Module):
    """The plan's 4-bit weight codes as they are stored: two codes per byte (`dlmcq_pack_int4`: element 2i in the low nibble),
    every layer's codes in the plan's own layout (KRSC / RSC / first-layer), concatenated.  The int8 kernels read one byte per
    code, so each forward starts with ONE `dlmcq_unpack_int4` launch that expands the whole network's weights into a scratch
    buffer the plan nodes' `wq` tensors are views of (BASELINE configs[4]: "sub-byte pack/unpack" on the timed path; MobileOne-S1:
    2.4 MB packed, ~3 us per step).  `expand()` is idempotent: concurrent streams write identical bytes."""

    def __init__(self, nodes, signed):
        super().__init__()
        self.signed = bool(signed)
        sizes = [n.wq.numel() for n in nodes]
        offs, total = [], 0
        for sz in sizes:
            offs.append(total)
            total += (sz + 31) // 32 * 32                     # 16 packed bytes: the kernels want 16-byte-aligned weights
        dev = nodes[0].wq.device
        flat = torch.zeros(total, dtype=torch.int8, device=dev)
        for n, o, sz in zip(nodes, offs, sizes):
            flat[o:o + sz] = n.wq.reshape(-1)
        self.register_buffer("packed", K.pack_int4(flat), persistent=False)
        self.register_buffer("scratch", torch.empty(total, dtype=torch.int8, device=dev), persistent=False)
        self.n = total
        for n, o, sz in zip(nodes, offs, sizes):              # the nodes keep no copy of their own: `wq` becomes a view of the scratch
            n._buffers["wq"] = self.scratch[o:o + sz].view(n.wq.shape)
            n._packed4 = True
        self.expand()

    def expand(self):
        K.unpack_int4(self.packed, self.n, self.signed, out=self.scratch)


def _pack_plan_weights(gm):
    """Store every plan node's weight codes whose range fits 4 bits packed (see PackedWeights4).  Returns the holders."""
    groups = {True: [], False: []}
    for m in gm.modules():
        if isinstance(m, _PlanLayer) and hasattr(m, "wq") and m.wq.dtype == torch.int8 and -8 <= m.w_lo and m.w_hi <= 15:
            lo, hi = int(m.wq.min()), int(m.wq.max())          # (plan build time: one read per layer)
            if 0 <= lo and hi <= 15:
                groups[False].append(m)
            elif -8 <= lo and hi <= 7:
                groups[True].append(m)
    holders = [PackedWeights4(nodes, signed) for signed, nodes in groups.items() if nodes]
    for i, h in enumerate(holders):
        gm.add_module(f"_packed_weights_{i}", h)
    if holders:
        gm.register_forward_pre_hook(lambda mod, args: [h.expand() for h in holders] and None)
    return holders


class EagerFused:
    """The model's forward with its wrappers UNFROZEN - they observe, calibrate and re-quantise exactly as in `model(x)` - but with
    every `layer -> (+ shortcut) -> ReLU` chain whose layer takes its int8 route evaluated by ONE launch (the int8 kernel's
    fused epilogue) instead of the layer, torch's add and torch's ReLU: the same bits (the epilogue is the kernel the plan uses,
    tested against the separate ops), so the scales a calibrating forward derives are identical, at roughly half the HBM traffic.
    This is what makes the first, calibrating batch cheap (bench.py `first_batch`); the frozen plan (`fuse_inference`) is for
    the steady state.  torch.fx reads the dataflow once (wrappers are leaves); execution is an interpreter over that graph.

        fused = EagerFused(model)      # once
        y = fused(x)                   # == model(x), bit for bit, including what the observers see

    Limits (each keeps `y == model(x)` by NOT fusing): a shortcut that is not an fp32 tensor of the layer's exact output shape
    (broadcast adds, other dtypes) runs layer, add and ReLU one by one; an in-place add INTO the shortcut (`short += layer(x)`) is
    left to torch, because the fused launch would not mutate `short`.  Not preserved on fused chains: forward hooks registered on
    the wrapper, the add or the ReLU (`forward_fused` is called directly and the add / ReLU never run as modules)."""

    def __init__(self, model):
        try:
            graph = _Tracer().trace(model)
        except Exception as e:
            raise RuntimeError(f"EagerFused reads the model's dataflow with torch.fx and could not trace it ({type(e).__name__}: {e})") from e
        self.gm = fx.GraphModule(model, graph)
        modules = dict(self.gm.named_modules())
        for node in list(graph.nodes):      # folded BatchNorms / eval-mode Dropout are wires
            if node.op == "call_module" and isinstance(modules[node.target], (nn.Identity, nn.Dropout)) and len(node.args) == 1 and \
                    not (isinstance(modules[node.target], nn.Dropout) and model.training):
                node.replace_all_uses_with(node.args[0])
                graph.erase_node(node)
        self.gm.recompile()
        self.chains = {}      # layer node -> (add node or None, shortcut node or None, relu node or None)
        taken = set()         # an add belongs to the FIRST layer (in program order) that feeds it: the other operand is its shortcut
        for node in graph.nodes:
            if node.op != "call_module" or len(node.args) != 1 or node.kwargs or not hasattr(modules[node.target], "forward_fused"):
                continue
            add = short = relu = None
            users = list(node.users)
            if len(users) == 1 and _is_add(users[0]) and users[0].args[0] is not users[0].args[1]:
                if users[0] in taken:
                    continue
                if _inplace_add(users[0]) and users[0].args[0] is not node:
                    continue      # `short += layer(x)` mutates the shortcut tensor, which other readers may hold: left to torch
                add = users[0]
                taken.add(add)
                short = add.args[1] if add.args[0] is node else add.args[0]
                users = list(add.users)
            if len(users) == 1 and _is_relu(users[0], modules):
                relu = users[0]
            if add is not None or relu is not None:
                self.chains[node] = (add, short, relu)

    def __call__(self, *args):
        # Freshly calibrated layers decide their int8 route by a value on the device (an integer zero point?): the forward runs on the
        # assumption that they may and checks all of them with ONE host read at its end (54 synchronisations saved in ResNet-50's first batch);
        # a wrong guess - a tensor without a zero in front of an unsigned quantiser - re-arms what calibrated and runs again, unspeculated
        from ..quantization.scalar._wrapper import ZeroPointSpeculation
        with ZeroPointSpeculation() as sp:
            interp = _EagerInterp(self.gm, self.chains)
            out = interp.run(*args)
        self.speculation = {"layers": len(sp.pending), "held": True}
        if not sp.verify():
            sp.rearm()
            self.speculation["held"] = False
            interp = _EagerInterp(self.gm, self.chains)
            out = interp.run(*args)
        self.last_states = {n.target: ("fused" if st == "fused" else "plain") for n, st in interp.state.items()}   # (tests, reports)
        return out


class _EagerInterp(fx.Interpreter):
    def __init__(self, gm, chains):
        super().__init__(gm)
        self.chains = chains
        self.add_of = {c[0]: n for n, c in chains.items() if c[0] is not None}
        self.relu_of = {c[2]: n for n, c in chains.items() if c[2] is not None}
        self.state = {}       # layer node -> "fused" | "plain" | ("pending", layer, x)

    def _launch(self, node, layer, x, short):
        add, _, relu = self.chains[node]
        if add is not None and not self._fusable_shortcut(layer, x, short):
            self.state[node] = "plain"       # a broadcast / differently shaped / non-fp32 shortcut: the ops one by one
            return None
        # (observe_out: the launch also leaves the min / max partials of its output for the consumer's observer - the calibrating forward's
        #  extra read of every activation tensor is gone wherever the kernel that ran has the observing epilogue)
        y = layer.forward_fused(x, residual=short, relu=relu is not None, observe_out=True)
        self.state[node] = "plain" if y is None else "fused"
        return y

    @staticmethod
    def _fusable_shortcut(layer, x, short):
        """The fused epilogue adds an fp32 tensor of exactly the layer's output shape; anything else keeps `y == model(x)` by
        running layer, add and ReLU separately."""
        if not isinstance(short, torch.Tensor) or short.dtype != torch.float32 or short.device != x.device:
            return False
        w = layer.weight
        if w.dim() == 2:
            return tuple(short.shape) == (*x.shape[:-1], w.shape[0])
        if x.dim() != 4:
            return False
        def side(n, k, s, p, d):
            return (n + 2 * p - d * (k - 1) - 1) // s + 1
        p = layer.padding if not isinstance(layer.padding, str) else None
        if p is None:
            return False
        return tuple(short.shape) == (x.shape[0], w.shape[0], side(x.shape[2], w.shape[2], layer.stride[0], p[0], layer.dilation[0]),
                                      side(x.shape[3], w.shape[3], layer.stride[1], p[1], layer.dilation[1]))

    def run_node(self, n):
        if n in self.chains:
            add, short, _ = self.chains[n]
            layer = self.fetch_attr(n.target)
            (x,), _ = self.fetch_args_kwargs_from_env(n)
            if add is not None and short not in self.env:      # the shortcut is computed later in program order (a downsample branch): at the add
                self.state[n] = ("pending", layer, x)
                return None
            y = self._launch(n, layer, x, self.env[short] if add is not None else None)
            return layer(x) if y is None else y
        if n in self.add_of:
            c = self.add_of[n]
            st = self.state.get(c)
            if st == "fused":
                return self.env[c]
            if isinstance(st, tuple):
                _, layer, x = st
                short = self.env[self.chains[c][1]]
                y = self._launch(c, layer, x, short)
                if y is not None:
                    return y
                self.env[c] = layer(x)           # not on the int8 route after all: the ops one by one
        elif n in self.relu_of:
            if self.state.get(self.relu_of[n]) == "fused":
                (v,), _ = self.fetch_args_kwargs_from_env(n)
                return v
        return super().run_node(n)


def _codes_from_blob(mod_name, blob, layer):
    """A layer's integer weight codes [K, C, R, S] (int16, on the layer's device) from an integer checkpoint of
    dlmc.utils.export (packed int4 or int8), expanded ON THE DEVICE - the plan never sees fp32 weights for that layer."""
    rec = blob["layers"].get(mod_name)
    if rec is None:
        return None
    dev = layer.weight.device
    n = int(torch.tensor(rec["shape"]).prod())
    if rec["packed_int4"]:
        q = K.unpack_int4(rec["codes"].to(dev), n, rec["lo"] < 0)
    else:
        q = rec["codes"].to(dev)
    return q.reshape(rec["shape"]).to(torch.int16)


class _Decision:
    """What the main pass decided for one plan node: the wrapper `node` calls (`mod`, its `spec`) and what it absorbs."""

    def __init__(self, node, mod, spec):
        self.node, self.mod, self.spec = node, mod, spec
        self.chain = [node]                    # the graph nodes the plan node replaces: the wrapper's, (the add), (the ReLU / ReLU6), (the max-pool)
        self.residual = None                   # the other addend of the folded add
        self.relu = self.relu6 = False
        self.pool = None                       # (kernel, stride, padding) of the max-pool behind it
        self.pad_shortcut = None               # `residual` is an option-A shortcut (_PadShortcut), read in place at its source
        self.emit, self.takers = None, ()      # the quantiser (_ActSpec) of the readers that take codes, and those readers
        self.want_out, self.narrow = True, False       # someone reads the fp32 output; fp32 rows at the real width
        self.dw5 = False                       # a depthwise 5x5 / padding 2 layer on csrc/conv_dw5_i8.hip's kernel (fuse_inference(dw5=True))
        self.dual_mod = self.dual_spec = None  # the convolution on the shortcut, run by the same (dual) kernel, and its spec
        self.dual_inputs = None                # a dual node's activation quantisers: of its input 0, of its input 1

    @property
    def dual(self):
        return self.dual_inputs is not None

    @property
    def last(self):
        """The graph node whose readers become the plan node's."""
        return self.chain[-1]

    def args(self):
        """The plan node's inputs: the activation(s), or the activation and the fp32 shortcut (a pad shortcut: its source)."""
        if self.residual is None:
            return (self.node.args[0],)
        if self.dual:
            return self.node.args[0], self.residual.args[0]
        return self.node.args[0], (self.residual if self.pad_shortcut is None else self.pad_shortcut.source)

    def options(self):
        """The decision as _PlanLayer._structure takes it."""
        return dict(relu=self.relu, relu6=self.relu6, emit=self.emit, want_out=self.want_out, pool=self.pool, narrow=self.narrow, dw5=self.dw5,
                    pad_shortcut=None if self.pad_shortcut is None else (self.pad_shortcut.stride, self.pad_shortcut.lo))


class _MainPass:
    """fuse_inference's main pass: every eligible wrapper becomes a plan node `(fp32 or None, codes or None)` that has absorbed the add,
    the activation and the max-pool behind it.  Per wrapper, in graph order: decide (reads the graph and the specs, changes nothing),
    build (the module, by mode), splice (the graph), FusionReport.count.  A new flag is a field of _Decision set in `decide`, handed to
    the node by `_Decision.options` / `_PlanLayer._structure` and counted in `FusionReport.count`."""

    def __init__(self, gm, dry_run, weight_blob, dwpw, relu6, act_offsets, narrow_rows, pad_shortcuts, dw5=False):
        self.dw5 = dw5
        self.gm, self.graph, self.modules = gm, gm.graph, dict(gm.named_modules())
        self.dry_run, self.weight_blob, self.dwpw = dry_run, weight_blob, dwpw
        self.relu6, self.act_offsets, self.narrow_rows, self.pad_shortcuts = relu6, act_offsets, narrow_rows, pad_shortcuts
        self.specs, self.skipped = {}, []      # wrapper -> its _LayerSpec or None, made when first asked for; those without, in that order
        self.planned = {}                      # plan node -> its _Decision (the average-pool and head passes read it)

    def run(self, report):
        live = set(self.graph.nodes)
        for node in list(self.graph.nodes):
            d = self.decide(node) if node in live else None       # (not live: absorbed into an earlier node)
            if d is not None:
                live.difference_update(self.splice(d, self.build(d)))
                report.count(d)
        report.skipped += self.skipped
        _settle(self.gm)
        return self.planned

    def spec_of(self, node):
        if node.op != "call_module" or len(node.args) != 1 or node.kwargs:
            return None
        if node.target not in self.specs:
            mod = self.modules.get(node.target)      # (a plan node's module is not in here: no spec)
            self.specs[node.target] = _frozen_spec(mod, self.act_offsets) if isinstance(mod, (QBase, FSPTQBase)) else None
            if self.specs[node.target] is None and isinstance(mod, (QBase, FSPTQBase, RootQBase)):
                self.skipped.append(node.target)
        return self.specs[node.target]

    def accepts(self, u, t):
        """The activation quantiser `u` applies to tensor `t`, if `u` can take `t` as codes instead."""
        d = self.planned.get(u)
        if d is not None and d.dual:
            acts = {d.dual_inputs[i].key: d.dual_inputs[i] for i in (0, 1) if u.args[i] is t}
            return next(iter(acts.values())) if len(acts) == 1 else None
        s = self.spec_of(u) if u.args and u.args[0] is t else None
        return s.act if s is not None and s.kind in ("gemm", "dw") else None

    def source_channels(self, src):
        """Channels of `src` if its fp32 value is known to be dense channels_last at its real width - the fp32 output of a plan node
        that is unpadded or narrow, or the network input as a planned convolution reads it - else None."""
        if src.op == "call_function" and src.target is operator.getitem and src.args[1] == 0 and src.args[0] in self.planned:
            d = self.planned[src.args[0]]
            w = d.mod.weight
            ok = w.dim() == 4 and d.spec.kind in ("gemm", "dw") and d.pool is None and (w.shape[0] % 64 == 0 or d.narrow)
            return int(w.shape[0]) if ok else None
        # the network input: its width is read off a planned (ungrouped) convolution that takes it as its activation; with no such
        # reader yet (or only readers planned later) the answer is None and nothing folds.  Dense only once it is channels_last: an
        # NCHW-contiguous input is converted per call by Int8Layer.forward (one copy of the input, in place of the slice and the pad)
        if src.op == "placeholder":
            for u in src.users:
                d = self.planned.get(u)
                if d is not None and u.args[0] is src and d.mod.weight.dim() == 4 and d.mod.groups == 1:
                    return int(d.mod.weight.shape[1])
        return None

    # ---- decide: add, then ReLU / ReLU6, then max-pool, then pad shortcut, then readers, then dual, then narrow (later ones read earlier ones)
    def decide(self, node):
        """The _Decision for the wrapper `node` calls, or None if it has no spec."""
        spec = self.spec_of(node)
        if spec is None:
            return None
        mod, modules = self.modules[node.target], self.modules
        d = _Decision(node, mod, spec)
        # the chain  layer -> (+ shortcut) -> ReLU, each link the sole user of the previous one.  (The stem kernel has no shortcut input;
        # a layer whose output channels are zero-padded to a multiple of 64 - MobileNetV2's 24 / 96 / 160-channel projections, CIFAR
        # ResNets' 16 / 32 - computes a k_pad-wide tile: the k-wide fp32 shortcut does not fit it, so the add stays outside the kernel)
        wn = mod.weight
        unpadded = wn.dim() != 4 or wn.shape[0] % 64 == 0
        # ... unless the layer runs with narrow fp32 rows (narrow_rows): a padded "gemm" convolution of k % 4 == 0 channels without the
        # border term of a float activation offset (the *_xoff kernels have no narrow form)
        can_narrow = (self.narrow_rows and spec.kind == "gemm" and not unpadded and wn.shape[0] % 4 == 0 and not _border_term(spec.act, mod))
        add = _sole_user(node)
        if spec.kind == "gemm" and (unpadded or can_narrow) and add is not None and _is_add(add) and add.args[0] is not add.args[1]:
            d.residual = add.args[1] if add.args[0] is node else add.args[0]
            d.chain.append(add)
        act = _sole_user(d.last)
        if act is not None and (_is_relu(act, modules) or (self.relu6 and _is_relu6(act, modules))):
            d.relu = _is_relu(act, modules)
            d.relu6 = not d.relu
            d.chain.append(act)
        self._decide_pool(d)
        self._decide_pad_shortcut(d)
        self._decide_readers(d)
        self._decide_dual(d, unpadded)
        # every narrow-capable layer that writes fp32 (or reads a shortcut) does so at the real width
        d.narrow = bool(can_narrow and (d.want_out or d.residual is not None))
        d.dw5 = bool(self.dw5 and _takes_dw5(spec, mod))
        return d

    def _decide_pool(self, d):
        """A max-pool read only by int8 layers of one quantiser runs on the codes (monotone quantiser)."""
        mp = _sole_user(d.last)
        params = _pool_params(mp, self.modules) if mp is not None else None
        if params is None or d.mod.weight.shape[0] % 4 != 0:
            return
        cons = [self.accepts(u, mp) for u in mp.users]
        on_codes = cons and all(c is not None for c in cons) and len({c.key for c in cons}) == 1
        # the first-layer kernel pools in fp32 itself (any consumers); elsewhere the pool runs on the emitted codes
        # (the pooling first-layer kernel has no weight-offset term, and ReLU alone)
        in_stem = (d.spec.kind == "stem" and params == (3, 2, 1) and d.mod.weight.shape[0] <= 64 and d.spec.symmetric and not d.relu6 and
                   not d.spec.act.xoff)
        if on_codes or in_stem:
            d.pool = params
            d.chain.append(mp)

    def _decide_pad_shortcut(self, d):
        """An option-A shortcut (pad_shortcuts): the epilogue reads its source in place.  (Not for a layer with the border term of a
        float activation offset: it runs on the *_xoff kernels, which have no narrow form - the exclusion `can_narrow` and the dual
        decision carry; its add keeps folding with the materialised tensor.)"""
        res = d.residual
        if not self.pad_shortcuts or res is None or res.op != "call_function" or _border_term(d.spec.act, d.mod):
            return
        m = _pad_shortcut(res)
        cs = self.source_channels(m.source) if m is not None else None
        if cs is not None and m.lo % 4 == 0 and cs % 4 == 0 and cs >= 4 and m.lo + cs + m.hi == d.mod.weight.shape[0]:
            d.pad_shortcut = m

    def _decide_readers(self, d):
        """Who reads the result: int8 layers fed ONLY through their activation argument take codes (the most common quantiser's)."""
        consumers, fp32_needed = {}, not d.last.users
        for u in d.last.users:
            a = self.accepts(u, d.last)
            if a is None:
                fp32_needed = True
            else:
                consumers.setdefault(a.key, []).append((u, a))
        if consumers:
            key = max(consumers, key=lambda k: len(consumers[k]))
            d.takers = [u for u, _ in consumers[key]]
            d.emit = consumers[key][0][1]
            fp32_needed = fp32_needed or len(consumers) > 1
        d.want_out = bool(fp32_needed or d.emit is None)

    def _decide_dual(self, d, unpadded):
        """The shortcut is itself a not-yet-planned int8 convolution read by nobody else: one dual kernel (ReLU alone, symmetric weights,
        no border term).  (A narrow layer is never a dual operand: the convolution on its shortcut runs as its own node.)"""
        res = d.residual
        other = self.spec_of(res) if res is not None and res.op == "call_module" else None
        omod = self.modules[res.target] if other is not None else None
        if (other is not None and unpadded and other.kind == "gemm" and list(res.users) == [d.chain[1]] and d.spec.symmetric and other.symmetric and
                d.mod.weight.dim() == 4 and omod.weight.dim() == 4 and not d.relu6 and
                not _border_term(d.spec.act, d.mod) and not _border_term(other.act, omod)):
            d.dual_mod, d.dual_spec, d.dual_inputs = omod, other, (d.spec.act, other.act)

    # ---- build
    def build(self, d):
        """The module of the plan node: the plan layer (real), a structural stand-in of an Int8Layer (`dry_run="chains"`) or a placeholder."""
        cls = {"gemm": Int8Layer, "dw": DwInt8Layer}.get(d.spec.kind, StemLayer)
        if self.dry_run == "chains" and cls is Int8Layer:    # ... a structural stand-in the chain-level passes can read
            plan = _DryInt8Layer(d.mod, d.spec, **d.options())
            return DualInt8Layer(plan, _DryInt8Layer(d.dual_mod, d.dual_spec)) if d.dual else plan
        if self.dry_run:      # decisions only (CPU-side tests): the node is a placeholder, nothing is quantised or launched
            return _DryNode()
        # codes of an unsigned-byte quantiser read only by matrix-core layers (no channel padding, no pooling on the way)
        # travel re-centred (see _PlanLayer.__init__); the consumers recognise them by dtype
        shift = (cls is Int8Layer and d.pool is None and (d.mod.weight.dim() != 4 or d.mod.weight.shape[0] % 64 == 0) and
                 _emits_shifted(d.emit, [(self.spec_of(u), self.modules.get(u.target)) for u in d.takers], self.dwpw))
        plan = cls(d.mod, self._from_blob(d.node.target, d.spec), emit_shift=shift, **d.options())
        return DualInt8Layer(plan, Int8Layer(d.dual_mod, self._from_blob(d.residual.target, d.dual_spec))) if d.dual else plan

    def _from_blob(self, name, spec):
        """`spec`, the layer's weight codes coming from the integer checkpoint (expanded on the device) where it holds them."""
        blob = self.weight_blob
        if blob is None or name not in blob["layers"]:
            return spec
        return spec.with_codes(lambda: _codes_from_blob(name, blob, self.modules[name]))

    # ---- splice
    def splice(self, d, module):
        """Put the plan node behind the last node it absorbs, hand its readers the codes or the fp32 output, erase what it replaces.
        Returns the erased nodes the pass has not visited yet and must not plan."""
        fused, outs = _call_plan_module(self.gm, d.last, f"_int8_plan_{len(self.planned)}", module, d.args())
        self.planned[fused] = d
        for u in list(d.last.users):
            if u not in outs.values():
                u.replace_input_with(d.last, outs[1] if u in d.takers else outs[0])
        for n in reversed(d.chain):
            self.graph.erase_node(n)
        if d.dual:
            self.specs[d.residual.target] = None   # never planned on its own
        # the convolution on the shortcut; the pad, then the slice: their only readers are gone
        gone = ([d.residual] if d.dual else []) + (d.pad_shortcut.nodes if d.pad_shortcut is not None else [])
        for n in gone:
            self.graph.erase_node(n)
        return gone


def fuse_inference(model, report=None, dry_run=False, chain_pairs=True, pack_int4=True, weight_blob=None, dwpw=False, block_layout=True,
                   relu6=True, act_offsets=False, gap_head=False, narrow_rows=False, pad_shortcuts=False, avg_pools=False,
                   recompute_shortcuts=None, gates=False, swish=False, dw5=False, layer_norms=False, gelu=False, attention=False,
                   patch_embed=False, squeezes=False, hardswish=False):
    """Return a `torch.fx.GraphModule` executing `model`'s calibrated quantised forward as the fused int8 plan.
    `pack_int4`: weight codes whose range fits 4 bits are stored packed and expanded by one launch per forward (PackedWeights4).
    `weight_blob`: an integer checkpoint (`dlmc.utils.export.export_quantized_state`) of the same model - the plan takes the
    layers' weight codes from it (expanded on the device) instead of quantising the fp32 weights again.
    Layers that are not eligible (grouped / 3-channel convs, non-integer zero points, RootQ, ...) keep running
    their own wrapper.  `model` must be on the GPU, in eval mode, already calibrated.  `dry_run=True` only takes the
    fusion decisions (graph + `fusion_report`, placeholder nodes): it needs no GPU and the result cannot be run.  `dry_run="chains"`
    also takes the chain-level decisions (chain pairs, block layout, recomputed shortcuts) on structural stand-ins of the plan layers.
    `recompute_shortcuts`: a stage's first block hands on its fp32 output unstored (K.DeferredBlock) where the next chain
    alone reads it, and that chain recomputes it from the block's two code operands (_recompute_pass; RECOMPUTE_ENABLED shapes: ResNet-50's stage 1).
    Bit-identical.  None: the environment's DLMCQ_RECOMPUTE_SHORTCUTS (0 / 1), on when unset; False: the plan as it was.
    `chain_pairs=False` keeps every block end and the 1x1 convolution behind it as two launches (A/B and tests).
    `dwpw=True` runs every depthwise 3x3 / stride 1 + pointwise 1x1 unit (MobileOne, MobileNet) as ONE launch
    (csrc/conv_dwpw_i8.hip: the code tensor between the two layers stays in LDS; bit-identical).  Off by default: at MobileOne-S1
    W4A8, batch 1024, the unit takes 270 us either way at 28^2 and 14^2 (148 + 123 and 108 + 114 us as two launches) - both halves
    are bound by their vector arithmetic (~24 instructions per depthwise element), which fusing does not remove.
    `block_layout=False` keeps every fp32 block tensor row-major (channels_last) instead of chunk-major between two chain kernels
    (_block_layout_pass; A/B and tests).
    `relu6=False` keeps every ReLU6 (nn.ReLU6, nn.Hardtanh(0, 6), F.relu6, F.hardtanh(x, 0, 6)) a separate op after an fp32 output
    instead of fusing it into the layer's epilogue (DLMCQ_ACT_RELU6) - the plan before ReLU6 fusion, for A/B runs and tests.  The
    dual, chain and depthwise + pointwise kernels know ReLU alone: a layer ending in ReLU6 runs on its own kernel.
    `act_offsets=True` also plans QBase layers whose activation quantiser has a per-tensor FLOAT offset (x^ = q * s^ + o: the
    unsigned min/max quantiser of any tensor that can go negative - shortcut sums, normalised images): producers emit their codes
    with that offset, the offset times the weight sums goes into the bias, and padded layers run the border term of the *_xoff
    entry points.  Off by default: the plan without it is the plan as it was.
    `gap_head`: the tail `global average pool -> flatten -> quantised Linear` on the plan.  The pool
    (nn.AdaptiveAvgPool2d(1), F.adaptive_avg_pool2d(x, 1), x.mean((2, 3)) / torch.mean, keepdim either way) and the reshape behind it
    (flatten(1), view / reshape(x.size(0), -1), squeeze) become one node that hands a plan-eligible Linear its activation codes [N, C].
    True: where the pool's producer is a 1x1 / stride 1 plan convolution (+ shortcut, ReLU / ReLU6) read by nothing else, the kernel
    is built for it (K.gap_head_supported) AND it was not measured slower there (K.gap_head_profitable), the two run as ONE kernel that
    never writes the fp32 map (csrc/conv_gap_i8.hip); else the pool kernel (csrc/gap.hip) follows the producer's ordinary launch.  On
    the last layers of ResNet-50, MobileNetV2 and MobileOne-S1 the fused head is slower than those two launches at batch 512 / 1024
    (DESIGN.md 5.14), so True runs them as two.  "separate": always the pool kernel; "fused": the fused head wherever it is built,
    profitable or not (both: A/B and tests).  All settings agree bit for bit.  The pooled sum is sequential fp32 in pixel order - not
    torch.mean's order - so against the plan WITHOUT heads a pooled value can differ in its last bit, which now and then flips a
    pooled activation code by one; the classifier amplifies such a flip (ResNet-50 b512: logits differ by up to 1.6 where they reach 3.7e3).
    A pool whose reader is not plan-eligible (RootQ, a disabled quantiser, a non-integer zero point, in-features % 64 != 0), any other
    output size, and F.avg_pool2d(x, x.size(3)) (a kernel size read from the tensor) are left as they are.  One spelling is folded
    although it differs from the model at batch 1: a bare x.squeeze() gives [C] there, the plan's node [1, C].  Off by default: the
    plan without it is the plan as it was.
    `narrow_rows=True`: a convolution whose output channels are zero-padded to a multiple of 64 (MobileNetV2's 24 / 32 /
    96 / 160-channel projections, CIFAR ResNets' 16 / 32) and a multiple of 4 reads and writes its fp32 tensors at the REAL width while
    its codes stay padded (dlmcq_conv2d_i8_nhwc_narrow; the tiled kernel, 64-wide tiles).  The shortcut add behind such a layer is then
    folded into its epilogue like any other (with the ReLU / ReLU6, pool and emit rules behind it), its fp32 output is dense - the next
    block reads it as its shortcut without a copy - and every such layer that writes fp32 at all writes it that way
    (`fusion_report.narrow` counts them).  Such a layer is never half of a dual kernel: a convolution on its shortcut runs as its own
    node; the chain, block-layout and fused-head passes keep requiring unpadded channels.  A padded layer with the border term of a
    float activation offset (the *_xoff kernels have no narrow form) or with k % 4 != 0 keeps its add outside.  Bit-identical to the
    plan without it (IEEE addition commutes; the codes are those of the stored value either way).  Off by default: the plan without it
    is the plan as it was.
    `pad_shortcuts=True`: where a foldable add's shortcut is the parameter-free "option A" one of the CIFAR ResNets -
    `F.pad(x[:, :, ::s, ::s], (0, 0, 0, 0, lo, hi))`, constant mode, value 0 (or F.pad alone: s = 1), each node read by the next alone -
    the layer's epilogue reads x itself at the pixel stride and the channel offset and adds +0 elsewhere (K.PadShortcut,
    dlmcq_conv2d_i8_nhwc_padres); the slice and the pad leave the graph (`fusion_report.pad_shortcuts` counts them).  Taken for a "gemm"
    convolution whose add folds anyway (unpadded, or narrow under `narrow_rows`), with lo % 4 == 0, x's channels % 4 == 0, lo + channels
    + hi == the layer's channels, and x known to be dense channels_last at its real width: the fp32 output of a plan node that is
    unpadded or narrow, or the network input (>= 4 channels; read in place when it is channels_last, else copied to channels_last
    once per call).  Not for a layer with the border term of a float activation offset (`act_offsets`: the *_xoff kernels have no
    narrow form).  Such a node always runs the tiled kernel's narrow epilogue and is never
    half of a chain, chunk-major or a fused head.  Anything else keeps today's graph.  Bit-identical to the plan without it.  Off by
    default: the plan without it is the plan as it was.
    `avg_pools=True`: a windowed average pool in front of plan convolutions - the shortcut of a ResNet-C / -D block
    (`workloads.CifarResNet(3, option="C")`), a DenseNet transition, an "anti-aliased" downsample - becomes a plan node (AvgPoolLayer,
    csrc/avgpool.hip) that hands those convolutions their activation codes; the pooled fp32 tensor and the consumer's quantise pass
    leave the step (`fusion_report.avg_pools` counts the nodes).  Taken: nn.AvgPool2d / F.avg_pool2d in any argument spelling with the
    kernel a Python int or an equal pair in 2 .. 8, stride None or equal to the kernel, padding 0, ceil_mode False, divisor_override
    None, read by at least one "gemm" plan convolution through its activation argument (as its own node or as either operand of a dual
    node) whose input channels are a multiple of 4, all such readers sharing one activation quantiser (the max-pool rule).  The codes
    are as wide as the readers take them (padded to 64 with their zero point, or code 0 under a float activation offset), shifted
    where every reader takes shifted codes, a QBase reader's g taken over the pooled tensor; other readers of the pool get the pooled
    fp32 tensor from the same launch.  Whatever the main pass decided for the convolution behind the pool - dual operand, own node,
    narrow, chain - stays; only its input changes.  Left as they are: a pool with no plan-eligible reader or with readers of different
    quantisers, a kernel size read from the tensor (F.avg_pool2d(x, x.size(3))), ceil_mode=True, any padding, stride != kernel,
    divisor_override, pools in front of depthwise or first-layer kernels.  The kernel sums each window sequentially from +0 in
    row-major order and divides once - torch's own loop - so the plan is bit-identical to the plan without the flag
    (tests/test_gpu_avgpool.py: torch.equal against F.avg_pool2d on the device and between the two plans' logits).  Measured (tools/avgpool_shortcut_ab.py,
    profiles/avgpool_shortcut_ab.json; ResNet-20 / -56, options C / D, FSPTQ and QBase, batch 512 at 32^2, interleaved): flag off / flag on =
    0.976 ... 1.103 in ms per step, no case slower beyond the run-to-run spread.
    Off by default: the plan without it is the plan as it was.
    `gates=True`: a squeeze-excite channel gate `x * gate(squeeze(x))` in front of plan convolutions - EfficientNet's
    MBConv, GhostNet, MobileNetV3, RepVGG-SE (`workloads.mobilenet_v2(se=True)`) - becomes a plan node (GateLayer, csrc/gate.hip) that
    multiplies the fp32 map by its (N, C, 1, 1) gate, applies the ReLU / ReLU6 behind the multiply and hands those convolutions their
    activation codes in one pass; the gated fp32 tensor, the activation and the consumer's quantise pass leave the step
    (`fusion_report.gates` counts the nodes).  The squeeze path - pool, two small layers, gate function - stays as it is.  Taken:
    `a * b`, torch.mul(a, b), a.mul(b) of two graph values where exactly one operand derives, through first arguments only (either
    operand of a multiply on the way; at most 16 nodes back), from a global average pool in a spelling the head pass knows
    (nn.AdaptiveAvgPool2d(1), F.adaptive_avg_pool2d(x, 1), x.mean((2, 3))) and that pool reads the other operand; a ReLU, or a ReLU6
    under `relu6`, that is the multiply's only reader is absorbed; the readers follow the average-pool rule ("gemm" plan convolutions
    through their activation argument, input channels a multiple of 4, one quantiser and one channel count; padded, shifted and
    g-scaled as there; other readers get the fp32 map from the same launch).  Left as they are: a gate that does not derive from a pool
    of x, F.avg_pool2d(x, x.size(3)), spatial gates, in-place mul_, readers of different quantisers, depthwise or first-layer readers.
    A gate that at run time is not (N, C, 1, 1) is multiplied, activated and quantised by torch and K.fake_quant inside the node - the
    unfused graph's values.  One IEEE multiply rounded to fp32, then the device's own ReLU (clamp_min: NaN passes, -0 becomes +0): the
    plan is bit-identical to the plan without the flag (tests/test_gpu_gate.py: fp32 bits and codes against torch on the device,
    torch.equal between the two plans' logits).  Measured (tools/gate_ab.py, profiles/gate_ab.json; MobileNetV2-SE, 17 gates, batch 1024
    at 224^2, interleaved): flag off / flag on = 40.23 / 32.58 ms per step (FSPTQ W8A8) and 40.51 / 32.87 (QBase W8A8), ratio 1.23 at
    a run-to-run spread of 0.19 ms; the gate kernel moves 4.4 TB/s over its 17 launches (the average-pool kernel's launch-bound nodes:
    0.9 - 2.6 TB/s).  No case slower.  Off by default: the plan without it is the plan as it was.
    `swish=True`: swish / SiLU `x * sigmoid(x)` of a 4-D map - EfficientNet's MBConv activation
    (`workloads.mobilenet_v2(se=True, act="swish")`) - becomes a plan node (SwishLayer, csrc/swish.hip) that hands the plan convolutions
    behind it, depthwise ones included, their activation codes in one pass and every other reader (a squeeze-excite pool, the gate node, a
    shortcut add) the activated fp32 map from the same launch (`fusion_report.swishes` counts the nodes).  Taken: `x * torch.sigmoid(x)`
    with either operand first, x.sigmoid(), torch.mul / x.mul, the sigmoid read by that multiply alone; nn.SiLU; F.silu, not in place; a
    user module whose body is one of these.  The readers follow the average-pool rule, plus depthwise plan convolutions; a swish nobody
    takes as codes is a node too where its input is known to be a map.  Left as they are: the swish on the (N, mid) vector inside a
    squeeze path, F.silu(inplace=True), a sigmoid with a second reader.  An input that at run time is no 4-D fp32 map of the planned width
    takes the node's torch path.  e = expf(-x), d = 1 + e, s = 1 / d, v = x * s, each rounded to fp32: within 3 * 2^-23 relative of the
    real value and, as measured, bit-identical to x * torch.sigmoid(x) on the device (F.silu differs in the last bit of a quarter of the
    elements) - the plan of a network that spells the multiply is bit-identical to the plan without the flag (tests/test_swish_gpu.py).
    The pass runs before the gate pass, which finds its gates behind the swish nodes.  Measured (tools/swish_ab.py,
    profiles/swish_ab.json; the MBConv-SE network, 35 swishes, batch 1024 at 224^2, gates=True in both, interleaved): flag off / flag on
    = 67.53 / 41.80 ms per step (FSPTQ W8A8), 67.58 / 41.97 (QBase W8A8), ratio 1.61 at a spread of 0.14 / 0.24 ms.  Off by default: the
    plan without it is the plan as it was.
    `dw5=True`: a depthwise 5x5 layer with padding 2 and stride 1 or 2 - 9 of the 16 depthwise layers of EfficientNet-B0,
    MobileNetV3's (`workloads.InvertedResidual(..., k=5)`) - runs on the integer dot-product kernel of csrc/conv_dw5_i8.hip (K.conv2d_dw5_i8:
    byte transposes + v_dot4_i32_i8, as the 3x3 kernels) instead of the any-filter kernel, which converts every byte of every tap to fp32
    (`fusion_report.dw5` counts the layers).  Taken: a "dw" plan layer whose filter is 5x5, padding 2 and stride 1 or 2 in both axes, at most
    2048 channels once padded to 64, whose input quantiser has no float offset; everything else about the node - codes in, codes and / or
    fp32 out, ReLU / ReLU6, channel padding, shifted codes - is as it is.  Left on today's route: any other filter or padding (the reference's
    SameConv, an F.pad in front of an unpadded convolution, included), wider layers; a padded 5x5 layer behind a float activation offset
    stays unplanned.  Same exact integer sums, same fp32 steps in the same order: bit-identical to the plan without the flag
    (tests/test_gpu_dw5.py: torch.equal against K.conv2d_dw_i8 and between the two plans' logits).  Measured stand-alone (tools/dw5_ab.py,
    profiles/dw5_ab.json; the five 5x5 layer shapes of EfficientNet-B0 at batch 256, interleaved): 1.8 - 5.1 times the generic kernel's
    rate on codes-only layers, 1.4 times with the fp32 output, every case beyond the run-to-run spread; the whole
    EfficientNet-B0 plan (`workloads.efficientnet_b0()`, batch 128, gates and swish on): flag off / on = 6.86 / 6.85 ms per step (FSPTQ W8A8),
    6.54 / 6.28 (QBase W8A8), logits equal.  Off by default: the plan without it is the plan as it was.
    `layer_norms=True`, `gelu=True`: the two operators in front of a transformer block's Linear layers
    (`workloads.vit_small()`) become plan nodes that hand those layers their activation codes in one read of the fp32 rows and every other
    reader the fp32 values from the same launch (`fusion_report.layer_norms`, `.gelus` count the nodes).  `layer_norms`: an nn.LayerNorm
    over the last dimension alone, called with one positional argument, C % 4 == 0, 4 <= C <= 2048, whose code readers are Linear plan
    layers of C in-features sharing one quantiser (LayerNormLayer, csrc/layernorm.hip: one wave per row, two-pass mean / variance in a
    fixed summation order).  `gelu`: nn.GELU() / F.gelu in the erf form (`approximate="none"`), not in place, a user module whose body is
    one of these included, read by Linear plan layers (rows) or by 4-D "gemm" plan convolutions (a map with the channel-padded code rows
    of the average-pool rule), never both (GeluLayer, csrc/gelu.hip: the fourth map-to-codes op).  Left as they are: F.layer_norm, a
    LayerNorm over more dimensions, other widths, the tanh form, a LayerNorm or GELU nobody takes as codes, readers that disagree on
    their quantiser.  Both passes run after the main pass, whose decisions for the Linear layers stay - only their input changes, from
    fp32 to codes - and before the head pass; attention's products and softmax stay in torch unless `attention=True` (below).  An input that at run time is no fp32
    device tensor of the planned width takes the node's torch restatement.  The codes are K.fake_quant of the node's own fp32 values bit
    for bit, so the plan equals the flag-off plan of the network whose LayerNorm / GELU modules return the kernels' fp32 outputs
    (tests/test_gpu_transformer.py); against torch's own LayerNorm the values differ in the last bits (another summation order), within
    the stated bounds.  Measured (tools/transformer_ab.py, profiles/transformer_ab.json; ViT-S/16, 25 LayerNorm and 12 GELU nodes, batch
    256 at 224^2, interleaved): flags off / on = 16.54 / 13.84 ms per step (FSPTQ W8A8), 16.52 / 13.84 (QBase W8A8), ratio 1.20 / 1.19 at a
    spread of 0.06 ms; about half the logits differ, by at most 0.035 at a largest logit of 1.3.  Off by default: the plan without them
    is the plan as it was.
    `attention=True`: `matmul(softmax(matmul(q, k.transpose(-1, -2)) * c, dim=-1), v)` - c a Python float on either
    side; torch.softmax, F.softmax, the method or an nn.Softmax module over the last axis; every intermediate read once - or
    F.scaled_dot_product_attention(q, k, v) without mask, dropout or causal flag becomes one AttentionLayer node (csrc/attention.hip: a
    flash forward on the f32 matrix cores, fp32 semantics, the stated operation order and error bound of include/dlmcq.h;
    `fusion_report.attentions` counts the nodes).  With the merge-heads tail behind it - `permute(0, 2, 1, 3)` / `transpose(1, 2)`,
    then `reshape` / `view` to three sizes or `flatten(2)`, each read once - the node stands where the reshape stood, writes
    [B, Tq, H * D] directly and hands the Linear plan layers that read it (one quantiser) their activation codes from the same launch;
    without it the node stands where the second product stood, fp32 only.  Left alone: a mask added to the scores, is_causal, dropout,
    a softmax over another axis, scores with a second reader, a head dimension spelled as an int other than 32 or 64.  At run time,
    anything that is not three fp32 device views the kernel reads in place (unit stride in D, strides multiples of 4 elements, 16-byte
    aligned, D 32 or 64), or a reshape that turns out not to merge the heads, takes the node's torch restatement: the graph's own ops.
    Runs after the LayerNorm and GELU passes.  Off by default: the plan without it is the plan as it was.
    `patch_embed=True`: what stands in front of a vision transformer's first block (`workloads.vit_small()`).  The
    rearrangement `reshape | view(-1, C, g1, p, g2, p) -> permute(0, 2, 4, 3, 5, 1) -> reshape | view(-1, g1 * g2, p * p * C)` - every
    size a Python int, each node read by the next alone, p % 4 == 0, a strip of g2 * p * p * C elements within 65536 - read by Linear
    plan layers of p * p * C in-features sharing one quantiser becomes a PatchRowsLayer node (csrc/patch_rows.hip): one read of the
    image hands the embedding its activation codes, and anyone else the fp32 rows (`fusion_report.patch_rows`).  The main pass's
    decision for the embedding stays - only its input changes, from fp32 to codes.  `cat((cls.expand(B, -1, -1), x), dim=1) + pos` -
    cls [1, 1, C] and pos [1, T + 1, C] parameters of the model, C % 4 == 0, x any fp32 value, each intermediate read once; the add in
    either operand order or in place (`x += pos`), pos whole or as `pos[:, :n]` with a Python int n - becomes a TokenAssembleLayer node
    (csrc/tokens.hip): one add per element in one launch (`fusion_report.token_assemblies`); the parameters are read at every call.
    Left alone, with the reason in `fusion_report.patch_embed_left`: another permute, a second reader of an intermediate, a Linear of
    other in-features, p % 4 != 0, a position embedding whose length is not the token count the graph states, a slice bound read from
    a tensor (the reference's `pos[:, :(n + 1)]` with n from x.shape).  Both nodes are bit-identical to the ops they replace - no
    arithmetic but the quantiser's in the first, one IEEE add in the second (tests/test_gpu_patch_rows.py, tests/test_gpu_tokens.py) -
    so the plan's logits are torch.equal to the plan's without the flag (tests/test_gpu_patch_embed_plan.py).  At run time an input the
    kernels do not take (not fp32, a channels_last image batch, misaligned) runs the same torch ops inside the node.  Runs after the
    main pass and before the LayerNorm pass.  Off by default: the plan without it is the plan as it was.
    `squeezes=True`: the squeeze path of a squeeze-excite block - a global average pool of x (a spelling the head pass
    knows), an optional flatten / view / reshape(x.size(0), -1), a QBase or FSPTQ Linear or unpadded 1x1 / stride 1 convolution, nothing,
    a ReLU or a swish (x * sigmoid(x)), a second such layer, an optional view(N, C, 1, 1), and torch.sigmoid, nn.Hardsigmoid,
    F.hardsigmoid or the spelled-out relu6(v + 3) / 6, every node read by the next alone - becomes one SqueezeLayer node: the pool
    kernel hands layer 1 its activation codes and one launch (csrc/squeeze_i8.hip) takes them to the fp32 gate, the hidden vector never
    leaving the chip (`fusion_report.squeezes` counts the nodes).  The layers' frozen quantisers are read with kind "gemm" directly - the
    64-channel rule of the tiled kernel does not apply - so EfficientNet's 4- to 48-wide layers leave `not eligible`; layers the main
    pass had planned (MobileNetV2-SE's convolutions) leave `int8 layers`.  Left as they are, with the reason in
    `fusion_report.squeeze_left`: asymmetric weights or weight codes beyond int8, a float activation offset, AdaRound / dist_recon
    weights, more than 2048 channels or 512 hidden units, a plan built with `weight_blob`, 4-bit weights under `pack_int4`.  Runs behind
    the gate pass, which therefore takes every gate it took.  The two layers compute dlmcq_conv2d_i8_nhwc_fused's values bit for bit
    (tests/test_gpu_squeeze.py); against the plan without the flag the pooled sum's order and integer arithmetic where fp32 F.linear was
    move values across quantiser ties, so logits differ in their last digits.  Off by default: the plan without it is the plan as it was.
    `hardswish=True`: hard swish `x * relu6(x + 3) / 6` of a 4-D map - MobileNetV3's activation
    (`workloads.mobilenet_v3_large()`, `mobilenet_v3_small()`) - becomes a plan node (HardswishLayer, csrc/hardswish.hip) that hands the
    plan convolutions behind it, depthwise ones included, their activation codes in one pass and every other reader (a squeeze-excite
    pool, the gate node, a shortcut add) the activated fp32 map from the same launch (`fusion_report.hardswishes` counts the nodes).
    Taken: nn.Hardswish (an inplace one only where nothing else reads its input); F.hardswish, not in place; the spelled-out
    `x * relu6(x + 3) / 6` and `x * (relu6(x + 3) / 6)` - the addend exactly 3, F.relu6 / nn.ReLU6 / F.hardtanh(., 0, 6), `/ 6` or
    `* (1 / 6)`, either operand first, each intermediate read by the next node alone; `x * F.hardsigmoid(x)` / `x * nn.Hardsigmoid()(x)`;
    a user module whose body is one of these.  The two multiplies round differently in about a quarter of the elements, so the node
    computes them in the order of the spelling it replaces (`.order`, `.decision`): (x * r) * fl32(1 / 6) for nn.Hardswish, F.hardswish
    and `(x * r) / 6`, x * (r * fl32(1 / 6)) for `x * (r / 6)` and `x * hardsigmoid(x)` - bit-identical to those ops on the device, so
    the plan's logits equal the flag-off plan's (tests/test_hardswish_gpu.py).  The readers and the no-taker case are the swish pass's.
    Left as they are: the hard swish on the (N, hidden) vector of the classifier or inside a squeeze path, `x * hardsigmoid(y)`, a
    squeeze-excite gate, F.hardswish(inplace=True), another addend or divisor, an intermediate with a second reader.  An input that at
    run time is no 4-D fp32 map of the planned width takes the node's torch path: the spelling that was matched.  The pass runs beside
    the swish pass, before the gate pass.  Measured (tools/hardswish_ab.py, profiles/hardswish_ab.json; batch 256 at 224^2, gates and dw5
    on in both, interleaved): MobileNetV3-Large flag off / on = 6.61 / 5.17 ms per step (FSPTQ W8A8), 6.56 / 5.15 (QBase W8A8), beyond the
    run-to-run spread; MobileNetV3-Small 3.69 / 3.78 and 3.34 / 3.32, inside it; logits equal in all four.  Off by default: the plan
    without it is the plan as it was."""
    if not any(gap_head is v for v in (False, True)) and gap_head not in ("separate", "fused"):
        raise ValueError(f"fuse_inference: gap_head is False, True, 'separate' or 'fused', not {gap_head!r}")
    if model.training:
        raise RuntimeError("fuse_inference: the plan is for inference - call model.eval() first")
    report = report if report is not None else FusionReport()
    try:
        graph = _Tracer().trace(model)
    except Exception as e:   # data-dependent control flow, *args signatures, ... - torch.fx says which line
        raise RuntimeError(f"fuse_inference reads the model's dataflow with torch.fx and could not trace it ({type(e).__name__}: "
                           f"{e}); the module-by-module path (quantize_model(..., int8_gemm=True)) needs no tracing") from e
    gm = fx.GraphModule(model, graph)
    # folded BatchNorms (merge_bn leaves nn.Identity) and eval-mode Dropout are wires, not operations
    modules = dict(gm.named_modules())
    for node in list(graph.nodes):
        if node.op == "call_module" and isinstance(modules[node.target], (nn.Identity, nn.Dropout)) and len(node.args) == 1:
            node.replace_all_uses_with(node.args[0])
            graph.erase_node(node)
    planned = _MainPass(gm, dry_run, weight_blob, dwpw, relu6, act_offsets, narrow_rows, pad_shortcuts, dw5).run(report)
    if swish:           # (before the gate pass, which finds its gated map and the squeeze's pool behind a swish node's fp32 output)
        _swish_pass(gm, report, planned, dry_run, dwpw)
    if hardswish:       # (beside the swish pass and before the gate pass, for the same reason)
        _hardswish_pass(gm, report, planned, dry_run, dwpw)
    if gates:           # (first: the squeeze's global pool is a plain node still, and so are the nodes behind the gate)
        _gate_pass(gm, report, planned, dry_run, relu6)
    if squeezes:        # (behind the gate pass: the gate node keeps reading the value the squeeze node now returns; before the head pass, which would take a squeeze's pool in front of a 64-aligned Linear for a head)
        _squeeze_pass(gm, report, planned, dry_run, weight_blob, pack_int4)
    if avg_pools:       # (before the head and the chain passes, like the head pass: the nodes behind the pool are plain plan nodes still)
        _avgpool_pass(gm, report, planned, dry_run)
    if patch_embed:     # (after the main pass, whose decision for the embedding stays; before the LayerNorm pass, which reads the token tensor)
        _patch_embed_pass(gm, report, planned, dry_run)
    if layer_norms:     # (after the main pass, whose decisions for the Linear layers stay; before the head pass, like the average pools)
        _layernorm_pass(gm, report, planned, dry_run)
    if gelu:
        _gelu_pass(gm, report, planned, dry_run, dwpw)
    if attention:
        _attention_pass(gm, report, planned, dry_run)
    if gap_head:        # (before the chain / layout passes: the head reads its shortcut row-major)
        _gap_pass(gm, report, gap_head, planned, dry_run)
    if chain_pairs and (not dry_run or dry_run == "chains"):
        _chain_pass(gm, report)
        if block_layout:
            _block_layout_pass(gm, report)
        if RECOMPUTE_DEFAULT if recompute_shortcuts is None else recompute_shortcuts:
            _recompute_pass(gm, report, RECOMPUTE_ENABLED)
        if dwpw:      # (off by default: measured no faster than the two launches - both halves of a MobileOne unit are bound by their
            #            own vector arithmetic, not by the code tensor between them: LABNOTES round 4)
            _dwpw_pass(gm, report)
    gm.packed_weights = _pack_plan_weights(gm) if (pack_int4 and not dry_run) else []
    gm.fusion_report = report
    return gm


_STREAM_POOL = {}


def _plan_streams(device, n):
    """The side streams of every StreamedPlan on a device come from ONE pool: the runtime maps streams onto a few hardware queues,
    and a second plan's fresh streams can land on queues the first plan's already occupy - its shares then run one after the other
    (RepVGG-A1 behind ResNet-50 in one process: 2.28 ms per step on fresh streams, 1.85 on the shared ones = what it takes alone)."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    pool = _STREAM_POOL.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=device))
    return pool[:n]


class StreamedPlan:
    """Run a frozen plan on `n_streams` HIP streams, each taking a contiguous share of the batch.

    A ResNet alternates layers bound by HBM (1x1 expansions that write a shortcut) with layers bound by the operand
    path of the matrix cores (3x3s, 1x1 reductions), and every launch has a ramp and a tail.  Two shares of the batch,
    one layer apart on two streams, fill each other's gaps: ResNet-50 at 512 images, 8.81 -> 8.14 ms (+8 %), three or
    four streams give less.  Outputs are bit-identical to the single-stream plan: nothing in the plan depends on the
    batch size once the scales are frozen - except the QBase family, whose `grad_scale` factor g = 1/sqrt(numel*hi)
    (modules/base.py:96-97) does; such plans are refused.

        fast = StreamedPlan(fuse_inference(model), n_streams=2)
        y = fast(x)
    """

    def __init__(self, plan, n_streams=2):
        if n_streams < 1:
            raise ValueError("n_streams must be >= 1")
        for m in plan.modules():
            if isinstance(m, _PlanLayer) and (m.act.needs_g or (m.emit is not None and m.emit.needs_g)):
                raise ValueError("StreamedPlan: this plan holds QBase quantisers whose scale depends on the number of "
                                 "elements per call (grad_scale); splitting the batch would change the result")
        self.plan, self.n = plan, int(n_streams)
        self.streams = None

    def __call__(self, x):
        if self.n == 1 or x.shape[0] < self.n:
            return self.plan(x)
        if self.streams is None:
            self.streams = _plan_streams(x.device, self.n)
        cur = torch.cuda.current_stream(x.device)
        parts = x.chunk(self.n, dim=0)
        outs = [None] * len(parts)
        for i, part in enumerate(parts):
            s = self.streams[i]
            s.wait_stream(cur)
            with torch.cuda.stream(s):
                outs[i] = self.plan(part)
        for s in self.streams[:len(parts)]:
            cur.wait_stream(s)
        for o, s in zip(outs, self.streams):
            o.record_stream(cur)       # produced on a side stream, consumed (and later freed) on the caller's
        return torch.cat(outs, dim=0)
