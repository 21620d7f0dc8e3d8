"""The staged exactness conditions of the full-range tests (tests/test_gpu_tiled_variants.py, tests/test_gpu_halo_variants.py), asserted on
the CPU before any launch (tests/test_gpu_dw_variants.py: `dw_pair_stages`, the depthwise kernels' chain).  TEST INFRASTRUCTURE ONLY.

The int32 sums of the int8 kernels are exact, every scale of a full-range layer (tests/exact_layers.py: make_full_range_layer) is a power of
two, and every fp32 operation of the epilogue's chain (conv_epilogue.h) is a single rounding of an exact value - so the kernel's fp32
result equals the float64 convolution of the dequantised operands whenever every stage's real-valued result is an fp32 number.
`pair_stages` walks the chain stage by stage and asserts exactly that; `assert_final_units` bounds the final value."""
import torch
import torch.nn.functional as F

import exact_layers as X

DEV = "cuda:0"
LIMIT = float(1 << 24)
XOFF_O = -101           # the float activation offset in units of s_in


def conv(x, w, g, second=False):
    sfx = "2" if second else ""
    return F.conv2d(x, w, stride=g["stride" + sfx], padding=g["pad" + sfx], dilation=g["dil" + sfx])


def pair_stages(lay, g, shift, second=False, xoff=False):
    """One operand pair: (true float64 result before shortcut / activation, the bias the kernel is handed, tap sums or None), with the
    chain's conditions asserted stage by stage."""
    u = lay.unit.reshape(1, -1, 1, 1)
    xi = lay.xint()
    A = conv(xi, lay.wq.double(), g, second)                        # SUM (q - zp) qw over the real taps = SUM q' qw + (shift - zp) SUM qw
    wsum = lay.wq.double().sum(dim=(1, 2, 3))
    corr = ((shift - lay.zp) * wsum).reshape(1, -1, 1, 1)
    assert float((A - corr).abs().max()) < LIMIT and float(corr.abs().max()) < LIMIT and float(A.abs().max()) < LIMIT
    bias = lay.bias
    o = XOFF_O * lay.s_in if xoff else 0.0
    x_true = xi * lay.s_in
    tap_f = None
    if xoff:
        x_true = x_true + o                                          # x^ = q s + o, zero padded as a value: the padding is 0, not o
        tap = lay.w64().sum(dim=1)                                   # [K, R, S]: per-tap sums of the dequantised weights
        tap_f = X.exact_f32(tap, "tap sums")
        assert bool((tap.abs().sum(dim=(1, 2)) / lay.s_w.double() < LIMIT).all())
        bias = X.exact_f32(lay.bias.double() + o * tap.sum(dim=(1, 2)), "folded bias")
    true = conv(x_true, lay.w64(), g, second) + lay.bias.double().reshape(1, -1, 1, 1)
    v = X.exact_f32(A * u + bias.double().reshape(1, -1, 1, 1), "dequant1").double()
    live_ = (v / u)[:, lay.nz:]                                     # (channels [0, nz) carry the edge values: 0 * unit + bias, exact as it is)
    assert float(live_[live_.isfinite()].abs().max()) < LIMIT
    if lay.w_int is not None:
        woff = X.exact_f32(lay.s_in * lay.w_off.double(), "s_in * w_off").double().reshape(1, -1, 1, 1)
        s0 = conv(xi, torch.ones(1, *lay.wq.shape[1:], dtype=torch.float64), g, second)
        assert float(s0.abs().max()) < LIMIT
        v = X.exact_f32(v + X.exact_f32(s0 * woff, "rowsum * woff").double(), "+ weight-offset term").double()
    if xoff:
        ones = torch.ones(1, 1, *xi.shape[2:], dtype=torch.float64)
        inside = conv(ones, tap.unsqueeze(1), g)                     # the in-bounds taps' sum per output pixel
        border = tap.sum(dim=(1, 2)).reshape(1, -1, 1, 1) - inside
        v = X.exact_f32(v - o * border, "- o * border").double()
    ok = (v == true) | (v.isnan() & true.isnan())
    assert bool(ok.all()), "the staged chain and the convolution of the dequantised operands disagree"
    return true, bias, tap_f


def dw_conv(x, w, stride, pad):
    """Depthwise convolution in NHWC, float64: x (N, H, W, C) zero padded, w (R, S, C) -> (N, P, Q, C), as R S shifted multiply-adds (every
    product and sum of the full-range operands is an integer times a power of two below 2^53: exact, whatever the order)."""
    n, h, wd, c = x.shape
    r, s, _ = w.shape
    p, q = (h + 2 * pad - r) // stride + 1, (wd + 2 * pad - s) // stride + 1
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    y = torch.zeros(n, p, q, c, dtype=torch.float64, device=x.device)
    for i in range(r):
        for j in range(s):
            y.addcmul_(xp[:, i:i + (p - 1) * stride + 1:stride, j:j + (q - 1) * stride + 1:stride, :], w[i, j])
    return y


def dw_pair_stages(lay, g, shift, xoff=False):
    """pair_stages for a depthwise layer (make_full_range_layer(depthwise=True)), everything NHWC: (true float64 result (N, P, Q, C) before the
    activation, the bias the kernel is handed, tap sums fp32 (R S, C) or None), on the device the layer's tensors live on.

    The fp32 chain of ALL the depthwise kernels - conv_dw3p2_i8_kernel, conv_dw3_i8_kernel (FAST or not: on pairs, the same operations),
    conv_dw_i8_kernel, conv_dwm_i8_kernel and the first half of conv_dwpw_i8_kernel - is, from exact integer sums S1 = SUM (q - zp) qw and
    S0 = SUM (q - zp) over the real taps (v_dot4 / MFMA int32; the generic kernel: fp32 fmas of integers below 2^24),
        r = S1 * (s_in s_w);  r = r + S0 * (s_in o_w);  r = r + bias;  r = fma(-o, border, r)      (separate roundings but for the last)
    where a kernel leaves a step out (symmetric weights, a null bias) or adds a zero in its place (FAST, dwm).  Unlike the tiled kernels
    there is no fma(S1, m, bias).  Each partial result is asserted to be an fp32 number in that order, and - so that no other association
    order can differ - the SUM OF THE MAGNITUDES of the four terms is asserted to stay below 2^24 units of s_in s_w[c]: every partial sum of
    every subset is then an integer number of units below 2^24."""
    dev = lay.codes.device
    u = lay.unit.to(dev).reshape(1, 1, 1, -1)
    st, pad = g["stride"], g["pad"]
    xi = nhwc(lay.codes).double() - lay.zp
    wq = lay.wq[:, 0].permute(1, 2, 0).double().to(dev)                  # (R, S, C)
    A = dw_conv(xi, wq, st, pad)
    wsum = wq.sum(dim=(0, 1))
    corr = (shift - lay.zp) * wsum
    assert float((A - corr).abs().max()) < LIMIT and float(corr.abs().max()) < LIMIT and float(A.abs().max()) < LIMIT
    mags = A.abs()
    v = X.exact_f32(A * u, "S1 * (s_in s_w)").double()
    w64 = lay.w64()[:, 0].permute(1, 2, 0).to(dev)
    if lay.w_int is not None:
        woff = X.exact_f32(lay.s_in * lay.w_off.double(), "s_in * w_off").double().to(dev).reshape(1, 1, 1, -1)
        s0 = dw_conv(xi, torch.ones_like(wq), st, pad)
        assert float(s0.abs().max()) < LIMIT
        v = X.exact_f32(v + X.exact_f32(s0 * woff, "S0 * (s_in o_w)").double(), "+ weight-offset term").double()
        mags = mags + (s0 * woff / u).abs()
    bias = lay.bias
    o = XOFF_O * lay.s_in if xoff else 0.0
    x_true = xi * lay.s_in
    tap_f = None
    if xoff:
        x_true = x_true + o                                           # x^ = q s + o, zero padded as a value: the padding is 0, not o
        tap = w64                                                     # (R, S, C): one input channel per group - the tap sums are the weights
        tap_f = X.exact_f32(tap, "tap sums").reshape(-1, tap.shape[2]).contiguous()
        assert bool((tap.abs().sum(dim=(0, 1)) / lay.s_w.double().to(dev) < LIMIT).all())
        bias = X.exact_f32(lay.bias.double() + (o * tap.sum(dim=(0, 1))).cpu(), "folded bias")
    b = bias.double().to(dev).reshape(1, 1, 1, -1)
    v = X.exact_f32(v + b, "+ bias").double()
    mags = mags + (b / u).abs()
    if xoff:
        ones = torch.ones(1, *xi.shape[1:3], 1, dtype=torch.float64, device=dev)
        inside = dw_conv(ones.expand(1, -1, -1, tap.shape[2]), tap, st, pad)   # the in-bounds taps' sum per output pixel
        border = tap.sum(dim=(0, 1)).reshape(1, 1, 1, -1) - inside
        v = X.exact_f32(v - o * border, "- o * border").double()
        mags = mags + (o * border / u).abs()
    live_ = mags[..., lay.nz:]
    assert float(live_[live_.isfinite()].max()) < LIMIT, "the terms' magnitudes add up to 2^24 units or more"
    true = dw_conv(x_true, w64, st, pad) + lay.bias.double().to(dev).reshape(1, 1, 1, -1)
    ok = (v == true) | (v.isnan() & true.isnan())
    assert bool(ok.all()), "the staged chain and the depthwise convolution of the dequantised operands disagree"
    return true, bias, tap_f


def chain_stages(own, shift, *, residual=None, sampled=None, shift_s=0, stride=1, unit=None, shift_u=0, relu_shortcut=0):
    """The first epilogue of conv_chain_i8_kernel on full-range operands: the true float64 value (N, K, P, Q) before the block's own
    activation, every partial result asserted to be an fp32 number in the kernel's order -
        plain form:        fma(S, s_in s_w, b)                                     + residual
        dual form:         fma(S2, ..) of the SAMPLED operand first;  fma(S, ..) + that
        recomputing form:  fma(Sb, ..) sampled, fma(Sa, ..) unit;  a + b;  ReLU?;  fma(S, ..) + that   (the shortcut rounded to fp32 as the dual form stores it)
    each fma under pair_stages' conditions (integer sums below 2^24, the result a multiple of the unit below 2^24 units).  And, as dw_pair_stages
    does, so that no association order of the terms can differ: the SUM OF THE TERMS' MAGNITUDES stays below 2^24 units of the smallest unit among
    them, per channel, on the live channels (the edge channels of the extra operands are zero: there the sum is the edge value + 0)."""
    g1 = dict(stride=1, pad=0, dil=1)
    v, _, _ = pair_stages(own, g1, shift)
    terms, units = [v], [own.unit]
    if unit is not None:                                                 # the recomputed block: unit-stride operand a, sampled operand b
        assert sampled is not None and residual is None
        vb, _, _ = pair_stages(sampled, dict(stride=stride, pad=0, dil=1), shift_s)
        va, _, _ = pair_stages(unit, g1, shift_u)
        sc = X.exact_f32(va + vb, "recomputed shortcut: a + b").double()
        sc = X.exact_f32(X.activation(sc, 1 if relu_shortcut else 0), "recomputed shortcut").double()
        true = X.exact_f32(v + sc, "+ recomputed shortcut").double()
        terms += [va, vb]
        units += [unit.unit, sampled.unit]
    elif sampled is not None:
        assert residual is None
        vs, _, _ = pair_stages(sampled, dict(stride=stride, pad=0, dil=1), shift_s)
        true = X.exact_f32(v + vs, "+ convolution shortcut").double()
        terms.append(vs)
        units.append(sampled.unit)
    else:
        r = residual.double()
        true = X.exact_f32(v + r, "+ shortcut").double()
        terms.append(r)
        units.append(torch.full_like(own.unit, 0.25))                   # (edge_residual: multiples of 1/4 on the live channels)
    u = torch.stack(units).min(dim=0).values.reshape(1, -1, 1, 1)
    mags = (sum(t.abs() for t in terms) / u)[:, own.nz:]
    assert float(mags[mags.isfinite()].max()) < LIMIT, "the terms' magnitudes add up to 2^24 units or more"
    assert_final_units(true, own)
    return true


def assert_final_units(true, lay):
    """The final pre-activation value in units of s_in * s_w[k], on the live channels: below 2^24."""
    units = (true / lay.unit.reshape(1, -1, 1, 1))[:, lay.nz:]
    assert float(units[units.isfinite()].abs().max()) < LIMIT


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def sentinel(numel, dtype):
    """A device buffer whose every byte is 0xA5: what a kernel did not write still holds it."""
    t = torch.empty(numel, dtype=dtype, device=DEV)
    t.view(torch.uint8).fill_(0xA5)
    return t
