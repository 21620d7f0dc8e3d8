"""The staged exactness conditions of the full-range tests (tests/test_gpu_tiled_variants.py, tests/test_gpu_halo_variants.py), asserted on
the CPU before any launch.  TEST INFRASTRUCTURE ONLY.

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
