"""Every instantiation of conv_i8_mfma_kernel (csrc/conv_i8.hip: the 48 (tile width, flags) pairs of DLMCQ_CV_TABLE) against an
independent float64 reference, whole tensor, NO tolerance - on full-range operands (tests/exact_layers.py: make_full_range_layer): codes
over all 256 byte values, weight codes in +-127, per-channel dyadic weight scales that differ from channel to channel, a dyadic input
scale != 1, an input zero point in 1..254 other than 128 (uint8 calls: above 128 on strided borders, below on dilated ones), biases that are multiples of each channel's s_in * s_w[k].  The
calls are tests/tiled_variant_cases.py's (smallest reduction that reaches the pair, a ring wrap at another phase, partial row tiles with
image seams, column tiles at n0 != 0, ragged last tiles, strided / dilated borders, both input types); each is first asked with
DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_VARIANT, for the very arguments about to be launched, which pair it runs.

Reference: float64 convolution of the DEQUANTISED operands (zero padding) + bias + shortcut + second pair, the activation, exact_f32.
Why the kernel's fp32 result must equal it bit for bit: the int32 sums are exact, every scale is a power of two, and every fp32 operation
of the epilogue's chain (conv_epilogue.h / conv_i8.hip) is a single rounding of an exact value - so it is exact whenever its real-valued
result is an fp32 number.  The conditions, asserted on the CPU before any launch (tests/exact_stages.py: `pair_stages`; `reference`):
  * |SUM q' qw|, |(shift - zp) SUM qw| and their sum below 2^24 (the sum is converted to fp32);
  * dequant1 = fma(sum, s_in s_w[k], bias[k]) representable (a multiple of the unit s_in s_w[k] below 2^24 units);
  * ASYM: woff = s_in * w_off[k] representable (w_off an integer multiple of s_w[k]); the row sum SUM (q - zp) over the real taps below
    2^24; the product rowsum * woff representable; v + product representable;
  * XOFF (the construction of tests/test_gpu_act_offset.py: x^ = q s + o, zero point 0, o an integer multiple of s): the folded bias
    bias + o * SUM_taps tap[k] representable; every per-tap sum an fp32 number and SUM |tap| below 2^24 s_w[k], so every partial sum of
    xoff_border4 / xoff_border1 is exact in any order; fma(-o, border, v) representable;
  * DUAL: the second pair's dequant1 representable, and the sum of the two;
  * + shortcut representable (the shortcut values are multiples of 1/4, or edge values on channels whose convolution is 0).
ReLU, ReLU6's bound and the quantiser add no rounding to the fp32 value.  No form needed unit scales.
Unswapped pairs: fp32 output and codes together; SWAP pairs: codes, against the oracle's quantiser of the exact fp32 reference.  Buffers
are sentinel-filled and checked beyond the written extent (rows past M; NARROW: fp32 rows are kf wide, nothing beyond M * kf)."""
import functools

import pytest
import torch

import exact_layers as X
import test_conv_dispatch_host as D
import tiled_variant_cases as V
from exact_stages import XOFF_O, assert_final_units, nhwc, pair_stages as _pair_stages, sentinel as _sentinel      # (shared with the halo file)
from test_gpu_epilogue_exact import DEV, expect_codes, same, settle

pytestmark = pytest.mark.gpu


def quant_of(kind, relu):
    """The consumer quantisers: `plain` spreads the outputs over 0..255 (ReLU6: [0, 6] / 2^-5 = 0..192; else sigma 12 / 2^-2), `signed` has
    a zero point and a signed range, `shift` emits DLMCQ_EMIT_SHIFT128 bytes."""
    s = 2.0 ** -5 if relu == 2 else 0.25
    if kind == "plain":
        return X.Quant(s)
    if kind == "shift":
        return X.Quant(s, shift128=True)
    return X.Quant(2.0 ** -5, -100.0, -128, 127) if relu == 2 else X.Quant(0.5, 3.0, -128, 127)


@functools.lru_cache(maxsize=None)
def reference(bn, flags, index):
    """Operands + the exact pre-activation reference of call `index` of the pair without R6 (its ReLU6 twin shares both)."""
    case = V.BY_PAIR[(bn, flags)][index]
    g = dict(D.BASE, **case.geo)
    gen = torch.Generator().manual_seed(7700 + 64 * V.PAIRS.index((bn, flags)) + index)
    with_res = case.mode == "res_out_codes"
    xoff, narrow, padres, dual = case.entry == "xoff", case.entry in ("narrow", "padres"), case.entry == "padres", case.entry == "dual"
    live = g["Kf"] if narrow else g["K"]
    lay = X.make_full_range_layer(gen, g["N"], g["C"], g["H"], g["W"], g["K"], g["R"], g["S"], signed_in=not g["uns"], asym=case.asym,
                                  zp=0 if xoff else None, live=live, edge_bias=not with_res, zp_side=None if g["pad"] == 0 else ("low" if g["dil"] == 2 else "high"))
    true, bias, tap = _pair_stages(lay, g, 128 if g["uns"] else 0, xoff=xoff)
    ops = dict(lay=lay, bias=bias, tap=tap, g=g, live=live)
    if dual:
        lay2 = X.make_full_range_layer(gen, g["N"], g["C2"], g["H2"], g["W2"], g["K"], 1, signed_in=False, edge_bias=False)
        lay2.wq[:lay.nz] = 0
        lay2.bias[:lay.nz] = 0.0
        true2, _, _ = _pair_stages(lay2, g, 128, second=True)
        true = X.exact_f32(true + true2, "sum of the two pairs").double()
        ops["lay2"] = lay2
    n, k, p, q = true.shape
    if with_res:
        if padres:
            cs, lo, rs = g["res_c"], g["res_clo"], g["res_stride"]
            src = X.edge_residual((n, cs, g["res_h"], g["res_w"]), max(0, min(cs, lay.nz - lo)), gen)
            res = torch.zeros(n, k, p, q)
            res[:, lo:lo + cs] = src[:, :, ::rs, ::rs]
            ops["src"] = src
        else:
            res = X.edge_residual((n, k, p, q), lay.nz, gen)
            res[:, live:] = 0.0                                      # (NARROW: the padded columns have no shortcut)
        ops["res"] = res
        true = X.exact_f32(true + res.double(), "+ shortcut").double()
    assert_final_units(true, lay)                                      # the final value in units of s_in * s_w[k]
    return ops, true


def run_case(case, errs):
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    bn, flags = case.pair
    index = V.BY_PAIR[case.pair].index(case)
    ops, base = reference(bn, flags & ~V.CV_R6, index)
    lay, g, live = ops["lay"], ops["g"], ops["live"]
    want = X.exact_f32(X.activation(base, case.relu), "activation")
    n, k, p, q_ = want.shape
    m = n * p * q_
    if case.relu == 2:      # a ReLU6 test in which everything saturates proves nothing
        vals = want[:, lay.nz:live][want[:, lay.nz:live].isfinite()]
        inside = float(((vals > 0) & (vals < 6)).float().mean())
        assert inside >= 0.10 and bool((vals == 0).any()) and bool((vals == 6).any()), (case.cid, inside)
    quant = quant_of(case.quant, case.relu)
    t = {}      # name -> device tensor (kept alive until the launch is done)

    def pair_tensors(lay_, sfx, bias):
        t["x" + sfx] = nhwc(lay_.codes).to(DEV)
        t["w" + sfx] = nhwc(lay_.wq).to(DEV)
        t["wsum" + sfx] = lay_.wq.to(torch.int32).sum(dim=(1, 2, 3)).to(torch.int32).to(DEV)
        t["bias" + sfx] = bias.to(DEV)
        t["s_in" + sfx] = torch.tensor([lay_.s_in], dtype=torch.float32, device=DEV)
        t["zp_in" + sfx] = torch.tensor([float(lay_.zp)], dtype=torch.float32, device=DEV)
        t["s_w" + sfx] = lay_.s_w.to(DEV)
    pair_tensors(lay, "", ops["bias"])
    if "lay2" in ops:
        pair_tensors(ops["lay2"], "2", ops["lay2"].bias)
    if case.asym:
        t["w_off"] = lay.w_off.to(DEV)
    if case.entry == "xoff":
        t["x_off"] = torch.tensor([XOFF_O * lay.s_in], dtype=torch.float32, device=DEV)
        t["x_tap"] = ops["tap"].permute(1, 2, 0).reshape(-1, k).contiguous().to(DEV)          # [R * S][K]
    if "res" in ops:
        t["res"] = nhwc(ops["src"]).to(DEV) if "src" in ops else nhwc(ops["res"])[..., :live].contiguous().to(DEV)
    t["q_scale"] = torch.tensor([quant.scale], dtype=torch.float32, device=DEV)
    if quant.zp is not None:
        t["q_zp"] = torch.tensor([quant.zp], dtype=torch.float32, device=DEV)
    rows = (m + 127) // 128 * 128 + 128                               # the row tiles' extent and one tile more
    t["out"] = _sentinel(rows * live, torch.float32)
    t["codes"] = _sentinel(rows * k, torch.uint8)
    args = case.route_args(ptr=lambda name: t[name].data_ptr())
    what = f"{case.cid} {case.entry} steps={case.steps} relu={case.relu} {quant.tag()}"
    # ---- which instantiation: asked for these very arguments
    assert V.decode(D.call(N.lib, case.entry, args)) == case.pair, what
    torch.cuda.synchronize()
    rc = V.launch(N.lib, case.entry, dict(args, ctl=args["ctl"] & ~V.ROUTE_VARIANT, stream=torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)
    out, codes = t["out"].cpu(), t["codes"].cpu()
    assert bool((codes[m * k:] == 0xA5).all()), what + ": code bytes written beyond row M"
    if case.mode == "codes":
        assert bool((out.view(torch.uint8) == 0xA5).all()), what + ": a codes-only call wrote fp32 values"
    else:
        assert bool((out[m * live:].view(torch.uint8) == 0xA5).all()), what + ": fp32 values written beyond the rows"
        same(out[:m * live].reshape(n, p, q_, live), nhwc(want)[..., :live].contiguous(), what + " fp32", errs)
    want_codes = nhwc(expect_codes(K, want, quant))
    same(codes[:m * k].view(want_codes.dtype).reshape(n, p, q_, k), want_codes, what + " codes", errs)


@pytest.mark.parametrize("pair", V.PAIRS, ids=V.pair_name)
def test_tiled_variant_is_exact_on_full_range_operands(pair):
    cases = V.BY_PAIR[pair]
    assert len(cases) >= 2
    errs = []
    for case in cases:
        run_case(case, errs)
    settle(errs)
