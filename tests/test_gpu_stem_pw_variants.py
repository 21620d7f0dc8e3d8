"""Every instantiation of the first-layer kernels (csrc/conv_stem_i8.hip: 40 + 7; csrc/conv_stem_pool7_i8.hip: 2), of the pointwise kernel
(csrc/conv_pw_i8.hip: 36) and of the block-end kernel (csrc/conv_pwr_i8.hip: 8) against an independent float64 reference, whole tensor, NO
tolerance, on full-range operands (tests/exact_layers.py: make_full_range_layer): codes over all 256 byte values, weight codes in +-127,
per-channel dyadic weight scales that differ from channel to channel, a dyadic input scale != 1, uint8 zero points either side of 128, int8
codes, weight offsets of whole units of s_w[k], biases that are multiples of each channel's s_in * s_w[k] (or a null bias), edge values (NaN,
+-inf, ties) on zero-weight channels or, where a shortcut is added, in the shortcut (edge_residual).  The calls are
tests/stem_pw_variant_cases.py's; each is first asked with DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_PW_VARIANT, for the very arguments about to be
launched, which record it runs, and is launched once through the C ABI into sentinel-filled buffers.

Reference: float64 convolution of the DEQUANTISED operands (+ bias, + the second pair, + the shortcut), the activation, the float64 maximum
over the 3 x 3 / 2 / 1 window for the pooled first layer (F.max_pool2d: NaN wins, as test_stem_with_the_pool_inside pins), exact_f32, then the
oracle's quantiser (expect_codes).  Why the kernels' fp32 value equals it bit for bit - the chains, read from the kernels:
  first layer, unswapped (conv_stem_i8_kernel):  v = float(acc + (shift - zp) SUM qw) * (s_in s_w[k]) + bias[k]   (a product and a sum:
      -ffp-contract=off);  ASYM: v = v + float(S0) * (s_in o_w[k]), S0 = SUM q' + (shift - zp) R S C over the real taps and channels;
      XOFF: v = fma(-o, border, v) on border pixels (xoff_border4's sum of tap sums, r-major);  ReLU, ReLU6's bound;  store / quantise.
  first layer, SWAP:  the accumulators start from (shift - zp) SUM qw;  the same product, sum and ASYM term on channel pairs;  ReLU6's bound;
      the ReLU is the quantiser's lower clamp.
  pooled first layer (both kernels):  the maximum of the integer sums over the window (the dequantisation is monotone in the sum for a
      positive scale), then  v = float(max + (shift - zp) SUM qw) * (s_in s_w[k]) + bias[k];  ReLU;  store / quantise.
  pointwise (conv_pw_i8_kernel):  v = fma(float(acc), s_in s_w[k], bias[k]) with the accumulators started from (shift - zp) SUM qw;  ASYM:
      v = v + float(S0) * (s_in o_w[k]);  ReLU6's bound;  the ReLU is the plain quantiser's lower clamp.
  block end (conv_pwr_i8_kernel):  v = fma(float(acc), s_in s_w[k], bias[k]);  the dual form: the same of the sampled pair, then first pair +
      second pair;  else v = v + shortcut;  ReLU;  store / quantise.
Every operation is a single rounding of an exact value, so it is exact whenever its real-valued result is an fp32 number.  The conditions,
asserted on the ACTUAL operands before any launch (tests/exact_stages.py: `pair_stages`, `assert_final_units`; a seed that violates one is
changed, never the condition):
  * |SUM q' qw|, |(shift - zp) SUM qw| and their sum below 2^24 (1024 channels x 127 x 127 is just under it: asserted, not assumed);
  * every scale a power of two; the bias a multiple of s_in s_w[k]; the dequantised value a multiple of that unit below 2^24 units - so the
    product, the sum and the fma give the same number;
  * ASYM: s_in * w_off[k] representable (w_off a whole multiple of s_w[k]), the code sum below 2^24, the product and the sum representable;
  * XOFF (the construction of tests/test_gpu_act_offset.py: zero point 0, o a whole multiple of s_in, the buffer's border holds code 0): the
    folded bias representable, every tap sum an fp32 number and SUM |tap| below 2^24 s_w[k], fma(-o, border, v) representable;
  * the dual form: the second pair's value under the same conditions, and the sum of the two representable;
  * the shortcut: multiples of 1/4 on the live channels (edge values where the convolution is 0), v + shortcut representable.
The pooled kernels add none: the maximum of exact values is one of them.

Buffers are sentinel-filled and longer than the tensor: nothing beyond row M may change - for the first layer the rows of the partial last
tile, for pointwise the rest of the last block (M = 4232 = 132 blocks + 8 rows); a codes-only call must leave the fp32 buffer untouched.
Conditions that keep a case from proving nothing (computed from the reference alone; tests/test_stem_pw_variants_host.py asserts them on the
CPU for every case): ReLU6 cases have at least 10 % of the live values strictly inside (0, 6) and both bounds hit; the cases with a plain
quantiser reach the upper clamp.

The two conv_stem_pool7_i8_kernel records run on buffers WITHOUT padding, whose size is 4 and 12 mod 16: the kernel's window units start 8
bytes before a row, so the first unit of image 0 and the last of the last image straddle the buffer's ends and hold real pixels
(csrc/conv_stem_pool7_i8.hip: issue_group)."""
import functools

import pytest
import torch
import torch.nn.functional as F

import exact_layers as X
import exact_stages as S
import stem_pw_variant_cases as W
import test_conv_dispatch_host as T
import test_dw_stem_refusals_host as D
import tiled_variant_cases as V
from test_gpu_epilogue_exact import DEV, expect_codes, same, settle

pytestmark = pytest.mark.gpu

# the consumer quantisers: `plain` / `shift` (DLMCQ_EMIT_SHIFT128 bytes) clamp at 255 * 2^-4 = 15.9, 1.3 sigma of the widest channels; the
# ReLU6 ones spread [0, 6] over 0 .. 192
QUANTS = {"plain": X.Quant(2.0 ** -4), "shift": X.Quant(2.0 ** -4, shift128=True), "signed": X.Quant(0.5, 3.0, -128, 127), "plainx": X.Quant(2.0 ** -5),
          "plain6": X.Quant(2.0 ** -5), "shift6": X.Quant(2.0 ** -5, shift128=True), "signed6": X.Quant(2.0 ** -5, -100.0, -128, 127)}
TAIL = 4096


def _seed(case):
    base = W.BY_ID[case.ref] if case.ref else case
    return 91000 + 7 * W.CASES.index(base)


@functools.lru_cache(maxsize=8)
def operands(cid, cus):
    """Operands + the exact pre-activation reference (N, K, P, Q) float64 of a case (a ReLU6 twin shares its sibling's), conditions asserted."""
    case = W.BY_ID[cid]
    g = case.geo_for(cus)
    gen = torch.Generator().manual_seed(_seed(case))
    shift = 128 if case.uns else 0
    ops = dict(g=g)
    if case.family == "stem":
        pad = g["pad"] if case.xoff else 0
        lay = X.make_full_range_layer(gen, g["N"], g["C"], g["H"] - 2 * pad, g["W"] - 2 * pad, g["K"], g["R"], g["S"], signed_in=not case.uns,
                                      asym=case.asym, zp=case.zp)
        if not case.bias:
            lay.bias = torch.zeros(g["K"])
        true, bias, tap = S.pair_stages(lay, dict(stride=g["stride"], pad=pad, dil=1), shift, xoff=case.xoff)
        ops.update(lay=lay, bias=bias, tap=tap, gen=gen)
    else:
        g = dict(T.BASE, **g)
        ops["g"] = g
        dual = case.entry == "dual"
        lay = X.make_full_range_layer(gen, g["N"], g["C"], g["H"], g["W"], g["K"], 1, signed_in=not case.uns, asym=case.asym, zp=case.zp,
                                      edge_bias=not case.res)
        if not case.bias:
            lay.bias = torch.zeros(g["K"])
        true, bias, _ = S.pair_stages(lay, g, shift)
        ops.update(lay=lay, bias=bias)
        if dual:
            lay2 = X.make_full_range_layer(gen, g["N"], g["C2"], g["H2"], g["W2"], g["K"], 1, signed_in=not g["uns2"], edge_bias=False)
            lay2.wq[:lay.nz] = 0
            lay2.bias[:lay.nz] = 0.0
            true2, _, _ = S.pair_stages(lay2, g, 128 if g["uns2"] else 0, second=True)
            true = X.exact_f32(true + true2, "sum of the two pairs").double()
            ops["lay2"] = lay2
        if case.res:
            res = X.edge_residual(tuple(true.shape), lay.nz, gen)
            true = X.exact_f32(true + res.double(), "+ shortcut").double()
            ops["res"] = res
    S.assert_final_units(true, lay)
    return ops, true


def reference(case, cus, codes_of):
    """(operands, fp32 reference NHWC, its code bytes NHWC or None, facts) - facts: share of the live values strictly inside (0, 6), the
    lower / upper activation bounds hit, the quantiser's upper clamp reached."""
    ops, base = operands(case.ref or case.cid, cus)
    lay = ops["lay"]
    v = X.activation(base, case.act)
    if case.record[0] in ("pool", "pool7"):
        v = F.max_pool2d(v, 3, 2, 1)
    want = X.exact_f32(v, "activation")
    live = want[:, lay.nz:]
    vals = live[live.isfinite()]
    quant = QUANTS[case.quant] if case.quant else None
    want_codes = S.nhwc(codes_of(want, quant)) if quant else None
    facts = dict(inside=float(((vals > 0) & (vals < 6)).float().mean()), zero=bool((vals == 0).any()), six=bool((vals == 6).any()),
                 upper=bool(quant and quant.plain and (want_codes.view(torch.uint8)[..., lay.nz:] == (0x7f if quant.shift128 else 0xff)).any()))
    return ops, S.nhwc(want), want_codes, facts


def assert_facts(case, facts):
    if case.act == 2:
        assert facts["inside"] >= 0.10 and facts["zero"] and facts["six"], (case.cid, facts)
    elif case.quant in ("plain", "shift", "plainx"):
        assert facts["upper"], (case.cid, "the upper clamp does not occur")


def _t(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


def _pair(t, lay, sfx, bias):
    t["x" + sfx] = S.nhwc(lay.codes).to(DEV)
    t["w" + sfx] = S.nhwc(lay.wq).to(DEV)
    t["wsum" + sfx] = lay.wq.to(torch.int32).sum(dim=(1, 2, 3)).to(torch.int32).to(DEV)
    t["bias" + sfx] = bias.to(DEV)
    t["s_in" + sfx], t["zp_in" + sfx], t["s_w" + sfx] = _t(lay.s_in), _t(float(lay.zp)), lay.s_w.to(DEV)


def _stem_tensors(case, ops, t):
    """The first layer's operands as the entry points take them: the NHWC4 code buffer (padded with code 0 under a float offset; the
    channels past C hold random bytes, and 64 bytes follow the last row: a fragment load reads 8 taps whatever S is), weights [K][R][8][4]."""
    lay, g = ops["lay"], ops["g"]
    n, c, h, w = lay.codes.shape
    k, _, r, s = lay.wq.shape
    pad = g["pad"] if case.xoff else 0
    gen = torch.Generator().manual_seed(5)
    x4 = torch.randint(0, 256, (n, h, w, 4), generator=gen).to(torch.uint8)
    x4[..., :c] = S.nhwc(lay.codes).view(torch.uint8)
    xp = torch.zeros(n, h + 2 * pad, w + 2 * pad, 4, dtype=torch.uint8)
    xp[:, pad:pad + h, pad:pad + w] = x4
    assert (xp.shape[1], xp.shape[2]) == (g["H"], g["W"])
    buf = torch.cat([xp.reshape(-1), torch.randint(0, 256, (64 + 16,), generator=gen).to(torch.uint8)]).to(DEV)
    t["xbuf"] = buf
    w8 = torch.zeros(k, r, 8, 4, dtype=torch.int8)
    w8[:, :, :s, :c] = lay.wq.permute(0, 2, 3, 1)
    t["w"] = w8.to(DEV)
    t["wsum"] = lay.wq.to(torch.int32).sum(dim=(1, 2, 3)).to(torch.int32).to(DEV)
    t["bias"] = ops["bias"].to(DEV)
    t["s_in"], t["zp_in"], t["s_w"] = _t(lay.s_in), _t(float(lay.zp)), lay.s_w.to(DEV)
    if case.xoff:
        t["x_off"] = _t(S.XOFF_O * lay.s_in)
        t["x_tap"] = ops["tap"].permute(1, 2, 0).reshape(-1, k).contiguous().to(DEV)


def _chunk_major(v):
    """(M, K) row-major -> [K / 64][M][64] (DLMCQ_FP32_*_CHUNK_MAJOR)."""
    m, k = v.shape
    return v.reshape(m, k // 64, 64).permute(1, 0, 2).contiguous()


def run_case(case, errs):
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    cus = int(torch.cuda.get_device_properties(0).multi_processor_count)
    ops, want, want_codes, facts = reference(case, cus, lambda v, q: expect_codes(K, v, q))
    assert_facts(case, facts)
    lay = ops["lay"]
    quant = QUANTS[case.quant] if case.quant else None
    n, p, q_, k = want.shape
    m = n * p * q_
    t = {}
    if case.family == "stem":
        _stem_tensors(case, ops, t)
    else:
        _pair(t, lay, "", ops["bias"])
        if "lay2" in ops:
            _pair(t, ops["lay2"], "2", ops["lay2"].bias)
        if "res" in ops:
            r = S.nhwc(ops["res"]).reshape(m, k)
            t["res"] = (_chunk_major(r) if case.cm else r).contiguous().to(DEV)
    if case.asym:
        t["w_off"] = lay.w_off.to(DEV)
    if quant:
        t["q_scale"] = _t(quant.scale)
        if quant.zp is not None:
            t["q_zp"] = _t(quant.zp)
    t["out"] = S.sentinel(m * k + TAIL, torch.float32)
    t["codes"] = S.sentinel(m * k + TAIL, torch.uint8)
    what = f"{case.cid} {case.entry} {ops['g']} act={case.act} bias={case.bias} {'u8' if case.uns else 'i8'} zp={lay.zp} {quant.tag() if quant else 'fp32 only'}"
    ptr = lambda name: (t["xbuf"] if name == "x" and "xbuf" in t else t[name]).data_ptr()      # noqa: E731
    args = case.route_args(ptr=ptr, cus=cus)
    assert case.ask(N.lib, args) == case.record, what
    torch.cuda.synchronize()
    st = torch.cuda.current_stream().cuda_stream
    if case.family == "stem":
        rc = D.call(N.lib, case.entry, dict(args, q_form=args["q_form"] & ~(W.ROUTE_ONLY | W.ROUTE_PW_VARIANT), stream=st))
    else:
        rc = V.launch(N.lib, case.entry, dict(args, ctl=args["ctl"] & ~W.ROUTE_PW_VARIANT, stream=st))
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)
    out, codes = t["out"].cpu(), t["codes"].cpu()
    assert bool((codes[m * k:] == 0xA5).all()), what + ": code bytes written beyond row M"
    assert bool((out[m * k:].view(torch.uint8) == 0xA5).all()), what + ": fp32 values written beyond row M"
    if case.out:
        got = out[:m * k]
        got = got.reshape(k // 64, m, 64).permute(1, 0, 2).reshape(m, k) if case.cm else got.reshape(m, k)
        same(got.reshape(n, p, q_, k).contiguous(), want.contiguous(), what + " fp32", errs)
    else:
        assert bool((out.view(torch.uint8) == 0xA5).all()), what + ": a call without an fp32 output wrote fp32 values"
    if quant:
        same(codes[:m * k].view(want_codes.dtype).reshape(n, p, q_, k), want_codes.contiguous(), what + " codes", errs)
    else:
        assert bool((codes == 0xA5).all()), what + ": a call without a quantiser wrote codes"


@pytest.mark.parametrize("record", W.RECORDS, ids=W.record_name)
def test_variant_is_exact_on_full_range_operands(record):
    cases = W.BY_RECORD[record]
    assert len(cases) >= 2
    errs = []
    for case in cases:
        run_case(case, errs)
    settle(errs)
