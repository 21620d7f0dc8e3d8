"""Every instantiation of the depthwise kernels - the 26 records of DW_TABLE (csrc/conv_dw_i8.hip), the 8 of DWM_TABLE (csrc/conv_dwm_i8.hip)
and the 6 of DWPW_TABLE (csrc/conv_dwpw_i8.hip) - against an independent float64 reference, whole tensor, NO tolerance, on full-range
operands (tests/exact_layers.py: make_full_range_layer(depthwise=True)): codes over all 256 byte values, weight codes in +-127, per-channel
dyadic weight scales that differ from channel to channel, a dyadic input scale != 1, uint8 zero points 0, above and below 128, int8 zero
points 0 and not 0, weight offsets of whole units of s_w[c], biases that are multiples of each channel's s_in * s_w[c] (or a null bias),
edge values (NaN, +-inf, ties) on zero-weight channels.  The calls are tests/dw_variant_cases.py's; a depthwise call is first asked with
DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_DW_VARIANT, for the very arguments about to be launched, which record it runs, and is launched once through
the C ABI (dlmc._native.lib).  The depthwise + pointwise entry point has no route query: its record follows from K and W
(tests/test_dw_variants_host.py proves the formula for every case).

Reference: float64 depthwise convolution of the DEQUANTISED operands (zero padding; with a float activation offset x^ = (q - zp) s + o padded
with the VALUE 0) + bias, activation, exact_f32, then the oracle's quantiser (expect_codes).  The kernels' fp32 value before the quantiser
equals it bit for bit under the staged conditions of tests/exact_stages.py (`dw_pair_stages`), asserted before any launch.  The unit of
depthwise + pointwise goes on from the reference's OWN first-stage codes (exact_layers.second_gemm_full_ref: +-127 pointwise weights, dyadic
scales, |integer sum| < 2^24 asserted).  The large cases (the two grid-stride ones, the two with unequal tile counts per workgroup) stage
their float64 reference with torch on the device - elementwise float64 arithmetic, none of the library's code.

Code and fp32 buffers are sentinel-filled and longer than the tensor: nothing beyond it may be written.  Compared: the code bytes of the
whole tensor, and where the call wants fp32, the fp32 output bit for bit.

Conditions that keep a case from proving nothing, computed from the reference alone before the launch, on the live channels:
  * at least 10 % of the reference codes lie strictly between the quantiser's bounds (under ReLU / ReLU6 the lower bound is the code of 0
    where that lies above the range's lower end); a call without a quantiser: 10 % of the values are not clamped by the activation;
  * the lower clamp occurs in every ReLU / ReLU6 case, and every ReLU6 case has reference values above 6;
  * at least one case per record has reference codes at the upper bound; which cases carry it is printed.  Under ReLU6 the upper bound is
    the code of 6 where that lies below the range's upper end, as the lower one is the code of 0: no value passes 6, and 6 / 2^-5 = 192 is
    the largest code the plain quantisers of QUANTS (the only ones the FAST and matrix-core R6 records take) can give."""
import dataclasses
import functools

import pytest
import torch

import dw_variant_cases as W
import exact_layers as X
import exact_stages as S
import test_dw_stem_refusals_host as D
from test_gpu_epilogue_exact import DEV, expect_codes, same, settle
from test_gpu_halo_variants import QUANTS

pytestmark = pytest.mark.gpu

# the quantiser between the two layers of a depthwise + pointwise unit: range 0..255 (the matrix step reads unsigned bytes), dyadic scale
Q1S = {"q1_plain": X.Quant(0.25), "q1_zp": X.Quant(0.25, 64.0), "q1_sym": X.Quant(0.5, form=X.FORM_SYMMETRIC), "q1_zp128": X.Quant(0.125, 128.0)}
assert set(Q1S) == set(W.Q1)
ON_DEVICE = 1 << 21         # elements from which the float64 staging runs on the device
TAIL = 4096


@functools.lru_cache(maxsize=None)
def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _t(v, dtype=torch.float32):
    return torch.tensor([v], dtype=dtype, device=DEV)


def _first_layer(case, g):
    """The depthwise layer of a case and its exact pre-activation reference (NHWC), the staged conditions asserted."""
    gen = torch.Generator().manual_seed(66000 + case.seed)
    lay = X.make_full_range_layer(gen, g["N"], g["C"], g["H"], g["W"], g["C"], g["R"], g["S"], signed_in=not case.uns, asym=case.asym, zp=case.zp,
                                  depthwise=True)
    assert lay.s_in != 1.0 and lay.zp == case.zp
    if not case.bias:
        lay.bias = torch.zeros(g["C"])
    if lay.codes.numel() >= ON_DEVICE:
        lay = dataclasses.replace(lay, codes=lay.codes.to(DEV))
    true, bias, tap = S.dw_pair_stages(lay, g, 128 if case.uns else 0, xoff=case.xoff)
    return gen, lay, true, bias, tap


def _first_operands(case, lay, bias, tap):
    c = lay.wq.shape[0]
    t = dict(x=S.nhwc(lay.codes).to(DEV), w=lay.wq[:, 0].permute(1, 2, 0).contiguous().to(DEV), s_in=_t(lay.s_in), zp_in=_t(float(lay.zp)),
             s_w=lay.s_w.to(DEV))
    assert t["x"].shape[-1] == c and t["w"].shape[-1] == c and t["x"].is_contiguous()
    if case.bias or case.xoff:          # (a float offset's folded term o * SUM tap rides in the bias: never null then)
        t["bias"] = bias.to(DEV)
    if case.asym:
        t["w_off"] = lay.w_off.to(DEV)
    if case.xoff:
        t["x_off"] = _t(S.XOFF_O * lay.s_in)
        t["x_tap"] = tap.to(DEV)
    return t


def code_facts(want_codes, q, relu, nz):
    """(share of the live channels' reference codes strictly inside the bounds, the lower clamp occurs, the upper clamp occurs); NHWC bytes."""
    c = want_codes[..., nz:].to(torch.int32)
    lo, hi = q.lo, q.hi
    if relu:
        lo = max(lo, int(X.oracle_codes(torch.zeros(1), q)))
    if relu == 2:
        hi = min(hi, int(X.oracle_codes(torch.full((1,), 6.0), q)))
    return float(((c > lo) & (c < hi)).float().mean()), bool((c == lo).any()), bool((c == hi).any())


def _conditions(what, case_act, facts, above6):
    inside, lower, upper = facts
    assert inside >= 0.10, (what, inside)
    assert lower or not case_act, what + ": the lower clamp does not occur"
    assert above6 or case_act != 2, what + ": no reference value above 6"
    return upper


def _untouched(buf, used, what):
    tail = buf.view(torch.uint8)[used * buf.element_size():].cpu()
    assert bool((tail == 0xA5).all()), what + ": bytes written beyond the tensor"


def dw_reference(case, cus, codes_of):
    """Everything a depthwise case knows before its launch: (layer, the bias and tap sums the kernel is handed, fp32 reference NHWC, its code
    bytes or None, the upper clamp occurs, a description), the conditions asserted.  `codes_of(v32, quantiser)`: the reference's bytes."""
    g = case.geo_for(cus)
    _, lay, true, bias, tap = _first_layer(case, g)
    quant = QUANTS[case.quant] if case.quant else None
    what = (f"{case.cid} {g['N']}x{g['H']}x{g['W']} C{g['C']} {g['R']}x{g['S']}/{g['stride']}/{g['pad']} act={case.act} bias={case.bias} "
            f"{'u8' if case.uns else 'i8'} zp={lay.zp} asym={case.asym} out={case.out} {quant.tag() if quant else 'fp32 only'}")
    if case.record[0] == "dwm":
        a = dict(ntiles=-(-g["N"] * (g["H"] + 1) * (g["W"] + 1) // W.DWM_TP), groups=W.dwm_groups(cus, g["C"] // 64))
        assert g["N"] * g["H"] * g["W"] >= 4096 and (g["N"] * (g["H"] + 1) * (g["W"] + 1)) % W.DWM_TP, what       # a partial last tile
        if case.geo["N"] is None:         # workgroups own two tiles or one
            assert a["groups"] < a["ntiles"] < 2 * a["groups"], (what, a)
    want = X.exact_f32(X.activation(true, case.act), "activation").cpu()
    n, p, q_, c = want.shape
    m = n * p * q_
    live = true[..., lay.nz:]
    above6 = bool((live[live.isfinite()] > 6).any())
    if quant:
        want_codes = codes_of(want, quant)
        upper = _conditions(what, case.act, code_facts(want_codes, quant, case.act, lay.nz), above6)
    else:
        kept = (live > 0) & ((live < 6) | (case.act != 2)) if case.act else live.isfinite()
        want_codes = None
        upper = _conditions(what, case.act, (float(kept.float().mean()), bool((live <= 0).any()), False), above6)
    return lay, bias, tap, want, want_codes, upper, what


def run_dw_case(case, errs):
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    cus = _cus()
    lay, bias, tap, want, want_codes, upper, what = dw_reference(case, cus, lambda v, q: expect_codes(K, v, q))
    quant = QUANTS[case.quant] if case.quant else None
    n, p, q_, c = want.shape
    m = n * p * q_
    t = _first_operands(case, lay, bias, tap)
    if quant:
        t["codes"] = S.sentinel(m * c + TAIL, torch.uint8)
        t["q_scale"] = _t(quant.scale)
        if quant.zp is not None:
            t["q_zp"] = _t(quant.zp)
    if case.out:
        t["out"] = S.sentinel(m * c + TAIL, torch.float32)
    args = case.route_args(ptr=lambda name: t[name].data_ptr(), cus=cus)
    assert W.decode(D.call(N.lib, case.entry, args)) == case.record, what
    torch.cuda.synchronize()
    rc = D.call(N.lib, case.entry, dict(args, q_form=args["q_form"] & ~(W.ROUTE_ONLY | W.ROUTE_DW_VARIANT), stream=torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)
    if quant:
        _untouched(t["codes"], m * c, what + " codes")
        same(t["codes"][:m * c].cpu().view(want_codes.dtype).reshape(n, p, q_, c), want_codes, what + " codes", errs)
    if case.out:
        _untouched(t["out"], m * c, what + " fp32")
        same(t["out"][:m * c].cpu().reshape(n, p, q_, c), want, what + " fp32", errs)
    return upper


def dwpw_reference(case, codes_of):
    """dw_reference for a depthwise + pointwise unit: (first layer, its bias, the pointwise layer's operands, the reference's code bytes NHWC,
    the upper clamp occurs, a description)."""
    g = case.geo_for()
    k, c = case.k, g["C"]
    gen, lay, true, bias, _ = _first_layer(case, g)
    q1, q2 = Q1S[case.q1], QUANTS[case.quant]
    what = (f"{case.cid} {g['N']}x{g['H']}x{g['W']} C{c} K{k} dw_relu={case.dw_relu} relu={case.act} bias={case.bias} {'u8' if case.uns else 'i8'} "
            f"zp={lay.zp} asym={case.asym}/{case.asym2} {q1.tag()} -> {q2.tag()}")
    assert W.dwpw_pieces(g["W"]) <= 12 and (2 if W.dwpw_pieces(g["W"]) <= 8 else 3) == case.record[2] and k == case.record[1], what
    mid = X.exact_f32(X.activation(true, case.dw_relu), "first activation")
    c1 = X.quantise(mid, q1)                                             # the reference's own first-stage codes, NHWC
    # the pointwise layer: zero-weight channels in front for the edge biases, dyadic scales, a bias in units of q1.scale * s_w2[k]
    nz2 = min(len(X.EDGE_VALUES), k - max(8, k // 4))
    wq2 = torch.randint(-127, 128, (k, c, 1, 1), generator=gen).to(torch.int8)
    wq2[:nz2] = 0
    s_w2 = (2.0 ** -(10 + torch.arange(k) % 5).double()).float()
    w_int2 = None
    if case.asym2:
        w_int2 = torch.randint(-1, 2, (k,), generator=gen)
        w_int2[:nz2] = 0
    bias2 = X.full_range_bias(k, nz2, k, q1.scale * s_w2.double(), gen)
    v2 = X.second_gemm_full_ref(c1.permute(0, 3, 1, 2), q1, wq2, s_w2, bias2, case.act, w_int2)
    want = S.nhwc(v2)
    want_codes = codes_of(want, q2)
    upper = _conditions(what, case.act, code_facts(want_codes, q2, case.act, nz2), True)
    return lay, bias, (wq2, s_w2, w_int2, bias2), want_codes, upper, what


def run_dwpw_case(case, errs):
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    lay, bias, (wq2, s_w2, w_int2, bias2), want_codes, upper, what = dwpw_reference(case, lambda v, q: expect_codes(K, v, q))
    g = case.geo_for()
    k, c = case.k, g["C"]
    q1, q2 = Q1S[case.q1], QUANTS[case.quant]
    n, p, q_, _ = want_codes.shape
    m = n * p * q_
    t = _first_operands(case, lay, bias, None)
    t.update(table=torch.zeros(c // 64 * 512, dtype=torch.int32, device=DEV), q_scale=_t(q1.scale), w2=wq2.reshape(k, c).contiguous().to(DEV),
             wsum=wq2.to(torch.int32).sum(dim=(1, 2, 3)).to(torch.int32).to(DEV), bias2=bias2.to(DEV), s_w2=s_w2.to(DEV), s_in2=_t(q1.scale),
             q2_scale=_t(q2.scale), codes=S.sentinel(m * k + TAIL, torch.uint8))
    if q1.zp is not None:
        t["q_zp"] = _t(q1.zp)
    if q2.zp is not None:
        t["q2_zp"] = _t(q2.zp)
    if w_int2 is not None:
        t["w_off2"] = X.exact_f32(w_int2.double() * s_w2.double(), "pointwise weight offset").to(DEV)
    ptr = lambda name: t[name].data_ptr() if name in t else None        # noqa: E731
    st = torch.cuda.current_stream().cuda_stream
    rc = N.lib.dlmcq_dwpw_pack_table(ptr("w"), ptr("bias"), ptr("s_in"), ptr("zp_in"), ptr("s_w"), ptr("w_off"), c, int(case.uns), ptr("table"), st)
    assert rc == 0, (what, rc)
    rc = D.call(N.lib, "dwpw_i8_nhwc", dict(
        x=ptr("x"), table=ptr("table"), dw_asym=int(case.asym), dw_bias=int(case.bias), dw_relu=case.dw_relu, zp_in=ptr("zp_in"), N=n, H=g["H"],
        W=g["W"], C=c, uns=int(case.uns), q_scale=ptr("q_scale"), q_zp=ptr("q_zp") or 0, q_lo=0, q_hi=255, q_form=q1.form, g=0.0, w=ptr("w2"),
        bias=ptr("bias2"), wsum=ptr("wsum"), s_in=ptr("s_in2"), s_w=ptr("s_w2"), w_off=ptr("w_off2") or 0, K=k, relu=case.act, codes=ptr("codes"),
        q2_scale=ptr("q2_scale"), q2_zp=ptr("q2_zp") or 0, q2_lo=q2.lo, q2_hi=q2.hi, q2_form=q2.form, g2=0.0, stream=st))
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)
    _untouched(t["codes"], m * k, what + " codes")
    same(t["codes"][:m * k].cpu().view(want_codes.dtype).reshape(n, p, q_, k), want_codes, what + " codes", errs)
    return upper


@pytest.mark.parametrize("record", W.RECORDS, ids=W.record_name)
def test_depthwise_variant_is_exact_on_full_range_operands(record):
    cases = W.BY_RECORD[record]
    assert len(cases) >= 2
    errs, carriers = [], []
    for case in cases:
        if (run_dwpw_case if record[0] == "dwpw" else run_dw_case)(case, errs):
            carriers.append(case.cid)
    settle(errs)
    print(f"upper clamp of {W.record_name(record)}: {carriers}")
    assert carriers, "no case of this record has reference codes at the upper bound"
