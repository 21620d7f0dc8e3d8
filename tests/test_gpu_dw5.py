"""The 5 x 5 depthwise kernel (csrc/conv_dw5_i8.hip; dlmcq_conv2d_dw5_i8_nhwc, K.conv2d_dw5_i8, fuse_inference(dw5=True)) on the GPU.

Every case of tests/dw5_cases.py is first asked, for the very arguments about to be launched, which record it runs (DLMCQ_ROUTE_ONLY |
DLMCQ_ROUTE_DW_VARIANT), launched once through the C ABI on sentinel-filled buffers, and held against TWO independent yardsticks, on the code
bytes and, where the call wants it, on the fp32 output's bits:
  * dlmcq_conv2d_dw_i8_nhwc - the generic kernel, the parent's route for such a layer - on the same operands: the route query must answer the
    `generic` family, and the two results must be equal byte for byte (no +0 / -0 allowance on the codes; fp32 by bits up to the sign of zero);
  * the exact float64 reference + oracle quantiser of tests/test_gpu_dw_variants.py (dw_reference: tests/exact_layers.py's full-range layer,
    tests/exact_stages.py's staged conditions), NO tolerance, with that file's conditions on every case (a tenth of the codes strictly inside
    the bounds, the lower clamp in every ReLU case, values above 6 in every ReLU6 case) and the upper clamp in at least one case per record.
Nothing beyond a tensor's end may be written.  Every record of the library's table is launched by at least one case: asserted from the
route answers.  The full-range case of each record puts every code at an end of the byte range against -128 / +127 weights in all 25 taps
(|S1| reaches 25 * 255 * 128 with one sign and 25 * 255 * 127 with the other, asserted) at the consumer scale 2^-5, where the upper clamp occurs; its reference is
float64 arithmetic on dyadic scales (every step exact in fp32, asserted by exact_f32).

The plan test: a small MBConv network (16 -> 96 and 24 -> 144 channels: padded to 128 and 192; a 5x5 / 1 block with squeeze-excite and swish,
a 5x5 / 2 block with ReLU6), batch 2 at 24^2, FSPTQ and QBase W8A8: the logits of dw5=True and dw5=False are torch.equal, 2 layers counted."""
import pytest
import torch
from torch import nn

import dw5_cases as W5
import exact_layers as X
import test_dw_stem_refusals_host as D
import test_gpu_dw_variants as TG
import workloads as WL
from exact_stages import nhwc, sentinel
from test_gpu_epilogue_exact import DEV, expect_codes, same, settle
from test_gpu_gate import PLAN_CASES, _net
from test_gpu_halo_variants import QUANTS

pytestmark = pytest.mark.gpu
TAIL = 4096
LAUNCHED = set()


def _buffers(t, quant, want_out, m, c):
    b = {}
    if quant:
        b["codes"] = sentinel(m * c + TAIL, torch.uint8)
    if want_out:
        b["out"] = sentinel(m * c + TAIL, torch.float32)
    return dict(t, **b)


def run_case(case, errs):
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    lay, bias, tap, want, want_codes, upper, what = TG.dw_reference(case, 256, lambda v, q: expect_codes(K, v, q))
    quant = QUANTS[case.quant] if case.quant else None
    n, p, q_, c = want.shape
    m = n * p * q_
    t = TG._first_operands(case, lay, bias, tap)
    if quant:
        t["q_scale"] = TG._t(quant.scale)
        if quant.zp is not None:
            t["q_zp"] = TG._t(quant.zp)
    new, old = _buffers(t, quant, case.out, m, c), _buffers(t, quant, case.out, m, c)
    st = torch.cuda.current_stream().cuda_stream
    args = W5.route_args(case, ptr=lambda name: new[name].data_ptr())
    assert W5.decode(W5.call(N.lib, args)) == case.record, what
    args_old = dict(case.route_args(ptr=lambda name: old[name].data_ptr()))
    assert TG.W.decode(D.call(N.lib, "dw_i8_nhwc", args_old))[:2] == ("dw", "generic"), what
    launch = ~(W5.ROUTE_ONLY | W5.ROUTE_DW_VARIANT)
    torch.cuda.synchronize()
    rc = W5.call(N.lib, dict(args, q_form=args["q_form"] & launch, stream=st))
    rc_old = D.call(N.lib, "dw_i8_nhwc", dict(args_old, q_form=args_old["q_form"] & launch, stream=st))
    torch.cuda.synchronize()
    assert (rc, rc_old) == (0, 0), (what, rc, rc_old)
    LAUNCHED.add(case.record)
    if quant:
        TG._untouched(new["codes"], m * c, what + " codes")
        assert torch.equal(new["codes"][:m * c], old["codes"][:m * c]), what + ": codes differ from the generic kernel's"
        same(new["codes"][:m * c].cpu().view(want_codes.dtype).reshape(n, p, q_, c), want_codes, what + " codes", errs)
    if case.out:
        TG._untouched(new["out"], m * c, what + " fp32")
        same(new["out"][:m * c].cpu(), old["out"][:m * c].cpu(), what + " fp32 against the generic kernel", errs)
        same(new["out"][:m * c].cpu().reshape(n, p, q_, c), want, what + " fp32", errs)
    return upper


@pytest.mark.parametrize("record", W5.RECORDS, ids=W5.record_name)
def test_dw5_variant_equals_the_generic_kernel_and_the_exact_reference(record):
    cases = W5.BY_RECORD[record]
    assert len(cases) >= W5.PER_RECORD
    errs, carriers = [], []
    for case in cases:
        if run_case(case, errs):
            carriers.append(case.cid)
    settle(errs)
    print(f"upper clamp of {W5.record_name(record)}: {carriers}")
    assert carriers, "no case of this record has reference codes at the upper bound"


def _full_range_operands(record):
    """Codes at the ends of the byte range (constant per channel: four channels the upper end, the next four the lower), weights -128 / +127 in all 25
    taps (channel % 4: all +127, all -128, -128 on even taps and +127 on odd ones, all -128), dyadic scales, offsets and biases in whole units."""
    f = W5.FULL_RANGE[record]
    g = W5.FULL_GEO
    n, h, w, c = g["N"], g["H"], g["W"], g["C"]
    ch = torch.arange(c)
    lo, hi = (0, 255) if f["uns"] else (-128, 127)
    codes = torch.where((ch // 4) % 2 == 0, hi, lo).reshape(1, 1, 1, c).expand(n, h, w, c).contiguous()
    taps = torch.arange(25).reshape(5, 5, 1)
    wq = torch.where((ch % 4 == 0).reshape(1, 1, c), 127, -128).expand(5, 5, c).clone()
    wq = torch.where((ch % 4 == 2).reshape(1, 1, c) & (taps % 2 == 1), 127, wq)
    s_in = 0.5
    s_w = 2.0 ** -(14.0 + (ch % 3).double())
    w_int = ((ch % 3) - 1).double() if f["asym"] else None
    gen = torch.Generator().manual_seed(4242 + W5.RECORDS.index(record))
    bias = torch.randint(-(1 << 19), 1 << 19, (c,), generator=gen).double() * (s_in * s_w)
    return f, g, codes, wq, s_in, s_w, w_int, bias


def full_range_reference(record):
    """(operands, float64 pre-activation reference NHWC, the integer sums S1): plain float64 arithmetic; every term a whole number of units
    s_in * s_w[c] with magnitudes summing below 2^24, so each fp32 step of the kernels is exact (exact_f32 asserts the values are fp32)."""
    f, g, codes, wq, s_in, s_w, w_int, bias = _full_range_operands(record)
    xi = codes.double() - f["zp"]
    s1 = TG.S.dw_conv(xi, wq.double(), g["stride"], 2)
    s0 = TG.S.dw_conv(xi, torch.ones_like(wq).double(), g["stride"], 2)
    u = (s_in * s_w).reshape(1, 1, 1, -1)
    units = s1.abs() + (s0 * w_int.reshape(1, 1, 1, -1)).abs() if w_int is not None else s1.abs()
    assert float((units + (bias / (s_in * s_w)).abs().reshape(1, 1, 1, -1)).max()) < 2 ** 24
    v = X.exact_f32(s1 * u, "S1 * (s_in s_w)").double()
    if w_int is not None:
        v = X.exact_f32(v + X.exact_f32(s0 * (w_int * s_w * s_in).reshape(1, 1, 1, -1), "S0 * (s_in o_w)").double(), "+ offset term").double()
    v = X.exact_f32(v + bias.reshape(1, 1, 1, -1), "+ bias").double()
    return (f, g, codes, wq, s_in, s_w, w_int, bias), v, s1


@pytest.mark.parametrize("record", W5.RECORDS, ids=W5.record_name)
def test_dw5_full_range_sums_reach_their_bound(record):
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    (f, g, codes, wq, s_in, s_w, w_int, bias), true, s1 = full_range_reference(record)
    dq = 255 if (f["uns"] or f["zp"] != 0) else 128          # the largest |q - zp|: the sum reaches 25 dq 128 with one sign, 25 dq 127 with the other
    assert float(s1.abs().max()) == 25 * dq * 128 and float(s1.max()) >= 25 * dq * 127 and float(s1.min()) <= -25 * dq * 127, (float(s1.min()), float(s1.max()))
    quant = QUANTS[f["quant"]]
    want = X.exact_f32(X.activation(true, f["act"]), "activation")
    want_codes = expect_codes(K, want, quant)
    top = min(quant.hi, int(X.oracle_codes(torch.full((1,), 6.0), quant))) if f["act"] == 2 else quant.hi     # (ReLU6: the code of 6, as in dw_reference)
    assert bool((X.oracle_codes(want, quant) == top).any()), "the upper clamp does not occur"
    x = codes.to(torch.uint8 if f["uns"] else torch.int8).permute(0, 3, 1, 2).to(DEV)       # (N, C, H, W) view of NHWC memory
    emit = K.EmitCodes(TG._t(quant.scale), None if quant.zp is None else TG._t(quant.zp), quant.lo, quant.hi, quant.form)
    kw = dict(w_offset=None if w_int is None else X.exact_f32(w_int * s_w, "w_off").to(DEV), stride=g["stride"], act=f["act"], emit=emit, want_out=f["out"])
    ops = (x, wq.to(torch.int8).contiguous().to(DEV), X.exact_f32(bias, "bias").to(DEV), TG._t(s_in), TG._t(float(f["zp"])), s_w.float().to(DEV))
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        new = K.conv2d_dw5_i8(*ops, **kw)
        old = K.conv2d_dw_i8(*ops, padding=2, **kw)
    finally:
        K.PROFILE.enabled = False
    assert [r[0] for r in K.PROFILE.records] == ["conv_dw5", "conv_dw"]
    K.PROFILE.reset()
    # which record ran: the entry point's own answer for these operands
    rq = dict(N=g["N"], H=g["H"], W=g["W"], C=g["C"], stride=g["stride"], uns=int(f["uns"]), relu=f["act"], out=D.P if f["out"] else 0,
              w_off=D.P if w_int is not None else 0, q_zp=D.P if quant.zp is not None else 0, q_lo=quant.lo, q_hi=quant.hi,
              q_form=quant.form | W5.ROUTE_ONLY | W5.ROUTE_DW_VARIANT)
    assert W5.decode(W5.call(N.lib, rq)) == record
    errs = []
    for got, ref in zip(new, old):
        if got is not None:
            assert torch.equal(got, ref), "differs from the generic kernel"
    if f["out"]:
        same(new[0].permute(0, 2, 3, 1).cpu(), want, "fp32", errs)
    same(new[1].permute(0, 2, 3, 1).cpu().view(want_codes.dtype), want_codes, "codes", errs)
    settle(errs)


@pytest.mark.parametrize("high", [False, True], ids=["bit31_clear", "bit31_set"])
def test_dw5_input_at_an_address_with_bit_31_of_its_low_half(high):
    """The zero-point-0 path addresses its taps through a buffer descriptor built from the two halves of the input pointer: the low half
    with bit 31 set must not leak into the high one.  A 2 GiB + 1 MiB allocation (never filled) holds 16-byte-aligned addresses of both
    kinds; the input is placed at one of each and the result compared with the generic kernel's, for a FAST 2 and a FAST 0 call."""
    from dlmc.quantization.scalar import kernels as K
    n, c, h, w = 2, 32, 6, 7
    room = torch.empty((1 << 31) + (1 << 20), dtype=torch.uint8, device=DEV)
    base = room.data_ptr()
    want_low = (1 << 31) if high else 0
    off = next(o for o in range(0, room.numel() - n * c * h * w, 1 << 20) if ((base + o) & 0xffffffff) & (1 << 31) == want_low)
    gen = torch.Generator().manual_seed(31 + high)
    x = room[off:off + n * h * w * c].view(n, h, w, c)
    x.copy_(torch.randint(0, 256, (n, h, w, c), generator=gen, dtype=torch.uint8).to(DEV))
    x = x.permute(0, 3, 1, 2)
    assert x.data_ptr() == base + off and bool(x.data_ptr() & (1 << 31)) == high and x.is_contiguous(memory_format=torch.channels_last)
    wq = torch.randint(-127, 128, (5, 5, c), generator=gen, dtype=torch.int8).to(DEV)
    ops = (x, wq, torch.randn(c, generator=gen).to(DEV), TG._t(0.05), TG._t(0.0), (torch.rand(c, generator=gen) * 0.01 + 0.001).to(DEV))
    emit = K.EmitCodes(TG._t(0.5), None, 0, 255, X.FORM_ZEROPOINT)
    for want_out in (False, True):
        new = K.conv2d_dw5_i8(*ops, stride=1, relu=True, emit=emit, want_out=want_out)
        old = K.conv2d_dw_i8(*ops, stride=1, padding=2, relu=True, emit=emit, want_out=want_out)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(new, old) if a is not None)


def test_every_dw5_record_is_launched():
    """From the route answers of the calls the cases above launched (run after them: pytest keeps a file's order)."""
    from dlmc import _native as N
    assert set(N.dw5_variant_table()) == set(W5.RECORDS)
    if LAUNCHED:          # (a run that selected this test alone launches nothing)
        assert LAUNCHED == set(W5.RECORDS), set(W5.RECORDS) - LAUNCHED


class MBConv5(nn.Module):
    """A first layer, then two MBConv blocks on 5x5 depthwise layers: 16 -> 96 channels at stride 1 with squeeze-excite and swish, 24 -> 144 at
    stride 2 with ReLU6."""
    reader = "none"

    def __init__(self):
        super().__init__()
        self.first = WL._conv_bn_act(8, 16, 3, act="swish")
        self.a = WL.InvertedResidual(16, 24, 1, 6, se=True, act="swish", k=5)
        self.b = WL.InvertedResidual(24, 32, 2, 6, se=False, act="relu6", k=5)
        self.head = nn.Conv2d(32, 64, 1)

    def forward(self, x):
        return self.head(self.b(self.a(self.first(x))))


@pytest.mark.parametrize("tag", ["fsptq", "qbase"])
def test_plan_with_dw5_equals_the_plan_without(tag):
    from dlmc.utils.fuse import DwInt8Layer, fuse_inference
    from dlmc.quantization.scalar import kernels as K
    cfg, qtype, kw = PLAN_CASES[tag]
    net, x = _net(MBConv5, 8, cfg, qtype, 71, False)
    x = x[:2, :, :24, :24].contiguous()
    off = fuse_inference(net, gates=True, swish=True, **kw)
    on = fuse_inference(net, gates=True, swish=True, dw5=True, **kw)
    ro, rn = off.fusion_report, on.fusion_report
    print(ro, rn, sep="\n")
    assert (ro.dw5, rn.dw5) == (0, 2) and rn.skipped == ro.skipped and rn.layers == ro.layers
    dws = [m for m in on.modules() if isinstance(m, DwInt8Layer)]
    assert [(m.k, m.k_pad, m.dw5) for m in dws] == [(96, 128, True), (144, 192, True)]
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        with torch.no_grad():
            b = on(x)
    finally:
        K.PROFILE.enabled = False
    assert [r[0] for r in K.PROFILE.records].count("conv_dw5") == 2
    K.PROFILE.reset()
    with torch.no_grad():
        a = off(x)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} logits differ"
