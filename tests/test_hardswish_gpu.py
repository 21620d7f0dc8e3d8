"""Hard swish on the GPU (include/dlmcq.h: dlmcq_hardswish_nhwc_f32; K.hardswish_quant; fuse_inference(hardswish=True)), both orders of
the two multiplies throughout.

Part A: exact - the codes are K.fake_quant of the kernel's OWN fp32 output, padded as _pad_channels pads; the codes-only and fp32-only
        calls return the same bits; guard bytes and unrequested buffers untouched.
Part B: against float64 - |v - v64| <= 5 * 2^-24 |v64| where 2^-100 <= |x| <= 2^100 and v64 != 0, and v == 0 where v64 == 0, with
        v64 = x * clip(x + 3, 0, 6) / 6 in float64 from the same fp32 input.  Four roundings of at most 2^-24 relative each (the add,
        two multiplies and the constant fl32(1 / 6)), the clamps exact: 4 * 2^-24 to first order, rounded up to 5 for the second-order
        terms.  torch's own results on the device pass the same assertion in the same test.
Part C: how many elements differ in their bits from each spelling of torch on the device, per order, printed and summed over the Part A
        inputs and the knees (DESIGN.md 5.30 records them).  MATCHES states what was measured: a named order pins torch.equal here and on
        the logits of Part E; None asserts Part B for the differing elements.
Part D: special values - +-0, +-inf, NaN, -3 and 3 and their neighbours, 1e30, FLT_MAX / 6 and its neighbours, FLT_MAX, denormals, the
        rounding ties of each quantiser behind the op - bit for bit against the matching torch spelling on the device.
Part E: whole plans - every net of tests/hardswish_nets.py and workloads.mobilenet_v3_small()."""
import ctypes
import functools
import struct

import pytest
import torch
import torch.nn.functional as F

from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from hardswish_nets import NETS as SPELLED_NETS
from test_gpu_gate import CODE_SENTINEL, DEV, PLAN_CASES, SENTINEL, _net, bits, quantisers, tagged
from test_swish_gpu import classes, own_codes, tie_quantisers

pytestmark = pytest.mark.gpu
ORDERS = {"mul_first": N.HSWISH_MUL_FIRST, "gate_first": N.HSWISH_GATE_FIRST}
BOUND = 5 * 2.0 ** -24
# spelling -> the order whose bits it has on an MI355X (Part C: 0 differing elements of the Part A inputs and the knees), or None where it
# matches neither.  The same table as hardswish_nets.NETS and DESIGN.md 5.30.
SPELLINGS = {"nn.Hardswish": lambda x: torch.nn.Hardswish()(x), "F.hardswish": F.hardswish,
             "x * relu6(x + 3) / 6": lambda x: x * F.relu6(x + 3) / 6, "(relu6(3 + x) * x) * (1 / 6)": lambda x: (F.relu6(3.0 + x) * x) * (1.0 / 6.0),
             "x * (relu6(x + 3) / 6)": lambda x: x * (F.relu6(x + 3) / 6), "(relu6(x + 3) / 6) * x": lambda x: (F.relu6(x + 3) / 6) * x,
             "x * F.hardsigmoid(x)": lambda x: x * F.hardsigmoid(x), "nn.Hardsigmoid()(x) * x": lambda x: torch.nn.Hardsigmoid()(x) * x}
MATCHES = {"nn.Hardswish": "mul_first", "F.hardswish": "mul_first", "x * relu6(x + 3) / 6": "mul_first",
           "(relu6(3 + x) * x) * (1 / 6)": "mul_first", "x * (relu6(x + 3) / 6)": "gate_first", "(relu6(x + 3) / 6) * x": "gate_first",
           "x * F.hardsigmoid(x)": "gate_first", "nn.Hardsigmoid()(x) * x": "gate_first"}


def test_the_tables_agree():
    assert sorted(MATCHES) == sorted(SPELLINGS) == sorted(SPELLED_NETS)
    for s, order in MATCHES.items():
        assert order is None or order == SPELLED_NETS[s][1], s       # a spelling that matches neither order keeps the table's


def raw(x, c, qz, want_out, want_codes, c_pad, order):
    """One call of the entry point on guarded buffers; `x`: (N, >= C, H, W) channels_last memory of which channels 0 .. c - 1 are read.
    Returns (out [N, H, W, C] or None, code bytes [N, H, W, c_pad] or None)."""
    n, xs, h, w = x.shape
    assert x.is_contiguous(memory_format=torch.channels_last) or (h == 1 and w == 1 and x.stride(1) == 1)
    no, nc = n * h * w * c, n * h * w * c_pad
    obuf = torch.full((no + 1024,), SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full((nc + 1024,), CODE_SENTINEL, dtype=torch.uint8, device=DEV)
    sc, z, lo, hi, form, gq, shifted, pad = qz
    rc = N.lib.dlmcq_hardswish_nhwc_f32(N.ptr(x), N.ptr(obuf) if want_out else None, N.ptr(cbuf) if want_codes else None, n, h, w, c, xs,
                                        c_pad, pad - (128 if shifted else 0), N.ptr(sc), N.ptr(z), lo, hi,
                                        form | (N.EMIT_SHIFT128 if shifted else 0), gq, ORDERS[order], N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((obuf[no:] == SENTINEL).all()) and bool((cbuf[nc:] == CODE_SENTINEL).all()), "guard bytes behind an output were written"
    if not want_out:
        assert bool((obuf == SENTINEL).all())
    if not want_codes:
        assert bool((cbuf == CODE_SENTINEL).all())
    return (obuf[:no].view(torch.float32).view(n, h, w, c) if want_out else None, cbuf[:nc].view(n, h, w, c_pad) if want_codes else None)


def part_a(x, c, c_pad, order, qs=None):
    """Every quantiser, the three calls; returns the kernel's fp32 output [N, H, W, C] (the same bits from every call)."""
    first = None
    for name, qz in (quantisers() if qs is None else qs).items():
        out, codes = raw(x, c, qz, True, True, c_pad, order)
        if first is None:
            first = out
            only_out, none = raw(x, c, qz, True, False, c, order)          # (the fp32-only call has no quantiser: once)
            assert none is None and torch.equal(bits(only_out), bits(first))
        assert torch.equal(bits(out), bits(first)), name
        want = own_codes(out, qz, c_pad)
        assert torch.equal(codes, want), f"{name}: {int((codes != want).sum())} code bytes differ from fake_quant of the kernel's own output"
        none, only = raw(x, c, qz, False, True, c_pad, order)
        assert none is None and torch.equal(only, codes), f"{name}: the codes-only call returns other bytes"
    return first


def part_b(x_rows, v_rows, what, where=None):
    """|v - v64| <= 5 * 2^-24 |v64| where 2^-100 <= |x| <= 2^100 and v64 != 0; v == 0 where v64 == 0.  Returns the largest error in
    units of 2^-24 |v64|.  `where`: the elements to look at (all)."""
    x64 = x_rows.double()
    v64 = x64 * torch.clamp(x64 + 3.0, 0.0, 6.0) / 6.0
    sel = torch.ones_like(x64, dtype=torch.bool) if where is None else where
    ok = (x64.abs() >= 2.0 ** -100) & (x64.abs() <= 2.0 ** 100) & (v64 != 0) & sel
    err = ((v_rows.double() - v64).abs() / v64.abs())[ok]
    worst = float(err.max()) / 2.0 ** -24 if err.numel() else 0.0
    print(f"{what}: max |v - v64| / |v64| = {worst:.3f} * 2^-24 over {int(ok.sum())} elements")
    assert worst * 2.0 ** -24 <= BOUND, what
    zero = (v64 == 0) & sel & ~torch.isnan(x64)
    assert bool((v_rows[zero] == 0).all()), f"{what}: a non-zero value where the real one is 0"
    return worst


def _next(v, up):
    return float(torch.nextafter(torch.tensor(v, dtype=torch.float32), torch.tensor(float("inf") if up else float("-inf"))))


KNEES = [3.0, _next(3.0, True), _next(3.0, False), -3.0, _next(-3.0, True), _next(-3.0, False), 6.0]
# N, H, W, C, x_stride, c_pad: pad threads only beside one data thread, twice; a channel slice read in place; 72 of 128; several workgroups
# with a ragged last one (3 * 9 * 11 * 16 = 4752 threads)
SHAPES = [(1, 1, 1, 4, 4, 4), (1, 1, 1, 4, 4, 64), (2, 3, 5, 12, 16, 64), (1, 7, 7, 72, 72, 128), (3, 9, 11, 40, 40, 64)]
IDS = ["x".join(map(str, s)) for s in SHAPES]


@functools.lru_cache(maxsize=None)
def case(shape):
    """(the tensor handed to the kernel, its dense input as [N, H, W, C] rows, {spelling: torch's result on the device as such rows}) for
    one shape: made once, shared by the tests, never written.  The knees stand at the front of the data where they fit."""
    n, h, w, c, xs, c_pad = shape
    g = torch.Generator().manual_seed(sum(shape))
    rows = torch.randn(n, h, w, c, generator=g) * 3
    flat = rows.view(-1)
    k = min(len(KNEES), flat.numel() - 1)
    flat[1:1 + k] = torch.tensor(KNEES[:k])
    full = torch.full((n, h, w, xs), float("nan"))          # (a stride error reads NaN)
    full[..., :c] = rows
    given = full.to(DEV).permute(0, 3, 1, 2)                 # (N, xs, H, W), channels_last memory
    dense = given[:, :c].permute(0, 2, 3, 1).contiguous()
    return given, dense, {s: fn(dense) for s, fn in SPELLINGS.items()}


COUNTS = {}


def count(shape, order, v, torch_rows):
    COUNTS[shape, order] = {s: int((bits(v) != bits(t)).sum()) for s, t in torch_rows.items()}, v.numel()


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kernel(shape, order):
    given, dense, torch_rows = case(shape)
    n, h, w, c, xs, c_pad = shape
    v = part_a(given, c, c_pad, order)
    part_b(dense, v, f"kernel, {order}")
    for s, t in torch_rows.items():
        part_b(dense, t, f"torch {s}")                   # the bound is not vacuous against the paths being replaced
    count(shape, order, v, torch_rows)
    print(f"{order}: bits differ from torch in {COUNTS[shape, order][0]} of {v.numel()}")
    for s, t in torch_rows.items():
        if MATCHES[s] == order:
            assert torch.equal(bits(v), bits(t)), f"{s}: {COUNTS[shape, order][0][s]} of {v.numel()} elements differ from the {order} kernel"
        elif MATCHES[s] is None and SPELLED_NETS[s][1] == order:
            part_b(dense, v, f"{order} where {s} differs", bits(v) != bits(t))


def kernel_rows(shape, order):
    """K.hardswish_quant's fp32 output for the shape's dense input, as [N, H, W, C] rows."""
    return K.hardswish_quant(case(shape)[1].permute(0, 3, 1, 2), order)[0].permute(0, 2, 3, 1)


def test_part_c_totals():
    for shape in SHAPES:
        for order in ORDERS:
            if (shape, order) not in COUNTS:
                count(shape, order, kernel_rows(shape, order), case(shape)[2])
    total = sum(c[1] for (s, o), c in COUNTS.items() if o == "mul_first")
    for s in SPELLINGS:
        differ = {o: sum(c[0][s] for (sh, oo), c in COUNTS.items() if oo == o) for o in ORDERS}
        print(f"PART C: {s}: of {total} elements {differ['mul_first']} differ in their bits from mul_first, {differ['gate_first']} from gate_first")
        measured = [o for o in sorted(ORDERS) if differ[o] == 0]
        assert measured == ([MATCHES[s]] if MATCHES[s] else []), f"MATCHES no longer states what the device does for {s}: bit-identical to {measured}"
    both = sum(int((bits(kernel_rows(sh, "mul_first")) != bits(kernel_rows(sh, "gate_first"))).sum()) for sh in SHAPES)
    print(f"PART C: the two orders differ from each other in {both} of {total} elements")
    assert both > 0


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("shape", SHAPES[2:], ids=IDS[2:])
def test_wrapper(shape, order):
    """K.hardswish_quant: shapes, layouts and dtypes of what it returns; an NCHW input is copied, a channel slice read in place."""
    given, dense, torch_rows = case(shape)
    n, h, w, c, xs, c_pad = shape
    x = given[:, :c]
    copies = []
    real = K._nhwc
    K._nhwc = lambda t: copies.append(t) or real(t)        # the wrapper's only way to a copy
    try:
        (out, none), tags = tagged(lambda: K.hardswish_quant(x, order))
    finally:
        K._nhwc = real
    assert tags == ["hardswish"] and not copies and none is None and tuple(out.shape) == (n, c, h, w)
    assert out.is_contiguous(memory_format=torch.channels_last)
    ref = part_a(given, c, c_pad, order, {"fsptq_zeropoint_u8": quantisers()["fsptq_zeropoint_u8"]})
    assert torch.equal(bits(out.permute(0, 2, 3, 1)), bits(ref))
    assert torch.equal(bits(K.hardswish_quant(x.contiguous(), order)[0]), bits(out))              # NCHW-contiguous: copied to channels_last
    for name, qz in quantisers().items():
        sc, z, lo, hi, form, gq, shifted, pad = qz
        em = K.EmitCodes(sc, z, lo, hi, form, gq, shift128=shifted)
        o2, codes = K.hardswish_quant(x, order, emit=em, c_pad=c_pad, pad_code=pad - (128 if shifted else 0))
        assert codes.dtype == em.dtype and tuple(codes.shape) == (n, c_pad, h, w) and codes.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(bits(o2), bits(out))
        assert torch.equal(codes.view(torch.uint8).permute(0, 2, 3, 1), own_codes(ref, qz, c_pad)), name
        none, only = K.hardswish_quant(x, order, emit=em, want_out=False, c_pad=c_pad, pad_code=pad - (128 if shifted else 0))
        assert none is None and torch.equal(only, codes)
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        K.hardswish_quant(x, order, emit=em, c_pad=c_pad)
        (rec,) = K.PROFILE.records
    finally:
        K.PROFILE.enabled = False
        K.PROFILE.reset()
    assert rec[0] == "hardswish" and rec[1] == n * h * w * (c * 4 + c * 4 + c_pad)          # read, fp32 written, codes written
    with pytest.raises(ValueError):
        K.hardswish_quant(x, "division")
    with pytest.raises(ValueError):
        K.hardswish_quant(x, order, want_out=False)
    with pytest.raises(ValueError):
        K.hardswish_quant(x, order, c_pad=c_pad + 4)
    with pytest.raises(ValueError):
        K.hardswish_quant(x[0], order)
    with pytest.raises(ValueError):
        K.hardswish_quant(x.double(), order)
    with pytest.raises(N.DlmcqError, match="no CPU fallback"):
        K.hardswish_quant(x.cpu(), order)


# ------------------------------------------------------------------------------------------------------------------ part D
FLT_MAX = struct.unpack("f", struct.pack("I", 0x7f7fffff))[0]
SIXTH_OF_MAX = float(torch.tensor(FLT_MAX, dtype=torch.float32) / 6)


def special_inputs():
    gen = torch.Generator().manual_seed(5)
    n, c, h, w = 3, 68, 3, 3
    out = {}
    x = torch.randn(n, c, h, w, generator=gen) * 3
    x[:, ::2] = -0.0
    x[0, 1] = 0.0
    out["zeros"] = x
    x = torch.randn(n, c, h, w, generator=gen) * 3
    x[0, 9, 2, 1], x[1, 11, 0, 0], x[2, 13], x[0, 3, 0, 0], x[1, 5] = float("inf"), float("-inf"), float("inf"), float("nan"), float("-inf")
    x[2, 20] = float("nan")
    out["inf_nan"] = x
    x = torch.randn(n, c, h, w, generator=gen) * 3
    knees = []
    for k in (-3.0, 3.0):
        lo = hi = k
        knees.append(k)
        for _ in range(3):
            lo, hi = _next(lo, False), _next(hi, True)
            knees += [lo, hi]
    x.view(-1)[:len(knees)] = torch.tensor(knees)
    x[1] = -3.0 - torch.rand(c, h, w, generator=gen) * 100            # x <= -3: r = 0, v = -0
    x[2, :8] = 3.0 + torch.rand(8, h, w, generator=gen) * 100         # x >= 3: (x * 6) * c or x * (6 * c)
    out["knees"] = x
    x = torch.rand(n, c, h, w, generator=gen) * 3e38
    big = [1e30, SIXTH_OF_MAX, FLT_MAX]
    lo = hi = SIXTH_OF_MAX
    for _ in range(4):
        lo, hi = _next(lo, False), _next(hi, True)
        big += [lo, hi]
    x.view(-1)[:len(big)] = torch.tensor(big)
    x[1] = -x[1]
    out["large"] = x
    x = torch.randn(n, c, h, w, generator=gen) * 1e-39                     # denormal inputs: v = x / 2 rounded twice, denormal too
    x[1] = torch.randn(c, h, w, generator=gen) * 1e-44
    out["denormals"] = x
    return out


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("name", ["zeros", "inf_nan", "knees", "large", "denormals"])
def test_special_values(name, order):
    x = special_inputs()[name].to(DEV).contiguous(memory_format=torch.channels_last)
    v = part_a(x, 68, 128, order)                                           # codes == fake_quant of the kernel's own output, NaN included
    dense = x.permute(0, 2, 3, 1).contiguous()
    differ = {}
    for s, fn in SPELLINGS.items():
        if SPELLED_NETS[s][1] != order:
            continue
        ref = fn(dense)
        assert torch.equal(torch.isnan(v), torch.isnan(ref)), f"{s}: NaN positions"
        ok = ~torch.isnan(ref)
        assert torch.equal(classes(v)[:, ok], classes(ref)[:, ok]), f"{s}: class (inf / zero / finite) and sign against torch on the device"
        differ[s] = int((bits(v) != bits(ref))[ok].sum())
        if MATCHES[s] == order:
            assert torch.equal(bits(v)[ok], bits(ref)[ok]), f"{s}: {differ[s]} elements differ"
    print(name, order, "bits differ from torch in", differ, "of", v.numel())
    xs, vs = dense.flatten(), v.flatten()
    if name == "zeros":
        assert bool((bits(vs[bits(xs) == bits(torch.tensor(-0.0))]) == bits(torch.tensor(-0.0, device=DEV))).all())       # -0 -> -0
        assert bool((bits(vs[bits(xs) == 0]) == 0).all())                                                                   # +0 -> +0
    if name == "inf_nan":
        assert bool(torch.isnan(vs[xs == float("-inf")]).all()) and bool((vs[xs == float("inf")] == float("inf")).all())
        assert bool(torch.isnan(vs[torch.isnan(xs)]).all())
    if name == "knees":
        low = xs <= -3.0
        assert bool(low.any()) and bool((bits(vs[low]) == bits(torch.tensor(-0.0, device=DEV))).all()), "x <= -3: v = -0"
        assert bool((vs[(xs > -3.0) & (xs < 0)] < 0).all()) and bool((vs[xs > 0] > 0).all())
    if name == "large":
        over = xs > SIXTH_OF_MAX
        assert bool(over.any()) and bool((xs[~over & (xs > 0)] > 1e29).any())
        if order == "mul_first":
            assert bool((vs[over] == float("inf")).all()) and bool(torch.isfinite(vs[(xs > 0) & (xs < SIXTH_OF_MAX)]).all())
        else:
            assert bool(torch.isfinite(vs[xs > 0]).all()), "x * (6 * c) does not overflow"
        assert bool((bits(vs[xs < -3.0]) == bits(torch.tensor(-0.0, device=DEV))).all())
    if name == "denormals":
        assert bool(((v != 0) & (v.abs() < 2.0 ** -126)).any())             # (not flushed)


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_ties_round_half_to_even(order):
    """test_swish_gpu.py's tie quantisers (the dyadic scale 0.25) behind inputs the op returns unchanged: x = (k + 0.5) / 4 from 3.125
    on, so that r = 6.  fl32(1 / 6) = (2^26 + 2) / (6 * 2^26), hence 6 * c = 1 + 2^-25: under gate_first fl32(6 * c) = 1 and v = x; under
    mul_first x * 6 is exact (x has 11 significant bits at most) and (x * 6) * c = x + x * 2^-25, less than half an ulp above x, is
    rounded to x.  So v / s lands on the tie k + 0.5 (less an integer zero point; the float offset 0.125 moves it off - and 2.125 onto
    the next one)."""
    k = torch.arange(12, 268, dtype=torch.float32).reshape(1, 16, 4, 4)      # x = 3.125 .. 66.875
    x = ((k + 0.5) * 0.25).to(DEV).contiguous(memory_format=torch.channels_last)
    kk = k.permute(0, 2, 3, 1).to(DEV)
    for name, qz in tie_quantisers().items():
        out, codes = raw(x, 16, qz, True, True, 16, order)
        assert torch.equal(out, x.permute(0, 2, 3, 1)), "v = x from x = 3 on, for inputs of few bits"
        assert torch.equal(codes, own_codes(out, qz, 16)), name
        if name == "plain_u8":                                                 # code = clamp(R(k + 0.5)): half to even (torch.round)
            assert torch.equal(codes, torch.clamp(torch.round(kk + 0.5), 0, 255).to(torch.uint8))


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_leaves_the_outputs_untouched():
    x = torch.zeros(2, 16, 8, 8, device=DEV).contiguous(memory_format=torch.channels_last)
    obuf = torch.full((4096,), SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full((16384,), CODE_SENTINEL, dtype=torch.uint8, device=DEV)
    sc = torch.tensor([0.01], device=DEV)
    base = dict(x=x.data_ptr(), out=obuf.data_ptr(), codes=cbuf.data_ptr(), n=2, h=8, w=8, c=16, xs=16, c_pad=16, pad_code=0,
                scale=sc.data_ptr(), lo=0, hi=255, form=N.FORM_ZEROPOINT, order=0)
    cases = {
        "order -1": (dict(order=-1), -1), "order 2": (dict(order=2), -1), "order 2 and N == 0": (dict(order=2, n=0), -1),
        "H < 1": (dict(h=0), -1), "C % 4": (dict(c=6), -1), "x_stride < C": (dict(xs=12), -1), "c_pad % 4": (dict(c_pad=18), -1),
        "pad_code 256": (dict(pad_code=256), -1), "both outputs NULL": (dict(out=None, codes=None), -1),
        "c_pad != C without codes": (dict(codes=None, c_pad=64), -1), "x NULL": (dict(x=None), -1),
        "codes without a scale": (dict(scale=None), -1), "lo > hi": (dict(lo=9, hi=3), -1), "unknown form": (dict(form=9), -1),
        "FORCE_TILED": (dict(form=N.FORM_ZEROPOINT | N.FORCE_TILED), -1),
        "x not 16-byte aligned": (dict(x=x.data_ptr() + 4), -4), "out not 16-byte aligned": (dict(out=obuf.data_ptr() + 8), -4),
        "codes not 4-byte aligned": (dict(codes=cbuf.data_ptr() + 2), -4),
        "an index past 2^31": (dict(n=1 << 31, h=1, w=1, c=4, xs=4, c_pad=4), -2),
    }
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731

    def call(a):
        return N.lib.dlmcq_hardswish_nhwc_f32(p(a["x"]), p(a["out"]), p(a["codes"]), a["n"], a["h"], a["w"], a["c"], a["xs"], a["c_pad"],
                                              a["pad_code"], p(a["scale"]), None, a["lo"], a["hi"], a["form"], 0.0, a["order"], N.stream_ptr())
    for order in (0, 1):
        for what, (kw, rc) in cases.items():
            assert call({**base, "order": order, **kw}) == rc, what
        assert call(dict(base, order=order, n=0)) == 0                         # N == 0: nothing to do
    torch.cuda.synchronize()
    assert bool((obuf == SENTINEL).all()) and bool((cbuf == CODE_SENTINEL).all())
    with pytest.raises(N.DlmcqError):
        K.hardswish_quant(torch.zeros(2, 6, 4, 4, device=DEV))                 # C % 4, through the wrapper


@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("shifted", [False, True])
def test_an_input_that_is_no_map_takes_the_torch_path(shifted, order):
    from dlmc.utils.fuse import HardswishLayer, _ActSpec
    given, dense, torch_rows = case(SHAPES[2])                                 # (2, 12, 3, 5) of 16, code rows 64 wide
    given = given[:, :12]
    spec = _ActSpec(torch.tensor([0.01], device=DEV), torch.tensor([4.0], device=DEV), 0, 255, N.FORM_ZEROPOINT, False)
    node = HardswishLayer(spec, True, 12, 64, 4 - (128 if shifted else 0), shifted, order=order)
    restated = SPELLINGS["nn.Hardswish" if order == "mul_first" else "x * F.hardsigmoid(x)"]
    qz = (spec.scale, spec.zp, 0, 255, N.FORM_ZEROPOINT, 0.0, shifted, 4)
    (out, codes), tags = tagged(lambda: node(given))
    assert tags == ["hardswish"] and codes.dtype == (torch.int8 if shifted else torch.uint8) and tuple(codes.shape) == (2, 64, 3, 5)
    assert torch.equal(codes.view(torch.uint8).permute(0, 2, 3, 1), own_codes(out.permute(0, 2, 3, 1), qz, 64))
    vec = given[:, :, 0, 0].contiguous()                                       # a 2-D input: (N, 12)
    (out, codes), tags = tagged(lambda: node(vec))
    assert "hardswish" not in tags and tuple(out.shape) == (2, 12) and torch.equal(bits(out), bits(restated(vec)))
    want = K.fake_quant(out, spec.scale, spec.zp, 0, 255, N.FORM_ZEROPOINT, codes="i8", want_y=False)[1].view(torch.uint8) ^ (0x80 if shifted else 0)
    assert codes.dtype == (torch.int8 if shifted else torch.uint8) and torch.equal(codes.view(torch.uint8), want)
    other = torch.randn(2, 20, 4, 4, device=DEV)                               # a map of another width than the plan's
    (out, codes), tags = tagged(lambda: node(other))
    assert "hardswish" not in tags and torch.equal(bits(out), bits(restated(other))) and tuple(codes.shape) == (2, 64, 4, 4)
    plain = HardswishLayer(None, True, None, None, 0, order=order)             # nobody takes codes
    (out, codes), tags = tagged(lambda: plain(given))
    assert tags == ["hardswish"] and codes is None
    assert torch.equal(bits(out.permute(0, 2, 3, 1)), bits(K.hardswish_quant(given, order)[0].permute(0, 2, 3, 1)))
    (out, codes), tags = tagged(lambda: plain(vec))
    assert not tags and codes is None and torch.equal(bits(out), bits(restated(vec)))


# ------------------------------------------------------------------------------------------------------------------ part E
from test_hardswish_host import COUNTS as PINNED      # noqa: E402  (hard swishes on maps per network, as the host test pins them)


def _v3_small():
    import workloads as W
    return W.mobilenet_v3_small()


# name -> (the network, its input shape, hard swishes on maps, gates, the spelling whose MATCHES entry decides the flag-off comparison)
PLAN_NETS = dict({s: (make, (2, 8, 9, 9), PINNED["small_net"][0], 1, s) for s, (make, _) in SPELLED_NETS.items()},
                 mobilenet_v3_small=(_v3_small, (2, 3, 64, 64), PINNED["mobilenet_v3_small"][0], 9, "nn.Hardswish"))
PLANS = [(tag, name) for name in sorted(PLAN_NETS) for tag in ("fsptq", "qbase")]


@pytest.mark.parametrize("tag, name", PLANS)
def test_plans(tag, name):
    from dlmc.utils.fuse import GateLayer, HardswishLayer, fuse_inference
    make, shape, n_hs, n_gates, spelling = PLAN_NETS[name]
    cfg, qtype, kw = PLAN_CASES[tag]
    net, _ = _net(make, shape[1], cfg, qtype, 71, False)
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    x = torch.relu(x) if shape[1] == 3 else x
    off = fuse_inference(net, gates=True, dw5=True, **kw)
    on = fuse_inference(net, gates=True, dw5=True, hardswish=True, **kw)
    ro, rn = off.fusion_report, on.fusion_report
    print(ro, rn, sep="\n")
    assert (ro.hardswishes, rn.hardswishes) == (0, n_hs) and ro.gates == rn.gates == n_gates and rn.skipped == ro.skipped
    assert (rn.layers, rn.residual, rn.relu, rn.relu6, rn.emit, rn.fp32_outputs, rn.narrow, rn.dual, rn.act_offset, rn.dw5) == \
           (ro.layers, ro.residual, ro.relu, ro.relu6, ro.emit, ro.fp32_outputs, ro.narrow, ro.dual, ro.act_offset, ro.dw5)
    nodes = {n_: m for n_, m in on.named_modules() if isinstance(m, HardswishLayer)}
    assert len(nodes) == n_hs and sum(isinstance(m, GateLayer) for m in on.modules()) == n_gates
    assert {m.order for m in nodes.values()} == {SPELLED_NETS[spelling][1]}
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, a, r, n_=n_: seen.__setitem__(n_, (a[0], r))) for n_, m in nodes.items()]
    with torch.no_grad():
        (a, _), (b, tags) = tagged(lambda: off(x)), tagged(lambda: on(x))
        for h in hooks:
            h.remove()
        again = on(x)
        for m in nodes.values():                       # every hard-swish node through its torch path: the spelling that was matched
            m.forward = m._unfused
        unfused, tags_unfused = tagged(lambda: on(x))
        for m in nodes.values():
            del m.forward
    assert tags.count("hardswish") == n_hs and tags.count("gate") == n_gates and "hardswish" not in tagged(lambda: off(x))[1]
    assert "hardswish" not in tags_unfused and tags_unfused.count("gate") == n_gates
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()) and torch.equal(b, again)
    # Parts A and B at the network's own shapes, on what every node was given and gave back
    assert sorted(seen) == sorted(nodes)
    worst = 0.0
    for n_, (t, (out, codes)) in seen.items():
        m = nodes[n_]
        assert t.dim() == 4 and (out is not None) == m.want_out and (codes is not None) == (m.emit is not None)
        own = K.hardswish_quant(t, m.order)[0]
        if out is not None:
            assert torch.equal(bits(out.permute(0, 2, 3, 1)), bits(own.permute(0, 2, 3, 1))), n_
        rows = own.permute(0, 2, 3, 1)
        worst = max(worst, part_b(t.permute(0, 2, 3, 1), rows, n_))
        if codes is not None:
            e = m.emit
            qz = (e.scale, e.zp, e.lo, e.hi, e.form, e.g(t.numel()), m.emit_shift, m.pad_code + (128 if m.emit_shift else 0))
            assert tuple(codes.shape) == (t.shape[0], m.c_pad) + tuple(t.shape[2:])
            assert torch.equal(codes.view(torch.uint8).permute(0, 2, 3, 1), own_codes(rows, qz, m.c_pad)), n_
    dev = float((a - b).abs().max())
    print(f"{tag} / {name}: max |logit(hardswish=True) - logit(hardswish=False)| = {dev:.3e}, {int((a != b).sum())} of {a.numel()} logits differ, "
          f"{int((unfused != b).sum())} from the nodes' torch path, worst Part B error {worst:.3f} * 2^-24")
    assert torch.equal(b, unfused), f"{int((unfused != b).sum())} of {b.numel()} logits differ from the plan with every node on its torch path"
    if MATCHES[spelling] is not None:
        assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} logits differ, max {dev}"
