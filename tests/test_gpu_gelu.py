"""GELU (erf form) on the GPU (include/dlmcq.h: dlmcq_gelu_nhwc_f32; K.gelu_quant), modelled on test_swish_gpu.py.

Part A: exact - the codes are K.fake_quant of the kernel's OWN fp32 output, padded as _pad_channels pads; the codes-only call returns the
        same bytes; guard bytes and unrequested buffers untouched.  Maps and rows, with and without c_pad > C, a channel slice in place.
Part B: against float64 - with v* = 0.5 x (1 + erf(x / sqrt(2))) (evaluated as 0.5 x erfc(-x / sqrt(2)): the same function without the
        cancellation of 1 + erf in the negative tail) from the same fp32 input and u = 2^-23 (|x| + |v*|):  |v - v*| <= 2 u.  erff is
        within 2 ulp by the device library's documentation, which puts at most about 2^-22 absolute on f = 1 + erff(z); |x| / 2 scales
        that to 2^-23 |x|; the two multiplies add 2^-23 |v*|; the factor 2 covers second order (csrc/gelu.hip).  The same five steps in
        torch fp32 on the CPU stay within 0.46 u.  The device's maximum is printed (DESIGN.md 5.23 records it).  u's terms are relative
        roundings, which fp32 has in its normal range only: the denormal inputs of Part D are those at which an fp32 result within
        2 u exists (special_inputs).
Part C: how many elements differ in their bits from F.gelu(x) on the device, printed; MATCHES_TORCH_GELU states what was measured: True
        pins torch.equal, False asserts that the count is not 0 and that every differing element satisfies Part B.
Part D: special values - their class (NaN / inf / zero with its sign / finite) is that of the five steps in torch ops on the device."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import GeluLayer
from test_gpu_gate import CODE_SENTINEL, DEV, SENTINEL, bits, quantisers, tagged
from test_swish_gpu import classes, own_codes

pytestmark = pytest.mark.gpu
MATCHES_TORCH_GELU = True      # Part C's count, as measured on an MI355X: 0 of the elements of the Part A inputs and the sweep
WORST = {}


def raw(x, c, qz, want_out, want_codes, c_pad):
    """One call of the entry point on guarded buffers; `x`: (N, >= C, H, W) channels_last memory of which channels 0 .. c - 1 are read.
    Returns (out [N, H, W, C] or None, code bytes [N, H, W, c_pad] or None)."""
    n, xs, h, w = x.shape
    assert x.is_contiguous(memory_format=torch.channels_last)
    no, nc = n * h * w * c, n * h * w * c_pad
    obuf = torch.full((no + 1024,), SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full((nc + 1024,), CODE_SENTINEL, dtype=torch.uint8, device=DEV)
    sc, z, lo, hi, form, gq, shifted, pad = qz
    rc = N.lib.dlmcq_gelu_nhwc_f32(N.ptr(x), N.ptr(obuf) if want_out else None, N.ptr(cbuf) if want_codes else None, n, h, w, c, xs, c_pad,
                                   pad - (128 if shifted else 0), N.ptr(sc), N.ptr(z), lo, hi, form | (N.EMIT_SHIFT128 if shifted else 0), gq,
                                   N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((obuf[no:] == SENTINEL).all()) and bool((cbuf[nc:] == CODE_SENTINEL).all()), "guard bytes behind an output were written"
    if not want_out:
        assert bool((obuf == SENTINEL).all())
    if not want_codes:
        assert bool((cbuf == CODE_SENTINEL).all())
    return (obuf[:no].view(torch.float32).view(n, h, w, c) if want_out else None, cbuf[:nc].view(n, h, w, c_pad) if want_codes else None)


def part_a(x, c, c_pad, names=None):
    """Every quantiser, the three calls; returns the kernel's fp32 output [N, H, W, C] (the same bits from every call)."""
    first = None
    for name, qz in quantisers().items():
        if names is not None and name not in names:
            continue
        out, codes = raw(x, c, qz, True, True, c_pad)
        if first is None:
            first = out
            only_out, none = raw(x, c, qz, True, False, c)
            assert none is None and torch.equal(bits(only_out), bits(first))
        assert torch.equal(bits(out), bits(first)), name
        want = own_codes(out, qz, c_pad)
        assert torch.equal(codes, want), f"{name}: {int((codes != want).sum())} code bytes differ from fake_quant of the kernel's own output"
        assert c_pad == c or bool((codes[..., c:] == ((qz[7] - (128 if qz[6] else 0)) & 0xff)).all()), "pad channels hold pad_code"
        none, only = raw(x, c, qz, False, True, c_pad)
        assert none is None and torch.equal(only, codes), f"{name}: the codes-only call returns other bytes"
    return first


def part_b(x, v, what):
    """|v - v*| <= 2 u over the finite inputs; returns the largest |v - v*| / u."""
    x64 = x.double()
    ok = torch.isfinite(x64)
    v64 = 0.5 * x64 * torch.special.erfc(-x64 / math.sqrt(2.0))
    u = 2.0 ** -23 * (x64.abs() + v64.abs())
    err = (v.double() - v64).abs()
    ratio = float((err / u.clamp_min(1e-320))[ok & (u > 0)].max()) if bool((ok & (u > 0)).any()) else 0.0
    WORST[what] = max(WORST.get(what, 0.0), ratio)
    print(f"{what}: max |v - v*| / u = {ratio:.3f} over {int(ok.sum())} elements")
    assert bool((err[ok] <= 2 * u[ok]).all()), f"{what}: {ratio:.3f} u"
    return ratio


def five_steps(x):
    return GeluLayer._gelu(x)


# N, C, H, W, c_pad (, x_stride): a single quad; odd sides; C % 64 != 0 past one chunk with several workgroups, plain and padded; rows
# [17, 128] and [3 * 17, 128] as N = rows, H = W = 1; a channel slice read in place
SHAPES = [(1, 4, 1, 1, 4), (2, 8, 3, 5, 8), (2, 8, 3, 5, 64), (1, 260, 7, 7, 260), (1, 260, 7, 7, 320), (17, 128, 1, 1, 128), (51, 128, 1, 1, 128),
          (2, 24, 6, 6, 64, 64)]
IDS = ["x".join(map(str, s)) for s in SHAPES[:-1]] + ["slice_24_of_64"]


@functools.lru_cache(maxsize=None)
def case(shape):
    """(the tensor handed to the kernel, its dense input as [N, H, W, C] rows, the five steps and F.gelu on the device as such rows)."""
    n, c, h, w, c_pad = shape[:5]
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(n, c, h, w, generator=g) * 3
    if len(shape) == 6:
        full = torch.full((n, shape[5], h, w), float("nan"))          # (a stride error reads NaN)
        full[:, :c] = x
        given = full.to(DEV).contiguous(memory_format=torch.channels_last)
    else:
        given = x.to(DEV).contiguous(memory_format=torch.channels_last)
    dense = given[:, :c].permute(0, 2, 3, 1).contiguous()
    return given, dense, five_steps(dense), F.gelu(dense)


COUNTS = {}


def count(key, v, ref):
    d = bits(v) != bits(ref)
    COUNTS[key] = (int(d.sum()), v.numel())
    return d


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kernel(shape):
    given, dense, steps, gelu = case(shape)
    c, c_pad = shape[1], shape[4]
    v = part_a(given, c, c_pad)
    part_b(dense, v, "kernel")
    part_b(dense, gelu, "F.gelu on the device")           # the bound is not vacuous against the path being replaced
    d = count(shape, v, gelu)
    print(f"bits differ from F.gelu(x): {COUNTS[shape][0]} of {v.numel()}; from the five steps in torch ops: {int((bits(v) != bits(steps)).sum())}")
    if MATCHES_TORCH_GELU:
        assert torch.equal(v, gelu)
    elif bool(d.any()):
        part_b(dense[d], v[d], "kernel where it differs from F.gelu")


def test_sweep_against_float64():
    x = torch.linspace(-12, 12, 64 * 1024 + 4).to(DEV)[:64 * 1024].view(512, 128, 1, 1).contiguous(memory_format=torch.channels_last)
    v = raw(x, 128, quantisers()["fsptq_zeropoint_u8"], True, True, 128)[0]
    dense = x.permute(0, 2, 3, 1)
    part_b(dense, v, "kernel")
    count("sweep", v, F.gelu(dense))
    print(f"sweep of [-12, 12]: bits differ from F.gelu(x) in {COUNTS['sweep'][0]} of {v.numel()}")
    deep = dense <= -6.0
    assert bool((v[deep] == 0).all()) and bool((bits(v[deep]) < 0).all()), "x <= about -5.9 (here: -6): e = -1, f = 0, v = -0"


def test_part_c_totals():
    for shape in SHAPES:
        if shape not in COUNTS:
            given, dense, steps, gelu = case(shape)
            count(shape, raw(given, shape[1], quantisers()["fsptq_zeropoint_u8"], True, False, shape[1])[0], gelu)
    tot = [sum(c[i] for c in COUNTS.values()) for i in range(2)]
    print(f"PART C: of {tot[1]} elements {tot[0]} differ in their bits from F.gelu(x) on the device; "
          f"PART B: largest |v - v*| / u = {WORST.get('kernel', float('nan')):.3f} (F.gelu: {WORST.get('F.gelu on the device', float('nan')):.3f})")
    assert (tot[0] == 0) == MATCHES_TORCH_GELU, "MATCHES_TORCH_GELU no longer states what the device does"


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[4], SHAPES[-1]], ids=["2x8x3x5_pad64", "1x260x7x7_pad320", "slice_24_of_64"])
def test_wrapper_on_maps(shape):
    given, dense, steps, gelu = case(shape)
    n, c, h, w, c_pad = shape[:5]
    x = given[:, :c]
    (out, none), tags = tagged(lambda: K.gelu_quant(x))
    assert tags == ["gelu"] and none is None and tuple(out.shape) == (n, c, h, w) and out.is_contiguous(memory_format=torch.channels_last)
    ref = part_a(given, c, c_pad, names=("fsptq_zeropoint_u8",))
    assert torch.equal(bits(out.permute(0, 2, 3, 1)), bits(ref))
    for name, qz in quantisers().items():
        sc, z, lo, hi, form, gq, shifted, pad = qz
        em = K.EmitCodes(sc, z, lo, hi, form, gq, shift128=shifted)
        o2, codes = K.gelu_quant(x, emit=em, c_pad=c_pad, pad_code=pad - (128 if shifted else 0))
        assert codes.dtype == em.dtype and tuple(codes.shape) == (n, c_pad, h, w) and torch.equal(o2, out)
        assert torch.equal(codes.view(torch.uint8).permute(0, 2, 3, 1), own_codes(ref, qz, c_pad)), name
        none, only = K.gelu_quant(x, emit=em, want_out=False, c_pad=c_pad, pad_code=pad - (128 if shifted else 0))
        assert none is None and torch.equal(only, codes)


@pytest.mark.parametrize("lead", [(17,), (3, 17)], ids=["17x128", "3x17x128"])
def test_wrapper_on_rows(lead):
    g = torch.Generator().manual_seed(len(lead))
    x = (torch.randn(*lead, 128, generator=g) * 3).to(DEV)
    m = x.numel() // 128
    as_map = x.reshape(m, 128, 1, 1).contiguous(memory_format=torch.channels_last)
    ref = part_a(as_map, 128, 128, names=("fsptq_zeropoint_u8",)).view(*lead, 128)
    (out, none), tags = tagged(lambda: K.gelu_quant(x))
    assert tags == ["gelu"] and none is None and tuple(out.shape) == tuple(x.shape) and torch.equal(bits(out), bits(ref))
    part_b(x, out, "kernel")
    for name, qz in quantisers().items():
        sc, z, lo, hi, form, gq, shifted, pad = qz
        em = K.EmitCodes(sc, z, lo, hi, form, gq, shift128=shifted)
        for c_pad in (128, 192):
            o2, codes = K.gelu_quant(x, emit=em, c_pad=c_pad, pad_code=pad - (128 if shifted else 0))
            assert codes.dtype == em.dtype and tuple(codes.shape) == lead + (c_pad,) and torch.equal(o2, out)
            want = own_codes(ref.view(m, 1, 1, 128), qz, c_pad).view(*lead, c_pad)
            assert torch.equal(codes.view(torch.uint8), want), name
    assert torch.equal(K.gelu_quant(x.transpose(0, -1).contiguous().transpose(0, -1))[0], out)      # strided rows: copied
    with pytest.raises(ValueError):
        K.gelu_quant(x, want_out=False)
    with pytest.raises(ValueError):
        K.gelu_quant(x, c_pad=192)
    with pytest.raises(ValueError):
        K.gelu_quant(x.double())
    with pytest.raises(N.DlmcqError):
        K.gelu_quant(torch.zeros(3, 6, device=DEV))                               # C % 4
    with pytest.raises(N.DlmcqError, match="no CPU fallback"):
        K.gelu_quant(x.cpu())


# ------------------------------------------------------------------------------------------------------------------ part D
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
    x = -torch.rand(n, c, h, w, generator=gen) * 104 - 6                   # -6 .. -110: erff(z) = -1, f = 0, v = -0
    x[0, 0, 0, 0], x[0, 1, 0, 0], x[0, 2, 0, 0], x[0, 3, 0, 0] = -5.5, -5.8, -5.9, -6.0
    out["deep_negative"] = x
    x = torch.rand(n, c, h, w, generator=gen) * 3e38
    x[0, 0, 0, 0] = 3e38
    out["large_positive"] = x
    # denormal inputs: v = x / 2, denormal too.  u is relative to |x|, fp32's spacing down here is not: for an odd multiple of 2^-149 the
    # two fp32 neighbours of x / 2 are 2^-150 away, which is within 2 u = 1.5 * 2^-22 |x| from |x| = 2^-128 on and for NO fp32 result
    # below that.  So: even multiples of 2^-149 over the whole denormal range (x / 2 exact), and both parities in [2^-128, 2^-126)
    # (x / 2 rounded to even)
    x = torch.randn(n, c, h, w, generator=gen) * 1e-39
    x[1] = torch.randn(c, h, w, generator=gen) * 1e-44
    x = (x.view(torch.int32) & ~1).view(torch.float32)
    x[2] = (3e-39 + torch.rand(c, h, w, generator=gen) * 8e-39) * (1 - 2 * torch.randint(0, 2, (c, h, w), generator=gen))
    out["denormals"] = x
    return out


@pytest.mark.parametrize("name", ["zeros", "inf_nan", "deep_negative", "large_positive", "denormals"])
def test_special_values(name):
    x = special_inputs()[name].to(DEV).contiguous(memory_format=torch.channels_last)
    v = part_a(x, 68, 128)                                                  # codes == fake_quant of the kernel's own output, NaN included
    dense = x.permute(0, 2, 3, 1).contiguous()
    ref = five_steps(dense)
    assert torch.equal(torch.isnan(v), torch.isnan(ref)), "NaN positions"
    ok = ~torch.isnan(ref)
    assert torch.equal(classes(v)[:, ok], classes(ref)[:, ok]), "class (inf / zero / finite) and sign against the five steps in torch ops on the device"
    fin = torch.isfinite(v) & torch.isfinite(dense)
    part_b(dense[fin], v[fin], f"special values: {name}")
    print(name, "bits differ from the five steps in torch ops in", int((bits(v) != bits(ref))[ok].sum()), "of", int(ok.sum()),
          "- from F.gelu in", int((bits(v) != bits(F.gelu(dense)))[ok].sum()))
    if name == "inf_nan":
        assert bool(torch.isnan(v[dense == float("-inf")]).all()) and bool((v[dense == float("inf")] == float("inf")).all())
    if name == "deep_negative":
        z = dense <= -6.0
        assert bool((v[z] == 0).all()) and bool((bits(v[z]) < 0).all())
    if name == "denormals":
        assert bool(((v != 0) & (v.abs() < 2.0 ** -126)).any())             # (not flushed)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_leaves_the_outputs_untouched():
    x = torch.zeros(2, 16, 8, 8, device=DEV).contiguous(memory_format=torch.channels_last)
    obuf = torch.full((4096,), SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full((16384,), CODE_SENTINEL, dtype=torch.uint8, device=DEV)
    sc = torch.tensor([0.01], device=DEV)
    base = dict(x=x.data_ptr(), out=obuf.data_ptr(), codes=cbuf.data_ptr(), n=2, h=8, w=8, c=16, xs=16, c_pad=16, pad_code=0,
                scale=sc.data_ptr(), lo=0, hi=255, form=N.FORM_ZEROPOINT)
    cases = {
        "H < 1": (dict(h=0), -1), "W < 1": (dict(w=0), -1), "C < 4": (dict(c=0), -1), "C % 4": (dict(c=6), -1),
        "x_stride < C": (dict(xs=12), -1), "x_stride % 4": (dict(xs=18), -1), "c_pad < C": (dict(c_pad=12), -1), "c_pad % 4": (dict(c_pad=18), -1),
        "pad_code 256": (dict(pad_code=256), -1), "pad_code -129": (dict(pad_code=-129), -1), "N < 0": (dict(n=-1), -1),
        "both outputs NULL": (dict(out=None, codes=None), -1), "c_pad != C without codes": (dict(codes=None, c_pad=64), -1),
        "x NULL": (dict(x=None), -1), "codes without a scale": (dict(scale=None), -1),
        "lo > hi": (dict(lo=9, hi=3), -1), "unknown form": (dict(form=9), -1),
        "shifted signed range": (dict(form=N.FORM_ZEROPOINT | N.EMIT_SHIFT128, lo=-128, hi=127), -1),
        "FORCE_TILED": (dict(form=N.FORM_ZEROPOINT | N.FORCE_TILED), -1), "ROUTE_ONLY": (dict(form=N.FORM_ZEROPOINT | N.ROUTE_ONLY), -1),
        "PIPELINED": (dict(form=N.FORM_ZEROPOINT | N.PIPELINED), -1), "IN_CHUNK_MAJOR": (dict(form=N.FORM_ZEROPOINT | N.FP32_IN_CHUNK_MAJOR), -1),
        "OUT_CHUNK_MAJOR": (dict(form=N.FORM_ZEROPOINT | N.FP32_OUT_CHUNK_MAJOR), -1),
        "x not 16-byte aligned": (dict(x=x.data_ptr() + 4), -4), "out not 16-byte aligned": (dict(out=obuf.data_ptr() + 8), -4),
        "codes not 4-byte aligned": (dict(codes=cbuf.data_ptr() + 2), -4),
        "an index past 2^31": (dict(n=1 << 31, h=1, w=1, c=4, xs=4, c_pad=4), -2),
        "padded threads past 2^31": (dict(n=1 << 10, h=1 << 10, w=1 << 6, c=4, xs=4, c_pad=128), -2),
    }
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731

    def call(a):
        return N.lib.dlmcq_gelu_nhwc_f32(p(a["x"]), p(a["out"]), p(a["codes"]), a["n"], a["h"], a["w"], a["c"], a["xs"], a["c_pad"],
                                         a["pad_code"], p(a["scale"]), None, a["lo"], a["hi"], a["form"], 0.0, N.stream_ptr())
    for what, (kw, rc) in cases.items():
        assert call(dict(base, **kw)) == rc, what
    assert call(dict(base, n=0)) == 0                                          # N == 0: nothing to do
    torch.cuda.synchronize()
    assert bool((obuf == SENTINEL).all()) and bool((cbuf == CODE_SENTINEL).all())


def test_the_plan_node_on_rows_and_its_torch_path():
    from dlmc.utils.fuse import _ActSpec
    spec = _ActSpec(torch.tensor([0.01], device=DEV), torch.tensor([4.0], device=DEV), 0, 255, N.FORM_ZEROPOINT, False)
    qz = (spec.scale, spec.zp, 0, 255, N.FORM_ZEROPOINT, 0.0, False, 4)
    x = (torch.randn(3, 17, 128, generator=torch.Generator().manual_seed(9)) * 3).to(DEV)
    node = GeluLayer(spec, True, 128, 128, 4, False, rows=True)
    (out, codes), tags = tagged(lambda: node(x))
    assert tags == ["gelu"] and tuple(out.shape) == tuple(codes.shape) == (3, 17, 128) and codes.dtype == torch.uint8
    assert torch.equal(codes.view(51, 1, 1, 128), own_codes(out.view(51, 1, 1, 128), qz, 128))
    four = x.view(3, 1, 17, 128)                                               # rows of rank 4: still rows (the last dimension is the width)
    (o4, c4), tags = tagged(lambda: node(four))
    assert tags == ["gelu"] and torch.equal(o4.view(3, 17, 128), out) and torch.equal(c4.view(3, 17, 128), codes)
    other = x[..., :64].contiguous()                                           # another width than the plan's: torch ops + fake_quant
    (out, codes), tags = tagged(lambda: node(other))
    assert "gelu" not in tags and torch.equal(bits(out), bits(five_steps(other))) and tuple(codes.shape) == (3, 17, 64)
    assert torch.equal(codes.view(51, 1, 1, 64), own_codes(out.view(51, 1, 1, 64), qz, 64))
