"""Swish on the GPU (include/dlmcq.h: dlmcq_swish_nhwc_f32; K.swish_quant; fuse_inference(swish=True)).

Part A: exact - the codes are K.fake_quant of the kernel's OWN fp32 output, padded as _pad_channels pads; the codes-only call returns the
        same bytes; guard bytes and unrequested buffers untouched.
Part B: against float64 - |v - v64| <= 3 * 2^-23 |v64| for |x| <= 80, v64 = x / (1 + exp(-x)) in float64 from the same fp32 input.  The
        kernel rounds three times (add, divide, multiply: <= 2^-24 relative each) and expf's error, <= 1 ulp = 2^-23 relative (the device
        library's documented bound for exp), reaches 1 + e scaled by e / (1 + e) < 1: <= 2.5 * 2^-23 to first order, rounded up to 3.
        torch's own x * torch.sigmoid(x) on the device passes the same bound in the same test.
Part C: how many elements differ in their bits from x * torch.sigmoid(x) and from F.silu(x) on the device, printed and summed over the
        Part A inputs (DESIGN.md 5.20 records them).  MATCHES_TORCH_MUL states what was measured: True pins torch.equal against
        x * torch.sigmoid(x) here and on the logits of Part E; False asserts that every differing element satisfies Part B.
Part D: special values - +-0, +-inf, NaN, x <= -88 (exp overflows), denormals, rounding ties of each quantiser behind the swish.
Part E: whole plans - three small nets in the three spellings and workloads.mobilenet_v2(se=True, act="swish")."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import _pad_channels
from test_gpu_gate import CODE_SENTINEL, DEV, PLAN_CASES, SENTINEL, _net, bits, quantisers, tagged

pytestmark = pytest.mark.gpu
MATCHES_TORCH_MUL = True       # Part C's first count, as measured on an MI355X: 0 of the elements of the Part A inputs
BOUND = 3 * 2.0 ** -23


def own_codes(v_nhwc, qz, c_pad):
    """K.fake_quant of the fp32 values `v_nhwc` [N, H, W, C] as code bytes [N, H, W, c_pad], shifted and padded as the plan does it."""
    s, z, lo, hi, form, gq, shifted, pad = qz
    v = v_nhwc.permute(0, 3, 1, 2)                         # (N, C, H, W), channels_last memory
    codes = K.fake_quant(v, s, z, lo, hi, form, g=gq, codes="i8", want_y=False)[1].view(torch.uint8) ^ (0x80 if shifted else 0)
    return _pad_channels(codes, c_pad, (pad - (128 if shifted else 0)) & 0xff).permute(0, 2, 3, 1).contiguous()


def raw(x, c, qz, want_out, want_codes, c_pad):
    """One call of the entry point on guarded buffers; `x`: (N, >= C, H, W) channels_last memory of which channels 0 .. c - 1 are read.
    Returns (out [N, H, W, C] or None, code bytes [N, H, W, c_pad] or None)."""
    n, xs, h, w = x.shape
    assert x.is_contiguous(memory_format=torch.channels_last)
    no, nc = n * h * w * c, n * h * w * c_pad
    obuf = torch.full((no + 1024,), SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full((nc + 1024,), CODE_SENTINEL, dtype=torch.uint8, device=DEV)
    sc, z, lo, hi, form, gq, shifted, pad = qz
    rc = N.lib.dlmcq_swish_nhwc_f32(N.ptr(x), N.ptr(obuf) if want_out else None, N.ptr(cbuf) if want_codes else None, n, h, w, c, xs, c_pad,
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
            only_out, none = raw(x, c, qz, True, False, c)          # (the fp32-only call has no quantiser: once)
            assert none is None and torch.equal(bits(only_out), bits(first))
        assert torch.equal(bits(out), bits(first)), name
        want = own_codes(out, qz, c_pad)
        assert torch.equal(codes, want), f"{name}: {int((codes != want).sum())} code bytes differ from fake_quant of the kernel's own output"
        none, only = raw(x, c, qz, False, True, c_pad)
        assert none is None and torch.equal(only, codes), f"{name}: the codes-only call returns other bytes"
    return first


def part_b(x_nhwc, v_nhwc, what):
    """|v - v64| <= 3 * 2^-23 |v64| where |x| <= 80; returns the largest error in units of 2^-23 |v64|."""
    x64 = x_nhwc.double()
    v64 = x64 / (1.0 + torch.exp(-x64))
    ok = (x64.abs() <= 80) & (v64 != 0)
    err = ((v_nhwc.double() - v64).abs() / v64.abs())[ok]
    worst = float(err.max()) / 2.0 ** -23 if err.numel() else 0.0
    print(f"{what}: max |v - v64| / |v64| = {worst:.3f} * 2^-23 over {int(ok.sum())} elements")
    assert worst * 2.0 ** -23 <= BOUND, what
    assert bool((v_nhwc[(x64 == 0)] == 0).all())
    return worst


# N, C, H, W, c_pad - the gate tests' shapes: one workgroup over three images; odd sides; padding quads; a single pixel; several
# workgroups with rows straddling them; C % 64 != 0 past one 64-channel chunk.  The last: a channel slice read in place (x_stride 64)
SHAPES = [(3, 20, 3, 3, 20), (2, 8, 5, 7, 8), (2, 24, 4, 4, 64), (1, 64, 1, 1, 64), (4, 96, 9, 9, 96), (2, 68, 3, 3, 128), (2, 24, 6, 6, 64, 64)]
IDS = ["x".join(map(str, s)) for s in SHAPES[:-1]] + ["slice_24_of_64"]


@functools.lru_cache(maxsize=None)
def case(shape):
    """(the tensor handed to the kernel, its dense (N, C, H, W) input as [N, H, W, C] rows, x * sigmoid(x) and F.silu(x) on the device
    as such rows) for one shape: made once, shared by the tests, never written."""
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
    return given, dense, dense * torch.sigmoid(dense), F.silu(dense)


COUNTS = {}


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kernel(shape):
    given, dense, mul, silu = case(shape)
    c, c_pad = shape[1], shape[4]
    v = part_a(given, c, c_pad)
    part_b(dense, v, "kernel")
    part_b(dense, mul, "torch x * sigmoid(x)")           # the bound is not vacuous against the path being replaced
    d_mul, d_silu = bits(v) != bits(mul), bits(v) != bits(silu)
    COUNTS[shape] = (int(d_mul.sum()), int(d_silu.sum()), v.numel())
    print(f"bits differ from x * torch.sigmoid(x): {COUNTS[shape][0]}, from F.silu(x): {COUNTS[shape][1]}, of {v.numel()}")
    if MATCHES_TORCH_MUL:
        assert torch.equal(v, mul)
    elif bool(d_mul.any()):
        x64 = dense.double()[d_mul]
        v64 = x64 / (1.0 + torch.exp(-x64))
        assert bool(((v.double()[d_mul] - v64).abs() <= BOUND * v64.abs()).all())


def test_part_c_totals():
    for shape in SHAPES:
        if shape not in COUNTS:
            given, dense, mul, silu = case(shape)
            v = K.swish_quant(given[:, :shape[1]])[0].permute(0, 2, 3, 1)
            COUNTS[shape] = (int((bits(v) != bits(mul)).sum()), int((bits(v) != bits(silu)).sum()), v.numel())
    tot = [sum(c[i] for c in COUNTS.values()) for i in range(3)]
    print(f"PART C: of {tot[2]} elements {tot[0]} differ in their bits from x * torch.sigmoid(x), {tot[1]} from F.silu(x)")
    assert (tot[0] == 0) == MATCHES_TORCH_MUL, "MATCHES_TORCH_MUL no longer states what the device does"


@pytest.mark.parametrize("shape", SHAPES[:3] + SHAPES[-1:], ids=IDS[:3] + IDS[-1:])
def test_wrapper(shape):
    """K.swish_quant: shapes, layouts and dtypes of what it returns; an NCHW input is copied, a channel slice read in place."""
    given, dense, mul, silu = case(shape)
    n, c, h, w, c_pad = shape[:5]
    x = given[:, :c]
    copies = []
    real = K._nhwc
    K._nhwc = lambda t: copies.append(t) or real(t)        # the wrapper's only way to a copy
    try:
        out, none = K.swish_quant(x)
    finally:
        K._nhwc = real
    assert not copies and none is None and tuple(out.shape) == (n, c, h, w) and out.is_contiguous(memory_format=torch.channels_last)
    ref = part_a(given, c, c_pad, names=("fsptq_zeropoint_u8",))
    assert torch.equal(bits(out.permute(0, 2, 3, 1)), bits(ref))
    assert torch.equal(K.swish_quant(x.contiguous())[0], out)              # NCHW-contiguous: copied to channels_last
    for name, qz in quantisers().items():
        sc, z, lo, hi, form, gq, shifted, pad = qz
        em = K.EmitCodes(sc, z, lo, hi, form, gq, shift128=shifted)
        o2, codes = K.swish_quant(x, emit=em, c_pad=c_pad, pad_code=pad - (128 if shifted else 0))
        assert codes.dtype == em.dtype and tuple(codes.shape) == (n, c_pad, h, w) and codes.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(o2, out)
        assert torch.equal(codes.view(torch.uint8).permute(0, 2, 3, 1), own_codes(ref, qz, c_pad)), name
        none, only = K.swish_quant(x, emit=em, want_out=False, c_pad=c_pad, pad_code=pad - (128 if shifted else 0))
        assert none is None and torch.equal(only, codes)
    with pytest.raises(ValueError):
        K.swish_quant(x, want_out=False)
    with pytest.raises(ValueError):
        K.swish_quant(x, c_pad=c_pad + 4)
    with pytest.raises(ValueError):
        K.swish_quant(x[0])
    with pytest.raises(ValueError):
        K.swish_quant(x.double())
    with pytest.raises(N.DlmcqError, match="no CPU fallback"):
        K.swish_quant(x.cpu())


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
    x = -torch.rand(n, c, h, w, generator=gen) * 30 - 80                   # -80 .. -110: exp(-x) overflows from 88.73 on
    x[0, 0, 0, 0], x[0, 1, 0, 0], x[0, 2, 0, 0], x[0, 3, 0, 0] = -88.0, -88.72, -88.73, -104.0
    out["exp_overflows"] = x
    out["large_positive"] = torch.rand(n, c, h, w, generator=gen) * 3e38
    x = torch.randn(n, c, h, w, generator=gen) * 1e-39                     # denormal inputs: v = x / 2, denormal too
    x[1] = torch.randn(c, h, w, generator=gen) * 1e-44
    out["denormals"] = x
    return out


def classes(t):
    return torch.stack([torch.isnan(t), torch.isinf(t), t == 0, bits(t) < 0])


@pytest.mark.parametrize("name", ["zeros", "inf_nan", "exp_overflows", "large_positive", "denormals"])
def test_special_values(name):
    x = special_inputs()[name].to(DEV).contiguous(memory_format=torch.channels_last)
    v = part_a(x, 68, 128)                                                  # codes == fake_quant of the kernel's own output, NaN included
    dense = x.permute(0, 2, 3, 1).contiguous()
    ref = dense * torch.sigmoid(dense)
    assert torch.equal(torch.isnan(v), torch.isnan(ref)), "NaN positions"
    ok = ~torch.isnan(ref)
    assert torch.equal(classes(v)[:, ok], classes(ref)[:, ok]), "class (inf / zero / finite) and sign against torch on the device"
    print(name, "bits differ from torch in", int((bits(v) != bits(ref))[ok].sum()), "of", int(ok.sum()))
    if name == "denormals":
        assert bool(((v != 0) & (v.abs() < 2.0 ** -126)).any())             # (not flushed)
    if MATCHES_TORCH_MUL:
        assert torch.equal(bits(v)[ok], bits(ref)[ok])


def tie_quantisers():
    """The five forms, and the plain one without a zero point, at the dyadic scale 0.25, so that x = (k + 0.5) / 4 is exact; from x = 17 on, 1 + expf(-x) rounds to 1, sigmoid to
    1 and v = x exactly: v / s lands on the tie k + 0.5 (less an integer zero point; the float offset 0.125 moves it off - and
    2.125 onto the next one)."""
    t = lambda v: torch.tensor([v], device=DEV)  # noqa: E731
    return {"fsptq_zeropoint_u8": (t(0.25), t(3.0), 0, 255, N.FORM_ZEROPOINT, 0.0, False, 3),
            "fsptq_zeropoint_s8": (t(0.25), t(-100.0), -128, 127, N.FORM_ZEROPOINT, 0.0, False, -100),
            "qbase_s8_g": (t(0.25), None, -128, 127, N.FORM_QBASE, 0.0, False, 0),
            "qbase_u8_float_offset": (t(0.25), t(0.25), 0, 255, N.FORM_QBASE, 0.0, False, 0),
            "shifted_u8": (t(0.25), t(5.0), 0, 255, N.FORM_ZEROPOINT, 0.0, True, 5),
            "plain_u8": (t(0.25), None, 0, 255, N.FORM_ZEROPOINT, 0.0, False, 0)}


def test_ties_round_half_to_even():
    k = torch.arange(68, 324, dtype=torch.float32).reshape(1, 16, 4, 4)      # x = 17.125 .. 80.875
    x = ((k + 0.5) * 0.25).to(DEV).contiguous(memory_format=torch.channels_last)
    kk = k.permute(0, 2, 3, 1).to(DEV)
    for name, qz in tie_quantisers().items():
        out, codes = raw(x, 16, qz, True, True, 16)
        assert torch.equal(out, x.permute(0, 2, 3, 1)), "sigmoid(x) = 1 from x = 17 on: v = x"
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
        return N.lib.dlmcq_swish_nhwc_f32(p(a["x"]), p(a["out"]), p(a["codes"]), a["n"], a["h"], a["w"], a["c"], a["xs"], a["c_pad"],
                                          a["pad_code"], p(a["scale"]), None, a["lo"], a["hi"], a["form"], 0.0, N.stream_ptr())
    for what, (kw, rc) in cases.items():
        assert call(dict(base, **kw)) == rc, what
    assert call(dict(base, n=0)) == 0                                          # N == 0: nothing to do
    torch.cuda.synchronize()
    assert bool((obuf == SENTINEL).all()) and bool((cbuf == CODE_SENTINEL).all())
    with pytest.raises(N.DlmcqError):
        K.swish_quant(torch.zeros(2, 6, 4, 4, device=DEV))                     # C % 4, through the wrapper


@pytest.mark.parametrize("shifted", [False, True])
def test_an_input_that_is_no_map_takes_the_torch_path(shifted):
    from dlmc.utils.fuse import SwishLayer, _ActSpec
    given, dense, mul, silu = case(SHAPES[2])                                  # (2, 24, 4, 4), code rows 64 wide
    spec = _ActSpec(torch.tensor([0.01], device=DEV), torch.tensor([4.0], device=DEV), 0, 255, N.FORM_ZEROPOINT, False)
    node = SwishLayer(spec, True, 24, 64, 4 - (128 if shifted else 0), shifted)
    qz = (spec.scale, spec.zp, 0, 255, N.FORM_ZEROPOINT, 0.0, shifted, 4)
    (out, codes), tags = tagged(lambda: node(given))
    assert tags == ["swish"] and codes.dtype == (torch.int8 if shifted else torch.uint8) and tuple(codes.shape) == (2, 64, 4, 4)
    assert torch.equal(codes.view(torch.uint8).permute(0, 2, 3, 1), own_codes(out.permute(0, 2, 3, 1), qz, 64))
    vec = given[:, :, 0, 0].contiguous()                                       # a 2-D input: (N, 24)
    (out, codes), tags = tagged(lambda: node(vec))
    assert "swish" not in tags and tuple(out.shape) == (2, 24) and torch.equal(bits(out), bits(vec * torch.sigmoid(vec)))
    want = K.fake_quant(out, spec.scale, spec.zp, 0, 255, N.FORM_ZEROPOINT, codes="i8", want_y=False)[1].view(torch.uint8) ^ (0x80 if shifted else 0)
    assert codes.dtype == (torch.int8 if shifted else torch.uint8) and torch.equal(codes.view(torch.uint8), want)
    other = torch.randn(2, 20, 4, 4, device=DEV)                               # a map of another width than the plan's
    (out, codes), tags = tagged(lambda: node(other))
    assert "swish" not in tags and torch.equal(bits(out), bits(other * torch.sigmoid(other))) and tuple(codes.shape) == (2, 64, 4, 4)
    plain = SwishLayer(None, True, None, None, 0)                              # nobody takes codes
    (out, codes), tags = tagged(lambda: plain(given))
    assert tags == ["swish"] and codes is None and torch.equal(bits(out.permute(0, 2, 3, 1)), bits(K.swish_quant(given)[0].permute(0, 2, 3, 1)))
    (out, codes), tags = tagged(lambda: plain(vec))
    assert not tags and codes is None and torch.equal(bits(out), bits(vec * torch.sigmoid(vec)))


# ------------------------------------------------------------------------------------------------------------------ part E
from swish_nets import FunctionalSiLU, ModuleSiLU, MulSwish      # noqa: E402


def _mbconv_se():
    import workloads as W
    return W.mobilenet_v2(se=True, act="swish")


NETS = {"mul": (MulSwish, 16, 2, 0), "module": (ModuleSiLU, 16, 2, 0), "functional": (FunctionalSiLU, 16, 2, 0), "mbconv_se": (_mbconv_se, 3, 35, 17)}
# (the MBConv network's readers behind a swish get no float offset planned: the tests' calibration sets every offset to 0)
PLANS = [(tag, name) for name in sorted(NETS) for tag in sorted(PLAN_CASES) if not (tag == "qbase_act_offsets" and name == "mbconv_se")]


def _sigmoids_on_maps(gm, x):
    """sigmoid / silu nodes of the plan whose input is a 4-D tensor with more than one pixel or that feed no gate node: run the graph
    node by node and look."""
    from torch import fx, nn
    found = []
    mods = dict(gm.named_modules())

    class Look(fx.Interpreter):
        def run_node(self, n):
            r = super().run_node(n)
            act = ((n.op == "call_function" and n.target in (torch.sigmoid, F.sigmoid, F.silu)) or (n.op == "call_method" and n.target == "sigmoid") or
                   (n.op == "call_module" and isinstance(mods.get(n.target), (nn.SiLU, nn.Sigmoid))))
            if act and torch.is_tensor(r) and r.dim() == 4:
                gate_only = all(u.op == "call_module" and str(u.target).startswith("_int8_gate_") and u.args[1] is n for u in n.users)
                if not (gate_only and tuple(r.shape[2:]) == (1, 1)):           # (the (N, C, 1, 1) gate of a squeeze path is no map)
                    found.append(n)
            return r
    with torch.no_grad():
        Look(gm).run(x)
    return found


@pytest.mark.parametrize("tag, name", PLANS)
def test_plans(tag, name):
    from dlmc.utils.fuse import GateLayer, SwishLayer, fuse_inference
    make, cin, n_swish, n_gates = NETS[name]
    cfg, qtype, kw = PLAN_CASES[tag]
    net, x = _net(make, cin, cfg, qtype, 67, "act_offsets" in kw)
    x = x[:2].contiguous()
    off = fuse_inference(net, gates=True, **kw)
    on = fuse_inference(net, gates=True, swish=True, **kw)
    ro, rn = off.fusion_report, on.fusion_report
    print(ro, rn, sep="\n")
    assert (ro.swishes, rn.swishes) == (0, n_swish) and ro.gates == rn.gates == n_gates and rn.skipped == ro.skipped
    assert (rn.layers, rn.residual, rn.relu, rn.relu6, rn.emit, rn.fp32_outputs, rn.narrow, rn.dual, rn.act_offset) == \
           (ro.layers, ro.residual, ro.relu, ro.relu6, ro.emit, ro.fp32_outputs, ro.narrow, ro.dual, ro.act_offset)
    nodes = {n_: m for n_, m in on.named_modules() if isinstance(m, SwishLayer)}
    assert len(nodes) == n_swish and sum(isinstance(m, GateLayer) for m in on.modules()) == n_gates
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, a, r, n_=n_: seen.__setitem__(n_, (a[0], r))) for n_, m in nodes.items()]
    with torch.no_grad():
        (a, _), (b, tags) = tagged(lambda: off(x)), tagged(lambda: on(x))
        for h in hooks:
            h.remove()
        again = on(x)
    assert tags.count("swish") == n_swish and tags.count("gate") == n_gates and "swish" not in tagged(lambda: off(x))[1]
    assert not _sigmoids_on_maps(on, x) and len(_sigmoids_on_maps(off, x)) >= n_swish
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()) and torch.equal(b, again)
    # Parts A and B at the network's own shapes, on what every node was given and gave back
    assert sorted(seen) == sorted(nodes)
    worst = 0.0
    for n_, (t, (out, codes)) in seen.items():
        m = nodes[n_]
        assert t.dim() == 4 and (out is not None) == m.want_out and (codes is not None) == (m.emit is not None)
        own = K.swish_quant(t)[0]
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
    top1 = int((a.flatten(1).argmax(1) == b.flatten(1).argmax(1)).sum())
    print(f"{tag} / {name}: max |logit(swish=True) - logit(swish=False)| = {dev:.3e}, top-1 equal in {top1} of {a.shape[0]}, "
          f"worst Part B error {worst:.3f} * 2^-23")
    # the node computes x * torch.sigmoid(x): equal logits are pinned where the network spells it so.  nn.SiLU / F.silu divide x by
    # 1 + exp(-x) instead and differ from the node in the last bit of about a quarter of the elements (Part C): recorded, not pinned
    if MATCHES_TORCH_MUL and name in ("mul", "mbconv_se"):
        assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} logits differ, max {dev}"
