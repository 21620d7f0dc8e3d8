"""Squeeze-excite gates on the GPU (include/dlmcq.h: dlmcq_gate_nhwc_f32; K.gate_quant; fuse_inference(gates=True)).

Part 1: the kernel against torch on the device - out == act(x * g.view(N, C, 1, 1)) bit for bit, codes == K.fake_quant of that tensor
        padded as _pad_channels pads, guard bytes behind every buffer untouched - at the smallest shapes at which each index computation
        can go wrong; a channel slice read in place.
Part 2: rounding ties, NaN, infinities, -0 under ReLU, values far outside the range.
Part 3: every refusal of the entry point, with sentinel-filled outputs left untouched; the node's torch path for a gate of another shape.
Part 4: whole plans - three small nets in the three spellings and MobileNetV2-SE: gates=True == gates=False, torch.equal on the logits.
Everything is exact: torch.equal, or the int32 views where NaN occurs."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import _pad_channels

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7fc12345          # a quiet NaN's bit pattern no arithmetic here produces
CODE_SENTINEL = 0xa5
ACTS = {"none": (N.ACT_NONE, lambda t: t), "relu": (N.ACT_RELU, torch.relu), "relu6": (N.ACT_RELU6, F.relu6)}


def bits(t):
    return t.contiguous().view(torch.int32)


def quantisers():
    """name -> (scale, zero point / offset, lo, hi, form, g, shifted emission, pad code of the unshifted codes): those of
    test_gpu_avgpool.py::quantisers()."""
    t = lambda v: torch.tensor([v], device=DEV)  # noqa: E731
    return {"fsptq_zeropoint_u8": (t(0.004), t(3.0), 0, 255, N.FORM_ZEROPOINT, 0.0, False, 3),
            "fsptq_zeropoint_s8": (t(0.01), t(-5.0), -128, 127, N.FORM_ZEROPOINT, 0.0, False, -5),
            "qbase_s8_g": (t(0.006), None, -128, 127, N.FORM_QBASE, 0.02, False, 0),
            "qbase_u8_float_offset": (t(0.003), t(-0.3), 0, 255, N.FORM_QBASE, 0.01, False, 0),
            "shifted_u8": (t(0.004), t(5.0), 0, 255, N.FORM_ZEROPOINT, 0.0, True, 5)}


def torch_path(x, g, act, qz, c_pad):
    """What the unfused graph computes on the device: (act(x * g) as [N, H, W, C] rows, its codes as bytes [N, H, W, c_pad])."""
    s, z, lo, hi, form, gq, shifted, pad = qz
    n, c = x.shape[:2]
    v = ACTS[act][1](x * g.view(n, c, 1, 1)).contiguous(memory_format=torch.channels_last)
    codes = K.fake_quant(v, s, z, lo, hi, form, g=gq, codes="i8", want_y=False)[1].view(torch.uint8) ^ (0x80 if shifted else 0)
    codes = _pad_channels(codes, c_pad, (pad - (128 if shifted else 0)) & 0xff)
    return v.permute(0, 2, 3, 1).contiguous(), codes.permute(0, 2, 3, 1).contiguous()


def raw(x, g, c, act, qz, want_out, want_codes, c_pad):
    """One call of the entry point on guarded buffers; `x`: (N, >= C, H, W) channels_last memory of which channels 0 .. c - 1 are gated.
    Returns (out [N, H, W, C] or None, code bytes [N, H, W, c_pad] or None)."""
    n, xs, h, w = x.shape
    assert x.is_contiguous(memory_format=torch.channels_last) and g.is_contiguous() and tuple(g.shape) == (n, c)
    no, nc = n * h * w * c, n * h * w * c_pad
    obuf = torch.full((no + 1024,), SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full((nc + 1024,), CODE_SENTINEL, dtype=torch.uint8, device=DEV)
    sc, z, lo, hi, form, gq, shifted, pad = qz
    rc = N.lib.dlmcq_gate_nhwc_f32(N.ptr(x), N.ptr(g), N.ptr(obuf) if want_out else None, N.ptr(cbuf) if want_codes else None, n, h, w, c,
                                   xs, c_pad, pad - (128 if shifted else 0), ACTS[act][0], N.ptr(sc), N.ptr(z), lo, hi,
                                   form | (N.EMIT_SHIFT128 if shifted else 0), gq, N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((obuf[no:] == SENTINEL).all()) and bool((cbuf[nc:] == CODE_SENTINEL).all()), "guard bytes behind an output were written"
    if not want_out:
        assert bool((obuf == SENTINEL).all())
    if not want_codes:
        assert bool((cbuf == CODE_SENTINEL).all())
    return (obuf[:no].view(torch.float32).view(n, h, w, c) if want_out else None, cbuf[:nc].view(n, h, w, c_pad) if want_codes else None)


def check_case(x, g, c, c_pad, acts=tuple(ACTS)):
    """`x`: the full-width channels_last tensor on the device, channels 0 .. c - 1 the map; `g`: (N, c) on the device."""
    dense = x[:, :c].contiguous(memory_format=torch.channels_last)
    for name, qz in quantisers().items():
        for act in acts:
            want_v, want_c = torch_path(dense, g, act, qz, c_pad)
            for want_out, want_codes in ((True, True), (False, True), (True, False)):
                if not want_codes and name != "fsptq_zeropoint_u8":
                    continue                              # (the fp32-only call has no quantiser: once)
                got, codes = raw(x, g, c, act, qz, want_out, want_codes, c_pad if want_codes else c)
                what = f"{name} / {act} / out={want_out} codes={want_codes}"
                if want_out:
                    bad = bits(got) != bits(want_v)
                    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {got.numel()} fp32 values differ from torch"
                if want_codes:
                    assert torch.equal(codes, want_c), f"{what}: {int((codes != want_c).sum())} code bytes differ from fake_quant"


# N, C, H, W, c_pad: one workgroup over three images (the gate row follows the thread's own n); odd sides; padding quads; a single
# pixel; several workgroups with rows straddling them; C % 64 != 0 past one 64-channel chunk
SHAPES = [(3, 20, 3, 3, 20), (2, 8, 5, 7, 8), (2, 24, 4, 4, 64), (1, 64, 1, 1, 64), (4, 96, 9, 9, 96), (2, 68, 3, 3, 128)]


def _input(n, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, c, h, w, generator=g) * 1.5, torch.rand(n, c, generator=g) * 1.2       # the map goes negative; gates in [0, 1.2)


# ------------------------------------------------------------------------------------------------------------------ part 1
@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_kernel_against_torch_on_the_device(shape):
    n, c, h, w, c_pad = shape
    x, g = _input(n, c, h, w, sum(shape))
    check_case(x.to(DEV).contiguous(memory_format=torch.channels_last), g.to(DEV), c, c_pad)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_wrapper(shape):
    """K.gate_quant: shapes, layouts and dtypes of what it returns; the gate as (N, C, 1, 1) or (N, C); an NCHW input is copied."""
    n, c, h, w, c_pad = shape
    x, g = _input(n, c, h, w, sum(shape) + 1)
    x, g = x.to(DEV).contiguous(memory_format=torch.channels_last), g.to(DEV)
    for act in ACTS:
        ref = ACTS[act][1](x * g.view(n, c, 1, 1))
        out, none = K.gate_quant(x, g, act=ACTS[act][0])
        assert none is None and out.shape == ref.shape and out.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(bits(out.permute(0, 2, 3, 1)), bits(ref.permute(0, 2, 3, 1)))
        assert torch.equal(K.gate_quant(x.contiguous(), g.view(n, c, 1, 1), act=ACTS[act][0])[0], out)
        for name, (sc, z, lo, hi, form, gq, shifted, pad) in quantisers().items():
            em = K.EmitCodes(sc, z, lo, hi, form, gq, shift128=shifted)
            o2, codes = K.gate_quant(x, g, act=ACTS[act][0], emit=em, c_pad=c_pad, pad_code=pad - (128 if shifted else 0))
            assert codes.dtype == em.dtype and tuple(codes.shape) == (n, c_pad, h, w) and codes.is_contiguous(memory_format=torch.channels_last)
            assert torch.equal(o2, out)
            want = torch_path(x, g, act, (sc, z, lo, hi, form, gq, shifted, pad), c_pad)[1]
            assert torch.equal(codes.view(torch.uint8).permute(0, 2, 3, 1), want), name
            none, only = K.gate_quant(x, g, act=ACTS[act][0], emit=em, want_out=False, c_pad=c_pad, pad_code=pad - (128 if shifted else 0))
            assert none is None and torch.equal(only, codes)
    with pytest.raises(ValueError):
        K.gate_quant(x, g, want_out=False)
    with pytest.raises(ValueError):
        K.gate_quant(x, g, c_pad=c_pad + 4)
    with pytest.raises(ValueError):
        K.gate_quant(x[0], g)
    with pytest.raises(ValueError):
        K.gate_quant(x, g.double())
    with pytest.raises(ValueError):
        K.gate_quant(x, g[:, :4])
    with pytest.raises(N.DlmcqError, match="no CPU fallback"):
        K.gate_quant(x.cpu(), g.cpu())


def test_channel_slice_of_a_wider_tensor_is_read_in_place():
    x, g = _input(2, 24, 6, 6, 77)
    full = torch.full((2, 64, 6, 6), float("nan"))
    full[:, :24] = x
    full, g = full.to(DEV).contiguous(memory_format=torch.channels_last), g.to(DEV)
    check_case(full, g, 24, 64, acts=("none", "relu6"))      # raw calls: x_stride 64, C 24 - a stride error reads NaN
    view = full[:, :24]
    assert not view.is_contiguous(memory_format=torch.channels_last) and K._nhwc_rows(view) == 64 and view.data_ptr() == full.data_ptr()
    sc, z, lo, hi, form, gq, shifted, pad = quantisers()["fsptq_zeropoint_u8"]
    em = K.EmitCodes(sc, z, lo, hi, form, gq)
    copies = []
    real = K._nhwc
    K._nhwc = lambda t: copies.append(t) or real(t)        # the wrapper's only way to a copy
    try:
        out, codes = K.gate_quant(view, g, emit=em, c_pad=64, pad_code=pad)
    finally:
        K._nhwc = real
    assert not copies
    dense = view.contiguous(memory_format=torch.channels_last)
    assert dense.data_ptr() != full.data_ptr()
    out2, codes2 = K.gate_quant(dense, g, emit=em, c_pad=64, pad_code=pad)
    assert torch.equal(bits(out.permute(0, 2, 3, 1)), bits(out2.permute(0, 2, 3, 1))) and torch.equal(codes, codes2)
    assert torch.equal(out, dense * g.view(2, 24, 1, 1))


# ------------------------------------------------------------------------------------------------------------------ part 2
def test_ties_round_half_to_even():
    """Scale 0.25 (dyadic): x = (k + 0.5) * s with gate 1.0, and 2 x with gate 0.5, put the product exactly on the tie k + 0.5."""
    s = 0.25
    k = torch.arange(0, 256, dtype=torch.float32).reshape(1, 16, 4, 4)
    x = (k + 0.5) * s
    x2 = torch.cat([x, 2 * x])                                             # image 0: gate 1.0; image 1: gate 0.5
    g = torch.cat([torch.full((1, 16), 1.0), torch.full((1, 16), 0.5)])
    assert torch.equal(x2 * g.view(2, 16, 1, 1), torch.cat([x, x]))
    qz = (torch.tensor([s], device=DEV), None, 0, 255, N.FORM_ZEROPOINT, 0.0, False, 0)
    xd, gd = x2.to(DEV).contiguous(memory_format=torch.channels_last), g.to(DEV)
    out, codes = raw(xd, gd, 16, "none", qz, True, True, 16)
    even = torch.clamp(torch.round(k + 0.5), 0, 255).permute(0, 2, 3, 1).to(torch.uint8)          # (torch.round: half to even)
    assert torch.equal(codes.cpu(), torch.cat([even, even]))
    want_v, want_c = torch_path(xd, gd, "none", qz, 16)
    assert torch.equal(bits(out), bits(want_v)) and torch.equal(codes, want_c)


def test_the_product_is_rounded_before_the_quantiser_subtracts_its_offset():
    """QBase with the float offset 1.0 and scale 2^-24: x = fl(t / g) for t = 1 + j * 2^-23, j = 1 .. 62, so the real product x * g lies within 2^-24
    of t.  Rounded to fp32 first it is a multiple of 2^-23 and its code (v - 1) / 2^-24 an EVEN integer; an x * g - 1 contracted into one
    fused multiply-add keeps the product's low bits and gives odd codes too."""
    gen = torch.Generator().manual_seed(9)
    j = (torch.arange(2048) % 62 + 1).float().reshape(2, 16, 8, 8)            # t >= 1 + 2^-23: fl(x * g) >= 1, codes 0 .. 126
    g = torch.rand(2, 16, generator=gen) * 0.5 + 0.5
    x = (1.0 + j * 2.0 ** -23) / g.view(2, 16, 1, 1)
    exact = x.double() * g.double().view(2, 16, 1, 1) - 1.0
    assert int((torch.round(exact * 2.0 ** 24) % 2 == 1).sum()) > 100           # what a contracted product would emit: many odd codes
    qo = (torch.tensor([2.0 ** -24], device=DEV), torch.tensor([1.0], device=DEV), -128, 127, N.FORM_QBASE, 0.0, False, 0)
    xd, gd = x.to(DEV).contiguous(memory_format=torch.channels_last), g.to(DEV)
    _, codes = raw(xd, gd, 16, "none", qo, False, True, 16)
    assert bool((codes % 2 == 0).all())
    assert torch.equal(codes, torch_path(xd, gd, "none", qo, 16)[1])


def special_inputs():
    gen = torch.Generator().manual_seed(5)
    n, c, h, w = 3, 68, 3, 3
    out = {}
    x, g = torch.randn(n, c, h, w, generator=gen), torch.rand(n, c, generator=gen)
    g[1, 5] = float("nan")                                # a NaN gate channel
    g[2, 7] = 0.0
    x[2, 7, 1, 1] = float("inf")                          # inf * 0 = NaN
    out["nan_gate"] = (x, g)
    x, g = torch.randn(n, c, h, w, generator=gen), torch.rand(n, c, generator=gen) + 0.1
    x[0, 9, 2, 1], x[1, 11, 0, 0], x[2, 13] = float("inf"), float("-inf"), float("inf")
    x[0, 3, 0, 0] = float("nan")
    out["inf_map"] = (x, g)
    x, g = torch.randn(n, c, h, w, generator=gen), torch.rand(n, c, generator=gen) + 0.1
    x[:, ::2] = -0.0                                      # -0 * a positive gate = -0: under ReLU / ReLU6 what torch makes of it
    x[0, 1] = 0.0
    out["minus_zero"] = (x, g)
    out["far_outside"] = (torch.randn(n, c, h, w, generator=gen) * 1e30, torch.rand(n, c, generator=gen) * 1e8)     # overflows to inf too
    out["tiny"] = (torch.randn(n, c, h, w, generator=gen) * 1e-30, torch.rand(n, c, generator=gen) * 1e-10)        # subnormal products
    return out


@pytest.mark.parametrize("name", ["nan_gate", "inf_map", "minus_zero", "far_outside", "tiny"])
def test_special_values(name):
    x, g = special_inputs()[name]
    if name == "minus_zero":
        v = torch.relu(x.to(DEV) * g.to(DEV).view(3, 68, 1, 1))
        print("torch.relu(-0 * g) on the device: sign bits set in", int((bits(v) < 0).sum()), "of", int((x == 0).sum()), "zeros")
    check_case(x.to(DEV).contiguous(memory_format=torch.channels_last), g.to(DEV), 68, 128)


# ------------------------------------------------------------------------------------------------------------------ part 3
def test_every_refusal_leaves_the_outputs_untouched():
    x = torch.zeros(2, 16, 8, 8, device=DEV).contiguous(memory_format=torch.channels_last)
    gate = torch.ones(2, 16, device=DEV)
    obuf = torch.full((4096,), SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full((16384,), CODE_SENTINEL, dtype=torch.uint8, device=DEV)
    sc = torch.tensor([0.01], device=DEV)
    base = dict(x=x.data_ptr(), gate=gate.data_ptr(), out=obuf.data_ptr(), codes=cbuf.data_ptr(), n=2, h=8, w=8, c=16, xs=16, c_pad=16,
                pad_code=0, act=0, scale=sc.data_ptr(), lo=0, hi=255, form=N.FORM_ZEROPOINT)
    cases = {
        "H < 1": (dict(h=0), -1), "W < 1": (dict(w=0), -1), "C < 4": (dict(c=0), -1), "C % 4": (dict(c=6), -1),
        "x_stride < C": (dict(xs=12), -1), "x_stride % 4": (dict(xs=18), -1), "c_pad < C": (dict(c_pad=12), -1), "c_pad % 4": (dict(c_pad=18), -1),
        "pad_code 256": (dict(pad_code=256), -1), "act 3": (dict(act=3), -1), "act -1": (dict(act=-1), -1),
        "both outputs NULL": (dict(out=None, codes=None), -1), "c_pad != C without codes": (dict(codes=None, c_pad=64), -1),
        "x NULL": (dict(x=None), -1), "gate NULL": (dict(gate=None), -1), "codes without a scale": (dict(scale=None), -1),
        "lo > hi": (dict(lo=9, hi=3), -1), "unknown form": (dict(form=9), -1),
        "shifted signed range": (dict(form=N.FORM_ZEROPOINT | N.EMIT_SHIFT128, lo=-128, hi=127), -1),
        "FORCE_TILED": (dict(form=N.FORM_ZEROPOINT | N.FORCE_TILED), -1), "ROUTE_ONLY": (dict(form=N.FORM_ZEROPOINT | N.ROUTE_ONLY), -1),
        "PIPELINED": (dict(form=N.FORM_ZEROPOINT | N.PIPELINED), -1), "IN_CHUNK_MAJOR": (dict(form=N.FORM_ZEROPOINT | N.FP32_IN_CHUNK_MAJOR), -1),
        "OUT_CHUNK_MAJOR": (dict(form=N.FORM_ZEROPOINT | N.FP32_OUT_CHUNK_MAJOR), -1),
        "x not 16-byte aligned": (dict(x=x.data_ptr() + 4), -4), "gate not 16-byte aligned": (dict(gate=gate.data_ptr() + 8), -4),
        "out not 16-byte aligned": (dict(out=obuf.data_ptr() + 8), -4), "codes not 4-byte aligned": (dict(codes=cbuf.data_ptr() + 2), -4),
        "an index past 2^31": (dict(n=1 << 31, h=1, w=1, c=4, xs=4, c_pad=4), -2),
    }
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731
    for what, (kw, rc) in cases.items():
        a = dict(base, **kw)
        got = N.lib.dlmcq_gate_nhwc_f32(p(a["x"]), p(a["gate"]), p(a["out"]), p(a["codes"]), a["n"], a["h"], a["w"], a["c"], a["xs"], a["c_pad"],
                                        a["pad_code"], a["act"], p(a["scale"]), None, a["lo"], a["hi"], a["form"], 0.0, N.stream_ptr())
        assert got == rc, (what, got)
    a = base
    assert N.lib.dlmcq_gate_nhwc_f32(p(a["x"]), p(a["gate"]), p(a["out"]), p(a["codes"]), 0, 8, 8, 16, 16, 16, 0, 0, p(a["scale"]), None, 0, 255,
                                     N.FORM_ZEROPOINT, 0.0, N.stream_ptr()) == 0                         # N == 0: nothing to do
    torch.cuda.synchronize()
    assert bool((obuf == SENTINEL).all()) and bool((cbuf == CODE_SENTINEL).all())
    with pytest.raises(N.DlmcqError):
        K.gate_quant(torch.zeros(2, 6, 4, 4, device=DEV), torch.ones(2, 6, device=DEV))          # C % 4, through the wrapper


def tagged(fn):
    """fn() with the launch profile on: (result, tags of the launches it made)."""
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        r = fn()
    finally:
        K.PROFILE.enabled = False
    tags = [rec[0] for rec in K.PROFILE.records]
    K.PROFILE.reset()
    return r, tags


@pytest.mark.parametrize("shifted", [False, True])
def test_a_gate_of_another_shape_takes_the_torch_path(shifted):
    from dlmc.utils.fuse import GateLayer, _ActSpec
    x, g = _input(2, 24, 5, 5, 31)
    x, g = x.to(DEV).contiguous(memory_format=torch.channels_last), g.to(DEV)
    spec = _ActSpec(torch.tensor([0.01], device=DEV), torch.tensor([4.0], device=DEV), 0, 255, N.FORM_ZEROPOINT, False)
    node = GateLayer(spec, True, N.ACT_RELU, 24, 64, 4 - (128 if shifted else 0), shifted)
    qz = (spec.scale, spec.zp, 0, 255, N.FORM_ZEROPOINT, 0.0, shifted, 4)
    (out, codes), tags = tagged(lambda: node(x, g.view(2, 24, 1, 1)))
    assert tags == ["gate"] and codes.dtype == (torch.int8 if shifted else torch.uint8) and tuple(codes.shape) == (2, 64, 5, 5)
    want_v, want_c = torch_path(x, g, "relu", qz, 64)
    assert torch.equal(bits(out.permute(0, 2, 3, 1)), bits(want_v)) and torch.equal(codes.view(torch.uint8).permute(0, 2, 3, 1), want_c)
    one = g[:, :1].contiguous().view(2, 1, 1, 1)                              # a per-image gate: (N, 1, 1, 1)
    (out, codes), tags = tagged(lambda: node(x, one))
    assert "gate" not in tags and codes.dtype == (torch.int8 if shifted else torch.uint8) and tuple(codes.shape) == (2, 64, 5, 5)
    ref = torch.relu(x * one)
    assert torch.equal(bits(out.permute(0, 2, 3, 1)), bits(ref.permute(0, 2, 3, 1)))
    rc = K.fake_quant(ref.contiguous(memory_format=torch.channels_last), spec.scale, spec.zp, 0, 255, N.FORM_ZEROPOINT, codes="i8", want_y=False)[1]
    rc = _pad_channels(rc.view(torch.uint8) ^ (0x80 if shifted else 0), 64, (4 - (128 if shifted else 0)) & 0xff)
    assert torch.equal(codes.view(torch.uint8), rc)


# ------------------------------------------------------------------------------------------------------------------ part 4
from gate_nets import GhostSE, MBConvSE, RepVGGSE      # noqa: E402
from test_gpu_narrow_rows import FSPTQ_W8A8, QBASE_W8A8      # noqa: E402  (the configurations of the other plan tests)


def _mobilenet_v2_se():
    import workloads as W
    return W.mobilenet_v2(se=True)


NETS = {"mbconv": (MBConvSE, 16, 1), "ghost": (GhostSE, 16, 1), "repvgg": (RepVGGSE, 16, 1), "mobilenet_v2_se": (_mobilenet_v2_se, 3, 17)}


def _net(make, cin, cfg, qtype, seed, offsets):
    """tests/test_gpu_avgpool.py::_net for a network with gates: calibrated on relu(N(0, 1)), the quantisers' offsets then set to exactly
    0 (so that no layer keeps its fp32 wrapper over a minimum that is merely close to 0) - except, with `offsets`, on the convolution that
    reads the gated map, which gets a float offset that act_offsets=True plans."""
    from dlmc.quantization.scalar.FSPTQuant import FSPTQBase
    from dlmc.quantization.scalar.modules.base import QBase
    from dlmc.utils.merge_bn import merge_bn
    from dlmc.utils.quantize import quantize_model
    torch.manual_seed(seed)
    net = make().to(DEV).eval()
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    net = merge_bn(net, inplace=True, allow_missing=True)
    if qtype:
        quantize_model(net, copy.deepcopy(cfg), None, qtype, int8_gemm=True)
    else:
        quantize_model(net, copy.deepcopy(cfg), None)
    x = torch.relu(torch.randn(4, cin, 32, 32, device=DEV))
    with torch.no_grad():
        net(x)                                   # calibrate
    for name, m in net.named_modules():
        if isinstance(m, FSPTQBase):
            m.in_offset.zero_()
            m._zp_is_int = None
        elif isinstance(m, QBase) and m.in_offset is not None:
            m.in_offset.zero_()
            if offsets and name == make.reader:
                m.in_offset.fill_(-0.03125)
    return net, x


PLAN_CASES = {"fsptq": (FSPTQ_W8A8, "FSPTQ", {}), "qbase": (QBASE_W8A8, None, {}), "qbase_act_offsets": (QBASE_W8A8, None, dict(act_offsets=True))}


# (MobileNetV2-SE's gated maps are ReLU6 outputs times a gate in [0, 1]: no offset to plan there)
PLANS = [(tag, name) for name in sorted(NETS) for tag in sorted(PLAN_CASES) if not (tag == "qbase_act_offsets" and name == "mobilenet_v2_se")]


@pytest.mark.parametrize("tag, name", PLANS)
def test_plan_flag_on_equals_flag_off(tag, name):
    from dlmc.utils.fuse import GateLayer, fuse_inference
    make, cin, n_gates = NETS[name]
    cfg, qtype, kw = PLAN_CASES[tag]
    offsets = "act_offsets" in kw
    net, x = _net(make, cin, cfg, qtype, 61, offsets)
    off = fuse_inference(net, **kw)
    on = fuse_inference(net, gates=True, **kw)
    with torch.no_grad():
        (a, _), (b, tags) = tagged(lambda: off(x)), tagged(lambda: on(x))
        again = on(x)
    ro, rn = off.fusion_report, on.fusion_report
    print(ro, rn, sep="\n")
    assert bool(torch.isfinite(a).all()) and torch.equal(b, again)
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} logits differ, max {float((a - b).abs().max())}"
    assert (ro.gates, rn.gates) == (0, n_gates) and rn.skipped == ro.skipped and tags.count("gate") == n_gates
    assert (rn.layers, rn.residual, rn.relu, rn.relu6, rn.emit, rn.fp32_outputs, rn.narrow, rn.dual, rn.act_offset) == \
           (ro.layers, ro.residual, ro.relu, ro.relu6, ro.emit, ro.fp32_outputs, ro.narrow, ro.dual, ro.act_offset)
    nodes = [m for m in on.modules() if isinstance(m, GateLayer)]
    assert len(nodes) == n_gates and not any(m.want_out for m in nodes)
    if offsets:
        assert rn.act_offset >= 1 and all(m.emit.xoff and m.pad_code == (-128 if m.emit_shift else 0) for m in nodes)
    if name == "repvgg":
        assert nodes[0].act == N.ACT_RELU
