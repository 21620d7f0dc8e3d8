"""Windowed average pools on the GPU (include/dlmcq.h: dlmcq_avgpool_nhwc_f32; K.avgpool_quant; fuse_inference(avg_pools=True)).

Part 1: the kernel against a restatement of its arithmetic written here with torch elementwise ops on the CPU (a sequential fp32 sum from
        +0 in row-major window order, one fp32 division) - pooled values bit for bit, codes equal to K.fake_quant of the restated values,
        pad channels equal to the pad code, guard bytes behind every buffer untouched - and against torch's own avg_pool2d on the device,
        bit for bit: the property the flag's contract (bit-identical plans) rests on.
Part 2: rounding ties, -0, NaN, infinities, values far outside the range.
Part 3: every refusal of the entry point, with sentinel-filled outputs left untouched.
Part 4: whole plans - CIFAR ResNet-20 with option-C / -D shortcuts: avg_pools=True == avg_pools=False, torch.equal on the logits."""
import copy
import ctypes

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 0x7fc12345          # a quiet NaN's bit pattern no arithmetic here produces
CODE_SENTINEL = 0xa5


def restate(x, s):
    """The definition, on the CPU: x fp32 (N, C, H, W) -> pooled fp32 (N, C, H // s, W // s)."""
    x = x.detach().cpu()
    n, c, h, w = x.shape
    p, q = h // s, w // s
    a = torch.zeros(n, c, p, q, dtype=torch.float32)                 # +0
    for dy in range(s):
        for dx in range(s):
            a = a + x[:, :, dy:p * s:s, dx:q * s:s]                  # fl32(a + x[n, c, p*s + dy, q*s + dx])
    return a / torch.tensor(float(s * s), dtype=torch.float32)      # one IEEE fp32 division


def bits(t):
    return t.contiguous().view(torch.int32)


def same(a, b, what):
    """Bit equality of two fp32 tensors, every NaN counting as one value (the sign of a zero is compared)."""
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert torch.equal(torch.isnan(a), torch.isnan(b)), f"{what}: NaNs in different places"
    inf = float("inf")
    a, b = torch.nan_to_num(a, nan=0.0, posinf=inf, neginf=-inf), torch.nan_to_num(b, nan=0.0, posinf=inf, neginf=-inf)
    bad = bits(a) != bits(b)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {a.numel()} differ"


def quantisers():
    """name -> (scale, zero point / offset, lo, hi, form, g, shifted emission, pad code of the unshifted codes)."""
    t = lambda v: torch.tensor([v], device=DEV)  # noqa: E731
    return {"fsptq_zeropoint_u8": (t(0.004), t(3.0), 0, 255, N.FORM_ZEROPOINT, 0.0, False, 3),
            "qbase_s8_g": (t(0.006), None, -128, 127, N.FORM_QBASE, 0.02, False, 0),
            "qbase_u8_float_offset": (t(0.003), t(-0.3), 0, 255, N.FORM_QBASE, 0.01, False, 0),
            "shifted_u8": (t(0.004), t(5.0), 0, 255, N.FORM_ZEROPOINT, 0.0, True, 5)}


def ref_codes(pooled, qz):
    """K.fake_quant's codes of the restated pooled values (N, C, P, Q) as bytes [N, P, Q, C]."""
    s, z, lo, hi, form, g, shifted, _ = qz
    dev = pooled.to(DEV).contiguous(memory_format=torch.channels_last)
    c = K.fake_quant(dev, s, z, lo, hi, form, g=g, codes="i8", want_y=False)[1].view(torch.uint8)
    return (c ^ (0x80 if shifted else 0)).permute(0, 2, 3, 1).contiguous()


def raw(x, s, c, qz, want_out, want_codes, c_pad):
    """One call of the entry point on guarded buffers; `x`: (N, >= C, H, W) channels_last memory of which channels 0 .. c - 1 are pooled.
    Returns (pooled [N, P, Q, C] or None, code bytes [N, P, Q, c_pad] or None)."""
    n, xs, h, w = x.shape
    assert x.is_contiguous(memory_format=torch.channels_last)
    p, q = h // s, w // s
    no, nc = n * p * q * c, n * p * q * c_pad
    obuf = torch.full((no + 1024,), SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full((nc + 1024,), CODE_SENTINEL, dtype=torch.uint8, device=DEV)
    sc, z, lo, hi, form, g, shifted, pad = qz
    rc = N.lib.dlmcq_avgpool_nhwc_f32(N.ptr(x), N.ptr(obuf) if want_out else None, N.ptr(cbuf) if want_codes else None, n, h, w, c, xs, s,
                                      c_pad, pad - (128 if shifted else 0), N.ptr(sc), N.ptr(z), lo, hi,
                                      form | (N.EMIT_SHIFT128 if shifted else 0), g, N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((obuf[no:] == SENTINEL).all()) and bool((cbuf[nc:] == CODE_SENTINEL).all()), "guard bytes behind an output were written"
    if not want_out:
        assert bool((obuf == SENTINEL).all())
    if not want_codes:
        assert bool((cbuf == CODE_SENTINEL).all())
    return (obuf[:no].view(torch.float32).view(n, p, q, c) if want_out else None, cbuf[:nc].view(n, p, q, c_pad) if want_codes else None)


def check_case(x, s, c, c_pad, want_pooled):
    """`x`: the full-width channels_last tensor on the device; channels 0 .. c - 1 are the map."""
    want_rows = want_pooled.permute(0, 2, 3, 1).contiguous().to(DEV)
    for name, qz in quantisers().items():
        want_c = ref_codes(want_pooled, qz)
        pad_byte = (qz[7] - (128 if qz[6] else 0)) & 0xff
        for want_out, want_codes in ((True, False), (False, True), (True, True)):
            if not want_codes and name != "fsptq_zeropoint_u8":
                continue                                  # (the pooled-only call has no quantiser: once)
            cp = c_pad if want_codes else c
            got, codes = raw(x, s, c, qz, want_out, want_codes, cp)
            if want_out:
                same(got, want_rows, f"{name}: pooled against the restatement")
            if want_codes:
                assert torch.equal(codes[..., :c], want_c), f"{name}: {int((codes[..., :c] != want_c).sum())} codes differ from fake_quant"
                assert bool((codes[..., c:] == pad_byte).all()), f"{name}: pad channels"


SHAPES = [(2, 4, 4, 4, 2, 4), (3, 16, 9, 9, 2, 64), (2, 72, 7, 5, 3, 128), (2, 64, 8, 8, 4, 64), (5, 32, 17, 17, 2, 64)]   # N, C, H, W, s, c_pad


def _input(n, c, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.relu(torch.randn(n, c, h, w, generator=g)) * 1.5


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_kernel_against_the_restatement(shape):
    n, c, h, w, s, c_pad = shape
    x = _input(n, c, h, w, sum(shape))
    check_case(x.to(DEV).contiguous(memory_format=torch.channels_last), s, c, c_pad, restate(x, s))


def test_channel_slice_of_a_wider_tensor_is_read_in_place():
    x = _input(2, 16, 8, 8, 77)
    full = torch.full((2, 64, 8, 8), float("nan"))
    full[:, :16] = x
    full = full.to(DEV).contiguous(memory_format=torch.channels_last)
    want = restate(x, 2)
    check_case(full, 2, 16, 64, want)                     # raw calls: x_stride 64, C 16 - a stride error reads NaN
    view = full[:, :16]
    assert not view.is_contiguous(memory_format=torch.channels_last) and K._nhwc_rows(view) == 64
    pooled, none = K.avgpool_quant(view, 2)
    assert none is None and pooled.is_contiguous(memory_format=torch.channels_last) and tuple(pooled.shape) == (2, 16, 4, 4)
    same(pooled.cpu(), want, "wrapper on the slice")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda v: "x".join(map(str, v)))
def test_wrapper_and_torch_on_the_device(shape):
    """K.avgpool_quant's pooled values == F.avg_pool2d on the device, bit for bit (channels_last input) - what lets
    fuse_inference(avg_pools=True) promise the plan without the flag - and its outputs' shapes, layouts and dtypes."""
    n, c, h, w, s, c_pad = shape
    x = _input(n, c, h, w, sum(shape)).to(DEV).contiguous(memory_format=torch.channels_last)
    pooled, none = K.avgpool_quant(x, s)
    ref = F.avg_pool2d(x, s)
    assert none is None and pooled.shape == ref.shape and pooled.is_contiguous(memory_format=torch.channels_last)
    diff = bits(pooled.contiguous()) != bits(ref.contiguous())
    print("elements differing from torch's avg_pool2d:", int(diff.sum()), "of", pooled.numel())
    assert torch.equal(pooled, ref)
    same(pooled.cpu(), restate(x, s), "wrapper against the restatement")
    nchw = x.contiguous()                                  # an NCHW-contiguous input is copied to channels_last
    assert torch.equal(K.avgpool_quant(nchw, s)[0], pooled)
    for name, (sc, z, lo, hi, form, g, shifted, pad) in quantisers().items():
        em = K.EmitCodes(sc, z, lo, hi, form, g, shift128=shifted)
        p2, codes = K.avgpool_quant(x, s, emit=em, c_pad=c_pad, pad_code=pad - (128 if shifted else 0))
        assert codes.dtype == em.dtype and tuple(codes.shape) == (n, c_pad, h // s, w // s) and codes.is_contiguous(memory_format=torch.channels_last)
        assert torch.equal(p2, pooled)
        want = K.fake_quant(pooled, sc, z, lo, hi, form, g=g, codes="i8", want_y=False)[1].view(torch.uint8) ^ (0x80 if shifted else 0)
        assert torch.equal(codes.view(torch.uint8)[:, :c], want), name
        assert bool((codes.view(torch.uint8)[:, c:] == ((pad - (128 if shifted else 0)) & 0xff)).all()), name
        none, only = K.avgpool_quant(x, s, emit=em, want_out=False, c_pad=c_pad, pad_code=pad - (128 if shifted else 0))
        assert none is None and torch.equal(only, codes)
    with pytest.raises(ValueError):
        K.avgpool_quant(x, s, want_out=False)
    with pytest.raises(ValueError):
        K.avgpool_quant(x, s, c_pad=c_pad + 4)
    with pytest.raises(N.DlmcqError, match="no CPU fallback"):
        K.avgpool_quant(x.cpu(), s)


# ------------------------------------------------------------------------------------------------------------------ part 2
def test_ties_round_half_to_even():
    """Scale 1, windows (k, k, k + 1, k + 1): the sum is 4k + 2, the pooled value k + 0.5 exactly, the code the even neighbour."""
    k = torch.arange(0, 128, dtype=torch.float32)                        # 128 windows: one 2 x 2 window per (pixel, channel)
    x = torch.zeros(1, 8, 8, 8)
    kk = k.reshape(1, 8, 4, 4)
    x[:, :, 0::2, 0::2], x[:, :, 0::2, 1::2], x[:, :, 1::2, 0::2], x[:, :, 1::2, 1::2] = kk, kk + 1, kk, kk + 1
    want = restate(x, 2)
    assert torch.equal(want, kk + 0.5)
    one = torch.ones(1, device=DEV)
    qz = (one, None, 0, 255, N.FORM_ZEROPOINT, 0.0, False, 0)
    pooled, codes = raw(x.to(DEV).contiguous(memory_format=torch.channels_last), 2, 8, qz, True, True, 8)
    same(pooled, want.permute(0, 2, 3, 1).contiguous().to(DEV), "pooled ties")
    even = (torch.floor(kk / 2) * 2 + (kk % 2) * 2).permute(0, 2, 3, 1).to(torch.uint8)     # k even -> k, k odd -> k + 1
    assert torch.equal(even.float(), torch.round(kk + 0.5).permute(0, 2, 3, 1))             # (torch.round: half to even)
    assert torch.equal(codes.cpu(), even)
    assert torch.equal(codes, ref_codes(want, qz))


def special_inputs():
    g = torch.Generator().manual_seed(5)
    n, c, h, w = 3, 68, 7, 7
    out = {"signed_x100": torch.randn(n, c, h, w, generator=g) * 100}
    x = torch.relu(torch.randn(n, c, h, w, generator=g))
    x[1, 5] = float("nan")
    x[0, 9, 3, 2] = float("nan")
    out["nan_channel"] = x
    x = torch.relu(torch.randn(n, c, h, w, generator=g))
    x[2, 9] = float("inf")
    x[1, 11] = float("-inf")
    x[0, 13, 0, 0], x[0, 13, 0, 1] = float("inf"), float("-inf")          # inf - inf inside one window: NaN
    out["inf_channel"] = x
    out["far_outside"] = torch.randn(n, c, h, w, generator=g) * 1e30
    return out


@pytest.mark.parametrize("name", ["signed_x100", "nan_channel", "inf_channel", "far_outside"])
@pytest.mark.parametrize("s", [2, 3])
def test_special_values(name, s):
    x = special_inputs()[name]
    check_case(x.to(DEV).contiguous(memory_format=torch.channels_last), s, 68, 128, restate(x, s))


def test_a_window_of_minus_zeros_pools_to_plus_zero():
    x = torch.full((2, 8, 4, 4), -0.0)
    want = restate(x, 2)
    assert bool((bits(want) == 0).all())                                  # +0 + -0 = +0 from the first addition on
    pooled, _ = raw(x.to(DEV).contiguous(memory_format=torch.channels_last), 2, 8, quantisers()["fsptq_zeropoint_u8"], True, True, 8)
    assert bool((bits(pooled) == 0).all())
    check_case(x.to(DEV).contiguous(memory_format=torch.channels_last), 2, 8, 64, want)


# ------------------------------------------------------------------------------------------------------------------ part 3
def test_every_refusal_leaves_the_outputs_untouched():
    x = torch.zeros(2, 16, 8, 8, device=DEV).contiguous(memory_format=torch.channels_last)
    obuf = torch.full((4096,), SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full((16384,), CODE_SENTINEL, dtype=torch.uint8, device=DEV)
    sc = torch.tensor([0.01], device=DEV)
    base = dict(x=x.data_ptr(), pooled=obuf.data_ptr(), codes=cbuf.data_ptr(), n=2, h=8, w=8, c=16, xs=16, s=2, c_pad=16, pad_code=0,
                scale=sc.data_ptr(), lo=0, hi=255, form=N.FORM_ZEROPOINT)
    cases = {
        "window < 2": (dict(s=1), -1), "window > 8": (dict(s=9), -1), "H < window": (dict(h=3, s=4), -1), "W < window": (dict(w=3, s=4), -1),
        "C < 4": (dict(c=0), -1), "C % 4": (dict(c=6), -1), "x_stride < C": (dict(xs=12), -1), "x_stride % 4": (dict(xs=18), -1),
        "c_pad < C": (dict(c_pad=12), -1), "c_pad % 4": (dict(c_pad=18), -1), "both outputs NULL": (dict(pooled=None, codes=None), -1),
        "c_pad != C without codes": (dict(codes=None, c_pad=64), -1),
        "FORCE_TILED": (dict(form=N.FORM_ZEROPOINT | N.FORCE_TILED), -1), "ROUTE_ONLY": (dict(form=N.FORM_ZEROPOINT | N.ROUTE_ONLY), -1),
        "PIPELINED": (dict(form=N.FORM_ZEROPOINT | N.PIPELINED), -1), "IN_CHUNK_MAJOR": (dict(form=N.FORM_ZEROPOINT | N.FP32_IN_CHUNK_MAJOR), -1),
        "OUT_CHUNK_MAJOR": (dict(form=N.FORM_ZEROPOINT | N.FP32_OUT_CHUNK_MAJOR), -1),
        "x not 16-byte aligned": (dict(x=x.data_ptr() + 4), -4), "pooled not 16-byte aligned": (dict(pooled=obuf.data_ptr() + 8), -4),
        "codes not 4-byte aligned": (dict(codes=cbuf.data_ptr() + 2), -4),
        "an index past 2^31": (dict(n=1 << 31, h=2, w=2, c=4, xs=4, c_pad=4), -2),
    }
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731
    for what, (kw, rc) in cases.items():
        a = dict(base, **kw)
        got = N.lib.dlmcq_avgpool_nhwc_f32(p(a["x"]), p(a["pooled"]), p(a["codes"]), a["n"], a["h"], a["w"], a["c"], a["xs"], a["s"], a["c_pad"],
                                           a["pad_code"], p(a["scale"]), None, a["lo"], a["hi"], a["form"], 0.0, N.stream_ptr())
        assert got == rc, (what, got)
    a = base
    assert N.lib.dlmcq_avgpool_nhwc_f32(p(a["x"]), p(a["pooled"]), p(a["codes"]), 0, 8, 8, 16, 16, 2, 16, 0, p(a["scale"]), None, 0, 255,
                                        N.FORM_ZEROPOINT, 0.0, N.stream_ptr()) == 0                      # N == 0: nothing to do
    torch.cuda.synchronize()
    assert bool((obuf == SENTINEL).all()) and bool((cbuf == CODE_SENTINEL).all())
    with pytest.raises(N.DlmcqError):
        K.avgpool_quant(torch.zeros(2, 6, 4, 4, device=DEV), 2)          # C % 4, through the wrapper


# ------------------------------------------------------------------------------------------------------------------ part 4
from test_gpu_narrow_rows import FSPTQ_W8A8, QBASE_W8A8      # noqa: E402  (the configurations of the other plan tests)


def _net(option, cfg, qtype, batch, side, seed, offsets):
    """tests/test_gpu_pad_shortcut.py::_net for an option-C / -D network.  Every tensor a layer reads is a ReLU output, an average of ReLU
    outputs or the relu(N(0, 1)) image: minimum 0 or just above it.  The quantisers' offsets are set to exactly 0 afterwards (as
    test_gpu_gap.py does for FSPTQ), so that no layer keeps its fp32 wrapper over a minimum that is merely close to 0 - except, with
    `offsets`, on the two pooled shortcuts, which get a float offset that act_offsets=True plans."""
    import workloads as W
    from dlmc.quantization.scalar.FSPTQuant import FSPTQBase
    from dlmc.quantization.scalar.modules.base import QBase
    from dlmc.utils.merge_bn import merge_bn
    from dlmc.utils.quantize import quantize_model
    torch.manual_seed(seed)
    net = W.CifarResNet(3, option=option).to(DEV).eval()
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    net = merge_bn(net, inplace=True)
    if qtype:
        quantize_model(net, copy.deepcopy(cfg), None, qtype, int8_gemm=True)
    else:
        quantize_model(net, copy.deepcopy(cfg), None)
    x = torch.relu(torch.randn(batch, 3, side, side, device=DEV))
    with torch.no_grad():
        net(x)                                   # calibrate
    for name, m in net.named_modules():
        if isinstance(m, FSPTQBase):
            m.in_offset.zero_()
            m._zp_is_int = None
        elif isinstance(m, QBase) and m.in_offset is not None:
            m.in_offset.zero_()
            if offsets and name in ("layer2.0.downsample.1", "layer3.0.downsample.1"):
                m.in_offset.fill_(-0.03125)
    return net, x


PLAN_CASES = {"fsptq": (FSPTQ_W8A8, "FSPTQ", {}), "qbase": (QBASE_W8A8, None, {}), "qbase_act_offsets": (QBASE_W8A8, None, dict(act_offsets=True)),
              "fsptq_narrow_rows": (FSPTQ_W8A8, "FSPTQ", dict(narrow_rows=True))}


@pytest.mark.parametrize("batch, side", [(8, 32), (2, 16)])
@pytest.mark.parametrize("option", ["C", "D"])
@pytest.mark.parametrize("tag", sorted(PLAN_CASES))
def test_cifar_resnet20_plan_flag_on_equals_flag_off(tag, option, batch, side):
    from dlmc.utils.fuse import AvgPoolLayer, StreamedPlan, fuse_inference
    cfg, qtype, kw = PLAN_CASES[tag]
    net, x = _net(option, cfg, qtype, batch, side, 51 + batch, offsets="act_offsets" in kw)
    off = fuse_inference(net, **kw)
    on = fuse_inference(net, avg_pools=True, **kw)
    with torch.no_grad():
        a, b = off(x), on(x)
        again = on(x)
    ro, rn = off.fusion_report, on.fusion_report
    print(ro, rn, sep="\n")
    assert bool(torch.isfinite(a).all()) and torch.equal(b, again)
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} logits differ, max {float((a - b).abs().max())}"
    assert (ro.avg_pools, rn.avg_pools) == (0, 2) and rn.skipped == ro.skipped
    assert (rn.layers, rn.residual, rn.relu, rn.emit, rn.fp32_outputs, rn.narrow, rn.dual, rn.act_offset) == \
           (ro.layers, ro.residual, ro.relu, ro.emit, ro.fp32_outputs, ro.narrow, ro.dual, ro.act_offset)
    mods = dict(on.named_modules())
    assert not [n for n in on.graph.nodes if n.op == "call_module" and isinstance(mods[n.target], nn.AvgPool2d)]
    nodes = [m for m in on.modules() if isinstance(m, AvgPoolLayer)]
    assert sorted((m.c, m.c_pad, m.window, m.want_out) for m in nodes) == [(16, 64, 2, False), (32, 64, 2, False)]
    if "act_offsets" in kw:
        assert rn.act_offset >= 2 and all(m.emit.xoff and m.pad_code == 0 for m in nodes)
    if qtype:           # (a QBase plan's scales depend on the elements per call: StreamedPlan refuses it, with or without the flag)
        with torch.no_grad():
            assert torch.equal(StreamedPlan(on, 2)(x), b)
    else:
        with pytest.raises(ValueError):
            StreamedPlan(on, 2)


@pytest.mark.parametrize("tag", ["fsptq", "qbase"])
def test_option_b_network_gets_the_plan_it_gets_today(tag):
    from dlmc.utils.fuse import fuse_inference
    cfg, qtype, kw = PLAN_CASES[tag]
    net, x = _net("B", cfg, qtype, 4, 32, 43, offsets=False)
    off = fuse_inference(net, **kw)
    on = fuse_inference(net, avg_pools=True, **kw)
    assert repr(on.fusion_report) == repr(off.fusion_report) and on.fusion_report.avg_pools == 0
    assert [(n.op, str(n.target), tuple(str(v) for v in n.args)) for n in on.graph.nodes] == \
           [(n.op, str(n.target), tuple(str(v) for v in n.args)) for n in off.graph.nodes]
    with torch.no_grad():
        assert torch.equal(on(x), off(x))


class _Wide(nn.Module):
    """64 -> 64 convolution + ReLU, AvgPool2d(2), a 1x1 convolution on the pooled map (64 input channels: its codes travel shifted and
    unpadded) and, beside it, a plain reader of the pooled fp32 tensor."""

    def __init__(self):
        super().__init__()
        self.a = nn.Conv2d(64, 64, 3, padding=1)
        self.pool = nn.AvgPool2d(2)
        self.b = nn.Conv2d(64, 64, 1)

    def forward(self, x):
        t = self.pool(torch.relu(self.a(x)))
        return torch.relu(self.b(t)) + t


def test_unpadded_shifted_codes_beside_an_fp32_reader():
    from dlmc.quantization.scalar.FSPTQuant import FSPTQBase
    from dlmc.utils.fuse import AvgPoolLayer, fuse_inference
    from dlmc.utils.quantize import quantize_model
    torch.manual_seed(71)
    net = _Wide().to(DEV).eval()
    quantize_model(net, copy.deepcopy(FSPTQ_W8A8), None, "FSPTQ", int8_gemm=True)
    x = torch.relu(torch.randn(3, 64, 9, 9, device=DEV))                  # an odd map: the last row and column are dropped
    with torch.no_grad():
        net(x)
    for m in net.modules():
        if isinstance(m, FSPTQBase):
            m.in_offset.fill_(2.0)                                        # an integer zero point that is not 0: the shifted pad code matters nowhere, the codes do
            m._zp_is_int = None
    off, on = fuse_inference(net), fuse_inference(net, avg_pools=True)
    with torch.no_grad():
        a, b = off(x), on(x)
    assert torch.equal(a, b) and tuple(b.shape) == (3, 64, 4, 4)
    (node,) = [m for m in on.modules() if isinstance(m, AvgPoolLayer)]
    assert (node.c, node.c_pad, node.want_out, node.emit_shift, node.pad_code) == (64, 64, True, True, 2 - 128)
