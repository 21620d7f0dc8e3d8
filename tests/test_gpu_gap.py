"""Global-average-pool heads on the GPU (include/dlmcq.h: dlmcq_gap_nhwc_f32, dlmcq_conv2d_i8_nhwc_gap; fuse_inference(gap_head=...)).

Part 1: the pool kernel against a numpy restatement of its arithmetic, bit for bit, and against the float64 mean within the bound of
        recursive summation.
Part 2: the fused head kernel == conv2d_i8 (fp32 output, same epilogue) followed by the pool kernel, bit for bit.
Part 3: whole plans: gap_head="fused" == gap_head=True == gap_head="separate" bit for bit, and the fp32 map the plan WITHOUT the flag hands its pool,
        pushed through the pool kernel and the plan's own classifier node, reproduces those logits - so the head is covered without an
        empirical tolerance on logits."""
import copy
import math

import numpy as np
import pytest
import torch
from torch import nn

from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def same(a, b, what):
    """Bit equality, treating +0 and -0 as one value and every NaN as one value."""
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    if a.dtype == torch.float32:
        assert torch.equal(torch.isnan(a), torch.isnan(b)), f"{what}: NaNs in different places"
        a, b = torch.nan_to_num(a, nan=0.0) + 0.0, torch.nan_to_num(b, nan=0.0) + 0.0
        bad = a.view(torch.int32) != b.view(torch.int32)
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {a.numel()} differ"
    else:
        assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} of {a.numel()} differ"


def restate(v):
    """The three lines of the definition in numpy: v fp32 [N, HW, C] -> pooled fp32 [N, C]."""
    s = v[:, 0, :].copy()
    for p in range(1, v.shape[1]):
        s = (s + v[:, p, :]).astype(np.float32)
    return (s / np.float32(v.shape[1])).astype(np.float32)


def nhwc_rows(x):
    """(N, C, H, W) tensor -> numpy [N, HW, C] in NHWC row order."""
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n, h * w, c).cpu().numpy()


def check_bound(pooled, v):
    """|pooled - mean64(v)| <= HW * 2^-24 * mean64(|v|): the first-order bound of a recursive fp32 sum of HW terms (each of the HW - 1
    additions rounds by at most 2^-24 of a partial sum <= SUM |v|) plus the division's rounding."""
    v64 = v.astype(np.float64)
    hw = v.shape[1]
    err = np.abs(pooled.astype(np.float64) - v64.mean(axis=1))
    bound = hw * 2.0 ** -24 * np.abs(v64).mean(axis=1)
    print("  bound check: HW", hw, "max err / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert bool((err <= bound).all()), float((err - bound).max())


# ------------------------------------------------------------------------------------------------------------------ part 1
SHAPES = [(3, 68, 7, 7), (2, 64, 1, 1), (2, 128, 8, 8), (1, 4, 13, 9), (2, 2048, 7, 7)]


def quantisers():
    t = lambda v: torch.tensor([v], device=DEV)  # noqa: E731
    return {"zeropoint_u8": (t(0.004), t(3.0), 0, 255, N.FORM_ZEROPOINT, 0.0),
            "qbase_u8": (t(0.004), None, 0, 255, N.FORM_QBASE, 0.01),
            "qbase_s8": (t(0.006), None, -128, 127, N.FORM_QBASE, 0.02),
            "qbase_u8_float_offset": (t(0.003), t(-0.3), 0, 255, N.FORM_QBASE, 0.01)}


def special_inputs():
    g = torch.Generator().manual_seed(5)
    n, c, h, w = 3, 68, 7, 7
    out = {"signed_x100": torch.randn(n, c, h, w, generator=g) * 100}
    x = torch.relu(torch.randn(n, c, h, w, generator=g))
    x[1, 5, 3, 2] = float("nan")
    out["nan_channel"] = x
    x = torch.relu(torch.randn(n, c, h, w, generator=g))
    x[2, 9, 0, 6] = float("inf")
    out["inf_channel"] = x
    out["minus_zero"] = torch.full((n, c, h, w), -0.0)
    return out


def pool_case(x, finite):
    x = x.to(DEV).contiguous(memory_format=torch.channels_last)
    v = nhwc_rows(x)
    with np.errstate(invalid="ignore", over="ignore"):
        want = restate(v)
    pooled = K.global_avgpool(x)
    same(pooled, torch.from_numpy(want).to(DEV), "pooled against the numpy restatement")
    same(K.global_avgpool(x), pooled, "two calls in a row")
    if finite:
        check_bound(pooled.cpu().numpy(), v)
    for name, (s, z, lo, hi, form, g) in quantisers().items():
        ref = K.fake_quant(pooled, s, z, lo, hi, form, g=g, codes="i8", want_y=False)[1].view(torch.uint8)
        for shifted in ((False, True) if lo >= 0 else (False,)):
            em = K.EmitCodes(s, z, lo, hi, form, g, shift128=shifted)
            p2, codes = K.global_avgpool(x, emit=em)
            assert codes.dtype == em.dtype and tuple(codes.shape) == tuple(pooled.shape)
            same(p2, pooled, f"{name}: fp32 beside codes")
            same(codes.view(torch.uint8) ^ (0x80 if shifted else 0), ref, f"{name} shifted={shifted}: codes against fake_quant")
            none, only = K.global_avgpool(x, emit=em, want_out=False)
            assert none is None
            same(only, codes, f"{name} shifted={shifted}: codes-only call")
            same(K.global_avgpool(x, emit=em, want_out=False)[1], codes, f"{name}: two calls in a row")


@pytest.mark.parametrize("shape", SHAPES)
def test_pool_kernel_against_the_restatement(shape):
    g = torch.Generator().manual_seed(sum(shape))
    pool_case(torch.relu(torch.randn(*shape, generator=g)), True)


@pytest.mark.parametrize("name", ["signed_x100", "nan_channel", "inf_channel", "minus_zero"])
def test_pool_kernel_special_values(name):
    pool_case(special_inputs()[name], name in ("signed_x100", "minus_zero"))


def test_pool_kernel_refuses_what_it_does_not_take():
    x = torch.zeros(2, 6, 3, 3, device=DEV).contiguous(memory_format=torch.channels_last)
    with pytest.raises(N.DlmcqError):
        K.global_avgpool(x)                       # C % 4
    with pytest.raises(ValueError):
        K.global_avgpool(torch.zeros(2, 8, 3, 3, device=DEV), want_out=False)
    with pytest.raises(N.DlmcqError, match="no CPU fallback"):
        K.global_avgpool(torch.zeros(2, 8, 3, 3))


# ------------------------------------------------------------------------------------------------------------------ part 2
def head_operands(n, c, k, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    u8 = torch.randint(0, 256, (n, c, h, w), generator=g, dtype=torch.int16)
    wf = torch.randn(k, c, 1, 1, generator=g) * math.sqrt(2 / c)
    sw = (wf.abs().amax(dim=(1, 2, 3)) / 127 + 1e-6).to(DEV)
    wq, wsum = K.quantize_weight_krsc(wf.to(DEV), sw, -127, 127)
    bias = torch.randn(k, generator=g).to(DEV)
    res = torch.randn(n, k, h, w, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    return u8, wq, wsum, sw, bias, res


def code_kinds(u8):
    """The same activation as unsigned codes (zero point 3), as shifted codes (int8 `code - 128`, zero point 3 - 128) and - other
    integers - as signed codes (zero point -5)."""
    cl = lambda t: t.to(DEV).contiguous(memory_format=torch.channels_last)  # noqa: E731
    t = lambda v: torch.tensor([v], device=DEV)  # noqa: E731
    return {"u8": (cl(u8.to(torch.uint8)), t(3.0)), "shifted": (cl((u8 - 128).to(torch.int8)), t(3.0 - 128.0)),
            "s8": (cl((u8 - 131).clamp(-128, 127).to(torch.int8)), t(-5.0))}


@pytest.mark.parametrize("hw", [(7, 7), (8, 8), (4, 4), (1, 1)])
@pytest.mark.parametrize("ck", [(64, 64), (192, 128), (512, 256)])
def test_fused_head_equals_convolution_then_pool(ck, hw):
    (c, k), (h, w) = ck, hw
    s_in = torch.tensor([0.02], device=DEV)
    em = K.EmitCodes(torch.tensor([0.05], device=DEV), torch.tensor([2.0], device=DEV), 0, 255, N.FORM_ZEROPOINT)
    em_off = K.EmitCodes(torch.tensor([0.05], device=DEV), torch.tensor([-0.7], device=DEV), 0, 255, N.FORM_QBASE, 0.01, shift128=True)
    routes = {}
    for n in (1, 5):
        u8, wq, wsum, sw, bias, res = head_operands(n, c, k, h, w, seed=c + h + n)
        # a bias folded from a float offset o = -0.75 of the input quantiser (an unpadded layer has no border term)
        tap = wq.reshape(k, c).double().sum(dim=1) * sw.double()
        folded = (bias.double() + (-0.75) * tap).float()
        for kind, (codes, zp) in code_kinds(u8).items():
            for shortcut in (None, res):
                for act in (N.ACT_NONE, N.ACT_RELU, N.ACT_RELU6):
                    for b, e in ((bias, em), (None, em)) + (((folded, em_off),) if kind == "u8" and act == N.ACT_RELU6 else ()):
                        what = f"C{c} K{k} {h}x{w} N{n} {kind} shortcut={shortcut is not None} act={act} bias={b is not None}"
                        full = K.conv2d_i8(codes, wq, wsum, b, s_in, zp, sw, residual=shortcut, act=act)
                        want, want_codes = K.global_avgpool(full, emit=e)
                        got, got_codes = K.conv2d_i8_gap(codes, wq, wsum, b, s_in, zp, sw, residual=shortcut, act=act, emit=e)
                        same(got, want, what + ": pooled fp32")
                        same(got_codes, want_codes, what + ": codes")
                        routes[what] = (float(want.abs().max()), int(want_codes.view(torch.uint8).max()))
                        if b is bias:
                            main_codes = got_codes
                    none, only = K.conv2d_i8_gap(codes, wq, wsum, bias, s_in, zp, sw, residual=shortcut, act=act, emit=em, want_out=False)
                    assert none is None
                    same(only, main_codes, what + ": codes-only call")
                    same(K.conv2d_i8_gap(codes, wq, wsum, bias, s_in, zp, sw, residual=shortcut, act=act), K.global_avgpool(
                        K.conv2d_i8(codes, wq, wsum, bias, s_in, zp, sw, residual=shortcut, act=act)), what + ": fp32-only call")
    assert all(mx > 0 and cmax > 2 for mx, cmax in routes.values()), "degenerate case: nothing to compare"


def test_fused_head_refusals_and_route():
    u8, wq, wsum, sw, bias, _ = head_operands(2, 64, 64, 9, 9, seed=1)
    codes, zp = code_kinds(u8)["u8"]
    s_in = torch.tensor([0.02], device=DEV)
    with pytest.raises(N.DlmcqError, match="invalid argument"):
        K.conv2d_i8_gap(codes, wq, wsum, bias, s_in, zp, sw)                       # H W = 81
    u8, wq, wsum, sw, bias, _ = head_operands(2, 64, 96, 7, 7, seed=2)
    codes, zp = code_kinds(u8)["u8"]
    with pytest.raises(N.DlmcqError, match="invalid argument"):
        K.conv2d_i8_gap(codes, wq, wsum, bias, s_in, zp, sw)                       # K = 96
    # DLMCQ_ROUTE_ONLY answers DLMCQ_ROUTE_GAP and launches nothing: the output keeps its sentinel
    u8, wq, wsum, sw, bias, _ = head_operands(2, 64, 64, 7, 7, seed=3)
    codes, zp = code_kinds(u8)["u8"]
    out = torch.full((2, 64), 7.5, device=DEV)
    args = (N.ptr(codes), N.ptr(wq), N.ptr(out), N.ptr(bias), N.ptr(wsum), N.ptr(s_in), N.ptr(zp), N.ptr(sw), 2, 7, 7, 64, 64, 1, None, 0,
            None, None, None, 0, 0)
    assert N.lib.dlmcq_conv2d_i8_nhwc_gap(*args, N.ROUTE_ONLY, 0.0, N.stream_ptr()) == N.ROUTE_GAP
    torch.cuda.synchronize()
    assert bool((out == 7.5).all())
    assert N.lib.dlmcq_conv2d_i8_nhwc_gap(*args, N.ROUTE_ONLY | N.FORCE_TILED, 0.0, N.stream_ptr()) == -1
    assert N.lib.dlmcq_conv2d_i8_nhwc_gap(*args, 0, 0.0, N.stream_ptr()) == 0
    torch.cuda.synchronize()
    same(out, K.global_avgpool(K.conv2d_i8(codes, wq, wsum, bias, s_in, zp, sw)), "the real call after the route query")


# ------------------------------------------------------------------------------------------------------------------ part 3
FSPTQ_W8A8 = {"weight": {"enable": True, "type": "minmax_channel", "args": {"n_bits": 8, "signed": True}},
              "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
              "exclude_layers": [], "override_options": []}
QBASE_W8A8 = {"weight": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": True}},
              "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
              "exclude_layers": [], "override_options": []}
PLANS = {  # name: (workload, family, fuse_inference arguments, the head's kind under gap_head="fused"; True leaves the measured-slower layers out)
    "resnet50_fsptq": ("resnet50", "FSPTQ", {}, "fused"),
    "mobilenet_v2_fsptq": ("mobilenet_v2", "FSPTQ", {}, "fused"),
    "mobilenet_v2_qbase_offsets": ("mobilenet_v2", "QBase", {"act_offsets": True}, "fused"),
    "repvgg_a1_fsptq": ("repvgg_a1", "FSPTQ", {}, "separate"),
}


def calibrated(workload, family):
    import workloads as W
    from dlmc.quantization.scalar.FSPTQuant import FSPTQBase
    from dlmc.utils.merge_bn import merge_bn
    from dlmc.utils.quantize import quantize_model
    torch.manual_seed(31)
    net = W.MODELS[workload]().to(DEV).eval()
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    net = merge_bn(net, inplace=True, allow_missing=True)
    if family == "FSPTQ":
        quantize_model(net, copy.deepcopy(FSPTQ_W8A8), None, "FSPTQ", int8_gemm=True)
    else:
        quantize_model(net, copy.deepcopy(QBASE_W8A8), None)
    x = torch.relu(torch.randn(2, 3, 224, 224, device=DEV))
    with torch.no_grad():
        net(x)                                   # calibrate
    # FSPTQ's zero point of a tensor whose minimum is not 0 (the pooled post-ReLU tensor the classifier reads, MobileNetV2's linear
    # bottleneck outputs) is no integer and the layer would keep its fp32 wrapper.  The zero points are set to 0 (quantisers like any
    # other, as in test_gpu_relu6.py's forced case and the host-side dry runs): every layer on the plan, which is what is tested
    for m in net.modules():
        if isinstance(m, FSPTQBase):
            m.in_offset.zero_()
            m._zp_is_int = None
    return net, x


@pytest.mark.parametrize("name", sorted(PLANS))
def test_plans_with_gap_heads(name):
    from dlmc.utils import fuse as FU
    from dlmc.utils.graph import GraphedForward
    workload, family, kw, kind = PLANS[name]
    net, x = calibrated(workload, family)
    off, sep, fus, tru = (FU.fuse_inference(net, gap_head=flag, **kw) for flag in (False, "separate", "fused", True))
    print(name, fus.fusion_report)
    assert off.fusion_report.gap_heads == []
    assert [k for _, k in sep.fusion_report.gap_heads] == ["separate"] and [k for _, k in fus.fusion_report.gap_heads] == [kind]
    assert [k for _, k in tru.fusion_report.gap_heads] == ["separate"]        # (all four last layers: measured slower, or not built)
    assert fus.fusion_report.fp32_outputs == off.fusion_report.fp32_outputs - (kind == "fused")
    seen = {}
    pool = next(m for m in off.modules() if isinstance(m, nn.AdaptiveAvgPool2d))
    hook = pool.register_forward_hook(lambda mod, i, o: seen.__setitem__("map", i[0].detach().clone()))
    with torch.no_grad():
        base = off(x)
        hook.remove()
        want = sep(x)
        got = fus(x)
        same(got, want, "gap_head='fused' against gap_head='separate'")
        same(tru(x), want, "gap_head=True against gap_head='separate'")
        assert bool(torch.isfinite(got).all()) and got.shape == base.shape
        same(GraphedForward(sep, x)(x), want, "graphed, separate")
        same(GraphedForward(fus, x)(x), want, "graphed, fused")
        # the map the plan without the flag pools -> the pool kernel -> the plan's own classifier node: the same logits
        fmap = seen["map"]
        assert fmap.dim() == 4 and fmap.shape[2] * fmap.shape[3] == 49
        gap = next(m for m in sep.modules() if isinstance(m, FU.GapLayer))
        fc = next(m for m in sep.modules() if isinstance(m, FU.Int8Layer) and m.layer.weight.dim() == 2)
        pooled, codes = K.global_avgpool(fmap, emit=gap.emit.emit(fmap.shape[0] * fmap.shape[1]))
        same(fc(codes)[0], want, "pool kernel + classifier node on the flag-off plan's map")
    check_bound(pooled.cpu().numpy(), nhwc_rows(fmap))
    same(pooled, torch.from_numpy(restate(nhwc_rows(fmap))).to(DEV), "pooled against the numpy restatement")
