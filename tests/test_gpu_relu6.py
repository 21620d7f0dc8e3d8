"""ReLU6 (DLMCQ_ACT_RELU6) in the fused epilogues and in the frozen plan: every kernel that implements it must give exactly what the
same call without an activation, followed by F.relu6 and the separate quantise kernel, gives - fp32 bit for bit (up to the sign of
zero), codes exactly; the entry points without it refuse it; a plan that fuses ReLU6 computes what the plan that keeps it a separate
op computes."""
import copy
import os
import re

import pytest
import torch
import torch.nn.functional as F
from torch import nn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def gen(seed):
    return torch.Generator().manual_seed(4242 + seed)


def same(a, b, what):
    """Bit equality, treating +0 and -0 as one value."""
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.dtype == torch.float32:
        a, b = a + 0.0, b + 0.0
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
            f"{what}: {(a.view(torch.int32) != b.view(torch.int32)).sum().item()} of {a.numel()} differ"
    else:
        assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} of {a.numel()} differ"


def tagged(K, fn):
    """fn() with the launch profile on: (result, tags of the launches it made - the library's own routing answer)."""
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        r = fn()
    finally:
        K.PROFILE.enabled = False
    tags = [rec[0] for rec in K.PROFILE.records]
    K.PROFILE.reset()
    return r, tags


# values around the bound, reached through the bias of channels whose weights are all zero (their output IS the bias)
EDGE = [6.0, float(torch.nextafter(torch.tensor(6.0), torch.tensor(0.0))), float(torch.nextafter(torch.tensor(6.0), torch.tensor(7.0))),
        float("nan"), float("inf"), -float("inf"), -0.0, 0.0, -1e-30, 5.99, 6.01, 1e30]


def quantisers():
    """(tag, EmitCodes args) of the consumer quantisers: the FSPTQ unsigned byte (the plain quantiser), QBase's unsigned byte with its
    grad_scale, and a signed zero-point form.  Scales set so that code(6) lies well inside [lo, hi): ReLU6 is visible in the codes."""
    from dlmc import _native as N
    return [("fsptq_u8", (torch.tensor([0.04], device=DEV), None, 0, 255, N.FORM_ZEROPOINT, 0.0)),
            ("qbase_u8", (torch.tensor([0.04], device=DEV), None, 0, 255, N.FORM_QBASE, 1e-3)),
            ("zeropoint_s8", (torch.tensor([0.06], device=DEV), torch.tensor([-5.0], device=DEV), -127, 127, N.FORM_ZEROPOINT, 0.0))]


def expect(K, pre, emit_args):
    want = F.relu6(pre)
    s, z, lo, hi, form, g = emit_args
    _, codes = K.fake_quant(want, s, z, lo, hi, form, g=g, codes="i8", want_y=False)
    return want, codes


def weights(gg, k, c, r, zero):
    wt = torch.randn(k, c, r, r, generator=gg) * 0.08
    wt[:zero] = 0.0
    bias = torch.randn(k, generator=gg) * 4.0
    bias[:len(EDGE)] = torch.tensor(EDGE)
    return wt.to(DEV), bias.to(DEV)


CONV_CASES = [  # N, C, H, W, K, R, stride, pad, asym, route of the codes-only call
    (4, 64, 32, 32, 128, 1, 1, 0, False, "conv_pw"),      # weight-resident pointwise kernel (plain quantiser)
    (4, 64, 32, 32, 192, 1, 1, 0, True, "conv_pw"),
    (2, 64, 9, 9, 64, 1, 1, 0, False, "conv_i8"),         # tiled, swapped epilogue
    (2, 128, 10, 10, 256, 3, 1, 1, False, "conv_i8"),     # would be the halo-tile kernel with ReLU: not with ReLU6
    (3, 64, 14, 14, 128, 3, 2, 1, True, "conv_i8"),
    (2, 64, 9, 9, 42, 3, 1, 1, False, "conv_i8"),         # K % 4 != 0: scalar epilogue
    (2, 64, 8, 8, 192, 1, 1, 0, True, "conv_i8"),         # 192-wide asymmetric tiles
]


@pytest.mark.parametrize("case", range(len(CONV_CASES)))
def test_relu6_conv_kernels(case):
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    n, c, h, w, k, r, stride, pad, asym, route = CONV_CASES[case]
    gg = gen(case)
    codes = torch.randint(0, 256, (n, c, h, w), generator=gg).to(torch.uint8).to(DEV).contiguous(memory_format=torch.channels_last)
    wt, bias = weights(gg, k, c, r, len(EDGE))
    s_w = wt.abs().amax(dim=(1, 2, 3)) / 127 + 1e-6
    wq, wsum = K.quantize_weight_krsc(wt, s_w, -127, 127)
    w_off = None
    if asym:
        w_off = (torch.randn(k, generator=gg) * 0.002).to(DEV)
        w_off[:len(EDGE)] = 0.0
    s_in, zp_in = torch.tensor([0.02], device=DEV), torch.tensor([2.0], device=DEV)
    kw = dict(stride=stride, padding=pad, w_offset=w_off)
    pre = K.conv2d_i8(codes, wq, wsum, bias, s_in, zp_in, s_w, act=N.ACT_NONE, **kw)
    assert bool((pre > 6).any()) and bool((pre < 0).any()) and bool(pre.isnan().any())
    for qtag, qa in quantisers():
        want, want_codes = expect(K, pre, qa)
        emit = K.EmitCodes(*qa)
        tag = f"case {case} {qtag}"
        assert bool(((want_codes.to(torch.int32) > qa[2]) & (want_codes.to(torch.int32) < qa[3])).any())
        out, got = K.conv2d_i8(codes, wq, wsum, bias, s_in, zp_in, s_w, act=N.ACT_RELU6, emit=emit, **kw)
        same(out, want, tag + " out")
        same(got, want_codes, tag + " codes")
        same(K.conv2d_i8(codes, wq, wsum, bias, s_in, zp_in, s_w, act=N.ACT_RELU6, **kw), want, tag + " out only")
        (none, only), tags = tagged(K, lambda: K.conv2d_i8(codes, wq, wsum, bias, s_in, zp_in, s_w, act=N.ACT_RELU6, emit=emit,
                                                           want_out=False, **kw))
        assert none is None
        same(only, want_codes, tag + " codes only")
        if qtag == "fsptq_u8" or route == "conv_i8":
            assert tags == [route], (tag, tags)
        _, tiled = K.conv2d_i8(codes, wq, wsum, bias, s_in, zp_in, s_w, act=N.ACT_RELU6, emit=emit, want_out=False, force_tiled=True, **kw)
        same(tiled, want_codes, tag + " codes only, tiled")
        if asym is False and r == 1:         # the observing entry point takes it too
            o2 = K.conv2d_i8(codes, wq, wsum, bias, s_in, zp_in, s_w, act=N.ACT_RELU6, observe=True, **kw)
            same(o2, want, tag + " observed")
    # ReLU keeps its meaning
    same(K.conv2d_i8(codes, wq, wsum, bias, s_in, zp_in, s_w, relu=True, **kw), torch.relu(pre), f"case {case} relu")


def test_relu6_pipelined_3x3_falls_back_to_the_tiled_kernel():
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    gg = gen(50)
    n, c, h, w, k = 48, 128, 56, 56, 128
    codes = torch.randint(0, 256, (n, c, h, w), generator=gg).to(torch.uint8).to(DEV).contiguous(memory_format=torch.channels_last)
    wt, bias = weights(gg, k, c, 3, len(EDGE))
    s_w = wt.abs().amax(dim=(1, 2, 3)) / 127 + 1e-6
    wq, wsum = K.quantize_weight_krsc(wt, s_w, -127, 127)
    s_in, zp_in = torch.tensor([0.02], device=DEV), torch.tensor([2.0], device=DEV)
    qa = quantisers()[0][1]
    pre = K.conv2d_i8(codes, wq, wsum, bias, s_in, zp_in, s_w, padding=1)
    _, want_codes = expect(K, pre, qa)
    (_, got), tags = tagged(K, lambda: K.conv2d_i8(codes, wq, wsum, bias, s_in, zp_in, s_w, padding=1, act=N.ACT_RELU6, emit=K.EmitCodes(*qa),
                                                   want_out=False, pipelined=True))
    assert tags == ["conv_i8"], tags
    same(got, want_codes, "pipelined request with ReLU6")


def test_relu6_block_end_does_not_take_the_pwr_kernel():
    """A 1x1 block end with an fp32 shortcut emitting plain codes: the block-end kernel with ReLU, the tiled kernel with ReLU6."""
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    gg = gen(60)
    n, c, h, w, k = 32, 256, 14, 14, 256
    codes = torch.randint(0, 256, (n, c, h, w), generator=gg).to(torch.uint8).to(DEV).contiguous(memory_format=torch.channels_last)
    wt, bias = weights(gg, k, c, 1, len(EDGE))
    s_w = wt.abs().amax(dim=(1, 2, 3)) / 127 + 1e-6
    wq, wsum = K.quantize_weight_krsc(wt, s_w, -127, 127)
    s_in, zp_in = torch.tensor([0.02], device=DEV), torch.tensor([0.0], device=DEV)
    res = (torch.randn(n, k, h, w, generator=gg) * 3).to(DEV).contiguous(memory_format=torch.channels_last)
    qa = quantisers()[0][1]
    emit = K.EmitCodes(*qa)
    pre = K.conv2d_i8(codes, wq, wsum, bias, s_in, zp_in, s_w, residual=res)
    _, tags = tagged(K, lambda: K.conv2d_i8(codes, wq, wsum, bias, s_in, zp_in, s_w, residual=res, relu=True, emit=emit))
    assert tags == ["conv_pwr"], tags                   # (the shape is one the block-end kernel takes)
    want, want_codes = expect(K, pre, qa)
    (out, got), tags = tagged(K, lambda: K.conv2d_i8(codes, wq, wsum, bias, s_in, zp_in, s_w, residual=res, act=N.ACT_RELU6, emit=emit))
    assert tags == ["conv_i8"], tags
    same(out, want, "block end out")
    same(got, want_codes, "block end codes")


DW_CASES = [  # N, C, H, W, R, stride, pad, asym, force_tiled, route of the codes-only call
    (4, 64, 32, 32, 3, 1, 1, False, False, "conv_dwm"),   # matrix-core depthwise kernel
    (4, 128, 32, 32, 3, 1, 1, True, False, "conv_dwm"),
    (2, 64, 15, 15, 3, 1, 1, False, True, "conv_dw"),     # two pixels per thread
    (2, 64, 15, 15, 3, 1, 1, True, True, "conv_dw"),
    (2, 96, 16, 16, 3, 2, 1, True, False, "conv_dw"),     # one pixel per thread (stride 2)
    (2, 48, 16, 16, 3, 2, 1, False, False, "conv_dw"),
    (2, 20, 9, 9, 5, 1, 2, True, False, "conv_dw"),       # any R, S: the generic kernel
]


@pytest.mark.parametrize("case", range(len(DW_CASES)))
def test_relu6_depthwise_kernels(case):
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    n, c, h, w, r, stride, pad, asym, force, route = DW_CASES[case]
    gg = gen(100 + case)
    codes = torch.randint(0, 256, (n, c, h, w), generator=gg).to(torch.uint8).to(DEV).contiguous(memory_format=torch.channels_last)
    wq = torch.randint(-127, 128, (r, r, c), generator=gg).to(torch.int8)
    wq[:, :, :len(EDGE)] = 0
    wq = wq.to(DEV)
    s_w = (torch.rand(c, generator=gg) * 0.01 + 0.002).to(DEV)
    bias = (torch.randn(c, generator=gg) * 4.0)
    bias[:len(EDGE)] = torch.tensor(EDGE)
    bias = bias.to(DEV)
    w_off = None
    if asym:
        w_off = (torch.randn(c, generator=gg) * 0.002).to(DEV)
        w_off[:len(EDGE)] = 0.0
    s_in, zp_in = torch.tensor([0.02], device=DEV), torch.tensor([2.0], device=DEV)
    kw = dict(w_offset=w_off, stride=stride, padding=pad)
    pre = K.conv2d_dw_i8(codes, wq, bias, s_in, zp_in, s_w, act=N.ACT_NONE, **kw)
    assert bool((pre > 6).any()) and bool((pre < 0).any()) and bool(pre.isnan().any())
    for qtag, qa in quantisers():
        want, want_codes = expect(K, pre, qa)
        emit = K.EmitCodes(*qa)
        tag = f"dw case {case} {qtag}"
        out, got = K.conv2d_dw_i8(codes, wq, bias, s_in, zp_in, s_w, act=N.ACT_RELU6, emit=emit, **kw)
        same(out, want, tag + " out")
        same(got, want_codes, tag + " codes")
        (none, only), tags = tagged(K, lambda: K.conv2d_dw_i8(codes, wq, bias, s_in, zp_in, s_w, act=N.ACT_RELU6, emit=emit, want_out=False,
                                                              force_tiled=force, **kw))
        assert none is None
        same(only, want_codes, tag + " codes only")
        if qtag == "fsptq_u8" or route == "conv_dw":
            assert tags == [route], (tag, tags)
    same(K.conv2d_dw_i8(codes, wq, bias, s_in, zp_in, s_w, relu=True, **kw), torch.relu(pre), f"dw case {case} relu")


STEM_CASES = [  # N, C, H, W, K, R, stride, pad, asym
    (2, 3, 32, 32, 64, 3, 2, 1, False),     # MobileNetV2's first layer: codes only -> the swapped epilogue
    (2, 3, 32, 32, 64, 3, 2, 1, True),
    (2, 3, 32, 32, 64, 7, 2, 3, False),
    (3, 3, 17, 23, 96, 3, 2, 1, True),
]


@pytest.mark.parametrize("case", range(len(STEM_CASES)))
def test_relu6_stem_kernels(case):
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    n, c, h, w, k, r, stride, pad, asym = STEM_CASES[case]
    gg = gen(200 + case)
    x = torch.rand(n, c, h, w, generator=gg).to(DEV)
    s_x, zp_x = torch.tensor([1 / 255], device=DEV), torch.tensor([0.0], device=DEV)
    xpad = K.quantize_pad_nhwc4(x, s_x, zp_x, 0, 255, N.FORM_ZEROPOINT, pad)
    wt, bias = weights(gg, k, c, r, len(EDGE))
    wt = wt * 20
    s_w = wt.abs().amax(dim=(1, 2, 3)) / 127 + 1e-6
    wq, wsum = K.quantize_weight_stem(wt, s_w, -127, 127)
    w_off = None
    if asym:
        w_off = (torch.randn(k, generator=gg) * 0.05).to(DEV)
        w_off[:len(EDGE)] = 0.0
    kw = dict(stride=stride, w_offset=w_off, channels=c)
    pre = K.conv2d_i8_stem(xpad, wq, wsum, bias, s_x, zp_x, s_w, r, act=N.ACT_NONE, **kw)
    assert bool((pre > 6).any()) and bool((pre < 0).any()) and bool(pre.isnan().any())
    for qtag, qa in quantisers():
        want, want_codes = expect(K, pre, qa)
        emit = K.EmitCodes(*qa)
        tag = f"stem case {case} {qtag}"
        out, got = K.conv2d_i8_stem(xpad, wq, wsum, bias, s_x, zp_x, s_w, r, act=N.ACT_RELU6, emit=emit, **kw)
        same(out, want, tag + " out")
        same(got, want_codes, tag + " codes")
        none, only = K.conv2d_i8_stem(xpad, wq, wsum, bias, s_x, zp_x, s_w, r, act=N.ACT_RELU6, emit=emit, want_out=False, **kw)
        assert none is None
        same(only, want_codes, tag + " codes only")
    same(K.conv2d_i8_stem(xpad, wq, wsum, bias, s_x, zp_x, s_w, r, relu=True, **kw), torch.relu(pre), f"stem case {case} relu")


def _act_positions(fname):
    """Indices of the activation arguments (relu / relu2 / relu3 / dw_relu) of an entry point, read from include/dlmcq.h."""
    header = open(os.path.join(ROOT, "include", "dlmcq.h")).read()
    m = re.search(r"\bint " + fname + r"\((.*?)\);", header, re.S)
    names = [re.split(r"[\s*]+", p.strip())[-1] for p in m.group(1).split(",")]
    return [i for i, nm in enumerate(names) if nm in ("relu", "relu2", "relu3", "dw_relu")]


REFUSING = ["dlmcq_conv2d_i8_nhwc_dual", "dlmcq_conv2d_i8_nhwc_chain", "dlmcq_conv2d_i8_nhwc_dual_chain", "dlmcq_conv2d_dwpw_i8_nhwc",
            "dlmcq_conv2d_i8_stem_pool_fused"]


def test_entry_points_without_relu6_refuse_it(monkeypatch):
    """Each call the plans make to an entry point without ReLU6 is made again first with DLMCQ_ACT_RELU6 in each activation argument:
    DLMCQ_EINVAL, and nothing launched (the real call that follows still gives the plan's result)."""
    import workloads as W
    from dlmc import _native as N
    from dlmc.utils.fuse import fuse_inference
    from dlmc.utils.merge_bn import merge_bn
    from dlmc.utils.quantize import quantize_model
    seen = {f: [] for f in REFUSING}
    for fname in REFUSING:
        orig, pos = getattr(N.lib, fname), _act_positions(fname)
        assert pos

        def wrapper(*args, orig=orig, pos=pos, fname=fname):
            for p in pos:
                bad = list(args)
                bad[p] = N.ACT_RELU6
                seen[fname].append(orig(*bad))
            return orig(*args)
        monkeypatch.setattr(N.lib, fname, wrapper)
    fsptq = {"weight": {"enable": True, "type": "minmax_channel", "args": {"n_bits": 8, "signed": True}},
             "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
             "exclude_layers": [], "override_options": []}
    torch.manual_seed(7)
    x = torch.relu(torch.randn(4, 3, 96, 96, device=DEV))
    for name, kw in (("resnet50", {}), ("mobileone_s1", {"dwpw": True})):
        net = merge_bn(W.MODELS[name]().to(DEV).eval(), inplace=True, allow_missing=True)
        quantize_model(net, copy.deepcopy(fsptq), None, "FSPTQ", int8_gemm=True)
        with torch.no_grad():
            want = net(x)
            got = fuse_inference(net, **kw)(x)
        assert got.shape == want.shape
    for fname, rcs in seen.items():
        assert rcs, f"{fname} was not called by the plans"
        assert all(rc == EINVAL for rc in rcs), (fname, rcs)


FSPTQ_W8A8 = {"weight": {"enable": True, "type": "minmax_channel", "args": {"n_bits": 8, "signed": True}},
              "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
              "exclude_layers": [], "override_options": []}
# the QBase configuration whose wrappers run on the int8 route (per-tensor symmetric weights): the wrapper path is then the same arithmetic
QBASE_W8A8 = {"weight": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": True}},
              "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": True}},
              "exclude_layers": [], "override_options": []}
QBASE_W4A8 = {"weight": {"enable": True, "type": "minmax_channel", "args": {"n_bits": 4, "signed": False}},
              "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
              "exclude_layers": [], "override_options": []}


def _mobilenet(family, batch, forced):
    import workloads as W
    from dlmc.quantization.scalar.FSPTQuant import FSPTQBase
    from dlmc.quantization.scalar.modules.base import QBase
    from dlmc.utils.merge_bn import merge_bn
    from dlmc.utils.quantize import quantize_model
    torch.manual_seed(31)
    net = W.mobilenet_v2().to(DEV).eval()
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    net = merge_bn(net, inplace=True)
    if family == "FSPTQ":
        quantize_model(net, copy.deepcopy(FSPTQ_W8A8), None, "FSPTQ", int8_gemm=True)
    else:
        quantize_model(net, copy.deepcopy(QBASE_W4A8), None)
    x = torch.relu(torch.randn(batch, 3, 224, 224, device=DEV))
    with torch.no_grad():
        net(x)                                   # calibrate
    if forced:       # every layer but the first reads its input with code(6) = 150 of [0, 255]: ReLU6's bound shows in the codes
        first = True
        for m in net.modules():
            if isinstance(m, (FSPTQBase, QBase)):
                if not first:
                    m.in_scale.data.fill_(0.04)
                    if getattr(m, "in_offset", None) is not None:
                        m.in_offset.zero_()
                first = False
    return net, x


@pytest.mark.parametrize("family", ["FSPTQ", "QBase"])
@pytest.mark.parametrize("batch", [8, 256])
@pytest.mark.parametrize("forced", [False, True])
def test_mobilenet_v2_plan_with_and_without_relu6_fusion(family, batch, forced):
    from dlmc.utils.fuse import fuse_inference
    from dlmc.utils.graph import GraphedForward
    net, x = _mobilenet(family, batch, forced)
    x = x * 0.8
    fused, sep = fuse_inference(net), fuse_inference(net, relu6=False)
    rf, rs = fused.fusion_report, sep.fusion_report
    print(family, batch, forced, rf, rs)
    assert (rf.layers, rf.skipped, rf.relu, rf.residual) == (rs.layers, rs.skipped, rs.relu, rs.residual) and rs.relu6 == 0
    if forced:       # (integer zero points everywhere: every layer on the int8 route, as in the host-side dry run)
        assert (rf.layers, rf.relu6, rf.relu, rf.residual, rf.skipped) == (53, 35, 0, 3, [])
        assert (rs.emit, rs.fp32_outputs) == (10, 50)
        if family == "FSPTQ":
            assert (rf.emit, rf.fp32_outputs) == (44, 16)
    else:            # (calibrated: the expansions read the shortcut sums - negative minimum, non-integer zero point - on their fp32 path)
        assert rf.relu6 >= 18 and rf.emit > rs.emit
    with torch.no_grad():
        want = sep(x)
        got = fused(x)
    same(got, want, f"{family} b{batch} forced={forced} logits")
    assert bool(torch.isfinite(got).all())
    same(GraphedForward(fused, x)(x), want, f"{family} b{batch} forced={forced} graphed")


class Net64(nn.Module):
    """MobileNetV2-shaped, every channel count a multiple of 64 (no padded layer, every shortcut add absorbed)."""

    def __init__(self):
        import workloads as W
        super().__init__()
        self.features = nn.Sequential(W._conv_bn_relu6(3, 64, 3, stride=2), W.InvertedResidual(64, 64, 1, 1),
                                      W.InvertedResidual(64, 64, 1, 6), W.InvertedResidual(64, 128, 2, 6),
                                      W.InvertedResidual(128, 128, 1, 6), W._conv_bn_relu6(128, 256, 1))
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(256, 10)

    def forward(self, x):
        return self.fc(torch.flatten(self.pool(self.features(x)), 1))


@pytest.mark.parametrize("family", ["FSPTQ", "QBase"])
def test_relu6_plan_is_bit_identical_to_the_wrappers(family):
    from dlmc.utils.fuse import fuse_inference
    from dlmc.utils.merge_bn import merge_bn
    from dlmc.utils.quantize import quantize_model
    torch.manual_seed(5)
    net = Net64().to(DEV).eval()
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    net = merge_bn(net, inplace=True)
    if family == "FSPTQ":
        quantize_model(net, copy.deepcopy(FSPTQ_W8A8), None, "FSPTQ", int8_gemm=True)
    else:
        quantize_model(net, copy.deepcopy(QBASE_W8A8), None, int8_gemm=True)
    x = torch.relu(torch.randn(4, 3, 64, 64, device=DEV))
    with torch.no_grad():
        net(x)
        want = net(x * 0.8)
        fused = fuse_inference(net)
        got = fused(x * 0.8)
    rep = fused.fusion_report
    print(family, rep)
    assert rep.relu6 >= 5
    same(got, want, f"{family} wrappers vs plan")


def test_eager_fused_still_matches_the_model_on_mobilenet_v2():
    """EagerFused knows ReLU alone: on MobileNetV2 it must not fold a ReLU6 as a ReLU."""
    import workloads as W
    from dlmc.utils.fuse import EagerFused
    from dlmc.utils.merge_bn import merge_bn
    from dlmc.utils.quantize import quantize_model
    torch.manual_seed(11)
    net = W.mobilenet_v2().to(DEV).eval()
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    net = merge_bn(net, inplace=True)
    quantize_model(net, copy.deepcopy(FSPTQ_W8A8), None, "FSPTQ", int8_gemm=True)
    twin = copy.deepcopy(net)
    x = torch.relu(torch.randn(4, 3, 96, 96, device=DEV))
    with torch.no_grad():
        want0 = net(x)
        fused = EagerFused(twin)
        got0 = fused(x)
        same(got0, want0, "calibrating forward")
        same(fused(x * 0.7), net(x * 0.7), "second forward")
