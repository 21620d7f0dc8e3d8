"""Float activation offsets on the int8 kernels (the *_xoff entry points, fuse_inference(act_offsets=True)).

Exact constructions in the manner of tests/exact_layers.py: codes 0..7, a dyadic scale and offset, weights in {-1, 0, 1} with dyadic
per-channel scales (and offsets), dyadic biases - every value of the float64 convolution of x^ = q * s + o (zero padding: x^ = 0) is an
fp32 number, so the kernel's fp32 output must equal it bit for bit and its codes must equal the quantiser's codes of that output byte
for byte.  Border classes: corners, edges, images smaller than the filter's reach, stride 2, dilation 2."""
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OFF = -0.75        # o
S_IN = 0.5         # s^


def same(a, b, what):
    """Bit equality, treating +0 and -0 as one value."""
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.dtype == torch.float32:
        a, b = a + 0.0, b + 0.0
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
            f"{what}: {(a.view(torch.int32) != b.view(torch.int32)).sum().item()} of {a.numel()} differ"
    else:
        assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} of {a.numel()} differ"


def operands(n, c, h, w, k, r, s, asym, groups=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 8, (n, c, h, w), generator=g, dtype=torch.int16)
    cin = c // groups
    qw = torch.randint(-1, 2, (k, cin, r, s), generator=g, dtype=torch.int16)
    sw = torch.tensor([0.25, 0.5, 0.125, 1.0])[torch.arange(k) % 4]
    ow = (torch.randint(-4, 5, (k,), generator=g).double() / 16).float() if asym else None
    bias = (torch.randint(-64, 65, (k,), generator=g).double() / 32).float()
    return q, qw, sw, ow, bias


def reference(q, qw, sw, ow, bias, stride, pad, dil=1, groups=1):
    """float64 conv of x^ = q * s + o with zero padding, w^ = qw * s_w (+ o_w), + bias; and the tap sums T [k, r, s] over real channels."""
    xh = q.double() * S_IN + OFF
    wh = qw.double() * sw.double()[:, None, None, None] + (0.0 if ow is None else ow.double()[:, None, None, None])
    out = F.conv2d(xh, wh, bias.double(), stride=stride, padding=pad, dilation=dil, groups=groups)
    tap = wh.sum(dim=1)
    assert torch.equal(out.float().double(), out), "construction is not exact"
    return out.float(), tap


def fold(bias, tap):
    return (bias.double() + OFF * tap.sum(dim=(1, 2))).float(), tap.permute(1, 2, 0).reshape(-1, tap.shape[0]).float().contiguous()


def emit_q(plain):
    """A consumer quantiser: plain unsigned bytes (the fast paths) or QBASE with its own float offset."""
    if plain:
        return K.EmitCodes(torch.tensor([0.25], device=DEV), None, 0, 255, N.FORM_ZEROPOINT)
    return K.EmitCodes(torch.tensor([0.25], device=DEV), torch.tensor([-1.5], device=DEV), 0, 255, N.FORM_QBASE)


def want_codes(ref, em, relu):
    v = torch.relu(ref) if relu else ref
    v = v.to(DEV).contiguous(memory_format=torch.channels_last)
    return K.fake_quant(v, em.scale, em.zero_point, em.lo, em.hi, em.form, g=0.0, codes="i8", want_y=False)[1]


def as_codes(q):
    return q.to(torch.uint8).to(DEV).contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------------------------------------- the tiled kernel
TILED = [  # (n, c, h, w, k, r, stride, pad, dil)
    (2, 64, 9, 11, 64, 3, 1, 1, 1),       # corners and edges
    (2, 64, 9, 10, 128, 3, 2, 1, 1),      # stride 2, 128-wide tiles
    (3, 64, 3, 2, 64, 3, 1, 2, 2),        # dilation 2, an image smaller than the filter's reach
    (2, 128, 5, 5, 10, 3, 1, 1, 1),       # K % 4 != 0: the element-wise epilogue
    (1, 64, 6, 6, 64, 5, 2, 2, 1),        # 5 x 5
]


@pytest.mark.parametrize("asym", [False, True])
@pytest.mark.parametrize("case", TILED)
def test_tiled_xoff_exact(case, asym):
    n, c, h, w, k, r, st, pd, dl = case
    q, qw, sw, ow, bias = operands(n, c, h, w, k, r, r, asym, seed=hash(case) & 0xffff)
    ref, tap = reference(q, qw, sw, ow, bias, st, pd, dl)
    bf, ts = fold(bias, tap)
    wq = qw.permute(0, 2, 3, 1).contiguous().to(torch.int8).to(DEV)
    wsum = qw.sum(dim=(1, 2, 3)).to(torch.int32).to(DEV)
    args = (as_codes(q), wq, wsum, bf.to(DEV), torch.tensor([S_IN], device=DEV), None, sw.to(DEV))
    kw = dict(stride=st, padding=pd, dilation=dl, in_offset=torch.tensor([OFF], device=DEV), tap_sums=ts.to(DEV),
              w_offset=None if ow is None else ow.to(DEV))
    out = K.conv2d_i8(*args, **kw)
    same(out.cpu(), ref, f"{case} asym={asym} fp32")
    for plain in (True, False):
        em = emit_q(plain)
        o2, codes = K.conv2d_i8(*args, emit=em, want_out=True, relu=True, **kw)
        same(o2.cpu(), torch.relu(ref), f"{case} fp32 + codes")
        same(codes.cpu(), want_codes(ref, em, True).cpu(), f"{case} codes plain={plain}")
        if k % 4 == 0:     # codes only (where the halo / swapped kernels would take a call without the offset)
            _, c2 = K.conv2d_i8(*args, emit=em, want_out=False, relu=True, **kw)
            same(c2.cpu(), codes.cpu(), f"{case} codes only plain={plain}")


def _xoff_route(codes, wq, wsum, bias, ts, r, pad, k, c, em, xoff):
    h, w = codes.shape[2], codes.shape[3]
    s_in = torch.tensor([S_IN], device=DEV)
    sw = torch.ones(k, device=DEV)
    out_codes = torch.empty((codes.shape[0], k, h, w), dtype=torch.uint8, device=DEV).contiguous(memory_format=torch.channels_last)
    common = (N.ptr(codes), N.ptr(wq), None, N.ptr(bias), N.ptr(wsum), N.ptr(s_in), None, N.ptr(sw))
    geo = (codes.shape[0], h, w, c, k, r, r, 1, pad, 1, 1, None, 1, N.ptr(out_codes), N.ptr(em.scale), None, 0, 255, N.FORM_ZEROPOINT | N.ROUTE_ONLY, 0.0)
    if xoff:
        return N.lib.dlmcq_conv2d_i8_nhwc_xoff(*common, None, *geo, N.ptr(torch.tensor([OFF], device=DEV)), N.ptr(ts), None)
    return N.lib.dlmcq_conv2d_i8_nhwc_fused(*common, *geo, None)


def test_tiled_xoff_routes():
    """A codes-only 3x3 call: the halo-tile kernel takes it without the offset and declines it with it; the pipelined one likewise."""
    em = emit_q(True)
    for r, pad, k, c, plain_route in ((3, 1, 64, 64, N.ROUTE_HALO3X3), (3, 0, 64, 64, N.ROUTE_TILED)):
        codes = as_codes(torch.zeros(2, c, 8, 8, dtype=torch.int16))
        wq = torch.zeros(k, r, r, c, dtype=torch.int8, device=DEV)
        wsum = torch.zeros(k, dtype=torch.int32, device=DEV)
        bias = torch.zeros(k, device=DEV)
        ts = torch.zeros(r * r, k, device=DEV)
        assert _xoff_route(codes, wq, wsum, bias, ts, r, pad, k, c, em, False) == plain_route
        # (pad 0: no border exists - the call is the fused call itself and keeps its route)
        assert _xoff_route(codes, wq, wsum, bias, ts, r, pad, k, c, em, True) == N.ROUTE_TILED


def test_pointwise_folded_bias_exact():
    """1x1 layers need no kernel change: the folded bias alone, through the ordinary entry point and through the _xoff one."""
    q, qw, sw, ow, bias = operands(3, 64, 7, 5, 128, 1, 1, True, seed=7)
    ref, tap = reference(q, qw, sw, ow, bias, 1, 0)
    bf, ts = fold(bias, tap)
    wq = qw.permute(0, 2, 3, 1).contiguous().to(torch.int8).to(DEV)
    wsum = qw.sum(dim=(1, 2, 3)).to(torch.int32).to(DEV)
    args = (as_codes(q), wq, wsum, bf.to(DEV), torch.tensor([S_IN], device=DEV), None, sw.to(DEV))
    em = emit_q(False)
    o1, c1 = K.conv2d_i8(*args, w_offset=ow.to(DEV), emit=em)
    o2, c2 = K.conv2d_i8(*args, w_offset=ow.to(DEV), emit=em, in_offset=torch.tensor([OFF], device=DEV), tap_sums=ts.to(DEV))
    same(o1.cpu(), ref, "1x1 folded bias")
    same(o2.cpu(), ref, "1x1 through _xoff")
    same(c1.cpu(), want_codes(ref, em, False).cpu(), "1x1 codes")
    same(c2.cpu(), c1.cpu(), "1x1 codes through _xoff")


# ------------------------------------------------------------------------------------------------- depthwise
DW = [  # (n, c, h, w, stride)
    (2, 64, 7, 9, 1), (2, 32, 2, 2, 1), (2, 48, 9, 8, 2), (1, 960, 3, 3, 2), (2, 144, 5, 6, 1),
]


@pytest.mark.parametrize("asym", [False, True])
@pytest.mark.parametrize("case", DW)
def test_depthwise_xoff_exact(case, asym):
    n, c, h, w, st = case
    q, qw, sw, ow, bias = operands(n, c, h, w, c, 3, 3, asym, groups=c, seed=hash(case) & 0xffff)
    ref, tap = reference(q, qw, sw, ow, bias, st, 1, groups=c)
    bf, ts = fold(bias, tap)
    wq = qw[:, 0].permute(1, 2, 0).contiguous().to(torch.int8).to(DEV)       # [R, S, C]
    args = (as_codes(q), wq, bf.to(DEV), torch.tensor([S_IN], device=DEV), None, sw.to(DEV), None if ow is None else ow.to(DEV))
    kw = dict(stride=st, padding=1, in_offset=torch.tensor([OFF], device=DEV), tap_sums=ts.to(DEV))
    same(K.conv2d_dw_i8(*args, **kw).cpu(), ref, f"dw {case} fp32")
    for plain in (True, False):          # codes only with the plain quantiser: the FAST instantiations
        em = emit_q(plain)
        _, codes = K.conv2d_dw_i8(*args, relu=True, emit=em, want_out=False, **kw)
        same(codes.cpu(), want_codes(ref, em, True).cpu(), f"dw {case} codes plain={plain}")
        o2, c2 = K.conv2d_dw_i8(*args, relu=True, emit=em, want_out=True, **kw)
        same(o2.cpu(), torch.relu(ref), f"dw {case} fp32 + codes")
        same(c2.cpu(), codes.cpu(), f"dw {case} codes with fp32")


def test_depthwise_xoff_route_and_refusal():
    c, em = 64, emit_q(True)
    codes = as_codes(torch.zeros(32, c, 16, 16, dtype=torch.int16))           # (the matrix-core kernel's minimum: 4096 pixels, W >= 14)
    wq = torch.zeros(3, 3, c, dtype=torch.int8, device=DEV)
    s1, sw, b = torch.ones(1, device=DEV), torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
    oc = torch.empty_like(codes)
    ts, o = torch.zeros(9, c, device=DEV), torch.tensor([OFF], device=DEV)
    common = (N.ptr(codes), N.ptr(wq), None, N.ptr(b), N.ptr(s1), None, N.ptr(sw), None, 32, 16, 16, c, 3, 3, 1, 1, 1, 1, N.ptr(oc),
              N.ptr(em.scale), None, 0, 255, N.FORM_ZEROPOINT | N.ROUTE_ONLY, 0.0)
    assert N.lib.dlmcq_conv2d_dw_i8_nhwc(*common, None) == N.ROUTE_DWM
    assert N.lib.dlmcq_conv2d_dw_i8_nhwc_xoff(*common, N.ptr(o), N.ptr(ts), None) == N.ROUTE_DW
    c5 = list(common)
    c5[12] = c5[13] = 5                                                         # 5 x 5: the generic kernel has no border term
    assert N.lib.dlmcq_conv2d_dw_i8_nhwc_xoff(*c5, N.ptr(o), N.ptr(ts), None) == -1


# ------------------------------------------------------------------------------------------------- first layer
STEM = [  # (n, c, h, w, k, r, stride, pad)
    (2, 3, 13, 11, 64, 7, 2, 3), (2, 3, 2, 2, 64, 7, 2, 3), (2, 3, 9, 10, 32, 3, 2, 1), (1, 3, 5, 5, 64, 3, 1, 1),
]


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("asym", [False, True])
@pytest.mark.parametrize("case", STEM)
def test_stem_xoff_exact(case, asym, shift):
    n, c, h, w, k, r, st, pd = case
    q, qw, sw, ow, bias = operands(n, c, h, w, k, r, r, asym, seed=hash(case) & 0xffff)
    ref, tap = reference(q, qw, sw, ow, bias, st, pd)
    bf, ts = fold(bias, tap)
    x = (q.double() * S_IN + OFF).float().to(DEV)                   # the image whose QBase codes are q exactly
    xpad = K.quantize_pad_nhwc4(x, torch.tensor([S_IN], device=DEV), torch.tensor([OFF], device=DEV), 0, 255, N.FORM_QBASE, pd,
                                shift128=shift, pad_code0=True)
    got_q = xpad.to(torch.int16) + (128 if shift else 0)
    assert torch.equal(got_q[:, pd:pd + h, pd:pd + w, :c].cpu(), q.permute(0, 2, 3, 1)), "image codes"
    border = torch.ones_like(got_q, dtype=torch.bool)
    border[:, pd:pd + h, pd:pd + w] = False
    assert bool((got_q[border] == 0).all()), "the border holds code 0"
    full = torch.zeros((k, r, 8, 4), dtype=torch.int16)
    full[:, :, :r, :c] = qw.permute(0, 2, 3, 1)
    wq, wsum = full.to(torch.int8).contiguous().to(DEV), qw.sum(dim=(1, 2, 3)).to(torch.int32).to(DEV)
    zp = torch.tensor([-128.0], device=DEV) if shift else None
    kw = dict(stride=st, w_offset=None if ow is None else ow.to(DEV), channels=c, in_offset=torch.tensor([OFF], device=DEV),
              tap_sums=ts.to(DEV), pad=pd)
    args = (xpad, wq, wsum, bf.to(DEV), torch.tensor([S_IN], device=DEV), zp, sw.to(DEV), r)
    same(K.conv2d_i8_stem(*args, **kw).cpu(), ref, f"stem {case} fp32")
    for plain in (True, False):
        em = emit_q(plain)
        o2, codes = K.conv2d_i8_stem(*args, relu=True, emit=em, **kw)
        same(o2.cpu(), torch.relu(ref), f"stem {case} fp32 + codes")
        same(codes.cpu(), want_codes(ref, em, True).cpu(), f"stem {case} codes plain={plain}")


def test_quantize_pad_code0_is_refused_elsewhere():
    """DLMCQ_PAD_CODE0 belongs to quantize_pad_nhwc4: the convolution entry points refuse it in their quantiser form."""
    c, em = 64, emit_q(True)
    codes = as_codes(torch.zeros(1, c, 4, 4, dtype=torch.int16))
    wq = torch.zeros(c, 3, 3, c, dtype=torch.int8, device=DEV)
    wsum = torch.zeros(c, dtype=torch.int32, device=DEV)
    s1, sw = torch.ones(1, device=DEV), torch.ones(c, device=DEV)
    oc = torch.empty_like(codes)
    rc = N.lib.dlmcq_conv2d_i8_nhwc_fused(N.ptr(codes), N.ptr(wq), None, None, N.ptr(wsum), N.ptr(s1), None, N.ptr(sw), 1, 4, 4, c, c, 3, 3,
                                          1, 1, 1, 1, None, 1, N.ptr(oc), N.ptr(em.scale), None, 0, 255,
                                          N.FORM_ZEROPOINT | N.PAD_CODE0 | N.ROUTE_ONLY, 0.0, None)
    assert rc == -1


# ------------------------------------------------------------------------------------------------- the plan
QBASE_W4A8 = {"weight": {"enable": True, "type": "minmax_channel", "args": {"n_bits": 4, "signed": False}},
              "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
              "exclude_layers": [], "override_options": []}


def _mobilenet(batch):
    import workloads as W
    from dlmc.utils.merge_bn import merge_bn
    from dlmc.utils.quantize import quantize_model
    torch.manual_seed(31)
    net = W.mobilenet_v2().to(DEV).eval()
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    net = merge_bn(net, inplace=True)
    quantize_model(net, copy.deepcopy(QBASE_W4A8), None)
    mean = torch.tensor([0.485, 0.456, 0.406], device=DEV)[:, None, None]
    std = torch.tensor([0.229, 0.224, 0.225], device=DEV)[:, None, None]
    x = (torch.rand(batch, 3, 224, 224, device=DEV) - mean) / std           # ImageNet-normalised: the first layer's offset is not 0
    with torch.no_grad():
        net(x)                                   # calibrate
    return net, x


def _rel(got, want):
    return float((got.double() - want.double()).norm() / want.double().norm())


def _nodes_match_wrappers(net, plan, x):
    """Every plan node fed the fp32 input its wrapper saw gives the wrapper's output up to quantisation noise.  Returns how many of them
    carry a float activation offset."""
    from dlmc.utils import fuse as FU
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, i, o: seen.__setitem__(mod, (i[0].detach().clone(), o.detach().clone())))
             for m in net.modules() if hasattr(m, "in_scale")]
    with torch.no_grad():
        net(x)
    for h in hooks:
        h.remove()
    checked = 0
    for m in plan.modules():
        if isinstance(m, FU._PlanLayer) and m.layer in seen:
            xin, ref = seen[m.layer]
            saved = (m.emit, m.want_out, m.relu6, m.relu, m.pool)
            m.emit, m.want_out, m.relu6, m.relu, m.pool = None, True, False, False, None
            try:
                with torch.no_grad():
                    node = m(xin)[0]
            finally:
                m.emit, m.want_out, m.relu6, m.relu, m.pool = saved
            assert _rel(node, ref) < 1e-4, (tuple(m.layer.weight.shape), m.act.xoff, _rel(node, ref))
            checked += m.act.xoff
    return checked


@pytest.mark.parametrize("batch", [8, 256])
def test_mobilenet_v2_qbase_plan_with_offsets(batch):
    from dlmc.utils.fuse import fuse_inference
    from dlmc.utils.graph import GraphedForward
    net, x = _mobilenet(batch)
    base, plan = fuse_inference(net), fuse_inference(net, act_offsets=True)
    rb, rp = base.fusion_report, plan.fusion_report
    print(batch, rb, rp, rp.act_offset)
    assert rb.act_offset == 0 and rp.act_offset >= 18 and rp.layers == 53 and rp.skipped == [] and len(rb.skipped) >= 18
    with torch.no_grad():
        want = net(x)
        got = plan(x)
        same(GraphedForward(plan, x)(x), got, "graphed plan")
    assert bool(torch.isfinite(got).all())
    # the wrappers quantise the same values with the same quantisers; a code can flip where fp32 rounding differs (folded bias vs
    # the wrapper's convolution of x^), and flips compound over 53 W4A8 layers: today's plan is ~4 % from the wrappers' logits too
    rb_, rp_ = _rel(base(x), want), _rel(got, want)
    assert rp_ < max(2 * rb_, 0.1), (rp_, rb_)
    assert _nodes_match_wrappers(net, plan, x[:8]) == rp.act_offset


MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def flag_off_case():
    """MobileNetV2 under QBase W4A8, calibrated on 8 ImageNet-normalised images made on the host (offsets at the first layer and the 17
    layers that read shortcut sums).  tests/golden/act_offset_flag_off_mnv2_b8.npz holds the logits of the plan fuse_inference(net)
    built for it before act_offsets existed."""
    import workloads as W
    from dlmc.utils.merge_bn import merge_bn
    from dlmc.utils.quantize import quantize_model
    torch.manual_seed(41)
    net = W.mobilenet_v2().eval()
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    net = merge_bn(net.to(DEV), inplace=True)
    quantize_model(net, copy.deepcopy(QBASE_W4A8), None)
    g = torch.Generator().manual_seed(42)
    x = ((torch.rand(8, 3, 224, 224, generator=g) - torch.tensor(MEAN)[:, None, None]) / torch.tensor(STD)[:, None, None]).to(DEV)
    with torch.no_grad():
        net(x)
    return net, x


def test_flag_off_plan_is_the_plan_as_it_was():
    import os
    import numpy as np
    from dlmc.utils.fuse import fuse_inference
    net, x = flag_off_case()
    plan = fuse_inference(net, act_offsets=False)
    rep = plan.fusion_report
    assert (rep.layers, rep.act_offset, len(rep.skipped)) == (35, 0, 18)
    with torch.no_grad():
        got = plan(x).cpu()
    want = torch.from_numpy(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "act_offset_flag_off_mnv2_b8.npz"))["logits"])
    same(got, want, "act_offsets=False against the plan before the flag")


def test_resnet50_qbase_normalised_images():
    """ResNet-50 QBase W8A8 on ImageNet-normalised images: the 7 x 7 first layer carries the offset (border term in the first-layer
    kernel, its max-pool kept apart, on codes)."""
    import workloads as W
    from dlmc.utils.fuse import StemLayer, fuse_inference
    from dlmc.utils.graph import GraphedForward
    from dlmc.utils.merge_bn import merge_bn
    from dlmc.utils.quantize import quantize_model
    torch.manual_seed(7)
    net = merge_bn(W.resnet50().to(DEV).eval(), inplace=True)
    quantize_model(net, copy.deepcopy(QBASE_W8A8), None)
    g = torch.Generator().manual_seed(8)
    x = ((torch.rand(8, 3, 224, 224, generator=g) - torch.tensor(MEAN)[:, None, None]) / torch.tensor(STD)[:, None, None]).to(DEV)
    with torch.no_grad():
        net(x)
    base, plan = fuse_inference(net), fuse_inference(net, act_offsets=True)
    rb, rp = base.fusion_report, plan.fusion_report
    print(rb, rp)
    assert rb.act_offset == 0 and rb.stem == 0 and rp.act_offset == 1 and rp.stem == 1 and rp.layers == rb.layers + 1 and rp.skipped == []
    stem = next(m for m in plan.modules() if isinstance(m, StemLayer))
    assert stem.act.xoff and stem.xoff_padded and stem.pool == (3, 2, 1)
    with torch.no_grad():
        want = net(x)
        got = plan(x)
        same(GraphedForward(plan, x)(x), got, "graphed plan")
    rb_, rp_ = _rel(base(x), want), _rel(got, want)
    assert rp_ < max(2 * rb_, 0.05), (rp_, rb_)
    assert _nodes_match_wrappers(net, plan, x) == 1


QBASE_W8A8 = {"weight": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": True}},
              "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
              "exclude_layers": [], "override_options": []}


class DwLinear(nn.Module):
    """relu -> depthwise 3 x 3 / 1 / 1 WITHOUT activation -> 1 x 1: the pointwise layer's input (the depthwise output) has a float offset."""

    def __init__(self):
        super().__init__()
        self.dw = nn.Conv2d(64, 64, 3, padding=1, groups=64)
        self.pw = nn.Conv2d(64, 128, 1)

    def forward(self, x):
        return torch.relu(self.pw(self.dw(torch.relu(x))))


def test_dwpw_declines_an_offset_pointwise_input():
    from dlmc.utils.fuse import fuse_inference
    from dlmc.utils.quantize import quantize_model
    torch.manual_seed(3)
    net = DwLinear().to(DEV).eval()
    quantize_model(net, copy.deepcopy(QBASE_W8A8), None)
    x = torch.randn(4, 64, 20, 20, device=DEV)
    with torch.no_grad():
        net(x)
    fused = fuse_inference(net, act_offsets=True, dwpw=True)
    plain = fuse_inference(net, act_offsets=True)
    assert fused.fusion_report.act_offset == 1 and fused.fusion_report.dwpw == 0
    with torch.no_grad():
        same(fused(x), plain(x), "dwpw=True with an offset pointwise input")
        assert _rel(fused(x), net(x)) < 2e-2
