"""Float activation offsets in the frozen int8 plan, on the host: the plan's decisions for MobileNetV2 under QBase with offsets set by
hand (dry run, as test_relu6_host.py does for FSPTQ), and the ABI of the *_xoff entry points (refusals need no GPU)."""
import ctypes
import os
import re

import torch
from torch import nn

import workloads as W
from dlmc import _native as N
from dlmc.quantization.scalar.modules.base import QBase
from dlmc.utils.fuse import _Tracer, fuse_inference
from dlmc.utils.quantize import quantize_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QBASE_W4A8 = {"weight": {"enable": True, "type": "minmax_channel", "args": {"n_bits": 4, "signed": False}},
              "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
              "exclude_layers": [], "override_options": []}
NAMES = ("dlmcq_conv2d_i8_nhwc_xoff", "dlmcq_conv2d_dw_i8_nhwc_xoff", "dlmcq_conv2d_i8_stem_xoff")


def calibrated(first_offset=False):
    """MobileNetV2 under QBase, marked calibrated; every convolution whose input is no ReLU6 output (the shortcut sums the expansions and
    the last 1x1 read - and, with `first_offset`, the normalised image) gets a float offset, the others an offset of 0."""
    net = W.mobilenet_v2()
    for m in net.modules():
        for name, child in list(m.named_children()):
            if isinstance(child, nn.BatchNorm2d):
                setattr(m, name, nn.Identity())
    quantize_model(net, QBASE_W4A8, None)
    graph = _Tracer().trace(net)
    mods = dict(net.named_modules())
    negative = set()
    for nd in graph.nodes:
        m = mods.get(nd.target) if nd.op == "call_module" else None
        if isinstance(m, QBase):
            src = nd.args[0]
            while src.op == "call_module" and isinstance(mods.get(src.target), nn.Identity):
                src = src.args[0]
            is_relu6 = src.op == "call_module" and isinstance(mods.get(src.target), nn.Hardtanh)
            pooled = m.weight.dim() == 2            # (the classifier reads pooled ReLU6 outputs: non-negative)
            if (src.op == "placeholder" and first_offset) or (src.op != "placeholder" and not is_relu6 and not pooled):
                negative.add(m)
    for m in net.modules():
        if isinstance(m, QBase):
            m.in_init_state.fill_(1)
            m.wt_init_state.fill_(1)
            m.in_offset = torch.tensor([-0.625 if m in negative else 0.0])
    return net.eval(), len(negative)


def counts(rep):
    return dict(layers=rep.layers, relu6=rep.relu6, residual=rep.residual, emit=rep.emit, fp32_outputs=rep.fp32_outputs,
                stem=rep.stem, dual=rep.dual, act_offset=rep.act_offset, skipped=len(rep.skipped))


def test_mobilenet_v2_expansions_are_planned_with_offsets():
    net, neg = calibrated()
    assert neg == 17
    off = fuse_inference(net, dry_run=True).fusion_report
    assert counts(off) == dict(layers=36, relu6=18, residual=3, emit=18, fp32_outputs=18, stem=1, dual=0, act_offset=0, skipped=17)
    on = fuse_inference(net, dry_run=True, act_offsets=True).fusion_report
    assert counts(on) == dict(layers=53, relu6=35, residual=3, emit=44, fp32_outputs=16, stem=1, dual=0, act_offset=17, skipped=0)
    net, neg = calibrated(first_offset=True)
    assert neg == 18
    on = fuse_inference(net, dry_run=True, act_offsets=True).fusion_report
    assert on.layers == 53 and on.act_offset == 18 and on.skipped == []
    assert fuse_inference(net, dry_run=True).fusion_report.layers == 35


def test_offset_flag_off_is_the_plan_as_it_was():
    """Without offsets anywhere the flag changes nothing."""
    net, _ = calibrated()
    for m in net.modules():
        if isinstance(m, QBase):
            m.in_offset = torch.tensor([0.0])
    a = fuse_inference(net, dry_run=True).fusion_report
    b = fuse_inference(net, dry_run=True, act_offsets=True).fusion_report
    assert counts(a) == counts(b) and a.act_offset == 0


def test_xoff_entry_points_in_header_and_table():
    text = open(os.path.join(ROOT, "include", "dlmcq.h")).read()
    for name in NAMES:
        assert re.search(rf"\b{name}\s*\(", text), name
        assert name in N.SIGNATURES
    assert "#define DLMCQ_PAD_CODE0 0x8000" in text and N.PAD_CODE0 == 0x8000


def test_xoff_refusals_need_no_gpu():
    one = ctypes.c_void_p(16)
    odd = ctypes.c_void_p(20)
    conv = N.lib.dlmcq_conv2d_i8_nhwc_xoff
    base = (one, one, one, one, one, one, None, one, None, 1, 8, 8, 64, 64, 3, 3, 1, 1, 1, 1, None, 1, None, None, None, 0, 255, 2, 0.0)
    assert conv(*base, None, one, None) == -1                   # no in_offset
    assert conv(*base, one, None, None) == -1                   # no tap_sums
    assert conv(*base, one, odd, None) == -4                    # tap_sums not 16-byte aligned
    dw = N.lib.dlmcq_conv2d_dw_i8_nhwc_xoff
    dbase = (one, one, one, one, one, None, one, None, 1, 8, 8, 64, 5, 5, 1, 2, 1, 1, None, None, None, 0, 255, 2, 0.0)
    assert dw(*dbase, None, one, None) == -1
    assert dw(*dbase, one, one, None) == -1                     # 5 x 5: no depthwise kernel with the border term
    stem = N.lib.dlmcq_conv2d_i8_stem_xoff
    sbase = (one, one, one, one, one, one, None, one, None, 3, 1, 14, 14, 64, 5, 5, 2, 2, 1, 1, None, None, None, 0, 255, 2, 0.0)
    assert stem(*sbase, one, one, None) == -1                   # 5 x 5 first layer: the XOFF instantiations are 3 x 3 and 7 x 7
    assert stem(*sbase, None, one, None) == -1
    pad = N.lib.dlmcq_quantize_pad_nhwc4
    fused = N.lib.dlmcq_conv2d_i8_nhwc_fused
    fbase = (one, one, None, one, one, one, None, one, 1, 8, 8, 64, 64, 3, 3, 1, 1, 1, 1, None, 1, one, one, None, 0, 255)
    assert fused(*fbase, N.FORM_ZEROPOINT | N.PAD_CODE0, 0.0, None) == -1       # the padding flag is quantize_pad_nhwc4's alone
    assert pad(one, one, one, None, 1, 3, 8, 8, 192, 64, 8, 1, 2, -1, 255, N.FORM_QBASE | N.PAD_CODE0, 0.0, None) == -1   # still checked


class Shapes(nn.Module):
    """first layer 5 x 5 / pad 2 -> 1 x 1 -> depthwise 5 x 5 / pad 2 -> depthwise 3 x 3 / pad 1: with float offsets on every input, only
    the layers that have a kernel with the border term (or need none) are planned."""

    def __init__(self):
        super().__init__()
        self.stem = nn.Conv2d(3, 64, 5, padding=2)
        self.pw = nn.Conv2d(64, 64, 1)
        self.dw5 = nn.Conv2d(64, 64, 5, padding=2, groups=64)
        self.dw3 = nn.Conv2d(64, 64, 3, padding=1, groups=64)

    def forward(self, x):
        return self.dw3(self.dw5(self.pw(self.stem(x))))


def test_offset_layers_without_a_border_kernel_keep_their_fp32_path():
    net = Shapes()
    quantize_model(net, QBASE_W4A8, None)
    for m in net.modules():
        if isinstance(m, QBase):
            m.in_init_state.fill_(1)
            m.wt_init_state.fill_(1)
            m.in_offset = torch.tensor([-0.625])
    rep = fuse_inference(net.eval(), dry_run=True, act_offsets=True).fusion_report
    assert sorted(rep.skipped) == ["dw5", "stem"]                 # padded 5 x 5: no first-layer / depthwise kernel has the term
    assert (rep.layers, rep.act_offset, rep.stem) == (2, 2, 0)    # the 1 x 1 (folded bias) and the 3 x 3 depthwise
    net.stem.padding = (0, 0)                                     # unpadded: the folded bias is the whole term, any filter size
    rep = fuse_inference(net.eval(), dry_run=True, act_offsets=True).fusion_report
    assert rep.skipped == ["dw5"] and (rep.layers, rep.act_offset, rep.stem) == (3, 3, 1)
