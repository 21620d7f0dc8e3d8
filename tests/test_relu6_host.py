"""ReLU6 in the frozen int8 plan, on the host: the MobileNetV2 workload's shape, the plan's fusion decisions (dry run, wrappers
marked calibrated by hand as in test_host_logic.py::test_fusion_decisions_without_a_gpu) and the activation constants of the ABI."""
import os
import re

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import workloads as W
from dlmc import _native as N
from dlmc.quantization.scalar.FSPTQuant import FSPTQBase
from dlmc.utils.fuse import fuse_inference
from dlmc.utils.quantize import quantize_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = {"weight": {"enable": True, "type": "minmax_channel", "args": {"n_bits": 8, "signed": True}},
       "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
       "exclude_layers": [], "override_options": []}


def calibrated(net):
    for m in net.modules():                      # BatchNorm folded by hand: the pass treats Identity as a wire
        for name, child in list(m.named_children()):
            if isinstance(child, nn.BatchNorm2d):
                setattr(m, name, nn.Identity())
    quantize_model(net, CFG, None, "FSPTQ")
    for m in net.modules():
        if isinstance(m, FSPTQBase):
            m.in_init_state.fill_(1)
            m.wt_init_state.fill_(1)
            m.in_offset = torch.tensor(0.0)
    return net.eval()


def counts(rep):
    return dict(layers=rep.layers, relu6=rep.relu6, relu=rep.relu, residual=rep.residual, emit=rep.emit, fp32_outputs=rep.fp32_outputs,
                skipped=rep.skipped)


def test_mobilenet_v2_layer_table():
    net = W.MODELS["mobilenet_v2"]()
    assert W.table_totals(W.layer_table(net, torch.zeros(1, 3, 224, 224))) == (53, 6767200, 3469760, 300774272)
    assert sum(p.numel() for p in net.parameters()) == 3504872          # torchvision's count, BatchNorm included
    assert sum(isinstance(m, nn.ReLU6) for m in net.modules()) == 35


def test_mobilenet_v2_fusion_report():
    rep = fuse_inference(calibrated(W.mobilenet_v2()), dry_run=True).fusion_report
    assert counts(rep) == dict(layers=53, relu6=35, relu=0, residual=3, emit=44, fp32_outputs=16, skipped=[])
    assert "relu6 fused=35" in repr(rep)
    rep = fuse_inference(calibrated(W.mobilenet_v2()), dry_run=True, relu6=False).fusion_report
    assert counts(rep) == dict(layers=53, relu6=0, relu=0, residual=3, emit=10, fp32_outputs=50, skipped=[])


def test_mobilenet_v2_plan_keeps_no_relu6_op():
    gm = fuse_inference(calibrated(W.mobilenet_v2()), dry_run=True)
    left = [n for n in gm.graph.nodes if n.op == "call_module" and isinstance(dict(gm.named_modules()).get(n.target), nn.Hardtanh)]
    assert left == []
    gm = fuse_inference(calibrated(W.mobilenet_v2()), dry_run=True, relu6=False)
    mods = dict(gm.named_modules())
    assert sum(n.op == "call_module" and type(mods.get(n.target)) is nn.ReLU6 for n in gm.graph.nodes) == 35


class Block(nn.Module):
    """conv (64 -> 64) -> activation -> conv -> activation: which activation forms the plan folds into the first layer."""

    def __init__(self, act):
        super().__init__()
        self.a = nn.Conv2d(64, 64, 1)
        self.b = nn.Conv2d(64, 64, 1)
        self.act = act

    def forward(self, x):
        return torch.relu(self.b(self.act(self.a(x))))


class Mod(nn.Module):
    def __init__(self, m):
        super().__init__()
        self.m = m

    def forward(self, x):
        return self.m(x)


class Fn(nn.Module):
    def __init__(self, fn):
        super().__init__()
        self.fn = fn

    def forward(self, x):
        return self.fn(x)


@pytest.mark.parametrize("act, fused", [
    (nn.ReLU6(), True),
    (nn.ReLU6(inplace=True), True),
    (nn.Hardtanh(0.0, 6.0), True),
    (nn.Hardtanh(0, 6), True),
    (nn.Hardtanh(-1.0, 1.0), False),
    (nn.Hardtanh(0.0, 5.0), False),
    (nn.Hardtanh(), False),
])
def test_relu6_module_forms(act, fused):
    rep = fuse_inference(calibrated(Block(act)), dry_run=True).fusion_report
    assert (rep.layers, rep.relu6, rep.relu) == (2, int(fused), 1)
    assert rep.emit == 1 if fused else rep.emit == 0        # a separate op in between: the second layer quantises an fp32 tensor


class FnBlock(Block):
    def __init__(self, fn):
        super().__init__(None)
        self.fn = fn

    def forward(self, x):
        return torch.relu(self.b(self.fn(self.a(x))))


@pytest.mark.parametrize("name, fn, fused", [
    ("F.relu6", lambda x: F.relu6(x), True),
    ("F.relu6 inplace", lambda x: F.relu6(x, inplace=True), True),
    ("F.relu6 inplace positional", lambda x: F.relu6(x, True), True),
    ("F.hardtanh(x, 0., 6.)", lambda x: F.hardtanh(x, 0.0, 6.0), True),
    ("F.hardtanh keywords", lambda x: F.hardtanh(x, min_val=0.0, max_val=6.0), True),
    ("F.hardtanh(x, -1., 1.)", lambda x: F.hardtanh(x, -1.0, 1.0), False),
    ("F.hardtanh(x, 0., 5.)", lambda x: F.hardtanh(x, 0.0, 5.0), False),
    ("F.hardtanh(x)", lambda x: F.hardtanh(x), False),
    ("torch.clamp(x, 0, 6)", lambda x: torch.clamp(x, 0.0, 6.0), False),
])
def test_relu6_functional_forms(name, fn, fused):
    rep = fuse_inference(calibrated(FnBlock(fn)), dry_run=True).fusion_report
    assert (rep.layers, rep.relu6, rep.relu) == (2, int(fused), 1), name


def test_relu6_option_off_keeps_the_op():
    rep = fuse_inference(calibrated(Block(nn.ReLU6())), dry_run=True, relu6=False).fusion_report
    assert (rep.relu6, rep.relu, rep.emit) == (0, 1, 0)


class ConvShortcut(nn.Module):
    """A block end whose shortcut is a 1x1 convolution of width 64 k: with ReLU it runs as ONE dual kernel; with ReLU6 the dual kernel
    (ReLU only) is not used - the shortcut convolution runs on its own, the add and the ReLU6 fold into the block end."""

    def __init__(self, act):
        super().__init__()
        self.stem = nn.Conv2d(64, 64, 1)
        self.a = nn.Conv2d(64, 128, 3, padding=1)
        self.b = nn.Conv2d(128, 256, 1)
        self.down = nn.Conv2d(64, 256, 1)
        self.head = nn.Conv2d(256, 64, 1)
        self.act = act

    def forward(self, x):
        y = torch.relu(self.stem(x))
        return torch.relu(self.head(self.act(self.b(torch.relu(self.a(y))) + self.down(y))))


def test_relu6_block_end_gets_no_dual_kernel():
    rep = fuse_inference(calibrated(ConvShortcut(nn.ReLU())), dry_run=True).fusion_report
    assert (rep.layers, rep.dual, rep.relu6) == (5, 1, 0)
    rep = fuse_inference(calibrated(ConvShortcut(nn.ReLU6())), dry_run=True).fusion_report
    assert (rep.layers, rep.dual, rep.relu6, rep.residual) == (5, 0, 1, 1)
    rep = fuse_inference(calibrated(ConvShortcut(nn.ReLU6())), dry_run=True, relu6=False).fusion_report
    assert (rep.dual, rep.relu6) == (1, 0)


def test_eager_fused_does_not_take_relu6_for_relu():
    from dlmc.utils import fuse
    g = torch.fx.symbolic_trace(Block(nn.ReLU6()))
    mods = dict(g.named_modules())
    act = next(n for n in g.graph.nodes if n.op == "call_module" and n.target == "act")
    assert not fuse._is_relu(act, mods) and fuse._is_relu6(act, mods)


def test_activation_constants():
    header = open(os.path.join(ROOT, "include", "dlmcq.h")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define DLMCQ_ACT_(\w+)\s+(\d+)", header)}
    assert got == {"NONE": 0, "RELU": 1, "RELU6": 2}
    assert (N.ACT_NONE, N.ACT_RELU, N.ACT_RELU6) == (0, 1, 2)


def test_act_argument_of_the_wrappers():
    from dlmc.quantization.scalar import kernels as K
    assert (K._act(False, None), K._act(True, None), K._act(True, N.ACT_RELU6), K._act(False, N.ACT_NONE)) == (0, 1, 2, 0)
    with pytest.raises(ValueError):
        K._act(False, 3)
