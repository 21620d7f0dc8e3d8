"""Global-average-pool heads of the frozen int8 plan, on the host: which `pool -> flatten -> Linear` tails fuse_inference(gap_head=...)
folds (dry run, wrappers marked calibrated by hand as in test_relu6_host.py), what the workloads' reports say, and the boundary of the
two entry points (gap_head_supported's truth table, argument validation without a GPU)."""
import copy
import ctypes
import operator

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import workloads as W
from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from dlmc.quantization.scalar.FSPTQuant import FSPTQBase
from dlmc.utils.fuse import fuse_inference
from dlmc.utils.quantize import quantize_model

CFG = {"weight": {"enable": True, "type": "minmax_channel", "args": {"n_bits": 8, "signed": True}},
       "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
       "exclude_layers": [], "override_options": []}


def calibrated(net, cfg=CFG, method="FSPTQ"):
    for m in net.modules():                      # BatchNorm folded by hand: the pass treats Identity as a wire
        for name, child in list(m.named_children()):
            if isinstance(child, nn.BatchNorm2d):
                setattr(m, name, nn.Identity())
    quantize_model(net, copy.deepcopy(cfg), None, method)
    for m in net.modules():
        if isinstance(m, FSPTQBase):
            m.in_init_state.fill_(1)
            m.wt_init_state.fill_(1)
            m.in_offset = torch.tensor(0.0)
    return net.eval()


POOLS = {
    "module_1": lambda net, x: net.pool1(x),
    "module_11": lambda net, x: net.pool11(x),
    "functional_1": lambda net, x: F.adaptive_avg_pool2d(x, 1),
    "functional_11": lambda net, x: F.adaptive_avg_pool2d(x, (1, 1)),
    "method_mean_tuple": lambda net, x: x.mean((2, 3), keepdim=True),
    "torch_mean_tuple": lambda net, x: torch.mean(x, (2, 3), True),
    "method_mean_list": lambda net, x: x.mean([2, 3], keepdim=True),
    "method_mean_dim": lambda net, x: x.mean(dim=(2, 3), keepdim=True),
    "torch_mean_dim": lambda net, x: torch.mean(x, dim=[2, 3], keepdim=True),
}
FLATTENS = {
    "torch_flatten": lambda x: torch.flatten(x, 1),
    "method_flatten": lambda x: x.flatten(1),
    "view": lambda x: x.view(x.size(0), -1),
    "reshape": lambda x: x.reshape(x.size(0), -1),
    "squeeze": lambda x: x.squeeze(),
}
FLAT_POOLS = {       # keepdim=False: [N, C] at once, with or without a reshape behind it
    "method_mean": lambda net, x: x.mean((2, 3)),
    "torch_mean": lambda net, x: torch.mean(x, (2, 3)),
    "torch_mean_list": lambda net, x: torch.mean(x, [2, 3]),
    "method_mean_dim": lambda net, x: x.mean(dim=(2, 3)),
    "method_mean_keepdim_false": lambda net, x: x.mean((2, 3), keepdim=False),
}


class Tail(nn.Module):
    """conv -> ReLU -> 1x1 conv -> ReLU -> pool -> flatten -> (Dropout) -> Linear, the pool and the flatten as given."""

    def __init__(self, pool, flatten, width=64, out_size=1, dropout=False):
        super().__init__()
        self.c1 = nn.Conv2d(64, 64, 3, padding=1)
        self.c2 = nn.Conv2d(64, width, 1)
        self.pool1, self.pool11 = nn.AdaptiveAvgPool2d(out_size), nn.AdaptiveAvgPool2d((out_size, out_size))
        self.drop = nn.Dropout(0.2) if dropout else None
        self.fc = nn.Linear(width * out_size * out_size, 10)
        self._pool, self._flatten = pool, flatten

    def forward(self, x):
        x = torch.relu(self.c2(torch.relu(self.c1(x))))
        x = self._flatten(self._pool(self, x))
        if self.drop is not None:
            x = self.drop(x)
        return self.fc(x)


def pool_nodes(gm):
    """Nodes of the graph that still are a pool in one of the spellings."""
    mods = dict(gm.named_modules())
    return [n for n in gm.graph.nodes
            if (n.op == "call_module" and isinstance(mods.get(n.target), nn.AdaptiveAvgPool2d)) or
            (n.op == "call_function" and n.target in (F.adaptive_avg_pool2d, torch.mean)) or (n.op == "call_method" and n.target == "mean")]


def heads(gm):
    return [kind for _, kind in gm.fusion_report.gap_heads]


@pytest.mark.parametrize("flatten", sorted(FLATTENS))
@pytest.mark.parametrize("pool", sorted(POOLS))
def test_every_pool_and_flatten_spelling_is_folded(pool, flatten):
    gm = fuse_inference(calibrated(Tail(POOLS[pool], FLATTENS[flatten])), dry_run=True, gap_head=True)
    assert heads(gm) == ["fused"] and not pool_nodes(gm)
    assert "gap heads=" in repr(gm.fusion_report)
    gm = fuse_inference(calibrated(Tail(POOLS[pool], FLATTENS[flatten], dropout=True)), dry_run=True, gap_head="separate")
    assert heads(gm) == ["separate"] and not pool_nodes(gm)
    # nothing of the tail is left: the graph is placeholder, plan nodes and their getitems
    assert all(n.op in ("placeholder", "call_module", "output") or n.target is operator.getitem for n in gm.graph.nodes)


@pytest.mark.parametrize("flatten", [None] + sorted(set(FLATTENS) - {"squeeze"}))
@pytest.mark.parametrize("pool", sorted(FLAT_POOLS))
def test_mean_without_keepdim_is_folded(pool, flatten):
    gm = fuse_inference(calibrated(Tail(FLAT_POOLS[pool], FLATTENS[flatten] if flatten else (lambda x: x))), dry_run=True, gap_head=True)
    assert heads(gm) == ["fused"] and not pool_nodes(gm)


def test_the_head_node_takes_the_producers_inputs_and_feeds_the_linear_codes():
    gm = fuse_inference(calibrated(Tail(POOLS["module_1"], FLATTENS["torch_flatten"])), dry_run=True, gap_head=True)
    (name, kind), = gm.fusion_report.gap_heads
    head = next(n for n in gm.graph.nodes if n.op == "call_module" and n.target == name)
    fc = next(n for n in gm.graph.nodes if n.op == "call_module" and n.target != name and any(a.op == "call_function" and a.args[0] is head
                                                                                            for a in n.all_input_nodes))
    assert fc.args[0].target is operator.getitem and fc.args[0].args == (head, 1)        # the codes, not the fp32 pooled tensor
    assert head.args[0].target is operator.getitem and head.args[0].args[1] == 1         # ... from the first layer's codes
    sep = fuse_inference(calibrated(Tail(POOLS["module_1"], FLATTENS["torch_flatten"])), dry_run=True, gap_head="separate")
    assert sep.fusion_report.fp32_outputs == gm.fusion_report.fp32_outputs + 1           # the fused head's fp32 map is gone


def test_pooled_fp32_with_another_reader_is_produced_as_well():
    class Two(Tail):
        def forward(self, x):
            x = torch.flatten(self.pool1(torch.relu(self.c2(torch.relu(self.c1(x))))), 1)
            return self.fc(x) + x[:, :10]
    gm = fuse_inference(calibrated(Two(None, None)), dry_run=True, gap_head=True)
    (name, kind), = gm.fusion_report.gap_heads
    head = next(n for n in gm.graph.nodes if n.op == "call_module" and n.target == name)
    used = {u.args[1] for u in head.users if u.users}
    assert kind == "fused" and used == {0, 1} and not pool_nodes(gm)


# ---- negatives: the pool stays -------------------------------------------------------------------------------------------------------
def unfolded(net, **kw):
    gm = fuse_inference(net, dry_run=True, gap_head=True, **kw)
    return gm.fusion_report.gap_heads == [] and len(pool_nodes(gm)) == 1


def test_other_output_sizes_stay():
    assert unfolded(calibrated(Tail(POOLS["module_1"], FLATTENS["torch_flatten"], out_size=2)))


def test_a_pool_read_by_an_unplanned_linear_stays():
    cfg = dict(CFG, exclude_layers=["fc"])            # the classifier keeps its fp32 nn.Linear
    assert unfolded(calibrated(Tail(POOLS["module_1"], FLATTENS["torch_flatten"]), cfg))
    net = Tail(POOLS["module_1"], FLATTENS["torch_flatten"])
    quantize_model(net, dict(copy.deepcopy(CFG), momentum=0.1), None, "RootQ")
    assert unfolded(net.eval())
    net = calibrated(Tail(POOLS["module_1"], FLATTENS["torch_flatten"]))
    net.fc.act_quant = False                           # a disabled quantiser
    assert unfolded(net)
    net = calibrated(Tail(POOLS["module_1"], FLATTENS["torch_flatten"]))
    net.fc.in_offset = torch.tensor(0.5)               # a non-integer FSPTQ zero point
    assert unfolded(net)
    assert unfolded(calibrated(Tail(POOLS["module_1"], FLATTENS["torch_flatten"], width=100)))     # in-features % 64 != 0


def test_squeeze_excite_mean_feeding_a_convolution_stays():
    class SE(nn.Module):
        def __init__(self):
            super().__init__()
            self.c1, self.gate = nn.Conv2d(64, 64, 3, padding=1), nn.Conv2d(64, 64, 1)

        def forward(self, x):
            x = torch.relu(self.c1(x))
            return x * torch.sigmoid(self.gate(x.mean((2, 3), keepdim=True)))
    assert unfolded(calibrated(SE()))


def test_gap_head_false_is_the_plan_without_the_argument():
    a = fuse_inference(calibrated(W.resnet18()), dry_run=True)
    b = fuse_inference(calibrated(W.resnet18()), dry_run=True, gap_head=False)
    assert repr(a.fusion_report) == repr(b.fusion_report) and b.fusion_report.gap_heads == []
    assert [(n.op, str(n.target)) for n in a.graph.nodes] == [(n.op, str(n.target)) for n in b.graph.nodes]
    assert len(pool_nodes(b)) == 1
    with pytest.raises(ValueError):
        fuse_inference(calibrated(Tail(POOLS["module_1"], FLATTENS["torch_flatten"])), dry_run=True, gap_head="both")


# ---- workloads ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,forced,true", [("resnet50", "fused", "separate"), ("mobilenet_v2", "fused", "separate"),
                                              ("mobileone_s1", "fused", "separate"), ("repvgg_a1", "separate", "separate"),
                                              ("resnet18", "separate", "separate")])
def test_workload_reports(name, forced, true):
    """`forced`: the head under gap_head="fused" (wherever the kernel is built: the 1x1 last layers of ResNet-50, MobileNetV2 and
    MobileOne-S1; RepVGG-A1's 3x3 / stride 2 and ResNet-18's 3x3 last layers are not).  `true`: under gap_head=True, which leaves out
    the layers the fused head was measured slower on (K.GAP_HEAD_MEASURED_SLOWER: exactly those three)."""
    base = fuse_inference(calibrated(W.MODELS[name]()), dry_run=True).fusion_report
    gm = fuse_inference(calibrated(W.MODELS[name]()), dry_run=True, gap_head="fused")
    assert heads(gm) == [forced] and not pool_nodes(gm)
    assert gm.fusion_report.fp32_outputs == base.fp32_outputs - (forced == "fused")      # ResNet-50: one fp32 tensor fewer
    assert gm.fusion_report.layers == base.layers
    for flag, kind in ((True, true), ("separate", "separate")):
        rep = fuse_inference(calibrated(W.MODELS[name]()), dry_run=True, gap_head=flag)
        assert heads(rep) == [kind] and not pool_nodes(rep)
        assert rep.fusion_report.fp32_outputs == base.fp32_outputs - (kind == "fused")


def test_true_leaves_out_only_the_measured_slower_layers():
    assert K.GAP_HEAD_MEASURED_SLOWER == {(512, 2048), (320, 1280), (512, 1280)}
    assert not K.gap_head_profitable(512, 2048) and K.gap_head_profitable(64, 64) and K.gap_head_profitable(512, 1024)
    for width, kind in ((64, "fused"), (1280, "fused")):          # (64 -> 1280 is not in the table)
        assert heads(fuse_inference(calibrated(Tail(POOLS["module_1"], FLATTENS["torch_flatten"], width=width)), dry_run=True,
                                    gap_head=True)) == [kind]


def test_an_int_literal_batch_size_is_not_folded():
    assert unfolded(calibrated(Tail(POOLS["module_1"], lambda x: x.view(2, -1))))
    assert unfolded(calibrated(Tail(POOLS["module_1"], lambda x: x.reshape(2, -1))))
    gm = fuse_inference(calibrated(Tail(POOLS["module_1"], lambda x: x.view(x.shape[0], -1))), dry_run=True, gap_head=True)
    assert heads(gm) == ["fused"] and not pool_nodes(gm)


# ---- boundary -----------------------------------------------------------------------------------------------------------------------
def test_gap_head_supported_truth_table():
    ok = K.gap_head_supported
    assert ok(64, 64, 8, 8) and ok(512, 2048, 7, 7) and ok(320, 1280, 7, 7) and ok(64, 64, 1, 1) and ok(64, 64, 1, 64)
    assert not ok(64, 64, 5, 13) and not ok(64, 64, 65, 1)           # H W = 65
    assert not ok(96, 64, 8, 8) and not ok(64, 100, 8, 8) and not ok(64, 96, 8, 8) and not ok(0, 64, 8, 8)
    assert ok(2048, 64, 7, 7) and not ok(2112, 64, 7, 7)             # the slice's weights stay in LDS
    assert not ok(64, 64, 7, 7, ksize=3, padding=1) and not ok(64, 64, 7, 7, stride=2) and not ok(64, 64, 7, 7, asym=True)


def test_argument_validation_needs_no_gpu():
    """Bad arguments are rejected before anything is launched, and DLMCQ_ROUTE_ONLY launches nothing either."""
    p = ctypes.c_void_p(4096)
    gap = N.lib.dlmcq_gap_nhwc_f32
    assert gap(p, None, None, 2, 49, 64, None, None, 0, 0, 0, 0.0, None) == -1                  # neither output
    assert gap(None, p, None, 2, 49, 64, None, None, 0, 0, 0, 0.0, None) == -1                  # null input
    assert gap(p, p, None, 2, 49, 66, None, None, 0, 0, 0, 0.0, None) == -1                     # C % 4
    assert gap(p, p, None, 2, 0, 64, None, None, 0, 0, 0, 0.0, None) == -1                      # HW < 1
    assert gap(p, p, None, 2, 49, 64, None, None, 0, 0, N.FP32_IN_CHUNK_MAJOR, 0.0, None) == -1  # a chunk-major input
    assert gap(p, p, None, 2, 49, 64, None, None, 0, 0, N.ROUTE_ONLY, 0.0, None) == -1
    assert gap(p, None, p, 2, 49, 64, None, None, 0, 255, N.FORM_ZEROPOINT, 0.0, None) == -1    # codes without a scale
    assert gap(p, None, p, 2, 49, 64, p, None, 5, -5, N.FORM_ZEROPOINT, 0.0, None) == -1        # lo > hi
    assert gap(p, None, p, 2, 49, 64, p, None, -128, 127, N.FORM_QBASE | N.EMIT_SHIFT128, 0.0, None) == -1    # shifted signed codes
    assert gap(p, None, p, 2, 49, 64, p, None, 0, 255, N.FORM_ROOTQ_ACT, 0.0, None) == -1
    assert gap(None, None, None, 0, 49, 64, None, None, 0, 0, 0, 0.0, None) == 0                # empty batch: no-op

    f = N.lib.dlmcq_conv2d_i8_nhwc_gap

    def call(n=2, h=7, w=7, c=64, k=64, act=0, pooled=p, codes=None, q=(None, None, 0, 0), form=N.ROUTE_ONLY, x=p, res=None):
        return f(x, p, pooled, None, p, p, None, p, n, h, w, c, k, 1, res, act, codes, q[0], q[1], q[2], q[3], form, 0.0, None)
    assert call() == N.ROUTE_GAP and N.ROUTE_TAG[N.ROUTE_GAP] == "conv_gap"
    assert call(h=8, w=8, c=2048, k=128, act=N.ACT_RELU6, res=p, codes=p, q=(p, None, 0, 255), form=N.FORM_ZEROPOINT | N.EMIT_SHIFT128 | N.ROUTE_ONLY) == N.ROUTE_GAP
    assert call(h=9, w=9) == -1 and call(h=65, w=1) == -1                   # H W > 64
    assert call(k=96) == -1 and call(c=96) == -1 and call(c=2112) == -1
    assert call(act=3) == -1 and call(act=-1) == -1
    assert call(pooled=None) == -1 and call(x=None) == -1
    assert call(pooled=None, codes=p) == -1                                 # codes without a scale
    assert call(codes=p, q=(p, None, 0, 256)) == -1
    for bit in (N.FORCE_TILED, N.PIPELINED, N.FP32_IN_CHUNK_MAJOR, N.FP32_OUT_CHUNK_MAJOR, N.W2_CHUNK_MAJOR, N.PAD_CODE0):
        assert call(form=N.ROUTE_ONLY | bit) == -1, hex(bit)                # refused, not stripped
    assert call(pooled=ctypes.c_void_p(4100)) == -4                         # alignment
    assert call(n=0) == 0
