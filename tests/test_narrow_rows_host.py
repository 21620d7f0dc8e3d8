"""Narrow fp32 rows in the frozen int8 plan (fuse_inference(narrow_rows=True)), on the host: the plan's decisions for MobileNetV2 (FSPTQ;
QBase with float activation offsets set by hand) and the CIFAR ResNet-20 (dry run, wrappers marked calibrated by hand as in
test_relu6_host.py / test_act_offset_host.py), and the refusals of dlmcq_conv2d_i8_nhwc_narrow that need no GPU."""
import operator
import os

import pytest
import torch
from torch import nn

import workloads as W
from dlmc import _native as N
from dlmc.utils.fuse import fuse_inference
from test_act_offset_host import calibrated as qbase_mobilenet
from test_relu6_host import calibrated as fsptq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def counts(rep):
    return dict(layers=rep.layers, relu=rep.relu, relu6=rep.relu6, residual=rep.residual, emit=rep.emit, fp32_outputs=rep.fp32_outputs,
                stem=rep.stem, dual=rep.dual, act_offset=rep.act_offset, narrow=rep.narrow, skipped=list(rep.skipped))


def fp32_readers(gm):
    """The plan's convolutions whose activation argument is no other plan node's code output (the classifier behind the pool and the
    flatten is left out: gap_head is another flag)."""
    out = []
    for n in gm.graph.nodes:
        if n.op == "call_module" and n.target.startswith("_int8_"):
            a = n.args[0]
            if a.op == "call_function" and a.target is torch.flatten:
                continue
            if not (a.op == "call_function" and a.target is operator.getitem and a.args[1] == 1):
                out.append(n.target)
    return out


def graph_text(gm):
    return [(n.op, str(n.target), tuple(str(a) for a in n.args)) for n in gm.graph.nodes]


def test_mobilenet_v2_fsptq_folds_all_ten_adds():
    off = fuse_inference(fsptq(W.mobilenet_v2()), dry_run=True).fusion_report
    assert (off.residual, off.narrow) == (3, 0)
    gm = fuse_inference(fsptq(W.mobilenet_v2()), dry_run=True, narrow_rows=True)
    on = gm.fusion_report
    # 10 adds.  The padded projections that read or feed a shortcut: 24 x 2, 32 x 3, 96 x 3, 160 x 3 = 11 narrow nodes (64 and 320 are
    # unpadded; the 16-channel projection and the padded 96- / 144-channel expansions emit codes only)
    assert (on.layers, on.residual, on.relu6, on.skipped) == (53, 10, 35, [])
    assert on.narrow == 11 and "narrow fp32 rows=11" in repr(on)
    # every add is gone from the graph
    assert not [n for n in gm.graph.nodes if n.op == "call_function" and n.target in (operator.add, operator.iadd, torch.add)]
    assert fp32_readers(gm) == ["_int8_plan_0"]


def test_mobilenet_v2_qbase_offsets_only_the_first_layer_reads_fp32():
    net, neg = qbase_mobilenet(first_offset=True)
    assert neg == 18
    off = fuse_inference(net, dry_run=True, act_offsets=True)
    assert off.fusion_report.residual == 3 and len(fp32_readers(off)) == 8       # the image and the seven sums left outside
    gm = fuse_inference(net, dry_run=True, act_offsets=True, narrow_rows=True)
    on = gm.fusion_report
    assert (on.layers, on.residual, on.act_offset, on.skipped) == (53, 10, 18, [])
    assert on.narrow == 11
    assert fp32_readers(gm) == ["_int8_plan_0"]


def test_cifar_resnet20_decisions():
    net = W.cifar_resnet20()
    assert sum(isinstance(m, (nn.Conv2d, nn.Linear)) for m in net.modules()) == 22          # 19 3x3 + 2 shortcut 1x1 + the head
    assert sum(p.numel() for p in net.parameters() if p.dim() > 1) == 270896          # convolution and head weights
    off = fuse_inference(fsptq(W.cifar_resnet20()), dry_run=True).fusion_report
    # today: the three identity blocks of the 64-wide stage fold their add; its first block's 1x1 shortcut makes a dual kernel
    assert (off.residual, off.dual, off.narrow) == (3, 1, 0)
    on = fuse_inference(fsptq(W.cifar_resnet20()), dry_run=True, narrow_rows=True).fusion_report
    # all nine adds; the 32-wide stage's convolution shortcut is its own (narrow) node, the 64-wide one's still half of a dual kernel
    assert (on.residual, on.dual, on.relu) == (9, 1, off.relu + 6)
    assert on.narrow == 7 and on.layers == off.layers


@pytest.mark.parametrize("make", [lambda: fsptq(W.mobilenet_v2()), lambda: fsptq(W.cifar_resnet20()), lambda: fsptq(W.resnet18())])
def test_flag_off_is_the_plan_as_it_was(make):
    a = fuse_inference(make(), dry_run=True)
    b = fuse_inference(make(), dry_run=True, narrow_rows=False)
    assert graph_text(a) == graph_text(b)
    assert counts(a.fusion_report) == counts(b.fusion_report) and repr(a.fusion_report) == repr(b.fusion_report)
    assert "narrow" not in repr(a.fusion_report)


def test_flag_changes_nothing_without_padded_layers():
    a = fuse_inference(fsptq(W.resnet50()), dry_run=True)
    b = fuse_inference(fsptq(W.resnet50()), dry_run=True, narrow_rows=True)
    assert graph_text(a) == graph_text(b) and counts(a.fusion_report) == counts(b.fusion_report)


class PaddedBlock(nn.Module):
    """A residual block of `k` channels behind a 64 -> k convolution; `conv_shortcut`: a 1x1 convolution on the shortcut."""

    def __init__(self, k, conv_shortcut=False):
        super().__init__()
        self.stem = nn.Conv2d(64, k, 1)
        self.a = nn.Conv2d(k, 64, 3, padding=1)
        self.b = nn.Conv2d(64, k, 3, padding=1)
        self.down = nn.Conv2d(k, k, 1) if conv_shortcut else None

    def forward(self, x):
        y = torch.relu(self.stem(x))
        idt = y if self.down is None else self.down(y)
        return torch.relu(self.b(torch.relu(self.a(y))) + idt)


def adds(gm):
    return sum(n.op == "call_function" and n.target is operator.add for n in gm.graph.nodes)


def test_k_not_a_multiple_of_four_keeps_its_add_outside():
    gm = fuse_inference(fsptq(PaddedBlock(24)), dry_run=True, narrow_rows=True)
    assert (gm.fusion_report.residual, adds(gm)) == (1, 0)
    gm = fuse_inference(fsptq(PaddedBlock(22)), dry_run=True, narrow_rows=True)       # (22 input channels: `a` is no int8 layer, `b` is)
    assert (gm.fusion_report.residual, gm.fusion_report.narrow, adds(gm)) == (0, 0, 1)


def test_convolution_shortcut_on_a_padded_block_forms_no_dual_node():
    gm = fuse_inference(fsptq(PaddedBlock(32, conv_shortcut=True)), dry_run=True, narrow_rows=True)
    rep = gm.fusion_report
    assert (rep.layers, rep.dual, rep.residual, adds(gm)) == (4, 0, 1, 0)
    assert rep.narrow == 2                          # the block end and the shortcut convolution, each its own node
    rep = fuse_inference(fsptq(PaddedBlock(64, conv_shortcut=True)), dry_run=True, narrow_rows=True).fusion_report
    assert (rep.dual, rep.narrow) == (1, 0)           # unpadded: the dual kernel, as without the flag


# ------------------------------------------------------------------------------------------------- the ABI, without a GPU
def _call(K=64, Kf=24, form=N.FORM_ZEROPOINT, out=1 << 12, residual=None, codes=1 << 13):
    """dlmcq_conv2d_i8_nhwc_narrow on made-up addresses: every refusal below is decided before anything is touched or launched."""
    return N.lib.dlmcq_conv2d_i8_nhwc_narrow(1 << 8, 1 << 9, out, None, 1 << 10, 1 << 11, None, 1 << 14, None, 1, 4, 4, 64, K, 1, 1, 1, 0, 1, 1,
                                             residual, 1, codes, 1 << 15, None, 0, 255, form, 0.0, Kf, None)


def test_entry_point_is_declared_and_documented():
    header = open(os.path.join(ROOT, "include", "dlmcq.h")).read()
    assert "int dlmcq_conv2d_i8_nhwc_narrow(" in header and "int64_t Kf, dlmcq_stream_t stream);" in header
    assert "dlmcq_conv2d_i8_nhwc_narrow" in N.SIGNATURES


@pytest.mark.parametrize("K, Kf", [(64, 0), (64, -4), (64, 22), (64, 68), (128, 64), (128, 60), (192, 128), (96, 96), (60, 60), (0, 0)])
def test_kf_outside_the_rule_is_einval(K, Kf):
    assert _call(K=K, Kf=Kf) == -1


@pytest.mark.parametrize("bit", [N.PIPELINED, N.FP32_IN_CHUNK_MAJOR, N.FP32_OUT_CHUNK_MAJOR])
def test_pipelined_and_chunk_major_bits_are_einval(bit):
    assert _call(form=N.FORM_ZEROPOINT | bit) == -1
    assert _call(form=N.FORM_ZEROPOINT | bit | N.ROUTE_ONLY) == -1


def test_misaligned_tensors_are_ealign():
    assert _call(out=(1 << 12) + 4) == -4
    assert _call(residual=(1 << 16) + 8) == -4
    assert _call(codes=(1 << 13) + 4) == -4          # (4-byte aligned codes pass the other entry points; this one stores 16-byte pieces only)


def test_route_only_answers_tiled():
    for K, Kf in ((64, 24), (64, 64), (128, 96), (192, 160)):
        for extra in (0, N.FORCE_TILED, N.EMIT_SHIFT128):
            assert _call(K=K, Kf=Kf, form=N.FORM_ZEROPOINT | N.ROUTE_ONLY | extra) == N.ROUTE_TILED


def test_new_arguments_default_to_todays_path():
    import inspect
    from dlmc.quantization.scalar import kernels as Kn
    assert inspect.signature(Kn.conv2d_i8).parameters["out_channels"].default is None
    assert inspect.signature(fuse_inference).parameters["narrow_rows"].default is False
