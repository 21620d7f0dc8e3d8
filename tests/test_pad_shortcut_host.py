"""Option-A shortcuts (subsample + zero-pad) in the frozen int8 plan (fuse_inference(pad_shortcuts=True)), on the host: which spellings of
`F.pad(x[:, :, ::s, ::s], (0, 0, 0, 0, lo, hi))` the pass folds into the layer's epilogue and which it leaves exactly as they are (dry run,
wrappers marked calibrated by hand as in test_narrow_rows_host.py), the option-A CIFAR ResNet of workloads.py, and the refusals of
dlmcq_conv2d_i8_nhwc_padres that need no GPU."""
import inspect
import operator
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import workloads as W
from dlmc import _native as N
from dlmc.utils.fuse import fuse_inference
from test_narrow_rows_host import counts, graph_text
from test_relu6_host import calibrated as fsptq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Block(nn.Module):
    """A 64 -> cin convolution (the source: a plan node's fp32 output), then a residual block cin -> 64 -> k whose shortcut is
    `short(y)`; `extra(result, shortcut pieces)` adds further readers.  stride: of the block's first convolution."""

    def __init__(self, short, cin=64, k=128, stride=2, extra=None, down=False, from_input=False):
        super().__init__()
        self.stem = None if from_input else nn.Conv2d(64, cin, 1)
        self.a = nn.Conv2d(cin, 64, 3, stride=stride, padding=1)
        self.b = nn.Conv2d(64, k, 3, padding=1)
        self.down = nn.Conv2d(k, k, 1) if down else None
        self.short, self.extra = short, extra

    def forward(self, x):
        y = x if self.stem is None else torch.relu(self.stem(x))
        pieces = self.short(y)
        pieces = pieces if isinstance(pieces, tuple) else (pieces,)
        idt = pieces[0] if self.down is None else self.down(pieces[0])
        out = torch.relu(self.b(torch.relu(self.a(y))) + idt)
        return out if self.extra is None else self.extra(out, pieces)


def sub2(y):
    return y[:, :, ::2, ::2]


def pad_nodes(gm):
    return [n for n in gm.graph.nodes if n.op == "call_function" and n.target in (F.pad, torch._C._nn.pad)]


def slice_nodes(gm):
    return [n for n in gm.graph.nodes if n.op == "call_function" and n.target is operator.getitem and isinstance(n.args[1], tuple)]


def adds(gm):
    return [n for n in gm.graph.nodes if n.op == "call_function" and n.target in (operator.add, operator.iadd, torch.add)]


RECOGNISED = {
    "positional": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 32, 32), "constant", 0), {}),
    "keyword": (lambda y: F.pad(sub2(y), pad=(0, 0, 0, 0, 32, 32), mode="constant", value=0.0), {}),
    "keyword_input": (lambda y: F.pad(input=sub2(y), pad=[0, 0, 0, 0, 32, 32]), {}),
    "value_float": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 32, 32), "constant", 0.0), {}),
    "value_omitted": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 32, 32)), {}),
    "value_none": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 32, 32), value=None), {}),
    "unequal_pads": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 8, 56)), {}),
    "no_pad_in_front": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 0, 64)), {}),
    "pad_without_slice": (lambda y: F.pad(y, (0, 0, 0, 0, 32, 32)), dict(stride=1)),
    "slice_stride_1": (lambda y: F.pad(y[:, :, ::1, ::1], (0, 0, 0, 0, 32, 32)), dict(stride=1)),
    "stride_3": (lambda y: F.pad(y[:, :, ::3, ::3], (0, 0, 0, 0, 32, 32)), dict(stride=3)),
    "network_input_is_the_source": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 32, 32)), dict(from_input=True)),
    "same_width": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 0, 0)), dict(k=64)),
}


@pytest.mark.parametrize("name", sorted(RECOGNISED))
def test_recognised_spellings(name):
    short, kw = RECOGNISED[name]
    off = fuse_inference(fsptq(Block(short, **kw)), dry_run=True)
    gm = fuse_inference(fsptq(Block(short, **kw)), dry_run=True, pad_shortcuts=True)
    rep = gm.fusion_report
    assert len(pad_nodes(off)) == 1 and off.fusion_report.pad_shortcuts == 0 and "pad shortcuts" not in repr(off.fusion_report)
    assert rep.pad_shortcuts == 1 and "pad shortcuts=1" in repr(rep)
    assert not pad_nodes(gm) and not slice_nodes(gm) and not adds(gm)
    assert counts(rep) == counts(off.fusion_report)             # the add was folded before, with the materialised tensor
    # the node reads the source itself: the stem's fp32 output, or the network input
    node = [n for n in gm.graph.nodes if n.op == "call_module" and len(n.args) == 2][0]
    src = node.args[1]
    assert src.op == "placeholder" if kw.get("from_input") else (src.target is operator.getitem and src.args[1] == 0)


def _second_reader_of_pad(out, pieces):
    return out + pieces[0].amax()


def _second_reader_of_slice(out, pieces):
    return out + pieces[1].amax()


def _pad_and_slice(y):
    t = sub2(y)
    return F.pad(t, (0, 0, 0, 0, 32, 32)), t


LEFT_ALONE = {
    "non_zero_value": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 32, 32), "constant", 1.0), {}, {}),
    "mode_reflect": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 32, 32), mode="reflect"), {}, {}),
    "mode_replicate_positional": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 32, 32), "replicate"), {}, {}),
    "spatial_pad": (lambda y: F.pad(sub2(y), (0, 0, 1, 1, 32, 32)), {}, {}),
    "spatial_pad_w": (lambda y: F.pad(sub2(y), (1, 0, 0, 0, 32, 32)), {}, {}),
    "four_entry_pad": (lambda y: F.pad(sub2(y), (0, 0, 0, 0)), {}, {}),
    "eight_entry_pad": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 32, 32, 0, 0)), {}, {}),
    "negative_channel_pad": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, -4, 68)), {}, {}),
    "lo_not_a_multiple_of_4": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 30, 34)), {}, {}),
    "slice_with_a_start": (lambda y: F.pad(y[:, :, 1::2, ::2], (0, 0, 0, 0, 32, 32)), {}, {}),
    "slice_with_a_stop": (lambda y: F.pad(y[:, :, ::2, :8:2], (0, 0, 0, 0, 32, 32)), {}, {}),
    "strides_differ": (lambda y: F.pad(y[:, :, ::2, ::1], (0, 0, 0, 0, 32, 32)), {}, {}),
    "slice_on_the_channel_axis": (lambda y: F.pad(y[:, :32, ::2, ::2], (0, 0, 0, 0, 48, 48)), {}, {}),
    "slice_on_the_batch_axis": (lambda y: F.pad(y[::1, :, ::2, ::2], (0, 0, 0, 0, 32, 32)), {}, {}),
    "ellipsis": (lambda y: F.pad(y[..., ::2, ::2], (0, 0, 0, 0, 32, 32)), {}, {}),
    "pad_read_twice": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 32, 32)), dict(extra=_second_reader_of_pad), {}),
    "slice_read_twice": (_pad_and_slice, dict(extra=_second_reader_of_slice), {}),
    "widths_do_not_add_up": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 32, 28)), {}, {}),
    "padded_source_without_narrow_rows": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 16, 16)), dict(cin=32, k=64), {}),
    "layer_with_a_dual_partner": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 32, 32)), dict(down=True), {}),
    "padded_layer_without_narrow_rows": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 16, 16)), dict(cin=64, k=96), {}),
    "source_channels_not_a_multiple_of_4": (lambda y: F.pad(sub2(y), (0, 0, 0, 0, 4, 2)), dict(cin=22, k=28), dict(narrow_rows=True)),
}


@pytest.mark.parametrize("name", sorted(LEFT_ALONE))
def test_everything_else_is_left_exactly_as_today(name):
    short, kw, fkw = LEFT_ALONE[name]
    off = fuse_inference(fsptq(Block(short, **kw)), dry_run=True, **fkw)
    on = fuse_inference(fsptq(Block(short, **kw)), dry_run=True, pad_shortcuts=True, **fkw)
    assert graph_text(on) == graph_text(off)
    assert counts(on.fusion_report) == counts(off.fusion_report) and repr(on.fusion_report) == repr(off.fusion_report)
    assert on.fusion_report.pad_shortcuts == 0 and len(pad_nodes(on)) == 1 and len(slice_nodes(on)) == 1
    if name == "layer_with_a_dual_partner":
        assert on.fusion_report.dual == 1


def _qbase_block(offset_on_b, **kw):
    """The block under QBase, marked calibrated by hand as test_act_offset_host.py does; `offset_on_b`: the float activation offset of
    the block's last convolution (3x3, padding 1: a non-zero one puts it on the *_xoff kernel with its border term)."""
    import copy
    from dlmc.quantization.scalar.modules.base import QBase
    from dlmc.utils.quantize import quantize_model
    from test_act_offset_host import QBASE_W4A8
    net = Block(lambda y: F.pad(sub2(y), (0, 0, 0, 0, 32, 32)), **kw)
    quantize_model(net, copy.deepcopy(QBASE_W4A8), None)
    for m in net.modules():
        if isinstance(m, QBase):
            m.in_init_state.fill_(1)
            m.wt_init_state.fill_(1)
            m.in_offset = torch.tensor([offset_on_b if m is net.b else 0.0])
    return net.eval()


def test_a_layer_with_a_float_offset_border_term_is_left_alone():
    # the *_xoff kernels have no narrow form: the add keeps folding with the materialised tensor, as it does today
    off = fuse_inference(_qbase_block(-0.625), dry_run=True, act_offsets=True)
    on = fuse_inference(_qbase_block(-0.625), dry_run=True, act_offsets=True, pad_shortcuts=True)
    assert off.fusion_report.act_offset == 1 and off.fusion_report.residual == 1 and off.fusion_report.skipped == []
    assert graph_text(on) == graph_text(off) and repr(on.fusion_report) == repr(off.fusion_report)
    assert on.fusion_report.pad_shortcuts == 0 and len(pad_nodes(on)) == 1 and len(slice_nodes(on)) == 1
    # ... the same block without the offset is taken
    gm = fuse_inference(_qbase_block(0.0), dry_run=True, act_offsets=True, pad_shortcuts=True)
    assert gm.fusion_report.pad_shortcuts == 1 and gm.fusion_report.act_offset == 0 and not pad_nodes(gm) and not slice_nodes(gm)


def test_a_padded_source_is_taken_once_it_is_narrow():
    short, kw, _ = LEFT_ALONE["padded_source_without_narrow_rows"]
    gm = fuse_inference(fsptq(Block(short, **kw)), dry_run=True, pad_shortcuts=True, narrow_rows=True)
    assert (gm.fusion_report.pad_shortcuts, gm.fusion_report.narrow) == (1, 1) and not pad_nodes(gm) and not slice_nodes(gm)
    # ... and a padded LAYER (96 of 128 columns) once its add folds at all
    short, kw, _ = LEFT_ALONE["padded_layer_without_narrow_rows"]
    gm = fuse_inference(fsptq(Block(short, **kw)), dry_run=True, pad_shortcuts=True, narrow_rows=True)
    assert (gm.fusion_report.pad_shortcuts, gm.fusion_report.narrow, gm.fusion_report.residual) == (1, 1, 1) and not pad_nodes(gm)


@pytest.mark.parametrize("make", [lambda: W.cifar_resnet20(), lambda: W.resnet18(), lambda: W.mobilenet_v2(), lambda: W.resnet50()])
def test_networks_without_such_shortcuts_get_the_plan_they_get_today(make):
    for fkw in ({}, dict(narrow_rows=True)):
        a = fuse_inference(fsptq(make()), dry_run=True, **fkw)
        b = fuse_inference(fsptq(make()), dry_run=True, pad_shortcuts=True, **fkw)
        assert graph_text(a) == graph_text(b)
        assert counts(a.fusion_report) == counts(b.fusion_report) and repr(a.fusion_report) == repr(b.fusion_report)


def test_cifar_resnet20_option_a_decisions():
    off = fuse_inference(fsptq(W.cifar_resnet20(option="A")), dry_run=True, narrow_rows=True)
    ro = off.fusion_report
    assert (ro.layers, ro.residual, ro.dual, ro.skipped) == (20, 9, 0, []) and len(pad_nodes(off)) == 2 and len(slice_nodes(off)) == 2
    gm = fuse_inference(fsptq(W.cifar_resnet20(option="A")), dry_run=True, narrow_rows=True, pad_shortcuts=True)
    rep = gm.fusion_report
    assert rep.pad_shortcuts == 2 and counts(rep) == counts(ro)
    assert not pad_nodes(gm) and not slice_nodes(gm) and not adds(gm)
    # without narrow rows only the 32 -> 64 transition's add folds at all, and its source (32 of 64 columns, sliced) is not dense
    gm = fuse_inference(fsptq(W.cifar_resnet20(option="A")), dry_run=True, pad_shortcuts=True)
    assert gm.fusion_report.pad_shortcuts == 0 and len(pad_nodes(gm)) == 2


def test_flag_defaults_to_todays_path():
    from dlmc.quantization.scalar import kernels as Kn
    assert inspect.signature(fuse_inference).parameters["pad_shortcuts"].default is False
    assert inspect.signature(W.cifar_resnet20).parameters["option"].default == "B"
    assert inspect.signature(W.CifarResNet.__init__).parameters["option"].default == "B"
    assert not isinstance(Kn.PadShortcut, torch.Tensor) and not issubclass(Kn.PadShortcut, torch.Tensor)


# ------------------------------------------------------------------------------------------------- the workload
def test_option_a_layer_table_is_option_b_minus_the_two_shortcut_convolutions():
    x = torch.zeros(1, 3, 32, 32)
    b, a = W.layer_table(W.cifar_resnet20(), x), W.layer_table(W.cifar_resnet20(option="A"), x)
    assert len(b) == 22 and len(a) == 20
    assert [r for r in b if ".downsample." not in r[0]] == a
    assert [r[3] for r in b if ".downsample." in r[0]] == [(32, 16, 1, 1), (64, 32, 1, 1)]
    assert W.table_totals(W.layer_table(W.cifar_resnet56(option="A"), x))[0] == 56
    with pytest.raises(ValueError):
        W.cifar_resnet20(option="C")


def test_default_network_is_todays_bit_for_bit():
    torch.manual_seed(5)
    a = W.cifar_resnet20()
    torch.manual_seed(5)
    b = W.CifarResNet(3, 10, option="B")
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) for k in sa)
    assert sum(".downsample.0.weight" in k for k in sa) == 2


def _by_hand(net, x):
    """The option-A network with its shortcut restated pixel by pixel: every other pixel of x, the new channels zero on both sides."""
    x = torch.relu(net.bn1(net.conv1(x)))
    for stage in (net.layer1, net.layer2, net.layer3):
        for blk in stage:
            out = blk.bn2(blk.conv2(torch.relu(blk.bn1(blk.conv1(x)))))
            if out.shape == x.shape:
                sc = x
            else:
                sc = torch.zeros_like(out)
                lo = (out.shape[1] - x.shape[1]) // 2
                for i in range(out.shape[2]):
                    for j in range(out.shape[3]):
                        sc[:, lo:lo + x.shape[1], i, j] = x[:, :, 2 * i, 2 * j]
            x = torch.relu(out + sc)
    return net.fc(torch.flatten(net.avgpool(x), 1))


@pytest.mark.parametrize("side", [8, 7])
def test_option_a_forward_is_subsample_pad_add(side):
    torch.manual_seed(11)
    net = W.cifar_resnet20(option="A").eval()
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    assert not any(isinstance(m, nn.Conv2d) and m.kernel_size == (1, 1) for m in net.modules())
    x = torch.randn(2, 3, side, side)
    with torch.no_grad():
        got, want = net(x), _by_hand(net, x)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())


# ------------------------------------------------------------------------------------------------- the ABI, without a GPU
def _call(K=64, Kf=32, form=N.FORM_ZEROPOINT, out=1 << 12, src=1 << 16, codes=1 << 13, hw=4, rh=7, rw=8, rc=16, rs=2, clo=8, stride=1):
    """dlmcq_conv2d_i8_nhwc_padres on made-up addresses: every refusal below is decided before anything is touched or launched.  A 1x1
    convolution over hw x hw pixels, its shortcut subsampled from an rh x rw source."""
    return N.lib.dlmcq_conv2d_i8_nhwc_padres(1 << 8, 1 << 9, out, None, 1 << 10, 1 << 11, None, 1 << 14, None, 1, hw, hw, 64, K, 1, 1, stride, 0, 1, 1,
                                             src, rh, rw, rc, rs, clo, 1, codes, 1 << 15, None, 0, 255, form, 0.0, Kf, None)


def test_entry_point_is_declared_and_documented():
    header = open(os.path.join(ROOT, "include", "dlmcq.h")).read()
    assert "int dlmcq_conv2d_i8_nhwc_padres(" in header and "-0 + +0 = +0" in header
    assert "dlmcq_conv2d_i8_nhwc_padres" in N.SIGNATURES
    n_narrow, n_pad = len(N.SIGNATURES["dlmcq_conv2d_i8_nhwc_narrow"][1]), len(N.SIGNATURES["dlmcq_conv2d_i8_nhwc_padres"][1])
    assert n_pad == n_narrow + 5            # `residual` replaced by six arguments


def test_a_valid_call_routes_to_the_tiled_kernel():
    for extra in (0, N.FORCE_TILED, N.EMIT_SHIFT128):
        assert _call(form=N.FORM_ZEROPOINT | N.ROUTE_ONLY | extra) == N.ROUTE_TILED
    assert _call(form=N.ROUTE_ONLY | N.FORM_ZEROPOINT, rh=8, rw=7) == N.ROUTE_TILED                  # ceil(8 / 2) = ceil(7 / 2) = 4
    assert _call(form=N.ROUTE_ONLY | N.FORM_ZEROPOINT, K=64, Kf=64, rc=32, clo=16) == N.ROUTE_TILED  # Kf == K
    assert _call(form=N.ROUTE_ONLY | N.FORM_ZEROPOINT, rh=4, rw=4, rs=1, rc=32, clo=0) == N.ROUTE_TILED
    assert _call(form=N.ROUTE_ONLY | N.FORM_ZEROPOINT, rc=4, clo=28) == N.ROUTE_TILED


@pytest.mark.parametrize("bad", [dict(src=None), dict(rs=0), dict(rs=-1), dict(rh=9), dict(rh=6), dict(rw=9), dict(rw=6), dict(rh=0), dict(rc=0),
                                 dict(rc=2, clo=0), dict(rc=6), dict(rc=18), dict(clo=6), dict(clo=-4), dict(rc=16, clo=20), dict(rc=36, clo=0),
                                 dict(Kf=30), dict(Kf=0), dict(K=128, Kf=64, rc=16), dict(K=96, Kf=96), dict(rs=1), dict(hw=3)],
                         ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_refusals_are_einval(bad):
    assert _call(**bad) == -1
    assert _call(form=N.FORM_ZEROPOINT | N.ROUTE_ONLY, **bad) == -1


@pytest.mark.parametrize("bit", [N.PIPELINED, N.FP32_IN_CHUNK_MAJOR, N.FP32_OUT_CHUNK_MAJOR])
def test_pipelined_and_chunk_major_bits_are_einval(bit):
    assert _call(form=N.FORM_ZEROPOINT | bit) == -1
    assert _call(form=N.FORM_ZEROPOINT | bit | N.ROUTE_ONLY) == -1


def test_misaligned_tensors_are_ealign():
    assert _call(src=(1 << 16) + 4) == -4
    assert _call(src=(1 << 16) + 8) == -4
    assert _call(out=(1 << 12) + 4) == -4
    assert _call(codes=(1 << 13) + 4) == -4
