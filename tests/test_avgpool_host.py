"""Windowed average pools in the frozen int8 plan (fuse_inference(avg_pools=True)), on the host: which pools the pass hands to the plan
(dry run, wrappers marked calibrated by hand as in test_relu6_host.py) and which it leaves exactly as they are, the option-C / -D CIFAR
ResNets of workloads.py, and the refusals of dlmcq_avgpool_nhwc_f32 that need no GPU."""
import ctypes
import operator

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import workloads as W
from dlmc import _native as N
from dlmc.utils.fuse import fuse_inference
from test_relu6_host import calibrated as fsptq


def pools(gm):
    mods = dict(gm.named_modules())
    return [n for n in gm.graph.nodes if (n.op == "call_module" and isinstance(mods.get(n.target), nn.AvgPool2d)) or
            (n.op == "call_function" and n.target in (F.avg_pool2d, torch._C._nn.avg_pool2d))]


def pool_nodes(gm):
    return [n for n in gm.graph.nodes if n.op == "call_module" and str(n.target).startswith("_int8_avgpool_")]


def listing(gm):
    return [(n.op, str(n.target), tuple(str(v) for v in n.args), tuple(sorted((k, str(v)) for k, v in n.kwargs.items()))) for n in gm.graph.nodes]


def both(make, **kw):
    return fuse_inference(fsptq(make()), dry_run=True, **kw), fuse_inference(fsptq(make()), dry_run=True, avg_pools=True, **kw)


# ------------------------------------------------------------------------------------------- the workloads
@pytest.mark.parametrize("option", ["C", "D"])
def test_shortcut_modules_follow_the_reference(option):
    """cifarresnet.py:57-87: C = AvgPool2d(stride, stride) + 1x1 / stride 1 convolution + BN where the shape changes; D = the same where
    the stride is not 1, and a 1x1 convolution + BN on every stride-1 shortcut."""
    net = W.CifarResNet(3, option=option)       # (the networks are built with the class: cifar_resnet20(option=) keeps refusing all but "A" / "B")
    blocks = [b for stage in (net.layer1, net.layer2, net.layer3) for b in stage]
    assert len(blocks) == 9
    for i, b in enumerate(blocks):
        down = b.downsample
        if i in (3, 6):
            pool, conv, bn = down
            assert type(pool) is nn.AvgPool2d and pool.kernel_size == 2 and pool.stride == 2 and pool.padding == 0
        elif option == "D":
            conv, bn = down
        else:
            assert down is None and b.subsample is None
            continue
        cin = b.conv1.in_channels
        assert type(conv) is nn.Conv2d and conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.bias is None
        assert (conv.in_channels, conv.out_channels) == (cin, b.conv2.out_channels) and type(bn) is nn.BatchNorm2d
    rows = W.layer_table(net, torch.zeros(1, 3, 32, 32))
    assert len(rows) == (22 if option == "C" else 29)
    assert tuple(net(torch.zeros(2, 3, 32, 32)).shape) == (2, 10)
    assert W.CifarResNet(9, option=option).layer2[0].downsample[0].kernel_size == 2


def test_unknown_option_raises():
    with pytest.raises(ValueError):
        W.CifarResNet(3, option="E")
    for option in ("C", "D", "E"):      # the named networks stay what they were (tests/test_pad_shortcut_host.py): "A" and "B" only
        with pytest.raises(ValueError):
            W.cifar_resnet20(option=option)
        with pytest.raises(ValueError):
            W.cifar_resnet56(option=option)
    with pytest.raises(ValueError):
        W.BasicBlock(16, 32, 2, option="E")


# ------------------------------------------------------------------------------------------- CIFAR ResNet-20 plans
@pytest.mark.parametrize("narrow", [False, True])
@pytest.mark.parametrize("option", ["C", "D"])
def test_cifar_resnet20_pools_go_on_the_plan(option, narrow):
    off, on = both(lambda: W.CifarResNet(3, option=option), narrow_rows=narrow)
    ro, rn = off.fusion_report, on.fusion_report
    assert len(pools(off)) == 2 and ro.avg_pools == 0 and "average pools" not in repr(ro)
    assert rn.avg_pools == 2 and "average pools on the plan=2" in repr(rn) and not pools(on) and len(pool_nodes(on)) == 2
    # whatever the main pass decided for the convolutions behind the pools stays
    for f in ("layers", "dual", "residual", "relu", "emit", "fp32_outputs", "narrow", "skipped", "stem"):
        assert getattr(rn, f) == getattr(ro, f), f
    assert rn.layers == (22 if option == "C" else 29)
    # the 64-wide blocks' shortcut convolutions are dual operands (option D: all three, option B's one), the 32-wide ones their own node
    assert rn.dual == (1 if option == "C" else 3)
    mods_b = fuse_inference(fsptq(W.cifar_resnet20(option="B")), dry_run=True, narrow_rows=narrow).fusion_report
    assert (mods_b.dual, mods_b.layers) == (1, 22)
    for nd in pool_nodes(on):
        gets = {u.args[1]: u for u in nd.users}
        assert set(gets) == {1} or not gets[0].users          # codes only: nothing reads the pooled fp32 tensor
        (reader,) = gets[1].users
        assert reader.op == "call_module" and str(reader.target).startswith("_int8_plan_")
        src = nd.args[0]
        if narrow:        # the block tensor in front is a plan node's fp32 output (without narrow rows the 16- / 32-wide adds stay torch ops)
            assert src.target is operator.getitem and src.args[1] == 0


@pytest.mark.parametrize("option", ["A", "B"])
def test_options_a_and_b_are_untouched(option):
    off, on = both(lambda: W.CifarResNet(3, option=option))
    assert listing(on) == listing(off)
    assert repr(on.fusion_report) == repr(off.fusion_report) and vars(on.fusion_report) == vars(off.fusion_report)
    assert on.fusion_report.avg_pools == 0


@pytest.mark.parametrize("option", ["C", "D"])
def test_flag_off_keeps_the_pools(option):
    plain = fuse_inference(fsptq(W.CifarResNet(3, option=option)), dry_run=True)
    explicit = fuse_inference(fsptq(W.CifarResNet(3, option=option)), dry_run=True, avg_pools=False)
    assert len(pools(plain)) == 2 and plain.fusion_report.avg_pools == 0
    assert listing(plain) == listing(explicit) and repr(plain.fusion_report) == repr(explicit.fusion_report)


# ------------------------------------------------------------------------------------------- three-layer toy models
class Toy(nn.Module):
    """64 -> 64 convolution + ReLU, `pool`, then `tail(pooled)`; by default one 1x1 convolution + ReLU and a third convolution."""

    def __init__(self, pool, tail=None, cin=64):
        super().__init__()
        self.a = nn.Conv2d(64, cin, 3, padding=1)
        self.b = nn.Conv2d(cin, 64, 1)
        self.c = nn.Conv2d(64, 64, 3, padding=1)
        self.pool, self.tail = pool, tail

    def forward(self, x):
        t = self.pool(torch.relu(self.a(x)))
        if self.tail is not None:
            return self.tail(self, t)
        return self.c(torch.relu(self.b(t)))


TAKEN = {
    "module": lambda: nn.AvgPool2d(2),
    "module_stride": lambda: nn.AvgPool2d(kernel_size=2, stride=2),
    "module_pair": lambda: nn.AvgPool2d((3, 3), (3, 3)),
    "module_count_include_pad_false": lambda: nn.AvgPool2d(2, count_include_pad=False),      # (no padding: nothing to count)
    "function": lambda: (lambda t: F.avg_pool2d(t, 2)),
    "function_stride": lambda: (lambda t: F.avg_pool2d(t, 2, 2)),
    "function_keywords": lambda: (lambda t: F.avg_pool2d(input=t, kernel_size=(4, 4), stride=None, padding=0, ceil_mode=False)),
    "function_pairs": lambda: (lambda t: F.avg_pool2d(t, [2, 2], [2, 2], (0, 0), False, True, None)),
    "window_8": lambda: nn.AvgPool2d(8),
}


@pytest.mark.parametrize("name", sorted(TAKEN))
def test_recognised_spellings(name):
    off, on = both(lambda: Toy(TAKEN[name]()))
    assert len(pools(off)) == 1 and not pools(on) and on.fusion_report.avg_pools == 1
    (nd,) = pool_nodes(on)
    gets = {u.args[1]: u for u in nd.users}
    assert 1 in gets and (0 not in gets or not gets[0].users)


def _two_quantisers(self, t):
    return self.b(t) + self.c(t)


def _plain_reader_only(self, t):
    return self.c(torch.relu(self.b(torch.sigmoid(t))))


LEFT_ALONE = {
    "ceil_mode": (lambda: nn.AvgPool2d(2, ceil_mode=True), None),
    "padding_1": (lambda: nn.AvgPool2d(2, padding=1), None),
    "kernel_3_stride_2": (lambda: nn.AvgPool2d(3, stride=2), None),
    "divisor_override": (lambda: nn.AvgPool2d(2, divisor_override=3), None),
    "kernel_from_the_tensor": (lambda: (lambda t: F.avg_pool2d(t, t.size(3))), None),
    "window_9": (lambda: nn.AvgPool2d(9), None),
    "window_1": (lambda: nn.AvgPool2d(1), None),
    "unequal_pair": (lambda: nn.AvgPool2d((2, 4)), None),
    "function_ceil_mode": (lambda: (lambda t: F.avg_pool2d(t, 2, ceil_mode=True)), None),
    "function_padding": (lambda: (lambda t: F.avg_pool2d(t, 2, 2, 1)), None),
    "two_quantisers": (lambda: nn.AvgPool2d(2), _two_quantisers),
    "plain_reader_only": (lambda: nn.AvgPool2d(2), _plain_reader_only),
}


@pytest.mark.parametrize("name", sorted(LEFT_ALONE))
def test_left_alone(name):
    pool, tail = LEFT_ALONE[name]

    def make():
        net = Toy(pool(), tail)
        return net

    def prep(net):
        net = fsptq(net)
        if name == "two_quantisers":
            with torch.no_grad():
                net.c.in_scale.fill_(0.5)
            assert float(net.c.in_scale.detach().reshape(-1)[0]) != float(net.b.in_scale.detach().reshape(-1)[0])
        return net
    off = fuse_inference(prep(make()), dry_run=True)
    on = fuse_inference(prep(make()), dry_run=True, avg_pools=True)
    assert listing(on) == listing(off) and len(pools(on)) == 1
    assert on.fusion_report.avg_pools == 0 and repr(on.fusion_report) == repr(off.fusion_report)


def _plan_layer_and_plain_op(self, t):
    return self.c(torch.relu(self.b(t))) + t.amax()


def test_second_plain_reader_gets_the_fp32_tensor():
    off, on = both(lambda: Toy(nn.AvgPool2d(2), _plan_layer_and_plain_op))
    assert on.fusion_report.avg_pools == 1 and not pools(on) and len(pools(off)) == 1
    (nd,) = pool_nodes(on)
    gets = {u.args[1]: u for u in nd.users}
    assert [u.target for u in gets[0].users] == ["amax"]                       # want_out: the plain op reads the pooled fp32 tensor
    assert [str(u.target)[:10] for u in gets[1].users] == ["_int8_plan"]       # the plan layer reads codes


def test_same_quantiser_twice_is_taken_once():
    def tail(self, t):
        return self.b(t) + self.c(t)
    off, on = both(lambda: Toy(nn.AvgPool2d(2), tail))        # (fsptq() leaves both readers with the same frozen quantiser)
    assert on.fusion_report.avg_pools == 1 and len(pool_nodes(on)) == 1 and not pools(on)


def test_channels_not_a_multiple_of_four_or_unplanned_readers_keep_the_pool():
    off, on = both(lambda: Toy(nn.AvgPool2d(2), cin=6))
    assert listing(on) == listing(off) and on.fusion_report.avg_pools == 0


# ------------------------------------------------------------------------------------------- the entry point, without a GPU
def _call(x=1 << 12, pooled=1 << 13, codes=1 << 14, n=2, h=8, w=8, c=16, xs=16, s=2, c_pad=16, pad_code=0, scale=1 << 15, zp=None,
          lo=0, hi=255, form=None, g=0.0):
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731
    form = N.FORM_ZEROPOINT if form is None else form
    return N.lib.dlmcq_avgpool_nhwc_f32(p(x), p(pooled), p(codes), n, h, w, c, xs, s, c_pad, pad_code, p(scale), p(zp), lo, hi, form, g, None)


REFUSED = {
    "window_1": (dict(s=1), -1), "window_9": (dict(s=9, h=16, w=16), -1), "h_below_window": (dict(h=1), -1), "w_below_window": (dict(w=1), -1),
    "c_below_4": (dict(c=0, xs=16), -1), "c_mod_4": (dict(c=6), -1), "stride_below_c": (dict(xs=12), -1), "stride_mod_4": (dict(xs=18), -1),
    "c_pad_below_c": (dict(c_pad=12), -1), "c_pad_mod_4": (dict(c_pad=18), -1), "no_output": (dict(pooled=None, codes=None), -1),
    "c_pad_without_codes": (dict(codes=None, c_pad=64), -1), "negative_n": (dict(n=-1), -1), "pad_code_300": (dict(pad_code=300), -1),
    "codes_without_scale": (dict(scale=None), -1), "lo_above_hi": (dict(lo=5, hi=4), -1), "unknown_form": (dict(form=9), -1),
    "force_tiled": (dict(form=N.FORM_ZEROPOINT | N.FORCE_TILED), -1), "route_only": (dict(form=N.FORM_ZEROPOINT | N.ROUTE_ONLY), -1),
    "pipelined": (dict(form=N.FORM_ZEROPOINT | N.PIPELINED), -1), "chunk_major_in": (dict(form=N.FORM_ZEROPOINT | N.FP32_IN_CHUNK_MAJOR), -1),
    "chunk_major_out": (dict(form=N.FORM_ZEROPOINT | N.FP32_OUT_CHUNK_MAJOR), -1),
    "shifted_signed_range": (dict(form=N.FORM_ZEROPOINT | N.EMIT_SHIFT128, lo=-128, hi=127), -1),
    "x_misaligned": (dict(x=(1 << 12) + 4), -4), "pooled_misaligned": (dict(pooled=(1 << 13) + 8), -4), "codes_misaligned": (dict(codes=(1 << 14) + 2), -4),
    "threads_reach_2_31": (dict(n=1 << 31, h=2, w=2, c=4, xs=4, c_pad=4), -2), "pixels_reach_2_31": (dict(h=1 << 16, w=1 << 15), -2),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_need_no_gpu(name):
    """Nothing is launched on these placeholder pointers: every call is answered by the argument checks."""
    kw, rc = REFUSED[name]
    assert N.lib.dlmcq_strerror(rc) and _call(**kw) == rc


def test_empty_batch_is_ok():
    assert _call(n=0) == 0
    assert _call(n=0, x=None, pooled=None, codes=None) == 0
