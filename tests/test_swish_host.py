"""Swish activations in the frozen int8 plan (fuse_inference(swish=True)), on the host: which spellings the pass hands to the plan (dry
run, wrappers marked calibrated by hand as in test_relu6_host.py), who gets codes and who the fp32 map, the gate pass behind it, the
plan without the flag, the MBConv workload beside the unchanged default one, and the refusals of dlmcq_swish_nhwc_f32 that need no
GPU."""
import ctypes
import operator
import os
import re

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import workloads as W
from dlmc import _native as N
from dlmc.utils.fuse import SwishLayer, fuse_inference
from swish_nets import FunctionalSiLU, ModuleSiLU, MulSwish
from test_relu6_host import calibrated as fsptq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def swish_nodes(gm):
    return [n for n in gm.graph.nodes if n.op == "call_module" and str(n.target).startswith("_int8_swish_")]


def gate_nodes(gm):
    return [n for n in gm.graph.nodes if n.op == "call_module" and str(n.target).startswith("_int8_gate_")]


def activations_left(gm):
    """sigmoid / silu nodes of any spelling."""
    mods = dict(gm.named_modules())
    return [n for n in gm.graph.nodes if (n.op == "call_function" and n.target in (torch.sigmoid, F.sigmoid, F.silu)) or
            (n.op == "call_method" and n.target == "sigmoid") or (n.op == "call_module" and isinstance(mods.get(n.target), (nn.SiLU, nn.Sigmoid)))]


def readers(nd):
    """{0: the readers of the node's fp32 output, 1: of its codes} as target-name prefixes."""
    gets = {u.args[1]: u for u in nd.users}
    return {i: sorted(str(u.target)[:10] for u in g.users) for i, g in gets.items() if g.users}


def both(make, **kw):
    return fuse_inference(fsptq(make()), dry_run=True, **kw), fuse_inference(fsptq(make()), dry_run=True, swish=True, **kw)


# ------------------------------------------------------------------------------------------- the three spellings
def test_mul_spelling_and_a_second_fp32_reader():
    off, on = both(MulSwish)
    assert off.fusion_report.swishes == 0 and "swishes on the plan" not in repr(off.fusion_report) and not swish_nodes(off)
    assert on.fusion_report.swishes == 2 and "swishes on the plan=2" in repr(on.fusion_report)
    assert len(activations_left(off)) == 2 and not activations_left(on)
    first, second = swish_nodes(on)
    mods = dict(on.named_modules())
    # the first: codes to `b`, the fp32 map to the shortcut add folded into `b2`
    assert readers(first) == {0: ["_int8_plan"], 1: ["_int8_plan"]}
    m = mods[first.target]
    assert isinstance(m, SwishLayer) and m.want_out and m.emit is not None and (m.c, m.c_pad) == (64, 64)
    # the second: codes alone
    assert readers(second) == {1: ["_int8_plan"]}
    m = mods[second.target]
    assert not m.want_out and m.emit is not None and (m.c, m.c_pad) == (64, 64)
    for f in ("layers", "dual", "residual", "relu", "relu6", "emit", "fp32_outputs", "narrow", "skipped", "stem"):
        assert getattr(on.fusion_report, f) == getattr(off.fusion_report, f), f      # whatever the main pass decided stays


def test_module_spelling_depthwise_reader_and_padded_rows():
    off, on = both(ModuleSiLU)
    assert on.fusion_report.swishes == 2 and len(activations_left(off)) == 2 and not activations_left(on)
    mods = dict(on.named_modules())
    for nd in swish_nodes(on):
        m = mods[nd.target]
        assert readers(nd) == {1: ["_int8_plan"]} and not m.want_out and (m.c, m.c_pad) == (48, 64) and not m.emit_shift


def test_functional_spelling():
    off, on = both(FunctionalSiLU)
    assert on.fusion_report.swishes == 2 and len(activations_left(off)) == 2 and not activations_left(on)
    mods = dict(on.named_modules())
    assert [(mods[nd.target].c, mods[nd.target].c_pad, mods[nd.target].want_out) for nd in swish_nodes(on)] == [(32, 64, False), (64, 64, False)]


class Toy(nn.Module):
    def __init__(self, tail):
        super().__init__()
        self.a = nn.Conv2d(64, 64, 3, padding=1)
        self.b = nn.Conv2d(64, 64, 1)
        self.fc = nn.Linear(64, 64)
        self.tail = tail

    def forward(self, x):
        return self.tail(self, self.a(x))


def _inplace_functional(self, x):
    return self.b(F.silu(x, inplace=True))


def _sigmoid_read_twice(self, x):
    s = torch.sigmoid(x)
    return self.b(x * s) + s


def _sigmoid_of_another_tensor(self, x):
    return self.b(x * torch.sigmoid(x + 1.0))


def _a_vector(self, x):
    v = self.fc(x.mean((2, 3)))
    return self.b(x) + (v * torch.sigmoid(v)).view(-1, 64, 1, 1)


LEFT_ALONE = {"inplace_functional": _inplace_functional, "sigmoid_read_twice": _sigmoid_read_twice,
              "sigmoid_of_another_tensor": _sigmoid_of_another_tensor, "a_vector": _a_vector}


@pytest.mark.parametrize("name", sorted(LEFT_ALONE))
def test_left_alone(name):
    off, on = both(lambda: Toy(LEFT_ALONE[name]))
    assert on.fusion_report.swishes == 0 and str(on.graph) == str(off.graph) and repr(on.fusion_report) == repr(off.fusion_report)


def test_a_map_nobody_takes_as_codes_is_still_activated_by_the_node():
    off, on = both(lambda: Toy(lambda self, x: torch.tanh(x * torch.sigmoid(x))))
    (nd,) = swish_nodes(on)
    m = dict(on.named_modules())[nd.target]
    gets = {u.args[1]: u for u in nd.users}
    assert m.emit is None and m.want_out and [u.target for u in gets[0].users] == [torch.tanh] and (1 not in gets or not gets[1].users)
    assert not activations_left(on) and len(activations_left(off)) == 1


# ------------------------------------------------------------------------------------------- the gate pass behind a swish
@pytest.mark.parametrize("se", [False, True])
def test_mbconv_workload(se):
    make = lambda: W.mobilenet_v2(se=se, act="swish")  # noqa: E731
    off = fuse_inference(fsptq(make()), dry_run=True, gates=True)
    on = fuse_inference(fsptq(make()), dry_run=True, gates=True, swish=True)
    ro, rn = off.fusion_report, on.fusion_report
    gates = 17 if se else 0
    assert (ro.swishes, rn.swishes) == (0, 35) and ro.gates == rn.gates == gates and len(gate_nodes(on)) == gates
    mods = dict(on.named_modules())
    nodes = [mods[nd.target] for nd in swish_nodes(on)]
    # without SE every swish but the head's feeds plan convolutions alone; with SE the 17 behind the depthwise layers are read by the
    # squeeze's pool and the gate node (fp32), the head's by the global pool
    assert sum(m.emit is None for m in nodes) == (18 if se else 1) and all(m.want_out == (m.emit is None) for m in nodes)
    # what is left: the swish on the (N, mid) vector inside each squeeze and the gate's own sigmoid
    assert len(activations_left(on)) == 2 * gates and len(activations_left(off)) == 35 + 2 * gates
    for nd in gate_nodes(on):                                  # the gated map IS a swish node's fp32 output, and so is the pool's input
        x, g = nd.args
        assert x.op == "call_function" and x.target is operator.getitem and x.args[0] in swish_nodes(on) and x.args[1] == 0
        assert any(u.op == "call_module" and str(u.target).endswith("pool") for u in x.users)
    for f in ("layers", "dual", "residual", "relu", "relu6", "emit", "fp32_outputs", "narrow", "skipped", "stem"):
        assert getattr(rn, f) == getattr(ro, f), f
    assert len(gate_nodes(off)) == gates                       # a swish multiply in front of the gate is no gate, flag or no flag


def test_workload_default_is_unchanged_and_swish_runs():
    torch.manual_seed(3)
    a = W.mobilenet_v2()
    torch.manual_seed(3)
    b = W.mobilenet_v2(act="relu6")
    assert [(k, tuple(v.shape)) for k, v in a.state_dict().items()] == [(k, tuple(v.shape)) for k, v in b.state_dict().items()]
    assert all(torch.equal(u, v) for u, v in zip(a.state_dict().values(), b.state_dict().values()))
    assert [type(m).__name__ for m in a.modules()] == [type(m).__name__ for m in b.modules()]
    net = W.mobilenet_v2(se=True, act="swish").eval()
    assert sum(isinstance(m, W.Swish) for m in net.modules()) == 35 and not any(isinstance(m, nn.ReLU6) for m in net.modules())
    se = [m for m in net.modules() if isinstance(m, W.SqueezeExcite)]
    assert len(se) == 17 and all(m.gate == "sigmoid" and m.squeeze == "linear" for m in se)
    assert all(m.kernel_size == (3, 3) for m in net.modules() if isinstance(m, nn.Conv2d) and m.groups > 1)
    assert tuple(net(torch.zeros(1, 3, 32, 32)).shape) == (1, 1000)
    with pytest.raises(ValueError):
        W.mobilenet_v2(act="gelu")


# ------------------------------------------------------------------------------------------- the flag off
@pytest.mark.parametrize("make", [W.mobilenet_v2, lambda: W.mobilenet_v2(se=True), lambda: W.mobilenet_v2(se=True, act="swish"), MulSwish],
                         ids=["mobilenet_v2", "mobilenet_v2_se", "mbconv", "mul_swish"])
def test_flag_off_is_the_plan_as_it_was(make):
    plain = fuse_inference(fsptq(make()), dry_run=True, gates=True)
    explicit = fuse_inference(fsptq(make()), dry_run=True, gates=True, swish=False)
    assert [(n.op, str(n.target), str(n.args)) for n in plain.graph.nodes] == [(n.op, str(n.target), str(n.args)) for n in explicit.graph.nodes]
    assert repr(plain.fusion_report) == repr(explicit.fusion_report) and plain.fusion_report.swishes == 0 and not swish_nodes(plain)


def test_no_swish_in_the_network_nothing_to_take():
    off, on = both(lambda: W.mobilenet_v2(se=True), gates=True)
    assert str(off.graph) == str(on.graph) and repr(off.fusion_report) == repr(on.fusion_report)


# ------------------------------------------------------------------------------------------- header, exports, ctypes table
def test_header_exports_and_ctypes_table_agree():
    with open(os.path.join(ROOT, "include", "dlmcq.h")) as f:
        header = f.read()
    (decl,) = re.findall(r"\nint dlmcq_swish_nhwc_f32\(([^;]*)\);", header)
    params = [p.strip() for p in decl.replace("\n", " ").split(",")]
    kinds = [ctypes.c_void_p if "*" in p or p.startswith("dlmcq_stream_t") else {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
             "float": ctypes.c_float}[p.split()[0]] for p in params]
    res, args = N.SIGNATURES["dlmcq_swish_nhwc_f32"]
    assert res is ctypes.c_int and list(args) == kinds and len(args) == 17
    fn = N.lib.dlmcq_swish_nhwc_f32
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == kinds
    assert N.lib.dlmcq_version() == 100
    gate = N.SIGNATURES["dlmcq_gate_nhwc_f32"][1]                 # the gate entry point's arguments without `gate` and `act`
    assert list(args) == list(gate[:1]) + list(gate[2:11]) + list(gate[12:])


# ------------------------------------------------------------------------------------------- the entry point, without a GPU
def _call(x=1 << 12, out=1 << 13, codes=1 << 14, n=2, h=8, w=8, c=16, xs=16, c_pad=16, pad_code=0, scale=1 << 15, zp=None, lo=0, hi=255,
          form=None, g=0.0):
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731
    form = N.FORM_ZEROPOINT if form is None else form
    return N.lib.dlmcq_swish_nhwc_f32(p(x), p(out), p(codes), n, h, w, c, xs, c_pad, pad_code, p(scale), p(zp), lo, hi, form, g, None)


REFUSED = {
    "h_0": (dict(h=0), -1), "w_0": (dict(w=0), -1), "c_below_4": (dict(c=0), -1), "c_mod_4": (dict(c=6), -1),
    "stride_below_c": (dict(xs=12), -1), "stride_mod_4": (dict(xs=18), -1), "c_pad_below_c": (dict(c_pad=12), -1),
    "c_pad_mod_4": (dict(c_pad=18), -1), "no_output": (dict(out=None, codes=None), -1), "c_pad_without_codes": (dict(codes=None, c_pad=64), -1),
    "negative_n": (dict(n=-1), -1), "pad_code_300": (dict(pad_code=300), -1), "pad_code_minus_129": (dict(pad_code=-129), -1),
    "null_x": (dict(x=None), -1), "codes_without_scale": (dict(scale=None), -1), "lo_above_hi": (dict(lo=5, hi=4), -1),
    "unknown_form": (dict(form=9), -1),
    "force_tiled": (dict(form=N.FORM_ZEROPOINT | N.FORCE_TILED), -1), "route_only": (dict(form=N.FORM_ZEROPOINT | N.ROUTE_ONLY), -1),
    "pipelined": (dict(form=N.FORM_ZEROPOINT | N.PIPELINED), -1), "chunk_major_in": (dict(form=N.FORM_ZEROPOINT | N.FP32_IN_CHUNK_MAJOR), -1),
    "chunk_major_out": (dict(form=N.FORM_ZEROPOINT | N.FP32_OUT_CHUNK_MAJOR), -1),
    "shifted_signed_range": (dict(form=N.FORM_ZEROPOINT | N.EMIT_SHIFT128, lo=-128, hi=127), -1),
    "x_misaligned": (dict(x=(1 << 12) + 4), -4), "out_misaligned": (dict(out=(1 << 13) + 8), -4),
    "codes_misaligned": (dict(codes=(1 << 14) + 2), -4),
    "threads_reach_2_31": (dict(n=1 << 31, h=1, w=1, c=4, xs=4, c_pad=4), -2), "pixels_reach_2_31": (dict(n=1, h=1 << 16, w=1 << 15), -2),
    "padded_threads_reach_2_31": (dict(n=1 << 10, h=1 << 10, w=1 << 6, c=4, xs=4, c_pad=128), -2),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_need_no_gpu(name):
    """Nothing is launched on these placeholder pointers: every call is answered by the argument checks."""
    kw, rc = REFUSED[name]
    assert N.lib.dlmcq_strerror(rc) and _call(**kw) == rc


def test_empty_batch_is_ok():
    assert _call(n=0) == 0
    assert _call(n=0, x=None, out=None, codes=None) == 0
