"""Squeeze-excite gates in the frozen int8 plan (fuse_inference(gates=True)), on the host: which multiplies the pass hands to the plan
(dry run, wrappers marked calibrated by hand as in test_relu6_host.py) and which it leaves exactly as they are, the MobileNetV2-SE
workload beside the unchanged default one, and the refusals of dlmcq_gate_nhwc_f32 that need no GPU."""
import ctypes
import json
import operator
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import workloads as W
from dlmc import _native as N
from dlmc.utils.fuse import fuse_inference
from gate_nets import GhostSE, MBConvSE, RepVGGSE
from test_relu6_host import calibrated as fsptq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def muls(gm):
    return [n for n in gm.graph.nodes if (n.op == "call_function" and n.target in (operator.mul, torch.mul, operator.imul)) or
            (n.op == "call_method" and n.target in ("mul", "mul_"))]


def gate_nodes(gm):
    return [n for n in gm.graph.nodes if n.op == "call_module" and str(n.target).startswith("_int8_gate_")]


def both(make, **kw):
    return fuse_inference(fsptq(make()), dry_run=True, **kw), fuse_inference(fsptq(make()), dry_run=True, gates=True, **kw)


# ------------------------------------------------------------------------------------------- the three spellings
@pytest.mark.parametrize("name, make, act_gone", [("mbconv", MBConvSE, None), ("ghost", GhostSE, None), ("repvgg", RepVGGSE, "relu")])
def test_gate_goes_on_the_plan(name, make, act_gone):
    off, on = both(make)
    ro, rn = off.fusion_report, on.fusion_report
    n_mul = len(muls(off))
    assert ro.gates == 0 and "gates on the plan" not in repr(ro) and not gate_nodes(off)
    assert rn.gates == 1 and "gates on the plan=1" in repr(rn)
    assert len(muls(on)) == n_mul - 1                         # the gate's multiply is gone (a swish inside the squeeze stays)
    (nd,) = gate_nodes(on)
    gets = {u.args[1]: u for u in nd.users}
    assert 1 in gets and (0 not in gets or not gets[0].users)          # codes only: nothing reads the gated fp32 tensor
    (reader,) = gets[1].users
    assert reader.op == "call_module" and str(reader.target).startswith("_int8_plan_") and reader.args[0] is gets[1]
    # the node reads the map and the gate; the map is also what the squeeze's pool reads
    x, g = nd.args
    assert any(u is not nd and u.op == "call_module" and str(u.target).endswith("pool") for u in x.users)
    if act_gone:                                               # the ReLU behind the multiply went into the node
        count = lambda gm: sum(1 for n in gm.graph.nodes if n.op == "call_function" and n.target in (torch.relu, F.relu))  # noqa: E731
        assert count(on) == count(off) - 1
    # whatever the main pass decided stays
    for f in ("layers", "dual", "residual", "relu", "relu6", "emit", "fp32_outputs", "narrow", "skipped", "stem"):
        assert getattr(rn, f) == getattr(ro, f), f


def test_mobilenet_v2_se_gates():
    off, on = both(lambda: W.mobilenet_v2(se=True))
    assert off.fusion_report.gates == 0 and on.fusion_report.gates == 17 and len(gate_nodes(on)) == 17
    assert len(muls(off)) == 17 and not muls(on)
    for nd in gate_nodes(on):
        gets = {u.args[1]: u for u in nd.users}
        assert [str(u.target)[:10] for u in gets[1].users] == ["_int8_plan"] and (0 not in gets or not gets[0].users)


# ------------------------------------------------------------------------------------------- gates left as they are
class Toy(nn.Module):
    """64 -> 64 convolution + ReLU, a squeeze (pool, 1x1 convolution, sigmoid) and `tail(self, x, g)`."""

    def __init__(self, tail):
        super().__init__()
        self.a = nn.Conv2d(64, 64, 3, padding=1)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Conv2d(64, 64, 1)
        self.b = nn.Conv2d(64, 64, 1)
        self.c = nn.Conv2d(64, 64, 3, padding=1)
        self.tail = tail

    def forward(self, x):
        return self.tail(self, torch.relu(self.a(x)))


def _tensor_sized_pool(self, x):
    return self.b(x * torch.sigmoid(self.fc(F.avg_pool2d(x, x.size(3)))))


def _pooled_from_another_tensor(self, x):
    return self.b(x * torch.sigmoid(self.fc(self.pool(x + 1.0))))


def _two_quantisers(self, x):
    t = x * torch.sigmoid(self.fc(self.pool(x)))
    return self.b(t) + self.c(t)


def _inplace(self, x):
    return self.b(x.mul_(torch.sigmoid(self.fc(self.pool(x)))))


def _spatial_gate(self, x):
    return self.b(x * torch.sigmoid(self.fc(x)))


def _plain_reader_only(self, x):
    return self.b(torch.tanh(x * torch.sigmoid(self.fc(self.pool(x)))))


LEFT_ALONE = {"tensor_sized_pool": _tensor_sized_pool, "pooled_from_another_tensor": _pooled_from_another_tensor,
              "two_quantisers": _two_quantisers, "inplace_mul": _inplace, "spatial_gate": _spatial_gate,
              "plain_reader_only": _plain_reader_only}


@pytest.mark.parametrize("name", sorted(LEFT_ALONE))
def test_left_alone(name):
    def prep():
        net = fsptq(Toy(LEFT_ALONE[name]))
        if name == "two_quantisers":
            with torch.no_grad():
                net.c.in_scale.fill_(0.5)
            assert float(net.c.in_scale.detach().reshape(-1)[0]) != float(net.b.in_scale.detach().reshape(-1)[0])
        return net
    off = fuse_inference(prep(), dry_run=True)
    on = fuse_inference(prep(), dry_run=True, gates=True)
    assert on.fusion_report.gates == 0 and str(on.graph) == str(off.graph)
    assert repr(on.fusion_report) == repr(off.fusion_report) and len(muls(on)) == 1


def _taken(self, x):
    return self.b(x * torch.sigmoid(self.fc(self.pool(x))))


def _second_plain_reader(self, x):
    t = torch.mul(torch.sigmoid(self.fc(x.mean((2, 3), keepdim=True))), x)          # the gate first, torch.mul, the mean spelling
    return self.b(t) + t.amax()


def test_the_toy_itself_is_taken_and_a_plain_reader_gets_fp32():
    off, on = both(lambda: Toy(_taken))
    assert on.fusion_report.gates == 1 and not muls(on) and len(muls(off)) == 1
    off, on = both(lambda: Toy(_second_plain_reader))
    assert on.fusion_report.gates == 1 and not muls(on)
    (nd,) = gate_nodes(on)
    gets = {u.args[1]: u for u in nd.users}
    assert [u.target for u in gets[0].users] == ["amax"] and [str(u.target)[:10] for u in gets[1].users] == ["_int8_plan"]
    assert nd.args[0].users and nd.args[1].target is torch.sigmoid          # (x, g) whichever side of the multiply they stood on


# ------------------------------------------------------------------------------------------- the flag off, the default workload
def test_flag_off_is_the_default_plan():
    plain = fuse_inference(fsptq(W.mobilenet_v2()), dry_run=True)
    explicit = fuse_inference(fsptq(W.mobilenet_v2()), dry_run=True, gates=False)
    on = fuse_inference(fsptq(W.mobilenet_v2()), dry_run=True, gates=True)          # no gate in the default network: nothing to take
    assert str(plain.graph) == str(explicit.graph) == str(on.graph)
    assert repr(plain.fusion_report) == repr(explicit.fusion_report) == repr(on.fusion_report) and plain.fusion_report.gates == 0


def test_default_mobilenet_v2_is_what_it_was():
    """tests/golden/mobilenet_v2_state.json: the state_dict keys and shapes, the modules in order and four weight sums under seed 2333,
    written from the commit before `se=` existed."""
    with open(os.path.join(ROOT, "tests", "golden", "mobilenet_v2_state.json")) as f:
        pinned = json.load(f)
    torch.manual_seed(pinned["seed"])
    net = W.mobilenet_v2()
    sd = net.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == pinned["keys"]
    assert [[n, type(m).__name__] for n, m in net.named_modules()] == pinned["modules"]
    for k, want in pinned["checksum"].items():
        assert float(sd[k].double().sum()) == want, k
    assert not any(isinstance(m, W.SqueezeExcite) for m in net.modules())
    se = W.mobilenet_v2(se=True)
    assert sum(isinstance(m, W.SqueezeExcite) for m in se.modules()) == 17
    assert tuple(se.eval()(torch.zeros(1, 3, 32, 32)).shape) == (1, 1000)
    with pytest.raises(ValueError):
        W.SqueezeExcite(16, 8, gate="tanh")


# ------------------------------------------------------------------------------------------- the entry point, without a GPU
def _call(x=1 << 12, gate=1 << 16, out=1 << 13, codes=1 << 14, n=2, h=8, w=8, c=16, xs=16, c_pad=16, pad_code=0, act=0, scale=1 << 15,
          zp=None, lo=0, hi=255, form=None, g=0.0):
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731
    form = N.FORM_ZEROPOINT if form is None else form
    return N.lib.dlmcq_gate_nhwc_f32(p(x), p(gate), p(out), p(codes), n, h, w, c, xs, c_pad, pad_code, act, p(scale), p(zp), lo, hi, form, g, None)


REFUSED = {
    "h_0": (dict(h=0), -1), "w_0": (dict(w=0), -1), "c_below_4": (dict(c=0), -1), "c_mod_4": (dict(c=6), -1),
    "stride_below_c": (dict(xs=12), -1), "stride_mod_4": (dict(xs=18), -1), "c_pad_below_c": (dict(c_pad=12), -1),
    "c_pad_mod_4": (dict(c_pad=18), -1), "no_output": (dict(out=None, codes=None), -1), "c_pad_without_codes": (dict(codes=None, c_pad=64), -1),
    "negative_n": (dict(n=-1), -1), "pad_code_300": (dict(pad_code=300), -1), "pad_code_minus_129": (dict(pad_code=-129), -1),
    "act_3": (dict(act=3), -1), "act_minus_1": (dict(act=-1), -1), "null_x": (dict(x=None), -1), "null_gate": (dict(gate=None), -1),
    "codes_without_scale": (dict(scale=None), -1), "lo_above_hi": (dict(lo=5, hi=4), -1), "unknown_form": (dict(form=9), -1),
    "force_tiled": (dict(form=N.FORM_ZEROPOINT | N.FORCE_TILED), -1), "route_only": (dict(form=N.FORM_ZEROPOINT | N.ROUTE_ONLY), -1),
    "pipelined": (dict(form=N.FORM_ZEROPOINT | N.PIPELINED), -1), "chunk_major_in": (dict(form=N.FORM_ZEROPOINT | N.FP32_IN_CHUNK_MAJOR), -1),
    "chunk_major_out": (dict(form=N.FORM_ZEROPOINT | N.FP32_OUT_CHUNK_MAJOR), -1),
    "shifted_signed_range": (dict(form=N.FORM_ZEROPOINT | N.EMIT_SHIFT128, lo=-128, hi=127), -1),
    "x_misaligned": (dict(x=(1 << 12) + 4), -4), "gate_misaligned": (dict(gate=(1 << 16) + 8), -4), "out_misaligned": (dict(out=(1 << 13) + 8), -4),
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
    assert _call(n=0, x=None, gate=None, out=None, codes=None) == 0
