"""Hard-swish activations in the frozen int8 plan (fuse_inference(hardswish=True)), on the host: which spellings the pass hands to the plan
and in which order of the kernel's two multiplies (dry run, wrappers marked calibrated by hand as in test_relu6_host.py), the near misses
it leaves alone, the plan without the flag, the gate and squeeze passes beside it, the MobileNetV3 workloads beside the unchanged ones,
their recorded plans, and the refusals of dlmcq_hardswish_nhwc_f32 that need no GPU.

The recorded plans lie in tests/golden/hardswish_plans/, a directory of their own: tests/test_plan_snapshot_host.py requires
tests/golden/plans/ to hold its own cases and nothing else.  Regenerate with `python tests/test_hardswish_host.py` and review the
difference."""
import ctypes
import functools
import hashlib
import os
import re
import sys

import pytest
import torch
import torch.nn.functional as F
from torch import nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hardswish_plans")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(os.path.abspath(__file__)), ROOT, os.path.join(ROOT, "dlmc-quant_amd")]

import workloads as W  # noqa: E402
from dlmc import _native as N  # noqa: E402
from dlmc.utils.fuse import HardswishLayer, fuse_inference  # noqa: E402
from hardswish_nets import NETS  # noqa: E402
from test_relu6_host import calibrated as fsptq  # noqa: E402
from test_swish_host import REFUSED, Toy  # noqa: E402

# hard swishes on maps / of which hand activation codes on, per network (tests/test_hardswish_gpu.py reads the first).  Codes go from the
# first layer's and every expansion's hard swish to the depthwise layer behind it and, in a block without squeeze-excite, from the
# depthwise layer's to the projection; behind a squeeze-excite block's depthwise layer the pool and the gate node read fp32, and so does
# the global pool behind the last layer.  Large: 1 + 2 * 4 + 5 of 1 + 2 * 9 + 1; Small: 1 + 8 of 1 + 2 * 8 + 1.
COUNTS = {"small_net": (3, 1), "mobilenet_v3_large": (20, 14), "mobilenet_v3_small": (18, 9)}


def hardswish_nodes(gm):
    return [n for n in gm.graph.nodes if n.op == "call_module" and str(n.target).startswith("_int8_hardswish_")]


def activations_left(gm):
    """hard-swish / hard-sigmoid / ReLU6 nodes of any spelling."""
    mods = dict(gm.named_modules())
    return [n for n in gm.graph.nodes if (n.op == "call_function" and n.target in (F.hardswish, F.hardsigmoid, F.relu6, F.hardtanh)) or
            (n.op == "call_module" and isinstance(mods.get(n.target), (nn.Hardswish, nn.Hardsigmoid, nn.ReLU6)))]


def both(make, **kw):
    return fuse_inference(fsptq(make()), dry_run=True, **kw), fuse_inference(fsptq(make()), dry_run=True, hardswish=True, **kw)


def nodes_of(gm):
    return [(n.op, str(n.target), str(n.args)) for n in gm.graph.nodes]


# ------------------------------------------------------------------------------------------- the spellings and their orders
@pytest.mark.parametrize("spelling", sorted(NETS))
def test_every_spelling_is_taken_with_the_order_of_the_table(spelling):
    make, order = NETS[spelling]
    off, on = both(make, gates=True)
    assert off.fusion_report.hardswishes == 0 and "hard swishes on the plan" not in repr(off.fusion_report) and not hardswish_nodes(off)
    n, codes = COUNTS["small_net"]
    assert on.fusion_report.hardswishes == n and f"hard swishes on the plan={n}" in repr(on.fusion_report)
    mods = dict(on.named_modules())
    nodes = [mods[nd.target] for nd in hardswish_nodes(on)]
    assert len(nodes) == n and all(isinstance(m, HardswishLayer) for m in nodes)
    assert [m.order for m in nodes] == [order] * n and all(m.decision.order == order and m.decision.spelling == m.spelling for m in nodes)
    # the expansion's hard swish: codes alone, to the depthwise layer, 24 of 64 channels; the other two: fp32 alone
    first, second, third = nodes
    assert first.emit is not None and not first.want_out and (first.c, first.c_pad) == (24, 64)
    assert all(m.emit is None and m.want_out and (m.c, m.c_pad) == (None, None) for m in (second, third))
    assert sum(m.emit is not None for m in nodes) == codes
    # what is left of the spelling: the squeeze-excite gate's own relu6(v + 3) / 6 alone
    assert len(activations_left(on)) == 1 and len(activations_left(off)) >= 1 + (0 if "hardswish" in spelling.lower() else n)
    assert on.fusion_report.gates == off.fusion_report.gates == 1
    for f in ("layers", "dual", "residual", "relu", "relu6", "emit", "fp32_outputs", "narrow", "skipped", "stem"):
        assert getattr(on.fusion_report, f) == getattr(off.fusion_report, f), f      # whatever the main pass decided stays


def test_the_table_names_both_orders_and_every_spelling_of_the_issue():
    assert sorted({order for _, order in NETS.values()}) == ["gate_first", "mul_first"]
    assert {s: o for s, (_, o) in NETS.items()} == {
        "nn.Hardswish": "mul_first", "F.hardswish": "mul_first", "x * relu6(x + 3) / 6": "mul_first", "(relu6(3 + x) * x) * (1 / 6)": "mul_first",
        "x * (relu6(x + 3) / 6)": "gate_first", "(relu6(x + 3) / 6) * x": "gate_first", "x * F.hardsigmoid(x)": "gate_first",
        "nn.Hardsigmoid()(x) * x": "gate_first"}


# ------------------------------------------------------------------------------------------- near misses
def _plus_2(self, x):
    return self.b(x * F.relu6(x + 2) / 6)


def _div_5(self, x):
    return self.b(x * F.relu6(x + 3) / 5)


def _gate_div_5(self, x):
    return self.b(x * (F.relu6(x + 3) / 5))


def _relu6_read_twice(self, x):
    r = F.relu6(x + 3)
    return self.b(x * r / 6) + r


def _hardsigmoid_of_another_tensor(self, x):
    return self.b(x * F.hardsigmoid(x + 1.0))


def _relu6_of_another_tensor(self, x):
    return self.b(x * (F.relu6(self.a(x) + 3) / 6))


def _se_gate(self, x):
    return self.b(x * F.hardsigmoid(F.adaptive_avg_pool2d(x, 1)))


def _inplace_functional(self, x):
    return self.b(F.hardswish(x, inplace=True))


def _a_vector(self, x):
    return self.b(x) + F.hardswish(self.fc(x.mean((2, 3)))).view(-1, 64, 1, 1)


def _a_vector_spelled_out(self, x):
    v = self.fc(x.mean((2, 3)))
    return self.b(x) + (v * F.relu6(v + 3) / 6).view(-1, 64, 1, 1)


LEFT_ALONE = {"plus_2": _plus_2, "div_5": _div_5, "gate_div_5": _gate_div_5, "relu6_read_twice": _relu6_read_twice,
              "hardsigmoid_of_another_tensor": _hardsigmoid_of_another_tensor, "relu6_of_another_tensor": _relu6_of_another_tensor,
              "se_gate": _se_gate, "inplace_functional": _inplace_functional, "a_vector": _a_vector, "a_vector_spelled_out": _a_vector_spelled_out}


class InplaceModuleReadTwice(nn.Module):
    """nn.Hardswish(inplace=True) on a tensor the shortcut add reads too."""

    def __init__(self):
        super().__init__()
        self.a = nn.Conv2d(64, 64, 3, padding=1)
        self.act = nn.Hardswish(inplace=True)
        self.b = nn.Conv2d(64, 64, 1)

    def forward(self, inp):
        x = self.a(inp)
        return self.b(self.act(x)) + x


@pytest.mark.parametrize("name", sorted(LEFT_ALONE) + ["inplace_module_read_twice"])
def test_left_alone(name):
    make = InplaceModuleReadTwice if name == "inplace_module_read_twice" else (lambda: Toy(LEFT_ALONE[name]))
    for kw in (dict(), dict(gates=True)):
        off, on = both(make, **kw)
        assert on.fusion_report.hardswishes == 0 and str(on.graph) == str(off.graph) and repr(on.fusion_report) == repr(off.fusion_report)
        assert on.fusion_report.gates == (1 if kw and name == "se_gate" else 0)


def test_an_inplace_module_nobody_else_reads_is_taken():
    class Alone(InplaceModuleReadTwice):
        def forward(self, inp):
            return self.b(self.act(self.a(inp)))
    off, on = both(Alone)
    assert on.fusion_report.hardswishes == 1 and not activations_left(on) and len(activations_left(off)) == 1


def test_a_map_nobody_takes_as_codes_is_still_activated_by_the_node():
    off, on = both(lambda: Toy(lambda self, x: torch.tanh(x * F.hardsigmoid(x))))
    (nd,) = hardswish_nodes(on)
    m = dict(on.named_modules())[nd.target]
    gets = {u.args[1]: u for u in nd.users}
    assert m.emit is None and m.want_out and m.order == "gate_first" and [u.target for u in gets[0].users] == [torch.tanh]
    assert (1 not in gets or not gets[1].users) and not activations_left(on) and len(activations_left(off)) == 1


def test_a_node_built_by_hand_checks_its_order():
    assert HardswishLayer(None, True, None, None, 0).order == "mul_first"
    assert HardswishLayer(None, True, None, None, 0, order="gate_first").spelling == "hardsigmoid"
    with pytest.raises(ValueError):
        HardswishLayer(None, True, None, None, 0, order="division")


# ------------------------------------------------------------------------------------------- the flag off; gates and squeezes beside it
MAKERS = dict({s: m for s, (m, _) in NETS.items()}, mobilenet_v3_large=W.mobilenet_v3_large, mobilenet_v3_small=W.mobilenet_v3_small,
              mobilenet_v2_se=lambda: W.mobilenet_v2(se=True))


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_flag_off_is_the_plan_as_it_was(name):
    plain = fuse_inference(fsptq(MAKERS[name]()), dry_run=True, gates=True, dw5=True)
    explicit = fuse_inference(fsptq(MAKERS[name]()), dry_run=True, gates=True, dw5=True, hardswish=False)
    assert nodes_of(plain) == nodes_of(explicit) and repr(plain.fusion_report) == repr(explicit.fusion_report)
    assert plain.fusion_report.hardswishes == 0 and not hardswish_nodes(plain)


@pytest.mark.parametrize("name", sorted(MAKERS))
def test_gates_and_squeezes_are_those_of_the_flag_off_plan(name):
    off, on = both(MAKERS[name], gates=True, squeezes=True, dw5=True)
    ro, rn = off.fusion_report, on.fusion_report
    assert (rn.gates, rn.squeezes, rn.squeeze_left) == (ro.gates, ro.squeezes, ro.squeeze_left)
    want = dict(mobilenet_v3_large=(8, 8), mobilenet_v3_small=(9, 9), mobilenet_v2_se=(17, 17)).get(name, (1, 1))
    assert (rn.gates, rn.squeezes) == want
    assert rn.hardswishes == (0 if name == "mobilenet_v2_se" else COUNTS.get(name, COUNTS["small_net"])[0])
    for f in ("layers", "dual", "residual", "relu", "relu6", "emit", "fp32_outputs", "narrow", "skipped", "stem", "dw5"):
        assert getattr(rn, f) == getattr(ro, f), f


# ------------------------------------------------------------------------------------------- the workloads
@pytest.mark.parametrize("name, params, hs, se", [("mobilenet_v3_large", 5483032, 21, 8), ("mobilenet_v3_small", 2542856, 19, 9)])
def test_mobilenet_v3(name, params, hs, se):
    net = getattr(W, name)().eval()
    assert sum(p.numel() for p in net.parameters()) == params
    assert sum(isinstance(m, nn.Hardswish) for m in net.modules()) == hs               # (one of them on the classifier's vector)
    blocks = [m for m in net.modules() if isinstance(m, W.SqueezeExcite)]
    assert len(blocks) == se and all(m.gate == "hardsigmoid" and m.squeeze == "conv" and m.reduce.out_channels % 8 == 0 for m in blocks)
    assert not any(isinstance(m, (nn.ReLU6, W.Swish)) for m in net.modules())
    with torch.no_grad():
        assert tuple(net(torch.zeros(1, 3, 64, 64)).shape) == (1, 1000)
    # torchvision's layout: every BatchNorm behind its convolution under merge_bn's default mapping
    from dlmc.utils.merge_bn import DEFAULT_CONV_MAPPING_FN
    mods = dict(net.named_modules())
    bns = [n for n, m in mods.items() if isinstance(m, nn.BatchNorm2d)]
    assert bns and all(isinstance(mods.get(DEFAULT_CONV_MAPPING_FN(n)), nn.Conv2d) for n in bns)
    assert name not in W.MODELS


def _modules_digest(net):
    text = "\n".join(f"{n} {type(m).__name__} {getattr(m, 'inplace', '')}" for n, m in net.named_modules())
    return hashlib.sha256(text.encode()).hexdigest()[:16], sum(p.numel() for p in net.parameters())


def test_the_other_mobile_networks_are_module_for_module_what_they_were():
    """The digests are those of the tree before `_conv_bn_act` learnt "relu" and "hardswish"."""
    assert _modules_digest(W.mobilenet_v2()) == ("fdf309877bbb524c", 3504872)
    assert _modules_digest(W.efficientnet_b0()) == ("960fa4f7f0f339df", 5288548)
    for act in ("relu6", "swish"):
        kinds = {type(m) for m in W._conv_bn_act(8, 8, 3, act=act)}
        assert kinds == {nn.Conv2d, nn.BatchNorm2d, nn.ReLU6 if act == "relu6" else W.Swish}
    assert isinstance(W._conv_bn_act(8, 8, 3, act="relu")[2], nn.ReLU) and type(W._conv_bn_act(8, 8, 3, act="hardswish")[2]) is nn.Hardswish
    with pytest.raises(ValueError):
        W._conv_bn_act(8, 8, 3, act="gelu")


# ------------------------------------------------------------------------------------------- the recorded plans
CASES = {f"{name}-dw5_True-gates_True{'-hardswish_True' if on else ''}-dry": (name, on)
         for name in ("mobilenet_v3_large", "mobilenet_v3_small") for on in (False, True)}


@functools.lru_cache(maxsize=None)
def plan(case):
    name, on = CASES[case]
    return fuse_inference(fsptq(getattr(W, name)()), dry_run=True, gates=True, dw5=True, **(dict(hardswish=True) if on else {}))


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_is_the_recorded_plan(case):
    from plan_dump import plan_text
    with open(os.path.join(GOLDEN, case + ".txt")) as f:
        assert plan_text(plan(case)) == f.read()
    assert sorted(os.listdir(GOLDEN)) == sorted(c + ".txt" for c in CASES)


@pytest.mark.parametrize("case", sorted(c for c in CASES if "hardswish_True" in c))
def test_what_the_recorded_plan_says(case):
    gm = plan(case)
    n, codes = COUNTS[CASES[case][0]]
    mods = dict(gm.named_modules())
    nodes = [mods[nd.target] for nd in hardswish_nodes(gm)]
    assert gm.fusion_report.hardswishes == len(nodes) == n and sum(m.emit is not None for m in nodes) == codes
    assert all(m.order == "mul_first" and m.spelling == "hardswish" and (m.want_out or m.emit is not None) for m in nodes)
    # codes AND fp32 from one launch: Large's first layer alone, whose map the first block's depthwise layer and its shortcut add read
    assert [i for i, m in enumerate(nodes) if m.want_out and m.emit is not None] == ([0] if "large" in case else [])
    # what stays: the hard swish on the classifier's vector and the hard sigmoid of every squeeze path
    left = [nd for nd in activations_left(gm) if nd.op == "call_module" and isinstance(mods[nd.target], nn.Hardswish)]
    assert [nd.target for nd in left] == ["classifier.1"] and gm.fusion_report.skipped == []


# ------------------------------------------------------------------------------------------- header, exports, ctypes table
def test_header_exports_and_ctypes_table_agree():
    with open(os.path.join(ROOT, "include", "dlmcq.h")) as f:
        header = f.read()
    (decl,) = re.findall(r"\nint dlmcq_hardswish_nhwc_f32\(([^;]*)\);", header)
    params = [p.strip() for p in decl.replace("\n", " ").split(",")]
    kinds = [ctypes.c_void_p if "*" in p or p.startswith("dlmcq_stream_t") else {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
             "float": ctypes.c_float}[p.split()[0]] for p in params]
    res, args = N.SIGNATURES["dlmcq_hardswish_nhwc_f32"]
    assert res is ctypes.c_int and list(args) == kinds and len(args) == 18 and params[-2] == "int32_t order"
    fn = N.lib.dlmcq_hardswish_nhwc_f32
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == kinds
    swish = N.SIGNATURES["dlmcq_swish_nhwc_f32"][1]               # the swish entry point's arguments, `order` in front of the stream
    assert list(args) == list(swish[:-1]) + [ctypes.c_int32] + list(swish[-1:])
    assert re.search(r"#define DLMCQ_HSWISH_MUL_FIRST 0\n#define DLMCQ_HSWISH_GATE_FIRST 1\n", header)
    assert (N.HSWISH_MUL_FIRST, N.HSWISH_GATE_FIRST) == (0, 1) and N.lib.dlmcq_version() == 100


# ------------------------------------------------------------------------------------------- the entry point, without a GPU
def _call(x=1 << 12, out=1 << 13, codes=1 << 14, n=2, h=8, w=8, c=16, xs=16, c_pad=16, pad_code=0, scale=1 << 15, zp=None, lo=0, hi=255,
          form=None, g=0.0, order=0):
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731
    form = N.FORM_ZEROPOINT if form is None else form
    return N.lib.dlmcq_hardswish_nhwc_f32(p(x), p(out), p(codes), n, h, w, c, xs, c_pad, pad_code, p(scale), p(zp), lo, hi, form, g, order, None)


@pytest.mark.parametrize("order", [-1, 2])
def test_an_order_outside_the_two_is_refused_first(order):
    """Nothing is launched on these placeholder pointers: every call is answered by the argument checks."""
    assert _call(order=order) == -1
    assert _call(order=order, n=0) == -1                            # before N == 0
    assert _call(order=order, x=(1 << 12) + 4) == -1               # before the alignment (which alone is -4)
    assert _call(order=order, n=1 << 31, h=1, w=1, c=4, xs=4, c_pad=4) == -1      # before the 2^31 limits (which alone are -2)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_need_no_gpu(name, order):
    """test_swish_host.py's table: the same argument sets, the same codes."""
    kw, rc = REFUSED[name]
    assert N.lib.dlmcq_strerror(rc) and _call(order=order, **kw) == rc


@pytest.mark.parametrize("order", [0, 1])
def test_empty_batch_is_ok(order):
    assert _call(n=0, order=order) == 0
    assert _call(n=0, x=None, out=None, codes=None, order=order) == 0


if __name__ == "__main__":
    from plan_dump import plan_text
    os.makedirs(GOLDEN, exist_ok=True)
    for case in sorted(CASES):
        with open(os.path.join(GOLDEN, case + ".txt"), "w") as f:
            f.write(plan_text(plan(case)))
        print(case)
