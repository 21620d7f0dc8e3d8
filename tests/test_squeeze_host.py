"""The squeeze path on the int8 plan (fuse_inference(squeezes=True)), on the host: header, exports and ctypes table;
every refusal of dlmcq_squeeze_gate_i8 and K.squeeze_gate without a GPU; the dry-run decisions for the squeeze-excite workloads; one
small model per refusal reason of the pass; and the plan without the flag, which is the recorded one."""
import copy
import ctypes
import os
import re

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import workloads as W
from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import SqueezeLayer, fuse_inference
from test_gap_host import CFG, calibrated

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
NAME = "dlmcq_squeeze_gate_i8"


# ------------------------------------------------------------------------------------------- header, exports, ctypes table
def test_header_exports_and_ctypes_table_agree():
    with open(os.path.join(ROOT, "include", "dlmcq.h")) as f:
        header = f.read()
    (decl,) = re.findall(r"\nint " + NAME + r"\(([^;]*)\);", header)
    params = [p.strip() for p in decl.replace("\n", " ").split(",")]
    kinds = [ctypes.c_void_p if "*" in p or p.startswith("dlmcq_stream_t") else {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
             "float": ctypes.c_float}[p.split()[0]] for p in params]
    res, args = N.SIGNATURES[NAME]
    assert res is ctypes.c_int and list(args) == kinds and len(args) == 26
    fn = getattr(N.lib, NAME)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == kinds
    for macro, value in (("DLMCQ_SQUEEZE_MAX_C", N.SQUEEZE_MAX_C), ("DLMCQ_SQUEEZE_MAX_R", N.SQUEEZE_MAX_R), ("DLMCQ_SQUEEZE_IMAGES", N.SQUEEZE_IMAGES),
                         ("DLMCQ_SQUEEZE_NONE", N.SQUEEZE_NONE), ("DLMCQ_SQUEEZE_RELU", N.SQUEEZE_RELU), ("DLMCQ_SQUEEZE_SWISH", N.SQUEEZE_SWISH),
                         ("DLMCQ_GATE_NONE", N.GATE_NONE), ("DLMCQ_GATE_SIGMOID", N.GATE_SIGMOID), ("DLMCQ_GATE_HARDSIGMOID", N.GATE_HARDSIGMOID)):
        assert re.search(rf"#define {macro} {value}\n", header), macro
    with open(os.path.join(ROOT, "dlmc-quant_amd", "csrc", "Makefile")) as f:
        assert " squeeze_i8.hip " in f.read()


# ------------------------------------------------------------------------------------------- the entry point, without a GPU
A = 1 << 12      # placeholder addresses, 16-byte aligned and apart


def _call(x=A, w1=2 * A, wsum1=3 * A, bias1=4 * A, s1=5 * A, zp1=6 * A, ws1=7 * A, inner=0, w2=8 * A, wsum2=9 * A, bias2=10 * A, ws2=11 * A,
          fn=0, gate=12 * A, hidden=13 * A, n=2, c=16, r4=4, uns=1, scale=14 * A, zp=None, lo=0, hi=255, form=None, g=0.0):
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731
    form = N.FORM_ZEROPOINT if form is None else form
    return getattr(N.lib, NAME)(p(x), p(w1), p(wsum1), p(bias1), p(s1), p(zp1), p(ws1), inner, p(w2), p(wsum2), p(bias2), p(ws2), fn, p(gate),
                                p(hidden), n, c, r4, uns, p(scale), p(zp), lo, hi, form, g, None)


REFUSED = {
    "negative_n": (dict(n=-1), -1), "c_below_4": (dict(c=0), -1), "c_mod_4": (dict(c=18), -1), "c_above_2048": (dict(c=2052), -1),
    "r4_0": (dict(r4=0), -1), "r4_mod_4": (dict(r4=6), -1), "r4_above_512": (dict(r4=516), -1),
    "inner_act_3": (dict(inner=3), -1), "inner_act_negative": (dict(inner=-1), -1), "gate_fn_3": (dict(fn=3), -1), "gate_fn_negative": (dict(fn=-1), -1),
    "no_scale": (dict(scale=None), -1), "lo_above_hi": (dict(lo=5, hi=4), -1), "range_beyond_a_byte": (dict(lo=-128, hi=255), -1),
    "range_neither_u8_nor_s8": (dict(lo=-1, hi=200), -1), "range_neither_at_the_edge": (dict(lo=-1, hi=128), -1),
    "unknown_form": (dict(form=9), -1), "rootq_form": (dict(form=N.FORM_ROOTQ_ACT), -1),
    "shifted_emission": (dict(form=N.FORM_ZEROPOINT | N.EMIT_SHIFT128), -1), "force_tiled": (dict(form=N.FORM_ZEROPOINT | N.FORCE_TILED), -1),
    "route_only": (dict(form=N.FORM_ZEROPOINT | N.ROUTE_ONLY), -1), "chunk_major_out": (dict(form=N.FORM_ZEROPOINT | N.FP32_OUT_CHUNK_MAJOR), -1),
    "no_output": (dict(gate=None, hidden=None), -1),
    "null_x": (dict(x=None), -1), "null_w1": (dict(w1=None), -1), "null_wsum1": (dict(wsum1=None), -1), "null_in_scale1": (dict(s1=None), -1),
    "null_w_scale1": (dict(ws1=None), -1), "null_w2": (dict(w2=None), -1), "null_wsum2": (dict(wsum2=None), -1), "null_w_scale2": (dict(ws2=None), -1),
    "w1_misaligned": (dict(w1=2 * A + 4), -4), "w2_misaligned": (dict(w2=8 * A + 8), -4), "gate_misaligned": (dict(gate=12 * A + 4), -4),
    "hidden_misaligned": (dict(hidden=13 * A + 8), -4), "x_misaligned": (dict(x=A + 2), -4), "bias1_misaligned": (dict(bias1=4 * A + 1), -4),
    "wsum2_misaligned": (dict(wsum2=9 * A + 2), -4), "q_scale_misaligned": (dict(scale=14 * A + 3), -4),
    "codes_reach_2_31": (dict(n=1 << 20, c=2048), -2), "hidden_reaches_2_31": (dict(n=1 << 22, c=4, r4=512), -2),
    # two faults at once: the earlier check answers (geometry, quantiser, the empty problem, pointers, alignment, 2^31)
    "geometry_before_quantiser": (dict(c=18, scale=None), -1), "quantiser_before_empty": (dict(n=0, form=9), -1),
    "mixed_range_before_empty": (dict(n=0, lo=-1, hi=200), -1), "mixed_range_before_pointers": (dict(lo=-1, hi=200, w1=2 * A + 4), -1),
    "quantiser_before_pointers": (dict(scale=None, w1=2 * A + 4), -1), "null_before_alignment": (dict(w2=None, w1=2 * A + 4), -1),
    "alignment_before_range": (dict(n=1 << 20, c=2048, gate=12 * A + 4), -4), "no_output_before_alignment": (dict(gate=None, hidden=None, x=A + 2), -1),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_need_no_gpu(name):
    """Nothing is launched on these placeholder pointers: every call is answered by the argument checks."""
    kw, rc = REFUSED[name]
    assert N.lib.dlmcq_strerror(rc) and _call(**kw) == rc


def test_empty_batch_is_ok():
    assert _call(n=0) == 0
    assert _call(n=0, x=None, w1=None, w2=None, gate=None, hidden=None) == 0
    assert _call(n=0, c=18) == -1 and _call(n=0, scale=None) == -1      # (the geometry and the quantiser are checked first)


def test_optional_pointers_may_be_null():
    """bias1, bias2, the two zero points: NULL passes the checks (the call is then refused by the one fault it still has)."""
    assert _call(bias1=None, bias2=None, zp1=None, zp=None, gate=12 * A + 4) == -4
    assert _call(bias1=None, bias2=None, zp1=None, zp=None, n=1 << 20, c=2048) == -2


# ------------------------------------------------------------------------------------------- the wrapper, without a GPU
def _operands(n=3, c=8, r=2):
    g = torch.Generator().manual_seed(1)
    w1 = torch.randint(-5, 6, (r, c), generator=g, dtype=torch.int8)
    w2 = torch.randint(-5, 6, (c, r), generator=g, dtype=torch.int8)
    l1 = dict(wq=w1, wsum=w1.sum(1, dtype=torch.int32), bias=torch.zeros(r), in_scale=torch.tensor([0.5]), in_zp=torch.tensor([3.0]), w_scale=torch.ones(r))
    l2 = dict(wq=w2, wsum=w2.sum(1, dtype=torch.int32), bias=torch.zeros(c), w_scale=torch.ones(c))
    codes = torch.randint(0, 256, (n, c), generator=g, dtype=torch.uint8)
    return codes, l1, l2, K.EmitCodes(torch.tensor([0.25]), torch.tensor([2.0]), 0, 255, N.FORM_ZEROPOINT)


def _wrapper_refusals():
    codes, l1, l2, emit = _operands()
    shifted = K.EmitCodes(emit.scale, emit.zero_point, 0, 255, N.FORM_ZEROPOINT, shift128=True)
    cases = {
        "inner_act": (dict(inner_act="gelu"), ValueError, "inner_act"), "gate_fn": (dict(gate_fn="tanh"), ValueError, "gate_fn"),
        "nothing": (dict(want_gate=False), ValueError, "nothing to produce"), "no_quantiser": (dict(emit=None), ValueError, "quantiser"),
        "shifted": (dict(emit=shifted), ValueError, "shift128"),
        "mixed_range": (dict(emit=K.EmitCodes(emit.scale, emit.zero_point, -1, 200, N.FORM_ZEROPOINT)), ValueError, "neither"),
        "shifted_before_mixed_range": (dict(emit=shifted, codes=codes.float()), ValueError, "shift128"),
        "codes_fp32": (dict(codes=codes.float()), ValueError, "activation codes"), "codes_4d": (dict(codes=codes[:, :, None, None]), ValueError, "activation codes"),
        "w1_width": (dict(l1=dict(l1, wq=l1["wq"][:, :4])), ValueError, "layer 1's weight codes"),
        "w1_dtype": (dict(l1=dict(l1, wq=l1["wq"].to(torch.int16))), ValueError, "layer 1's weight codes"),
        "w2_shape": (dict(l2=dict(l2, wq=l2["wq"].t().contiguous())), ValueError, "layer 2's weight codes"),
        "wsum1": (dict(l1=dict(l1, wsum=l1["wsum"].long())), ValueError, "layer 1's wsum"),
        "wsum2": (dict(l2=dict(l2, wsum=l2["wsum"][:3])), ValueError, "layer 2's wsum"),
        "bias1": (dict(l1=dict(l1, bias=torch.zeros(5))), ValueError, "layer 1's bias"),
        "bias2": (dict(l2=dict(l2, bias=torch.zeros(8, dtype=torch.float64))), ValueError, "layer 2's bias"),
        "w_scale1": (dict(l1=dict(l1, w_scale=torch.ones(3))), ValueError, "layer 1's w_scale"),
        "w_scale2": (dict(l2=dict(l2, w_scale=torch.ones(3))), ValueError, "layer 2's w_scale"),
        "cpu": (dict(), N.DlmcqError, "GPU only"),
        # two faults at once: the earlier check answers
        "name_before_nothing": (dict(inner_act="gelu", want_gate=False), ValueError, "inner_act"),
        "nothing_before_quantiser": (dict(want_gate=False, emit=None), ValueError, "nothing to produce"),
        "codes_before_weights": (dict(codes=codes.float(), l1=dict(l1, wq=l1["wq"][:, :4])), ValueError, "activation codes"),
        "shape_before_gpu": (dict(l2=dict(l2, wsum=l2["wsum"][:3])), ValueError, "layer 2's wsum"),
    }
    base = dict(codes=codes, l1=l1, inner_act="relu", emit=emit, l2=l2, gate_fn="sigmoid", want_gate=True, want_hidden=False)
    return {k: (dict(base, **kw), exc, text) for k, (kw, exc, text) in cases.items()}


WRAPPER = _wrapper_refusals()


@pytest.mark.parametrize("fn", ["squeeze_gate", "squeeze_gate_torch"])
@pytest.mark.parametrize("name", sorted(WRAPPER))
def test_wrapper_refusals_need_no_gpu(name, fn):
    kw, exc, text = WRAPPER[name]
    with pytest.raises(exc, match=text):
        getattr(K, fn)(**kw)


def test_widths_the_kernel_takes():
    ok = K.squeeze_gate_supported
    assert ok(4, 1) and ok(2048, 512) and ok(32, 8) and ok(1152, 48) and ok(960, 240) and ok(144, 6) and ok(2048, 509)
    assert not ok(2, 1) and not ok(18, 4) and not ok(2052, 4) and not ok(64, 513) and not ok(64, 0)


# ------------------------------------------------------------------------------------------- the pass, dry run
@pytest.fixture(scope="module")
def nets():
    return {"efficientnet_b0": (calibrated(W.efficientnet_b0()), dict(gates=True, swish=True, dw5=True)),
            "mobilenet_v2_se": (calibrated(W.mobilenet_v2(se=True)), dict(gates=True)),
            "mobilenet_v2_se_swish": (calibrated(W.mobilenet_v2(se=True, act="swish")), dict(gates=True, swish=True))}


def _squeeze_nodes(gm):
    return [m for m in gm.modules() if isinstance(m, SqueezeLayer)]


def test_efficientnet_b0_decisions(nets):
    net, kw = nets["efficientnet_b0"]
    off = fuse_inference(net, dry_run=True, **kw).fusion_report
    gm = fuse_inference(net, dry_run=True, squeezes=True, **kw)
    rep = gm.fusion_report
    assert rep.squeezes == 16 and rep.gates == 16 == off.gates and rep.skipped == [] and rep.squeeze_left == []
    assert len(off.skipped) == 28 and rep.swishes == off.swishes
    # four `reduce` layers (1152 in-features) were plan layers of the main pass: they leave `int8 layers`
    assert rep.layers == off.layers - 4
    nodes = _squeeze_nodes(gm)
    assert len(nodes) == 16
    assert sorted({(m.c, m.r) for m in nodes}) == [(32, 8), (96, 4), (144, 6), (240, 10), (480, 20), (672, 28), (1152, 48)]
    for m in nodes:
        d = m.decision
        assert (m.inner, m.gate_fn, m.rank4, m.r4) == ("swish", "sigmoid", True, (m.r + 3) // 4 * 4)
        assert d.layer1.endswith(".reduce") and d.layer2.endswith(".expand") and d.planned == ((m.c == 1152), False)
        assert m.act1.key == d.q1.key and m.act2.key == d.q2.key and not hasattr(m, "w1")
        with pytest.raises(RuntimeError, match="dry_run"):
            m(torch.zeros(1, m.c, 2, 2))
    assert "squeezes on the plan=16" in repr(rep) and "squeezes on the plan" not in repr(off)
    assert not any(n.op == "call_module" and n.target.endswith((".pool", ".reduce", ".expand")) and ".conv." in n.target for n in gm.graph.nodes)


@pytest.mark.parametrize("name", ["mobilenet_v2_se", "mobilenet_v2_se_swish"])
def test_mobilenet_v2_se_decisions(nets, name):
    net, kw = nets[name]
    off = fuse_inference(net, dry_run=True, **kw).fusion_report
    gm = fuse_inference(net, dry_run=True, squeezes=True, **kw)
    rep = gm.fusion_report
    assert rep.squeezes == 17 and rep.gates == 17 == off.gates and rep.skipped == [] and rep.squeeze_left == []
    nodes = _squeeze_nodes(gm)
    planned = sum(sum(m.decision.planned) for m in nodes)
    assert rep.layers == off.layers - planned and len(off.skipped) == 34 - planned
    want = ("relu", "hardsigmoid") if name == "mobilenet_v2_se" else ("swish", "sigmoid")
    assert all((m.inner, m.gate_fn, m.rank4) == want + (True,) for m in nodes)
    if name == "mobilenet_v2_se":      # 1x1 convolutions: all 34 were plan layers
        assert planned == 34 and rep.relu == off.relu - 17 and rep.emit == off.emit - 17 and rep.fp32_outputs == off.fp32_outputs - 17


def test_flag_off_is_the_recorded_plan(nets):
    from plan_dump import plan_text
    net, kw = nets["efficientnet_b0"]
    with open(os.path.join(ROOT, "tests", "golden", "plans", "efficientnet_b0-dw5_True-gates_True-swish_True-dry.txt")) as f:
        assert plan_text(fuse_inference(net, dry_run=True, squeezes=False, **kw)) == f.read()
    assert plan_text(fuse_inference(net, dry_run=True, **kw)) == plan_text(fuse_inference(net, dry_run=True, squeezes=False, **kw))


# ------------------------------------------------------------------------------------------- candidates the pass leaves alone
class Toy(nn.Module):
    """conv -> squeeze-excite (Linear spelling, `c` -> `r` -> `c`) -> conv."""

    def __init__(self, c=32, r=8, gate="sigmoid", inner="swish"):
        super().__init__()
        self.c1, self.c2 = nn.Conv2d(16, c, 3, padding=1), nn.Conv2d(c, 16, 1)
        self.reduce, self.expand, self.gate, self.inner = nn.Linear(c, r), nn.Linear(r, c), gate, inner
        self.hs = nn.Hardsigmoid()

    def forward(self, x):
        x = F.relu(self.c1(x))
        v = self.reduce(x.mean((2, 3)).flatten(1) if self.inner == "flat" else x.mean((2, 3)))
        v = v * torch.sigmoid(v) if self.inner == "swish" else (F.relu(v) if self.inner == "relu" else v)
        v = self.expand(v).view(x.size(0), x.size(1), 1, 1)
        g = {"sigmoid": torch.sigmoid, "module": self.hs, "functional": F.hardsigmoid, "spelled": lambda t: F.relu6(t + 3) / 6,
             "tanh": torch.tanh}[self.gate](v)
        return self.c2(x * g)


QBASE = {"weight": {"enable": True, "type": "minmax_channel", "args": {"n_bits": 8, "signed": True}},
         "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}}, "exclude_layers": [], "override_options": []}


def _toy(method="FSPTQ", cfg=CFG, **kw):
    net = calibrated(Toy(**kw), cfg, None if method == "QBase" else method)
    if method == "QBase":
        from dlmc.quantization.scalar.modules.base import QBase
        for m in net.modules():
            if isinstance(m, QBase):
                m.in_init_state.fill_(1)
                m.wt_init_state.fill_(1)
                m.in_offset = torch.tensor([0.0])
    return net


@pytest.mark.parametrize("gate", ["sigmoid", "module", "functional", "spelled"])
@pytest.mark.parametrize("inner", ["swish", "relu", "none", "flat"])
def test_spellings_taken(gate, inner):
    gm = fuse_inference(_toy(gate=gate, inner=inner), dry_run=True, gates=True, squeezes=True)
    rep = gm.fusion_report
    (m,) = _squeeze_nodes(gm)
    assert rep.squeezes == 1 and rep.gates == 1 and rep.squeeze_left == [] and rep.skipped == []
    assert m.gate_fn == ("sigmoid" if gate == "sigmoid" else "hardsigmoid") and m.inner == (inner if inner in ("swish", "relu") else None)
    assert (m.c, m.r, m.r4, m.rank4) == (32, 8, 8, True)


def test_another_gate_function_is_no_candidate():
    rep = fuse_inference(_toy(gate="tanh"), dry_run=True, gates=True, squeezes=True).fusion_report
    assert rep.squeezes == 0 and rep.squeeze_left == [] and sorted(rep.skipped) == ["expand", "reduce"]


def _asymmetric():
    cfg = copy.deepcopy(QBASE)
    cfg["weight"]["args"]["signed"] = False          # unsigned weights: QBase's offset = the channel minimum
    return _toy("QBase", cfg)


def _float_offset():
    net = _toy("QBase", QBASE)
    net.reduce.in_offset.data.fill_(0.25)
    return net


def _adaround():
    net = _toy()
    net.expand.qconfig["weight"]["recon_type"] = "adaround"
    return net


def _four_bit():
    cfg = copy.deepcopy(CFG)
    cfg["weight"]["args"]["n_bits"] = 4
    return _toy(cfg=cfg)


LEFT = {
    "asymmetric": (_asymmetric, {}, "asymmetric weights|weights with an offset"),
    "float_offset": (_float_offset, {}, "float activation offset"),
    "too_wide": (lambda: _toy(c=2112, r=8), {}, "beyond the kernel's limits"),
    "too_many_hidden": (lambda: _toy(c=32, r=516), {}, "beyond the kernel's limits"),
    "adaround": (_adaround, {}, "AdaRound"),
    "pack_int4": (_four_bit, {}, "pack_int4"),
    "weight_blob": (_toy, dict(weight_blob={"layers": {}}), "weight_blob"),
}


@pytest.mark.parametrize("name", sorted(LEFT))
def test_refused_candidates_are_listed_with_their_reason(name):
    make, kw, why = LEFT[name]
    net = make()
    off = fuse_inference(net, dry_run=True, gates=True, **kw)
    gm = fuse_inference(net, dry_run=True, gates=True, squeezes=True, **kw)
    rep = gm.fusion_report
    assert rep.squeezes == 0 and not _squeeze_nodes(gm) and len(rep.squeeze_left) == 1
    node, reason = rep.squeeze_left[0]
    assert node == "mean" and re.search(why, reason), reason
    assert rep.skipped == off.fusion_report.skipped and rep.layers == off.fusion_report.layers and rep.gates == off.fusion_report.gates == 1
    assert [n.name for n in gm.graph.nodes] == [n.name for n in off.graph.nodes]      # the candidate stays as it is


def test_four_bit_weights_are_taken_without_packing():
    rep = fuse_inference(_four_bit(), dry_run=True, gates=True, squeezes=True, pack_int4=False).fusion_report
    assert rep.squeezes == 1 and rep.squeeze_left == []
