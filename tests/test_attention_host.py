"""Attention nodes of the frozen int8 plan (fuse_inference(attention=True)), on the host: the dry-run decisions for the small ViT, the
spellings that are taken and those left alone, the plan without the flag, the torch restatement on CPU tensors, and the argument
checks of dlmcq_attention_f32, none of which needs a GPU (wrappers marked calibrated by hand, as in test_swish_host.py)."""
import ctypes
import os
import re

import pytest
import torch

import attention_nets as A
import transformer_nets as T
import workloads as W
from dlmc import _native as N
from dlmc.utils.fuse import AttentionLayer, fuse_inference
from plan_dump import plan_text
from test_relu6_host import calibrated as fsptq
from test_transformer_host import CONTROL_BITS, EALIGN, EINVAL, ERANGE, KEY, nodes, readers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dict(layer_norms=True, gelu=True, attention=True)


# ------------------------------------------------------------------------------------------- the small ViT
def test_small_vit_decisions():
    depth = 2
    off = fuse_inference(fsptq(T.small_vit()), dry_run=True, layer_norms=True, gelu=True)
    on = fuse_inference(fsptq(T.small_vit()), dry_run=True, **ALL)
    ro, rn = off.fusion_report, on.fusion_report
    assert rn.attentions == depth and ro.attentions == 0
    assert "attentions on the plan=2" in repr(rn) and "attentions" not in repr(ro)
    assert (rn.layer_norms, rn.gelus) == (ro.layer_norms, ro.gelus) == (2 * depth + 1, depth)
    mods = dict(on.named_modules())
    ats = nodes(on, "_int8_attention_")
    assert len(ats) == depth and not any(isinstance(m, AttentionLayer) for m in off.modules())
    for nd in ats:
        m = mods[nd.target]
        assert isinstance(m, AttentionLayer) and readers(nd) == {1: ["_int8_plan"]}      # to_out reads output 1, nobody output 0
        assert (m.want_out, m.merged, m.flatten, m.sdpa, m.c, m.emit.key) == (False, True, False, None, 64, KEY)
        assert m.scale == 32 ** -0.5 and len(nd.args) == 6 and nd.args[5] == 64
    left = [n for n in on.graph.nodes if n.op == "call_function" and n.target in (torch.matmul, torch.softmax)]
    assert not left
    for f in ("layers", "dual", "residual", "relu", "relu6", "emit", "fp32_outputs", "narrow", "skipped", "stem"):
        assert getattr(rn, f) == getattr(ro, f), f
    with pytest.raises(RuntimeError):
        mods[ats[0].target](*[torch.zeros(1, 2, 3, 32)] * 3, 1, 3, 64)


def test_the_flag_alone():
    on = fuse_inference(fsptq(T.small_vit()), dry_run=True, attention=True)
    rn = on.fusion_report
    assert (rn.attentions, rn.layer_norms, rn.gelus) == (2, 0, 0) and len(nodes(on, "_int8_attention_")) == 2


# ------------------------------------------------------------------------------------------- toys
@pytest.mark.parametrize("name", sorted(A.TAKEN))
def test_taken(name):
    on = fuse_inference(fsptq(A.TAKEN[name]()), dry_run=True, attention=True)
    (nd,) = nodes(on, "_int8_attention_")
    m = dict(on.named_modules())[nd.target]
    assert on.fusion_report.attentions == 1 and readers(nd) == {1: ["_int8_plan"]}
    assert (m.merged, m.want_out, m.c, m.emit.key) == (True, False, 64, KEY)
    assert m.flatten == (name == "functional_softmax_flatten")
    assert m.sdpa == {"sdpa": {}, "sdpa_scale": {"scale": 0.25}}.get(name)
    assert m.scale == {"sdpa": None, "sdpa_scale": 0.25}.get(name, 32 ** -0.5)
    assert not [n for n in on.graph.nodes if n.op == "call_function" and n.target in (torch.matmul, torch.softmax)]


@pytest.mark.parametrize("name", sorted(A.LEFT_ALONE))
def test_left_alone(name):
    off = fuse_inference(fsptq(A.LEFT_ALONE[name]()), dry_run=True)
    on = fuse_inference(fsptq(A.LEFT_ALONE[name]()), dry_run=True, attention=True)
    assert on.fusion_report.attentions == 0 and str(on.graph) == str(off.graph) and repr(on.fusion_report) == repr(off.fusion_report)


def test_a_tail_that_does_not_merge_heads_is_left_alone():
    """The core runs as an fp32-only node where the second product stood ([B, H, Tq, D]); what reads it, and to_out's own quantise
    pass, stay as they were."""
    off = fuse_inference(fsptq(A.Attn(A.vit_spelling, A.no_merge)), dry_run=True)
    on = fuse_inference(fsptq(A.Attn(A.vit_spelling, A.no_merge)), dry_run=True, attention=True)
    (nd,) = nodes(on, "_int8_attention_")
    m = dict(on.named_modules())[nd.target]
    assert (m.merged, m.emit, m.want_out) == (False, None, True) and len(nd.args) == 3
    assert set(readers(nd)) == {0} and all(not r.startswith("_int8_plan") for r in readers(nd)[0])
    for f in ("layers", "emit", "fp32_outputs", "skipped"):
        assert getattr(on.fusion_report, f) == getattr(off.fusion_report, f)


# ------------------------------------------------------------------------------------------- the flag off
@pytest.mark.parametrize("make", [T.small_vit, W.resnet50, W.mobilenet_v2], ids=["small_vit", "resnet50", "mobilenet_v2"])
def test_flag_off_is_the_plan_as_it_was(make):
    plain = fuse_inference(fsptq(make()), dry_run=True)
    explicit = fuse_inference(fsptq(make()), dry_run=True, attention=False)
    assert plan_text(plain) == plan_text(explicit)
    assert not nodes(plain, "_int8_attention_") and "attentions" not in plan_text(plain)


@pytest.mark.parametrize("make", [W.resnet50, W.mobilenet_v2], ids=["resnet50", "mobilenet_v2"])
def test_flag_on_changes_nothing_where_there_is_nothing_to_take(make):
    assert plan_text(fuse_inference(fsptq(make()), dry_run=True)) == plan_text(fuse_inference(fsptq(make()), dry_run=True, attention=True))


# ------------------------------------------------------------------------------------------- the restatement, on CPU tensors
@pytest.mark.parametrize("name", sorted(A.TAKEN) + ["no_merge", "small_vit"])
def test_cpu_tensors_take_the_restatement(name):
    """No quantised layer here, so the plan is torch ops plus the AttentionLayer, whose input on the CPU takes its torch restatement:
    the logits of the plan without the node, bit for bit."""
    torch.manual_seed(5)
    net = (T.small_vit() if name == "small_vit" else A.Attn(A.vit_spelling, A.no_merge) if name == "no_merge" else A.TAKEN[name]()).eval()
    x = torch.randn(3, 3, 32, 32) if name == "small_vit" else torch.randn(3, 16, 64)
    off, on = fuse_inference(net), fuse_inference(net, attention=True)
    assert on.fusion_report.attentions == (2 if name == "small_vit" else 1) and off.fusion_report.attentions == 0
    layers = [m for m in on.modules() if isinstance(m, AttentionLayer)]
    assert layers and all(m.emit is None and m.want_out for m in layers)
    with torch.no_grad():
        a, b, c = net(x), off(x), on(x)
    assert torch.equal(a, b) and torch.equal(b, c)


def test_a_reshape_that_is_no_merge_takes_the_restatement():
    """reshape(b, t * heads, d): rank 3 at trace time, no merge of the heads at run time."""
    def tail(self, o, b, t):
        return self.to_out(o.permute(0, 2, 1, 3).reshape(b, t // 2, 2 * self.heads * self.dim_head)[..., :64])
    net = A.Attn(A.vit_spelling, tail).eval()
    x = torch.randn(2, 16, 64)
    on = fuse_inference(net, attention=True)
    assert on.fusion_report.attentions == 1
    with torch.no_grad():
        assert torch.equal(on(x), net(x))


# ------------------------------------------------------------------------------------------- header, exports, ctypes table
def test_header_exports_and_ctypes_table_agree():
    name = "dlmcq_attention_f32"
    with open(os.path.join(ROOT, "include", "dlmcq.h")) as f:
        header = f.read()
    (decl,) = re.findall(r"\nint " + name + r"\(([^;]*)\);", header)
    params = [p.strip() for p in decl.replace("\n", " ").split(",")]
    kinds = [ctypes.c_void_p if "*" in p or p.startswith("dlmcq_stream_t") else {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
             "float": ctypes.c_float}[p.split()[0]] for p in params]
    res, args = N.SIGNATURES[name]
    assert res is ctypes.c_int and list(args) == kinds and len(args) == 30
    fn = getattr(N.lib, name)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == kinds
    assert list(args[-7:]) == list(N.SIGNATURES["dlmcq_layernorm_rows_f32"][1][-7:])      # the quantiser arguments and the stream
    with open(os.path.join(ROOT, "dlmc-quant_amd", "csrc", "Makefile")) as f:
        assert " attention.hip " in f.read()


# ------------------------------------------------------------------------------------------- the entry point, without a GPU
def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _at(q=1 << 12, k=1 << 13, v=1 << 14, out=1 << 15, codes=1 << 16, b=2, h=3, tq=17, tk=17, d=64, qs=None, ks=None, vs=None, os_=None,
        att_scale=0.125, scale=1 << 17, zp=None, lo=0, hi=255, form=None, g=0.0):
    form = N.FORM_ZEROPOINT if form is None else form
    packed = (tq * 3 * h * d, d, 3 * h * d)
    qs, ks, vs = (packed if s is None else s for s in (qs, ks, vs))
    os_ = (tq * h * d, d, h * d) if os_ is None else os_
    return N.lib.dlmcq_attention_f32(_p(q), _p(k), _p(v), _p(out), _p(codes), b, h, tq, tk, d, *qs, *ks, *vs, *os_, att_scale, _p(scale), _p(zp),
                                     lo, hi, form, g, None)


REFUSED = {
    "negative_b": (dict(b=-1), EINVAL), "negative_h": (dict(h=-1), EINVAL), "negative_tq": (dict(tq=-1), EINVAL), "tk_0": (dict(tk=0), EINVAL),
    "d_48": (dict(d=48), EINVAL), "d_128": (dict(d=128), EINVAL), "d_0": (dict(d=0), EINVAL),
    "scale_nan": (dict(att_scale=float("nan")), EINVAL), "scale_inf": (dict(att_scale=float("inf")), EINVAL),
    "q_stride_mod_4": (dict(qs=(3264, 64, 194)), EINVAL), "k_stride_negative": (dict(ks=(-3264, 64, 192)), EINVAL),
    "v_token_stride_below_d": (dict(vs=(3264, 64, 32)), EINVAL), "out_head_stride_mod_4": (dict(os_=(6528, 66, 384)), EINVAL),
    "no_output": (dict(out=None, codes=None), EINVAL), "null_q": (dict(q=None), EINVAL), "null_k": (dict(k=None), EINVAL),
    "null_v": (dict(v=None), EINVAL), "codes_without_scale": (dict(scale=None), EINVAL), "lo_above_hi": (dict(lo=5, hi=4), EINVAL),
    "unknown_form": (dict(form=9), EINVAL), "range_wider_than_a_byte": (dict(lo=-128, hi=255), EINVAL),
    "shifted_emission": (dict(form=N.FORM_ZEROPOINT | N.EMIT_SHIFT128), EINVAL),
    "q_misaligned": (dict(q=(1 << 12) + 4), EALIGN), "k_misaligned": (dict(k=(1 << 13) + 8), EALIGN), "v_misaligned": (dict(v=(1 << 14) + 4), EALIGN),
    "out_misaligned": (dict(out=(1 << 15) + 8), EALIGN), "codes_misaligned": (dict(codes=(1 << 16) + 2), EALIGN),
    "b_reaches_2_31": (dict(b=1 << 31, h=1), ERANGE), "heads_reach_2_31": (dict(b=1 << 16, h=1 << 15), ERANGE),
    "tq_reaches_2_31": (dict(b=1, h=1, tq=1 << 31), ERANGE), "tk_reaches_2_31": (dict(tk=1 << 31), ERANGE),
    "workgroups_reach_2_31": (dict(b=1 << 15, h=1 << 10, tq=1 << 13), ERANGE),
    # two faults: the earlier check of map_codes_call's order answers
    "geometry_before_quantiser": (dict(d=48, scale=None), EINVAL), "quantiser_before_alignment": (dict(lo=5, hi=4, q=(1 << 12) + 4), EINVAL),
    "null_before_alignment": (dict(q=None, out=(1 << 15) + 8), EINVAL), "alignment_before_range": (dict(tk=1 << 31, out=(1 << 15) + 8), EALIGN),
    **{k_: (dict(form=N.FORM_ZEROPOINT | v_), EINVAL) for k_, v_ in CONTROL_BITS.items()},
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refusals_need_no_gpu(name):
    """Nothing is launched on these placeholder pointers: every call is answered by the argument checks."""
    kw, rc = REFUSED[name]
    assert N.lib.dlmcq_strerror(rc) and _at(**kw) == rc


def test_empty_problems_are_ok():
    dense = (64, 64, 64)
    assert _at(b=0) == 0 and _at(h=0, qs=dense, ks=dense, vs=dense, os_=dense) == 0 and _at(tq=0) == 0
    assert _at(b=0, q=None, k=None, v=None, out=None, codes=None) == 0 and _at(tq=0, d=32, out=None, codes=None, scale=None) == 0
