"""LayerNorm and GELU nodes of the frozen int8 plan (fuse_inference(layer_norms=True, gelu=True)), on the host: the dry-run decisions for
the small ViT, the spellings that are taken and those left alone, the plan without the flags, and the argument checks of
dlmcq_layernorm_rows_f32 / dlmcq_gelu_nhwc_f32 that need no GPU (wrappers marked calibrated by hand, as in test_swish_host.py)."""
import ctypes
import os
import re

import pytest
import torch
from torch import nn

import transformer_nets as T
import workloads as W
from dlmc import _native as N
from dlmc.utils.fuse import GeluLayer, LayerNormLayer, fuse_inference
from plan_dump import plan_text
from test_relu6_host import calibrated as fsptq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = (N.FORM_ZEROPOINT, 0, 255, 1.0, 0.0, False)      # every wrapper's input quantiser as `fsptq` leaves it


def nodes(gm, prefix):
    return [n for n in gm.graph.nodes if n.op == "call_module" and str(n.target).startswith(prefix)]


def readers(nd):
    """{0: the readers of the node's fp32 output, 1: of its codes} as target-name prefixes."""
    gets = {u.args[1]: u for u in nd.users}
    return {i: sorted(str(u.target)[:10] for u in g.users) for i, g in gets.items() if g.users}


def both(make, **kw):
    return fuse_inference(fsptq(make()), dry_run=True), fuse_inference(fsptq(make()), dry_run=True, **kw)


ON = dict(layer_norms=True, gelu=True)


# ------------------------------------------------------------------------------------------- the small ViT
def test_small_vit_runs_and_every_linear_is_on_the_plan():
    net = T.small_vit().eval()
    assert tuple(net(torch.zeros(3, 3, 32, 32)).shape) == (3, 10)
    assert all(m.in_features % 64 == 0 for m in net.modules() if isinstance(m, nn.Linear))
    rep = fuse_inference(fsptq(T.small_vit()), dry_run=True).fusion_report
    assert (rep.layers, rep.residual, rep.skipped) == (10, 4, []) and (rep.layer_norms, rep.gelus) == (0, 0)


def test_vit_small_is_vit_s16():
    net = W.vit_small()
    lin = [m for m in net.modules() if isinstance(m, nn.Linear)]
    assert len(lin) == 1 + 4 * 12 + 1 and all(m.in_features % 64 == 0 for m in lin)
    assert tuple(net.pos_embedding.shape) == (1, 197, 384) and len(net.blocks) == 12
    assert (net.blocks[0].attn.heads, net.blocks[0].attn.dim_head, net.blocks[0].fc1.out_features) == (6, 64, 1536)
    # ViT-S/16 with a 1000-class head: 22 050 664 parameters, less the 12 q/k/v biases of 1152 that this spelling does not have
    assert sum(p.numel() for p in net.parameters()) == 22050664 - 12 * 1152
    assert "vit_small" not in W.MODELS and "vit_tiny" not in W.MODELS      # (the benchmark's table is as it was)
    assert tuple(W.vit_tiny().pos_embedding.shape) == (1, 197, 192)


def test_small_vit_decisions():
    off, on = both(T.small_vit, **ON)
    depth = 2
    ro, rn = off.fusion_report, on.fusion_report
    assert (rn.layer_norms, rn.gelus) == (2 * depth + 1, depth)
    assert "layer norms on the plan=5" in repr(rn) and "gelus on the plan=2" in repr(rn)
    assert "layer norms" not in repr(ro) and "gelus" not in repr(ro)
    mods = dict(on.named_modules())
    lns, gls = nodes(on, "_int8_layernorm_"), nodes(on, "_int8_gelu_")
    assert len(lns) == 5 and len(gls) == 2 and not any(isinstance(m, (LayerNormLayer, GeluLayer)) for m in off.modules())
    # every LayerNorm: codes to one Linear (to_qkv, fc1, the head), nobody reads the fp32 rows
    for nd in lns:
        m = mods[nd.target]
        assert isinstance(m, LayerNormLayer) and readers(nd) == {1: ["_int8_plan"]}
        assert (m.want_out, m.c, m.c_pad, m.emit_shift, m.emit.key) == (False, 64, 64, False, KEY)
        assert isinstance(m.norm, nn.LayerNorm) and m.norm.eps == 1e-5 and tuple(m.norm.normalized_shape) == (64,)
    # every GELU: codes to fc2 (128 in-features), rows, nobody reads the fp32 rows
    for nd in gls:
        m = mods[nd.target]
        assert isinstance(m, GeluLayer) and readers(nd) == {1: ["_int8_plan"]}
        assert (m.want_out, m.rows, m.c, m.c_pad, m.pad_code, m.emit_shift, m.emit.key) == (False, True, 128, 128, 0, False, KEY)
    # what is left of the two op kinds in the graph: nothing
    left = [n for n in on.graph.nodes if n.op == "call_module" and isinstance(mods.get(n.target), (nn.LayerNorm, nn.GELU))
            and not str(n.target).startswith("_int8_")]
    assert not left
    for f in ("layers", "dual", "residual", "relu", "relu6", "emit", "fp32_outputs", "narrow", "skipped", "stem"):
        assert getattr(rn, f) == getattr(ro, f), f      # whatever the main pass decided stays
    with pytest.raises(RuntimeError):
        mods[lns[0].target](torch.zeros(1, 64))         # a dry-run stand-in cannot be run


@pytest.mark.parametrize("flag, counts", [(dict(layer_norms=True), (5, 0)), (dict(gelu=True), (0, 2))])
def test_one_flag_alone(flag, counts):
    on = fuse_inference(fsptq(T.small_vit()), dry_run=True, **flag)
    assert (on.fusion_report.layer_norms, on.fusion_report.gelus) == counts
    assert (len(nodes(on, "_int8_layernorm_")), len(nodes(on, "_int8_gelu_"))) == counts


# ------------------------------------------------------------------------------------------- toys: taken
def test_a_second_fp32_reader_gets_the_fp32_rows():
    off, on = both(lambda: T.Rows(T.shared), **ON)
    mods = dict(on.named_modules())
    (ln,), (gl,) = nodes(on, "_int8_layernorm_"), nodes(on, "_int8_gelu_")
    assert mods[ln.target].want_out and mods[gl.target].want_out
    assert readers(ln)[1] == ["_int8_plan"] and readers(gl)[1] == ["_int8_plan"] and readers(ln)[0] and readers(gl)[0]


def test_functional_spellings_are_traced_into():
    off, on = both(lambda: T.Rows(T.functional_spellings), **ON)
    assert on.fusion_report.gelus == 2 and on.fusion_report.layer_norms == 1
    assert all(dict(on.named_modules())[n.target].rows for n in nodes(on, "_int8_gelu_"))


def test_a_convolution_reader_gets_channel_padded_rows():
    off, on = both(T.conv_reader, **ON)
    (gl,) = nodes(on, "_int8_gelu_")
    m = dict(on.named_modules())[gl.target]
    assert (m.rows, m.c, m.c_pad, m.want_out, m.pad_code) == (False, 24, 64, False, 0) and readers(gl) == {1: ["_int8_plan"]}


# ------------------------------------------------------------------------------------------- toys: left alone
def _two_quantisers():
    net = fsptq(T.Rows(T.two_quantisers))
    net.fc3.in_scale.data.fill_(2.0)
    return net


LEFT_ALONE = {
    "tanh_gelu": lambda: fsptq(T.Rows(T.tanh_gelu)),
    "tanh_gelu_module": lambda: fsptq(T.Rows(T.tanh_gelu_module)),
    "functional_layer_norm": lambda: fsptq(T.Rows(T.functional_layer_norm)),
    "layer_norm_over_two_dimensions": lambda: fsptq(T.Rows(lambda self, x: self.fc1(self.norm(x)), norm=nn.LayerNorm((16, 64)))),
    "c_2052": lambda: fsptq(T.Rows(lambda self, x: self.fc1(self.norm(x)), width=2052)),
    "c_2112_a_plan_linear_behind_it": lambda: fsptq(T.Rows(lambda self, x: self.fc1(self.norm(x)), width=2112)),
    "c_66": lambda: fsptq(T.Rows(lambda self, x: self.fc1(self.norm(x)), width=66)),
    "nobody_takes_codes": lambda: fsptq(T.Rows(T.nobody_takes_codes)),
    "two_quantisers": _two_quantisers,
}


@pytest.mark.parametrize("name", sorted(LEFT_ALONE))
def test_left_alone(name):
    off = fuse_inference(LEFT_ALONE[name](), dry_run=True)
    on = fuse_inference(LEFT_ALONE[name](), dry_run=True, **ON)
    rn = on.fusion_report
    assert (rn.layer_norms, rn.gelus) == (0, 0) and str(on.graph) == str(off.graph) and repr(rn) == repr(off.fusion_report)


def test_c_2112_is_left_alone_by_the_width_rule():
    """(2112 = 33 * 64: the Linear behind the LayerNorm IS on the plan; at 2048 the same network is taken.)"""
    rep = fuse_inference(LEFT_ALONE["c_2112_a_plan_linear_behind_it"](), dry_run=True, **ON).fusion_report
    assert rep.layers == 1 and rep.layer_norms == 0
    rep = fuse_inference(fsptq(T.Rows(lambda self, x: self.fc1(self.norm(x)), width=2048)), dry_run=True, **ON).fusion_report
    assert rep.layers == 1 and rep.layer_norms == 1


# ------------------------------------------------------------------------------------------- the flags off
@pytest.mark.parametrize("make", [T.small_vit, W.mobilenet_v2, W.resnet50, lambda: W.mobilenet_v2(se=True, act="swish")],
                         ids=["small_vit", "mobilenet_v2", "resnet50", "mbconv"])
def test_flags_off_is_the_plan_as_it_was(make):
    plain = fuse_inference(fsptq(make()), dry_run=True)
    explicit = fuse_inference(fsptq(make()), dry_run=True, layer_norms=False, gelu=False)
    assert plan_text(plain) == plan_text(explicit)
    assert not nodes(plain, "_int8_layernorm_") and not nodes(plain, "_int8_gelu_")
    assert "layer norms" not in plan_text(plain) and "gelus" not in plan_text(plain)


@pytest.mark.parametrize("make", [W.mobilenet_v2, W.resnet50], ids=["mobilenet_v2", "resnet50"])
def test_flags_on_change_nothing_where_there_is_nothing_to_take(make):
    off, on = both(make, **ON)
    assert plan_text(off) == plan_text(on)


# ------------------------------------------------------------------------------------------- header, exports, ctypes table
@pytest.mark.parametrize("name, count", [("dlmcq_gelu_nhwc_f32", 17), ("dlmcq_layernorm_rows_f32", 15)])
def test_header_exports_and_ctypes_table_agree(name, count):
    with open(os.path.join(ROOT, "include", "dlmcq.h")) as f:
        header = f.read()
    (decl,) = re.findall(r"\nint " + name + r"\(([^;]*)\);", header)
    params = [p.strip() for p in decl.replace("\n", " ").split(",")]
    kinds = [ctypes.c_void_p if "*" in p or p.startswith("dlmcq_stream_t") else {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32,
             "float": ctypes.c_float}[p.split()[0]] for p in params]
    res, args = N.SIGNATURES[name]
    assert res is ctypes.c_int and list(args) == kinds and len(args) == count
    fn = getattr(N.lib, name)
    assert fn.restype is ctypes.c_int and list(fn.argtypes) == kinds
    if name == "dlmcq_gelu_nhwc_f32":
        assert list(args) == list(N.SIGNATURES["dlmcq_swish_nhwc_f32"][1])


# ------------------------------------------------------------------------------------------- the entry points, without a GPU
def _p(v):
    return None if v is None else ctypes.c_void_p(v)


def _gelu(x=1 << 12, out=1 << 13, codes=1 << 14, n=2, h=8, w=8, c=16, xs=16, c_pad=16, pad_code=0, scale=1 << 15, zp=None, lo=0, hi=255,
          form=None, g=0.0):
    form = N.FORM_ZEROPOINT if form is None else form
    return N.lib.dlmcq_gelu_nhwc_f32(_p(x), _p(out), _p(codes), n, h, w, c, xs, c_pad, pad_code, _p(scale), _p(zp), lo, hi, form, g, None)


def _ln(x=1 << 12, gamma=1 << 16, beta=1 << 17, out=1 << 13, codes=1 << 14, m=5, c=64, eps=1e-5, scale=1 << 15, zp=None, lo=0, hi=255,
        form=None, g=0.0):
    form = N.FORM_ZEROPOINT if form is None else form
    return N.lib.dlmcq_layernorm_rows_f32(_p(x), _p(gamma), _p(beta), _p(out), _p(codes), m, c, eps, _p(scale), _p(zp), lo, hi, form, g, None)


EINVAL, ERANGE, EALIGN = -1, -2, -4
CONTROL_BITS = {"force_tiled": N.FORCE_TILED, "route_only": N.ROUTE_ONLY, "pipelined": N.PIPELINED, "chunk_major_in": N.FP32_IN_CHUNK_MAJOR,
                "chunk_major_out": N.FP32_OUT_CHUNK_MAJOR}
GELU_REFUSED = {
    "h_0": (dict(h=0), EINVAL), "w_0": (dict(w=0), EINVAL), "c_below_4": (dict(c=0), EINVAL), "c_mod_4": (dict(c=6), EINVAL),
    "stride_below_c": (dict(xs=12), EINVAL), "stride_mod_4": (dict(xs=18), EINVAL), "c_pad_below_c": (dict(c_pad=12), EINVAL),
    "c_pad_mod_4": (dict(c_pad=18), EINVAL), "no_output": (dict(out=None, codes=None), EINVAL),
    "c_pad_without_codes": (dict(codes=None, c_pad=64), EINVAL), "negative_n": (dict(n=-1), EINVAL), "pad_code_300": (dict(pad_code=300), EINVAL),
    "pad_code_minus_129": (dict(pad_code=-129), EINVAL), "null_x": (dict(x=None), EINVAL), "codes_without_scale": (dict(scale=None), EINVAL),
    "lo_above_hi": (dict(lo=5, hi=4), EINVAL), "unknown_form": (dict(form=9), EINVAL),
    "shifted_signed_range": (dict(form=N.FORM_ZEROPOINT | N.EMIT_SHIFT128, lo=-128, hi=127), EINVAL),
    "x_misaligned": (dict(x=(1 << 12) + 4), EALIGN), "out_misaligned": (dict(out=(1 << 13) + 8), EALIGN),
    "codes_misaligned": (dict(codes=(1 << 14) + 2), EALIGN),
    "rows_reach_2_31": (dict(n=1 << 31, h=1, w=1, c=4, xs=4, c_pad=4), ERANGE), "pixels_reach_2_31": (dict(n=1, h=1 << 16, w=1 << 15), ERANGE),
    "padded_threads_reach_2_31": (dict(n=1 << 10, h=1 << 10, w=1 << 6, c=4, xs=4, c_pad=128), ERANGE),
    **{k: (dict(form=N.FORM_ZEROPOINT | v), EINVAL) for k, v in CONTROL_BITS.items()},
}
LN_REFUSED = {
    "negative_m": (dict(m=-1), EINVAL), "c_below_4": (dict(c=0), EINVAL), "c_mod_4": (dict(c=66), EINVAL), "c_2052": (dict(c=2052), EINVAL),
    "eps_0": (dict(eps=0.0), EINVAL), "eps_negative": (dict(eps=-1e-5), EINVAL), "eps_inf": (dict(eps=float("inf")), EINVAL),
    "eps_nan": (dict(eps=float("nan")), EINVAL), "no_output": (dict(out=None, codes=None), EINVAL), "null_x": (dict(x=None), EINVAL),
    "codes_without_scale": (dict(scale=None), EINVAL), "lo_above_hi": (dict(lo=5, hi=4), EINVAL), "unknown_form": (dict(form=9), EINVAL),
    "range_wider_than_a_byte": (dict(lo=-128, hi=255), EINVAL),
    "shifted_emission": (dict(form=N.FORM_ZEROPOINT | N.EMIT_SHIFT128), EINVAL),
    "x_misaligned": (dict(x=(1 << 12) + 4), EALIGN), "gamma_misaligned": (dict(gamma=(1 << 16) + 4), EALIGN),
    "beta_misaligned": (dict(beta=(1 << 17) + 8), EALIGN), "out_misaligned": (dict(out=(1 << 13) + 8), EALIGN),
    "codes_misaligned": (dict(codes=(1 << 14) + 2), EALIGN),
    "rows_reach_2_31": (dict(m=1 << 31, c=4), ERANGE), "quads_reach_2_31": (dict(m=1 << 22, c=2048), ERANGE),
    # two faults: the earlier check of map_codes_call's order answers
    "geometry_before_quantiser": (dict(c=6, scale=None), EINVAL), "quantiser_before_alignment": (dict(lo=5, hi=4, x=(1 << 12) + 4), EINVAL),
    "null_before_alignment": (dict(x=None, out=(1 << 13) + 8), EINVAL), "alignment_before_range": (dict(m=1 << 31, c=4, out=(1 << 13) + 8), EALIGN),
    **{k: (dict(form=N.FORM_ZEROPOINT | v), EINVAL) for k, v in CONTROL_BITS.items()},
}


@pytest.mark.parametrize("name", sorted(GELU_REFUSED))
def test_gelu_refusals_need_no_gpu(name):
    """Nothing is launched on these placeholder pointers: every call is answered by the argument checks."""
    kw, rc = GELU_REFUSED[name]
    assert N.lib.dlmcq_strerror(rc) and _gelu(**kw) == rc


@pytest.mark.parametrize("name", sorted(LN_REFUSED))
def test_layernorm_refusals_need_no_gpu(name):
    kw, rc = LN_REFUSED[name]
    assert N.lib.dlmcq_strerror(rc) and _ln(**kw) == rc


def test_empty_problems_are_ok():
    assert _gelu(n=0) == 0 and _gelu(n=0, x=None, out=None, codes=None) == 0
    assert _ln(m=0) == 0 and _ln(m=0, x=None, gamma=None, beta=None, out=None, codes=None) == 0
    assert _ln(m=0, c=2048) == 0 and _ln(m=0, c=4) == 0
