"""Window attention on the f16 matrix cores, on the host: fuse_inference(window_attention="f16") plans the nodes of window_attention=True
with the operand choice on them and in the report; every other value is refused by name; the native prototype and the argument checks
are dlmcq_window_attention_f32's."""
import ctypes

import pytest
import torch

import workloads as W
from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import WindowAttentionLayer, fuse_inference
from test_relu6_host import calibrated as fsptq

FLAGS = dict(dry_run=True, layer_norms=True, gelu=True)


def test_f16_plans_the_same_nodes_and_says_so():
    f32 = fuse_inference(fsptq(W.window_vit()), window_attention=True, **FLAGS)
    f16 = fuse_inference(fsptq(W.window_vit()), window_attention="f16", **FLAGS)
    assert f16.fusion_report.window_attentions == f32.fusion_report.window_attentions == 4
    assert (f16.fusion_report.window_attention_operands, f32.fusion_report.window_attention_operands) == ("f16", "f32")
    assert "window attention operands=f16" in repr(f16.fusion_report) and "f16" not in repr(f32.fusion_report)
    for plan, want in ((f16, "f16"), (f32, "f32")):
        layers = [m for m in plan.modules() if isinstance(m, WindowAttentionLayer)]
        assert len(layers) == 4 and all(m.operands == want for m in layers)
    assert str(f16.graph) == str(f32.graph) and len(f16.graph.nodes) == len(f32.graph.nodes)
    assert fuse_inference(fsptq(W.window_vit()), **FLAGS).fusion_report.window_attention_operands is None


@pytest.mark.parametrize("value", ["f32", "bf16", 1, 1.5])
def test_other_flag_values_are_refused(value):
    with pytest.raises(ValueError, match="window_attention is False, True .* or 'f16'"):
        fuse_inference(fsptq(W.window_vit()), window_attention=value, **FLAGS)


def test_other_operand_types_are_refused():
    t = torch.zeros(1, 1, 4, 32)
    with pytest.raises(ValueError, match=r"operands is one of \('f32', 'f16'\), not 'f64'"):
        K.window_attention_quant(t, t, t, 1.0, operands="f64")
    with pytest.raises(ValueError, match=r"operands is one of \('f32', 'f16'\)"):
        WindowAttentionLayer(None, True, 0, 1.0, False, False, True, False, operands="bf16")


@pytest.mark.parametrize("entry", ["dlmcq_window_attention_f32", "dlmcq_window_attention_f16"])
def test_the_prototype_and_the_checks_are_the_fp32_kernels(entry):
    assert N.SIGNATURES[entry] == N.SIGNATURES["dlmcq_window_attention_f32"] and len(N.SIGNATURES[entry][1]) == 36
    p = [ctypes.c_void_p(1 << n) for n in range(12, 19)]      # q, k, v, bias, mask, out, codes: placeholders, nothing is launched

    def call(b=4, t=49, d=32, bias_st=52):
        packed = (t * 288, d, 288)
        return getattr(N.lib, entry)(*p, b, 3, t, d, 2, *packed, *packed, *packed, t * 96, d, 96, t * bias_st, bias_st, t * 52, 52, 0.125,
                                     ctypes.c_void_p(1 << 20), None, 0, 255, N.FORM_ZEROPOINT, 0.0, None)
    assert call(b=0) == 0      # empty: nothing launched
    assert call(d=48) == call(t=65) == call(bias_st=50) == -1
