"""Attention on the f16 matrix cores, on the host: fuse_inference(attention="f16") plans the nodes of attention=True with the operand
choice on them and in the report; every other value is refused by name; the native prototype is dlmcq_attention_f32's."""
import pytest
import torch

import transformer_nets as T
from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import AttentionLayer, fuse_inference
from test_relu6_host import calibrated as fsptq

FLAGS = dict(dry_run=True, layer_norms=True, gelu=True)


def test_f16_plans_the_same_nodes_and_says_so():
    f32 = fuse_inference(fsptq(T.small_vit()), attention=True, **FLAGS)
    f16 = fuse_inference(fsptq(T.small_vit()), attention="f16", **FLAGS)
    assert f16.fusion_report.attentions == f32.fusion_report.attentions == 2
    assert (f16.fusion_report.attention_operands, f32.fusion_report.attention_operands) == ("f16", "f32")
    assert "attention operands=f16" in repr(f16.fusion_report) and "f16" not in repr(f32.fusion_report)
    for plan, want in ((f16, "f16"), (f32, "f32")):
        layers = [m for m in plan.modules() if isinstance(m, AttentionLayer)]
        assert len(layers) == 2 and all(m.operands == want for m in layers)
    assert str(f16.graph) == str(f32.graph)
    assert fuse_inference(fsptq(T.small_vit()), **FLAGS).fusion_report.attention_operands is None


@pytest.mark.parametrize("value", ["bf16", 1.5, "f32", 1])
def test_other_flag_values_are_refused(value):
    with pytest.raises(ValueError, match="attention is False, True .* or 'f16'"):
        fuse_inference(fsptq(T.small_vit()), attention=value, **FLAGS)


def test_other_operand_types_are_refused():
    t = torch.zeros(1, 1, 4, 32)
    with pytest.raises(ValueError, match=r"operands is one of \('f32', 'f16'\), not 'f64'"):
        K.attention_quant(t, t, t, 1.0, operands="f64")
    with pytest.raises(ValueError, match=r"operands is one of \('f32', 'f16'\)"):
        AttentionLayer(None, True, 0, None, False, operands="bf16")


def test_the_prototype_is_the_fp32_kernels():
    assert N.SIGNATURES["dlmcq_attention_f16"] == N.SIGNATURES["dlmcq_attention_f32"]
    fn = N.lib.dlmcq_attention_f16
    assert list(fn.argtypes) == list(N.lib.dlmcq_attention_f32.argtypes) and len(fn.argtypes) == 30
    assert fn(None, None, None, None, None, 0, 1, 1, 1, 64, *[64] * 12, 0.125, None, None, 0, 0, 0, 0.0, None) == 0      # empty: nothing launched
    assert fn(None, None, None, None, None, 1, 1, 1, 1, 48, *[64] * 12, 0.125, None, None, 0, 0, 0, 0.0, None) == -1     # D = 48
