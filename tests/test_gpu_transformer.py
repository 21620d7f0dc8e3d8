"""A transformer on the frozen int8 plan, on the GPU (fuse_inference(layer_norms=True, gelu=True)): the smallest ViT that has every
pattern (transformer_nets.small_vit: 17 tokens - an odd row count -, dim 64, 2 heads of 32, MLP 128, depth 2, batch 3), FSPTQ and QBase
W8A8, calibrated.
(a) the report counts 2 * depth + 1 LayerNorms and depth GELUs, and every taker Linear receives a code tensor;
(b) the logits are torch.equal to those of the flag-off plan of a copy whose nn.LayerNorm / nn.GELU modules are replaced by modules that
    return K.layernorm_quant(...)[0] / K.gelu_quant(...)[0]: the consumer's quantise pass of that fp32 tensor is what the node emits;
(c) the largest logit difference against the unmodified flag-off plan is printed, not gated (DESIGN.md 5.23 records it);
(d) a plan with one of the two flags runs and counts that flag's nodes alone."""
import copy
import functools

import pytest
import torch
from torch import nn

from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import GeluLayer, Int8Layer, LayerNormLayer, fuse_inference
from test_gpu_gate import DEV, tagged
from test_gpu_narrow_rows import FSPTQ_W8A8, QBASE_W8A8
from transformer_nets import small_vit

pytestmark = pytest.mark.gpu
DEPTH = 2
CASES = {"fsptq": (FSPTQ_W8A8, "FSPTQ"), "qbase": (QBASE_W8A8, None)}


@torch.fx.wrap
def _layernorm_fp32(x, weight, bias, eps):
    return K.layernorm_quant(x, weight, bias, eps)[0]


@torch.fx.wrap
def _gelu_fp32(x):
    return K.gelu_quant(x)[0]


class KernelLayerNorm(nn.Module):
    """The LayerNorm kernel's fp32 output in place of an nn.LayerNorm (a leaf call for the plan's tracer)."""

    def __init__(self, norm):
        super().__init__()
        self.weight, self.bias, self.eps = norm.weight, norm.bias, norm.eps

    def forward(self, x):
        return _layernorm_fp32(x, self.weight, self.bias, self.eps)


class KernelGelu(nn.Module):
    def forward(self, x):
        return _gelu_fp32(x)


def substituted(net):
    net = copy.deepcopy(net)
    for m in list(net.modules()):
        for name, child in list(m.named_children()):
            if type(child) is nn.LayerNorm:
                setattr(m, name, KernelLayerNorm(child))
            elif type(child) is nn.GELU:
                setattr(m, name, KernelGelu())
    return net


@functools.lru_cache(maxsize=None)
def calibrated(tag):
    """(the quantised, calibrated network, its input): made once per configuration, shared, never written.  FSPTQ keeps its calibrated
    zero points, rounded to integers (non-zero behind a LayerNorm, whose output is signed); QBase's float offsets are set to 0."""
    from dlmc.quantization.scalar.FSPTQuant import FSPTQBase
    from dlmc.quantization.scalar.modules.base import QBase
    from dlmc.utils.quantize import quantize_model
    cfg, qtype = CASES[tag]
    torch.manual_seed(11)
    net = small_vit().to(DEV).eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.LayerNorm):      # (not the identity: every gamma and beta takes part)
                m.weight.normal_(1.0, 0.2)
                m.bias.normal_(0.0, 0.2)
    if qtype:
        quantize_model(net, copy.deepcopy(cfg), None, qtype, int8_gemm=True)
    else:
        quantize_model(net, copy.deepcopy(cfg), None)
    x = torch.randn(3, 3, 32, 32, device=DEV)
    with torch.no_grad():
        net(x)                                   # calibrate
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, FSPTQBase):
                m.in_offset.round_().clamp_(m.in_min_val, m.in_max_val)
                m._zp_is_int = None
            elif isinstance(m, QBase) and m.in_offset is not None:
                m.in_offset.zero_()
    return net, x


def takers(gm):
    """{plan node name: its module} of the plan layers that read output 1 of a LayerNorm or GELU node."""
    mods = dict(gm.named_modules())
    out = {}
    for n in gm.graph.nodes:
        if n.op == "call_module" and isinstance(mods.get(n.target), (LayerNormLayer, GeluLayer)):
            for g in n.users:
                if g.args[1] == 1:
                    out.update({u.target: mods[u.target] for u in g.users})
    return out


@pytest.mark.parametrize("tag", sorted(CASES))
def test_both_flags(tag):
    net, x = calibrated(tag)
    off = fuse_inference(net)
    on = fuse_inference(net, layer_norms=True, gelu=True)
    ro, rn = off.fusion_report, on.fusion_report
    print(ro, rn, sep="\n")
    # (a)
    assert (ro.layer_norms, ro.gelus) == (0, 0) and (rn.layer_norms, rn.gelus) == (2 * DEPTH + 1, DEPTH)
    assert rn.layers == ro.layers == 4 * DEPTH + 2 and rn.skipped == ro.skipped == []
    assert (rn.residual, rn.emit, rn.fp32_outputs) == (ro.residual, ro.emit, ro.fp32_outputs)
    assert sum(isinstance(m, LayerNormLayer) for m in on.modules()) == 2 * DEPTH + 1 and sum(isinstance(m, GeluLayer) for m in on.modules()) == DEPTH
    assert not any(isinstance(m, (nn.LayerNorm, nn.GELU)) for n_, m in on.named_modules() if any(
        nd.op == "call_module" and nd.target == n_ for nd in on.graph.nodes))
    readers = takers(on)
    assert len(readers) == 3 * DEPTH + 1 and all(isinstance(m, Int8Layer) and m.layer.weight.dim() == 2 for m in readers.values())
    seen = {}
    hooks = [m.register_forward_hook(lambda mod, a, r, n_=n_: seen.__setitem__(n_, a[0].dtype)) for n_, m in readers.items()]
    with torch.no_grad():
        (a, tags_off), (b, tags_on) = tagged(lambda: off(x)), tagged(lambda: on(x))
        for h in hooks:
            h.remove()
        again = on(x)
    assert sorted(seen) == sorted(readers) and all(d in (torch.uint8, torch.int8) for d in seen.values()), seen
    assert tags_on.count("layernorm") == 2 * DEPTH + 1 and tags_on.count("gelu") == DEPTH
    assert "layernorm" not in tags_off and "gelu" not in tags_off
    # the consumers' own quantise passes are gone: one per taker
    assert tags_off.count("fq_tensor") - tags_on.count("fq_tensor") == 3 * DEPTH + 1
    assert tuple(b.shape) == (3, 10) and bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()) and torch.equal(b, again)
    # (b)
    sub = fuse_inference(substituted(net))
    assert sub.fusion_report.layers == ro.layers and (sub.fusion_report.layer_norms, sub.fusion_report.gelus) == (0, 0)
    with torch.no_grad():
        c, tags_sub = tagged(lambda: sub(x))
    assert tags_sub.count("layernorm") == 2 * DEPTH + 1 and tags_sub.count("gelu") == DEPTH
    assert torch.equal(b, c), f"{int((b != c).sum())} of {b.numel()} logits differ from the substituted network, max {float((b - c).abs().max())}"
    # (c)
    dev = float((a - b).abs().max())
    top1 = int((a.argmax(1) == b.argmax(1)).sum())
    print(f"{tag}: max |logit(flags on) - logit(flags off)| = {dev:.3e} at max |logit| = {float(a.abs().max()):.3e}; "
          f"{int((a != b).sum())} of {a.numel()} logits differ; top-1 equal in {top1} of {a.shape[0]}")


@pytest.mark.parametrize("flag, counts", [("layer_norms", (2 * DEPTH + 1, 0)), ("gelu", (0, DEPTH))])
@pytest.mark.parametrize("tag", sorted(CASES))
def test_one_flag(tag, flag, counts):
    net, x = calibrated(tag)
    on = fuse_inference(net, **{flag: True})
    assert (on.fusion_report.layer_norms, on.fusion_report.gelus) == counts
    with torch.no_grad():
        out, tags = tagged(lambda: on(x))
        ref = fuse_inference(net)(x)
    assert (tags.count("layernorm"), tags.count("gelu")) == counts and tuple(out.shape) == (3, 10) and bool(torch.isfinite(out).all())
    print(f"{tag} / {flag}: max |logit - logit(flags off)| = {float((out - ref).abs().max()):.3e}")
