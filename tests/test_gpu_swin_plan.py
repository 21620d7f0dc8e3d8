"""fuse_inference(swin_geometry=True) on a small SwinNet (dim 64, heads (2, 4), window 4, 32^2 images: an 8 x 8 map, then 4 x 4) at
batch 3: the node counts, codes into every taker Linear, and the "substituted network" check of DESIGN.md 5.23 - the logits are
torch.equal to the same plan with the three K wrappers replaced by a torch gather in front of K.layernorm_quant and a torch add.
Against the plan without the flag the window and merge norms differ in their summation order (as `layer_norms` does against torch):
the differing logits are printed (DESIGN.md 5.34 records them) and top-1 has to agree for QBase."""
import copy

import pytest
import torch

import workloads as W
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import MergeNormLayer, WindowNormLayer, fuse_inference
from test_gpu_transformer import CASES

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLAGS = dict(layer_norms=True, gelu=True, window_attention=True)


def window_norm(x, weight, bias, eps, window, shift, emit=None, want_out=True):
    b, h, w, c = x.shape
    rows = torch.roll(x, (-shift[0], -shift[1]), (1, 2)).reshape(b, h // window, window, w // window, window, c)
    return K.layernorm_quant(rows.permute(0, 1, 3, 2, 4, 5).reshape(-1, window * window, c), weight, bias, eps, emit=emit, want_out=want_out)


def merge_norm(x, weight, bias, eps, emit=None, want_out=True):
    rows = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1)
    return K.layernorm_quant(rows.reshape(x.shape[0], -1, 4 * x.shape[3]), weight, bias, eps, emit=emit, want_out=want_out)


def reverse_add(yw, shortcut, window, shift):
    b, h, w, c = shortcut.shape
    back = yw.reshape(b, h // window, w // window, window, window, c).permute(0, 1, 3, 2, 4, 5).reshape(b, h, w, c)
    return shortcut + torch.roll(back, tuple(shift), (1, 2))


@pytest.mark.parametrize("tag", ["fsptq", "qbase"])
def test_the_plan(tag, monkeypatch):
    from dlmc.quantization.scalar.FSPTQuant import FSPTQBase
    from dlmc.utils.quantize import quantize_model
    cfg, qtype = CASES[tag]
    torch.manual_seed(11)
    net = W.SwinNet(10, 64, (2, 2), (2, 4), 4, 32, 4).to(DEV).eval()
    quantize_model(net, copy.deepcopy(cfg), None, *([qtype] if qtype else []), **(dict(int8_gemm=True) if qtype else {}))
    x = torch.randn(3, 3, 32, 32, device=DEV)
    with torch.no_grad():
        net(x)
        for m in net.modules():      # (integer zero points for FSPTQ, no float offset for QBase: what the plan takes)
            if isinstance(m, FSPTQBase):
                m.in_offset.round_().clamp_(m.in_min_val, m.in_max_val)
                m._zp_is_int = None
            elif getattr(m, "in_offset", None) is not None:
                m.in_offset.zero_()
    on, off = fuse_inference(net, swin_geometry=True, **FLAGS), fuse_inference(net, **FLAGS)
    rep = on.fusion_report
    assert (rep.window_norms, rep.window_adds, rep.merge_norms, rep.window_attentions) == (4, 4, 1, 4)
    modules, fed = dict(on.named_modules()), []
    for node in on.graph.nodes:      # the readers of a gather node's codes (output 1): Linear plan layers
        if node.op == "call_module" and isinstance(modules[node.target], (WindowNormLayer, MergeNormLayer)):
            takers = [t for get in node.users for t in get.users]
            assert takers and all(get.args[1] == 1 for get in node.users)
            for t in takers:
                modules[t.target].register_forward_pre_hook(lambda mod, args: fed.append(args[0].dtype))
    with torch.no_grad():
        logits, plain = on(x), off(x)
        assert len(fed) == 5 and all(d in (torch.uint8, torch.int8) for d in fed)
        monkeypatch.setattr(K, "layernorm_window_quant", window_norm)
        monkeypatch.setattr(K, "layernorm_merge_quant", merge_norm)
        monkeypatch.setattr(K, "window_reverse_add", reverse_add)
        assert torch.equal(on(x), logits)
    differ = logits != plain
    print(f"{tag}: {int(differ.sum())} of {logits.numel()} logits differ from the flag-off plan, by at most "
          f"{float((logits - plain).abs().max()):.3g} at a largest logit of {float(plain.abs().max()):.3g}")
    assert bool(torch.isfinite(logits).all())
    if tag == "qbase":
        assert torch.equal(logits.argmax(1), plain.argmax(1))
