"""The front of a vision transformer on the frozen int8 plan, on the GPU (fuse_inference(patch_embed=True)): the small ViT of
test_gpu_transformer.py (17 tokens, 192 patch features, batch 3), FSPTQ and QBase W8A8, calibrated as there.  Both new nodes are
bit-exact restatements of the ops they replace, so nothing downstream may move: the logits of the plan with the flag are torch.equal to
the logits of the plan without it - with the flag alone, and with the LayerNorm, GELU and attention nodes on in both plans.  The
embedding receives a code tensor, its own quantise pass is gone from the launch stream, and a channels_last image batch - which the kernel
does not read in place - takes the torch restatement inside the node and still matches."""
import pytest
import torch

from dlmc.utils.fuse import PatchRowsLayer, TokenAssembleLayer, fuse_inference
from test_gpu_gate import tagged
from test_gpu_transformer import CASES, calibrated

pytestmark = pytest.mark.gpu
OTHERS = {"alone": {}, "every_transformer_flag": dict(layer_norms=True, gelu=True, attention=True)}


@pytest.mark.parametrize("others", sorted(OTHERS))
@pytest.mark.parametrize("tag", sorted(CASES))
def test_logits_equal_the_plan_without_the_flag(tag, others):
    net, x = calibrated(tag)
    kw = OTHERS[others]
    off = fuse_inference(net, **kw)
    on = fuse_inference(net, patch_embed=True, **kw)
    ro, rn = off.fusion_report, on.fusion_report
    print(rn)
    assert (ro.patch_rows, ro.token_assemblies) == (0, 0) and (rn.patch_rows, rn.token_assemblies, rn.patch_embed_left) == (1, 1, [])
    for f in ("layers", "residual", "emit", "fp32_outputs", "skipped", "layer_norms", "gelus", "attentions"):
        assert getattr(rn, f) == getattr(ro, f), f
    assert sum(isinstance(m, PatchRowsLayer) for m in on.modules()) == 1 and sum(isinstance(m, TokenAssembleLayer) for m in on.modules()) == 1
    embed = dict(on.named_modules())["_int8_plan_0"]
    seen = []
    hook = embed.register_forward_hook(lambda mod, a, r: seen.append(a[0].dtype))
    with torch.no_grad():
        (a, tags_off), (b, tags_on) = tagged(lambda: off(x)), tagged(lambda: on(x))
        hook.remove()
        again = on(x)
        cl, tags_cl = tagged(lambda: on(x.contiguous(memory_format=torch.channels_last)))
    assert len(seen) == 1 and seen[0] in (torch.uint8, torch.int8), seen      # the embedding reads codes
    assert tags_on.count("patch_rows") == 1 and tags_on.count("tokens") == 1 and "patch_rows" not in tags_off and "tokens" not in tags_off
    assert tags_off.count("fq_tensor") - tags_on.count("fq_tensor") == 1      # the embedding's own quantise pass is gone
    assert tuple(b.shape) == (3, 10) and bool(torch.isfinite(b).all())
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} logits differ from the plan without the flag, max {float((a - b).abs().max())}"
    assert torch.equal(b, again)
    # channels_last: the node's torch restatement (the quantise pass is K.fake_quant again), the same logits
    assert "patch_rows" not in tags_cl and tags_cl.count("tokens") == 1 and tags_cl.count("fq_tensor") == tags_off.count("fq_tensor")
    assert torch.equal(cl, a)
