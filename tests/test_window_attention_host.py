"""Window attention on the host: the argument checks of dlmcq_window_attention_f32 on placeholder pointers (nothing is launched), and
the dry-run decisions of fuse_inference(window_attention=True) for workloads.window_vit and for the unbiased ViT."""
import ctypes
import inspect

import pytest
import torch

import transformer_nets as T
import workloads as W
from dlmc import _native as N
from dlmc.utils.fuse import WindowAttentionLayer, fuse_inference
from plan_dump import plan_text
from test_relu6_host import calibrated as fsptq
from test_transformer_host import EALIGN, EINVAL, KEY, nodes, readers


def _wa(q=1 << 12, k=1 << 13, v=1 << 14, bias=1 << 18, mask=1 << 19, out=1 << 15, codes=1 << 16, b=4, h=3, t=49, d=32, nw=2, bias_s=None,
        mask_s=None, scale=1 << 17, lo=0, hi=255, form=N.FORM_ZEROPOINT, entry="dlmcq_window_attention_f32"):
    packed, pad = (t * 3 * max(h, 1) * d, d, 3 * max(h, 1) * d), (t + 3) // 4 * 4      # (h = 0: strides of one head)
    bias_s, mask_s = bias_s or (t * pad, pad), mask_s or (t * pad, pad)
    _p = lambda x: None if x is None else ctypes.c_void_p(x)  # noqa: E731
    return getattr(N.lib, entry)(_p(q), _p(k), _p(v), _p(bias), _p(mask), _p(out), _p(codes), b, h, t, d, nw, *packed, *packed, *packed,
                                 packed[0] // 3, d, packed[2] // 3, *bias_s, *mask_s, 0.125, _p(scale), None, lo, hi, form, 0.0, None)


ANSWERS = {      # (empty problems are DLMCQ_OK with nothing launched; nW is not read without a mask)
    "b_0": (dict(b=0), 0), "h_0": (dict(h=0), 0), "b_0_null_pointers": (dict(b=0, q=None, k=None, v=None, out=None, codes=None), 0), "b_0_no_mask_nw_0": (dict(b=0, mask=None, nw=0), 0),
    "t_65": (dict(t=65), EINVAL), "t_0": (dict(t=0), EINVAL), "d_48": (dict(d=48), EINVAL),
    "bias_row_stride_49": (dict(bias_s=(49 * 49, 49)), EINVAL), "bias_row_stride_below_t": (dict(bias_s=(48 * 49, 48)), EINVAL),
    "mask_row_stride_50": (dict(mask_s=(49 * 50, 50)), EINVAL), "b_not_a_multiple_of_nw": (dict(b=5), EINVAL),
    "shifted_emission": (dict(form=N.FORM_ZEROPOINT | N.EMIT_SHIFT128), EINVAL), "no_output": (dict(out=None, codes=None), EINVAL),
    "out_misaligned": (dict(out=(1 << 15) + 8), EALIGN), "bias_misaligned": (dict(bias=(1 << 18) + 4), EALIGN),
    "quantiser_before_alignment": (dict(lo=5, hi=4, out=(1 << 15) + 8), EINVAL),      # (two faults: the earlier check answers)
}


@pytest.mark.parametrize("name", sorted(ANSWERS))
def test_return_codes_need_no_gpu(name):
    kw, rc = ANSWERS[name]
    assert _wa(**kw) == rc and len(N.SIGNATURES["dlmcq_window_attention_f32"][1]) == 36
    assert _wa(entry="dlmcq_window_attention_f16", **kw) == rc      # (the same window_attention_args, csrc/attention_common.h)


def test_window_vit_decisions():
    flags = dict(layer_norms=True, gelu=True)
    off = fuse_inference(fsptq(W.window_vit()), dry_run=True, **flags)
    on = fuse_inference(fsptq(W.window_vit()), dry_run=True, window_attention=True, **flags)
    ro, rn = off.fusion_report, on.fusion_report
    assert (rn.window_attentions, ro.window_attentions) == (4, 0) and "window attentions on the plan=4" in repr(rn) and "window" not in repr(ro)
    assert (rn.layers, rn.layer_norms, rn.gelus, rn.attentions) == (ro.layers, ro.layer_norms, ro.gelus, 0)
    mods = dict(on.named_modules())
    for i, nd in enumerate(nodes(on, "_int8_window_attention_")):
        m = mods[nd.target]
        assert isinstance(m, WindowAttentionLayer) and readers(nd) == {1: ["_int8_plan"]}      # to_out reads the codes, nobody the fp32
        assert (m.want_out, m.merged, m.flatten, m.pre_scaled, m.has_bias, m.has_mask, m.c, m.emit.key) == (False, True, False, False, True, bool(i % 2), 128, KEY)
        assert m.scale == 32 ** -0.5 and len(nd.args) == 3 + 1 + 2 * (i % 2) + 3      # (q, k, v, bias, [mask, nW], three sizes)
    assert not [n for n in on.graph.nodes if n.op == "call_function" and n.target in (torch.matmul, torch.softmax)]
    assert fuse_inference(fsptq(W.window_vit()), dry_run=True, attention=True, **flags).fusion_report.attentions == 0      # (left to this flag)


def test_the_unbiased_vit_and_the_default_are_as_they_were():
    assert inspect.signature(fuse_inference).parameters["window_attention"].default is False
    for kw in (dict(), dict(layer_norms=True, gelu=True, attention=True)):
        was = plan_text(fuse_inference(fsptq(T.small_vit()), dry_run=True, **kw))
        assert plan_text(fuse_inference(fsptq(T.small_vit()), dry_run=True, window_attention=True, **kw)) == was and "window" not in was


def test_a_pre_scaled_query_and_cpu_tensors_take_the_restatement():      # (the graph's own ops: the model's logits, bit for bit)
    class Pre(W.WindowAttention):
        def forward(self, x):
            qkv = self.to_qkv(x).reshape(x.shape[0], self.tokens, 3, self.heads, self.dim_head).permute(2, 0, 3, 1, 4)
            attn = torch.matmul(qkv[0] * 0.25, qkv[1].transpose(-2, -1)) + self.bias_table[self.bias_index].view(16, 16, -1).permute(2, 0, 1)
            return self.to_out(torch.matmul(attn.softmax(dim=-1), qkv[2]).transpose(1, 2).flatten(2))
    for net, x in ((Pre(64, 2, 4).eval(), torch.randn(4, 16, 64)), (W.window_vit(10, 64, 2, 4, depth=2).eval(), torch.randn(2, 64, 8, 8))):
        on = fuse_inference(net, window_attention=True)
        (first, *_) = [m for m in on.modules() if isinstance(m, WindowAttentionLayer)]
        assert on.fusion_report.window_attentions > 0 and first.pre_scaled == isinstance(net, Pre)
        assert torch.equal(on(x), net(x))
