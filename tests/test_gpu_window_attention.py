"""Window attention on the GPU (include/dlmcq.h: dlmcq_window_attention_f32; K.window_attention_quant; fuse_inference(window_attention=
True)) against float64 on the CPU from the same fp32 inputs.  The header's bound, u = 2^-24, nb = ceil(T / 32), t = the terms given:
    delta_i = max over the finite keys j of (D + 1) u |scale| sum_k |q_ik k_jk| + t u (|scale a*_ij| + |bias_ij| + |mask_ij|)
    |out_ic - o*_ic| <= (2 delta_i + (2 (104 + 2 + 32 nb) + 1) u) sum_j p*_ij |v_jc| + 2^-126 max_j |v_jc|."""
import copy
import functools

import pytest
import torch

import workloads as W
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import WindowAttentionLayer, fuse_inference
from test_gpu_attention import f32, unmerge
from test_gpu_gate import DEV, bits
from test_gpu_layernorm import own_codes, quantisers

pytestmark = pytest.mark.gpu
SHAPES = [(4, 3, 49, 32, 2), (2, 2, 64, 64, 2), (3, 1, 16, 32, 1), (2, 2, 33, 64, 1), (1, 2, 1, 32, 1)]      # (B, H, T, D, nW)


def reference(q, k, v, scale, bias, mask, U=2.0 ** -24):
    """(o*, bound) in float64 from fp32 CPU tensors; bias [H, T, T] or None, mask [nW, T, T] or None."""
    q, k, v = q.double(), k.double(), v.double()
    (b, h, t, d), terms = q.shape, (bias is not None) + (mask is not None)
    s = scale * (q @ k.transpose(-1, -2))
    add, mag = torch.zeros(b, h, t, t, dtype=torch.float64), s.abs()
    for term in ([] if bias is None else [bias.double()[None]]) + ([] if mask is None else [mask.double().repeat(b // mask.shape[0], 1, 1)[:, None]]):
        add, mag = add + term, mag + term.abs()
    p = torch.softmax(s + add, dim=-1)
    delta = (d + 1) * U * abs(scale) * (q.abs() @ k.abs().transpose(-1, -2)) + terms * U * mag
    delta = torch.where(torch.isfinite(add), delta, torch.zeros(())).amax(-1, keepdim=True)
    kappa = 2 * (104 + 2 + 32 * ((t + 31) // 32)) + 1
    return p @ v, (2 * delta + kappa * U) * (p @ v.abs()) + 2.0 ** -126 * v.abs().amax(-2, keepdim=True)


def within(out, q, k, v, scale, bias, mask, what):
    ref, bnd = reference(q.cpu(), k.cpu(), v.cpu(), scale, None if bias is None else bias.cpu(), None if mask is None else mask.cpu())
    err, live = (unmerge(out, q.shape[1]).cpu().double() - ref).abs(), ~ref.isnan()
    ratio = float((err / bnd.clamp_min(1e-300))[live].max())
    print(f"{what}: max |out - o*| / bound = {ratio:.4f}")
    return ratio, ref


@functools.lru_cache(maxsize=None)
def case(shape):
    """(q, k, v views of one packed projection output, bias [H, T, T], mask [nW, T, T] of 0 / -100, diagonal 0) on the device, shared."""
    b, h, t, d, nw = shape
    g = torch.Generator().manual_seed(sum(shape))
    p = torch.randn(b, t, 3 * h * d, generator=g).to(DEV).reshape(b, t, 3, h, d).permute(2, 0, 3, 1, 4)
    mask = torch.where((torch.rand(nw, t, t, generator=g) < 0.4) & ~torch.eye(t, dtype=torch.bool), -100.0, 0.0)
    return p[0], p[1], p[2], torch.randn(h, t, t, generator=g).to(DEV), mask.to(DEV)


def integers(b, h, t, d):
    return (torch.arange(b * h * t * d).reshape(b, h, t, d) + 1).float()


@pytest.mark.parametrize("term", ["bias", "mask", "shared_bias"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_placement_through_the_term(shape, term):
    """q = 0: the term alone decides.  Its largest entry of a row leads by 150, it is not symmetric in (i, j) - the kernel computes S^T -
    and differs per head (bias) / per window (mask: b % nW); shared_bias: one [1, T, T] tile for every head (T = 49: the padded copy)."""
    b, h, t, d, _ = shape
    rows = h if term == "bias" else 1 if term == "shared_bias" else (2 if b % 2 == 0 else 1)
    r, i, j = torch.arange(rows)[:, None, None], torch.arange(t)[None, :, None], torch.arange(t)[None, None, :]
    pick = (7 * i + 3 + 5 * r) % t
    table = torch.where(j == pick, 200.0, ((3 * i + 5 * j + r) % 50).float())
    top = table.topk(min(2, t), dim=-1).values
    assert t == 1 or (bool((top[..., 0] - top[..., 1] > 110).all()) and not torch.equal(table, table.transpose(1, 2)))
    v = integers(b, h, t, d)
    assert float(v.max()) < 2 ** 24 and v.unique().numel() == v.numel()
    sel = pick[:, :, 0].expand(h, t)[None].expand(b, h, t) if "bias" in term else pick[:, :, 0].repeat(b // rows, 1)[:, None].expand(b, h, t)
    want = torch.gather(v, 2, sel[..., None].expand(b, h, t, d))
    kw = dict(bias=table.to(DEV)) if "bias" in term else dict(mask=table.to(DEV)[None, :, None])      # (Swin's [1, nW, 1, T, T])
    got = unmerge(K.window_attention_quant(torch.zeros(b, h, t, d, device=DEV), torch.randn(b, h, t, d, device=DEV), v.to(DEV), 0.125, **kw)[0], h).cpu()
    assert torch.equal(bits(got), bits(want)), f"{int((got != want).sum())} of {want.numel()} elements are not the selected v"


@pytest.mark.parametrize("t", [1, 2, 31, 32, 33, 49, 63, 64])
def test_uniform_rows(t):
    """q = 0, constant terms: p = 1, l = T, out = fl32(column sum / T), bitwise; every operand a view into a NaN-filled parent."""
    b, h, d, pad = 2, 2, 32, (t + 3) // 4 * 4
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    q, k, v = (p[:, :, 1:t + 1] for p in (nan(b, h, t + 2, d), nan(b, h, t + 2, d), nan(b, h, t + 2, d)))
    bias, mask = nan(h, t + 2, pad + 8)[:, 1:t + 1, 4:4 + t], nan(2, t + 2, pad + 8)[:, 1:t + 1, 4:4 + t]
    assert K.window_term_view(bias, t) is not None and K.window_term_view(mask, t) is not None      # (read in place)
    q.zero_(), k.normal_(), bias.fill_(1.5), mask.fill_(-2.25), v.copy_(integers(b, h, t, d))
    want = (v.cpu().double().sum(2, keepdim=True).float() / t).expand(b, h, t, d)
    got = unmerge(K.window_attention_quant(q, k, v, 0.125, bias=bias, mask=mask)[0], h).cpu()
    assert torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("terms", ["bias", "mask", "bias+mask"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_bound(shape, terms):
    q, k, v, bias, mask = case(shape)
    bias, mask = (bias if "bias" in terms else None), (mask if "mask" in terms else None)
    scale, m5 = f32(shape[3] ** -0.5), (None if mask is None else mask[None, :, None])      # (Swin's [1, nW, 1, T, T])
    out, _ = K.window_attention_quant(q, k, v, scale, bias=bias, mask=m5)
    ratio, _ = within(out, q, k, v, scale, bias, mask, f"{shape} {terms}")
    assert ratio <= 1.0


@pytest.mark.parametrize("shape", SHAPES[:2], ids=str)
def test_minus_infinity_mask(shape):
    """-inf removes a key: float64 attention over the other keys; a row with every key removed is NaN and its neighbours are finite."""
    q, k, v, bias, mask = case(shape)
    mask = torch.where(mask < 0, float("-inf"), 0.0)
    mask[1, 2] = float("-inf")
    out, _ = K.window_attention_quant(q, k, v, 0.125, bias=bias, mask=mask)
    ratio, ref = within(out, q, k, v, 0.125, bias, mask, f"{shape} -inf")
    got = unmerge(out, shape[1]).cpu()
    assert ratio <= 1.0 and torch.equal(got.isnan(), ref.isnan()) and bool(got[1::shape[4], :, 2].isnan().all())
    assert int(got.isnan().sum()) == (shape[0] // shape[4]) * shape[1] * shape[3]      # (those rows and no other)


@pytest.mark.parametrize("name", ["fsptq_zeropoint_u8", "qbase_s8_g"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=str)
def test_codes_outputs_and_one_head_alone(shape, name):
    b, h, t, d, nw = shape
    q, k, v, bias, mask = case(shape)
    sc, z, lo, hi, form, gq = qz = quantisers()[name]
    em = lambda: K.EmitCodes(sc, z, lo, hi, form, gq)  # noqa: E731
    plain = K.window_attention_quant(q, k, v, 0.125, bias=bias, mask=mask)[0]
    out, codes = K.window_attention_quant(q, k, v, 0.125, bias=bias, mask=mask, emit=em())
    assert tuple(out.shape) == tuple(codes.shape) == (b, t, h * d) and torch.equal(bits(out), bits(plain))
    assert torch.equal(codes.view(torch.uint8), own_codes(out, qz))
    none, only = K.window_attention_quant(q, k, v, 0.125, bias=bias, mask=mask, emit=em(), want_out=False)
    assert none is None and torch.equal(only, codes)
    for bi, hi_ in ((1, h - 1), (0, 0)):
        one = lambda x: x[bi:bi + 1, hi_:hi_ + 1]  # noqa: E731
        alone = K.window_attention_quant(one(q), one(k), one(v), 0.125, bias=bias[hi_:hi_ + 1], mask=mask[bi % nw:bi % nw + 1])[0]
        assert torch.equal(bits(alone[0]), bits(unmerge(plain, h)[bi, hi_]))


@pytest.mark.parametrize("tag", ["fsptq", "qbase"])
def test_the_plan(tag):
    """window_vit (T = 49, D = 32, 12 windows, 2 blocks, the second masked): one node per block, every node within the bound on the
    inputs it received, codes of its own output.  Logits against the flag-off plan: a node within its bound (asserted) moves a code only
    across a quantiser tie, so by at most one step against its torch restatement's codes (asserted per node); the tolerance is that
    one step of an 8-bit quantiser, 1 / 255, of the logits' own range."""
    from dlmc.utils.quantize import quantize_model
    from dlmc.quantization.scalar.FSPTQuant import FSPTQBase
    from test_gpu_transformer import CASES
    cfg, qtype = CASES[tag]
    torch.manual_seed(7)
    net = W.window_vit(num_classes=10, dim=64, heads=2, depth=2).to(DEV).eval()
    quantize_model(net, copy.deepcopy(cfg), None, *([qtype] if qtype else []), **(dict(int8_gemm=True) if qtype else {}))
    x = torch.randn(3, 64, 14, 14, device=DEV)
    with torch.no_grad():
        net(x)
        for m in net.modules():      # (test_gpu_transformer.calibrated's: integer zero points for FSPTQ, no float offset for QBase)
            if isinstance(m, FSPTQBase):
                m.in_offset.round_().clamp_(m.in_min_val, m.in_max_val)
                m._zp_is_int = None
            elif getattr(m, "in_offset", None) is not None:
                m.in_offset.zero_()
    off, on = fuse_inference(net, layer_norms=True, gelu=True), fuse_inference(net, window_attention=True, layer_norms=True, gelu=True)
    layers = [m for m in on.modules() if isinstance(m, WindowAttentionLayer)]
    assert on.fusion_report.window_attentions == len(layers) == 2 and off.fusion_report.window_attentions == 0
    assert [m.has_mask for m in layers] == [False, True] and all(m.has_bias and m.merged and m.emit is not None for m in layers)
    seen = []
    for m in layers:
        m.want_out = True
        m.register_forward_hook(lambda mod, a, r: seen.append((mod, a, r)))
    with torch.no_grad():
        a, bb = off(x), on(x)
    for m, args, (out, codes) in seen:
        q, k, v, bias = args[:4]
        mask = args[4][0, :, 0] if m.has_mask else None
        torch_codes = m._torch(q, k, v, bias, *(args[4:6] if m.has_mask else (None, None)), args[-3:])[1]
        assert int((codes.view(torch.uint8).short() - torch_codes.view(torch.uint8).short()).abs().max()) <= 1
        ratio, _ = within(out, q, k, v, m.scale, bias[0], mask, f"{tag} node")
        e = m.emit
        want = K.fake_quant(out, e.scale, e.zp, e.lo, e.hi, e.form, g=e.g(q.numel()), codes="i8", want_y=False)[1]
        assert ratio <= 1.0 and torch.equal(codes.view(torch.uint8), want.view(torch.uint8))
    delta, top = float((a - bb).abs().max()), float(a.abs().max())
    print(f"{tag}: max |delta logit| = {delta:.3e} at max |logit| = {top:.3e}")
    assert bool(torch.isfinite(bb).all()) and delta <= top / 255
