"""Window attention past 64 tokens on the GPU (include/dlmcq.h: dlmcq_window_attention_stream_f32; K.window_attention_quant(stream=...);
fuse_inference(window_attention=True) at T = 144) against float64 on the CPU from the same fp32 inputs.  The header's bound is
dlmcq_window_attention_f32's with kappa = 2 (104 + 2 + 3 nb + 32 nb) + 1: the streamed fold adds 3 nb per side (`al` and its multiply).
Measured max |out - o*| / bound, MI355X: the bound cases 0.003 .. 0.010, the plan's nodes 0.006 .. 0.008."""
import copy
import functools

import pytest
import torch

import test_gpu_window_attention as WA
import workloads as W
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import WindowAttentionLayer, fuse_inference
from test_gpu_attention import f32, unmerge
from test_gpu_gate import DEV, bits
from test_gpu_layernorm import own_codes, quantisers
from test_gpu_window_attention import case, integers

pytestmark = pytest.mark.gpu
SHAPES = [(2, 2, 65, 32, 2), (2, 1, 96, 64, 1), (4, 3, 144, 32, 2), (1, 2, 256, 64, 1), (2, 2, 49, 32, 2)]      # (B, H, T, D, nW)
NEG = float("-inf")
stream = functools.partial(K.window_attention_quant, stream=True)      # (T = 49: forced; T > 64: what None picks)


def ratio(out, q, k, v, scale, bias, mask, what):
    """max |out - o*| / bound: WA.reference's bound plus 2 * 3 nb u sum_j p*_ij |v_jc| (the streamed kernel's kappa; its o* of |v|)."""
    cpu = [q.cpu(), k.cpu(), v.cpu(), scale, None if bias is None else bias.cpu(), None if mask is None else mask.cpu()]
    ref, bnd = WA.reference(*cpu)
    bnd = bnd + 6 * ((q.shape[2] + 31) // 32) * 2.0 ** -24 * WA.reference(cpu[0], cpu[1], cpu[2].abs(), *cpu[3:])[0]
    r = float(((unmerge(out, q.shape[1]).cpu().double() - ref).abs() / bnd.clamp_min(1e-300))[~ref.isnan()].max())
    print(f"{what}: max |out - o*| / bound = {r:.4f}")
    return r


@pytest.mark.parametrize("terms", ["bias", "mask", "bias+mask", "none"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_bound(shape, terms):
    q, k, v, bias, mask = case(shape)
    bias, mask = (bias if "bias" in terms else None), (mask if "mask" in terms else None)
    scale, m5 = f32(shape[3] ** -0.5), (None if mask is None else mask[None, :, None])      # (Swin's [1, nW, 1, T, T])
    out, _ = stream(q, k, v, scale, bias=bias, mask=m5)
    assert ratio(out, q, k, v, scale, bias, mask, f"{shape} {terms}") <= 1.0
    if shape[2] > K.WINDOW_TOKENS:      # (stream=None routes here; the other routes refuse as they did)
        assert torch.equal(bits(K.window_attention_quant(q, k, v, scale, bias=bias, mask=m5)[0]), bits(out))
        for kw in (dict(stream=False), dict(operands="f16"), dict(operands="f16", stream=True)):
            with pytest.raises(ValueError, match="T in 1 .. 64"):
                K.window_attention_quant(q, k, v, scale, bias=bias, mask=m5, **kw)


@pytest.mark.parametrize("term", ["bias", "mask"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_placement_through_minus_infinity(shape, term):
    """q = 0, the term -inf but at key pi(i) = (11 i + 3 + 5 r) mod T of row i (r: the head, or the window b % nW): out = v[pi], bitwise.
    Rows whose key lies in the last block have met only -inf blocks before it, rows whose key lies in the first only such after it."""
    b, h, t, d, nw = shape
    rows = h if term == "bias" else nw
    r, i, j = torch.arange(rows)[:, None, None], torch.arange(t)[None, :, None], torch.arange(t)[None, None, :]
    pick = (11 * i + 3 + 5 * r) % t
    assert pick[0].unique().numel() == t
    v = integers(b, h, t, d)
    sel = pick[:, :, 0].expand(h, t)[None].expand(b, h, t) if term == "bias" else pick[:, :, 0].repeat(b // rows, 1)[:, None].expand(b, h, t)
    want, table = torch.gather(v, 2, sel[..., None].expand(b, h, t, d)), torch.where(j == pick, 0.0, NEG).to(DEV)
    kw = dict(bias=table) if term == "bias" else dict(mask=table[None, :, None])
    got = unmerge(stream(torch.zeros(b, h, t, d, device=DEV), torch.randn(b, h, t, d, device=DEV), v.to(DEV), 0.125, **kw)[0], h).cpu()
    assert torch.equal(bits(got), bits(want)), f"{int((got != want).sum())} of {want.numel()} elements are not the selected v"


@pytest.mark.parametrize("t", [65, 144, 256])
def test_uniform_rows(t):
    """q = 0, finite zero terms: p = 1, l = T, out = fl32(column sum / T), bitwise (integer v, column sums below 2^24: exact)."""
    (b, h, d), zero = (2, 2, 32), torch.zeros(2, t, t, device=DEV)
    v = (integers(b, h, t, d) % 1000).to(DEV)
    want = (v.cpu().sum(2, keepdim=True) / t).expand(b, h, t, d)      # (on the CPU: a true fp32 division, not a multiply by 1 / T)
    got = unmerge(stream(torch.zeros(b, h, t, d, device=DEV), torch.randn(b, h, t, d, device=DEV), v, 0.125, bias=zero, mask=zero)[0], h).cpu()
    assert float(v.sum(2).max()) < 2 ** 24 and torch.equal(bits(got), bits(want))


@pytest.mark.parametrize("shape", SHAPES[:4], ids=str)
def test_a_fully_masked_row(shape):
    """One row of window 0 all -inf: NaN in every channel where that window applies; every other row as without it, bitwise."""
    q, k, v, bias, mask = case(shape)
    (b, h, t, d, nw), row = shape, shape[2] - 2
    dead = mask.clone()
    dead[0, row] = NEG
    plain, got = (unmerge(stream(q, k, v, 0.125, bias=bias, mask=m)[0], h) for m in (mask, dead))
    hit = torch.zeros(b, h, t, dtype=torch.bool, device=DEV)
    hit[0::nw, :, row] = True
    assert bool(got[hit].isnan().all()) and torch.equal(bits(got[~hit]), bits(plain[~hit])) and not bool(plain.isnan().any())


@pytest.mark.parametrize("name", ["fsptq_zeropoint_u8", "qbase_s8_g"])
@pytest.mark.parametrize("shape", SHAPES[2:], ids=str)
def test_codes_outputs_and_one_head_alone(shape, name):
    b, h, t, d, nw = shape
    q, k, v, bias, mask = case(shape)
    sc, z, lo, hi, form, gq = qz = quantisers()[name]
    em = lambda: K.EmitCodes(sc, z, lo, hi, form, gq)  # noqa: E731
    plain = stream(q, k, v, 0.125, bias=bias, mask=mask)[0]
    out, codes = stream(q, k, v, 0.125, bias=bias, mask=mask, emit=em())
    assert tuple(out.shape) == tuple(codes.shape) == (b, t, h * d) and torch.equal(bits(out), bits(plain))
    assert torch.equal(codes.view(torch.uint8), own_codes(out, qz))
    none, only = stream(q, k, v, 0.125, bias=bias, mask=mask, emit=em(), want_out=False)
    assert none is None and torch.equal(only, codes)
    for bi, hi_ in ((b - 1, h - 1), (0, 0)):
        one = lambda x: x[bi:bi + 1, hi_:hi_ + 1]  # noqa: E731
        alone = stream(one(q), one(k), one(v), 0.125, bias=bias[hi_:hi_ + 1], mask=mask[bi % nw:bi % nw + 1])[0]
        assert torch.equal(bits(alone[0]), bits(unmerge(plain, h)[bi, hi_]))


def test_the_plan():
    """window_vit(window=12): T = 144, D = 32, 2 blocks, the second masked: both launches are the streamed kernel's, and per node
    test_gpu_window_attention.test_the_plan's assertions - codes within one step of the torch restatement's, fp32 within the bound."""
    from dlmc.utils.quantize import quantize_model
    from dlmc.quantization.scalar.FSPTQuant import FSPTQBase
    from test_gpu_transformer import CASES
    torch.manual_seed(7)
    net = W.window_vit(num_classes=10, dim=64, heads=2, window=12, grid=2, depth=2).to(DEV).eval()
    quantize_model(net, copy.deepcopy(CASES["fsptq"][0]), None, CASES["fsptq"][1], int8_gemm=True)
    x = torch.randn(2, 64, 24, 24, device=DEV)
    with torch.no_grad():
        net(x)
        for m in (m for m in net.modules() if isinstance(m, FSPTQBase)):      # (test_gpu_transformer.calibrated's integer zero points)
            m.in_offset.round_().clamp_(m.in_min_val, m.in_max_val)
            m._zp_is_int = None
    on = fuse_inference(net, window_attention=True, layer_norms=True, gelu=True)
    layers, seen = [m for m in on.modules() if isinstance(m, WindowAttentionLayer)], []
    assert on.fusion_report.window_attentions == len(layers) == 2 and [m.has_mask for m in layers] == [False, True]
    for m in layers:
        m.want_out = True
        m.register_forward_hook(lambda mod, a, r: seen.append((mod, a, r)))
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        with torch.no_grad():
            logits = on(x)
    finally:
        tags, K.PROFILE.enabled = [r[0] for r in K.PROFILE.records if r[0].startswith("window_attention")], False
        K.PROFILE.reset()
    assert tags == ["window_attention_stream"] * 2 and bool(torch.isfinite(logits).all()) and len(seen) == 2
    for m, args, (out, codes) in seen:
        q, k, v, bias = args[:4]
        torch_codes = m._torch(q, k, v, bias, *(args[4:6] if m.has_mask else (None, None)), args[-3:])[1]
        assert tuple(q.shape[1:]) == (2, 144, 32) and int((codes.view(torch.uint8).short() - torch_codes.view(torch.uint8).short()).abs().max()) <= 1
        assert ratio(out, q, k, v, m.scale, bias[0], args[4][0, :, 0] if m.has_mask else None, "plan node") <= 1.0
