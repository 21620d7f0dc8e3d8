"""Window attention on the f16 matrix cores (include/dlmcq.h: dlmcq_window_attention_f16; K.window_attention_quant(operands="f16");
fuse_inference(window_attention="f16")) against float64 on the CPU from the same fp32 inputs.  The bound csrc/window_attention_f16.hip
derives, e = 2^-11, u = 2^-24, nb = ceil(T / 32), t = the terms given, kappa = 2 (3 * 104 + 2 + 68 nb) + 1:
    delta_i = max over the finite keys j of ((2 e + e^2) + (2 D + 1) u) |scale| sum_k |q_ik k_jk| + t u (|scale a*_ij| + |bias_ij| + |mask_ij|)
    rho_i = expm1(2 delta_i + 3 e + 2^-20 + kappa u);   |out_ic - o*_ic| <= rho_i sum_j p*_ij |v_jc| + T 2^-24 max_j |v_jc| + 2^-25
Measured ratios (MI355X): test_bound at most 0.085, the -inf masks 0.064, the plan's nodes 0.120; per shape: DESIGN.md 5.33."""
import copy

import pytest
import torch

import workloads as W
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import WindowAttentionLayer, fuse_inference
from test_gpu_attention_f16 import integers
from test_gpu_window_attention import DEV, SHAPES, bits, case, own_codes, quantisers, unmerge

pytestmark = pytest.mark.gpu
E, U = 2.0 ** -11, 2.0 ** -24


def f16(q, k, v, scale, **kw):
    """The kernel's out as [B, H, T, D] on the CPU."""
    return unmerge(K.window_attention_quant(q, k, v, scale, operands="f16", **kw)[0], q.shape[1]).cpu()


def ratio(got, q, k, v, scale, bias, mask, what, skip=None):
    """(max |got - o*| / bound over the rows that are not NaN in o* nor in `skip`, o*): float64 from the fp32 tensors; bias [H, T, T],
    mask [nW, T, T] or None."""
    q, k, v = q.cpu().double(), k.cpu().double(), v.cpu().double()
    (b, h, t, d), given = q.shape, [x.cpu().double() for x in (bias, mask) if x is not None]
    s = scale * (q @ k.transpose(-1, -2))
    add, mag = torch.zeros_like(s), s.abs()
    for term in ([] if bias is None else [given[0][None]]) + ([] if mask is None else [given[-1].repeat(b // mask.shape[0], 1, 1)[:, None]]):
        add, mag = add + term, mag + term.abs()
    p = torch.softmax(s + add, dim=-1)
    delta = ((2 * E + E * E) + (2 * d + 1) * U) * abs(scale) * (q.abs() @ k.abs().transpose(-1, -2)) + len(given) * U * mag
    delta = torch.where(torch.isfinite(add), delta, torch.zeros(())).amax(-1, keepdim=True)
    rho = torch.expm1(2 * delta + 3 * E + 2.0 ** -20 + (2 * (3 * 104 + 2 + 68 * ((t + 31) // 32)) + 1) * U)
    ref, bnd = p @ v, rho * (p @ v.abs()) + t * 2.0 ** -24 * v.abs().amax(-2, keepdim=True) + 2.0 ** -25
    live = ~ref.isnan() if skip is None else ~ref.isnan() & ~skip
    worst = float(((got.double() - ref).abs() / bnd)[live].nan_to_num(nan=float("inf")).max())
    print(f"{what}: max |out - o*| / bound = {worst:.4f}")
    return worst, ref


@pytest.mark.parametrize("term", ["bias", "mask", "shared_bias"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_placement_through_the_term(shape, term):
    """q = 0 and test_gpu_window_attention's table: the chosen key leads its row by 150, so every other P is an f16 zero and l = 1; the
    table is not symmetric in (i, j) and differs per head (bias) / window (mask: b % nW).  The output is the selected row of v."""
    b, h, t, d, _ = shape
    rows = h if term == "bias" else 1 if term == "shared_bias" else (2 if b % 2 == 0 else 1)
    r, i, j = torch.arange(rows)[:, None, None], torch.arange(t)[None, :, None], torch.arange(t)[None, None, :]
    pick = (7 * i + 3 + 5 * r) % t
    table = torch.where(j == pick, 200.0, ((3 * i + 5 * j + r) % 50).float())
    sel = pick[:, :, 0].expand(h, t)[None].expand(b, h, t) if "bias" in term else pick[:, :, 0].repeat(b // rows, 1)[:, None].expand(b, h, t)
    v = integers(b, h, t, d)
    want = torch.gather(v, 2, sel[..., None].expand(b, h, t, d))
    kw = dict(bias=table.to(DEV)) if "bias" in term else dict(mask=table.to(DEV)[None, :, None])      # (Swin's [1, nW, 1, T, T])
    got = f16(torch.zeros(b, h, t, d, device=DEV), torch.randn(b, h, t, d, device=DEV), v.to(DEV), 0.125, **kw)
    assert torch.equal(bits(got), bits(want)), f"{int((got != want).sum())} of {want.numel()} elements are not the selected v"


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_lane_and_key_maps(shape):
    """No term: k_j = the +-1 code of j's bits, q_i = the code of its chosen key, scale 16 - every other key is at least 4 D behind."""
    b, h, t, d, _ = shape
    j = torch.arange(t)
    code = torch.stack([((j >> (c % 8)) & 1).float() * 2 - 1 for c in range(d)], dim=1)
    pi = (7 * torch.arange(t)[None, None, :] + 3 + 5 * torch.arange(h)[None, :, None] + 11 * torch.arange(b)[:, None, None]) % t
    k, q, v = code.expand(b, h, t, d).contiguous(), code[pi], integers(b, h, t, d)
    top = (16.0 * (q.double() @ k.double().transpose(-1, -2))).topk(min(2, t), dim=-1)
    assert bool((top.indices[..., 0] == pi).all()) and (t == 1 or bool((top.values[..., 0] - top.values[..., 1] >= 4 * d).all()))
    got, want = f16(q.to(DEV), k.to(DEV), v.to(DEV), 16.0), torch.gather(v, 2, pi[..., None].expand(b, h, t, d))
    assert torch.equal(bits(got), bits(want)), f"{int((got != want).sum())} of {want.numel()} elements are not the selected v"


@pytest.mark.parametrize("t", [1, 2, 31, 32, 33, 49, 63, 64])
def test_uniform_rows(t):
    """q = 0, constant terms: P = 1, l = T, out = fl32(column sum / T), bitwise; every operand a view into a NaN-filled parent."""
    b, h, d, pad = 2, 2, 32, (t + 3) // 4 * 4
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    q, k, v = (p[:, :, 1:t + 1] for p in (nan(b, h, t + 2, d), nan(b, h, t + 2, d), nan(b, h, t + 2, d)))
    bias, mask = nan(h, t + 2, pad + 8)[:, 1:t + 1, 4:4 + t], nan(2, t + 2, pad + 8)[:, 1:t + 1, 4:4 + t]
    assert K.window_term_view(bias, t) is not None and K.window_term_view(mask, t) is not None      # (read in place)
    q.zero_(), k.normal_(), bias.fill_(1.5), mask.fill_(-2.25), v.copy_(integers(b, h, t, d))
    want = (v.cpu().double().sum(2, keepdim=True).float() / t).expand(b, h, t, d)
    assert torch.equal(bits(f16(q, k, v, 0.125, bias=bias, mask=mask)), bits(want))


@pytest.mark.parametrize("family", ["n01", "peaky"])
@pytest.mark.parametrize("terms", ["bias", "mask", "bias+mask"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_bound(shape, terms, family):
    q, k, v, bias, mask = case(shape)
    q = q * 4 if family == "peaky" else q
    bias, mask = (bias if "bias" in terms else None), (mask if "mask" in terms else None)
    scale, m5 = shape[3] ** -0.5, (None if mask is None else mask[None, :, None])      # (Swin's [1, nW, 1, T, T])
    assert ratio(f16(q, k, v, scale, bias=bias, mask=m5), q, k, v, scale, bias, mask, f"{shape} {terms} {family}")[0] <= 1.0


@pytest.mark.parametrize("shape", SHAPES[:2], ids=str)
def test_minus_infinity_mask(shape):
    """-inf removes a key: float64 attention over the other keys; a row with every key removed is NaN, and exactly those rows are."""
    q, k, v, bias, mask = case(shape)
    mask = torch.where(mask < 0, float("-inf"), 0.0)
    mask[1, 2] = float("-inf")
    got = f16(q, k, v, 0.125, bias=bias, mask=mask)
    worst, ref = ratio(got, q, k, v, 0.125, bias, mask, f"{shape} -inf")
    assert worst <= 1.0 and torch.equal(got.isnan(), ref.isnan()) and bool(got[1::shape[4], :, 2].isnan().all())
    assert int(got.isnan().sum()) == (shape[0] // shape[4]) * shape[1] * shape[3]      # (those rows and no other)


def test_range():
    """1e5 in one element of one query row is +inf as an operand: that row of that head is non-finite, every other row within the bound."""
    q, k, v, bias, mask = case(SHAPES[0])
    q = q.clone()
    q[1, 0, 40, 9] = 1e5
    hit = torch.zeros(q.shape, dtype=torch.bool)
    hit[1, 0, 40] = True
    got = f16(q, k, v, 0.125, bias=bias, mask=mask)
    assert not bool(torch.isfinite(got[hit]).any()) and ratio(got, q, k, v, 0.125, bias, mask, "range", skip=hit)[0] <= 1.0


@pytest.mark.parametrize("name", ["fsptq_zeropoint_u8", "qbase_s8_g"])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=str)
def test_codes_outputs_and_one_head_alone(shape, name):
    b, h, t, d, nw = shape
    q, k, v, bias, mask = case(shape)
    sc, z, lo, hi, form, gq = qz = quantisers()[name]
    run = lambda *a, **kw: K.window_attention_quant(*a, 0.125, operands="f16", **kw)  # noqa: E731
    plain = run(q, k, v, bias=bias, mask=mask)[0]
    out, codes = run(q, k, v, bias=bias, mask=mask, emit=K.EmitCodes(sc, z, lo, hi, form, gq))
    assert tuple(out.shape) == tuple(codes.shape) == (b, t, h * d) and torch.equal(bits(out), bits(plain))
    assert torch.equal(codes.view(torch.uint8), own_codes(out, qz))
    none, only = run(q, k, v, bias=bias, mask=mask, emit=K.EmitCodes(sc, z, lo, hi, form, gq), want_out=False)
    assert none is None and torch.equal(only, codes)
    for bi, hi_ in ((1, h - 1), (0, 0)):
        one = lambda x: x[bi:bi + 1, hi_:hi_ + 1]  # noqa: E731
        alone = run(one(q), one(k), one(v), bias=bias[hi_:hi_ + 1], mask=mask[bi % nw:bi % nw + 1])[0]
        assert torch.equal(bits(alone[0]), bits(unmerge(plain, h)[bi, hi_]))


@pytest.mark.parametrize("tag", ["fsptq", "qbase"])
def test_the_plan(tag):
    """test_gpu_window_attention's small window_vit (T = 49, D = 32, 12 windows, 2 blocks, the second masked) with window_attention="f16":
    one f16 node per block, each within the bound on the tensors it received, its codes those of its own output, finite logits."""
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
        for m in net.modules():      # (integer zero points for FSPTQ, no float offset for QBase: what the plan takes)
            if isinstance(m, FSPTQBase):
                m.in_offset.round_().clamp_(m.in_min_val, m.in_max_val)
                m._zp_is_int = None
            elif getattr(m, "in_offset", None) is not None:
                m.in_offset.zero_()
    on = fuse_inference(net, window_attention="f16", layer_norms=True, gelu=True)
    layers = [m for m in on.modules() if isinstance(m, WindowAttentionLayer)]
    assert on.fusion_report.window_attentions == len(layers) == 2 and on.fusion_report.window_attention_operands == "f16"
    assert [m.has_mask for m in layers] == [False, True] and all(m.operands == "f16" and m.has_bias and m.emit is not None for m in layers)
    seen = []
    for m in layers:
        m.want_out = True
        m.register_forward_hook(lambda mod, a, r: seen.append((mod, a, r)))
    with torch.no_grad():
        logits = on(x)
    for m, args, (out, codes) in seen:
        q, k, v, bias = args[:4]
        worst, _ = ratio(unmerge(out, q.shape[1]).cpu(), q, k, v, m.scale, bias[0], args[4][0, :, 0] if m.has_mask else None, f"{tag} node")
        e = m.emit
        want = K.fake_quant(out, e.scale, e.zp, e.lo, e.hi, e.form, g=e.g(q.numel()), codes="i8", want_y=False)[1]
        assert worst <= 1.0 and torch.equal(codes.view(torch.uint8), want.view(torch.uint8))
    assert len(seen) == 2 and bool(torch.isfinite(logits).all())
