"""Attention on the GPU (include/dlmcq.h: dlmcq_attention_f32; K.attention_quant; fuse_inference(attention=True)).

(a) exact placement: one-hot softmax rows (largest score ahead by more than 110, checked in float64) pick integer rows of v, bitwise;
(b) tail masking: q = 0, v constant, views into NaN-filled parents, T around every tile edge;
(c) accuracy: the header's bound against float64 on the same fp32 inputs, u = 2^-24,
        delta_i = (D + 1) u scale max_j sum_k |q_ik k_jk|,  kappa = 2 (104 + 2 + 3 nb + 32 nb) + 1,  nb = ceil(Tk / 32),
        |out_ic - o*_ic| <= (2 delta_i + kappa u) sum_j p*_ij |v_jc| + 2^-126 max_j |v_jc|,
    for four input families, the two packed-qkv layouts and contiguous inputs; the largest ratio is printed (DESIGN.md 5.24 records it
    and, on the same inputs, the ratio of torch's unfused graph on the device, which is printed and not asserted);
(d) a (b, h) launched alone gives the bits it has inside the batch;
(e) codes are K.fake_quant of the launch's own fp32 output; (f) non-finite inputs; (g) the small ViT with all three flags."""
import functools

import pytest
import torch

from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import AttentionLayer, fuse_inference
from test_gpu_gate import DEV, bits, tagged
from test_gpu_layernorm import own_codes, quantisers

pytestmark = pytest.mark.gpu
SHAPES = [(2, 3, 197, 197, 64), (3, 2, 17, 17, 32), (1, 1, 65, 65, 64), (2, 2, 50, 77, 32)]      # (B, H, Tq, Tk, D)
U = 2.0 ** -24


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def unmerge(out, h):
    """[B, Tq, H D] -> [B, H, Tq, D]"""
    b, t, c = out.shape
    return out.reshape(b, t, h, c // h).permute(0, 2, 1, 3)


# ------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_exact_placement(shape):
    b, h, tq, tk, d = shape
    scale = f32(d ** -0.5)
    nbits = 9
    j = torch.arange(tk)
    code = torch.zeros(tk, d)
    for bit in range(nbits):      # key j: +-1 in dimension `bit` (spread over the row: 7 bit mod d), 0 elsewhere
        code[:, (7 * bit + 3) % d] = ((j >> bit) & 1).float() * 2 - 1
    pi = (7 * torch.arange(tq)[None, None, :] + 3 + 5 * torch.arange(h)[None, :, None] + 11 * torch.arange(b)[:, None, None]) % tk
    k = code.expand(b, h, tk, d).contiguous()
    q = 512.0 * code[pi]                                   # q_i = 512 k_pi(i): score 512 scale (9 - 2 hamming(pi(i), j))
    s = scale * (q.double() @ k.double().transpose(-1, -2))
    top = s.topk(2, dim=-1).values
    assert bool((top[..., 0] - top[..., 1] > 110).all()) and bool((s.argmax(-1) == pi).all())
    v = ((((torch.arange(b)[:, None, None, None] * h + torch.arange(h)[None, :, None, None]) * tk + j[None, None, :, None]) * d
          + torch.arange(d)[None, None, None, :]) + 1).float()
    assert float(v.max()) < 2 ** 24 and v.unique().numel() == v.numel()
    want = torch.gather(v, 2, pi[..., None].expand(b, h, tq, d))
    out, _ = K.attention_quant(q.to(DEV), k.to(DEV), v.to(DEV), scale)
    got = unmerge(out, h).cpu()
    assert torch.equal(bits(got), bits(want)), f"{int((got != want).sum())} of {want.numel()} elements are not the selected v"


# ------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("t", [1, 2, 31, 32, 33, 63, 64, 65, 197, 257])
def test_tail_masking(t):
    d, c = 64, 1.7
    g = torch.Generator().manual_seed(t)
    parents = [torch.full((1, 2, t + 2, d), float("nan"), device=DEV) for _ in range(3)]
    q, k, v = (p[:, :, 1:t + 1] for p in parents)
    q.zero_()
    k.copy_(torch.randn(1, 2, t, d, generator=g))
    v.fill_(c)
    out, _ = K.attention_quant(q, k, v, 0.125)
    assert bool(torch.isfinite(out).all())
    ulp = 2.0 ** -23 * 1.0      # (1.7 lies in [1, 2))
    assert float((out.double() - f32(c)).abs().max()) <= 2 * ulp


# ------------------------------------------------------------------------------------------- (c)
def bound(q, k, v, scale):
    """(o*, bound) in float64 from fp32 tensors on the CPU."""
    q, k, v = q.double(), k.double(), v.double()
    d, tk = q.shape[-1], k.shape[-2]
    p = torch.softmax(scale * (q @ k.transpose(-1, -2)), dim=-1)
    delta = (d + 1) * U * abs(scale) * (q.abs() @ k.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    nb = (tk + 31) // 32
    kappa = 2 * (104 + 2 + 3 * nb + 32 * nb) + 1
    return p @ v, (2 * delta + kappa * U) * (p @ v.abs()) + 2.0 ** -126 * v.abs().amax(-2, keepdim=True)


FAMILIES = ("n01", "peaky", "constant_rows", "negative_outlier")
LAYOUTS = ("packed_vit", "packed_chunk", "contiguous")


@functools.lru_cache(maxsize=None)
def case(shape, family, layout):
    """(q, k, v) views on the device, made once, shared, never written."""
    b, h, tq, tk, d = shape
    g = torch.Generator().manual_seed(sum(shape) + 100 * FAMILIES.index(family))
    t = max(tq, tk)
    qkv = torch.randn(b, t, 3 * h * d, generator=g)
    a = qkv.view(b, t, 3, h, d)
    if family == "peaky":
        a[:, :, 0] *= 30.0
    elif family == "constant_rows":
        a[:, :, 0] = 0.5
        a[:, :, 1] = 0.25
    elif family == "negative_outlier":
        a[:, :, 0] = a[:, :, 0].abs()
        a[:, t // 2, 1] = -20.0
    qkv = qkv.to(DEV)
    if layout == "packed_chunk":      # the chunk(3, -1) spelling reads the row as [3][H][D] too
        q, k, v = (c.reshape(b, t, h, d).permute(0, 2, 1, 3) for c in qkv.chunk(3, dim=-1))
    else:
        p = qkv.reshape(b, t, 3, h, d).permute(2, 0, 3, 1, 4)
        q, k, v = p[0], p[1], p[2]
    q, k, v = q[:, :, :tq], k[:, :, :tk], v[:, :, :tk]
    if layout == "contiguous":
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    return q, k, v


def check_bound(out_bhtd, q, k, v, scale, what):
    ref, bnd = bound(q.cpu(), k.cpu(), v.cpu(), scale)
    err = (out_bhtd.cpu().double() - ref).abs()
    ratio = float((err / bnd.clamp_min(1e-300)).max())
    print(f"{what}: max |out - o*| / bound = {ratio:.4f}")
    return ratio, bool((err <= bnd).all())


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_accuracy(shape, family):
    b, h, tq, tk, d = shape
    scale = f32(d ** -0.5)
    first = None
    for layout in LAYOUTS:
        q, k, v = case(shape, family, layout)
        if layout != "contiguous":
            assert not q.is_contiguous()
        out, _ = K.attention_quant(q, k, v, scale)
        ratio, ok = check_bound(unmerge(out, h), q, k, v, scale, f"{shape} {family} {layout}")
        assert ok, f"{layout}: {ratio:.4f} of the bound"
        first = out if first is None else first
        assert torch.equal(bits(out), bits(first)), f"{layout}: other bits than {LAYOUTS[0]}"      # (the layout is addressing only)
    with torch.no_grad():
        unfused = torch.matmul(torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * scale, dim=-1), v)
    check_bound(unfused, q, k, v, scale, f"{shape} {family} torch's unfused graph on the device (not asserted)")


# ------------------------------------------------------------------------------------------- (d)
def test_one_head_alone_gives_the_same_bits():
    shape = SHAPES[0]
    b, h, tq, tk, d = shape
    q, k, v = case(shape, "n01", "packed_vit")
    full = unmerge(K.attention_quant(q, k, v, 0.125)[0], h)
    for bi, hi in ((0, 0), (1, 2), (0, 1)):
        alone = K.attention_quant(q[bi:bi + 1, hi:hi + 1], k[bi:bi + 1, hi:hi + 1], v[bi:bi + 1, hi:hi + 1], 0.125)[0]
        assert torch.equal(bits(unmerge(alone, 1)[0, 0]), bits(full[bi, hi])), (bi, hi)


# ------------------------------------------------------------------------------------------- (e)
@pytest.mark.parametrize("name", sorted(["fsptq_zeropoint_u8", "qbase_s8", "qbase_s8_g", "qbase_u8", "qbase_u8_g"]))
def test_codes_are_fake_quant_of_the_own_output(name):
    sc, z, lo, hi, form, gq = qz = quantisers()[name]
    for shape in SHAPES[:2]:
        b, h, tq, tk, d = shape
        q, k, v = case(shape, "n01", "packed_vit")
        em = lambda: K.EmitCodes(sc, z, lo, hi, form, gq)  # noqa: E731
        plain = K.attention_quant(q, k, v, 0.125)[0]
        out, codes = K.attention_quant(q, k, v, 0.125, emit=em())
        assert tuple(out.shape) == tuple(codes.shape) == (b, tq, h * d) and torch.equal(bits(out), bits(plain))
        want = own_codes(out, qz)
        assert torch.equal(codes.view(torch.uint8), want), f"{int((codes.view(torch.uint8) != want).sum())} code bytes differ"
        none, only = K.attention_quant(q, k, v, 0.125, emit=em(), want_out=False)
        assert none is None and torch.equal(only, codes)
        o4, c4 = K.attention_quant(q, k, v, 0.125, emit=em(), merged=False)
        assert tuple(o4.shape) == (b, h, tq, d) and torch.equal(bits(o4), bits(unmerge(out, h))) and torch.equal(c4, unmerge(codes, h))


# ------------------------------------------------------------------------------------------- (f)
def _torch_graph(q, k, v, scale):
    return torch.matmul(torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * scale, dim=-1), v)


@pytest.mark.parametrize("where", ["q_row", "k_row", "v_element", "inf_score"])
def test_non_finite_inputs(where):
    """The NaNs of torch's unfused graph, element for element: a NaN in q_i - row i alone; in k_j - every row of the head; in
    v_j[c] - column c of every row of the head, the other columns finite; a +inf score - its row."""
    shape = SHAPES[0]
    b, h, tq, tk, d = shape
    q, k, v = (t.clone() for t in case(shape, "n01", "contiguous"))
    nan = torch.zeros(b, h, tq, d, dtype=torch.bool)
    if where == "q_row":
        q[1, 2, 70, 5] = float("nan")
        nan[1, 2, 70] = True
    elif where == "k_row":
        k[0, 1, 130, 9] = float("nan")
        nan[0, 1] = True
    elif where == "v_element":
        v[1, 0, 196, 33] = float("nan")
        nan[1, 0, :, 33] = True
    else:
        q[0, 0, 3] = 0.0
        q[0, 0, 3, 0] = 1.0
        k[0, 0, 100, 0] = float("inf")      # s[0, 0, 3, 100] = +inf and nothing else of that row is non-finite
        nan[0, 0] = (q[0, 0, :, 0] >= 0).cpu()[:, None]      # +inf for every query with a positive first element (0 * inf: NaN)
        assert bool(nan[0, 0, 3].all()) and bool((q[0, 0, :, 0] < 0).any())      # -inf scores: p = 0, those rows stay finite
    ref = _torch_graph(q, k, v, 0.125).isnan().cpu()
    assert torch.equal(ref, nan), "the test's own expectation is not torch's"
    out = unmerge(K.attention_quant(q, k, v, 0.125)[0], h).cpu()
    assert torch.equal(out.isnan(), nan)
    assert bool(torch.isfinite(out[~nan]).all())


# ------------------------------------------------------------------------------------------- (g)
@pytest.mark.parametrize("tag", ["fsptq", "qbase"])
def test_small_vit(tag):
    from test_gpu_transformer import DEPTH, calibrated
    net, x = calibrated(tag)
    off = fuse_inference(net, layer_norms=True, gelu=True)
    on = fuse_inference(net, layer_norms=True, gelu=True, attention=True)
    rn = on.fusion_report
    assert rn.attentions == DEPTH and off.fusion_report.attentions == 0
    assert (rn.layer_norms, rn.gelus, rn.layers) == (off.fusion_report.layer_norms, off.fusion_report.gelus, off.fusion_report.layers)
    layers = {n_: m for n_, m in on.named_modules() if isinstance(m, AttentionLayer)}
    assert len(layers) == DEPTH and all(m.merged and m.emit is not None and not m.want_out for m in layers.values())
    seen = {}
    for n_, m in layers.items():
        m.want_out = True      # (for the check below: the fp32 values of the same launch; nobody reads them)
    hooks = [m.register_forward_hook(lambda mod, a, r, n_=n_: seen.__setitem__(n_, (a, r))) for n_, m in layers.items()]
    with torch.no_grad():
        (a, tags_off), (bb, tags_on) = tagged(lambda: off(x)), tagged(lambda: on(x))
    for hk in hooks:
        hk.remove()
    assert tags_on.count("attention") == DEPTH and "attention" not in tags_off
    assert tags_off.count("fq_tensor") - tags_on.count("fq_tensor") == DEPTH      # to_out's own quantise passes are gone
    assert sorted(seen) == sorted(layers)
    for n_, (args, (out, codes)) in seen.items():
        q, k, v = args[:3]
        m = layers[n_]
        assert tuple(out.shape) == (3, 17, 64) and codes.dtype in (torch.uint8, torch.int8)
        ratio, ok = check_bound(unmerge(out, 2), q, k, v, m.scale, f"{tag} {n_}")
        assert ok, ratio
        e = m.emit
        want = K.fake_quant(out, e.scale, e.zp, e.lo, e.hi, e.form, g=e.g(q.numel()), codes="i8", want_y=False)[1]
        assert torch.equal(codes.view(torch.uint8), want.view(torch.uint8))
    assert tuple(bb.shape) == (3, 10) and bool(torch.isfinite(bb).all())
    print(f"{tag}: {int((a != bb).sum())} of {a.numel()} logits differ from the attention-off plan, max |delta| = {float((a - bb).abs().max()):.3e} "
          f"at max |logit| = {float(a.abs().max()):.3e}")
