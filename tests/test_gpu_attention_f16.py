"""Attention on the f16 matrix cores (include/dlmcq.h: dlmcq_attention_f16; K.attention_quant(operands="f16");
fuse_inference(attention="f16")), against float64 on the same fp32 inputs.  Shapes (B, H, Tq, Tk, D): one token; a partial second query
tile and key block; Tq != Tk with a partial third key block; a second workgroup per head with idle waves, the wave rotation over 5
heads; ViT's T.  Dense tensors, and the three slices of a packed [B, T, 3, H, D] projection where Tq = Tk.
The bound (csrc/attention_f16.hip derives it), e = 2^-11, u = 2^-24, nb = ceil(Tk / 32), kappa = 2 (104 + 2 + 3 nb + 68 nb) + 1:
    delta_i = ((2 e + e^2) + (2 D + 3) u) |scale| max_j sum_k |q_ik k_jk|,   rho_i = expm1(2 delta_i + 3 e + 2^-20 + kappa u)
    |out_ic - o*_ic| <= rho_i sum_j p*_ij |v_jc| + Tk 2^-24 max_j |v_jc| + 2^-25"""
import functools

import pytest
import torch

from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import AttentionLayer, fuse_inference
from test_gpu_gate import DEV, bits, tagged
from test_gpu_layernorm import own_codes, quantisers

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 1, 1, 64), (1, 2, 33, 33, 32), (2, 2, 50, 77, 32), (1, 5, 129, 65, 64), (2, 3, 197, 197, 64)]
LAYOUTS = ("dense", "packed")
E, U = 2.0 ** -11, 2.0 ** -24


def place(q, k, v, layout):
    """fp32 CPU tensors [B, H, T, D] on the device: dense, or as the slices of one packed [B, T, 3, H, D] projection (Tq = Tk)."""
    if layout == "dense" or q.shape[2] != k.shape[2]:
        return q.to(DEV), k.to(DEV), v.to(DEV)
    p = torch.stack([t.permute(0, 2, 1, 3) for t in (q, k, v)], dim=2).contiguous().to(DEV).permute(2, 0, 3, 1, 4)
    return p[0], p[1], p[2]


def f16(q, k, v, scale, **kw):
    """The kernel's (out [B, H, Tq, D] on the CPU, codes)."""
    out, codes = K.attention_quant(q, k, v, scale, operands="f16", merged=False, **kw)
    return (None if out is None else out.cpu()), codes


def integers(b, h, t, d):
    """v[b, h, j, c]: integers of magnitude at most 1024, distinct over j for every (b, h, c) (7 is prime to 2049)."""
    i = [torch.arange(n).reshape([-1 if a == x else 1 for a in range(4)]) for x, n in enumerate((b, h, t, d))]
    return ((3 * i[0] + 5 * i[1] + 7 * i[2] + 13 * i[3]) % 2049 - 1024).float()


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_lane_and_key_maps(shape, layout):
    b, h, tq, tk, d = shape
    scale = 16.0      # (a key at distance D / 8 is exp(-4 D) behind: its p is f16 zero, and a block's rescale by it is fp32 zero)
    j = torch.arange(tk)
    code = torch.stack([((j >> (c % 8)) & 1).float() * 2 - 1 for c in range(d)], dim=1)      # bit c % 8 of j: distance >= D / 8
    pi = (7 * torch.arange(tq)[None, None, :] + 3 + 5 * torch.arange(h)[None, :, None] + 11 * torch.arange(b)[:, None, None]) % tk
    k, q, v = code.expand(b, h, tk, d).contiguous(), code[pi], integers(b, h, tk, d)
    s = scale * (q.double() @ k.double().transpose(-1, -2))
    top = s.topk(min(2, tk), dim=-1).values
    assert bool((s.argmax(-1) == pi).all())      # the maximum is unique and where it should be ...
    assert tk == 1 or bool((torch.exp(top[..., 1] - top[..., 0]) < 2.0 ** -25).all())      # ... every other p rounds to f16 zero ...
    assert tk == 1 or bool((top[..., 1] - top[..., 0] < -150 * 0.6932).all())      # ... and a block that met only such keys is rescaled by 0
    want = torch.gather(v, 2, pi[..., None].expand(b, h, tq, d))
    got, _ = f16(*place(q, k, v, layout), scale)
    assert torch.equal(bits(got), bits(want)), f"{int((got != want).sum())} of {want.numel()} elements are not the selected v"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_uniform_rows(shape, layout):
    b, h, tq, tk, d = shape
    v = integers(b, h, tk, d)
    want = (v.sum(2, keepdim=True) / torch.tensor(float(tk))).expand(b, h, tq, d)      # exact integer sums, one IEEE division
    got, _ = f16(*place(torch.zeros(b, h, tq, d), torch.randn(b, h, tk, d), v, layout), d ** -0.5)
    assert torch.equal(bits(got), bits(want.contiguous())), f"{int((got != want).sum())} of {want.numel()} elements differ"


def bound(q, k, v, scale):
    """(o*, bound) in float64 from fp32 tensors on the CPU."""
    q, k, v = q.double(), k.double(), v.double()
    d, tk = q.shape[-1], k.shape[-2]
    p = torch.softmax(scale * (q @ k.transpose(-1, -2)), dim=-1)
    delta = ((2 * E + E * E) + (2 * d + 3) * U) * abs(scale) * (q.abs() @ k.abs().transpose(-1, -2)).amax(-1, keepdim=True)
    nb = (tk + 31) // 32
    rho = torch.expm1(2 * delta + 3 * E + 2.0 ** -20 + (2 * (104 + 2 + 3 * nb + 68 * nb) + 1) * U)
    return p @ v, rho * (p @ v.abs()) + tk * 2.0 ** -24 * v.abs().amax(-2, keepdim=True) + 2.0 ** -25


def check_bound(out, q, k, v, scale, what):
    ref, bnd = bound(q.cpu(), k.cpu(), v.cpu(), scale)
    err = (out.cpu().double() - ref).abs()
    ratio = float((err / bnd).max())
    print(f"{what}: max |out - o*| / bound = {ratio:.4f}")
    assert bool((err <= bnd).all()), f"{what}: {ratio:.4f} of the bound"


@functools.lru_cache(maxsize=None)
def case(shape, family, layout):
    """(q, k, v) on the device: N(0, 1), `peaky` with q scaled by 4.  Made once, shared, never written."""
    b, h, tq, tk, d = shape
    g = torch.Generator().manual_seed(sum(shape) + (family == "peaky"))
    q, k, v = (torch.randn(b, h, t, d, generator=g) for t in (tq, tk, tk))
    return place(q * 4 if family == "peaky" else q, k, v, layout)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("family", ["n01", "peaky"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_bound(shape, family, layout):
    q, k, v = case(shape, family, layout)
    check_bound(f16(q, k, v, shape[-1] ** -0.5)[0], q, k, v, shape[-1] ** -0.5, f"{shape} {family} {layout}")


@pytest.mark.parametrize("name", ["fsptq_zeropoint_u8", "qbase_s8_g"])
def test_outputs(name):
    sc, z, lo, hi, form, gq = qz = quantisers()[name]
    b, h, tq, tk, d = shape = SHAPES[1]      # a partial query tile
    q, k, v = case(shape, "n01", "packed")
    plain = K.attention_quant(q, k, v, 0.25, operands="f16")[0]
    out, codes = K.attention_quant(q, k, v, 0.25, operands="f16", emit=K.EmitCodes(sc, z, lo, hi, form, gq))
    assert tuple(out.shape) == tuple(codes.shape) == (b, tq, h * d) and torch.equal(bits(out), bits(plain))
    assert torch.equal(codes.view(torch.uint8), own_codes(out, qz))
    none, only = K.attention_quant(q, k, v, 0.25, operands="f16", emit=K.EmitCodes(sc, z, lo, hi, form, gq), want_out=False)
    assert none is None and torch.equal(only, codes)
    # the entry point itself, out and codes as strided views into filled parents: every byte outside the views stays
    w = h * d + 8
    po = torch.full((b, tq + 2, w), float("nan"), device=DEV)
    pc = torch.full((b, tq + 2, w), 0xa5, dtype=torch.uint8, device=DEV)
    vo, vc = po[:, 1:tq + 1, 4:4 + h * d], pc[:, 1:tq + 1, 4:4 + h * d]
    rc = N.lib.dlmcq_attention_f16(N.ptr(q), N.ptr(k), N.ptr(v), vo.data_ptr(), vc.data_ptr(), b, h, tq, tk, d, *q.stride()[:3], *k.stride()[:3],
                                   *v.stride()[:3], (tq + 2) * w, d, w, 0.25, N.ptr(sc), N.ptr(z), lo, hi, form, gq, N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(bits(vo), bits(out)) and torch.equal(vc, codes.view(torch.uint8))
    inside = torch.zeros_like(pc, dtype=torch.bool)
    inside[:, 1:tq + 1, 4:4 + h * d] = True
    assert bool(po[~inside].isnan().all()) and bool((pc[~inside] == 0xa5).all())


@pytest.mark.parametrize("which", ["q", "v"])
def test_range(which):
    """An element above f16's 65504: its query row (q) or its channel of the head (v) is non-finite, everything else keeps its bits."""
    shape = SHAPES[2]
    q, k, v = (t.clone() for t in case(shape, "n01", "dense"))
    before, _ = f16(q, k, v, 0.25)
    (q if which == "q" else v)[1, 0, 40, 9] = 1e5
    after, _ = f16(q, k, v, 0.25)
    hit = torch.zeros(before.shape, dtype=torch.bool)
    if which == "q":
        hit[1, 0, 40] = True
    else:
        hit[1, 0, :, 9] = True
    assert bool(torch.isfinite(before).all()) and not bool(torch.isfinite(after[hit]).any())
    assert torch.equal(bits(after[~hit]), bits(before[~hit]))


@pytest.mark.parametrize("tag", ["fsptq", "qbase"])
def test_small_vit(tag):
    from test_gpu_transformer import DEPTH, calibrated
    net, x = calibrated(tag)
    f32_plan = fuse_inference(net, layer_norms=True, gelu=True, attention=True)
    on = fuse_inference(net, layer_norms=True, gelu=True, attention="f16")
    assert on.fusion_report.attentions == f32_plan.fusion_report.attentions == DEPTH
    assert (on.fusion_report.attention_operands, f32_plan.fusion_report.attention_operands) == ("f16", "f32")
    assert "attention operands=f16" in repr(on.fusion_report)
    layers = {n_: m for n_, m in on.named_modules() if isinstance(m, AttentionLayer)}
    assert len(layers) == DEPTH and all(m.operands == "f16" and m.emit is not None for m in layers.values())
    seen = {}
    for n_, m in layers.items():
        m.want_out = True      # (the fp32 values of the same launch, for the checks below; nobody reads them)
        m.register_forward_hook(lambda mod, a, r, n_=n_: seen.__setitem__(n_, (a, r)))
    with torch.no_grad():
        logits, tags = tagged(lambda: on(x))
    assert tags.count("attention_f16") == DEPTH and "attention" not in tags and bool(torch.isfinite(logits).all())
    for n_, (args, (out, codes)) in sorted(seen.items()):
        q, k, v = args[:3]
        m = layers[n_]
        check_bound(out.reshape(3, 17, 2, 32).permute(0, 2, 1, 3), q, k, v, m.scale, f"{tag} {n_}")
        e = m.emit
        want = K.fake_quant(out, e.scale, e.zp, e.lo, e.hi, e.form, g=e.g(q.numel()), codes="i8", want_y=False)[1]
        assert torch.equal(codes.view(torch.uint8), want.view(torch.uint8))
