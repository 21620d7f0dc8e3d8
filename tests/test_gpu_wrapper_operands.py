"""The operand marshalling of the int8 convolution wrappers (dlmc/quantization/scalar/kernels.py): every wrapper called twice - with its
operands in canonical form (flat fp32 [1] / [K] tensors, channels_last codes, contiguous bias) and in the loose forms the wrappers
absorb - must return the same bytes.  Shapes: the smallest at which each kernel still has a partial tile and two channel chunks.

Loose forms, each only where the wrapper has always taken it: 0-d scales with requires_grad, a Python-float zero point, a one-entry
`w_scale` against its [K] expansion, NCHW-contiguous codes (and residual), a non-contiguous bias view.  Left out because the wrappers
refuse them (or hand the kernel a short array): Python-number SCALES, and a one-entry per-channel scale for the depthwise layer
(conv2d_dw_i8, dwpw_table: their `w_scale` is passed as given, [C] entries)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ZP = 3.0


def _mods():
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    return N, K


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _codes(g, *shape):
    x = torch.randint(0, 256, shape, generator=g, device=DEV, dtype=torch.uint8)
    return x.contiguous(memory_format=torch.channels_last) if len(shape) == 4 else x


def _weights(g, k, r, c):
    wq = torch.randint(-127, 128, (k, r, r, c), generator=g, device=DEV, dtype=torch.int8)
    return wq, wq.to(torch.int32).sum(dim=(1, 2, 3)).to(torch.int32).contiguous()


def _layer(g, k, r, c, w_scale):
    wq, wsum = _weights(g, k, r, c)
    return dict(wq=wq, wsum=wsum, bias=torch.randn(k, generator=g, device=DEV), w_scale=torch.full((k,), w_scale, device=DEV))


def _operand(g, n, c, h, k, r=1, **conv):
    return dict(_layer(g, k, r, c, 0.003), codes=_codes(g, n, c, h, h), in_scale=torch.full((1,), 0.02, device=DEV),
                in_zp=torch.full((1,), ZP, device=DEV), **conv)


def _scalar(t):
    """[1] -> the same value 0-d, asking for a gradient."""
    return t.detach().reshape(()).clone().requires_grad_()


def _strided(b):
    """The same values as a non-contiguous view."""
    v = torch.stack((b, -b), dim=1)[:, 0]
    assert not v.is_contiguous()
    return v


def _nchw(x):
    """The same values in NCHW-contiguous memory."""
    y = x.contiguous()
    assert x.dim() != 4 or not y.is_contiguous(memory_format=torch.channels_last)
    return y


def _loose(d):
    """An operand / layer dict in the loose forms (a uniform [K] `w_scale` as one entry)."""
    out = dict(d, bias=_strided(d["bias"]), w_scale=d["w_scale"][:1].clone().requires_grad_())
    assert bool((d["w_scale"] == d["w_scale"][0]).all())
    if "codes" in d:
        out.update(codes=_nchw(d["codes"]), in_zp=float(d["in_zp"]))
    if "in_scale" in d:
        out["in_scale"] = _scalar(d["in_scale"])
    return out


def _emits(K, N, scale, zp):
    """The same quantiser, canonical and loose."""
    return (K.EmitCodes(torch.full((1,), scale, device=DEV), torch.full((1,), zp, device=DEV), 0, 255, N.FORM_ZEROPOINT),
            K.EmitCodes(torch.tensor(scale, device=DEV, requires_grad=True), zp, 0, 255, N.FORM_ZEROPOINT))


def _same(got, want):
    _, K = _mods()
    got, want = (got, want) if isinstance(got, tuple) else ((got,), (want,))
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        if a is None or b is None:
            assert a is None and b is None, i
            continue
        assert type(a) is type(b), i
        if isinstance(a, K.ChunkMajor):
            a, b = a.to_nhwc(), b.to_nhwc()
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), f"result {i} differs"


def test_conv2d_i8():
    N, K = _mods()
    g = _gen(11)
    o = _operand(g, 2, 64, 5, 128, r=3)
    lo = _loose(o)
    e, le = _emits(K, N, 0.05, 2.0)

    def run(t, emit):
        return K.conv2d_i8(t["codes"], t["wq"], t["wsum"], t["bias"], t["in_scale"], t["in_zp"], t["w_scale"], padding=1, relu=True, emit=emit)
    _same(run(lo, le), run(o, e))


def test_conv2d_i8_linear():
    _, K = _mods()
    g = _gen(12)
    o = dict(_layer(g, 64, 1, 64, 0.002), codes=_codes(g, 3, 64), in_scale=torch.full((1,), 0.02, device=DEV),
             in_zp=torch.full((1,), ZP, device=DEV))
    lo = dict(_loose(o), codes=o["codes"].t().contiguous().t())

    def run(t):
        return K.conv2d_i8(t["codes"], t["wq"], t["wsum"], t["bias"], t["in_scale"], t["in_zp"], t["w_scale"])
    assert not lo["codes"].is_contiguous()
    _same(run(lo), run(o))


def test_conv2d_dw_i8():
    N, K = _mods()
    g = _gen(13)
    c = 16
    codes = _codes(g, 2, c, 5, 5)
    wq = torch.randint(-127, 128, (3, 3, c), generator=g, device=DEV, dtype=torch.int8)
    bias, w_scale = torch.randn(c, generator=g, device=DEV), torch.rand(c, generator=g, device=DEV) * 0.004 + 0.001
    s_in, zp = torch.full((1,), 0.02, device=DEV), torch.full((1,), ZP, device=DEV)
    e, le = _emits(K, N, 0.05, 2.0)
    want = K.conv2d_dw_i8(codes, wq, bias, s_in, zp, w_scale, padding=1, relu=True, emit=e)
    got = K.conv2d_dw_i8(_nchw(codes), wq, _strided(bias), _scalar(s_in), ZP, w_scale.clone().requires_grad_(), padding=1, relu=True, emit=le)
    _same(got, want)


@pytest.mark.parametrize("out_cm", [False, True])
def test_conv2d_i8_dual(out_cm):
    N, K = _mods()
    g = _gen(14)
    a, b = _operand(g, 2, 64, 5, 128), _operand(g, 2, 64, 10, 128, stride=2)
    e, le = _emits(K, N, 0.07, 4.0)
    _same(K.conv2d_i8_dual(_loose(a), _loose(b), relu=True, emit=le, out_chunk_major=out_cm),
          K.conv2d_i8_dual(a, b, relu=True, emit=e, out_chunk_major=out_cm))


@pytest.mark.parametrize("out_cm", [False, True])
def test_conv2d_i8_chain(out_cm):
    N, K = _mods()
    g = _gen(15)
    a, b = _operand(g, 2, 64, 5, 128), _layer(g, 64, 1, 128, 0.001)          # M = 50 rows: a partial 64-row tile
    assert K.chain_supported(64, 128, 64, 50)
    res = (torch.randn(2, 128, 5, 5, generator=g, device=DEV) * 2).contiguous(memory_format=torch.channels_last)
    (e, le), (e2, le2) = _emits(K, N, 0.05, 2.0), _emits(K, N, 0.11, 0.0)
    kw = dict(want_out=True, want_codes=True, out_chunk_major=out_cm)
    _same(K.conv2d_i8_chain(_loose(a), _loose(b), _nchw(res), emit=le, emit2=le2, **kw), K.conv2d_i8_chain(a, b, res, emit=e, emit2=e2, **kw))


def test_conv2d_i8_dual_chain():
    N, K = _mods()
    g = _gen(16)
    a, b, c3 = _operand(g, 2, 64, 5, 128), _operand(g, 2, 64, 10, 128, stride=2), _layer(g, 64, 1, 128, 0.001)
    assert K.dual_chain_supported(64, 64, 128, 64, 50)
    (e, le), (e3, le3) = _emits(K, N, 0.07, 4.0), _emits(K, N, 0.13, 0.0)
    kw = dict(want_out=True, want_codes=True)
    _same(K.conv2d_i8_dual_chain(_loose(a), _loose(b), _loose(c3), emit=le, emit3=le3, **kw),
          K.conv2d_i8_dual_chain(a, b, c3, emit=e, emit3=e3, **kw))


def test_conv2d_i8_recompute_chain():
    N, K = _mods()
    g = _gen(19)
    a, b = _operand(g, 2, 64, 5, 128), _layer(g, 64, 1, 128, 0.001)          # M = 50 rows: a partial 64-row tile, two chunks
    pa, pb = _operand(g, 2, 64, 5, 128), _operand(g, 2, 64, 10, 128, stride=2)
    assert K.recompute_chain_supported(64, 64, 64, 128, 64, 50)

    def emits(scale):     # the recomputing form takes the plain quantiser alone: [0, 255], zero point 0 passed as none
        return (K.EmitCodes(torch.full((1,), scale, device=DEV), None, 0, 255, N.FORM_ZEROPOINT),
                K.EmitCodes(torch.tensor(scale, device=DEV, requires_grad=True), None, 0, 255, N.FORM_ZEROPOINT))
    (e, le), (e2, le2) = emits(0.05), emits(0.11)
    kw = dict(want_out=True, want_codes=True)
    _same(K.conv2d_i8_recompute_chain(_loose(a), _loose(b), _loose(pa), _loose(pb), emit=le, emit2=le2, **kw),
          K.conv2d_i8_recompute_chain(a, b, pa, pb, emit=e, emit2=e2, **kw))


@pytest.mark.parametrize("pool", [False, True])
def test_conv2d_i8_stem(pool):
    N, K = _mods()
    g = _gen(17)
    k = 64
    x = torch.randn(2, 3, 18, 18, generator=g, device=DEV)
    s_in, zp = torch.full((1,), 0.03, device=DEV), torch.full((1,), 120.0, device=DEV)
    xpad = K.quantize_pad_nhwc4(x, s_in, zp, 0, 255, N.FORM_ZEROPOINT, 3)
    s_w = torch.full((k,), 0.004, device=DEV)
    wq, wsum = K.quantize_weight_stem(torch.randn(k, 3, 7, 7, generator=g, device=DEV) * 0.2, s_w, -127, 127)
    bias = torch.randn(k, generator=g, device=DEV)
    e, le = _emits(K, N, 0.05, 2.0)
    want = K.conv2d_i8_stem(xpad, wq, wsum, bias, s_in, zp, s_w, 7, stride=2, relu=True, emit=e, pool=pool)
    got = K.conv2d_i8_stem(xpad, wq, wsum, _strided(bias), _scalar(s_in), 120.0, s_w[:1].clone().requires_grad_(), 7, stride=2, relu=True,
                           emit=le, pool=pool)
    assert want[0].shape == ((2, k, 5, 5) if pool else (2, k, 9, 9))
    _same(got, want)


def test_dwpw_table_and_conv2d_dwpw_i8():
    N, K = _mods()
    g = _gen(18)
    c, k = 64, 128
    assert K.dwpw_supported(c, k, 5, 5, 1, 1, 3)
    codes = _codes(g, 2, c, 5, 5)
    wq = torch.randint(-127, 128, (3, 3, c), generator=g, device=DEV, dtype=torch.int8)
    bias, w_scale = torch.randn(c, generator=g, device=DEV), torch.rand(c, generator=g, device=DEV) * 0.004 + 0.001
    s_in, zp = torch.full((1,), 0.02, device=DEV), torch.full((1,), ZP, device=DEV)
    table = K.dwpw_table(wq, bias, s_in, zp, w_scale, None)
    loose_table = K.dwpw_table(wq, _strided(bias), _scalar(s_in), ZP, w_scale.clone().requires_grad_(), None)
    _same(loose_table, table)
    (e, le), (e2, le2) = _emits(K, N, 0.05, 2.0), _emits(K, N, 0.11, 0.0)
    pw = dict(_layer(g, k, 1, c, 0.002), in_scale=e.scale)
    want = K.conv2d_dwpw_i8(codes, table, False, True, True, zp, e, pw, emit2=e2)
    _same(K.conv2d_dwpw_i8(_nchw(codes), table, False, True, True, ZP, le, _loose(pw), emit2=le2), want)
