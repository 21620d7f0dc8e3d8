"""The squeeze kernel on the GPU (include/dlmcq.h: dlmcq_squeeze_gate_i8; K.squeeze_gate).

Part 1: `hidden` and `gate` with gate_fn = none are torch.equal to K.squeeze_gate_torch - the restatement out of K.conv2d_i8 and
        K.fake_quant, the kernels that were there before - for every inner activation, uint8 and int8 input codes and the four quantiser
        forms with a non-zero integer zero point, at the widths of the squeeze-excite networks, the kernel's limits and batch sizes
        around its images-per-workgroup constant.
Part 2: sigmoid against float64 of the kernel's own gate_fn = none output: |g - g*| <= 4 * 2^-24 |g*| + 2^-126 (one ulp of expf, then
        the roundings of 1 + e and of 1 / d); the largest ratio is printed.  MATCHES_TORCH_SIGMOID states whether it
        equals torch.sigmoid on the device.  Hard sigmoid is torch.equal to F.relu6(v + 3) / 6 on the device, -3, 3, -0, NaN, +-inf included.
Part 3: one exact family - dyadic scales, full-range codes, both integer sums below 2^24 (asserted) - against a float64 reference
        computed from the integers; the hidden codes recovered through an identity second layer.
Part 4: outputs written as views into pattern-filled parents keep their surroundings; gate alone and hidden alone."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G = N.SQUEEZE_IMAGES
MATCHES_TORCH_SIGMOID = True      # as measured on an MI355X: 0 elements of Part 2's inputs differ in their bits from torch.sigmoid(v)
SHAPES = [(1, 4, 1), (3, 32, 8), (5, 96, 4), (7, 144, 6), (9, 240, 10), (2, 1152, 48), (3, 960, 240), (2, 2048, 512),
          (G - 1, 48, 12), (G, 48, 12), (G + 1, 48, 12), (2 * G + 1, 48, 12)]
INNER = [None, "relu", "swish"]
WORST = {}
SIGMOID_BOUND = 4 * 2.0 ** -24      # Part 2's relative bound (+ 2^-126 absolute): shared with tests/test_gpu_squeeze_exact.py


def sigmoid_ratio(g, v):
    """The largest |g - g*| / (SIGMOID_BOUND |g*| + 2^-126) of a sigmoid output `g` against float64 g* = 1 / (1 + exp(-v))."""
    ref = 1.0 / (1.0 + torch.exp(-v.double()))
    return float(((g.double() - ref).abs() / (SIGMOID_BOUND * ref.abs() + 2.0 ** -126)).max())


def t(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


def quantisers():
    """The hidden quantiser in its four forms, each with a non-zero integer zero point: (scale, zero point, lo, hi, form, g)."""
    return {"emulate_u8": (t(0.031), t(2.0), 0, 255, N.FORM_EMULATE, 0.0), "qbase_s8": (t(0.027), t(-3.0), -128, 127, N.FORM_QBASE, 0.02),
            "zeropoint_u8": (t(0.033), t(7.0), 0, 255, N.FORM_ZEROPOINT, 0.0), "symmetric_s8": (t(0.029), t(5.0), -128, 127, N.FORM_SYMMETRIC, 0.0)}


def operands(n, c, r, unsigned, seed=0):
    """Random full-range codes and weights, scales that put the hidden values and the gate's argument at a few units."""
    g = torch.Generator(device="cpu").manual_seed(1000 * c + 10 * r + n + seed)
    codes = torch.randint(0, 256, (n, c), generator=g).to(torch.uint8 if unsigned else torch.int16)
    codes = codes if unsigned else (codes - 128).to(torch.int8)
    w1 = torch.randint(-127, 128, (r, c), generator=g).to(torch.int8)
    w2 = torch.randint(-127, 128, (c, r), generator=g).to(torch.int8)
    s_in = 0.02
    ws1 = (0.5 + torch.rand(r, generator=g)) * 3.0 / (s_in * 74 * 73 * c ** 0.5)
    ws2 = (0.5 + torch.rand(c, generator=g)) * 4.0 / (0.03 * 74 * 73 * r ** 0.5)
    l1 = dict(wq=w1.to(DEV), wsum=w1.sum(1, dtype=torch.int32).to(DEV), bias=(torch.randn(r, generator=g) * 0.5).to(DEV), in_scale=t(s_in),
              in_zp=t(3.0 if unsigned else -4.0), w_scale=ws1.to(DEV))
    l2 = dict(wq=w2.to(DEV), wsum=w2.sum(1, dtype=torch.int32).to(DEV), bias=(torch.randn(c, generator=g) * 0.5).to(DEV), w_scale=ws2.to(DEV))
    return codes.to(DEV), l1, l2


def emit_of(q):
    s, z, lo, hi, form, g = q
    return K.EmitCodes(s, z, lo, hi, form, g)


def same(a, b):
    """torch.equal that also takes NaN for NaN, and the sign of a zero."""
    if a.shape != b.shape or not bool((torch.isnan(a) == torch.isnan(b)).all()):
        return False
    a, b = torch.nan_to_num(a, nan=1.0), torch.nan_to_num(b, nan=1.0)      # (a NaN's sign and payload are not compared)
    return torch.equal(a, b) and torch.equal(torch.signbit(a), torch.signbit(b))


# ------------------------------------------------------------------------------------------- Part 1
@pytest.mark.parametrize("inner", INNER, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_hidden_and_gate_equal_the_restatement(shape, inner):
    n, c, r = shape
    for unsigned in (True, False):
        codes, l1, l2 = operands(n, c, r, unsigned)
        for name, q in quantisers().items():
            gate, hidden = K.squeeze_gate(codes, l1, inner, emit_of(q), l2, None, want_hidden=True)
            want_gate, want_hidden = K.squeeze_gate_torch(codes, l1, inner, emit_of(q), l2, None, want_hidden=True)
            assert gate.shape == (n, c) and hidden.shape == (n, r)
            assert torch.equal(hidden, want_hidden), (name, unsigned, int((hidden != want_hidden).sum()))
            assert torch.equal(gate, want_gate), (name, unsigned, int((gate != want_gate).sum()))
            assert float(gate.abs().max()) > 0      # (not a comparison of zeros)


# ------------------------------------------------------------------------------------------- Part 2
@pytest.mark.parametrize("inner", INNER, ids=lambda v: str(v))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sigmoid_bound_and_hard_sigmoid(shape, inner):
    n, c, r = shape
    differ = total = 0
    for unsigned in (True, False):
        codes, l1, l2 = operands(n, c, r, unsigned, seed=5)
        for name, q in quantisers().items():
            v = K.squeeze_gate(codes, l1, inner, emit_of(q), l2, None)[0]
            g = K.squeeze_gate(codes, l1, inner, emit_of(q), l2, "sigmoid")[0]
            ratio = sigmoid_ratio(g, v)
            WORST["sigmoid"] = max(WORST.get("sigmoid", 0.0), ratio)
            assert ratio <= 1.0, (name, unsigned, ratio)
            differ += int((g != torch.sigmoid(v)).sum())
            total += g.numel()
            hs = K.squeeze_gate(codes, l1, inner, emit_of(q), l2, "hardsigmoid")[0]
            assert torch.equal(hs, F.relu6(v + 3) / 6), (name, unsigned)
    print(f"sigmoid: largest |g - g*| / (4 * 2^-24 |g*| + 2^-126) so far = {WORST['sigmoid']:.3f}; {differ} of {total} elements differ from torch.sigmoid(v)")
    assert (differ == 0) == MATCHES_TORCH_SIGMOID, "MATCHES_TORCH_SIGMOID no longer states what the device does"


def test_gate_functions_on_special_values():
    """The gate's argument placed exactly: zero weights in layer 2 make v = bias2 (and -0 through a negative weight scale)."""
    vals = [-3.0, 3.0, 0.0, float("nan"), float("inf"), -float("inf"), -3.0000002, 2.9999998, 1.0, -1.0, 6.0, -6.0, 1e-40, 100.0, -100.0, -0.0]
    c, r, n = len(vals), 4, 3
    codes, l1, l2 = operands(n, c, r, True)
    l2 = dict(l2, wq=torch.zeros_like(l2["wq"]), wsum=torch.zeros_like(l2["wsum"]), bias=torch.tensor(vals, device=DEV),
              w_scale=torch.tensor([1.0] * (c - 1) + [-1.0], device=DEV))
    q = emit_of(quantisers()["zeropoint_u8"])
    v = K.squeeze_gate(codes, l1, "relu", q, l2, None)[0]
    want = torch.tensor(vals, device=DEV).expand(n, c)
    assert same(v, want) and bool(torch.signbit(v[:, -1]).all())
    assert same(K.squeeze_gate(codes, l1, "relu", q, l2, "hardsigmoid")[0], F.relu6(v + 3) / 6)
    s = K.squeeze_gate(codes, l1, "relu", q, l2, "sigmoid")[0]
    if MATCHES_TORCH_SIGMOID:
        assert same(s, torch.sigmoid(v))
    assert same(s, 1.0 / (1.0 + torch.exp(-v)))      # the three steps in torch ops on the device: the same special values


# ------------------------------------------------------------------------------------------- Part 3
@pytest.mark.parametrize("unsigned", [True, False], ids=["u8", "s8"])
@pytest.mark.parametrize("inner", [None, "relu"], ids=lambda v: str(v))
def test_exact_family(unsigned, inner):
    """Dyadic scales, codes at the ends of their range, weights small enough for both sums to stay below 2^24: every fp32 step is exact or
    a single rounding of an exactly known number, so float64 from the integers must give the same bytes."""
    n, c, r = 6, 32, 32
    g = torch.Generator().manual_seed(7)
    lo_c, hi_c = (0, 255) if unsigned else (-128, 127)
    codes = torch.where(torch.rand(n, c, generator=g) < 0.5, lo_c, hi_c).to(torch.int16)
    w1 = torch.randint(-127, 128, (r, c), generator=g).to(torch.int16)
    w2 = torch.randint(-127, 128, (c, r), generator=g).to(torch.int16)
    zp1, zp2, s_in, s_q = (3 if unsigned else -4), 7, 2.0 ** -6, 2.0 ** -3
    ws1, ws2 = 2.0 ** -torch.randint(8, 11, (r,), generator=g).double(), 2.0 ** -torch.randint(6, 9, (c,), generator=g).double()
    b1, b2 = torch.randint(-64, 65, (r,), generator=g).double() / 16, torch.randint(-64, 65, (c,), generator=g).double() / 16
    s1 = (codes.long() - zp1) @ w1.long().t()
    h = (s1.double() * (s_in * ws1) + b1).float()                   # one rounding of the exact value: the fused multiply-add
    h = torch.where(h < 0, torch.zeros_like(h), h) if inner == "relu" else h
    qh = torch.clamp(torch.round(h.double() / s_q) + zp2, 0, 255).long()     # ZEROPOINT form, dyadic scale: h / s exact, round half to even
    s2 = (qh - zp2) @ w2.long().t()
    assert int(s1.abs().max()) < 2 ** 24 and int(s2.abs().max()) < 2 ** 24 and int(qh.max()) > int(qh.min())
    want = (s2.double() * (s_q * ws2) + b2).float()
    dt = torch.uint8 if unsigned else torch.int8
    l1 = dict(wq=w1.to(torch.int8).to(DEV), wsum=w1.sum(1).to(torch.int32).to(DEV), bias=b1.float().to(DEV), in_scale=t(s_in), in_zp=t(float(zp1)),
              w_scale=ws1.float().to(DEV))
    l2 = dict(wq=w2.to(torch.int8).to(DEV), wsum=w2.sum(1).to(torch.int32).to(DEV), bias=b2.float().to(DEV), w_scale=ws2.float().to(DEV))
    emit = K.EmitCodes(t(s_q), t(float(zp2)), 0, 255, N.FORM_ZEROPOINT)
    gate, hidden = K.squeeze_gate(codes.to(dt).to(DEV), l1, inner, emit, l2, None, want_hidden=True)
    assert torch.equal(hidden.cpu().view(torch.int32), h.view(torch.int32))
    assert torch.equal(gate.cpu().view(torch.int32), want.view(torch.int32))
    # the hidden codes themselves, through an identity second layer with scale 1 and no bias: gate = (qh - zp2) * s_q
    eye = torch.eye(c, dtype=torch.int8, device=DEV)
    ident = dict(wq=eye, wsum=eye.sum(1, dtype=torch.int32), bias=None, w_scale=torch.ones(c, device=DEV))
    back = K.squeeze_gate(codes.to(dt).to(DEV), l1, inner, emit, ident, None)[0]
    assert torch.equal((back.cpu().double() / s_q + zp2).long(), qh)


# ------------------------------------------------------------------------------------------- Part 4
@pytest.mark.parametrize("which", ["both", "gate", "hidden"])
def test_outputs_as_views_keep_their_surroundings(which):
    n, c, r4 = 5, 48, 12
    codes, l1, l2 = operands(n, c, r4, True)
    s, z, lo, hi, form, g = quantisers()["zeropoint_u8"]
    pattern = 0x7fc12345
    gp = torch.full((n + 2, c), pattern, dtype=torch.int32, device=DEV)
    hp = torch.full((n + 2, r4), pattern, dtype=torch.int32, device=DEV)
    gv, hv = gp[1:n + 1].view(torch.float32), hp[1:n + 1].view(torch.float32)
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731
    rc = N.lib.dlmcq_squeeze_gate_i8(p(codes), p(l1["wq"]), p(l1["wsum"]), p(l1["bias"]), p(l1["in_scale"]), p(l1["in_zp"]), p(l1["w_scale"]),
                                     N.SQUEEZE_SWISH, p(l2["wq"]), p(l2["wsum"]), p(l2["bias"]), p(l2["w_scale"]), N.GATE_SIGMOID,
                                     p(gv) if which != "hidden" else None, p(hv) if which != "gate" else None, n, c, r4, 1, p(s), p(z), lo, hi,
                                     form, g, N.stream_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    gate, hidden = K.squeeze_gate(codes, l1, "swish", emit_of(quantisers()["zeropoint_u8"]), l2, "sigmoid", want_hidden=True)
    for parent, view, want, written in ((gp, gv, gate, which != "hidden"), (hp, hv, hidden, which != "gate")):
        assert bool((parent[0] == pattern).all()) and bool((parent[-1] == pattern).all())
        assert torch.equal(view, want) if written else bool((parent == pattern).all())
    only_gate = K.squeeze_gate(codes, l1, "swish", emit_of(quantisers()["zeropoint_u8"]), l2, "sigmoid")
    only_hidden = K.squeeze_gate(codes, l1, "swish", emit_of(quantisers()["zeropoint_u8"]), l2, "sigmoid", want_gate=False, want_hidden=True)
    assert only_gate[1] is None and only_hidden[0] is None and torch.equal(only_gate[0], gate) and torch.equal(only_hidden[1], hidden)


def test_hidden_width_padded_per_call_and_widths_the_kernel_does_not_take():
    """r % 4 != 0 is zero-padded by the wrapper (hidden comes back r wide); C % 4 != 0 runs the restatement."""
    for n, c, r in ((3, 32, 6), (3, 32, 1), (2, 30, 4)):
        codes, l1, l2 = operands(n, c, r, True)
        q = emit_of(quantisers()["zeropoint_u8"])
        got = K.squeeze_gate(codes, l1, "swish", q, l2, None, want_hidden=True)
        want = K.squeeze_gate_torch(codes, l1, "swish", q, l2, None, want_hidden=True)
        assert got[1].shape == (n, r) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
