"""CPU part of the backward tests: pins oracle.fakequant_oracle's float64 anchors (`fq_backward_f64`,
`rootq_weight_backward_f64`) and checks, without a GPU, the conditions that tests/test_gpu_backward.py relies on - that the
exact cases really are exact in fp32 in any order, and that every planted element is visible in the result."""
import math

import pytest
import torch

import _bwd_cases as C
from _cmp import assert_bits_equal
from oracle import fakequant_oracle as O

F64 = torch.float64


# ------------------------------------------------------------------------------------------- pins, hand-unrolled
def _one(form, x, gy, s, o, lo, hi, g=0.0):
    t = lambda v: torch.tensor([[[v]]], dtype=torch.float32)
    gx, value, abs_sum, contrib = O.fq_backward_f64(form, t(x), t(gy), torch.tensor([s]), None if o is None else torch.tensor([o]), lo, hi, g)
    return float(gx), float(value), float(abs_sum), float(contrib)


def test_fq_backward_f64_by_hand():
    # qbase, s = 1/4, o = 1/2, g = 1/2 (s^ = s exactly):  v = (x - o)/s
    assert _one("qbase", 1.0, 3.0, 0.25, 0.5, -8, 7, 0.5) == (3.0, 0.0, 0.0, 0.0)                      # v = 2, on the grid
    assert _one("qbase", 1.0625, 3.0, 0.25, 0.5, -8, 7, 0.5) == (3.0, 0.5 * 3.0 * -0.25, 0.75, -0.75)   # v = 2.25, q = 2
    assert _one("qbase", 2.25, 3.0, 0.25, 0.5, -8, 7, 0.5) == (3.0, 0.0, 0.0, 0.0)                     # v = 7 = hi: inside
    assert _one("qbase", 2.3125, -2.0, 0.25, 0.5, -8, 7, 0.5) == (0.0, 0.5 * -14.0, 14.0, -14.0)        # v = 7.25: q = hi, no v
    assert _one("qbase", -1.5625, 1.0, 0.25, 0.5, -8, 7, 0.5) == (0.0, -4.0, 8.0, -8.0)                 # v = -8.25: q = lo
    assert _one("qbase", 0.875, 1.0, 0.25, 0.5, -8, 7, 0.5)[3] == 0.5                                    # v = 1.5: tie to even, q = 2
    # zeropoint, s = 1/4, zp = 3, codes 0..15:  a = R(x/s) + zp
    assert _one("zeropoint", 0.5625, 2.0, 0.25, 3.0, 0, 15) == (2.0, -0.5, 0.5, -0.5)                    # v = 2.25, q = 2
    assert _one("zeropoint", 3.0625, 2.0, 0.25, 3.0, 0, 15) == (2.0, -0.5, 0.5, -0.5)                    # v = 12.25, a = 15: inside
    assert _one("zeropoint", 3.1875, 2.0, 0.25, 3.0, 0, 15) == (0.0, 24.0, 24.0, 24.0)                   # v = 12.75, a = 16: q = 12
    assert _one("zeropoint", -0.9375, 2.0, 0.25, 3.0, 0, 15) == (0.0, -6.0, 6.0, -6.0)                   # v = -3.75, a = -1: q = -3
    # symmetric ignores the offset
    assert _one("symmetric", 0.5625, 2.0, 0.25, 3.0, -7, 7) == (2.0, -0.5, 0.5, -0.5)
    assert _one("symmetric", 1.9375, 1.0, 0.25, None, -7, 7) == (0.0, 7.0, 7.0, 7.0)                     # v = 7.75 -> 8: q = 7
    # rootq_act, s = 1/4, codes 0..15: up = 3.75
    assert _one("rootq_act", 0.5625, 2.0, 0.25, None, 0, 15) == (2.0, -0.5, 0.5, -0.5)
    assert _one("rootq_act", -0.5, 2.0, 0.25, None, 0, 15) == (0.0, 0.0, 0.0, 0.0)                       # below: t = 0
    assert _one("rootq_act", 4.0, 2.0, 0.25, None, 0, 15) == (0.0, 30.0, 30.0, 30.0)                     # above: gy * (hi - lo)
    # sums are per channel, over outer and inner
    x = torch.tensor([0.5625, 0.5, 1.0625, 0.3125]).reshape(2, 2, 1)
    gy = torch.tensor([1.0, 5.0, 2.0, -4.0]).reshape(2, 2, 1)
    _, value, abs_sum, contrib = O.fq_backward_f64("symmetric", x, gy, torch.tensor([0.25, 0.125]), None, -7, 7)
    assert contrib.reshape(-1).tolist() == [-0.25, 0.0, -0.5, 2.0] and value.tolist() == [-0.75, 2.0] and abs_sum.tolist() == [0.75, 2.0]


@pytest.mark.parametrize("form", C.FORMS[:3])
def test_fq_backward_f64_agrees_with_the_autograd_restatements(form):
    g = torch.Generator().manual_seed(11)
    lo, hi = C.RANGE[form]
    x = torch.randn(3, 4, 5, generator=g) * 0.5
    gy = torch.randn(3, 4, 5, generator=g)
    per_channel = form == "symmetric"
    scale = torch.rand(4, generator=g) * 0.05 + 0.02 if per_channel else torch.full((4,), 0.043)
    if form == "qbase":
        off, gg = torch.full((4,), 0.0137), 0.01
        want_gx, want_gs = O.qbase_backward(x, scale[0], off[0], gy, lo, hi, gg)
    elif form == "zeropoint":
        off, gg = torch.full((4,), 5.0), 0.0
        want_gx, want_gs = O.fsptq_act_backward(x, scale[0], off[0], gy, lo, hi)
    else:
        off, gg = None, 0.0
        want_gx, want_gs = O.fsptq_weight_backward(x.transpose(0, 1), scale.reshape(4, 1, 1), gy.transpose(0, 1), lo, hi)
        want_gx = want_gx.transpose(0, 1)
    gx, value, _, _ = O.fq_backward_f64(form, x, gy, scale, off, lo, hi, gg)
    assert_bits_equal(gx, want_gx, form + " gx")
    got = value if per_channel else value.sum()
    torch.testing.assert_close(got.float().reshape(-1), want_gs.reshape(-1), rtol=2e-5, atol=1e-6)


def _rootq_composite64(w, up, lw, alpha, lo, hi):
    """RootQ/base.py:146-155 in float64 with the straight-through floor and sign and the detached interval middle."""
    wc = w + torch.relu(lw - w)
    wc = wc - torch.relu(wc - up)
    delta = (up - lw) / (hi - lo)
    v = (wc - lw) / delta
    iv = (v.floor() - v).detach() + v
    mi = ((iv + 0.5) * delta + lw).detach()
    a = alpha + torch.relu(1e-4 - alpha)
    a = a - torch.relu(a - 1)
    e = wc - mi
    phi = torch.pow(2 / delta * e.abs() + 1e-5, a) * (e / (e.abs() + 1e-5))
    s = (phi.sgn() - phi).detach() + phi
    return ((s + 1) / 2 + iv) * delta + lw


@pytest.mark.parametrize("bits,alpha", [(4, 0.25), (2, 0.7), (3, 1.5), (4, 5e-5)])
def test_rootq_weight_backward_f64_agrees_with_autograd(bits, alpha):
    g = torch.Generator().manual_seed(5)
    hi = 2 ** (bits - 1) - 1
    lo = -hi
    # dyadic weights and bounds (delta = 2^-4): every fp32 step up to e = wc - mi is exact, so float64 takes the same decisions
    up, lw = (hi - lo) / 32, -(hi - lo) / 32
    w = (torch.randn(400, generator=g) * 0.6 * up * 4096).round() / 4096
    gy = torch.randn(400, generator=g)
    leaves = [torch.tensor(v, dtype=F64, requires_grad=True) for v in (float(torch.tensor(up)), float(torch.tensor(lw)), float(torch.tensor(alpha)))]
    wr = w.double().requires_grad_(True)
    _rootq_composite64(wr, *leaves, lo, hi).backward(gy.double())
    gw, scalars, abs_sums = O.rootq_weight_backward_f64(w, gy, up, lw, alpha, lo, hi)
    assert int((w > up).sum()) > 3 and int((w < lw).sum()) > 3
    torch.testing.assert_close(gw, wr.grad, rtol=1e-5, atol=1e-6)
    for got, leaf, name in zip(scalars, leaves, ("g_upper", "g_lower", "g_alpha")):
        assert abs(float(got) - float(leaf.grad)) <= 1e-5 * float(abs_sums["d"] + abs_sums["l"]), name
    if alpha > 1 or alpha < 1e-4:
        assert float(scalars[2]) == 0.0 and float(abs_sums["a"]) == 0.0


def test_rootq_weight_backward_f64_by_hand():
    # 2 bits (-1..1), bounds +-0.5: delta = 0.5, k = 4.  alpha = 1 makes pow the identity.
    w = torch.tensor([0.75, -0.875, 0.125])
    gy = torch.tensor([2.0, 3.0, 4.0])
    gw, (gu, gl, ga), ab = O.rootq_weight_backward_f64(w, gy, 0.5, -0.5, 1.0, -1, 1)
    eps = float(torch.tensor(1e-5, dtype=torch.float32))

    def g_wc(g, v, e):       # g_v/delta + g_e with a = 1: B^(a-1) = 1
        ae, sg = abs(e), math.copysign(1.0, e)
        den, B = ae + eps, 4 * ae + eps
        g_phi = g * 0.25
        return g + g_phi * (e / den) * 4 * sg + g_phi * B / den - g_phi * B * e / den ** 2 * sg
    # element 0: clipped above, wc = 0.5, v = 2, I = 2, mi = 0.75, e = -0.25;  1: clipped below, wc = -0.5, v = 0, e = -0.25;
    # 2: inside, v = 1.25, I = 1, mi = 0.25, e = -0.125
    up_add, lo_add, mid = g_wc(2.0, 2.0, -0.25), g_wc(3.0, 0.0, -0.25), g_wc(4.0, 1.25, -0.125)
    assert gw.tolist() == [0.0, 0.0, pytest.approx(mid, rel=1e-12)]
    d = 0.0
    for g, v, iv, e in ((2.0, 2.0, 2.0, -0.25), (3.0, 0.0, 0.0, -0.25), (4.0, 1.25, 1.0, -0.125)):
        sign = e / (abs(e) + eps)
        d += g * (0.0 + iv) - g * 0.5 * (v / 0.5) + (g * 0.25 * sign) * abs(e) * (-2.0 / 0.25)      # sphi = -1 everywhere
    assert float(gu) == pytest.approx(up_add + d / 2, rel=1e-12)
    assert float(gl) == pytest.approx(lo_add - d / 2, rel=1e-12)          # the direct path g - g_v/delta is 0
    want_a = sum(g * 0.25 * (e / (abs(e) + eps)) * (4 * abs(e) + eps) * math.log(4 * abs(e) + eps) for g, e in ((2.0, -0.25), (3.0, -0.25), (4.0, -0.125)))
    assert float(ga) == pytest.approx(want_a, rel=1e-12)
    assert float(ab["u"]) == pytest.approx(abs(up_add), rel=1e-12) and float(ab["l"]) == pytest.approx(2 * 9.0 + abs(lo_add), rel=1e-12)


# ------------------------------------------------------------------------------------------- geometry
def test_plans_are_the_geometries_the_shapes_are_here_for():
    for shape, want in C.CHANNEL_PLANS.items():
        assert C.plan(*shape)[:2] == want, shape
    assert C.plan(1, 1, 262148)[0] == 257 and C.plan(1, 1, C.MULTI_MAX_N)[0] == 8192 and C.plan(1, 1, C.BIG)[0] == 8192
    assert C.chain_length(1, 1, C.BIG, True) == 9 and C.chain_length(1, 1, C.BIG, False) == 5
    assert C.chain_length(1, 1, 3, True) == 1 and C.chain_length(1, 1, 1024, True) == 4 and C.chain_length(1, 1, 1027, True) == 5
    assert C.chain_length(5, 1024, 12, True) == 12 and C.chain_length(5, 1024, 9, False) == 3
    assert C.chain_length(1, 257, 1028, True) == 8 and C.chain_length(1, 257, 1027, False) == 5


# ------------------------------------------------------------------------------------------- exact cases
@pytest.mark.parametrize("form,shape", C.all_fq_cases(), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_exact_cases_are_exact_and_every_planted_element_counts(form, shape):
    case, (gx, value, abs_sum, contrib) = C.case_with_reference("exact", form, shape)
    units = contrib / C.UNIT
    assert torch.equal(units, units.round()), "a contribution is not a multiple of 2^-2"
    assert float(abs_sum.max()) / C.UNIT < 2 ** 24, "a partial sum could need more than 24 bits"
    assert torch.equal(value.float().double(), value), "the scale gradient itself is not an fp32 number"
    flat = contrib.reshape(-1)
    ch = shape[1]
    for c in (range(ch) if ch <= 3 else (0, ch // 2, ch - 1)):
        planted = flat[case.planted[:, c]]
        assert sorted(planted.abs().tolist()) == [2.0 ** (j - 2) for j in range(planted.numel())], "planted contributions are distinct powers of two"
        total = flat.reshape(shape)[:, c, :].sum()
        g = 2.0 ** -10 if form == "qbase" else 1.0
        assert float(total * g) == float(value[c])
        for p in planted.tolist():                   # the reference without that element is another fp32 number
            assert float(((total - p) * g).float()) != float(value[c].float())
    assert torch.equal(gx.reshape(-1)[case.planted.reshape(-1)], case.gy.reshape(-1)[case.planted.reshape(-1)])
    assert int((contrib != 0).sum()) > case.planted.numel() or shape[2] * shape[0] < 16


@pytest.mark.parametrize("form,shape", [c for c in C.all_fq_cases() if c[1][2] < 2 ** 20], ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_random_cases_stay_clear_of_underflow(form, shape):
    """The summation bound has no underflow term: a channel's sum|contrib| is 0 (nothing to err on) or far above 2^-126."""
    _, (_, value, abs_sum, _) = C.case_with_reference("random", form, shape)
    assert bool(torch.isfinite(value).all()) and bool(((abs_sum == 0) | (abs_sum > 2.0 ** -40)).all())
    assert shape[0] * shape[2] < 16 or bool((abs_sum > 0).all())


# ------------------------------------------------------------------------------------------- RootQ planted elements
@pytest.mark.parametrize("n", C.RQ_N)
@pytest.mark.parametrize("bits", C.RQ_BITS)
@pytest.mark.parametrize("alpha", C.RQ_ALPHA)
def test_rootq_planted_elements_outweigh_the_tolerance(n, bits, alpha):
    case, (gw, scalars, abs_sums) = C.rootq_case(n, bits, alpha)
    bu, bl, ba = case.bounds(abs_sums)
    assert case.planted and (n < 4 or len(case.planted_above) == 2)
    assert bool((case.w[case.planted_above] > case.upper).all())
    for i in case.planted + case.planted_above:
        gy = case.gy.clone()
        gy[i] = 0.0
        _, without, _ = case.reference(gy)
        moved = [abs(float(a) - float(b)) for a, b in zip(scalars, without)]
        if i in case.planted_above:     # clipped above: v = I, B = k|e| + 1e-5 = 1 and log B = 0 - the element reaches g_upper
            assert moved[0] > 4 * bu, f"element {i} does not move g_upper: {moved[0]} vs bound {bu}"      # (and neither other sum much)
            continue
        assert moved[1] > 4 * bl, f"element {i} does not move g_lower: {moved[1]} vs bound {bl}"
        if alpha <= 1:                  # a clipped alpha has no gradient: g_alpha is exactly 0 and so is its bound
            assert moved[2] > 4 * ba, f"element {i} does not move g_alpha: {moved[2]} vs bound {ba}"
    if alpha > 1:
        assert float(scalars[2]) == 0.0 and ba == 0.0
