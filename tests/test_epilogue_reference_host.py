"""Host-side checks of the exact int8 layer reference (tests/exact_layers.py) that tests/test_gpu_epilogue_exact.py compares every
kernel family with: the constructed layers are exact and carry the cases they exist for, and the oracle's codes round each tie half
to even.  No GPU needed."""
import math

import torch

import exact_layers as X


def gen(seed):
    return torch.Generator().manual_seed(77 + seed)


def ties_of(y):
    """The finite elements of y that sit exactly on a rounding tie (x.5)."""
    f = y[torch.isfinite(y)]
    return f[(f - f.floor()) == 0.5]


def test_edge_values_hold_the_hard_cases():
    ev = torch.tensor(X.EDGE_VALUES, dtype=torch.float32)
    assert bool(ev.isnan().any()) and bool((ev == math.inf).any()) and bool((ev == -math.inf).any())
    assert bool((ev >= 255.5).any()) and bool((ev <= -128.5).any()) and bool(((ev == 0) & torch.signbit(ev)).any())
    near = [v for v in X.EDGE_VALUES if math.isfinite(v) and abs(v - math.floor(v) - 0.5) < 1e-4 and v - math.floor(v) != 0.5]
    assert len(near) >= 8, "values one ulp either side of a tie"
    missed = 0
    for s in X.AWKWARD_SCALES:
        st = torch.tensor(s, dtype=torch.float32)
        vs = torch.tensor([v for v in X.EDGE_VALUES if math.isfinite(v) and (v / s) % 1 == 0.5], dtype=torch.float32)
        assert vs.numel() >= 5 and bool((vs < 0).any())
        q = vs / st                                   # correctly rounded: the tie itself
        assert bool(((q - q.floor()) == 0.5).all())
        t = vs * (1 / st)                             # what a reciprocal fast path computes
        off = (t - t.floor()) != 0.5
        missed += int((off & (torch.round(t) != torch.round(q))).sum())
    assert missed >= 8, "too few ties that v * fl(1 / s) misses in the direction that changes the code"


def test_oracle_rounds_ties_half_to_even_and_maps_codes_to_bytes():
    v = torch.tensor([0.5, 1.5, 2.5, 3.5, -0.5, -1.5, -2.5, 254.5, 255.5, float("nan"), float("inf"), -float("inf")])
    signed = X.oracle_codes(v, X.Quant(1.0, None, -128, 127))
    assert signed[:7].tolist() == [0, 2, 2, 4, 0, -2, -2] and signed[7:9].tolist() == [127, 127]
    uns = X.quantise(v, X.Quant(1.0))
    assert uns.dtype == torch.uint8 and uns.tolist() == [0, 2, 2, 4, 0, 0, 0, 254, 255, 0, 0, 0]   # (ZEROPOINT's STE round: +-inf -> NaN -> 0)
    emu = X.quantise(v, X.Quant(1.0, 0.0, 0, 255, X.FORM_EMULATE))
    assert emu[9:].tolist() == [0, 255, 0]                                                       # (EMULATE's plain round saturates +-inf)
    zp = X.quantise(torch.tensor([-1.5, -4.5]), X.Quant(3.0, 3.0))
    assert zp.tolist() == [3, 1]                  # -1.5 / 3 = -0.5 -> 0, -4.5 / 3 = -1.5 -> -2 (ties to even), + 3
    s8 = X.quantise(torch.tensor([-1.0, -128.0, 5.0]), X.Quant(1.0, None, -128, 127))
    assert s8.dtype == torch.int8 and s8.tolist() == [-1, -128, 5]
    sh = X.quantise(torch.tensor([0.0, 1.0, 255.0]), X.Quant(1.0, shift128=True))
    assert sh.dtype == torch.int8 and sh.tolist() == [-128, -127, 127]


def test_conv_reference_carries_ties_edges_and_saturation():
    lay = X.make_layer(gen(1), 2, 64, 9, 9, 128, 3)
    for act in (0, 1, 2):
        y = X.conv_ref(lay, 1, 1, act=act)
        assert bool(y.isnan().any())
        live = y[:, lay.nz:]
        ties = ties_of(live)
        assert bool(((ties.floor() % 2) == 0).any()) and bool(((ties.floor() % 2) == 1).any()), "ties on even and odd integers"
        if act != 2:
            assert bool(y.isinf().any()) and bool((y >= 255.5).any())
    codes = X.quantise(X.conv_ref(lay, 1, 1, act=1), X.Quant(1.0))
    assert bool((codes == 255).any()) and bool((codes == 0).any())


def test_residual_reference_puts_edges_per_pixel():
    gg = gen(2)
    lay = X.make_layer(gg, 2, 64, 8, 8, 128, 1, zp=2.0)
    lay.bias[:lay.nz] = 0.0
    res = X.edge_residual((2, 128, 8, 8), lay.nz, gg)
    y = X.conv_ref(lay, residual=res)
    edge = y[:, :lay.nz]
    assert bool(edge.isnan().any()) and bool(edge.isinf().any())
    assert len(set(edge[0, 0].flatten().tolist())) > 4, "edge values vary from pixel to pixel"
    live = y[:, lay.nz:]
    assert bool(live.isinf().any()) and ties_of(live).numel() > 0


def test_depthwise_asymmetric_and_pooling_references_are_exact():
    gg = gen(3)
    dw = X.make_layer(gg, 2, 64, 15, 15, 64, 3, depthwise=True, asym=True, zp=2.0)
    y = X.conv_ref(dw, 1, 1, act=1)
    assert y.shape == (2, 64, 15, 15) and ties_of(y[:, dw.nz:]).numel() > 0
    stem = X.make_layer(gg, 2, 3, 32, 32, 64, 7, zp=2.0)
    yp = X.conv_ref(stem, 2, 3, act=1, pool=True)
    assert yp.shape == (2, 64, 8, 8) and bool(yp.isnan().any())
    sg = X.make_layer(gg, 2, 64, 9, 9, 128, 3, signed_in=True, asym=True)
    assert sg.codes.dtype == torch.int8 and int(sg.codes.min()) == -2
    X.conv_ref(sg, 2, 1)


def test_second_gemm_reads_the_reference_codes():
    """Chain / dwpw: the 1x1 layer after the first quantiser sees that quantiser's codes channel for channel."""
    gg = gen(4)
    lay = X.make_layer(gg, 2, 64, 8, 8, 128, 1)
    mid = X.conv_ref(lay, act=1)
    q1 = X.Quant(0.5, 3.0)
    c1 = X.quantise(mid, q1)
    wq2, b2 = X.identity_pw(256, 128, 24, gg)
    y2 = X.second_gemm_ref(c1, q1, wq2, b2, act2=0)
    want = (c1.double() - 3.0) * 0.5 + b2[:128].double().reshape(1, -1, 1, 1)
    assert torch.equal(y2[:, :128].double(), want)
    torch.testing.assert_close(y2[:, 128:152].flatten(2)[:, :, 0], b2[128:152].reshape(1, -1).expand(2, -1), rtol=0, atol=0, equal_nan=True)
    assert bool(y2[:, 128:152].isnan().any())


def test_quantisers_cover_plain_nonplain_and_degenerate_scales():
    plain = X.plain_quants()
    assert all(q.plain for q in plain)
    scales = {q.scale for q in plain}
    assert {1.0, 0.5, 3.0, 6.0, 7.0, 15.0, 2.0 ** -100}.issubset(scales)
    assert any(0 < s < 2.0 ** -126 for s in scales), "a denormal scale"
    assert float(torch.tensor(1e-41, dtype=torch.float32)) != 0.0
    assert not any(q.plain for q in X.nonplain_quants())
    assert any(q.zp and q.zp > 0 and q.lo == 0 for q in X.nonplain_quants()), "a positive zero point: ReLU folded into the clamp"
