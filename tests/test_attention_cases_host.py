"""The constructions of tests/attention_exact_cases.py, on the host (no GPU): what tests/test_gpu_attention_exact.py rests on, proven from
the tensors it launches - exact ties and score gaps above 104, integer sums below 2^24, the counts and the elements that tell a division
from a multiply by the reciprocal, the probe's exact scores and its 4 u model bound, the NaN masks against torch's unfused graph, the
geometry of the padded output views."""
import numpy as np
import pytest
import torch

import attention_exact_cases as C
from test_gpu_attention import SHAPES, U

DIMS = C.DIMS


def scores(q, k, scale):
    """fp32 scores the way the kernel forms them where the chain is exact (integer products): fl32(a scale); and float64's."""
    a = q.double() @ k.double().transpose(-1, -2)
    assert bool((a == a.float().double()).all()) and float(a.abs().max()) < 2 ** 24      # the chain's partial sums are integers below 2^24
    return a.float() * torch.tensor(scale, dtype=torch.float32), a * scale


# ------------------------------------------------------------------------------------------- 1. ties
def test_the_tie_shapes_are_the_six_base_shapes_and_one_more():
    assert C.BASE_TIE_SHAPES == [s[:4] for s in SHAPES] + [(1, 5, 129, 257), (1, 4, 97, 40)] and C.TIE_SHAPES[:6] == C.BASE_TIE_SHAPES
    assert all(b * h <= 8 and max(tq, tk) <= 257 for b, h, tq, tk in C.TIE_SHAPES)
    reach = lambda tk: {int(n) for z in C.ZSETS for n in C.tied(torch.arange(512), torch.full((512,), C.zmask(z)), tk).sum(-1)}  # noqa: E731
    assert all(3 not in reach(s[3]) for s in C.BASE_TIE_SHAPES) and 3 in reach(37)      # why (1, 2, 40, 37) is there


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("shape", C.TIE_SHAPES, ids=str)
def test_ties_are_exact_and_the_rest_lies_beyond_expf(shape, d):
    c = C.tie_case(shape, d)
    b, h, tq, tk = shape
    s32, s64 = scores(c["q"], c["k"], c["scale"])
    mask, count = c["mask"], c["count"]
    top = s32.amax(-1, keepdim=True)
    assert torch.equal(s32 == top, mask), "the maximal fp32 scores are not the tied keys"
    assert bool((count >= 1).all()) and bool((c["pi"] < tk).all()) and bool(mask.gather(-1, c["pi"][..., None]).all())
    gap = (s64.amax(-1, keepdim=True) - s64)[~mask]
    assert float(gap.min()) > C.GAP + 20, float(gap.min())      # 128 (D = 64), 181 (D = 32)
    v = c["v"]
    assert v.unique().numel() == v.numel() and bool((v == v.round()).all()) and float(v.min()) >= 1
    assert float(v.amax((0, 1, 2)).max()) * 8 < 2 ** 24 and float(c["total"].max()) < 2 ** 24
    exact = mask.double() @ v.double()
    assert torch.equal(c["total"].double(), exact)
    assert torch.equal(c["want"], (exact / count[..., None]).float()), "fl32 of float64's quotient is another number than the fp32 division"
    assert set(c["zi"].unique().tolist()) == set(range(len(C.ZSETS)))
    for n, z in enumerate(C.ZSETS):      # where the whole group lies below Tk, it is 2^|Z| keys
        assert int(count[c["zi"] == n].max()) == 2 ** len(z) or tk < 128
    j = torch.arange(tk)
    if tk >= 128:      # ties in two key blocks, and in both lane halves of one block
        blocks = torch.stack([(mask & ((j >> 5) == kb)).any(-1) for kb in range((tk + 31) // 32)], -1).sum(-1)
        assert int(blocks.max()) >= 2 and bool(((blocks >= 2) & (c["zi"] == 2)).any()) and bool(((blocks >= 2) & (c["zi"] == 3)).any())
    halves = torch.stack([(mask & (((j >> 2) & 1) == hf)).any(-1) for hf in (0, 1)], -1).all(-1)
    assert bool((halves & (c["zi"] == 1)).any()) or tk < 8


@pytest.mark.parametrize("d", DIMS)
def test_the_counts_and_what_tells_a_division_from_a_reciprocal(d):
    cases = [C.tie_case(s, d) for s in C.TIE_SHAPES]
    count = torch.cat([c["count"].reshape(-1) for c in cases])
    sep = torch.cat([C.separating(c["total"], c["count"]).reshape(-1, d) for c in cases])
    assert {1, 2, 3, 4, 5, 6, 7, 8} == set(count.unique().tolist())
    odd = (count & (count - 1)) != 0
    assert not bool(sep[~odd].any())                               # a power of two divides exactly either way
    for n in (3, 5, 6, 7):
        assert int(sep[count == n].sum()) >= 25, n                 # each of them is told apart, in 25 elements or more
    part = float(sep[odd].float().mean())
    print(f"D = {d}: {int(odd.sum())} of {count.numel()} rows have a count in (3, 5, 6, 7); {int(sep.sum())} of their {int(odd.sum()) * d} elements "
          f"({part:.3f}) separate x / c from x fl32(1 / c); of all {sep.numel()} elements: {float(sep.float().mean()):.4f}")
    assert part >= 0.25


# ------------------------------------------------------------------------------------------- 2. uniform rows
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("tk", C.UNIFORM_TK)
def test_uniform_rows(tk, d):
    assert C.UNIFORM_BH == (1, 5) and len(C.UNIFORM_TQ) == 14 and max(C.UNIFORM_TQ) <= 257
    for tq in (C.UNIFORM_TQ[0], C.UNIFORM_TQ[-1]):
        for zero_scale in (False, True):
            c = C.uniform_case(tq, tk, d, zero_scale)
            v, q = c["v"], c["q"]
            assert tuple(q.shape) == (1, 5, tq, d) and tuple(v.shape) == (1, 5, tk, d)
            assert v.unique().numel() == v.numel() and bool((v == v.round()).all()) and float(v.max()) * tk < 2 ** 24
            assert torch.equal(c["total"].double(), v.double().sum(2))
            assert torch.equal(c["want"], (v.double().sum(2) / tk).float()[0])
            if zero_scale:
                assert c["scale"] == 0.0 and bool((q != 0).all()) and bool(torch.isfinite(q).all())
            else:
                assert c["scale"] > 0 and not bool(q.any())
            assert bool(((q.double() @ c["k"].double().transpose(-1, -2)) * c["scale"] == 0).all())      # every score +-0


# ------------------------------------------------------------------------------------------- 3. the probe
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("variant", C.PROBE_VARIANTS)
def test_probe_scores_are_the_grid(variant, d):
    c = C.probe_case(d, variant)
    x = C.probe_grid()
    assert torch.equal(c["x"].reshape(-1), x) and float(x[0]) == -0.125 and float(x[-1]) == -64.0
    s32, s64 = scores(c["q"], c["k"], c["scale"])
    assert torch.equal(s32.double(), s64)      # the power-of-two scale: no rounding
    low, top = (1, 0) if variant == "block0" else (0, 32)
    assert torch.equal(s64[..., low], c["x"]) and not bool(s64[..., top].any())
    if variant == "blocks":
        assert not bool(s64[..., 36].any()) and c["k"].shape[2] == 37
        rest = [j for j in range(37) if j not in (0, 32, 36)]
        assert bool((s64[..., rest] - c["x"][..., None] < -500).all())      # p = 0 against the running maximum x of block 0 already
        assert bool((c["v"][:, :, rest] == 3).all()) and bool((c["v"][:, :, 0] == 1).all()) and not bool(c["v"][:, :, [32, 36]].any())
    else:
        assert c["k"].shape[2] == 2 and bool((c["v"][:, :, 1] == 1).all()) and not bool(c["v"][:, :, 0].any())


def test_probe_model():
    """The figures for the two-key probe ("block0"), in units of 2^-24: the correctly rounded expf 1.72, expf off by one ulp
    either way 3.47 - inside 4 -, v_exp_f32 on a pre-scaled argument far outside.  "blocks" rounds l twice (fl(fl(e + 1) + 1)): the
    correctly rounded expf gives 2.73, every expf one ulp low 3.77; a model in which EVERY expf is one ulp high reaches 4.31 - the 4 u
    of the device test are not derived for such a library there, and the figure is printed."""
    x = C.probe_grid().numpy()
    e64 = np.exp(x)
    e32 = C.exp_rounded(x.astype(np.float32))
    mid = (e32.astype(np.float64) + np.nextafter(e32, np.where(e64 > e32, np.float32(np.inf), np.float32(0))).astype(np.float64)) / 2
    assert np.all(np.abs(e64 - mid) > 1e3 * np.spacing(e64)) and np.all(np.abs(e32 - e64) <= np.abs(mid - e32.astype(np.float64)))
    up, down = (lambda a: np.nextafter(C.exp_rounded(a), np.float32(np.inf))), (lambda a: np.nextafter(C.exp_rounded(a), np.float32(0)))
    worst = {}
    for variant, ref in (("block0", e64 / (1 + e64)), ("blocks", e64 / (2 + e64))):
        for name, fn in (("rounded", C.exp_rounded), ("up", up), ("down", down), ("exp2", C.exp2_prescaled)):
            out = C.probe_model(x, variant, fn).astype(np.float64)
            worst[variant, name] = float(np.max(np.abs(out - ref) / ref)) / U
    print({k: round(v, 2) for k, v in worst.items()})
    assert C.PROBE_TOL == 4 * U
    assert worst["block0", "rounded"] < 2 and worst["block0", "up"] < 4 and worst["block0", "down"] < 4
    assert worst["blocks", "rounded"] < 3 and worst["blocks", "down"] < 4 and worst["blocks", "up"] < 4.5
    assert worst["block0", "exp2"] > 40 and worst["blocks", "exp2"] > 40


# ------------------------------------------------------------------------------------------- 4. -inf
def _torch_graph(q, k, v, scale):
    return torch.matmul(torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * scale, dim=-1), v)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("every_key", [False, True])
@pytest.mark.parametrize("shape", C.INF_SHAPES, ids=str)
def test_inf_prefix_masks_are_torch_s(shape, every_key, d):
    c = C.inf_prefix_case(shape, d, every_key)
    q, k, v, nan = c["q"], c["k"], c["v"], c["nan"]
    tk = shape[3]
    assert C.INF_PREFIX == 40 and tk > 40 and c["first"] == (tk if every_key else 40)
    assert bool((k[:, :, :c["first"], 0] == float("-inf")).all()) and bool(torch.isfinite(k[:, :, c["first"]:]).all())
    assert bool(torch.isfinite(k[..., 1:]).all()) and bool(torch.isfinite(q).all()) and bool(torch.isfinite(v).all())
    ref = _torch_graph(q, k, v, c["scale"])
    assert torch.equal(ref.isnan(), nan[..., None].expand_as(ref)), "the case's mask is not torch's"
    assert bool(torch.isfinite(ref[~nan]).all())
    assert float(q[0, 0, 1, 0]) == 0.0 and bool(nan[0, 0, 1]) and bool((q[..., 0] < 0).any())
    if every_key:
        assert bool(nan.all()) and bool((q[..., 0] > 0).any())
    else:
        pos = q[..., 0] > 0
        assert torch.equal(pos, ~nan) and int(pos.sum()) * 3 > pos.numel()
        s = (q.double() @ k.double().transpose(-1, -2)) * c["scale"]
        assert bool((s[pos][:, :40] == float("-inf")).all()) and bool(torch.isfinite(s[pos][:, 40:]).all())
        rest = _torch_graph(q.double(), k[:, :, 40:].double(), v[:, :, 40:].double(), c["scale"])      # the remaining keys alone
        assert float((ref.double() - rest)[pos].abs().max()) < 1e-4


@pytest.mark.parametrize("d", DIMS)
def test_negative_scale_case(d):
    for shape in C.INF_SHAPES:
        c = C.negative_scale_case(shape, d)
        assert c["scale"] == -float(torch.tensor(d ** -0.5, dtype=torch.float32)) and all(bool(torch.isfinite(c[n]).all()) for n in "qkv")


# ------------------------------------------------------------------------------------------- 5. stores
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("tq", C.STORE_TQ)
def test_padded_view_is_one_the_entry_point_takes(tq, d):
    b, h, tk = C.STORE_BHTK
    assert b * h <= 8 and tk == 50 and tuple(C.store_case(tq, d)["q"].shape) == (b, h, tq, d)
    shape, off, (sb, sh, st) = C.padded(b, h, tq, d)
    assert shape == (b, tq + 2, h * d + 8) and off == shape[2] + 4 and (sb, sh, st) == (shape[1] * shape[2], d, shape[2])
    assert (4 * off) % 16 == 0 and off % 4 == 0 and all(s % 4 == 0 for s in (sb, sh, st)) and st >= d      # 16-byte rows of fp32, 4-byte words of codes
    parent = torch.arange(shape[0] * shape[1] * shape[2]).reshape(shape)
    view = parent[:, 1:tq + 1, 4:4 + h * d]
    assert view.storage_offset() == off and view.stride() == (sb, st, 1) and int(view[b - 1, tq - 1, h * d - 1]) < parent.numel() - shape[2]
