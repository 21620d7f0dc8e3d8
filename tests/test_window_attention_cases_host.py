"""The constructions of tests/window_attention_exact_cases.py, on the host (no GPU): what tests/test_gpu_window_attention_exact.py rests on,
proven from the tensors it launches - operands exact in f16, integer sums below 2^24, exact ties on a numpy float32 restatement of the
headers' score steps and gaps above 104 on float64, the counts and the elements that tell a division from a multiply by the reciprocal,
the alternative orders of the score steps apart by 1 or more, the probe's exact scores, its fp32 model bound and the f16 tolerance's
models, the non-finite masks against torch's unfused graph, the geometry of the views."""
import numpy as np
import pytest
import torch

import window_attention_exact_cases as C
from dlmc.quantization.scalar import kernels as K
from test_gpu_attention import U

DIMS = C.DIMS


def f16_exact(*tensors):
    return all(torch.equal(x.half().float(), x) for x in tensors)


def exact_scores(c):
    """(fp32 scores by the headers' steps, float64 scores); a = q . k is an integer below 2^24 here: the chain and every MFMA order are exact."""
    s32, a = C.score_steps(c["q"], c["k"], c["scale"], c["bias"], c["mask"])
    assert np.all(a == np.round(a)) and np.abs(a).max() < 2 ** 24
    return torch.from_numpy(s32), C.scores64(c["q"], c["k"], c["scale"], c["bias"], c["mask"])


# ------------------------------------------------------------------------------------------- 1. ties
def test_tie_shapes_and_sets():
    assert C.TIE_T == (1, 8, 33, 37, 49, 63, 64) and all(b * h <= 12 and b % nw == 0 for b, h, nw in C.TIE_BHW.values())
    assert C.TIE_BHW["mask"] == (6, 2, 3)
    bits = [set(z) for z in C.ZSETS]
    assert {0} in bits and {2} in bits and {3} in bits and {4} in bits and {5} in bits and max(len(z) for z in C.ZSETS) == 3
    ints = C.f16_integers()
    assert len(ints) == 5120 and f16_exact(ints) and float(ints.max()) * 64 < 2 ** 24


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("t", C.TIE_T)
@pytest.mark.parametrize("way", C.TIE_WAYS)
def test_ties_are_exact_and_the_rest_lies_beyond_the_exponential(way, t, d):
    c = C.tie_case(way, t, d)
    b, h, nw = C.TIE_BHW[way]
    q, k, v, tm, count = c["q"], c["k"], c["v"], c["tied"], c["count"]
    assert tuple(q.shape) == (b, h, t, d) and f16_exact(q, k, v)
    assert (c["bias"] is not None) == (way in ("bias", "split")) and (c["mask"] is not None) == (way in ("mask", "split"))
    assert c["mask"] is None or c["mask"].shape[0] == nw
    assert bool(q.any()) == (way == "qk")
    s32, s64 = exact_scores(c)
    assert torch.equal(s32 == s32.amax(-1, keepdim=True), tm), "the maximal fp32 scores are not the tied keys"
    assert torch.equal(s32.double(), s64) or way == "qk"      # (the terms are dyadic: their sums are exact; qk rounds a scale once)
    assert bool((count >= 1).all()) and int(count.max()) <= 8
    if t > 1 and bool((~tm).any()):
        gap = float((s64.amax(-1, keepdim=True) - s64)[~tm].min())
        assert gap >= C.GAP + 20, gap
    if way == "split" and t >= 8:      # neither term alone ties: the tied keys' bias values (and mask values) are all different
        rows = count > 1
        for term in (c["bias"][None].expand(b, h, t, t), c["mask"].repeat(b // nw, 1, 1)[:, None].expand(b, h, t, t)):
            top = torch.where(tm, term, torch.tensor(float("-inf"))).amax(-1, keepdim=True)
            assert bool((((term == top) & tm).sum(-1)[rows] == 1).all())
            assert not torch.equal(term == term.amax(-1, keepdim=True), tm)
    for i in range(b * h):      # distinct within a head, and another permutation per head
        vv = v.reshape(b * h, -1)[i]
        assert vv.unique().numel() == vv.numel()
    assert b * h == 1 or not torch.equal(v.reshape(b * h, -1)[0], v.reshape(b * h, -1)[1])
    exact = tm.double() @ v.double()
    assert float(exact.max()) < 2 ** 24 and torch.equal(c["total"].double(), exact)
    assert torch.equal(c["want"], (exact / count[..., None]).float()), "fl32 of float64's quotient is another number than the fp32 division"


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("way", C.TIE_WAYS)
def test_the_counts_the_placements_and_what_tells_a_division_from_a_reciprocal(way, d):
    cases = [C.tie_case(way, t, d) for t in C.TIE_T]
    count = torch.cat([c["count"].reshape(-1) for c in cases])
    sep = torch.cat([C.separating(c["total"], c["count"]).reshape(-1, d) for c in cases])
    assert {1, 2, 3, 4, 5, 6, 7, 8} == set(count.unique().tolist())
    odd = (count & (count - 1)) != 0
    assert not bool(sep[~odd].any())                               # a power of two divides exactly either way
    rows = {n: int((count == n).sum()) for n in range(1, 9)}
    assert all(rows[n] >= 8 for n in (3, 5, 6, 7)), rows
    part = float(sep[odd].float().mean())
    per = {n: round(float(sep[count == n].float().mean()), 3) for n in (3, 5, 6, 7)}
    print(f"{way} D = {d}: rows by count {rows}; of the {int(odd.sum()) * d} elements with a count in (3, 5, 6, 7), {int(sep.sum())} ({part:.3f}) "
          f"separate x / c from x fl32(1 / c); per count {per}")
    assert part >= 0.25 and all(x > 0 for x in per.values())
    # where the tied sets lie: neighbours in a register quad, the two lane halves, other quads, the two blocks, sets of 8
    for c, t in zip(cases, C.TIE_T):
        tm, zi = c["tied"], c["zi"]
        assert set(zi.unique().tolist()) == set(range(min(len(C.ZSETS), t * tm.shape[0] * tm.shape[1])))or t == 1
        if t == 64:
            j = torch.arange(t)
            for n, z in enumerate(C.ZSETS):
                group = tm[zi == n]
                assert bool((group.sum(-1) == 2 ** len(z)).all())
                for bit in z:
                    assert bool(((group & (((j >> bit) & 1) == 0)).any(-1) & (group & (((j >> bit) & 1) == 1)).any(-1)).all())


# ------------------------------------------------------------------------------------------- 2. the order of the score steps
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("t", C.ORDER_T)
@pytest.mark.parametrize("kind", C.ORDER_KINDS)
def test_order_probes_tie_under_the_pinned_order_only(kind, t, d):
    c = C.order_case(kind, t, d)
    q, k, v = c["q"], c["k"], c["v"]
    b, h = q.shape[:2]
    assert b * h == 8 and f16_exact(q, k, v) and C.ORDER_T == (37, 64)
    keys = [x for pair in C.ORDER_PAIRS for x in pair]
    assert len(set(keys)) == 16 and max(keys) < 37
    assert any((a ^ bb) == 1 for a, bb in C.ORDER_PAIRS) and any((a ^ bb) & 4 for a, bb in C.ORDER_PAIRS)       # a quad's neighbours, the lane halves
    assert any((a ^ bb) & 32 for a, bb in C.ORDER_PAIRS) and any(a >= 32 and bb >= 32 for a, bb in C.ORDER_PAIRS)      # across the blocks, inside block 1
    a64 = q.double() @ k.double().transpose(-1, -2)
    assert float(a64.abs().max()) < 2 ** 26 and torch.equal(a64.float().double(), a64)      # an fp32 number whatever the order of two exact products
    s32, _ = C.score_steps(q, k, c["scale"], c["bias"], c["mask"])
    s32 = torch.from_numpy(s32)
    ka, kb = (c[n][..., None, None].expand(b, h, t, 1) for n in ("a_key", "b_key"))
    sa, sb = s32.gather(-1, ka)[..., 0], s32.gather(-1, kb)[..., 0]
    assert torch.equal(sa, sb) and torch.equal(sa, c["pinned"]), "keys A and B do not tie under the pinned order"
    live = torch.zeros(b, h, t, t, dtype=torch.bool).scatter_(-1, ka, True).scatter_(-1, kb, True)
    assert float((sa[..., None].double() - s32.double())[~live].min()) >= 200
    assert not bool(k.gather(2, c["b_key"][..., None, None].expand(b, h, 1, d)).any())      # k_B = 0: its score is the term's value as placed
    a, bias_a, mask_a = (None if x is None else x.numpy() for x in c["parts"])
    models = C.order_models(a, c["scale"], bias_a, mask_a)
    assert np.array_equal(models["pinned"], sa.numpy())
    apart = {n: float(np.abs(s.astype(np.float64) - models["pinned"].astype(np.float64)).min()) for n, s in models.items() if n != "pinned"}
    print(f"{kind} T = {t} D = {d}: the least |alternative - pinned| over the {b * h * t} probe rows: {apart}")
    assert apart[C.ORDER_TARGET[kind]] >= 1
    sums = c["want"] * 2
    assert torch.equal(sums, sums.round()) and float(sums.max()) < 2 ** 24


def test_every_alternative_order_has_a_construction():
    assert set(C.ORDER_TARGET.values()) == {"mask_first", "terms_first", "fma"} and set(C.ORDER_TARGET) == set(C.ORDER_KINDS)
    # the construction first proposed for the FMA (2^24 + 2 m, bias -2^24) stays just under 1 apart: why it was replaced
    m = np.arange(1, 2049, dtype=np.float32)
    old = C.order_models(np.float32(2 ** 24) + 2 * m, 1 - 2.0 ** -24, np.full(2048, -2.0 ** 24, np.float32), None)
    assert np.array_equal(old["pinned"], 2 * m - 2) and float(np.abs(old["fma"] - old["pinned"]).max()) < 1


# ------------------------------------------------------------------------------------------- 3. uniform rows, placement
def padded_operands(c):
    """The case's tensors as the GPU test launches them: q, k, v views of NaN-filled parents, the terms views of NaN-filled parents with a
    row stride of roundup4(T) + 8."""
    t = c["q"].shape[2]
    qkv = [C.row_parent(c[n])[:, :, 1:t + 1] for n in "qkv"]
    terms = [None if c[n] is None else C.term_view(C.term_parent(c[n], float("nan")), t) for n in ("bias", "mask")]
    return qkv, terms


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("terms", C.TERMS)
def test_uniform_rows(terms, d):
    assert C.ALL_T == tuple(range(1, 65)) and C.UNIFORM_BH == (1, 5)
    for t in C.ALL_T:
        c = C.uniform_case(t, d, terms)
        q, k, v = c["q"], c["k"], c["v"]
        assert tuple(v.shape) == (1, 5, t, d) and not bool(q.any()) and f16_exact(k, v) and float(v.max()) * t < 2 ** 24
        assert (c["bias"] is not None) == ("bias" in terms) and (c["mask"] is not None) == ("mask" in terms)
        s32, s64 = exact_scores(c)
        assert bool((s32 == s32[..., :1]).all()) and torch.equal(s32.double(), s64)      # every score of a row the same fp32 number
        assert torch.equal(c["total"].double(), v.double().sum(2)) and torch.equal(c["want"], (v.double().sum(2) / t).float()[0])
        qkv, views = padded_operands(c)
        for x, dense in zip(qkv, (q, k, v)):
            assert torch.equal(x, dense) and bool(x._base[:, :, 0].isnan().all()) and bool(x._base[:, :, -1].isnan().all())
            assert K.window_attention_views(*qkv)
        for x in views:
            if x is not None:
                assert x.stride(-2) == C.roundup4(t) + 8 and int(x._base.isnan().sum()) == x._base.numel() - x.numel()
                assert K.window_term_view(x, t) is not None      # read in place


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("terms", C.TERMS)
def test_placement(terms, d):
    b, h, nw = C.PLACE_BHW
    assert b * h <= 12 and b // nw > 1
    for t in C.ALL_T:
        c = C.placement_case(t, d, terms)
        assert f16_exact(c["q"], c["k"], c["v"])
        s32, s64 = exact_scores(c)
        top = s32.topk(min(2, t), dim=-1)
        assert torch.equal(top.indices[..., 0], c["sel"]) and (t == 1 or float((top.values[..., 0] - top.values[..., 1]).min()) >= 150)
        assert torch.equal(s32.double(), s64)
        for n, rows in (("bias", h), ("mask", nw)):
            if c[n] is not None and t > 2:
                assert tuple(c[n].shape) == (rows, t, t) and not torch.equal(c[n], c[n].transpose(1, 2)) and not torch.equal(c[n][0], c[n][1])
        assert torch.equal(c["want"], torch.gather(c["v"], 2, c["sel"][..., None].expand_as(c["v"])))
        if t in (49, 64):      # the selected key differs between heads, and between windows where a mask decides
            assert not torch.equal(c["sel"][0, 0], c["sel"][0, 1]) or terms == "mask"
            assert not torch.equal(c["sel"][0, 0], c["sel"][1, 0]) or terms == "bias"
            assert torch.equal(c["sel"][0], c["sel"][2]) or terms == "none"      # b % nW


# ------------------------------------------------------------------------------------------- 4. the probe
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("place", sorted(C.PROBE_PLACES))
@pytest.mark.parametrize("variant", C.PROBE_VARIANTS)
def test_probe_scores_are_the_grid(variant, place, d):
    c = C.probe_case(d, variant, place)
    x = C.probe_grid()
    assert C.PROBE_BHT == (2, 4, 64) and torch.equal(c["x"].reshape(-1), x) and float(x[0]) == -0.125 and float(x[-1]) == -64.0
    assert f16_exact(c["q"], c["k"], c["v"]) and C.PROBE_PLACES == {"half": 4, "block": 32}
    a = c["q"].double() @ c["k"].double().transpose(-1, -2)
    s32, _ = C.score_steps(c["q"], c["k"], c["scale"], c["bias"], c["mask"])
    s32, s64 = torch.from_numpy(s32), C.scores64(c["q"], c["k"], c["scale"], c["bias"], c["mask"])
    assert torch.equal(a.float().double(), a) and torch.equal(s32.double(), s64)      # no step rounds
    second = c["second"]
    assert torch.equal(s64[..., second], c["x"]) and not bool(s64[..., 0].any())
    dead = [j for j in range(64) if j not in (0, second)]
    assert float(s64[..., dead].max()) <= -1000 and bool((c["v"][:, :, dead] == 3).all())
    assert bool((c["v"][:, :, second] == 1).all()) and not bool(c["v"][:, :, 0].any())
    assert (variant == "terms") == (not bool(c["q"].any())) and (variant == "terms") == (c["bias"] is not None)
    assert torch.equal(c["ref"], torch.exp(c["x"]) / (1 + torch.exp(c["x"])))


def test_probe_models():
    """fp32 kernel: the correctly rounded expf stays inside 4 u on the whole grid and v_exp_f32 on a pre-scaled argument does not.  f16
    kernel: its order with a correctly rounded exp2, and with every exp2 one ulp off either way, stays inside `probe_tol_f16`; the same
    with l summed from the unrounded weights does not."""
    x64 = C.probe_grid()
    x = x64.numpy()
    e = np.exp(x)
    ref = e / (1 + e)
    worst = {}
    for name, fn in (("rounded", C.exp_rounded), ("exp2_prescaled", C.exp2_prescaled)):
        out = C.probe_model(x, "block0", fn).astype(np.float64)
        worst[name] = float(np.max(np.abs(out - ref) / ref)) / U
    print(f"fp32 probe, max relative error in u = 2^-24 (tolerance 4): {({k: round(v, 2) for k, v in worst.items()})}")
    assert C.PROBE_TOL == 4 * U and worst["rounded"] < 4 and worst["exp2_prescaled"] > 4
    tol = C.probe_tol_f16(x64).numpy()
    up, down = (lambda t: np.nextafter(C.exp2_rounded(t), np.float32(np.inf))), (lambda t: np.nextafter(C.exp2_rounded(t), np.float32(0)))
    ratio = {}
    for name, fn in (("rounded", C.exp2_rounded), ("up", up), ("down", down)):
        for rounded_l in (True, False):
            out = C.probe_model_f16(x, fn, rounded_l).astype(np.float64)
            ratio[name, rounded_l] = np.abs(out - ref) / tol
    print("f16 probe, max |model - ref| / tolerance: " + ", ".join(
        f"{n} exp2, l of the {'rounded' if r else 'UNROUNDED'} weights: {float(v.max()):.3f} ({int((v > 1).sum())} points over)" for (n, r), v in ratio.items()))
    for name in ("rounded", "up", "down"):
        assert float(ratio[name, True].max()) <= 1 and int((ratio[name, False] > 1).sum()) >= 1
    assert float(tol.max()) < 2.0 ** -11 and np.all(tol[e < 2.0 ** -26] <= 2.0 ** -25 * 1.001)      # never looser than one f16 rounding of the weight


# ------------------------------------------------------------------------------------------- 5. non-finite values
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("kind", C.PLANT_KINDS + C.PLANT_KINDS_F16)
def test_planted_masks_are_torch_s(kind, d):
    b, h, t, nw = C.PLANT_SHAPE
    assert (b, h, t, nw) == (2, 3, 49, 2)
    pos = C.plant_positions(d)
    assert {(p[2] >> 2) & 1 for p in pos} == {0, 1} and {p[2] >> 5 for p in pos} == {0, 1} and {p[3] >> 5 for p in pos} == set(range(d // 32))
    for which in range(len(pos)):
        c = C.plant_case(kind, d, which)
        big = kind.startswith("big")
        q, k, v = ((c[n].half().float() if big else c[n]) for n in "qkv")
        ref = C.torch_graph(q, k, v, c["scale"], c["bias"], c["mask"])
        bad = ~torch.isfinite(ref) if big else ref.isnan()
        assert torch.equal(bad, c["hit"]), f"{kind} at {c['at']}: the case's mask is not torch's"
        assert bool(torch.isfinite(ref[~c["hit"]]).all()) and 0 < int(c["hit"].sum()) < c["hit"].numel()
        n_bad = sum(int((~torch.isfinite(c[n]) | (c[n].abs() > 65504)).sum()) for n in ("q", "k", "v", "bias"))
        assert n_bad == 1      # one planted value
        if kind == "big_k":
            rows = c["hit"][c["at"][0], c["at"][1], :, 0]
            assert 5 < int(rows.sum()) < t - 5      # rows of either sign: NaN rows and rows that lose the key


# ------------------------------------------------------------------------------------------- 6 .. 8. views and n01 cases
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("t", C.STORE_T)
def test_padded_output_view_is_one_the_entry_points_take(t, d):
    b, h = C.STORE_BH
    assert (b, h) == (1, 5) and C.STORE_T == (1, 33, 49)
    shape, off, (sb, sh, st) = C.padded(b, h, t, d)
    assert shape == (b, t + 2, h * d + 8) and off == shape[2] + 4 and (sb, sh, st) == (shape[1] * shape[2], d, shape[2])
    assert (4 * off) % 16 == 0 and all(s % 4 == 0 for s in (sb, sh, st)) and st >= d
    parent = torch.arange(shape[0] * shape[1] * shape[2]).reshape(shape)
    view = parent[:, 1:t + 1, 4:4 + h * d]
    assert view.storage_offset() == off and (t == 1 or view.stride() == (sb, st, 1)) and int(view[b - 1, t - 1, h * d - 1]) < parent.numel() - shape[2]


@pytest.mark.parametrize("d", DIMS)
def test_independence_tile_and_the_inf_tail(d):
    b, h, t = C.INDEP_BHT
    c = C.indep_tile(d)
    assert (b, h, t) == (3, 3, 49) and tuple(c["q"].shape) == (t, d) and tuple(c["bias"].shape) == (1, t, t) and tuple(c["mask"].shape) == (1, t, t)
    assert not torch.equal(c["other_v"][0, 0], c["v"]) and bool(torch.isfinite(c["other_k"]).all())
    for shape in C.BOUND_SHAPES:
        bb, hh, tt, nw = shape
        m = C.inf_tail_case(shape, d)
        assert bb * hh <= 12 and tt in (33, 49) and m["first_inf"] == 4 * ((tt - 1) // 4) and m["first_inf"] + 4 >= tt
        assert bool((m["mask"][:, :, m["first_inf"]:] == float("-inf")).all()) and bool(torch.isfinite(m["mask"][:, :, :m["first_inf"]]).all())
        parent = C.term_parent(m["mask"], float("-inf"))
        view = C.term_view(parent, tt)
        assert K.window_term_view(view, tt) is not None and torch.equal(view, m["mask"])
        row = parent[:, 1:tt + 1]
        assert bool((row[:, :, 4 + m["first_inf"]:] == float("-inf")).all())      # the last piece, whole, and every piece after it
