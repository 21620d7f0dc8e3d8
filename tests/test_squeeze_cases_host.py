"""tests/squeeze_cases.py on the CPU: every case holds the facts it states, so that tests/test_gpu_squeeze_exact.py compares what it
says it compares.  The shapes land in the instantiation and trip counts written beside them; every stage of the reference is one rounding
of an exactly known number (exact_layers.exact_fma asserts it inside `reference`, for every element) and agrees with a float64 product
of the dequantised operands; a quarter of the hidden codes lie inside the range and both bounds occur; the saturating cases pass 2^24 and
need the rounding; every edge value arrives as a hidden value and as a gate argument; the selector channels give the codes back; no
int32 sum can overflow."""
import pytest
import torch

import exact_layers as X
import squeeze_cases as Q

IDS = [c.cid for c in Q.CASES]


def test_shapes_land_where_the_table_says():
    for (n, c, r4), want in Q.SHAPES.items():
        assert Q.shape_facts(c, r4) == want, (n, c, r4, Q.shape_facts(c, r4))
        assert c % 4 == 0 and r4 % 4 == 0 and 4 <= c <= 2048 and 4 <= r4 <= 512
    pairs = {}
    for (n, c, r4), want in Q.SHAPES.items():
        pairs.setdefault(want[0], []).append(c)
    assert set(pairs) == {(a, b) for a in (True, False) for b in (True, False)}
    assert all(max(cs) > 256 for cs in pairs.values())                      # a second trip of layer 2's thread loop in each instantiation
    assert {c for _, c, _ in Q.SHAPES} >= {16, 240, 256, 272, 2048, 4, 20, 60, 68, 2044}
    assert {r for _, _, r in Q.SHAPES} >= {16, 32, 272, 512, 4, 8, 20, 260}
    assert {n for n, _, _ in Q.SHAPES} == {1, 3, 4, 5, 9}
    # the loop trips the table exists for
    assert {w[1] for w in Q.SHAPES.values()} >= {1, 2, 8, 32} and {w[3] for w in Q.SHAPES.values()} == {1, 2}
    assert {w[2] for w in Q.SHAPES.values()} >= {1, 2, 17, 32} and {w[4] for w in Q.SHAPES.values()} >= {1, 2, 8}


def test_quantisers_of_the_table():
    qs = [c.quant for c in Q.CASES]
    assert all(not q.shift128 for q in qs)
    want = [q for q in X.plain_quants() + X.nonplain_quants() if not q.shift128]
    assert len(want) == 20 and all(q in qs for q in want)
    for form in range(4):
        for rng in ((0, 255), (-128, 127), (0, 15), (-8, 7), (-127, 127)):
            assert any(q.form == form and (q.lo, q.hi) == rng and q.zp not in (None, 0.0) for q in qs), (form, rng)
    g = Q.qbase_g_quant()
    assert g in qs and g.g > 0 and X.dequant_scale(g) != float(X.f32(g.scale))      # s_h != s: a kernel that dequantised with s shows
    assert {c.kind for c in Q.CASES} == {"table", "sat1", "sat2", "mixed"}
    assert {c.uns for c in Q.CASES if c.kind == "sat1"} == {True, False} and all(c.c == 2048 for c in Q.CASES if c.kind == "sat1")
    (s2,) = [c for c in Q.CASES if c.kind == "sat2"]
    assert s2.r4 == 512 and s2.quant.lo >= 0 and s2.quant.zp < 0
    (m,) = [c for c in Q.CASES if c.kind == "mixed"]
    assert m.quant.lo < 0 and m.quant.hi > 127


@pytest.mark.parametrize("cid", IDS)
def test_case_holds_its_facts(cid):
    case, ops = Q.BY_ID[cid], Q.operands(cid)
    q = case.quant
    # ---- the operands
    codes = ops["codes"]
    assert codes.dtype == (torch.uint8 if case.uns else torch.int8) and (ops["zp1"] not in (0, 128) if case.uns else ops["zp1"] != 0)
    if codes.numel() >= 4096:
        assert codes.long().unique().numel() == 256
    assert int(ops["w1"].long().abs().max()) <= 127 and int(ops["w2"].long().abs().max()) <= 127
    assert not bool(ops["w1"][:ops["nz1"]].any()) and ops["nz1"] >= 1
    sel, nz2 = ops["sel"], ops["nz2"]
    assert sel == min(case.r4, case.c) and torch.equal(ops["w2"][:sel, :sel], torch.eye(sel, dtype=torch.int8)) and not bool(ops["w2"][:sel, sel:].any())
    assert bool((ops["ws2"][:sel] == 1).all()) and not bool(ops["w2"][sel:sel + nz2].any())
    assert (ops["b1"] is None) == (ops["b2"] is None) == (not case.bias) and (ops["b2"] is None or not bool(ops["b2"][:sel].any()))
    for s in (torch.tensor([ops["s_in"]]), ops["ws1"], ops["ws2"]):         # powers of two
        m, _ = torch.frexp(s.abs())
        assert bool((m == 0.5).all())
    assert ops["ws1"][ops["nz1"]:].abs().unique().numel() == min(3, case.r4 - ops["nz1"])
    if case.c - sel - nz2 >= 5 and not ops["selector_only"]:
        assert ops["ws2"][sel + nz2:].unique().numel() == 5
    # the degenerate scale whose product with a power of two is no fp32 number keeps the selector block alone (none needs it today)
    mult = X.dequant_scale(q) * ops["ws2"].double()
    assert bool((mult.float().double() == mult).all()) and (not ops["selector_only"] or not bool(ops["w2"][sel:].any()))
    # ---- the share inside the range, the clamps, the saturation
    share, lo, hi = Q.hidden_facts(case, ops)
    assert share >= 0.25 and lo and hi, (cid, share, lo, hi)
    sat = Q.saturation_facts(case, ops)
    if case.kind in ("sat1", "sat2"):
        assert sat[0] > 2 ** 24 and sat[1] >= 1, (cid, sat)
    assert Q.int32_bound(case, ops) < 2 ** 31
    # ---- the reference: staged (every fma asserted exact inside) against a float64 product of the dequantised operands
    for inner in (None, "relu"):
        ref = Q.reference(cid, inner)
        s1, s2 = ref["s1"], ref["s2"]
        assert int(s1.abs().max()) <= Q.int32_bound(case, ops) and int(s2.abs().max()) <= Q.int32_bound(case, ops)
        b1 = 0.0 if ops["b1"] is None else ops["b1"].double()
        y1 = ((codes.double() - ops["zp1"]) * ops["s_in"]) @ (ops["w1"].double() * ops["ws1"].double().reshape(-1, 1)).t() + b1
        y1 = torch.where(y1 < 0, torch.zeros_like(y1), y1) if inner == "relu" else y1
        fits1 = (s1.abs() < 2 ** 24)
        same1 = (y1.float() == ref["h"]) | (y1.isnan() & ref["h"].isnan())
        assert bool((same1 | ~fits1).all()) and (case.kind == "sat1" or bool(fits1.all()))
        b2 = 0.0 if ops["b2"] is None else ops["b2"].double()
        y2 = ((ref["qh"] - Q.zp2_of(q)).double() * X.dequant_scale(q)) @ (ops["w2"].double() * ops["ws2"].double().reshape(-1, 1)).t() + b2
        fits2 = (s2.abs() < 2 ** 24)
        same2 = (y2.float() == ref["v"]) | (y2.isnan() & ref["v"].isnan())
        assert bool((same2 | ~fits2).all()) and (case.kind == "sat2" or bool(fits2.all()))
        # the selector channels: fl32((qh - zp2) * s_h), and the codes back out of them
        back = ref["v"][:, :sel].double()
        want = ((ref["qh"][:, :sel] - Q.zp2_of(q)).double() * X.dequant_scale(q)).float().double()
        assert torch.equal(back, want)
        if X.dequant_scale(q) >= 2.0 ** -126:
            assert torch.equal(torch.round(back / X.dequant_scale(q)).long() + Q.zp2_of(q), ref["qh"][:, :sel])
        assert int(ref["qh"].min()) >= q.lo and int(ref["qh"].max()) <= q.hi
    if case.kind == "mixed":
        assert int(Q.reference(cid, None)["qh"].max()) > 127 and int(Q.reference(cid, None)["qh"].min()) < 0


def _bits(values):
    return {int(torch.tensor(v, dtype=torch.float32).view(torch.int32)) for v in values}


def test_every_edge_value_arrives_as_a_hidden_value_and_as_a_gate_argument():
    want = _bits(X.EDGE_VALUES)
    assert len(X.EDGE_VALUES) == Q.NEDGE == 51
    seen_h, seen_v = set(), set()
    for case in Q.RUN:
        if not case.bias:
            continue
        ops, ref = Q.operands(case.cid), Q.reference(case.cid, None)
        seen_h |= set(ref["h"][:, :ops["nz1"]].contiguous().view(torch.int32).flatten().tolist())
        seen_v |= set(ref["v"][:, ops["sel"]:ops["sel"] + ops["nz2"]].contiguous().view(torch.int32).flatten().tolist())
    nan = int(torch.tensor(float("nan")).view(torch.int32))
    assert want - {nan} <= seen_h and want - {nan} <= seen_v          # -0 included: its bits differ from +0's
    for case in Q.RUN:                                                # NaN: by value (its payload is not compared)
        ref, ops = Q.reference(case.cid, None), Q.operands(case.cid)
        if case.bias and ops["nz1"] >= 1 and bool(ref["h"].isnan().any()) and bool(ref["v"].isnan().any()):
            break
    else:
        raise AssertionError("no case has a NaN hidden value and a NaN gate argument")


def test_relu_passes_nan_and_negative_zero():
    hit = 0
    for case in Q.RUN:
        h = Q.reference(case.cid, "relu")["h"]
        neg0 = (h == 0) & torch.signbit(h)
        hit += int(bool(neg0.any()) and bool(h.isnan().any()))
        assert not bool((h < 0).any())
    assert hit >= 3
