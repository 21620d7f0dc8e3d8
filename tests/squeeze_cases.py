"""The calls of the squeeze kernel - csrc/squeeze_i8.hip: squeeze_gate_kernel<V1, V2>, dlmcq_squeeze_gate_i8 - that its four instantiations,
its loop trips, the hidden quantiser's forms and the epilogue's hard values need, with their float64 reference: ONE table for
tests/test_squeeze_cases_host.py (what each case states about itself, on the CPU) and tests/test_gpu_squeeze_exact.py (the same calls
launched through the raw entry point and compared byte for byte).  TEST INFRASTRUCTURE ONLY.

Operands of a case (`operands`), built on tests/exact_layers.py:
  input codes  uniform over all 256 byte values; uint8 with an integer zero point other than 0 and 128, int8 with a non-zero one.
  w1, w2       uniform in +-127, zero on the edge units [0, nz1) of layer 1 and the edge channels [sel, sel + nz2) of layer 2.  The SELECTOR
               block of w2 reads each hidden code back on its own: channel c < sel = min(R4, C) has w2[c, r] = (c == r), w_scale2[c] = 1
               and bias 0, so gate[n, c] = fl32((qh[n, c] - zp2) * s_h).
  scales       every one a power of two, different from unit to unit: in_scale1 * w_scale1[r] = 2^(e1 - r % 3) with e1 sized from the
               shape (exact_layers.full_range_sigma) so that the widest units' hidden values spread over one width of the hidden
               quantiser's code range about its middle: a good share inside, both clamps reached (`hidden_facts`, asserted per case);
               w_scale2[c] = 2^(e2 - c % 5) sized as exact_layers.make_full_range_second sizes its own (from the reference's codes' second
               moment, output sigma FULL_TARGET_SIGMA).  The hidden quantiser's scale is whatever the quantiser has (3, 7, 0.1, 1e-30,
               1e-41, ...): s_h * w_scale2[c] stays an exact fp32 number because w_scale2 is a power of two (asserted; a case where it is
               not keeps the selector block alone: `selector_only`).
  bias1        edge units: exact_layers.EDGE_VALUES (all 51 where R4 >= 260, a window that moves from case to case where R4 is narrow -
               nz1 = R4 // 4, the narrow widths' own placement); h IS the bias there.  The unit that carries -0 has a NEGATIVE weight scale:
               fma(+0, -u, -0) = -0, where a positive one would give +0.  Live units: off + s (k + f), f the tie fractions against the
               hidden quantiser's scale, k integers about the middle of its range.
  bias2        the same edge values on the edge channels (the gate functions see them), dyadic values on the live ones.
  NULL biases  three cases (`bias=False`), in three shapes.
  saturating   `sat1` (C = 2048, one per input signedness): image 0's codes sit at the end of the byte range that matches the sign of the
               weight under them for units nz1 (weights +127 p) and nz1 + 1 (-127 p): |S1| > 2^24 and fl32(S1) != S1.  `sat2` (R4 = 512,
               unsigned hidden codes, zero point -200): channels sel + nz2 (+127) and sel + nz2 + 1 (-127): |S2| > 2^24, fl32(S2) != S2.
  mixed        the range -1 .. 200, neither a uint8 nor an int8 one: refused by the entry point; its operands and
               reference are kept, the reference being what the header's arithmetic gives for it.

The reference (`first_half`, `second_half`), float64 from the integers, every fma through exact_layers.exact_fma (one rounding of an
exactly known number, asserted for every element):
  S1 = SUM (x - zp1) w1 (exact)    pre = fl32(fl32(S1) * unit1 + b1)    h = pre | pre < 0 ? 0 : pre  (swish: the kernel's own hidden)
  qh = the oracle's codes of h (exact_layers.code_ints; NaN -> 0)       S2 = SUM (qh - zp2) w2, zp2 = the rounded zero point in every form
  s_h = exact_layers.dequant_scale (QBASE: (s - s g) + s g in fp32)     v = fl32(fl32(S2) * (s_h * w_scale2) + b2)"""
import functools
import math
from dataclasses import dataclass

import torch

import exact_layers as X

G, BLOCK, LANES = 4, 256, 16          # DLMCQ_SQUEEZE_IMAGES, DLMCQ_BLOCK, lanes per hidden unit (csrc/squeeze_i8.hip)
NEDGE = len(X.EDGE_VALUES)
INNER = (None, "relu", "swish")

# (N, C, R4): (V1, V2), trips of layer 1's piece loop (the busiest lane), of the hidden-unit loop, of the code4 loop, of layer 2's thread loop
SHAPES = {
    (1, 16, 16): ((True, True), 1, 1, 1, 1),        # C = 16: lane 0 alone has a piece; one image: three rows of the group are zeros
    (4, 256, 32): ((True, True), 1, 2, 1, 1),       # every lane one 16-byte piece, a full group, two trips of the unit loop
    (5, 272, 272): ((True, True), 2, 17, 2, 2),     # lane 0 alone makes a second trip; R4 > 256: code4's second trip; C > 256
    (9, 2048, 512): ((True, True), 8, 32, 2, 8),    # the limits: eight trips, three workgroups, the last with one image
    (3, 240, 4): ((True, False), 1, 1, 1, 1),       # a ragged first trip (lanes 0 .. 14), the narrowest hidden layer, a partial group
    (5, 272, 260): ((True, False), 2, 17, 2, 2),    # 4-byte pieces in layer 2 with a second code4 trip; C > 256
    (4, 2048, 20): ((True, False), 8, 2, 1, 8),
    (3, 4, 16): ((False, True), 1, 1, 1, 1),        # C = 4: one 4-byte piece in lane 0
    (5, 60, 32): ((False, True), 1, 2, 1, 1),       # lanes 0 .. 14 at PB = 4
    (9, 2044, 272): ((False, True), 32, 17, 2, 8),  # a ragged last trip at PB = 4 (lanes 0 .. 14); C > 256
    (1, 20, 8): ((False, False), 1, 1, 1, 1),       # lanes 0 .. 4
    (4, 68, 20): ((False, False), 2, 2, 1, 1),      # lane 0 alone makes a second trip at PB = 4
    (5, 2044, 260): ((False, False), 32, 17, 2, 8),
    (9, 4, 4): ((False, False), 1, 1, 1, 1),        # the smallest call, three workgroups
}
SHAPE_LIST = list(SHAPES)


def shape_facts(c, r4):
    """The instantiation and trip counts of a shape, restated from the kernel's loops."""
    v1, v2 = c % 16 == 0, r4 % 16 == 0
    pb = 16 if v1 else 4
    return (v1, v2), -(-c // (LANES * pb)), -(-r4 // (BLOCK // LANES)), -(-(G * r4 // 4) // BLOCK), -(-c // BLOCK)


def qbase_g_quant():
    """A QBASE quantiser with g > 0 whose dequantising scale (s - s g) + s g differs from s in fp32 (a power-of-two s never does: the
    first (s, g) of a fixed grid that does)."""
    for s in (0.1, 0.043, 0.189, 0.027):
        for g in (0.02, 0.3):
            q = X.Quant(s, 3.0, 0, 255, X.FORM_QBASE, g=g)
            if X.dequant_scale(q) != float(X.f32(s)):
                return q
    raise AssertionError("no (s, g) of the grid has (s - s g) + s g != s")


def form_quants():
    """The four forms, each with a non-zero zero point, at unsigned and signed 8-bit and sub-byte ranges."""
    out = []
    for lo, hi, z in ((0, 255, 7.0), (-128, 127, -5.0), (0, 15, 3.0), (-8, 7, 2.0), (-127, 127, 5.0)):
        for form, s in ((X.FORM_EMULATE, 0.031), (X.FORM_QBASE, 2.0 ** -4), (X.FORM_ZEROPOINT, 2.0 ** -3), (X.FORM_SYMMETRIC, 2.0 ** -5)):
            out.append(X.Quant(s, z, lo, hi, form, g=0.02 if form == X.FORM_QBASE and lo == 0 else 0.0))
    return out


@dataclass(frozen=True)
class Case:
    cid: str
    n: int
    c: int
    r4: int
    uns: bool              # uint8 input codes
    quant: X.Quant
    bias: bool = True
    kind: str = "table"    # "table" | "sat1" | "sat2" | "mixed"


def _cases():
    quants = [q for q in X.plain_quants() + X.nonplain_quants() if not q.shift128] + form_quants() + [qbase_g_quant()]
    out = []
    for i, q in enumerate(quants):
        n, c, r4 = SHAPE_LIST[i % len(SHAPE_LIST)]
        out.append(Case(f"{i:02d}_{n}x{c}x{r4}_{q.tag()}", n, c, r4, (i + i // len(SHAPE_LIST)) % 2 == 0, q, bias=i not in (3, 18, 38)))
    out.append(Case("sat1_u8", 4, 2048, 16, True, X.Quant(2.0 ** -3, 7.0, 0, 255, X.FORM_ZEROPOINT), kind="sat1"))
    out.append(Case("sat1_s8", 5, 2048, 20, False, X.Quant(2.0 ** -3, -5.0, -128, 127, X.FORM_ZEROPOINT), kind="sat1"))
    out.append(Case("sat2", 3, 516, 512, True, X.Quant(2.0 ** -3, -200.0, 0, 255, X.FORM_ZEROPOINT), kind="sat2"))
    out.append(Case("mixed", 5, 32, 16, True, X.Quant(2.0 ** -3, 3.0, -1, 200, X.FORM_ZEROPOINT), kind="mixed"))
    return out


CASES = _cases()
BY_ID = {c.cid: c for c in CASES}
RUN = [c for c in CASES if c.kind != "mixed"]          # the cases the entry point takes
assert len(BY_ID) == len(CASES) and {(c.n, c.c, c.r4) for c in CASES if c.kind == "table"} == set(SHAPES)
assert sum(not c.bias for c in CASES) == 3 and len({(c.n, c.c, c.r4) for c in CASES if not c.bias}) == 3


def zp2_of(q):
    return 0 if q.zp is None else int(round(q.zp))


def hidden_window(q):
    """(value of the middle of the code range, width of the range in values, the offset the form subtracts before it divides)."""
    z = 0.0 if q.zp is None else q.zp
    s, mid = float(X.f32(q.scale)), 0.5 * (q.lo + q.hi)
    if q.form in (X.FORM_EMULATE, X.FORM_QBASE):
        return z + mid * s, (q.hi - q.lo) * s, z
    return ((mid - z) if q.form == X.FORM_ZEROPOINT else mid) * s, (q.hi - q.lo) * s, 0.0


def _edge_bias(b, ws, first, count, start):
    """EDGE_VALUES[start ...] (cycled) into b[first : first + count]; the scale of the entry that carries -0 becomes negative."""
    for i in range(count):
        v = X.EDGE_VALUES[(start + i) % NEDGE]
        b[first + i] = v
        if v == 0.0 and math.copysign(1.0, v) < 0:
            ws[first + i] = -ws[first + i]


def _pow2(e):
    return X.exact_f32(2.0 ** e.double() if isinstance(e, torch.Tensor) else torch.tensor(2.0 ** e, dtype=torch.float64), "a scale")


def _layer1(case, gen, idx):
    n, c, r4, q = case.n, case.c, case.r4, case.quant
    if case.uns:
        codes = torch.randint(0, 256, (n, c), generator=gen).to(torch.uint8)
        d = int(torch.randint(1, 127, (1,), generator=gen))
        zp1 = 128 + d if bool(torch.randint(0, 2, (1,), generator=gen)) else 128 - d
    else:
        codes = torch.randint(-128, 128, (n, c), generator=gen).to(torch.int8)
        zp1 = int(torch.randint(1, 100, (1,), generator=gen)) * (1 if bool(torch.randint(0, 2, (1,), generator=gen)) else -1)
    nz1 = min(NEDGE, r4 // 4)
    w1 = torch.randint(-127, 128, (r4, c), generator=gen).to(torch.int8)
    w1[:nz1] = 0
    centre, width, off = hidden_window(q)
    s = float(X.f32(q.scale))
    e1 = round(math.log2(width / X.full_range_sigma(c, not case.uns, zp1)))
    unit = 2.0 ** (e1 - torch.arange(r4) % 3).double()
    e_in = -(-e1 // 2)
    s_in = float(_pow2(e_in))
    ws1 = _pow2(e1 - e_in - torch.arange(r4) % 3)
    assert bool((s_in * ws1.double() == unit).all()) and s_in != 1.0
    live = r4 - nz1
    idxs = torch.arange(live)
    frac = torch.tensor(X.TIE_FRACTIONS, dtype=torch.float64)[idxs % len(X.TIE_FRACTIONS)]
    k = round((centre - off) / s) + torch.randint(-3, 4, (live,), generator=gen).double()
    b1 = torch.zeros(r4, dtype=torch.float32)
    b1[nz1:] = (off + s * (k + frac)).float()
    if case.kind == "sat1":       # image 0 against units nz1 (+127 p) and nz1 + 1 (-127 p); no bias there: h = fl32(S1) * unit exactly
        p = torch.where(torch.rand(c, generator=gen) < 0.5, -1, 1)
        lo_c, hi_c = (0, 255) if case.uns else (-128, 127)
        codes[0] = torch.where(p > 0, hi_c, lo_c).to(codes.dtype)
        w1[nz1], w1[nz1 + 1] = (127 * p).to(torch.int8), (-127 * p).to(torch.int8)
        b1[nz1:nz1 + 2] = 0.0
    _edge_bias(b1, ws1, 0, nz1, 7 * idx)
    return dict(codes=codes, zp1=zp1, w1=w1, s_in=s_in, ws1=ws1, b1=b1 if case.bias else None, nz1=nz1)


def first_half(ops, inner):
    """(S1 int64, pre fp32: the hidden value before the activation, h fp32 behind it - None for swish)."""
    s1 = ((ops["codes"].double() - ops["zp1"]) @ ops["w1"].double().t())
    b1 = torch.zeros(ops["w1"].shape[0], dtype=torch.float64) if ops["b1"] is None else ops["b1"].double()
    pre = X.exact_fma(s1.float().double(), (ops["s_in"] * ops["ws1"].double()).reshape(1, -1), b1.reshape(1, -1), "layer 1")
    if inner == "relu":
        h = torch.where(pre < 0, torch.zeros_like(pre), pre)
    else:
        h = pre if inner is None else None
    return s1.long(), pre, h


def second_half(ops, q, hidden):
    """(qh int64, S2 int64, v fp32) of fp32 hidden values - the reference's, or a launch's own."""
    qh = X.code_ints(hidden, q)
    s2 = ((qh - zp2_of(q)).double() @ ops["w2"].double().t())
    b2 = torch.zeros(ops["w2"].shape[0], dtype=torch.float64) if ops["b2"] is None else ops["b2"].double()
    mult = X.exact_f32(X.dequant_scale(q) * ops["ws2"].double(), "s_h * w_scale2")
    v = X.exact_fma(s2.float().double(), mult.double().reshape(1, -1), b2.reshape(1, -1), "layer 2")
    return qh, s2.long(), v


def _layer2(case, gen, idx, ops):
    c, r4, q = case.c, case.r4, case.quant
    sel = min(r4, c)
    rest = c - sel
    nz2 = min(NEDGE, max(1, rest // 4)) if rest else 0
    w2 = torch.randint(-127, 128, (c, r4), generator=gen).to(torch.int8)
    w2[:sel + nz2] = 0
    w2[torch.arange(sel), torch.arange(sel)] = 1
    qh = X.code_ints(first_half(ops, None)[2], q)
    ci = (qh - zp2_of(q)).double()
    s_h = X.dequant_scale(q)
    sigma_int = math.sqrt(r4 * max(float((ci * ci).mean()), 1.0) * (127 * 128) / 3.0)
    e2 = round(math.log2(X.FULL_TARGET_SIGMA / (abs(s_h) * sigma_int)))
    ws2 = 2.0 ** (e2 - torch.arange(c) % 5).double()
    mult = s_h * ws2
    selector_only = not bool(((mult.float().double() == mult) & (ws2.float().double() == ws2) & ws2.float().isfinite()).all())
    if selector_only:
        ws2 = torch.ones(c, dtype=torch.float64)
        w2[sel:] = 0
    ws2 = ws2.float()
    ws2[:sel] = 1.0
    b2 = torch.zeros(c, dtype=torch.float32)
    live = c - sel - nz2
    idxs = torch.arange(sel + nz2, c)
    frac = torch.tensor(X.TIE_FRACTIONS, dtype=torch.float64)[idxs % len(X.TIE_FRACTIONS)]
    if live and not selector_only:
        b2[sel + nz2:] = (2.0 ** -(idxs % 5).double() * (frac + torch.randint(-3, 4, (live,), generator=gen).double())).float()
    if case.kind == "sat2":
        w2[sel + nz2], w2[sel + nz2 + 1] = 127, -127
        b2[sel + nz2:sel + nz2 + 2] = 0.0
    _edge_bias(b2, ws2, sel, nz2, 11 * idx + 5)
    return dict(w2=w2, ws2=ws2, b2=b2 if case.bias else None, sel=sel, nz2=nz2, selector_only=selector_only)


def hidden_facts(case, ops):
    """(share of the live units' hidden values strictly inside the code range, the lower bound occurs, the upper one) - inner none."""
    q = case.quant
    codes = X.code_ints(first_half(ops, None)[2], q)[:, ops["nz1"]:]
    return float(((codes > q.lo) & (codes < q.hi)).double().mean()), bool((codes == q.lo).any()), bool((codes == q.hi).any())


def saturation_facts(case, ops):
    """sat1 / sat2: (largest |S|, elements with fl32(S) != S) of the layer the case saturates; None for the others."""
    if case.kind not in ("sat1", "sat2"):
        return None
    s1, _, h = first_half(ops, None)
    s = s1 if case.kind == "sat1" else second_half(ops, case.quant, h)[1]
    return int(s.abs().max()), int((s.float().double() != s.double()).sum())


def _facts_hold(case, ops):
    share, lo, hi = hidden_facts(case, ops)
    sat = saturation_facts(case, ops)
    return share >= 0.25 and lo and hi and (sat is None or (sat[0] > 2 ** 24 and sat[1] > 0))


@functools.lru_cache(maxsize=None)
def operands(cid):
    """The case's CPU operands (see above).  The inputs are drawn from a seed of the case; a draw that misses what the case states about
    itself (`hidden_facts`, `saturation_facts` - few values in the narrow shapes) is drawn again from the next seed, at most 32 times:
    other inputs, never a weaker statement.  Cached and shared: nobody writes to it."""
    case, idx = BY_ID[cid], CASES.index(BY_ID[cid])
    for attempt in range(32):
        gen = torch.Generator().manual_seed(52800 + 101 * idx + 7919 * attempt)
        ops = _layer1(case, gen, idx)
        ops.update(_layer2(case, gen, idx, ops))
        ops["attempt"] = attempt
        if _facts_hold(case, ops):
            return ops
    raise AssertionError(f"{cid}: no draw of 32 has a quarter of its hidden codes inside the range and both bounds")


@functools.lru_cache(maxsize=None)
def reference(cid, inner):
    """dict(s1, pre, h, qh, s2, v) for inner none / relu; for swish s1 and pre alone (the rest follows the launch's own hidden)."""
    case, ops = BY_ID[cid], operands(cid)
    s1, pre, h = first_half(ops, inner)
    if h is None:
        return dict(s1=s1, pre=pre)
    qh, s2, v = second_half(ops, case.quant, h)
    return dict(s1=s1, pre=pre, h=h, qh=qh, s2=s2, v=v)


def int32_bound(case, ops):
    """The largest magnitude the kernel's int32 arithmetic can reach, from the shape: the dot product of re-centred bytes (|x| <= 128,
    |w| <= 127) plus the (shift - zp) * wsum correction, for both layers."""
    shift1 = 128 if case.uns else 0
    shift2 = 128 if case.quant.lo >= 0 else 0
    return max(case.c * 127 * (128 + abs(shift1 - ops["zp1"])), case.r4 * 127 * (128 + abs(shift2 - zp2_of(case.quant))))


def swish64(pre):
    """float64 h * sigmoid(h) of the reference's pre-activation."""
    h = pre.double()
    return h / (1.0 + torch.exp(-h))
