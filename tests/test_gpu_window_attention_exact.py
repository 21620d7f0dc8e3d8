"""The two window attention kernels against what their headers promise (csrc/window_attention.hip, csrc/window_attention_f16.hip), on the
inputs of tests/window_attention_exact_cases.py, whose preconditions tests/test_window_attention_cases_host.py proves on the CPU.  Every
family for operands in ("f32", "f16") and D in {32, 64} unless it says otherwise; T <= 64, B H <= 12.

1. tied maxima, bitwise: 1 .. 8 keys share the exact maximal score - through q . k, the bias, the mask (nW = 3, B = 6) or split between
   bias and mask; out = fl32(integer sum / count), one IEEE division.  A multiply by fl32(1 / count) differs in a third of the elements
   whose count is 3, 5, 6 or 7.
2. the order and rounding of the score steps, bitwise: fl32(fl32(fl32(a scale) + bias) + mask) ties two keys; the mask before the bias,
   the two terms summed first, or the multiply fused with the first add leave them 1 or more apart.
3. uniform rows (strided views into NaN-filled parents, read in place) and placement, bitwise, at every T in 1 .. 64 x terms.
4. the exponential and the division: out = e / (1 + e) on x = -k / 8, k = 1 .. 512, against float64: within 4 2^-24 relative for the fp32
   kernel (expf, not v_exp_f32), within `probe_tol_f16` for the f16 kernel (numerator and denominator see the ROUNDED weight).
5. one planted NaN, +inf or (f16) 1e5: exactly the promised elements are NaN / not finite, every other is within the header's bound.
6. stores stay inside their rows: the entry points called directly on padded output views.
7. a (b, h)'s result does not depend on B, H, its place in the launch or its neighbours' data.
8. bound additions: a negative scale, scale = 0, q x 4 on the fp32 kernel, a -inf mask tail."""
import pytest
import torch

import window_attention_exact_cases as C
from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from test_gpu_attention import U, unmerge
from test_gpu_gate import CODE_SENTINEL, DEV, SENTINEL, bits
from test_gpu_layernorm import own_codes, quantisers
from test_gpu_window_attention import within
from test_gpu_window_attention_f16 import ratio

pytestmark = pytest.mark.gpu
DIMS, OPERANDS = C.DIMS, C.OPERANDS


def dev(x):
    return None if x is None else x.to(DEV)


def run(c, operands, **kw):
    """[B, H, T, D] on the CPU: K.window_attention_quant of the case's tensors (or of the tensors given in their place)."""
    q, k, v, bias, mask = (kw.pop(n) if n in kw else dev(c[n]) for n in ("q", "k", "v", "bias", "mask"))
    return unmerge(K.window_attention_quant(q, k, v, c["scale"], bias=bias, mask=mask, operands=operands, **kw)[0], q.shape[1]).cpu()


def differ(got, want):
    return (bits(got) != bits(want)).reshape(got.shape)


# ------------------------------------------------------------------------------------------- 1. tied maxima
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("way", C.TIE_WAYS)
def test_tied_maxima(way, operands, d):
    wrong = []
    for t in C.TIE_T:
        c = C.tie_case(way, t, d)
        got, want = run(c, operands), c["want"]
        bad = differ(got, want)
        if bool(bad.any()):
            rows = bad.any(-1)
            by_count = {int(n): f"{int((rows & (c['count'] == n)).sum())} of {int((c['count'] == n).sum())}" for n in c["count"].unique()}
            by_set = {C.ZSETS[int(n)]: int((rows & (c["zi"] == n)).sum()) for n in c["zi"].unique()}
            sep = C.separating(c["total"], c["count"])
            wrong.append(f"T = {t}: {int(bad.sum())} of {bad.numel()} elements are not fl32(sum of the tied rows / count); rows by count: {by_count}; "
                         f"by Z: {by_set}; {int((bad & sep).sum())} of them where x / c != x fl32(1 / c) ({int(sep.sum())} such elements); NaN: "
                         f"{int(got.isnan().sum())}; largest |got - want| / |want| = {float(((got.double() - want.double()).abs() / want.double()).nan_to_num(nan=float('inf')).max()):.3e}")
    assert not wrong, f"ties through {way}, {operands}, D = {d}:\n" + "\n".join(wrong)


# ------------------------------------------------------------------------------------------- 2. the order of the score steps
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("kind", C.ORDER_KINDS)
def test_order_of_the_score_steps(kind, operands, d):
    wrong = []
    for t in C.ORDER_T:
        c = C.order_case(kind, t, d)
        got = run(c, operands)
        bad = differ(got, c["want"])
        if bool(bad.any()):
            rows = bad.any(-1)
            va = torch.gather(c["v"], 2, c["a_key"][..., None, None].expand(*rows.shape[:2], 1, d)).expand_as(got)
            vb = torch.gather(c["v"], 2, c["b_key"][..., None, None].expand(*rows.shape[:2], 1, d)).expand_as(got)
            wrong.append(f"T = {t}: {int(rows.sum())} of {rows.numel()} probe rows are not fl32((v_A + v_B) / 2) - the two keys' scores differ; per head / "
                         f"window {rows.sum(-1).reshape(-1).tolist()}; rows that are v_B (key A lost): {int((got == vb).all(-1).sum())}, v_A (key A "
                         f"won): {int((got == va).all(-1).sum())}")
    assert not wrong, f"{kind} (an order it excludes: {C.ORDER_TARGET[kind]}), {operands}, D = {d}:\n" + "\n".join(wrong)


# ------------------------------------------------------------------------------------------- 3. uniform rows and placement at every T
def strided(c):
    """The case's tensors on the device as views: q, k, v rows 1 .. T of NaN-filled parents, the terms [:, 1:T + 1, 4:4 + T] of NaN-filled
    parents whose rows are roundup4(T) + 8 floats apart."""
    t = c["q"].shape[2]
    out = {n: C.row_parent(c[n]).to(DEV)[:, :, 1:t + 1] for n in "qkv"}
    for n in ("bias", "mask"):
        out[n] = None if c[n] is None else C.term_view(C.term_parent(c[n], float("nan")).to(DEV), t)
        assert out[n] is None or (K.window_term_view(out[n], t) is not None and out[n].stride(-2) == C.roundup4(t) + 8)      # read in place
    assert not out["q"].is_contiguous() or t == 0
    return out


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("terms", C.TERMS)
def test_uniform_rows(terms, operands, d):
    wrong = []
    for t in C.ALL_T:
        c = C.uniform_case(t, d, terms)
        got = run(c, operands, **strided(c))
        bad = differ(got, c["want"][None, :, None, :].expand_as(got))
        if bool(bad.any()):
            at = bad.nonzero()
            wrong.append(f"T = {t}: {int(bad.sum())} of {bad.numel()} elements, rows {sorted(set(at[:, 2].tolist()))[:8]}, heads {sorted(set(at[:, 1].tolist()))}, "
                         f"NaN: {int(got.isnan().sum())}")
    assert not wrong, f"terms {terms}, {operands}, D = {d}: not fl32(column sum / T):\n" + "\n".join(wrong)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("terms", C.TERMS)
def test_placement(terms, operands, d):
    wrong = []
    for t in C.ALL_T:
        c = C.placement_case(t, d, terms)
        got = run(c, operands)
        bad = differ(got, c["want"])
        if bool(bad.any()):
            at = bad.nonzero()
            wrong.append(f"T = {t}: {int(bad.sum())} of {bad.numel()} elements, rows {sorted(set(at[:, 2].tolist()))[:8]}, (b, h) "
                         f"{sorted(set(map(tuple, at[:, :2].tolist())))}, NaN: {int(got.isnan().sum())}")
    assert not wrong, f"terms {terms}, {operands}, D = {d}: not the selected row of v:\n" + "\n".join(wrong)


# ------------------------------------------------------------------------------------------- 4. the probe
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("place", sorted(C.PROBE_PLACES))
@pytest.mark.parametrize("variant", C.PROBE_VARIANTS)
def test_exponential_and_division_probe(variant, place, operands, d):
    c = C.probe_case(d, variant, place)
    got = run(c, operands).double()
    ref = c["ref"][..., None].expand_as(got)
    tol = (C.PROBE_TOL * c["ref"] if operands == "f32" else C.probe_tol_f16(c["x"]))[..., None].expand_as(got)
    err = (got - ref).abs()
    worst = err / tol
    at = int(worst.amax(-1).reshape(-1).argmax())
    print(f"probe {variant} / {place} {operands} D = {d}: max |out - ref| / tolerance = {float(worst.max()):.3f} at x = {float(c['x'].reshape(-1)[at])}; "
          + (f"max |out - ref| / ref = {float((err / ref).max()) / U:.3f} u" if operands == "f32" else f"max |out - ref| = {float(err.max()):.3e}"))
    assert torch.equal(bits(got.float()[..., :1].expand_as(got).contiguous()), bits(got.float())), "the channels of a row differ"
    assert bool((err <= tol).all()), f"{float(worst.max()):.3f} of the tolerance at x = {float(c['x'].reshape(-1)[at])}"


# ------------------------------------------------------------------------------------------- 5. non-finite values and the f16 range
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("operands,kind", [(o, k) for o in OPERANDS for k in C.PLANT_KINDS] + [("f16", k) for k in C.PLANT_KINDS_F16])
def test_planted_non_finite_values(operands, kind, d):
    for which in range(len(C.plant_positions(d))):
        c = C.plant_case(kind, d, which)
        q, k, v, bias, mask = (dev(c[n]) for n in ("q", "k", "v", "bias", "mask"))
        out = K.window_attention_quant(q, k, v, c["scale"], bias=bias, mask=mask, operands=operands)[0]
        got, hit, what = unmerge(out, q.shape[1]).cpu(), c["hit"], f"{kind} at {c['at']} {operands} D = {d}"
        bad = ~torch.isfinite(got) if kind.startswith("big") else got.isnan()
        assert torch.equal(bad, hit), (f"{what}: {int((bad & ~hit).sum())} elements outside the promised {int(hit.sum())} are affected, "
                                        f"{int((hit & ~bad).sum())} of the promised are not")
        assert bool(torch.isfinite(got[~hit]).all()), what
        if operands == "f32":
            worst, ref = within(out, q, k, v, c["scale"], bias, mask, what)
            assert torch.equal(ref.isnan(), hit)
        else:
            worst, _ = ratio(got, q, k, v, c["scale"], bias, mask, what, skip=hit)
        assert worst <= 1.0, what


# ------------------------------------------------------------------------------------------- 6. stores
def raw(entry, c, t, d, qz, want_out, want_codes):
    """One call of dlmcq_window_attention_f32 / _f16 whose outputs are views (rows 1 .., columns 4 ..) of parents [B, T + 2, H D + 8] holding
    a fill pattern: (fp32 parent as int32, code parent as uint8, the two views).  bias and mask: dense rows padded to 4 floats."""
    q, k, v = (dev(c[n]) for n in "qkv")
    b, h = q.shape[:2]
    pad = C.roundup4(t)
    bias, mask = (torch.zeros(x.shape[0], t, pad, device=DEV) for x in (c["bias"], c["mask"]))
    bias[:, :, :t], mask[:, :, :t] = dev(c["bias"]), dev(c["mask"])
    shape, off, o_strides = C.padded(b, h, t, d)
    obuf = torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full(shape, CODE_SENTINEL, dtype=torch.uint8, device=DEV)
    oview, cview = obuf[:, 1:t + 1, 4:4 + h * d], cbuf[:, 1:t + 1, 4:4 + h * d]
    assert oview.storage_offset() == off and oview.data_ptr() % 16 == 0 and cview.data_ptr() % 4 == 0
    sc, z, lo, hi, form, gq = qz if want_codes else (None, None, 0, 0, 0, 0.0)
    rc = entry(N.ptr(q), N.ptr(k), N.ptr(v), N.ptr(bias), N.ptr(mask), N.ptr(oview) if want_out else None, N.ptr(cview) if want_codes else None,
               b, h, t, d, mask.shape[0], *q.stride()[:3], *k.stride()[:3], *v.stride()[:3], *o_strides, t * pad, pad, t * pad, pad,
               float(c["scale"]), N.ptr(sc), N.ptr(z), lo, hi, form, gq, N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return obuf, cbuf, oview, cview


def outside_is_untouched(buf, view_rows, view_cols, fill):
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[:, 1:1 + view_rows, 4:4 + view_cols] = False
    return bool((buf[keep] == fill).all())


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("t", C.STORE_T)
def test_stores_stay_inside_their_rows(t, operands, d):
    b, h = C.STORE_BH
    c = C.n01_case(b, h, t, d, 1, seed=4)
    entry = N.lib.dlmcq_window_attention_f16 if operands == "f16" else N.lib.dlmcq_window_attention_f32
    plain = K.window_attention_quant(*(dev(c[n]) for n in "qkv"), c["scale"], bias=dev(c["bias"]), mask=dev(c["mask"]), operands=operands)[0]
    for name, qz in sorted(quantisers().items()):
        want_codes = own_codes(plain, qz)
        for want_out, want_c in ((True, True), (False, True)) + (((True, False),) if name == "qbase_s8" else ()):
            obuf, cbuf, oview, cview = raw(entry, c, t, d, qz, want_out, want_c)
            what = f"{name}, out = {want_out}, codes = {want_c}"
            assert outside_is_untouched(obuf, t, h * d, SENTINEL), f"{what}: fp32 elements around the view were written"
            assert outside_is_untouched(cbuf, t, h * d, CODE_SENTINEL), f"{what}: code bytes around the view were written"
            if want_out:
                assert torch.equal(oview.contiguous(), bits(plain)), f"{what}: other bits than the dense call"
            else:
                assert bool((obuf == SENTINEL).all()), f"{what}: out = NULL and fp32 elements were written"
            if want_c:
                assert torch.equal(cview.contiguous(), want_codes), f"{what}: {int((cview != want_codes).sum())} code bytes differ"
            else:
                assert bool((cbuf == CODE_SENTINEL).all()), f"{what}: codes = NULL and code bytes were written"


# ------------------------------------------------------------------------------------------- 7. independence of the launch
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("operands", OPERANDS)
def test_a_pair_does_not_depend_on_the_launch(operands, d):
    b, h, t = C.INDEP_BHT
    c = C.indep_tile(d)
    q, k, v = (dev(c[n]) for n in "qkv")
    bias, mask = dev(c["bias"]), dev(c["mask"]).expand(b, t, t).contiguous()      # one bias tile (head stride 0), nW = 3 identical mask tiles
    call = lambda q_, k_, v_, m_: unmerge(K.window_attention_quant(q_, k_, v_, c["scale"], bias=bias, mask=m_, operands=operands)[0], q_.shape[1])  # noqa: E731
    alone = call(q[None, None], k[None, None], v[None, None], mask[:1])[0, 0]
    rep = lambda x: x.expand(b, h, t, d).contiguous()  # noqa: E731
    every = call(rep(q), rep(k), rep(v), mask)
    same = [(bi, hi) for bi in range(b) for hi in range(h) if torch.equal(bits(every[bi, hi]), bits(alone))]
    assert len(same) == b * h, f"the replicated tile: only the pairs {same} equal the tile run alone"
    wrong = []
    for bi in range(b):      # the pair under test among eight neighbours that hold other k and v
        for hi in range(h):
            kk, vv = dev(c["other_k"]).clone(), dev(c["other_v"]).clone()
            kk[bi, hi], vv[bi, hi] = k, v
            if not torch.equal(bits(call(rep(q), kk, vv, mask)[bi, hi]), bits(alone)):
                wrong.append((bi, hi))
    assert not wrong, f"pairs {wrong} differ from the tile run alone when their neighbours hold other k and v"


# ------------------------------------------------------------------------------------------- 8. bound additions
def bound_ratio(c, operands, scale, what, q=None, mask=None):
    q, k, v, bias = dev(c["q"] if q is None else q), dev(c["k"]), dev(c["v"]), dev(c["bias"])
    dense = dev(c["mask"])
    out = K.window_attention_quant(q, k, v, scale, bias=bias, mask=dense if mask is None else mask, operands=operands)[0]
    if operands == "f32":
        return within(out, q, k, v, scale, bias, dense, what)
    return ratio(unmerge(out, q.shape[1]).cpu(), q, k, v, scale, bias, dense, what)


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("shape", C.BOUND_SHAPES, ids=str)
@pytest.mark.parametrize("family,operands", [(f, o) for f in ("negative_scale", "zero_scale") for o in OPERANDS] + [("peaky", "f32")])
def test_bound_additions(family, operands, shape, d):
    """(peaky, q x 4: the f16 kernel has it in tests/test_gpu_window_attention_f16.py::test_bound)"""
    b, h, t, nw = shape
    c = C.n01_case(b, h, t, d, nw, seed=5)
    scale = {"negative_scale": -c["scale"], "zero_scale": 0.0, "peaky": c["scale"]}[family]
    worst, _ = bound_ratio(c, operands, scale, f"{family} {shape} {operands} D = {d}", q=c["q"] * 4 if family == "peaky" else None)
    assert worst <= 1.0


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("operands", OPERANDS)
@pytest.mark.parametrize("shape", C.BOUND_SHAPES, ids=str)
def test_minus_infinity_tail(shape, operands, d):
    """-inf from the first key of the 16-byte piece that holds key T - 1 through the rest of every row's stride: float64 attention over
    the keys in front of it."""
    c = C.inf_tail_case(shape, d)
    t = shape[2]
    view = C.term_view(C.term_parent(c["mask"], float("-inf")).to(DEV), t)
    assert K.window_term_view(view, t) is not None
    worst, ref = bound_ratio(c, operands, c["scale"], f"-inf tail {shape} {operands} D = {d}", mask=view)
    assert worst <= 1.0 and not bool(ref.isnan().any())
