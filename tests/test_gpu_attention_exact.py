"""The attention kernel against what its header promises (csrc/attention.hip), on the inputs of tests/attention_exact_cases.py, whose
preconditions tests/test_attention_cases_host.py proves on the CPU.  Every family for D in {32, 64}; B H <= 8, T <= 257.

1. tied maxima, bitwise: 1 .. 8 keys share the exact maximal score - neighbours in one lane half, the two lane halves, other key blocks
   (al = expf(0) = 1), ties cut by Tk to 3, 5, 6, 7 keys; out = fl32(integer sum / count), one IEEE division.  A multiply by
   fl32(1 / count) differs in 43 - 45 % of the elements whose count is 3, 5, 6 or 7; a dropped or doubled tie, a wrong merge of the two
   halves of l, al != 1 between blocks differ everywhere in their rows.
2. uniform rows, bitwise, over Tq in {1, 31 .. 33, 95 .. 97, 127 .. 129, 160, 161, 256, 257} x Tk in {1, 2, 31 .. 33, 64, 65}, H = 5 (all
   four wave rotations and the wrap, each with the partial tile), q, k, v views into NaN-filled parents; q = 0, and scale = 0 with random q.
3. the expf and division probe: out = e / (1 + e) and, through al and both halves of l, e / (2 + e), e = expf(x), x = -k / 8, k = 1 .. 512,
   against float64 within 4 2^-24 relative (one ulp of expf, a rounding of l, a division).  Largest ratios seen on the device: see the
   table in DESIGN.md 5.24.
4. -inf scores: all of key block 0 and a part of block 1 (the m~ = 0 guard), every key (0 / 0: NaN, as torch), and a negative scale.
5. stores stay inside their rows: dlmcq_attention_f32 called directly on padded output views; every element around them keeps its fill."""
import pytest
import torch

import attention_exact_cases as C
from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from test_gpu_attention import U, bound, check_bound, unmerge
from test_gpu_gate import CODE_SENTINEL, DEV, SENTINEL, bits
from test_gpu_layernorm import own_codes, quantisers

pytestmark = pytest.mark.gpu
DIMS = C.DIMS


def run(c, **kw):
    """[B, H, Tq, D] on the CPU: K.attention_quant of the case's tensors."""
    q, k, v = (c[n].to(DEV) for n in "qkv")
    return unmerge(K.attention_quant(q, k, v, c["scale"], **kw)[0], q.shape[1]).cpu()


# ------------------------------------------------------------------------------------------- 1. tied maxima
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("shape", C.TIE_SHAPES, ids=str)
def test_tied_maxima(shape, d):
    c = C.tie_case(shape, d)
    got, want = run(c), c["want"]
    bad = bits(got) != bits(want)
    if bool(bad.any()):
        rows = bad.any(-1)
        by_count = {int(n): f"{int((rows & (c['count'] == n)).sum())} of {int((c['count'] == n).sum())}" for n in c["count"].unique()}
        by_set = {C.ZSETS[int(n)]: int((rows & (c["zi"] == n)).sum()) for n in c["zi"].unique()}
        sep = C.separating(c["total"], c["count"])
        pytest.fail(f"{int(bad.sum())} of {bad.numel()} elements are not fl32(sum of the tied rows / count); rows by count: {by_count}; by Z: "
                    f"{by_set}; {int((bad & sep).sum())} of them where x / c != x fl32(1 / c) ({int(sep.sum())} such elements); largest "
                    f"|got - want| / |want| = {float(((got.double() - want.double()).abs() / want.double()).max()):.3e}")


# ------------------------------------------------------------------------------------------- 2. uniform rows
def nan_views(c):
    """The case's q, k, v as views [:, :, 1:T + 1] of NaN-filled parents on the device."""
    out = []
    for n in "qkv":
        b, h, t, d = c[n].shape
        parent = torch.full((b, h, t + 2, d), float("nan"), device=DEV)
        parent[:, :, 1:t + 1] = c[n].to(DEV)
        out.append(parent[:, :, 1:t + 1])
    return out


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("tk", C.UNIFORM_TK)
def test_uniform_rows(tk, d):
    wrong = []
    for tq in C.UNIFORM_TQ:
        for zero_scale in (False, True):
            c = C.uniform_case(tq, tk, d, zero_scale)
            q, k, v = nan_views(c)
            assert not q.is_contiguous() and bool(torch.isnan(q._base[:, :, 0]).all())
            got = unmerge(K.attention_quant(q, k, v, c["scale"])[0], q.shape[1]).cpu()
            want = c["want"][None, :, None, :].expand_as(got)
            bad = (bits(got) != bits(want)).reshape(got.shape)
            if bool(bad.any()):
                wrong.append(f"Tq = {tq}, scale = {c['scale']}: {int(bad.sum())} of {bad.numel()} elements, rows {sorted(set(bad.nonzero()[:, 2].tolist()))[:8]}, "
                             f"heads {sorted(set(bad.nonzero()[:, 1].tolist()))}, NaN: {int(got.isnan().sum())}")
    assert not wrong, f"Tk = {tk}: not fl32(column sum / Tk):\n" + "\n".join(wrong)


# ------------------------------------------------------------------------------------------- 3. the probe
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("variant", C.PROBE_VARIANTS)
def test_expf_and_division_probe(variant, d):
    c = C.probe_case(d, variant)
    got = run(c).double()
    ref = c["ref"][..., None].expand_as(got)
    rel = (got - ref).abs() / ref
    at = int(rel.amax(-1).reshape(-1).argmax())
    print(f"probe {variant} D = {d}: max |out - ref| / ref = {float(rel.max()) / U:.3f} u at x = {float(c['x'].reshape(-1)[at])}; "
          f"{float(rel.max()) / C.PROBE_TOL:.3f} of the tolerance")
    assert torch.equal(bits(got.float()[..., :1].expand_as(got).contiguous()), bits(got.float())), "the channels of a row differ"
    assert bool((rel <= C.PROBE_TOL).all()), f"{float(rel.max()) / U:.2f} u > 4 u at x = {float(c['x'].reshape(-1)[at])}"


# ------------------------------------------------------------------------------------------- 4. -inf scores, a negative scale
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("shape", C.INF_SHAPES, ids=str)
def test_inf_prefix(shape, d):
    """Rows with a positive q[0]: -inf scores for the keys 0 .. 39 (m~ = 0 in block 0, al = expf(-inf) = 0 after it): finite and within
    bound() of float64's attention over the keys 40 .. alone.  The other rows: +inf or 0 inf, NaN - torch's mask."""
    c = C.inf_prefix_case(shape, d, False)
    q, k, v = (c[n].to(DEV) for n in "qkv")
    nan = c["nan"]
    ref_nan = torch.matmul(torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * c["scale"], dim=-1), v).isnan().cpu()
    assert torch.equal(ref_nan, nan[..., None].expand_as(ref_nan)), "the test's own expectation is not torch's"
    got = run(c)
    assert torch.equal(got.isnan(), ref_nan)
    assert bool(torch.isfinite(got[~nan]).all())
    ref, bnd = bound(c["q"], c["k"][:, :, c["first"]:], c["v"][:, :, c["first"]:], c["scale"])
    err = (got.double() - ref).abs()[~nan]
    ratio = float((err / bnd[~nan]).max())
    print(f"{shape} D = {d} -inf prefix: max |out - o*| / bound = {ratio:.4f}")
    assert bool((err <= bnd[~nan]).all()), ratio


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("shape", C.INF_SHAPES, ids=str)
def test_every_key_minus_inf(shape, d):
    c = C.inf_prefix_case(shape, d, True)
    q, k, v = (c[n].to(DEV) for n in "qkv")
    ref_nan = torch.matmul(torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * c["scale"], dim=-1), v).isnan().cpu()
    assert bool(ref_nan.all()) and bool(c["nan"].all())
    assert bool(run(c).isnan().all())


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("shape", C.INF_SHAPES, ids=str)
def test_negative_scale(shape, d):
    c = C.negative_scale_case(shape, d)
    q, k, v = (c[n].to(DEV) for n in "qkv")
    out, _ = K.attention_quant(q, k, v, c["scale"])
    ratio, ok = check_bound(unmerge(out, q.shape[1]), q, k, v, c["scale"], f"{shape} D = {d} scale = {c['scale']:.4f}")
    assert ok, ratio


# ------------------------------------------------------------------------------------------- 5. stores
def raw(q, k, v, scale, qz, want_out, want_codes):
    """One call of dlmcq_attention_f32 whose outputs are views (rows 1 .., columns 4 ..) of parents [B, Tq + 2, H D + 8] holding a fill
    pattern: (fp32 parent as int32, code parent as uint8, the two views)."""
    b, h, tq, d = q.shape
    shape, off, o_strides = C.padded(b, h, tq, d)
    obuf = torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full(shape, CODE_SENTINEL, dtype=torch.uint8, device=DEV)
    oview, cview = obuf[:, 1:tq + 1, 4:4 + h * d], cbuf[:, 1:tq + 1, 4:4 + h * d]
    assert oview.storage_offset() == off and oview.data_ptr() % 16 == 0 and cview.data_ptr() % 4 == 0
    sc, z, lo, hi, form, gq = qz if want_codes else (None, None, 0, 0, 0, 0.0)
    rc = N.lib.dlmcq_attention_f32(N.ptr(q), N.ptr(k), N.ptr(v), N.ptr(oview) if want_out else None, N.ptr(cview) if want_codes else None,
                                   b, h, tq, k.shape[2], d, *q.stride()[:3], *k.stride()[:3], *v.stride()[:3], *o_strides, float(scale),
                                   N.ptr(sc), N.ptr(z), lo, hi, form, gq, N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return obuf, cbuf, oview, cview


def outside_is_untouched(buf, view_rows, view_cols, fill):
    keep = torch.ones(buf.shape, dtype=torch.bool, device=buf.device)
    keep[:, 1:1 + view_rows, 4:4 + view_cols] = False
    return bool((buf[keep] == fill).all())


@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("tq", C.STORE_TQ)
def test_stores_stay_inside_their_rows(tq, d):
    c = C.store_case(tq, d)
    q, k, v = (c[n].to(DEV) for n in "qkv")
    b, h = q.shape[:2]
    plain = K.attention_quant(q, k, v, c["scale"])[0]                       # [B, Tq, H D], dense
    for name, qz in sorted(quantisers().items()):
        want_codes = own_codes(plain, qz)
        for want_out, want_c in ((True, True), (False, True)) + (((True, False),) if name == "qbase_s8" else ()):
            obuf, cbuf, oview, cview = raw(q, k, v, c["scale"], qz, want_out, want_c)
            what = f"{name}, out = {want_out}, codes = {want_c}"
            assert outside_is_untouched(obuf, tq, h * d, SENTINEL), f"{what}: fp32 elements around the view were written"
            assert outside_is_untouched(cbuf, tq, h * d, CODE_SENTINEL), f"{what}: code bytes around the view were written"
            if want_out:
                assert torch.equal(oview.contiguous(), bits(plain)), f"{what}: other bits than the dense call"
            else:
                assert bool((obuf == SENTINEL).all()), f"{what}: out = NULL and fp32 elements were written"
            if want_c:
                assert torch.equal(cview.contiguous(), want_codes), f"{what}: {int((cview != want_codes).sum())} code bytes differ"
            else:
                assert bool((cbuf == CODE_SENTINEL).all()), f"{what}: codes = NULL and code bytes were written"
