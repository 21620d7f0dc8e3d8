"""The QAT backward kernels (csrc/fq_backward.hip + csrc/fq_bodies.h, the segment-table launch of csrc/fake_quant_multi.hip,
`rootq_weight_bwd_kernel` of csrc/rootq.hip) against oracle.fakequant_oracle's float64 sums, at the smallest shapes that cross
each edge of their launch geometry (tests/_bwd_cases.py; DESIGN.md has the table).

gx is required bit for bit everywhere.  The scale gradient is required
  - bit for bit on the EXACT cases: dyadic inputs whose every partial sum is an fp32 number in any order, with a distinct power
    of two planted on every edge, so that one dropped or doubled element changes the result (tests/test_backward_cases.py
    checks both properties on the CPU);
  - within (L + 13) * 2^-24 * sum|contrib| * g on the RANDOM cases, L the longest per-lane chain of the geometry - a
    derivation (`_bwd_cases.sum_bound`), not a measurement.
Every launch runs twice and must repeat its bits; every launch gets a scratch buffer of exactly the queried size with a sentinel
behind it and behind gscale.  Each test prints `RATIO <case> <max error / bound>` for DESIGN.md's table."""

import pytest
import torch

import _bwd_cases as C
from _cmp import assert_bits_equal

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = 0x7FC0DEAD          # a NaN payload no kernel here produces
ESCRATCH = -3
ERANGE = -2


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "the gpu suite needs a GPU"
    from dlmc.quantization.scalar import kernels
    return kernels


@pytest.fixture(scope="module")
def N(K):
    from dlmc import _native
    return _native


def form_code(N, form):
    return {"qbase": N.FORM_QBASE, "zeropoint": N.FORM_ZEROPOINT, "symmetric": N.FORM_SYMMETRIC, "rootq_act": N.FORM_ROOTQ_ACT}[form]


def place(t, misaligned=False, fill=None):
    """`t` (or an uninitialised / sentinel-filled tensor of its size) on the device, 16-byte aligned or one float off."""
    n = t if isinstance(t, int) else t.numel()
    buf = torch.empty(n + 8, dtype=torch.float32, device=DEV)
    if fill is not None:
        buf.view(torch.int32).fill_(fill)
    view = buf[1:1 + n] if misaligned else buf[:n]
    assert view.data_ptr() % 16 == (4 if misaligned else 0)
    if not isinstance(t, int):
        view.copy_(t.reshape(-1))
    return view


class Launch:
    """One direct call of dlmcq_fake_quant_bwd_form_f32 on `case`, with scratch of exactly the queried size."""

    def __init__(self, N, case, misalign=(), want_gx=True, want_gs=True):
        self.N, self.case = N, case
        outer, ch, inner = case.shape
        self.x, self.gy = place(case.x, "x" in misalign), place(case.gy, "gy" in misalign)
        self.scale = case.scale.to(DEV)
        self.offset = None if case.offset is None else case.offset.to(DEV)
        self.gx = place(case.x.numel(), "gx" in misalign, fill=SENTINEL) if want_gx else None
        self.gs_buf = torch.full((ch + 1,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32) if want_gs else None
        self.nbytes = N.lib.dlmcq_fq_bwd_scratch_bytes(outer, ch, inner)
        assert self.nbytes == 4 * ch * C.plan(outer, ch, inner)[0], "the scratch query is not one float per (segment, channel)"
        self.scratch = torch.full((self.nbytes // 4 + 1,), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
        self.vec = not misalign and (ch == 1 or inner % 4 == 0)

    def run(self, nbytes=None):
        c, N = self.case, self.N
        outer, ch, inner = c.shape
        return N.lib.dlmcq_fake_quant_bwd_form_f32(
            N.ptr(self.x), N.ptr(self.gy), N.ptr(self.gx), N.ptr(self.gs_buf), N.ptr(self.scale), N.ptr(self.offset), outer, ch, inner,
            c.lo, c.hi, form_code(N, c.form), float(c.g), N.ptr(self.scratch), self.nbytes if nbytes is None else nbytes, N.stream_ptr())

    @property
    def gs(self):
        return self.gs_buf[:-1]

    def sentinels_intact(self):
        ok = int(self.scratch.view(torch.int32)[-1]) == SENTINEL
        if self.gs_buf is not None:
            ok = ok and int(self.gs_buf.view(torch.int32)[-1]) == SENTINEL
        return ok


def check_case(N, kind, form, shape, misalign=()):
    case, (gx, value, abs_sum, _) = C.case_with_reference(kind, form, shape)
    run = Launch(N, case, misalign)
    assert run.run(run.nbytes - 4) == ESCRATCH, "one float less of scratch was accepted"
    assert int(run.gx.view(torch.int32)[0]) == SENTINEL and int(run.gs_buf.view(torch.int32)[0]) == SENTINEL, "a refused call wrote"
    assert run.run() == 0
    first = run.gs.clone()
    assert run.run() == 0
    torch.cuda.synchronize()
    assert torch.equal(first.view(torch.int32), run.gs.view(torch.int32)), "the scale gradient must repeat run to run"
    assert run.sentinels_intact(), "the backward wrote behind its scratch or behind gscale"
    tag = f"{kind} {form} {shape} misaligned {'+'.join(misalign) or 'nothing'}"
    assert_bits_equal(run.gx, gx, tag + " gx")
    got = run.gs.cpu().double()
    if kind == "exact":
        print(f"RATIO {tag} exact")
        assert_bits_equal(got.float(), value.float(), tag + " gscale")
        return
    L = C.chain_length(*shape, run.vec)
    g = float(torch.tensor(case.g, dtype=torch.float32)) if form == "qbase" else 1.0
    bound = C.sum_bound(L, abs_sum, g)
    err = (got - value).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"RATIO {tag} L {L} {ratio:.4f}")
    assert bool((err <= bound).all()), f"{tag} gscale: error / bound = {ratio} at channel {int((err / bound.clamp_min(1e-300)).argmax())}"


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("form,shape", C.all_fq_cases(), ids=_ids)
def test_backward_against_float64(N, form, shape, kind):
    check_case(N, kind, form, shape)


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("which", ["x", "gy", "gx"])
@pytest.mark.parametrize("form,n", [(f, n) for n, forms in C.UNALIGNED_N for f in forms], ids=_ids)
def test_unaligned_per_tensor_backward_against_float64(N, form, n, which, kind):
    """One misaligned pointer of the three sends the whole tensor to the generic kernel."""
    check_case(N, kind, form, (1, 1, n), misalign=(which,))


@pytest.mark.parametrize("kind", ["exact", "random"])
@pytest.mark.parametrize("form", C.CHANNEL_FORMS)
def test_misaligned_rows_with_inner_a_multiple_of_four(N, form, kind):
    check_case(N, kind, form, C.MISALIGNED_CHANNEL_SHAPE, misalign=("x",))


@pytest.mark.parametrize("form,shape,misalign", [("qbase", (1, 1, 4099), ()), ("zeropoint", (1, 1, 4099), ("gy",)),
                                                 ("symmetric", (5, 1024, 12), ()), ("qbase", (5, 1024, 9), ())], ids=_ids)
def test_one_output_alone_is_the_same_output(N, form, shape, misalign):
    case, (gx, _, _, _) = C.case_with_reference("random", form, shape)
    both = Launch(N, case, misalign)
    assert both.run() == 0
    only_gs = Launch(N, case, misalign, want_gx=False)
    assert only_gs.run() == 0
    only_gx = Launch(N, case, misalign, want_gs=False)
    assert only_gx.run() == 0
    torch.cuda.synchronize()
    assert torch.equal(only_gs.gs.view(torch.int32), both.gs.view(torch.int32)), "gscale changes when gx is not wanted"
    assert torch.equal(only_gx.gx.view(torch.int32), both.gx.view(torch.int32)), "gx changes when gscale is not wanted"
    assert_bits_equal(only_gx.gx, gx, "gx alone")
    assert only_gs.sentinels_intact() and only_gx.sentinels_intact()


@pytest.mark.parametrize("form", ["qbase", "zeropoint"])
def test_non_finite_x_poisons_only_the_sum(N, K, form):
    """The full adversarial set (NaN, both infinities): gx still bit for bit, the scale gradient NaN like the reference's."""
    from test_gpu_fq_multi import adversarial
    case = C.random_case(form, (1, 1, 4099))
    adv = adversarial(float(case.scale[0]), float(case.offset[0]) if form == "qbase" else 0.0, case.lo, case.hi)
    case.x[0, 0, :adv.numel()] = adv
    gx, value, _, _ = case.reference()
    run = Launch(N, case)
    assert run.run() == 0
    torch.cuda.synchronize()
    assert_bits_equal(run.gx, gx, "gx")
    assert bool(torch.isnan(value).all()) and bool(torch.isnan(run.gs).all())


def test_segment_table_equals_the_one_tensor_launches(N, K):
    """Every aligned case with outer == 1 that the table takes, both kinds, in one call and in mixed order."""
    picks = [(k, f, s) for f, s in C.all_fq_cases() for k in ("exact", "random")
             if s[0] == 1 and s[1] * s[2] <= C.MULTI_MAX_N and f != "rootq_act"]
    assert sum(s[2] == C.MULTI_MAX_N for _, _, s in picks) == 6 and sum(s[1] == 257 for _, _, s in picks) == 12
    picks = picks[1::2] + picks[0::2][::-1]
    segs, gys, want = [], [], []
    for kind, form, shape in picks:
        case = (C.exact_case if kind == "exact" else C.random_case)(form, shape)
        run = Launch(N, case)
        assert run.run() == 0
        want.append((run.gx, run.gs))
        x = run.x.view(shape[1], shape[2]) if shape[1] > 1 else run.x
        scale = run.scale.reshape(-1, 1) if shape[1] > 1 else run.scale
        offset = run.offset if run.offset is None or shape[1] == 1 else run.offset.reshape(-1, 1)
        segs.append(K.Segment(x, scale, offset, case.lo, case.hi, form_code(N, form), case.g))
        gys.append(run.gy.view(x.shape))
    gxs, gss = K.fake_quant_multi_backward(segs, gys)
    torch.cuda.synchronize()
    for (kind, form, shape), gx, gs, (wgx, wgs) in zip(picks, gxs, gss, want):
        assert torch.equal(gx.reshape(-1).view(torch.int32), wgx.view(torch.int32)), f"{kind} {form} {shape} gx"
        assert torch.equal(gs.view(torch.int32), wgs.view(torch.int32)), f"{kind} {form} {shape} gscale"


def test_segment_table_refuses_a_tensor_past_its_cap(N, K):
    table = (N.FqSegment * 1)()
    x = torch.empty(4, device=DEV)          # prepare is host only: it reads the record, not the tensor
    rec = table[0]
    rec.x = rec.gy = rec.gx = x.data_ptr()
    rec.scale = rec.gscale = x.data_ptr()
    rec.n, rec.channels, rec.inner, rec.lo, rec.hi, rec.form = C.BIG, 1, C.BIG, -8, 7, N.FORM_QBASE
    assert K._prepare(table, 1)[0] == ERANGE
    rec.n = rec.inner = C.MULTI_MAX_N
    assert K._prepare(table, 1)[:3] == (0, 0, C.TENSOR_BLOCKS)


# ----------------------------------------------------------------------------------------------- RootQ weights
@pytest.mark.parametrize("alpha", C.RQ_ALPHA)
@pytest.mark.parametrize("bits", C.RQ_BITS)
@pytest.mark.parametrize("n", C.RQ_N)
def test_rootq_weight_backward_against_float64(K, n, bits, alpha):
    case, (gw, scalars, abs_sums) = C.rootq_case(n, bits, alpha)
    w, gy = case.w.to(DEV), case.gy.to(DEV)
    args = (torch.tensor(case.upper, device=DEV), torch.tensor(case.lower, device=DEV), torch.tensor(alpha, device=DEV), case.lo, case.hi)
    got = K.rootq_weight_backward(w, gy, *args)
    again = K.rootq_weight_backward(w, gy, *args)
    alone = K.rootq_weight_backward(w, gy, *args, want_gw=False)
    torch.cuda.synchronize()
    tag = f"rootq weight n {n} b{bits} alpha {alpha}"
    assert alone[0] is None
    for a, b, c, name in zip(got[1:], again[1:], alone[1:], ("g_upper", "g_lower", "g_alpha")):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{tag}: {name} must repeat run to run"
        assert torch.equal(a.view(torch.int32), c.view(torch.int32)), f"{tag}: {name} changes when gw is not wanted"
    torch.testing.assert_close(got[0].cpu().double(), gw, rtol=2e-4, atol=2e-5, msg=lambda m: f"{tag} gw: {m}")
    ratios = []
    for name, g, want, bound in zip(("g_upper", "g_lower", "g_alpha"), got[1:], scalars, case.bounds(abs_sums)):
        err = abs(float(g) - float(want))
        ratios.append(err / bound if bound else (0.0 if err == 0 else float("inf")))
        assert err <= bound, f"{tag} {name}: {float(g)} vs {float(want)}, error {err} > bound {bound}"
    print(f"RATIO {tag} L {case.L} {max(ratios):.4f}")
