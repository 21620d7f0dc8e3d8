"""The calibration estimators (csrc/estimator.hip), AdaRound (csrc/adaround.hip) and the weight transforms
(csrc/weight_fold.hip) past one workgroup: the smallest shapes that cross each boundary of their segment plans, strided
loops, row caching, wide channel counts and device-side state machines.  Every reference is a plain CPU restatement:
per-element arithmetic replays fp32 as oracle/fakequant_oracle.py does (the library is built without FMA contraction, so
per-element values are bit-identical), every sum that decides something is taken in float64.

Where a kernel takes a chain of strict comparisons on fp32 sums, the test replays the chain in float64, asserts ON THE CPU
that no decision of the committed seed is nearer than the stated gap, and only then requires bit equality.  The gaps and
seeds recorded in the docstrings were measured with the CPU replay alone, never with the kernel under test."""
import math
import os
import re

import pytest
import torch
from torch import nn

from _cmp import assert_bits_equal
from oracle import fakequant_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "the gpu suite needs a GPU"
    from dlmc.quantization.scalar import kernels
    return kernels


def N():
    from dlmc import _native
    return _native


def gen(seed):
    g = torch.Generator()
    g.manual_seed(2333 + seed)
    return g


def close(got, want, what="", rtol=1e-4, atol=1e-5):
    torch.testing.assert_close(got.detach().cpu(), want, rtol=rtol, atol=atol, msg=lambda m: f"{what}: {m}")


def _cus():
    with open(os.path.join(ROOT, "dlmc-quant_amd", "csrc", "dlmcq_internal.h")) as f:
        return int(re.search(r"#define\s+DLMCQ_CUS\s+(\d+)", f.read()).group(1))


CUS = _cus()
SEG_CAP = CUS * 8            # the most segments a plan uses
SEG_MIN = 16384              # the fewest elements of a per-tensor segment


def l2_plan(outer, ch, inner):
    """(nseg, npseg, ipseg) of estimator.hip's l2_plan, restated."""
    if ch == 1 and outer == 1:
        nseg = max(1, min((inner + SEG_MIN - 1) // SEG_MIN, SEG_CAP))
        ipseg = ((inner + nseg - 1) // nseg + 3) & ~3
        return max(1, (inner + ipseg - 1) // ipseg), outer, ipseg
    nseg = max(1, min((SEG_CAP + ch - 1) // ch, outer, 65535))
    npseg = (outer + nseg - 1) // nseg
    return (outer + npseg - 1) // npseg, npseg, inner


def _signed_or_relu(shape, signed, g):
    x = torch.randn(shape, generator=g)
    return x if signed else torch.relu(x) + 0.01


# ====================================================================================== 1. l2norm_step across plans
def _step_want(x, s, o, lo, hi, red):
    q = O.quantize_codes(x, s, o, lo, hi)
    a, b = (x * q).double(), (q * q + 1e-7).double()
    return (a.sum() / b.sum()) if red is None else (a.sum(dim=red) / b.sum(dim=red)).reshape(s.shape)


PER_TENSOR_N = [SEG_MIN, SEG_MIN + 1, 3 * SEG_MIN + 5, SEG_CAP * SEG_MIN + SEG_MIN + 3]


@pytest.mark.parametrize("n", PER_TENSOR_N)
def test_l2norm_step_per_tensor_segments(K, n):
    """One, two and four segments, and one size past the segment cap where `ipseg` is rounded up to a multiple of 4 (the
    only case of this file that allocates more than 150 MB).  The scale is the min/max scale of the tensor BEFORE values
    four times its maximum are planted on both sides of every segment boundary and in the last element: those clip, so
    each of them moves the result by about 3*max^2 / SUM x^2 of its segment (4e-3 at 16384 elements, 200 times the
    tolerance) and a segment that loses or repeats its edge element is seen - an unclipped element would not be, because
    its x*q and s*q*q cancel in the quotient.  rtol 2e-5: the figure test_l2norm_step_vs_oracle states for these sums."""
    nseg, _, ipseg = l2_plan(1, 1, n)
    assert nseg == min((n + SEG_MIN - 1) // SEG_MIN, SEG_CAP) and ipseg % 4 == 0
    if n > SEG_CAP * SEG_MIN:
        # the cap and the rounded segment length both apply.  (The rounding alone cannot change the number of segments:
        # with n = m*q + r, 1 <= r <= m, that needs m*q + r <= (m - 1)*(q + 4), i.e. q + r <= 4*(m - 1), while q >= 8192
        # and m <= SEG_CAP.  What it moves is every segment edge, and the planted values below sit on the moved edges.)
        assert nseg == SEG_CAP and ipseg != (n + nseg - 1) // nseg, "the capped case must round ipseg"
    for k, (signed, bits) in enumerate(((True, 8), (False, 4))):
        if n > SEG_CAP * SEG_MIN and k:
            continue                                     # the large case once: its reference costs a second
        lo, hi = O.qrange(signed, bits)
        x = _signed_or_relu((n,), signed, gen(800 + k))
        s, o = O.minmax_tensor(x, bits, signed)
        big = 4 * x.max()
        edges = torch.arange(ipseg, n, ipseg)
        x[edges] = big
        x[edges - 1] = big
        x[n - 1] = big
        want = _step_want(x, s, o, lo, hi, None)
        got = K.l2norm_step(x.to(DEV), s.to(DEV), o.to(DEV), lo, hi)
        assert got.shape == s.shape
        torch.testing.assert_close(got.cpu().double(), want, rtol=2e-5, atol=0)


def test_l2norm_step_per_tensor_flattens_outer_slices(K):
    """channels == 1 with outer > 1 through the C ABI: the entry point flattens the slices into one row and plans for that
    row, and the scratch size it reports for the same (outer, 1, inner) must be the one it then asks for."""
    n = N()
    outer, inner = 4, 20000                              # flat: 80000 elements, 5 segments of 16000
    lo, hi = O.qrange(True, 8)
    x = torch.randn(outer, 1, inner, generator=gen(810))
    s, o = O.minmax_tensor(x, 8, True)
    x.view(-1)[15999::16000] = 4 * x.max()
    want = _step_want(x, s, o, lo, hi, None)
    nb = n.lib.dlmcq_l2norm_scratch_bytes(outer, 1, inner)
    assert nb == l2_plan(1, 1, outer * inner)[0] * 2 * 4
    xd, sd, od = x.to(DEV), s.reshape(1).to(DEV), o.reshape(1).to(DEV)
    new = torch.empty(1, device=DEV)
    scr = torch.empty(nb // 4, device=DEV)
    n.check(n.lib.dlmcq_l2norm_step_f32(n.ptr(xd), n.ptr(sd), n.ptr(od), n.ptr(new), outer, 1, inner, lo, hi, n.ptr(scr), nb,
                                        n.stream_ptr()))
    torch.testing.assert_close(new.cpu().double().reshape(()), want, rtol=2e-5, atol=0)


PER_CHANNEL = [  # (shape, ch_axis, what the plan does)
    ((5, 3, 77), 1, "one row per segment"),
    ((7, 1000, 9), 1, "uneven last segment"),
    ((2, SEG_CAP + 1, 3), 1, "a single segment"),
    ((3, 257, 5), 1, "finalize needs a second workgroup"),
    ((300, 70), 0, "channel axis 0"),
]


@pytest.mark.parametrize("shape,ch_axis,what", PER_CHANNEL, ids=[p[2] for p in PER_CHANNEL])
def test_l2norm_step_per_channel_plans(K, shape, ch_axis, what):
    outer, ch, inner = math.prod(shape[:ch_axis]), shape[ch_axis], math.prod(shape[ch_axis + 1:])
    nseg, npseg, _ = l2_plan(outer, ch, inner)
    assert {"one row per segment": nseg == outer and npseg == 1, "uneven last segment": outer % npseg != 0 and nseg > 1,
            "a single segment": nseg == 1 and outer > 1, "finalize needs a second workgroup": ch > 256 and nseg > 1,
            "channel axis 0": outer == 1}[what]
    assert N().lib.dlmcq_l2norm_scratch_bytes(outer, ch, inner) == nseg * ch * 2 * 4
    red = tuple(i for i in range(len(shape)) if i != ch_axis)
    for k, (signed, bits) in enumerate(((True, 8), (False, 4))):
        lo, hi = O.qrange(signed, bits)
        x = _signed_or_relu(shape, signed, gen(820 + k))
        s, o = O.minmax_channel(x, bits, signed, ch_axis=ch_axis)
        # clipped values in the first and the last outer slice (see the per-tensor test): a dropped slice is seen
        big = 4 * x.max()
        first, last = x.select(0, 0) if ch_axis else x, x.select(0, shape[0] - 1) if ch_axis else x
        first[..., 0] = big
        last[..., -1] = big
        want = _step_want(x, s, o, lo, hi, red)
        got = K.l2norm_step(x.to(DEV), s.to(DEV), o.to(DEV), lo, hi)
        assert got.shape == s.shape
        torch.testing.assert_close(got.cpu().double(), want, rtol=2e-5, atol=0)


# ================================================================================ 2. l2norm_refine / dlmcq_l2norm_iterate
def _iterate(x, sc, off, state, geo, lo, hi, iterations, scr):
    n = N()
    n.check(n.lib.dlmcq_l2norm_iterate_f32(n.ptr(x), n.ptr(sc), n.ptr(off), n.ptr(state), *geo, int(lo), int(hi), int(iterations),
                                           1e-5, n.ptr(scr), scr.numel() * 4, n.stream_ptr()))


def l2norm_loop_f64_sums(x, n_bits, signed, ch_axis):
    """The oracle's l2norm loop with nothing changed but the precision of its two sums (float64, rounded to fp32 before
    the division).  Returns (scale [C], iterations)."""
    rows = x.reshape(1, -1) if ch_axis is None else x.transpose(0, ch_axis).reshape(x.shape[ch_axis], -1)
    s, o = O.minmax_channel(rows, n_bits, signed, ch_axis=0)
    lo, hi = O.qrange(signed, n_bits)
    diff, it = float("inf"), 0
    while diff > 1e-5 and it < 1000:
        q = O.quantize_codes(rows, s, o, lo, hi)
        new = ((rows * q).double().sum(dim=1).float() / (q * q + 1e-7).double().sum(dim=1).float()).reshape(s.shape)
        d = new - s
        diff = float((d.abs() / s).reshape(())) if ch_axis is None else float((d ** 2).sum().sqrt() / (s ** 2).sum().sqrt())
        s = new
        it += 1
    return s.reshape(-1), it


REFINE = [((SEG_MIN + 1,), None), ((3 * SEG_MIN + 5,), None), ((5, 3, 77), 1), ((7, 1000, 9), 1), ((3, 257, 5), 1)]
# (shape, signed) -> seed, where the default (840 + k) gives a tensor whose fixed point depends on the order of summation
REFINE_SEED = {((7, 1000, 9), True): 1200}


@pytest.mark.parametrize("shape,ch_axis", REFINE, ids=[str(p[0]) for p in REFINE])
def test_l2norm_refine_vs_oracle_loop(K, shape, ch_axis):
    """The device-side loop against the oracle's (same stopping rule of 1e-5; rtol 1e-4 as test_estimators_on_device): the
    converged scale, the iteration count within one of the oracle's, a converged state that further launches leave alone,
    and the same scale whether the host looks at the flag after every iteration or after every eighth.  One guarded
    iteration must equal `l2norm_step` bit for bit: the two kernels walk the same elements in the same order.
    The iteration rounds to codes, so it is not continuous in its sums: where (x - o)/(s + 1e-7) of one element lies on a
    rounding boundary, the last bit of a sum moves a code and with it that channel's fixed point.  Measured on the CPU
    alone: for (7,1000,9) signed 8 bit, seed 840, the oracle's loop with float64 sums ends 3.7e-4 away from the oracle in
    channel 501 and agrees to 3e-7 in the 999 others; for the committed seeds the two agree to 3e-7 everywhere.  The test
    asserts that condition (1e-5, and the same iteration count) on the CPU before it holds the kernel to rtol 1e-4."""
    for k, (signed, bits) in enumerate(((True, 8), (False, 4))):
        lo, hi = O.qrange(signed, bits)
        x = _signed_or_relu(shape, signed, gen(REFINE_SEED.get((shape, signed), 840 + k)))
        if ch_axis is None:
            s0, o0 = O.minmax_tensor(x, bits, signed)
            want, _, iters = O.l2norm_tensor(x, bits, signed, return_iters=True)
            geo = (1, 1, x.numel())
        else:
            s0, o0 = O.minmax_channel(x, bits, signed, ch_axis=ch_axis)
            want, _, iters = O.l2norm_channel(x, bits, signed, ch_axis=ch_axis, return_iters=True)
            geo = (math.prod(shape[:ch_axis]), shape[ch_axis], math.prod(shape[ch_axis + 1:]))
        assert 1 < iters < 200
        alt, alt_iters = l2norm_loop_f64_sums(x, bits, signed, ch_axis)
        assert alt_iters == iters and bool(((alt - want.reshape(-1)).abs() <= 1e-5 * alt).all()), \
            f"{shape} {'s' if signed else 'u'}{bits}: this seed's fixed point depends on the order of summation"
        xd, sd, od = x.to(DEV), s0.to(DEV), o0.to(DEV)
        got8 = K.l2norm_refine(xd, sd, od, lo, hi, ch_axis=ch_axis, batch=8)
        got1 = K.l2norm_refine(xd, sd, od, lo, hi, ch_axis=ch_axis, batch=1)
        assert got8.shape == s0.shape
        assert_bits_equal(got8, got1, f"{shape} batch 8 vs batch 1")
        close(got8, want, f"{shape} {'s' if signed else 'u'}{bits}", rtol=1e-4, atol=0)
        # the state machine, one iteration per launch
        sc = sd.reshape(-1).clone()
        off = od.reshape(-1).expand(sc.numel()).contiguous()
        state = torch.zeros(3, device=DEV)
        scr = torch.empty(N().lib.dlmcq_l2norm_scratch_bytes(*geo) // 4 + 1, device=DEV)
        _iterate(xd, sc, off, state, geo, lo, hi, 1, scr)
        assert_bits_equal(sc, K.l2norm_step(xd, sd, od, lo, hi), f"{shape}: first guarded iteration vs l2norm_step")
        assert state.cpu().tolist()[1] == 1.0
        launches = 1
        while float(state[0]) == 0.0 and launches < iters + 8:
            _iterate(xd, sc, off, state, geo, lo, hi, 1, scr)
            launches += 1
        st = state.cpu().tolist()
        assert st[0] == 1.0 and st[1] == float(launches), st
        assert abs(launches - iters) <= 1, f"{shape}: {launches} iterations on the device, {iters} in the oracle"
        assert_bits_equal(sc, got1, f"{shape}: launch by launch vs l2norm_refine")
        before_sc, before_st = sc.clone(), state.clone()
        _iterate(xd, sc, off, state, geo, lo, hi, 3, scr)
        assert_bits_equal(sc, before_sc, "scale after convergence")
        assert_bits_equal(state, before_st, "state after convergence")


# ============================================================================= 3. l2out_update state machine, both modes
L2OUT_D = (0.5, 0.3, 0.4, 0.2)       # out_q = out * (1 + d) + noise: improving, improving, worse, improving
L2OUT_R = 0.01                       # SUM noise^2 / SUM out^2 of those four steps


def _group_sum(t, per_channel):
    """Sums over axes (0, 2) of [B, C, L] as [1, C, 1] per channel, over everything as [1, 1, 1] per tensor."""
    return t.sum(dim=(0, 2), keepdim=True) if per_channel else t.sum().reshape(1, 1, 1)


def l2out_script(shape, per_channel, seed):
    """`out` and the five `out_q` of the script.  Within each group (a channel, or the whole tensor) out_q = alpha*out + nu
    with nu orthogonal to out and SUM nu^2 = r * SUM out^2, so the new scale is alpha / (alpha^2 + r) and the group's
    squared error ((1 - alpha)^2 + r) * SUM out^2.  The fifth step keeps the fourth's scale (r solved for it) at another
    alpha: it converges, and its error is 16% above the fourth's, so it is not a tie either."""
    g = gen(seed)
    b, c = shape[0], shape[1]
    out = torch.randn(shape, generator=g).double().reshape(b, c, -1)
    spread = 1 + 0.05 * torch.rand(1, c, 1, generator=g).double() if per_channel else torch.ones(1, 1, 1).double()
    oo = _group_sum(out * out, per_channel)
    steps = []
    alpha = r = None
    for k in range(5):
        if k < 4:
            alpha, r = 1 + L2OUT_D[k] * spread, torch.full_like(spread, L2OUT_R)
        else:
            ns4 = alpha / (alpha * alpha + r)
            alpha = alpha - 0.01
            r = alpha / ns4 - alpha * alpha
            assert bool((r > 0).all())
        nu = torch.randn(out.shape, generator=g).double()
        nu = nu - out * (_group_sum(nu * out, per_channel) / oo)
        nu = nu * (r * oo / _group_sum(nu * nu, per_channel)).sqrt()
        steps.append((alpha * out + nu).float().reshape(shape))
    return out.float().reshape(shape), steps


def l2out_replay(out, oq, scale, best, state, per_channel):
    """One step of l2_update_kernel after l2out_sums_kernel, sums in float64.  scale / best are float64 [C]; state is
    [done, iterations, best mse].  Returns (diff, mse, better) for the caller's margins."""
    if state[0] != 0.0:
        return None
    b, c = out.shape[0], out.shape[1]
    o3, q3 = out.reshape(b, c, -1), oq.reshape(b, c, -1)
    a = _group_sum((o3 * q3).double(), per_channel).reshape(-1)
    bb = _group_sum((q3 * q3 + 1e-7).double(), per_channel).reshape(-1)
    d = o3 - q3
    mse = float((d * d).double().sum()) / (out.numel() // c)
    new = a / bb
    if new.numel() == 1:
        diff = float((new - scale).abs() / scale)
    else:
        diff = float(((new - scale) ** 2).sum().sqrt() / (scale ** 2).sum().sqrt())
    better = mse < state[2]
    if better:
        best[:] = scale if per_channel else new      # mode 2 keeps the OLD scale, mode 1 the NEW one
        state[2] = mse
    scale[:] = new
    state[1] += 1.0
    if not diff > 1e-5:
        state[0] = 1.0
    return diff, mse, better


L2OUT = [((2, 16, 40, 40), False), ((3, 5, 33), True), ((2, 300, 7), True), ((4, 1, 50), True)]


@pytest.mark.parametrize("shape,per_channel", L2OUT, ids=[f"{s}-{'channel' if p else 'tensor'}" for s, p in L2OUT])
def test_l2out_update_state_machine(K, shape, per_channel):
    """dlmcq_l2out_update_f32 fed (out, out_q) pairs directly - no layer in the loop - against a float64 replay after each of
    five scripted steps: two that improve the error, one that is worse, one that improves again, one that converges; then
    one more call, which must change nothing.  Per tensor (mode 1) the best scale is the NEW one of an improving step, per
    channel (mode 2) the OLD one, held in the staging half of `best`: both are required bit for bit against the scales the
    kernel itself held before and after the step.  (2,16,40,40) is four segments of one flat row; (2,300,7) strides the
    update over more than 256 channels and reduces the stopping norm across threads; (4,1,50) is one channel on the
    per-channel plan, which takes the per-tensor stopping rule.  Measured on the CPU: consecutive errors differ by 14% to
    71%, every stopping quotient is above 5e-2 or below 1e-6; the sums are those of l2norm_step, rtol 2e-5."""
    out, steps = l2out_script(shape, per_channel, 860)
    c = shape[1] if per_channel else 1
    s_init = 0.5 + torch.rand(c, generator=gen(861))
    st = K.OutputAwareState(s_init.to(DEV))
    scale, best, state = s_init.double().clone(), s_init.double().clone(), [0.0, 0.0, float("inf")]
    outd = out.to(DEV)
    verdicts, prev_mse = [], None
    for k, oq in enumerate(steps):
        old = st.scale.clone()
        old_best = st.best[:c].clone()
        diff, mse, better = l2out_replay(out, oq, scale, best, state, per_channel)
        assert diff > 5e-2 or diff < 1e-6, f"step {k}: stopping quotient {diff} is too near 1e-5"
        if prev_mse is not None:
            assert abs(mse - prev_mse) >= 0.01 * max(mse, prev_mse), f"step {k}: errors {prev_mse} and {mse} are a near tie"
        prev_mse = mse
        verdicts.append(better)
        K.l2out_update(outd, oq.to(DEV), st, per_channel)
        tag = f"{shape} step {k}"
        close(st.scale.double(), scale, tag + " scale", rtol=2e-5, atol=0)
        assert_bits_equal(st.best[:c], (old if per_channel else st.scale) if better else old_best, tag + " best")
        close(st.best[:c].double(), best, tag + " best vs replay", rtol=2e-5, atol=0)
        got = st.state.cpu().tolist()
        assert got[0] == state[0] and got[1] == state[1], f"{tag}: state {got} vs {state}"
        assert abs(got[2] - state[2]) <= 2e-5 * state[2], f"{tag}: best mse {got[2]} vs {state[2]}"
    assert verdicts == [True, True, False, True, False] and state[0] == 1.0 and st.done() and st.iterations() == 5
    frozen = [t.clone() for t in (st.scale, st.best, st.state)]
    K.l2out_update(outd, steps[0].to(DEV), st, per_channel)
    for t, f, name in zip((st.scale, st.best, st.state), frozen, ("scale", "best", "state")):
        assert_bits_equal(t, f, f"{shape}: {name} after done")


def test_output_aware_channel_scale_end_to_end():
    """quantize_l2norm_output_channel on a small conv - x (4,3,12,12), w (8,3,3,3), 4 bit signed, patience 12 - against the
    oracle's loop; rtol 2e-4 as its per-tensor counterpart."""
    import torch.nn.functional as F
    from dlmc.quantization.scalar import ops

    class Layer:
        def _forward_func(self, x, w):
            return F.conv2d(x, w, None, 1, 1)
    g = gen(870)
    x = torch.randn(4, 3, 12, 12, generator=g)
    w = torch.randn(8, 3, 3, 3, generator=g) * 0.2
    conv = nn.Conv2d(3, 8, 3, padding=1, bias=False)
    s_ref, o_ref = O.l2norm_output_channel(conv, x, w, 4, True, patience=12)
    s, o = ops.quantize_l2norm_output_channel(x.to(DEV), w.to(DEV), Layer(), 4, True, patience=12)
    assert s.shape == (8, 1, 1, 1) and o.shape == (8, 1, 1, 1)
    assert_bits_equal(o, o_ref, "offset")
    close(s, s_ref, "output-aware per-channel scale", rtol=2e-4, atol=0)


# ============================================================================================ 4. l2loss_tensor
def l2loss_tensor_replay(x, vmax, vmin, n_bits, loss_div):
    """ops.py:36-68 with the candidates in fp32 exactly as O.l2loss_tensor and the losses in float64.
    Returns (scale, zero point, smallest relative gap between a candidate's loss and the running best, losses)."""
    qmax = 2 ** n_bits - 1
    mn = torch.zeros((), dtype=torch.float32) if vmin is None else vmin
    best, gap, losses = 1000.0, float("inf"), []
    scale, offset = vmax / qmax, torch.zeros(())
    for i in range(80):
        nmx, nmn = (1 - 0.01 * i) * vmax, (1 - 0.01 * i) * mn
        ns = (nmx - nmn) / qmax
        nz = torch.round(-nmn / ns)
        q = ((torch.round(x / ns) + nz).clamp(0, qmax) - nz) * ns
        d = q - x
        loss = float((d * d).double().sum()) / loss_div
        losses.append(loss)
        gap = min(gap, abs(loss - best) / max(loss, best))
        if loss < best:
            best, scale, offset = loss, ns, nz
    return scale, offset, gap, losses


def _l2loss_input(shape, seed):
    g = gen(seed)
    return torch.relu(torch.randn(shape, generator=g)) + 0.01 * torch.rand(shape, generator=g)


L2LOSS_T = [((SEG_MIN,), 900), ((SEG_MIN + 1,), 901), ((50001,), 902), ((6, 4, 50, 50), 903)]


@pytest.mark.parametrize("shape,seed", L2LOSS_T, ids=[str(p[0]) for p in L2LOSS_T])
def test_l2loss_tensor_across_workgroups(K, shape, seed):
    """The 80-candidate shrink search over one, two and four workgroups, and a 4-D tensor whose loss divisor is not 1, for
    unsigned 4 and 8 bit, with the tensor's minimum and without (allow_offset=False).  The pick is a chain of strict
    comparisons on fp32 sums, so it is replayed in float64; the kernel's fp32 sum of n positive terms is within
    (n/(256*blocks) + 9) * 2^-24 < 1e-5 of that, and the committed seeds keep every decision at least 1e-4 apart (asserted
    here, on the CPU), so the result must equal the replay's bit for bit.
    Smallest gap of each committed seed, measured with the replay alone (u4, then u8; with and without the minimum they
    agree to the digits shown): 16384: 4.2e-3, 7.4e-3; 16385: 1.5e-3, 3.2e-3; 50001: 9.0e-4, 9.0e-4; (6,4,50,50): 1.4e-3,
    1.9e-3."""
    x = _l2loss_input(shape, seed)
    x2 = x if x.dim() >= 2 else x.reshape(1, -1)
    loss_div = x2.numel() // x2.shape[1]
    assert (loss_div != 1) == (len(shape) == 4)
    mx, mn = x.max(), x.min()
    xd = x2.to(DEV)
    for bits in (4, 8):
        for vmin in (mn, None):
            s, z, gap, _ = l2loss_tensor_replay(x, mx, vmin, bits, loss_div)
            tag = f"{shape} u{bits}{'' if vmin is not None else ' no minimum'}"
            assert gap >= 1e-4, f"{tag}: a decision of this seed is only {gap:.3g} apart"
            gs, gz = K.l2loss_tensor(xd, mx.to(DEV), None if vmin is None else vmin.to(DEV), bits)
            assert_bits_equal(gs, s, tag + " scale")
            assert_bits_equal(gz, z, tag + " zero point")


def test_l2loss_tensor_nothing_below_the_initial_1000(K):
    """The reference starts from `min_loss = 1000`: a tensor scaled so that every candidate's loss is above it returns the
    initial (max / qmax, 0) - bit for bit, the zero a positive one."""
    x = _l2loss_input((SEG_MIN + 1,), 901) * 1024.0
    mx, mn = x.max(), x.min()
    for bits in (4, 8):
        _, _, _, losses = l2loss_tensor_replay(x, mx, mn, bits, 1)
        assert min(losses) >= 1000 * (1 + 1e-4)
        gs, gz = K.l2loss_tensor(x.reshape(1, -1).to(DEV), mx.to(DEV), mn.to(DEV), bits)
        assert_bits_equal(gs, mx / (2 ** bits - 1), f"u{bits} scale")
        assert_bits_equal(gz, torch.zeros(()), f"u{bits} zero point")


# ============================================================================================== 5. l2loss_rows
def _bits(v):
    return torch.tensor(v, dtype=torch.float32).view(torch.int32).item()


def l2loss_row_replay(row, s0, o0, n_bits, tol):
    """The 80 sequential steps of O.l2loss_channel for one row - aliasing quirk included: once a step is accepted the
    following candidates shrink the accepted ZERO POINT - with fp32 candidates and float64 losses.  A decision whose two
    sides are nearer than `tol` (relative) is taken both ways.  Returns (the set of reachable (scale, offset) pairs as
    fp32 bit patterns, the smallest gap over ALL decisions, the number of decisions that were taken both ways)."""
    qmax = 2 ** n_bits - 1
    mx = o0 + s0 * qmax
    paths = {(float(s0), float(o0), math.copysign(1.0, float(o0)), 1000.0)}      # (-0.0 == 0.0 in a set: the sign rides along)
    min_gap, branched = float("inf"), 0
    for i in range(80):
        nxt = set()
        for s, off, sign, best in paths:
            off_t = torch.tensor(off, dtype=torch.float32)          # (keeps the sign of a zero)
            nmn, nmx = (1 - 0.01 * i) * off_t, (1 - 0.01 * i) * mx
            ns = (nmx - nmn) / qmax
            nz = torch.round(-nmn / ns)
            q = ((torch.round(row / ns) + nz).clamp(0, qmax) - nz) * ns
            d = row - q
            loss = float((d * d).double().sum())
            if math.isnan(loss):
                nxt.add((s, off, sign, best))         # `best > nan` is false: never accepted
                continue
            gap = abs(loss - best) / max(loss, best) if max(loss, best) > 0 else 0.0
            taken = (float(ns), float(nz), math.copysign(1.0, float(nz)), loss)
            min_gap = min(min_gap, gap)
            if gap < tol:
                branched += 1
                nxt.add((s, off, sign, best))
                nxt.add(taken)
            else:
                nxt.add(taken if best > loss else (s, off, sign, best))
        paths = nxt
        assert len(paths) <= 16, "the replay branches without bound"
    return {(_bits(s), _bits(off)) for s, off, _, _ in paths}, min_gap, branched


def _rows_input(rows, inner, kind, seed):
    g = gen(seed)
    if kind == "s4":
        return torch.randn(rows, inner, generator=g) * 0.25, 4, True     # (0.25: a 9001-element row's loss stays below the 1000)
    x = torch.relu(torch.randn(rows, inner, generator=g)) + 0.01 * torch.rand(rows, inner, generator=g)
    return x, (4 if kind == "u4" else 8), False


def _check_rows(K, x, n_bits, signed, tol, exact):
    s0, o0 = O.minmax_channel(x, n_bits, signed, ch_axis=0)
    gs, go = K.l2loss_rows(x.to(DEV), s0.to(DEV), o0.to(DEV), n_bits)
    assert gs.shape == s0.shape and go.shape == o0.shape
    gs, go = gs.cpu().reshape(-1), go.cpu().reshape(-1)
    single, gaps, branchings = 0, [], []
    for r in range(x.shape[0]):
        reach, gap, branched = l2loss_row_replay(x[r], s0.reshape(-1)[r], o0.reshape(-1)[r], n_bits, tol)
        gaps.append(gap)
        branchings.append(branched)
        if exact:          # (not `len(reach) == 1`: two branches can meet again on a later candidate)
            assert branched == 0 and gap >= tol, f"row {r}: a decision of this seed is only {gap:.3g} apart"
        assert len(reach) <= (1 if exact else 4), f"row {r}: {len(reach)} reachable results"
        single += len(reach) == 1
        got = (_bits(float(gs[r])), _bits(float(go[r])))
        assert got in reach, f"row {r}: got bits {got} of {(float(gs[r]), float(go[r]))}, reachable bits {reach}"
    assert 4 * single >= 3 * x.shape[0], "the branching must stay the exception"
    return min(gaps), branchings


ROW_INNER = [1, 63, 64, 255, 256, 257, 8192, 8193, 9001]
# (inner, kind) -> seed, where the default (920 + index) leaves a row with a decision inside the branching tolerance
ROW_SEED = {(256, "s4"): 1102, (8192, "s4"): 1102, (9001, "s4"): 1100}


@pytest.mark.parametrize("inner", ROW_INNER)
@pytest.mark.parametrize("kind", ["u4", "u8", "s4"])
def test_l2loss_rows_strides_and_row_cache(K, inner, kind):
    """Three rows per case; inner below, at and above one 256-thread stride and one wave, 8192 the last size whose row is
    kept in LDS, 8193 the first that is re-read from memory.  Unsigned rows (relu(randn) + 0.01*rand): every decision of
    the committed seeds is at least 1e-4 apart (asserted on the CPU) and the result is required bit for bit.  Signed 4 bit
    Gaussian rows have a loss that is flat near its minimum (decisions 1e-6 to 5e-5 apart), so the replay takes a decision
    both ways when it is nearer than 2*(inner/256 + 9)*2^-24 - twice the bound of the kernel's fp32 sum - and the kernel's
    (scale, offset) must be one of the reachable pairs: at most 4 per row, and exactly one for three rows in four.
    Measured with the replay alone: the smallest gap of an unsigned case is 1.2e-4 (u4, 8192), of the others 1.7e-4 and
    more; no row of a committed signed seed branches (the default seeds left 1 or 2 rows of 3 branching at 256, 8192 and 9001),
    and their nearest decisions that are not branched lie between 1.6e-6 and 3.6e-5."""
    x, n_bits, signed = _rows_input(3, inner, kind, ROW_SEED.get((inner, kind), 920 + ROW_INNER.index(inner)))
    if signed:           # (a row of one element has a one-term sum: nothing to allow for, and its exact ties stay ties)
        _check_rows(K, x, n_bits, True, 2 * (inner / 256 + 9) * 2.0 ** -24 if inner > 1 else 0.0, exact=False)
    else:
        _check_rows(K, x, n_bits, False, 1e-4, exact=True)


@pytest.mark.parametrize("inner,seed", [(256, 924), (8192, 1101), (9001, 928)])
def test_l2loss_rows_one_row_of_four_branches(K, inner, seed):
    """Four signed 4 bit rows of which exactly one has decisions inside the tolerance (asserted on the CPU; measured with
    the replay alone: 3 such decisions, the nearest 1.4e-7 apart, at 256; 1 at 4.0e-6 at 8192; 1 at 1.1e-7 at 9001), so the
    both-ways replay is exercised and its caps hold with a row that branches: two reachable pairs for that row, one for the
    others, and the kernel's result among them."""
    x, n_bits, _ = _rows_input(4, inner, "s4", seed)
    _, branchings = _check_rows(K, x, n_bits, True, 2 * (inner / 256 + 9) * 2.0 ** -24, exact=False)
    assert sorted(b > 0 for b in branchings) == [False, False, False, True]


def test_l2loss_rows_many_rows_and_a_row_nothing_fits(K):
    """300 rows (one workgroup each) of 40 elements, unsigned 8 bit, bit for bit; row 7 is scaled until every candidate's
    loss is above the initial 1000, so nothing is accepted and the kernel must hand back the scale and offset it was given."""
    x, n_bits, _ = _rows_input(300, 40, "u8", 950)
    x[7] = x[7] * 1e5
    s0, o0 = O.minmax_channel(x, n_bits, False, ch_axis=0)
    _check_rows(K, x, n_bits, False, 1e-4, exact=True)
    reach, _, _ = l2loss_row_replay(x[7], s0[7, 0], o0[7, 0], n_bits, 1e-4)
    assert reach == {(_bits(float(s0[7, 0])), _bits(float(o0[7, 0])))}, "row 7 must accept nothing"
    x4, _, _ = _rows_input(3, 257, "u4", 951)
    x4[1] = x4[1] * 1e3
    s0, o0 = O.minmax_channel(x4, 4, False, ch_axis=0)
    reach, _, _ = l2loss_row_replay(x4[1], s0[1, 0], o0[1, 0], 4, 1e-4)
    assert reach == {(_bits(float(s0[1, 0])), _bits(float(o0[1, 0])))}
    _check_rows(K, x4, 4, False, 1e-4, exact=True)


# ======================================================================================= 6. AdaRound and span_scale
@pytest.mark.parametrize("inner", [255, 256, 257, 1153])
def test_adaround_rows_longer_than_one_stride(K, inner):
    """K = 3 rows below, at and above one 256-thread stride, and 1153 = 128*3*3 + 1.  Eval form bit for bit; training form
    and gradients against CPU autograd at the tolerances of test_adaround_fused_matches_the_reference_chain; g_scale
    against a float64 sum (its terms must not cancel by more than 100 to 1, asserted, for the relative bound to hold)."""
    g = gen(960 + inner + {257: 3, 1153: 1}.get(inner, 0))       # (seeds whose g_scale terms cancel by less than 50 to 1)
    lo, hi = -7, 7
    w = torch.randn(3, inner, generator=g) * 0.1
    s = O.minmax_channel(w, 4, True, ch_axis=0)[0] + 1e-6
    alpha = torch.randn(3, inner, generator=g) * 2.0
    gy = torch.randn(3, inner, generator=g)
    wd, ad, sd, gd = w.to(DEV), alpha.to(DEV), s.to(DEV), gy.to(DEV)
    assert_bits_equal(K.adaround_weight(wd, ad, sd, lo, hi, False), O.fq_adaround(w, s, alpha, lo, hi, training=False)[1], "eval")
    a_ref, s_ref = alpha.clone().requires_grad_(True), s.clone().requires_grad_(True)
    q = torch.floor(w / s_ref) + torch.clamp(torch.sigmoid(a_ref) * (1.1 - (-0.1)) + (-0.1), 0, 1)
    y_ref = q.clamp(lo, hi) * s_ref
    y_ref.backward(gy)
    close(K.adaround_weight(wd, ad, sd, lo, hi, True), y_ref.detach(), "train", rtol=1e-5, atol=1e-6)
    ga, gs = K.adaround_weight_backward(wd, ad, sd, gd, lo, hi)
    close(ga, a_ref.grad, "g_alpha", rtol=1e-4, atol=1e-6)
    terms = (gy * q.detach().clamp(lo, hi)).double()
    want_gs = terms.sum(dim=1, keepdim=True)
    assert bool((terms.abs().sum(dim=1, keepdim=True) < 100 * want_gs.abs()).all())
    assert gs.shape == s.shape
    close(gs.double(), want_gs, "g_scale", rtol=1e-4, atol=1e-5)
    ga2, none = K.adaround_weight_backward(wd, ad, sd, gd, lo, hi, want_scale=False)
    assert none is None
    assert_bits_equal(ga2, ga, "g_alpha alone")
    none, gs2 = K.adaround_weight_backward(wd, ad, sd, gd, lo, hi, want_alpha=False)
    assert none is None
    assert_bits_equal(gs2, gs, "g_scale alone")


@pytest.mark.parametrize("channels", [1, 255, 256, 257])
def test_span_scale_channel_counts(K, channels):
    """(max - min) / span with a true division, from the observer's [max | -min] pair, at one workgroup and past it."""
    x = torch.randn(channels, 37, generator=gen(970 + channels))
    mx, neg_mn = K.minmax(x.to(DEV), ch_axis=0, mode=N().MINMAX_NEGMIN)
    assert_bits_equal(mx, x.amax(dim=1), "max")
    assert_bits_equal(neg_mn, -x.amin(dim=1), "-min")
    for span in (255.0, 15.0, 3.0):
        got = K.span_scale(mx, neg_mn, span)
        assert got.shape == (channels,)
        assert_bits_equal(got, (mx.cpu() - (-neg_mn.cpu())) / span, f"span {span}")


# ======================================================================================== 7. fold_bn_ and repvgg_fuse
def _randomise_bn(bn, g):
    with torch.no_grad():
        bn.weight.copy_(torch.rand(bn.weight.shape, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(bn.bias.shape, generator=g) * 0.1)
        bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=g) + 0.3)
    return bn


def _bn_tuple(bn):
    return tuple(t.detach().cpu().clone() for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var))


FOLD = [("1x1, 255 inputs", lambda: nn.Conv2d(255, 5, 1)), ("1x1, 257 inputs", lambda: nn.Conv2d(257, 5, 1)),
        ("3x3, 64 inputs", lambda: nn.Conv2d(64, 6, 3, padding=1)), ("linear, 1 input", lambda: nn.Linear(1, 7)),
        ("3x3, 64 inputs, no bias", lambda: nn.Conv2d(64, 4, 3, padding=1, bias=False))]


@pytest.mark.parametrize("what,make", FOLD, ids=[f[0] for f in FOLD])
def test_fold_bn_rows_longer_than_one_stride(what, make):
    """fold_bn_ with inner = 255, 257, 576 and 1, and a conv without a bias (which gets a zero one), bit for bit."""
    from dlmc.utils.merge_bn import fold_bn_
    torch.manual_seed(2333 + 980)
    g = gen(980)
    layer = make()
    cout = layer.weight.shape[0]
    bn = _randomise_bn(nn.BatchNorm2d(cout), g)
    assert layer.weight.numel() // cout == {"1x1, 255 inputs": 255, "1x1, 257 inputs": 257, "linear, 1 input": 1}.get(what, 576)
    w0 = layer.weight.detach().clone()
    b0 = None if layer.bias is None else layer.bias.detach().clone()
    want_w, want_b = O.fold_bn(w0, b0, *_bn_tuple(bn))
    layer, bn = layer.to(DEV), bn.to(DEV)
    with torch.no_grad():
        fold_bn_(layer, bn)
    assert_bits_equal(layer.weight, want_w, what + " weight")
    assert layer.bias is not None
    assert_bits_equal(layer.bias, want_b, what + " bias")


class _Branch(nn.Module):
    def __init__(self, cin, cout, k, groups):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, padding=k // 2, groups=groups, bias=False)
        self.bn = nn.BatchNorm2d(cout)


class _RepBlock(nn.Module):
    """The attribute names of the reference's RepVGGBlock, which is all dlmc.utils.reparam looks at."""

    def __init__(self, cin, cout, groups, identity):
        super().__init__()
        self.rbr_dense = _Branch(cin, cout, 3, groups)
        self.rbr_1x1 = _Branch(cin, cout, 1, groups)
        if identity:
            self.rbr_identity = nn.BatchNorm2d(cin)


REPVGG = [(29, 29, 1, True), (58, 58, 2, True), (64, 64, 1, True), (128, 128, 2, True), (29, 7, 1, False), (64, 5, 1, False)]


@pytest.mark.parametrize("cin,cout,groups,identity", REPVGG)
def test_repvgg_fuse_rows_longer_than_one_stride(cin, cout, groups, identity):
    """29 and 64 input channels per group (261 and 576 taps per output channel: one row takes two and three strides), one and
    two groups with the identity branch - whose tap is chosen by `k % cin_per_group` - and one group without it."""
    from dlmc.utils.reparam import fused_kernel_bias
    torch.manual_seed(2333 + 990)
    g = gen(990)
    blk = _RepBlock(cin, cout, groups, identity)
    assert blk.rbr_dense.conv.weight.shape[1] in (29, 64)
    for bn in [blk.rbr_dense.bn, blk.rbr_1x1.bn] + ([blk.rbr_identity] if identity else []):
        _randomise_bn(bn, g)

    def bn5(bn):
        return _bn_tuple(bn) + (bn.eps,)
    want_k, want_b = O.repvgg_fuse(blk.rbr_dense.conv.weight.detach().clone(), bn5(blk.rbr_dense.bn),
                                   blk.rbr_1x1.conv.weight.detach().clone(), bn5(blk.rbr_1x1.bn),
                                   bn5(blk.rbr_identity) if identity else None, groups=groups)
    got_k, got_b = fused_kernel_bias(blk.to(DEV))
    assert_bits_equal(got_k, want_k, "kernel")
    assert_bits_equal(got_b, want_b, "bias")
