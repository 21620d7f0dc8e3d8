"""The squeeze kernel (csrc/squeeze_i8.hip, dlmcq_squeeze_gate_i8) against the float64 reference of tests/squeeze_cases.py, byte for byte:
all four instantiations, every loop trip, the hidden quantiser's four forms at full-range operands, the epilogue's hard values (NaN,
+-inf, -0, exact and awkward ties, the clamp bounds) through the hidden quantiser and into the gate functions, integer sums at and above
2^24 (tests/test_squeeze_cases_host.py proves on the CPU that every case holds these facts).

Every launch goes through the raw entry point into views of pattern-filled parents: the guard rows before and behind `gate` and `hidden`
stay as they were.  Per case:
  from the integers          inner none / relu: `hidden` and `gate` (gate_fn none) equal the reference bit for bit, NaN for NaN and the sign
                             of a zero included; the selector channels give fl32((qh - zp2) s_h); `gate` alone and `hidden` alone return
                             the same bytes.
  from the launch's hidden   every inner activation, swish included: gate(none) equals the reference's second half applied to the
                             launch's own `hidden`.  For swish `hidden` is held to the bound dlmcq_swish_nhwc_f32's header states - within
                             3 * 2^-23 relative of float64 h sigmoid(h) of the reference's pre-activation h for |h| <= 80 - on the results
                             in the normal range (below 2^-126 a value has no relative precision to hold to; denormals are compared through
                             their codes by the line above).  The largest ratio is printed.
  the gate functions         on the launch's own gate(none) v, edge values through bias2 included: hard sigmoid is F.relu6(v + 3) / 6 on
                             the device; sigmoid is held to test_gpu_squeeze.py's bound (imported) on finite v, to the device's own three
                             steps on the others, and to MATCHES_TORCH_SIGMOID.
Then: K.squeeze_gate once per instantiation; every image's rows equal those of the image launched alone, once per instantiation; the
range -1 .. 200 is refused and nothing is written."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import exact_layers as X
import squeeze_cases as Q
from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from test_gpu_squeeze import MATCHES_TORCH_SIGMOID, same, sigmoid_ratio

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PATTERN = 0x7fc12345
ACT = {None: N.SQUEEZE_NONE, "relu": N.SQUEEZE_RELU, "swish": N.SQUEEZE_SWISH}
FN = {None: N.GATE_NONE, "sigmoid": N.GATE_SIGMOID, "hardsigmoid": N.GATE_HARDSIGMOID}
SWISH_BOUND = 3 * 2.0 ** -23
WORST = {"swish": 0.0}
PER_INSTANTIATION = {v: next(c.cid for c in Q.RUN if Q.shape_facts(c.c, c.r4)[0] == v and c.n >= 5 and c.bias) for v in
                     [(a, b) for a in (True, False) for b in (True, False)]}


def t(v):
    return None if v is None else torch.tensor([float(v)], dtype=torch.float32, device=DEV)


@functools.lru_cache(maxsize=None)
def device_operands(cid):
    case, ops = Q.BY_ID[cid], Q.operands(cid)
    d = lambda x: None if x is None else x.to(DEV)  # noqa: E731
    q = case.quant
    return dict(codes=d(ops["codes"]), w1=d(ops["w1"]), wsum1=d(ops["w1"].sum(1, dtype=torch.int32)), b1=d(ops["b1"]), s_in=t(ops["s_in"]),
                zp1=t(ops["zp1"]), ws1=d(ops["ws1"]), w2=d(ops["w2"]), wsum2=d(ops["w2"].sum(1, dtype=torch.int32)), b2=d(ops["b2"]),
                ws2=d(ops["ws2"]), qs=t(q.scale), qz=t(q.zp))


def launch(cid, inner, fn, gate=True, hidden=True, image=None):
    """One raw call of the case (`image`: that image alone, N = 1).  Returns (rc, gate or None, hidden or None) - CPU copies of the
    views - after asserting that the guard rows around both outputs, and an output that was not asked for, kept their pattern."""
    case, o = Q.BY_ID[cid], device_operands(cid)
    q = case.quant
    n = case.n if image is None else 1
    codes = o["codes"] if image is None else o["codes"][image:image + 1]
    gp = torch.full((n + 2, case.c), PATTERN, dtype=torch.int32, device=DEV)
    hp = torch.full((n + 2, case.r4), PATTERN, dtype=torch.int32, device=DEV)
    gv, hv = gp[1:n + 1].view(torch.float32), hp[1:n + 1].view(torch.float32)
    p = lambda x: None if x is None else ctypes.c_void_p(x.data_ptr())  # noqa: E731
    rc = N.lib.dlmcq_squeeze_gate_i8(p(codes), p(o["w1"]), p(o["wsum1"]), p(o["b1"]), p(o["s_in"]), p(o["zp1"]), p(o["ws1"]), ACT[inner], p(o["w2"]),
                                     p(o["wsum2"]), p(o["b2"]), p(o["ws2"]), FN[fn], p(gv) if gate else None, p(hv) if hidden else None, n, case.c,
                                     case.r4, int(case.uns), p(o["qs"]), p(o["qz"]), q.lo, q.hi, q.form, q.g, N.stream_ptr())
    torch.cuda.synchronize()
    for parent, asked in ((gp, gate), (hp, hidden)):
        assert bool((parent[0] == PATTERN).all()) and bool((parent[-1] == PATTERN).all()), (cid, "a guard row was written")
        assert asked and rc == 0 or bool((parent == PATTERN).all()), (cid, "an output that was not asked for, or a refused call, wrote")
    return rc, (gv.cpu() if gate and rc == 0 else None), (hv.cpu() if hidden and rc == 0 else None)


def bits_differ(a, b):
    return int((a.view(torch.int32) != b.view(torch.int32)).sum())


@pytest.mark.parametrize("cid", [c.cid for c in Q.RUN])
def test_case(cid):
    case, ops = Q.BY_ID[cid], Q.operands(cid)
    q, sel = case.quant, ops["sel"]
    gate0 = None
    for inner in Q.INNER:
        ref = Q.reference(cid, inner)
        rc, gate, hidden = launch(cid, inner, None)
        assert rc == 0
        # ---- from the integers
        if inner != "swish":
            assert same(hidden, ref["h"]), (cid, inner, "hidden", bits_differ(hidden, ref["h"]))
            assert same(gate, ref["v"]), (cid, inner, "gate", bits_differ(gate, ref["v"]))
            want = ((ref["qh"][:, :sel] - Q.zp2_of(q)).double() * X.dequant_scale(q)).float()
            assert same(gate[:, :sel], want), (cid, inner, "selector channels")
        else:
            pre, want = ref["pre"].double(), Q.swish64(ref["pre"])
            held = (pre.abs() <= 80) & (want.abs() >= 2.0 ** -126)
            ratio = float(((hidden.double() - want).abs()[held] / (SWISH_BOUND * want.abs()[held])).max()) if bool(held.any()) else 0.0
            WORST["swish"] = max(WORST["swish"], ratio)
            print(f"{cid}: swish largest |h - h*| / (3 * 2^-23 |h*|) = {ratio:.3f} over {int(held.sum())} values; so far {WORST['swish']:.3f}")
            assert ratio <= 1.0, (cid, ratio)
            assert torch.equal(hidden.isnan(), pre.isnan() | (pre == -float("inf")))          # -inf * 0
        # ---- from the launch's own hidden
        assert same(gate, Q.second_half(ops, q, hidden)[2]), (cid, inner, "gate from the launch's hidden")
        if inner is None:
            gate0 = gate
            assert same(launch(cid, inner, None, hidden=False)[1], gate) and same(launch(cid, inner, None, gate=False)[2], hidden)
    # ---- the gate functions on the launch's own v (inner none)
    v = gate0.to(DEV)
    hs = launch(cid, None, "hardsigmoid", hidden=False)[1]
    assert same(hs, (F.relu6(v + 3) / 6).cpu()), (cid, "hardsigmoid")
    sg = launch(cid, None, "sigmoid", hidden=False)[1].to(DEV)
    fin = v.isfinite()
    ratio = sigmoid_ratio(sg[fin], v[fin])
    assert ratio <= 1.0, (cid, "sigmoid", ratio)
    assert same(sg[~fin], 1.0 / (1.0 + torch.exp(-v[~fin]))), (cid, "sigmoid of the values that are not finite")
    differ = int((sg[fin] != torch.sigmoid(v[fin])).sum())
    if MATCHES_TORCH_SIGMOID:
        assert differ == 0, (cid, "sigmoid differs from torch.sigmoid on the device", differ)


@pytest.mark.parametrize("inst", sorted(PER_INSTANTIATION), ids=lambda v: f"V1_{v[0]}_V2_{v[1]}")
def test_wrapper(inst):
    cid = PER_INSTANTIATION[inst]
    case, o = Q.BY_ID[cid], device_operands(cid)
    q = case.quant
    l1 = dict(wq=o["w1"], wsum=o["wsum1"], bias=o["b1"], in_scale=o["s_in"], in_zp=o["zp1"], w_scale=o["ws1"])
    l2 = dict(wq=o["w2"], wsum=o["wsum2"], bias=o["b2"], w_scale=o["ws2"])
    for inner in (None, "relu"):
        ref = Q.reference(cid, inner)
        gate, hidden = K.squeeze_gate(o["codes"], l1, inner, K.EmitCodes(o["qs"], o["qz"], q.lo, q.hi, q.form, q.g), l2, None, want_hidden=True)
        assert same(hidden.cpu(), ref["h"]) and same(gate.cpu(), ref["v"]), (cid, inner)


@pytest.mark.parametrize("inst", sorted(PER_INSTANTIATION), ids=lambda v: f"V1_{v[0]}_V2_{v[1]}")
def test_images_are_independent(inst):
    """Image i's rows equal those of the same image launched alone, whatever slot of its workgroup it sat in."""
    cid = PER_INSTANTIATION[inst]
    case = Q.BY_ID[cid]
    _, gate, hidden = launch(cid, "relu", "hardsigmoid")
    for i in range(case.n):
        rc, g1, h1 = launch(cid, "relu", "hardsigmoid", image=i)
        assert rc == 0 and same(g1[0], gate[i]) and same(h1[0], hidden[i]), (cid, i)


def test_the_range_that_is_neither_uint8_nor_int8_is_refused():
    """-1 .. 200: the codes above 127 have no byte that layer 2 could re-read with the range's sign.  DLMCQ_EINVAL, and
    nothing is written (`launch` asserts it); the wrappers say the same."""
    (case,) = [c for c in Q.CASES if c.kind == "mixed"]
    for gate, hidden in ((True, True), (True, False), (False, True)):
        assert launch(case.cid, None, None, gate=gate, hidden=hidden)[0] == -1
    o, q = device_operands(case.cid), case.quant
    l1 = dict(wq=o["w1"], wsum=o["wsum1"], bias=o["b1"], in_scale=o["s_in"], in_zp=o["zp1"], w_scale=o["ws1"])
    l2 = dict(wq=o["w2"], wsum=o["wsum2"], bias=o["b2"], w_scale=o["ws2"])
    for fn in (K.squeeze_gate, K.squeeze_gate_torch):
        with pytest.raises(ValueError, match="neither"):
            fn(o["codes"], l1, None, K.EmitCodes(o["qs"], o["qz"], q.lo, q.hi, q.form, q.g), l2, None)
