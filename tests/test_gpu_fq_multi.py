"""One-launch fake-quant of many tensors (csrc/fake_quant_multi.hip) against the one-tensor launches, BYTE FOR BYTE: both run
the same per-workgroup bodies, so there is no tolerance anywhere in this file.  Shapes are the smallest that cross each
boundary of the kernels: the 0-3 element tail, the 256-element forward chunk, the 1024-element backward chunk, rows shorter
and longer than a chunk, float4s that straddle rows, the scalar and the float4 row walk."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TENSOR_N = (0, 1, 3, 4, 255, 256, 257, 1023, 1024, 1025, 4099)
CHANNEL_SHAPES = ((1, 5), (8, 9), (3, 147), (16, 64), (64, 4), (5, 1030))
SENTINEL = 0x7FC0DEAD      # a NaN payload no kernel here produces
GAP = 16                   # 64 bytes of fp32


@pytest.fixture(scope="module")
def K():
    assert torch.cuda.is_available(), "the gpu suite needs a GPU"
    from dlmc.quantization.scalar import kernels
    return kernels


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def same_bits(got, want, what):
    assert got.shape == want.shape, f"{what}: {tuple(got.shape)} vs {tuple(want.shape)}"
    assert torch.equal(bits(got), bits(want)), what


def adversarial(scale, offset, lo, hi):
    """Exact rounding ties and clamp edges of the quantiser, one ulp either side of each, both zeros, NaN, both infinities
    and denormals."""
    k = torch.arange(lo - 2, hi + 2, dtype=torch.float32)
    ties = torch.cat([(k + 0.5) * scale + offset, k * scale + offset])
    inf = torch.tensor(float("inf"))
    around = torch.cat([ties, torch.nextafter(ties, inf), torch.nextafter(ties, -inf)])
    special = torch.tensor([0.0, -0.0, float("nan"), float("inf"), float("-inf"), 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 3e-39])
    return torch.cat([special, around])


@pytest.fixture(scope="module")
def case(K):
    """Segments (mixed forms, 4-bit and 8-bit ranges), their gy, and the one-tensor reference of each - computed once."""
    from dlmc import _native as N
    g = torch.Generator().manual_seed(2333)
    shapes = [(n,) for n in TENSOR_N] + list(CHANNEL_SHAPES)
    forms = (N.FORM_QBASE, N.FORM_ZEROPOINT, N.FORM_SYMMETRIC)
    segs, gys = [], []
    for i, shape in enumerate(shapes):
        form = forms[i % 3]
        lo, hi = ((-8, 7), (-127, 127), (0, 15), (0, 255))[i % 4]
        per_channel = len(shape) == 2
        ch = shape[0] if per_channel else 1
        sshape = (ch, 1) if per_channel else (1,)
        scale = torch.rand(sshape, generator=g) * 0.05 + 0.01
        scale.view(-1)[0] = 2.0 ** -4                         # a dyadic scale: exact ties exist
        if form == N.FORM_QBASE:
            offset = torch.randn(sshape, generator=g) * 0.05 + 0.0137
        elif form == N.FORM_ZEROPOINT:
            offset = torch.randint(lo + 1, hi, sshape, generator=g).float()      # an in-range zero point
        else:
            offset = None
        x = torch.randn(shape, generator=g) * 0.4
        if i in (8, 9, 10, 16):                               # 1024, 1025 and 4099 per tensor (one of each form), (5, 1030) per channel
            o0 = 0.0 if offset is None or form == N.FORM_ZEROPOINT else float(offset.view(-1)[0])
            adv = adversarial(float(scale.view(-1)[0]), o0, lo, hi)
            x.view(-1)[:adv.numel()] = adv[:x.numel()]
        gy = torch.randn(shape, generator=g)
        flat = gy.view(-1)
        flat[::13] = 0.0
        flat[5::97] = float("inf")
        flat[6::101] = float("-inf")
        ste_g = 1 / math.sqrt(max(x.numel(), 1) * hi) if form == N.FORM_QBASE else 0.0
        segs.append(K.Segment(x.to(DEV), scale.to(DEV), None if offset is None else offset.to(DEV), lo, hi, form, ste_g))
        gys.append(gy.to(DEV))
    ref = []
    for s, gy in zip(segs, gys):
        y = K.fake_quant(s.x, s.scale, s.offset, s.lo, s.hi, s.form, g=s.g)
        gx, gs = K.fake_quant_backward(s.x, gy, s.scale, s.offset, s.lo, s.hi, s.g, form=s.form)
        ref.append((y, gx, gs))
    torch.cuda.synchronize()
    return segs, gys, ref


def check(K, segs, gys, ref, what):
    ys = K.fake_quant_multi(segs)
    gxs, gss = K.fake_quant_multi_backward(segs, gys)
    for i, (s, (y, gx, gs)) in enumerate(zip(segs, ref)):
        tag = f"{what} segment {i} {tuple(s.x.shape)} form {s.form}"
        same_bits(ys[i], y, tag + " y")
        same_bits(gxs[i], gx, tag + " gx")
        same_bits(gss[i], gs, tag + " gscale")


def test_segments_equal_one_tensor_launches(K, case):
    segs, gys, ref = case
    assert any(bool(torch.isnan(r[0]).any()) for r in ref) and any(r[0].numel() == 0 for r in ref)
    check(K, segs, gys, ref, "in order")


def test_segment_order_does_not_matter(K, case):
    segs, gys, ref = case
    check(K, segs[::-1], gys[::-1], ref[::-1], "reversed")
    r = 7
    check(K, segs[r:] + segs[:r], gys[r:] + gys[:r], ref[r:] + ref[:r], "rotated")


def _arena(sizes, pad):
    """An int32 arena filled with SENTINEL, one view per size with GAP words between neighbours (and at both ends); each view
    starts on a multiple of `pad` words."""
    offs, total = [], GAP
    for n in sizes:
        total = (total + pad - 1) // pad * pad
        offs.append(total)
        total += n + GAP
    arena = torch.full((total + pad,), SENTINEL, dtype=torch.int32, device=DEV)
    keep = torch.ones(total + pad, dtype=torch.bool, device=DEV)
    for o, n in zip(offs, sizes):
        keep[o:o + n] = False
    return arena, keep, [arena[o:o + n].view(torch.float32) for o, n in zip(offs, sizes)]


def test_nothing_is_written_outside_a_segment(K, case):
    segs, gys, ref = case
    n = len(segs)
    ya, ykeep, ys = _arena([s.x.numel() for s in segs], 4)
    K.fake_quant_multi(segs, out=[y.view(s.x.shape) for y, s in zip(ys, segs)])
    assert bool((ya[ykeep] == SENTINEL).all()), "the forward wrote between two outputs"
    for i, (y, r) in enumerate(zip(ys, ref)):
        same_bits(y.view(r[0].shape), r[0], f"segment {i} y in the arena")
    # backward: segment 4 without gx, segment 7 without gscale, segment 12 with neither, segment 14 without gy
    want_gx = [i not in (4, 12) for i in range(n)]
    want_gs = [i not in (7, 12) for i in range(n)]
    gys = [None if i == 14 else g for i, g in enumerate(gys)]
    ga, gkeep, gxs = _arena([s.x.numel() for s in segs], 4)
    sa, skeep, gss = _arena([s.channels for s in segs], 1)
    total = sum(max(1, -(-(s.x.numel() // 4) // 256)) if s.channels == 1 else s.channels
                for i, s in enumerate(segs) if s.x.numel() and gys[i] is not None and (want_gx[i] or want_gs[i]))
    pa, pkeep, (part,) = _arena([total], 1)
    got_gx, got_gs = K.fake_quant_multi_backward(segs, gys, want_gx, want_gs, gx_out=[t.view(s.x.shape) for t, s in zip(gxs, segs)],
                                                 gscale_out=gss, scratch=part)
    for arena, keep, what in ((ga, gkeep, "gx"), (sa, skeep, "gscale"), (pa, pkeep, "partials")):
        assert bool((arena[keep] == SENTINEL).all()), f"the backward wrote outside a segment's {what}"
    for i, r in enumerate(ref):
        untouched_gx = not want_gx[i] or gys[i] is None
        untouched_gs = not want_gs[i] or gys[i] is None
        if untouched_gx:
            assert got_gx[i] is None and bool((gxs[i].view(torch.int32) == SENTINEL).all()), f"segment {i}: gx was not wanted"
        else:
            same_bits(gxs[i].view(r[1].shape), r[1], f"segment {i} gx in the arena")
        if untouched_gs:
            assert got_gs[i] is None and bool((gss[i].view(torch.int32) == SENTINEL).all()), f"segment {i}: gscale was not wanted"
        else:
            same_bits(gss[i], r[2], f"segment {i} gscale in the arena")


def test_autograd_function_equals_per_layer_functions(K, case):
    from dlmc.quantization.scalar._wrapper import FakeQuantFn, MultiFakeQuantFn
    segs, _, _ = case
    pick = [3, 8, 10, 12, 13, 15, 16]
    segs = [segs[i] for i in pick]
    left_out = 2
    g = torch.Generator().manual_seed(7)
    rs = [torch.randn(s.x.shape, generator=g).to(DEV) for s in segs]

    def leaves():
        ws = [s.x.clone().requires_grad_(True) for s in segs]
        ss = [s.scale.clone().requires_grad_(i != 4) for i, s in enumerate(segs)]     # one scale is frozen
        ws[5].requires_grad_(False)                                                    # and one weight
        return ws, ss
    ws, ss = leaves()
    plan = K.FqMultiPlan([K.Segment(w, s, seg.offset, seg.lo, seg.hi, seg.form, seg.g) for w, s, seg in zip(ws, ss, segs)])
    ys = MultiFakeQuantFn.apply(plan, *ws, *ss)
    sum((y * r).sum() for i, (y, r) in enumerate(zip(ys, rs)) if i != left_out).backward()
    ws2, ss2 = leaves()
    zero = torch.zeros((), device=DEV)
    for i, (w, s, seg, r) in enumerate(zip(ws2, ss2, segs, rs)):
        y = FakeQuantFn.apply(w, s, zero if seg.offset is None else seg.offset, seg.lo, seg.hi, seg.form, seg.g)
        same_bits(ys[i], y, f"tensor {i} y")
        if i != left_out:
            (y * r).sum().backward()
    for i in range(len(segs)):
        for got, want, what in ((ws[i], ws2[i], "weight"), (ss[i], ss2[i], "scale")):
            if not got.requires_grad:
                assert got.grad is None, f"tensor {i}: a frozen {what} got a gradient"
            elif i == left_out:
                assert got.grad is not None and not bool(got.grad.view(torch.int32).any()), f"tensor {i}: left out of the loss, {what}.grad is not +0"
            else:
                same_bits(got.grad, want.grad, f"tensor {i} {what}.grad")


# ------------------------------------------------------------------------------------- wrappers under the handle
class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.c1 = torch.nn.Conv2d(3, 8, 3, padding=1)
        self.dw = torch.nn.Conv2d(8, 8, 3, padding=1, groups=8)
        self.pw = torch.nn.Conv2d(8, 16, 1)
        self.c2 = torch.nn.Conv2d(16, 16, 3, padding=1)
        self.fc = torch.nn.Linear(16, 10)

    def forward(self, x):
        x = torch.relu(self.c1(x))
        x = torch.relu(self.dw(x))
        x = torch.relu(self.pw(x))
        x = torch.relu(self.c2(x))
        return self.fc(x.mean((2, 3)))


def _model(family, wtype):
    from dlmc.utils.quantize import quantize_model
    torch.manual_seed(2333)
    net = _Net().to(DEV).train()
    cfg = {"weight": {"enable": True, "type": wtype, "args": {"n_bits": 4, "signed": True}},
           "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 4, "signed": False}},
           "momentum": 0.1, "exclude_layers": [], "override_options": []}
    if "channel" in wtype and family is None:
        cfg["weight"]["args"]["ch_axis"] = 0
    quantize_model(net, cfg, None, family)
    x = torch.rand(2, 3, 12, 12, generator=torch.Generator().manual_seed(5)).to(DEV)
    with torch.no_grad():
        net(x)                      # the calibrating forward
    return net, x


def _profiled(K, fn):
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        fn()
        torch.cuda.synchronize()
        return [(r[0], r[1]) for r in K.PROFILE.records]
    finally:
        K.PROFILE.enabled = False
        K.PROFILE.reset()


@pytest.mark.parametrize("family,wtype", [(None, "minmax_tensor"), (None, "minmax_channel"), ("FSPTQ", "minmax_channel")],
                         ids=["qbase-tensor", "qbase-channel", "fsptq-channel"])
def test_wrappers_under_the_handle(K, family, wtype):
    from dlmc import _native as N
    from dlmc.utils.quantize import WeightQuantBatch
    net, x = _model(family, wtype)
    layers = [net.c1, net.dw, net.pw, net.c2, net.fc]
    wqb = WeightQuantBatch(net)
    assert wqb.members == layers and not wqb.skipped
    if "channel" in wtype:
        assert all(m.wt_scale.numel() == m.weight.shape[0] for m in layers)
    # forward: the same logits with and without the handle, with autograd and without
    want = net(x)
    with wqb.step():
        got = net(x)
        assert set(wqb.outputs) == set(layers)
    assert not wqb.outputs
    assert torch.equal(got, want) and got.requires_grad
    with torch.no_grad():
        want_ng = net(x)
        with wqb.step():
            got_ng = net(x)
    assert torch.equal(got_ng, want_ng) and torch.equal(got_ng, want.detach())
    # backward: record each gy inside the batched run, then every gradient against the one-tensor backward of that gy
    gy = {}
    net.zero_grad(set_to_none=True)

    def run():
        with wqb.step():
            for m in layers:
                wqb.outputs[m].register_hook(lambda g, m=m: gy.__setitem__(m, g.clone()))
            out = net(x)
        (out * torch.arange(10, device=DEV)).sum().backward()
    records = _profiled(K, run)
    form = N.FORM_SYMMETRIC if family == "FSPTQ" else N.FORM_QBASE
    for m in layers:
        g_w = 1 / math.sqrt(m.weight.numel() * m.wt_max_val) if family is None else 0.0
        offset = m.wt_offset if family is None else None
        gx, gs = K.fake_quant_backward(m.weight.detach(), gy[m], m.wt_scale.detach(), offset, m.wt_min_val, m.wt_max_val, g_w, form=form)
        same_bits(m.weight.grad, gx, "weight.grad")
        same_bits(m.wt_scale.grad, gs.reshape(m.wt_scale.shape), "wt_scale.grad")
    # launches: one fq_multi, one fq_multi_bwd, and of the one-tensor kernels only the five activation quantisers' (forward
    # and backward) - told from a weight's by their algorithmic bytes
    tags = [t for t, _ in records]
    assert tags.count("fq_multi") == 1 and tags.count("fq_multi_bwd") == 1
    n_w = sum(m.weight.numel() for m in layers)
    assert dict(records)["fq_multi"] == 8 * n_w and dict(records)["fq_multi_bwd"] == 12 * n_w
    acts = sorted(8 * n for n in (2 * 3 * 144, 2 * 8 * 144, 2 * 8 * 144, 2 * 16 * 144, 2 * 16))
    assert sorted(b for t, b in records if t in ("fq_tensor", "fq_channel")) == acts
    # (the first layer's input needs no gradient, but its scale does: 8 bytes per element there, 12 elsewhere)
    assert sorted(b for t, b in records if t == "fq_bwd") == sorted([8 * 2 * 3 * 144] + [12 * n for n in (2 * 8 * 144, 2 * 8 * 144, 2 * 16 * 144, 2 * 16)])
    # a weight written to inside the step sends that layer - and only it - to its own launch; the result is the unbatched one
    def touched():
        with torch.no_grad(), wqb.step():
            net.pw.weight.mul_(1.25)
            return net(x)
    got_t = None

    def run_t():
        nonlocal got_t
        got_t = touched()
    records = _profiled(K, run_t)
    with torch.no_grad():
        assert torch.equal(got_t, net(x)) and not torch.equal(got_t, want_ng)
    assert sorted(b for t, b in records if t in ("fq_tensor", "fq_channel")) == sorted(acts + [8 * net.pw.weight.numel()])


def test_rootq_model_is_left_alone(K):
    from dlmc.utils.quantize import WeightQuantBatch
    net, x = _model("RootQ", "minmax_tensor")
    net.eval()                      # (in train mode RootQ's running bounds move with every forward: two runs would differ anyway)
    wqb = WeightQuantBatch(net)
    assert not wqb.members and set(wqb.skipped) == {"c1", "dw", "pw", "c2", "fc"}
    want = net(x)
    got = None

    def run():
        nonlocal got
        with wqb.step():
            got = net(x)
    records = _profiled(K, run)
    assert torch.equal(got, want)
    assert not [t for t, _ in records if t.startswith("fq_multi")]
