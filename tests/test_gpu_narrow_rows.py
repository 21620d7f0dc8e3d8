"""Narrow fp32 rows (dlmcq_conv2d_i8_nhwc_narrow, conv2d_i8(out_channels=), fuse_inference(narrow_rows=True)) on the GPU.

A layer whose K rows of weights are Kf real channels zero-padded to a multiple of 64 reads its fp32 shortcut and writes its fp32 output
Kf wide while its codes stay K wide.  The reference is the call this one replaces: the existing entry point at K with the shortcut
zero-padded to K columns - `out[:, :Kf]` and the whole code tensor must agree bit for bit (torch.equal; no tolerance anywhere here)."""
import copy

import pytest
import torch
from torch import nn

from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = [(4, 64), (16, 64), (24, 64), (60, 64), (96, 128), (160, 192)]          # (Kf, K)
S_Q = 0.25                                                                       # the consumer's scale (dyadic: ties are exact fp32 values)


def _emit(kind):
    """The consumer's quantiser by the kind of codes it wants: unsigned bytes, signed bytes (with a zero point), unsigned bytes stored
    shifted (DLMCQ_EMIT_SHIFT128)."""
    s = torch.tensor([S_Q], device=DEV)
    if kind == "u8":
        return K.EmitCodes(s, None, 0, 255, N.FORM_ZEROPOINT)
    if kind == "s8":
        return K.EmitCodes(s, torch.tensor([-3.0], device=DEV), -128, 127, N.FORM_ZEROPOINT)
    return K.EmitCodes(s, torch.tensor([5.0], device=DEV), 0, 255, N.FORM_ZEROPOINT, shift128=True)


def _layer(kf, k, c, n, h, w, ksize, asym, x_kind, seed):
    """Operands of a Kf -> K padded layer: rows Kf .. K - 1 of the weights, their sums, bias and offsets are 0, their scale 1 (what
    fuse.py's _padk builds)."""
    g = torch.Generator().manual_seed(seed)
    if x_kind == "s8":
        x, zp = torch.randint(-128, 128, (n, c, h, w), generator=g, dtype=torch.int16).to(torch.int8), torch.tensor([-7.0])
    else:
        x, zp = torch.randint(0, 256, (n, c, h, w), generator=g, dtype=torch.int16).to(torch.uint8), torch.tensor([3.0])
    wq = torch.randint(-4, 5, (k, ksize, ksize, c), generator=g, dtype=torch.int16)
    wq[kf:] = 0
    ws = torch.rand(k, generator=g) * 0.01 + 0.002
    ws[kf:] = 1.0
    bias = torch.randn(k, generator=g)
    bias[kf:] = 0.0
    woff = None
    if asym:
        woff = torch.randn(k, generator=g) * 0.003
        woff[kf:] = 0.0
    d = lambda t: None if t is None else t.to(DEV)      # noqa: E731
    return dict(codes=x.to(DEV).contiguous(memory_format=torch.channels_last), wq=wq.to(torch.int8).to(DEV),
                wsum=wq.sum(dim=(1, 2, 3)).to(torch.int32).to(DEV), bias=d(bias), in_scale=torch.tensor([0.02], device=DEV), in_zp=d(zp),
                w_scale=d(ws)), d(woff)


def _shortcut(plain_out, kf, seed):
    """An fp32 shortcut [N, Kf, P, Q] with negative values (so that ReLU matters) and, on every third element, the value that puts the
    sum on a rounding tie of the consumer's quantiser ((m + 0.5) * S_Q) or next to one."""
    g = torch.Generator().manual_seed(seed)
    base = plain_out[:, :kf].cpu()
    r = torch.randn(base.shape, generator=g) * 8.0
    m = torch.randint(-6, 30, base.shape, generator=g).float()
    tie = (m + 0.5) * S_Q - base                     # fl(base + fl(tie - base)) is the tie itself or its fp32 neighbour
    pick = torch.rand(base.shape, generator=g) < 1 / 3
    r = torch.where(pick, tie, r)
    return r.to(DEV).contiguous(memory_format=torch.channels_last)


def _pad_cols(t, k):
    out = torch.zeros((t.shape[0], k) + tuple(t.shape[2:]), device=t.device).contiguous(memory_format=torch.channels_last)
    out[:, :t.shape[1]] = t
    return out


# (Kf, K), C, (N, H, W), (ksize, stride), shortcut, want_out, emitted codes (None: fp32 only), input codes, activation, asymmetric weights
def _cases():
    geoms, convs = [(1, 5, 5), (2, 9, 7)], [(1, 1), (3, 1), (3, 2)]
    acts, kinds = [N.ACT_NONE, N.ACT_RELU, N.ACT_RELU6], ["u8", "s8", "shift"]
    out = []
    for i, kk in enumerate(WIDTHS):
        # the combination every width gets: shortcut + codes only
        out.append((kk, (64, 192)[i % 2], geoms[(i // 2) % 2], convs[i % 3], True, False, kinds[i % 3], ("u8", "s8")[i % 2], acts[(i + 1) % 3],
                    bool(i % 2)))
        # ... and with the fp32 output beside the codes, the other weights, another activation
        out.append((kk, (192, 64)[i % 2], geoms[(i // 2 + 1) % 2], convs[(i + 1) % 3], True, True, kinds[(i + 1) % 3], ("s8", "u8")[i % 2],
                    acts[i % 3], not bool(i % 2)))
    # no shortcut: fp32 only, codes only, both
    for i, (kk, em, wo) in enumerate([((24, 64), None, True), ((96, 128), "u8", False), ((160, 192), "shift", True), ((16, 64), "s8", False),
                                      ((60, 64), None, True), ((4, 64), "u8", True)]):
        out.append((kk, (64, 192)[i % 2], geoms[i % 2], convs[i % 3], False, wo, em, ("u8", "s8")[i % 2], acts[i % 3], bool(i % 2)))
    return out


CASES = _cases()


def test_the_pruned_grid_keeps_every_value_of_every_axis():
    col = lambda j: {c[j] for c in CASES}      # noqa: E731
    assert col(0) == set(WIDTHS) and col(1) == {64, 192} and col(2) == {(1, 5, 5), (2, 9, 7)} and col(3) == {(1, 1), (3, 1), (3, 2)}
    assert col(4) == {True, False} and col(5) == {True, False} and col(6) == {None, "u8", "s8", "shift"} and col(7) == {"u8", "s8"}
    assert col(8) == {N.ACT_NONE, N.ACT_RELU, N.ACT_RELU6} and col(9) == {True, False}
    for kk in WIDTHS:       # shortcut + emit + want_out=False for every width
        assert any(c[0] == kk and c[4] and not c[5] and c[6] is not None for c in CASES)
    assert not any((not c[5]) and c[6] is None for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c).replace(" ", ""))
def test_narrow_call_equals_the_padded_call(case):
    (kf, k), c, (n, h, w), (ksize, stride), shortcut, want_out, em_kind, x_kind, act, asym = case
    op, woff = _layer(kf, k, c, n, h, w, ksize, asym, x_kind, seed=CASES.index(case))
    kw = dict(stride=stride, padding=ksize // 2, w_offset=woff)
    args = (op["codes"], op["wq"], op["wsum"], op["bias"], op["in_scale"], op["in_zp"], op["w_scale"])
    res = None
    if shortcut:
        res = _shortcut(K.conv2d_i8(*args, **kw), kf, seed=1000 + CASES.index(case))
        assert bool((res < 0).any())
    emit = None if em_kind is None else _emit(em_kind)
    ekw = dict(act=act, emit=emit, want_out=want_out)
    got = K.conv2d_i8(*args, residual=res, out_channels=kf, **ekw, **kw)
    ref = K.conv2d_i8(*args, residual=None if res is None else _pad_cols(res, k), **ekw, **kw)
    got_out, got_codes = got if emit is not None else (got, None)
    ref_out, ref_codes = ref if emit is not None else (ref, None)
    if want_out:
        assert tuple(got_out.shape) == (n, kf) + tuple(ref_out.shape[2:]) and got_out.is_contiguous(memory_format=torch.channels_last)
        assert got_out.permute(0, 2, 3, 1).is_contiguous()          # dense rows of Kf floats
        assert torch.equal(got_out, ref_out[:, :kf])
        assert bool(torch.isfinite(got_out).all())
    else:
        assert got_out is None
    if emit is not None:
        assert got_codes.shape == ref_codes.shape and got_codes.shape[1] == k and got_codes.dtype == ref_codes.dtype
        assert torch.equal(got_codes, ref_codes)
        if shortcut and want_out:       # the construction did put sums on ties of the quantiser: the test saw the rounding cases it is about
            t = got_out / S_Q
            assert int(((t - torch.floor(t)) == 0.5).sum()) > 0


def _raw(op, woff, kf, k, geom, out, residual, codes, emit, act=N.ACT_RELU, flags=0, stride=1, pad=0, ksize=1):
    n, h, w, c = geom
    return N.lib.dlmcq_conv2d_i8_nhwc_narrow(
        N.ptr(op["codes"]), N.ptr(op["wq"]), out, N.ptr(op["bias"]), N.ptr(op["wsum"]), N.ptr(op["in_scale"]), N.ptr(op["in_zp"]),
        N.ptr(op["w_scale"]), N.ptr(woff), n, h, w, c, k, ksize, ksize, stride, pad, 1, int(op["codes"].dtype == torch.uint8), residual, act,
        codes, N.ptr(emit.scale), N.ptr(emit.zero_point), emit.lo, emit.hi, emit.form_arg | flags, emit.g, kf, N.stream_ptr())


SENTINEL = 0x7fc12345          # a quiet NaN's bit pattern no arithmetic here produces


@pytest.mark.parametrize("kf, k", WIDTHS)
def test_nothing_is_written_outside_the_rows(kf, k):
    n, h, w, c = 2, 9, 7, 64
    m = n * h * w
    op, woff = _layer(kf, k, c, n, h, w, 1, True, "u8", seed=kf)
    emit = _emit("u8")
    obuf = torch.full((m * kf + 4096,), SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full((m * k + 4096,), 0xa5, dtype=torch.uint8, device=DEV)
    res = torch.randn(m * kf, device=DEV)
    rc = _raw(op, woff, kf, k, (n, h, w, c), obuf.data_ptr(), res.data_ptr(), cbuf.data_ptr(), emit)
    torch.cuda.synchronize()
    assert rc == 0
    assert bool((obuf[m * kf:] == SENTINEL).all()) and bool((cbuf[m * k:] == 0xa5).all())
    assert not bool((obuf[:m * kf] == SENTINEL).any())
    # and what is inside is what the wrapper gives
    o2, c2 = K.conv2d_i8(op["codes"], op["wq"], op["wsum"], op["bias"], op["in_scale"], op["in_zp"], op["w_scale"], w_offset=woff,
                         residual=res.view(n, h, w, kf).permute(0, 3, 1, 2), relu=True, emit=emit, out_channels=kf)
    assert torch.equal(obuf[:m * kf].view(torch.float32), o2.permute(0, 2, 3, 1).reshape(-1))
    assert torch.equal(cbuf[:m * k], c2.permute(0, 2, 3, 1).reshape(-1))


@pytest.mark.parametrize("k", [64, 128])
@pytest.mark.parametrize("asym", [False, True])
@pytest.mark.parametrize("act", [N.ACT_RELU, N.ACT_RELU6])
def test_kf_equal_k_is_the_existing_entry_point(k, asym, act):
    n, h, w, c = 2, 9, 7, 64
    op, woff = _layer(k, k, c, n, h, w, 3, asym, "u8", seed=k + asym)
    args = (op["codes"], op["wq"], op["wsum"], op["bias"], op["in_scale"], op["in_zp"], op["w_scale"])
    kw = dict(padding=1, w_offset=woff, act=act)
    res = _shortcut(K.conv2d_i8(*args, padding=1, w_offset=woff), k, seed=9)
    for em_kind in ("u8", "shift"):
        emit = _emit(em_kind)
        for want_out in (True, False):
            for force in (False, True):        # (_fused / _asym on whatever kernel the dispatch picks, and on the tiled one)
                ref = K.conv2d_i8(*args, residual=res, emit=emit, want_out=want_out, force_tiled=force, **kw)
                got = K.conv2d_i8(*args, residual=res, emit=emit, want_out=want_out, out_channels=k, **kw)
                assert torch.equal(got[1], ref[1])
                assert (got[0] is None and ref[0] is None) if not want_out else torch.equal(got[0], ref[0])


def test_refusals_launch_nothing_and_route_only_answers_tiled():
    kf, k, (n, h, w, c) = 24, 64, (1, 5, 5, 64)
    m = n * h * w
    op, woff = _layer(kf, k, c, n, h, w, 1, False, "u8", seed=1)
    emit = _emit("u8")
    obuf = torch.full((m * k + 64,), SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full((m * k + 64,), 0xa5, dtype=torch.uint8, device=DEV)
    res = torch.zeros(m * k + 64, device=DEV)
    o, r, cd = obuf.data_ptr(), res.data_ptr(), cbuf.data_ptr()
    geo = (n, h, w, c)
    for bad_kf, bad_k in ((0, 64), (-4, 64), (22, 64), (68, 64), (64, 128), (60, 128), (128, 192), (96, 96)):
        assert _raw(op, woff, bad_kf, bad_k, geo, o, r, cd, emit) == -1, (bad_kf, bad_k)
    assert _raw(op, woff, kf, k, geo, o + 4, r, cd, emit) == -4
    assert _raw(op, woff, kf, k, geo, o, r + 8, cd, emit) == -4
    assert _raw(op, woff, kf, k, geo, o, r, cd + 4, emit) == -4
    for bit in (N.PIPELINED, N.FP32_IN_CHUNK_MAJOR, N.FP32_OUT_CHUNK_MAJOR, N.FP32_IN_CHUNK_MAJOR | N.FP32_OUT_CHUNK_MAJOR):
        assert _raw(op, woff, kf, k, geo, o, r, cd, emit, flags=bit) == -1
        assert _raw(op, woff, kf, k, geo, o, r, cd, emit, flags=bit | N.ROUTE_ONLY) == -1
    for extra in (0, N.FORCE_TILED):
        assert _raw(op, woff, kf, k, geo, o, r, cd, emit, flags=N.ROUTE_ONLY | extra) == N.ROUTE_TILED
        assert _raw(op, woff, kf, k, geo, o, r, cd, emit, flags=N.ROUTE_ONLY | extra, ksize=3, pad=1) == N.ROUTE_TILED     # (3x3: no halo kernel)
    assert _raw(op, woff, k, k, geo, None, None, cd, emit, flags=N.ROUTE_ONLY) == N.ROUTE_TILED      # (codes only 1x1: no pointwise kernel)
    torch.cuda.synchronize()
    assert bool((obuf == SENTINEL).all()) and bool((cbuf == 0xa5).all())
    # DLMCQ_FORCE_TILED is accepted and changes nothing
    assert _raw(op, woff, kf, k, geo, o, r, cd, emit) == 0
    a_out, a_codes = obuf.clone(), cbuf.clone()
    obuf.fill_(SENTINEL)
    cbuf.fill_(0xa5)
    assert _raw(op, woff, kf, k, geo, o, r, cd, emit, flags=N.FORCE_TILED) == 0
    torch.cuda.synchronize()
    assert torch.equal(obuf, a_out) and torch.equal(cbuf, a_codes) and not bool((obuf[:m * kf] == SENTINEL).any())


def test_wrapper_refuses_what_has_no_narrow_form():
    kf, k = 24, 64
    op, woff = _layer(kf, k, 64, 1, 5, 5, 3, False, "u8", seed=2)
    args = (op["codes"], op["wq"], op["wsum"], op["bias"], op["in_scale"], op["in_zp"], op["w_scale"])
    ok = dict(padding=1, out_channels=kf)
    res = torch.zeros(1, kf, 5, 5, device=DEV).contiguous(memory_format=torch.channels_last)
    for bad in (dict(observe=True), dict(pipelined=True), dict(out_chunk_major=True),
                dict(in_offset=torch.zeros(1, device=DEV), tap_sums=torch.zeros(9, k, device=DEV)),
                dict(residual=K.ChunkMajor(torch.zeros(1, 25, 64, device=DEV), (1, 64, 5, 5)))):
        with pytest.raises(ValueError):
            K.conv2d_i8(*args, **ok, **bad)
    with pytest.raises(ValueError):          # the shortcut has the fp32 output's shape: Kf wide, not K
        K.conv2d_i8(*args, residual=_pad_cols(res, k), **ok)
    assert tuple(K.conv2d_i8(*args, residual=res, **ok).shape) == (1, kf, 5, 5)


# ------------------------------------------------------------------------------------------------- the plan
FSPTQ_W8A8 = {"weight": {"enable": True, "type": "minmax_channel", "args": {"n_bits": 8, "signed": True}},
              "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
              "exclude_layers": [], "override_options": []}
QBASE_W4A8 = {"weight": {"enable": True, "type": "minmax_channel", "args": {"n_bits": 4, "signed": False}},
              "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
              "exclude_layers": [], "override_options": []}
QBASE_W8A8 = {"weight": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": True}},
              "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
              "exclude_layers": [], "override_options": []}


def _net(name, cfg, qtype, normalised, seed):
    import workloads as W
    from dlmc.utils.merge_bn import merge_bn
    from dlmc.utils.quantize import quantize_model
    torch.manual_seed(seed)
    net = getattr(W, name)().to(DEV).eval()
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    net = merge_bn(net, inplace=True)
    if qtype:
        quantize_model(net, copy.deepcopy(cfg), None, qtype, int8_gemm=True)
    else:
        quantize_model(net, copy.deepcopy(cfg), None)
    if normalised:
        mean = torch.tensor([0.485, 0.456, 0.406], device=DEV)[:, None, None]
        std = torch.tensor([0.229, 0.224, 0.225], device=DEV)[:, None, None]
        x = (torch.rand(3, 3, 32, 32, device=DEV) - mean) / std
    else:
        x = torch.relu(torch.randn(3, 3, 32, 32, device=DEV))
    with torch.no_grad():
        net(x)                                   # calibrate
    return net, x


def _fp32_reading_nodes(plan, x):
    """The plan's convolution nodes (first-layer nodes included) that were handed an fp32 activation in a forward of `x`."""
    from dlmc.utils import fuse as FU
    seen, hooks = [], []
    for name, m in plan.named_modules():
        if isinstance(m, FU._PlanLayer) and m.layer.weight.dim() == 4:
            hooks.append(m.register_forward_pre_hook(lambda mod, a, name=name: seen.append(name) if a[0].dtype == torch.float32 else None))
    with torch.no_grad():
        plan(x)
    for h in hooks:
        h.remove()
    return seen


def _narrow_nodes(plan):
    from dlmc.utils import fuse as FU
    return [m for m in plan.modules() if isinstance(m, FU.Int8Layer) and m.narrow]


def _both(net, x, **kw):
    from dlmc.utils.fuse import fuse_inference
    off, on = fuse_inference(net, **kw), fuse_inference(net, narrow_rows=True, **kw)
    with torch.no_grad():
        a, b = off(x), on(x)
        again = on(x)
    print(off.fusion_report, on.fusion_report, sep="\n")
    assert bool(torch.isfinite(a).all())
    assert torch.equal(b, again)
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} logits differ, max {float((a - b).abs().max())}"
    return off, on


def test_mobilenet_v2_fsptq_plan_flag_on_equals_flag_off():
    net, x = _net("mobilenet_v2", FSPTQ_W8A8, "FSPTQ", False, 31)
    off, on = _both(net, x)
    ro, rn = off.fusion_report, on.fusion_report
    assert (ro.residual, ro.narrow) == (3, 0)
    assert rn.residual == 10 and rn.narrow > 0 and rn.narrow == len(_narrow_nodes(on))
    assert (rn.layers, rn.skipped, rn.relu6) == (ro.layers, ro.skipped, ro.relu6)
    for m in _narrow_nodes(on):
        assert m.k_pad != m.k and m.k % 4 == 0


def test_mobilenet_v2_qbase_offset_plan_flag_on_equals_flag_off():
    net, x = _net("mobilenet_v2", QBASE_W4A8, None, True, 32)
    off, on = _both(net, x, act_offsets=True)
    ro, rn = off.fusion_report, on.fusion_report
    assert (ro.layers, ro.residual, ro.narrow, ro.skipped) == (53, 3, 0, [])
    assert (rn.layers, rn.residual, rn.skipped) == (53, 10, []) and rn.narrow > 0
    assert any(m.w_off is not None for m in _narrow_nodes(on))         # the asymmetric instantiations ran
    assert len(_fp32_reading_nodes(off, x)) == 8                          # the image and the seven sums whose adds stay outside
    assert _fp32_reading_nodes(on, x) == ["_int8_plan_0"]                 # no layer reads fp32 but the first


def test_cifar_resnet20_qbase_plan_flag_on_equals_flag_off():
    net, x = _net("cifar_resnet20", QBASE_W8A8, None, False, 33)
    off, on = _both(net, x)
    ro, rn = off.fusion_report, on.fusion_report
    assert (ro.residual, ro.dual, ro.narrow) == (3, 1, 0)
    assert (rn.residual, rn.dual, rn.narrow) == (9, 1, 7) and rn.relu == ro.relu + 6
    assert all(m.w_off is None for m in _narrow_nodes(on))             # the symmetric instantiations
