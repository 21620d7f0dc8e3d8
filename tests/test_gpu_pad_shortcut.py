"""Option-A shortcuts read in place by the int8 epilogue (dlmcq_conv2d_i8_nhwc_padres, conv2d_i8(residual=PadShortcut(...)),
fuse_inference(pad_shortcuts=True)) on the GPU.

The shortcut `pad(src[:, ::s, ::s, :])` is never built: the kernel reads `src` at a pixel stride and a channel offset and adds +0 in the
zero columns.  The references are code that exists without the feature, fed the materialised tensor: dlmcq_conv2d_i8_nhwc_narrow with
`residual = pad(src[:, ::s, ::s, :])`, and the unfused sequence narrow call (no shortcut, no activation) -> torch `+=` -> torch ReLU ->
dlmcq_fake_quant_f32.  IEEE addition of the same two fp32 numbers, the same quantiser on the same stored value: everything is compared
with torch.equal, no tolerance anywhere.

The plan is compared with the plan without the flag.  It is NOT compared with the wrappers' own forward: test_gpu_narrow_rows.py states
no conditions for that comparison, and for the CIFAR widths (16 / 32 channels) test_gpu_fuse.py explains why there are none - the
wrappers run such layers as fp32 convolutions, the plan pads them onto the int8 kernel (another accumulation order)."""
import copy

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from test_gpu_narrow_rows import FSPTQ_W8A8, QBASE_W8A8, SENTINEL, _emit, _layer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NEG0 = -0x80000000          # the bit pattern of -0.0f as an int32


class Case:
    """One problem: `ksize` x `ksize` / stride 1 convolution C -> K (Kf real) over [n, p, q] pixels, its shortcut subsampled at `s` from
    an [n, hs, ws, cs] source, `lo` zero channels in front."""

    def __init__(self, n, hs, ws, s, c, k, kf, cs, lo, ksize=1, asym=False, x_kind="u8", seed=0):
        self.n, self.hs, self.ws, self.s, self.c, self.k, self.kf, self.cs, self.lo, self.ksize, self.asym = n, hs, ws, s, c, k, kf, cs, lo, ksize, asym
        self.p, self.q = -(-hs // s), -(-ws // s)
        self.m = n * self.p * self.q
        op, woff = _layer(kf, k, c, n, self.p, self.q, ksize, asym, x_kind, seed)
        # planted -0: channels with zero weights, a NEGATIVE weight scale and bias -0.0 give fma(+0, s_in * s_w, -0) = -0 before the shortcut
        # (asymmetric weights: the offset term is (row sum > 0) * -0 = -0 as well) - one in the zero columns, one in the source's range
        zero_cols = [col for col in range(0, kf, 4) if not (lo <= col < lo + cs)]
        self.planted = ([zero_cols[0] + 1, zero_cols[-1] + 2] if zero_cols else []) + [lo + 1, lo + cs - 2]
        for col in self.planted:
            op["wq"][col] = 0
            op["wsum"][col] = 0
            op["w_scale"][col] = -0.004
            op["bias"][col] = -0.0
            if woff is not None:
                woff[col] = -0.0
        self.op, self.woff = op, woff
        g = torch.Generator().manual_seed(seed + 77)
        src = torch.randn(n, hs, ws, cs, generator=g) * 3.0
        src[..., 1] = 0.0                     # +0 under the planted -0 of column lo + 1 ...
        src[..., cs - 2] = 0.0                # ... and of column lo + cs - 2
        self.src_values = src.to(DEV)

    def source(self, holes):
        """The source in the middle of a larger NaN-filled buffer (16-byte aligned); `holes`: NaN at every pixel the subsample skips."""
        pre, numel = 1024 + 4 * (self.cs % 7), self.n * self.hs * self.ws * self.cs
        buf = torch.full((pre + numel + 4096,), float("nan"), device=DEV)
        v = self.src_values.clone()
        if holes:
            keep = torch.zeros(self.hs, self.ws, dtype=torch.bool, device=DEV)
            keep[::self.s, ::self.s] = True
            v[:, ~keep] = float("nan")
        buf[pre:pre + numel] = v.reshape(-1)
        view = buf[pre:pre + numel]
        assert view.data_ptr() % 16 == 0
        return buf, view

    def materialised(self):
        """pad(src[:, ::s, ::s, :]) as torch builds it: flat [m, kf]."""
        sub = self.src_values[:, ::self.s, ::self.s, :]
        return F.pad(sub, (self.lo, self.kf - self.lo - self.cs)).contiguous().reshape(-1)

    def head(self, out):
        op = self.op
        return (N.ptr(op["codes"]), N.ptr(op["wq"]), out, N.ptr(op["bias"]), N.ptr(op["wsum"]), N.ptr(op["in_scale"]), N.ptr(op["in_zp"]),
                N.ptr(op["w_scale"]), N.ptr(self.woff), self.n, self.p, self.q, self.c, self.k, self.ksize, self.ksize, 1, self.ksize // 2, 1,
                int(op["codes"].dtype == torch.uint8))

    def tail(self, act, codes, emit, flags=0, kf=None):
        return (act, codes, N.ptr(emit.scale), N.ptr(emit.zero_point), emit.lo, emit.hi, emit.form_arg | flags, emit.g,
                self.kf if kf is None else kf, N.stream_ptr())

    def padres(self, out, src, codes, emit, act=N.ACT_RELU, flags=0, **bad):
        a = dict(h=self.hs, w=self.ws, c=self.cs, s=self.s, lo=self.lo, kf=None)
        a.update(bad)
        return N.lib.dlmcq_conv2d_i8_nhwc_padres(*self.head(out), src, a["h"], a["w"], a["c"], a["s"], a["lo"],
                                                 *self.tail(act, codes, emit, flags, a["kf"]))

    def narrow(self, out, residual, codes, emit, act=N.ACT_RELU):
        return N.lib.dlmcq_conv2d_i8_nhwc_narrow(*self.head(out), residual, *self.tail(act, codes, emit))


def _buffers(case):
    obuf = torch.full((case.m * case.kf + 4096,), SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full((case.m * case.k + 4096,), 0xa5, dtype=torch.uint8, device=DEV)
    return obuf, cbuf


def _run_padres(case, emit, act, want_out, want_codes, holes):
    obuf, cbuf = _buffers(case)
    sbuf, src = case.source(holes)
    before = sbuf.view(torch.int32).clone()
    rc = case.padres(obuf.data_ptr() if want_out else None, src.data_ptr(), cbuf.data_ptr() if want_codes else None, emit, act)
    torch.cuda.synchronize()
    assert rc == 0
    assert torch.equal(sbuf.view(torch.int32), before)                                    # the source is read, never written
    assert bool((obuf[case.m * case.kf:] == SENTINEL).all()) and bool((cbuf[case.m * case.k:] == 0xa5).all())
    if not want_out:
        assert bool((obuf == SENTINEL).all())
    if not want_codes:
        assert bool((cbuf == 0xa5).all())
    return obuf[:case.m * case.kf], cbuf[:case.m * case.k]


def _check(case, em_kind="u8", act=N.ACT_RELU, want_out=True, want_codes=True):
    emit = _emit(em_kind)
    got_out, got_codes = _run_padres(case, emit, act, want_out, want_codes, holes=False)
    # ---- every case runs twice (the bits repeat), and a second time on a source whose skipped pixels are NaN
    for holes in (False, True):
        o2, c2 = _run_padres(case, emit, act, want_out, want_codes, holes)
        assert torch.equal(o2, got_out) and torch.equal(c2, got_codes), f"holes={holes}"
    # ---- reference 1: the narrow entry point on the materialised shortcut
    mat = case.materialised()
    obuf, cbuf = _buffers(case)
    assert case.narrow(obuf.data_ptr(), mat.data_ptr(), cbuf.data_ptr(), emit, act) == 0
    torch.cuda.synchronize()
    ref_out, ref_codes = obuf[:case.m * case.kf], cbuf[:case.m * case.k]
    if want_out:
        assert not bool(torch.isnan(got_out.view(torch.float32)).any()), "a read outside the source (NaN) reached the output"
        assert torch.equal(got_out, ref_out)             # int32 views: bit patterns, the sign of a zero included
    if want_codes:
        assert torch.equal(got_codes, ref_codes)
    # ---- reference 2: narrow call without shortcut and activation -> torch += -> torch ReLU -> dlmcq_fake_quant_f32
    pbuf, _ = _buffers(case)
    assert case.narrow(pbuf.data_ptr(), None, None, emit, N.ACT_NONE) == 0
    torch.cuda.synchronize()
    plain = pbuf[:case.m * case.kf].view(case.m, case.kf)
    for col in case.planted:                                # the construction did plant -0 in front of the shortcut
        assert bool((plain[:, col] == NEG0).all()), col
    t = plain.view(torch.float32).clone()
    t += mat.view(case.m, case.kf)
    if act == N.ACT_RELU:
        t = torch.relu(t)
    elif act == N.ACT_RELU6:
        t = F.relu6(t)
    if want_out:
        assert torch.equal(got_out.view(torch.float32).view(case.m, case.kf), t)
        for col in case.planted:                            # -0 + +0 = +0, by bit pattern
            assert bool((got_out.view(case.m, case.kf)[:, col] == 0).all()), col
    if want_codes:
        full = torch.zeros(case.m, case.k, device=DEV)      # columns Kf .. K - 1: zero weights, bias and offsets - the consumer's code of 0
        full[:, :case.kf] = t
        z = emit.zero_point
        want = K.fake_quant(full, emit.scale, z, emit.lo, emit.hi, emit.form, codes="i8", want_y=False)[1].view(torch.uint8).reshape(-1)
        if emit.shift128:
            want = want ^ 0x80
        assert torch.equal(got_codes, want)


# the smallest shapes that cross each boundary (csrc/conv_i8.hip: 128-row x 64-column tiles, four waves of 32 rows, quads of 4 columns)
SHAPES = {
    "odd_source_one_partial_tile": dict(n=3, hs=9, ws=9, s=2, c=64, k=64, kf=32, cs=16, lo=8),           # 75 rows: image seams inside a tile
    "even_source_ceil": dict(n=3, hs=10, ws=10, s=2, c=64, k=64, kf=32, cs=16, lo=8),
    "mixed_extents": dict(n=3, hs=10, ws=9, s=2, c=64, k=64, kf=32, cs=16, lo=8),
    "two_tiles_kf_equals_k": dict(n=5, hs=13, ws=13, s=2, c=64, k=64, kf=64, cs=32, lo=16),           # 245 rows: an image straddles the tile seam
    "pad_only_two_column_tiles": dict(n=2, hs=6, ws=6, s=1, c=128, k=128, kf=128, cs=64, lo=32),      # the source spans the column-tile seam
    "unequal_pads": dict(n=3, hs=9, ws=9, s=2, c=64, k=64, kf=32, cs=16, lo=4),
    "no_high_pad": dict(n=3, hs=9, ws=9, s=2, c=64, k=64, kf=32, cs=16, lo=16),
    "no_pad_at_all": dict(n=3, hs=9, ws=9, s=2, c=64, k=64, kf=32, cs=32, lo=0),
    "single_quad_in_the_last_columns": dict(n=3, hs=9, ws=9, s=2, c=64, k=64, kf=32, cs=4, lo=28),
    "stride_3_3x3": dict(n=2, hs=10, ws=8, s=3, c=64, k=64, kf=32, cs=16, lo=8, ksize=3),
    "padded_second_column_tile": dict(n=2, hs=9, ws=9, s=2, c=64, k=128, kf=96, cs=48, lo=24, ksize=3),
}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_padres_equals_the_narrow_call_on_the_materialised_shortcut(name):
    kw = SHAPES[name]
    _check(Case(**kw, seed=len(name)))


# the first shape with the epilogue's options: fp32 / codes / both, the three activations, asymmetric weights, the consumer's quantiser
OPTIONS = [  # (emit kind, activation, want_out, want_codes, asymmetric weights, input codes)
    ("u8", N.ACT_RELU, True, False, False, "u8"), ("u8", N.ACT_RELU, False, True, False, "u8"), ("u8", N.ACT_NONE, True, True, False, "s8"),
    ("u8", N.ACT_RELU6, True, True, False, "u8"), ("s8", N.ACT_RELU, True, True, False, "u8"), ("shift", N.ACT_RELU, True, True, False, "s8"),
    ("u8", N.ACT_RELU, True, True, True, "u8"), ("s8", N.ACT_NONE, True, True, True, "u8"), ("shift", N.ACT_RELU6, True, True, True, "u8"),
    ("u8", N.ACT_RELU6, False, True, True, "u8"), ("s8", N.ACT_RELU6, True, False, False, "s8"), ("shift", N.ACT_NONE, False, True, False, "u8"),
]


@pytest.mark.parametrize("opt", OPTIONS, ids=lambda o: "-".join(str(v) for v in o))
def test_epilogue_options(opt):
    em_kind, act, want_out, want_codes, asym, x_kind = opt
    case = Case(**SHAPES["odd_source_one_partial_tile"], ksize=3, asym=asym, x_kind=x_kind, seed=OPTIONS.index(opt))
    _check(case, em_kind, act, want_out, want_codes)


def test_the_option_grid_reaches_all_four_instantiations():
    assert {(o[4], o[1] == N.ACT_RELU6) for o in OPTIONS} == {(False, False), (False, True), (True, False), (True, True)}
    assert {o[0] for o in OPTIONS} == {"u8", "s8", "shift"} and {(o[2], o[3]) for o in OPTIONS} == {(True, True), (True, False), (False, True)}


def test_refusals_launch_nothing_and_route_only_answers_tiled():
    case = Case(**SHAPES["odd_source_one_partial_tile"], seed=3)
    emit = _emit("u8")
    obuf, cbuf = _buffers(case)
    sbuf, src = case.source(False)
    o, s_, cd = obuf.data_ptr(), src.data_ptr(), cbuf.data_ptr()
    bads = [dict(kf=30), dict(kf=0), dict(kf=68),                     # what _narrow refuses
            dict(s=0), dict(s=-2),                                    # res_stride < 1
            dict(h=11), dict(h=8), dict(w=11), dict(w=8), dict(s=1), dict(s=3),     # P / Q != ceil(res_h / res_stride), ceil(res_w / res_stride)
            dict(c=0), dict(c=2, lo=0), dict(c=6), dict(c=18),        # res_c < 4, res_c % 4 != 0
            dict(lo=6), dict(lo=-4),                                  # res_clo % 4 != 0, res_clo < 0
            dict(lo=20), dict(c=36, lo=0)]                            # res_clo + res_c > Kf
    for bad in bads:
        assert case.padres(o, s_, cd, emit, **bad) == -1, bad
    assert case.padres(o, None, cd, emit) == -1                       # res_src == NULL
    assert case.padres(None, s_, None, emit) == -1                    # nothing to produce
    for bit in (N.PIPELINED, N.FP32_IN_CHUNK_MAJOR, N.FP32_OUT_CHUNK_MAJOR):
        assert case.padres(o, s_, cd, emit, flags=bit) == -1
        assert case.padres(o, s_, cd, emit, flags=bit | N.ROUTE_ONLY) == -1
    assert case.padres(o, s_ + 4, cd, emit) == -4                     # a source 4 bytes off
    assert case.padres(o + 4, s_, cd, emit) == -4
    assert case.padres(o, s_, cd + 4, emit) == -4
    for extra in (0, N.FORCE_TILED, N.EMIT_SHIFT128):
        assert case.padres(o, s_, cd, emit, flags=N.ROUTE_ONLY | extra) == N.ROUTE_TILED
    torch.cuda.synchronize()
    assert bool((obuf == SENTINEL).all()) and bool((cbuf == 0xa5).all())


def _wrapper_args(case):
    op = case.op
    return (op["codes"], op["wq"], op["wsum"], op["bias"], op["in_scale"], op["in_zp"], op["w_scale"])


def test_wrapper_takes_a_pad_shortcut_on_the_narrow_path_only():
    case = Case(**SHAPES["even_source_ceil"], ksize=3, seed=5)
    emit = _emit("u8")
    src = case.src_values.permute(0, 3, 1, 2)                         # (N, Cs, Hs, Ws), channels_last memory
    ps = K.PadShortcut(src, case.s, case.lo)
    kw = dict(padding=1, relu=True, emit=emit)
    out, codes = K.conv2d_i8(*_wrapper_args(case), residual=ps, out_channels=case.kf, **kw)
    mat = ps.materialise(case.kf)
    assert torch.equal(mat.permute(0, 2, 3, 1).reshape(-1), case.materialised())
    ref_out, ref_codes = K.conv2d_i8(*_wrapper_args(case), residual=mat, out_channels=case.kf, **kw)
    assert tuple(out.shape) == (case.n, case.kf, case.p, case.q) and torch.equal(out, ref_out) and torch.equal(codes, ref_codes)
    # ... not without out_channels, and not beside what the narrow path has no form of
    with pytest.raises(ValueError):
        K.conv2d_i8(*_wrapper_args(case), residual=ps, **kw)
    for bad in (dict(observe=True), dict(pipelined=True), dict(out_chunk_major=True),
                dict(in_offset=torch.zeros(1, device=DEV), tap_sums=torch.zeros(9, case.k, device=DEV))):
        with pytest.raises(ValueError):
            K.conv2d_i8(*_wrapper_args(case), residual=ps, out_channels=case.kf, **kw, **bad)
    with pytest.raises(ValueError):            # a shortcut of another shape: the 10 x 10 source at stride 1
        K.conv2d_i8(*_wrapper_args(case), residual=K.PadShortcut(src, 1, case.lo), out_channels=case.kf, **kw)
    with pytest.raises(ValueError):            # source and pad wider than the layer
        K.conv2d_i8(*_wrapper_args(case), residual=K.PadShortcut(src, case.s, 20), out_channels=case.kf, **kw)
    # ... and no source that is not dense in channels_last memory: a channel slice, a strided view, an NCHW-contiguous tensor
    wide = torch.randn(case.n, case.hs, case.ws, 2 * case.cs, device=DEV).permute(0, 3, 1, 2)
    for bad_src in (wide[:, :case.cs], src[:, :, ::2, ::2], src.contiguous()):
        with pytest.raises(ValueError):
            K.PadShortcut(bad_src, case.s, case.lo)
    for bad in (dict(stride=0), dict(lo=6), dict(lo=-4)):
        with pytest.raises(ValueError):
            K.PadShortcut(src, **{**dict(stride=2, lo=8), **bad})
    assert not isinstance(ps, torch.Tensor)          # (no tensor: a path that knows no pad shortcut cannot take it for one)


# ------------------------------------------------------------------------------------------------- the plan
def _net(option, cfg, qtype, batch, side, seed):
    import workloads as W
    from dlmc.quantization.scalar.FSPTQuant import FSPTQBase
    from dlmc.utils.merge_bn import merge_bn
    from dlmc.utils.quantize import quantize_model
    torch.manual_seed(seed)
    net = W.cifar_resnet20(option=option).to(DEV).eval()
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    net = merge_bn(net, inplace=True)
    if qtype:
        quantize_model(net, copy.deepcopy(cfg), None, qtype, int8_gemm=True)
    else:
        quantize_model(net, copy.deepcopy(cfg), None)
    x = torch.relu(torch.randn(batch, 3, side, side, device=DEV))
    with torch.no_grad():
        net(x)                                   # calibrate
    # every tensor a layer reads here is a ReLU output or the relu(N(0, 1)) image: minimum 0.  FSPTQ's zero point is set to exactly 0
    # (as test_gpu_gap.py does) so that no layer keeps its fp32 wrapper over a minimum that is merely close to 0
    for m in net.modules():
        if isinstance(m, FSPTQBase):
            m.in_offset.zero_()
            m._zp_is_int = None
    return net, x


def _graph_has_no_pad_or_slice(plan):
    import operator
    for n in plan.graph.nodes:
        if n.op == "call_function":
            assert n.target not in (F.pad, torch._C._nn.pad), n
            assert not (n.target is operator.getitem and not isinstance(n.args[1], int)), n


PLAN_CASES = [("qbase", QBASE_W8A8, None), ("fsptq", FSPTQ_W8A8, "FSPTQ")]


@pytest.mark.parametrize("batch, side", [(8, 32), (2, 16)])
@pytest.mark.parametrize("tag, cfg, qtype", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_cifar_resnet20_option_a_plan_flag_on_equals_flag_off(tag, cfg, qtype, batch, side):
    from dlmc.utils.fuse import Int8Layer, StreamedPlan, fuse_inference
    net, x = _net("A", cfg, qtype, batch, side, seed=41 + batch)
    off = fuse_inference(net, narrow_rows=True)
    on = fuse_inference(net, narrow_rows=True, pad_shortcuts=True)
    with torch.no_grad():
        a, b = off(x), on(x)
        again = on(x)
    print(off.fusion_report, on.fusion_report, sep="\n")
    ro, rn = off.fusion_report, on.fusion_report
    assert bool(torch.isfinite(a).all()) and torch.equal(b, again)
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} logits differ, max {float((a - b).abs().max())}"
    # (QBase at batch 2: the classifier reads a pooled tensor whose minimum is not 0 and keeps its wrapper, in both plans alike)
    assert (ro.pad_shortcuts, rn.pad_shortcuts) == (0, 2) and rn.skipped == ro.skipped
    assert (rn.layers, rn.residual, rn.relu, rn.emit, rn.fp32_outputs, rn.narrow, rn.dual) == \
           (ro.layers, ro.residual, ro.relu, ro.emit, ro.fp32_outputs, ro.narrow, ro.dual)
    _graph_has_no_pad_or_slice(on)
    nodes = [m for m in on.modules() if isinstance(m, Int8Layer) and m.pad_shortcut is not None]
    assert sorted((m.k, m.k_pad, m.pad_shortcut) for m in nodes) == [(32, 64, (2, 8)), (64, 64, (2, 16))]
    if qtype:           # (a QBase plan's scales depend on the elements per call: StreamedPlan refuses it, with or without the flag)
        with torch.no_grad():
            assert torch.equal(StreamedPlan(on, 2)(x), b)
    else:
        with pytest.raises(ValueError):
            StreamedPlan(on, 2)


@pytest.mark.parametrize("tag, cfg, qtype", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_option_b_network_gets_the_plan_it_gets_today(tag, cfg, qtype):
    from dlmc.utils.fuse import fuse_inference
    net, x = _net("B", cfg, qtype, 4, 32, seed=43)
    off = fuse_inference(net, narrow_rows=True)
    on = fuse_inference(net, narrow_rows=True, pad_shortcuts=True)
    assert repr(on.fusion_report) == repr(off.fusion_report) and on.fusion_report.pad_shortcuts == 0
    assert [(n.op, str(n.target), tuple(str(v) for v in n.args)) for n in on.graph.nodes] == \
           [(n.op, str(n.target), tuple(str(v) for v in n.args)) for n in off.graph.nodes]
    with torch.no_grad():
        assert torch.equal(on(x), off(x))


class _OffsetBlock(nn.Module):
    """A 64 -> 128 option-A block behind a 64 -> 64 convolution.  `relu_between=False`: the block's last convolution (3x3, padding 1)
    reads a tensor that goes negative, so that under QBase its unsigned quantiser gets a float offset and the layer the border term of
    the *_xoff kernels."""

    def __init__(self, relu_between):
        super().__init__()
        self.stem = nn.Conv2d(64, 64, 1)
        self.a = nn.Conv2d(64, 64, 3, stride=2, padding=1)
        self.b = nn.Conv2d(64, 128, 3, padding=1)
        self.relu_between = relu_between

    def forward(self, x):
        y = torch.relu(self.stem(x))
        t = self.a(y)
        t = torch.relu(t) if self.relu_between else t
        return torch.relu(self.b(t) + F.pad(y[:, :, ::2, ::2], (0, 0, 0, 0, 32, 32)))


@pytest.mark.parametrize("relu_between", [False, True])
def test_float_activation_offsets_beside_pad_shortcuts(relu_between):
    """The *_xoff kernels have no narrow form: a layer with their border term keeps the materialised shortcut (and the plan runs); the
    same block without the offset takes the pad shortcut under act_offsets=True as well."""
    from dlmc.utils.fuse import fuse_inference
    from dlmc.utils.quantize import quantize_model
    torch.manual_seed(61 + relu_between)
    net = _OffsetBlock(relu_between).to(DEV).eval()
    quantize_model(net, copy.deepcopy(QBASE_W8A8), None)
    x = torch.relu(torch.randn(3, 64, 9, 9, device=DEV))
    with torch.no_grad():
        net(x)                                   # calibrate
    off = fuse_inference(net, act_offsets=True)
    on = fuse_inference(net, act_offsets=True, pad_shortcuts=True)
    print(off.fusion_report, on.fusion_report, sep="\n")
    with torch.no_grad():
        a, b = off(x), on(x)
    assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    ro, rn = off.fusion_report, on.fusion_report
    assert (ro.layers, ro.residual, ro.skipped) == (3, 1, []) and (rn.layers, rn.residual, rn.skipped) == (3, 1, [])
    if relu_between:
        assert (ro.act_offset, rn.act_offset, rn.pad_shortcuts) == (0, 0, 1)
        _graph_has_no_pad_or_slice(on)
    else:
        assert (ro.act_offset, rn.act_offset, rn.pad_shortcuts) == (1, 1, 0)
        assert repr(rn) == repr(ro)
