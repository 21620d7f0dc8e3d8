"""dlmcq_conv2d_i8_nhwc_recompute_chain (a chain launch that recomputes its shortcut - the previous, convolution-shortcut block's output -
from that block's two code operands) against the pair of launches it replaces: dlmcq_conv2d_i8_nhwc_dual_chain writing its fp32 output
and dlmcq_conv2d_i8_nhwc_chain reading it.  Exact: fp32 compared as int32 bits, codes as bytes.

Shapes: the one instantiation there is (64 | 64, 64 -> 256 -> 64; ResNet-50's stage 1, stride 1; the 28^2 stride-2 form is not built,
nor a run-time-flag form, so no K = 128 / stride-2 cases).  2 x 9 x 7 = 126 pixels: two tiles, the last one partial (three at 56 rows);
K = 256: four chunks, the double buffer wraps; 1 x 5 x 7 = 35 pixels: less than one tile."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
C, K_, K2 = 64, 256, 64


def _layer(g, k, c):
    wq = torch.randint(-127, 128, (k, 1, 1, c), generator=g, device=DEV, dtype=torch.int8)
    return dict(wq=wq, wsum=wq.to(torch.int32).sum(dim=(1, 2, 3)).to(torch.int32).contiguous(), bias=torch.randn(k, generator=g, device=DEV),
                w_scale=(torch.rand(k, generator=g, device=DEV) * 0.004 + 0.001))


def _operand(g, n, h, w, k, c, zp, signed=False):
    lo, hi, dt = (-128, 128, torch.int8) if signed else (0, 256, torch.uint8)
    x = torch.randint(lo, hi, (n, c, h, w), generator=g, device=DEV, dtype=dt).contiguous(memory_format=torch.channels_last)
    return dict(_layer(g, k, c), codes=x, in_scale=torch.full((1,), 0.02, device=DEV),
                in_zp=None if zp is None else torch.full((1,), float(zp), device=DEV))


def _case(seed, n=2, h=9, w=7, zps=(None, None, None), signed=(False, False, False), no_bias=None):
    """x: this block's operand; pa, pb: the previous block's two; c3 / nxt: the reductions behind the two block ends."""
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    g = torch.Generator(device=DEV).manual_seed(seed)
    ops = [_operand(g, n, h, w, K_, C, zps[i], signed[i]) for i in range(3)]
    if no_bias is not None:
        ops[no_bias]["bias"] = None
    c3, nxt = {k: v for k, v in _layer(g, K2, K_).items()}, _layer(g, K2, K_)
    emits = [K.EmitCodes(torch.full((1,), s, device=DEV), None, 0, 255, N.FORM_ZEROPOINT) for s in (0.06, 0.11, 0.09, 0.13)]
    return K, ops[0], ops[1], ops[2], c3, nxt, emits


def _bits(t):
    return t.view(torch.int32)


def _compare(K, x, pa, pb, c3, nxt, emits, rows=0, out_cm=False, want_codes=True):
    e0, e03, e1, e12 = emits
    # the two existing launches: the first block writes its fp32 output, the second reads it
    y0, _, c0_r = K.conv2d_i8_dual_chain(pa, pb, c3, relu=True, emit=e0, want_out=True, relu3=True, emit3=e03, rows_per_tile=rows)
    y1_r, codes_r, c1_r = K.conv2d_i8_chain(x, nxt, y0, relu=True, emit=e1, want_out=True, want_codes=want_codes, relu2=True, emit2=e12,
                                            rows_per_tile=rows, out_chunk_major=out_cm)
    # the new pair: no fp32 output from the first, the second recomputes it
    none, _, c0 = K.conv2d_i8_dual_chain(pa, pb, c3, relu=True, emit=e0, want_out=False, relu3=True, emit3=e03, rows_per_tile=rows)
    y1, codes, c1 = K.conv2d_i8_recompute_chain(x, nxt, pa, pb, relu_shortcut=True, relu=True, emit=e1, want_out=True, want_codes=want_codes,
                                                relu2=True, emit2=e12, rows_per_tile=rows, out_chunk_major=out_cm)
    torch.cuda.synchronize()
    assert none is None and torch.equal(c0, c0_r)
    assert isinstance(y1, K.ChunkMajor) == out_cm
    if out_cm:
        assert y1.shape == y1_r.shape and torch.equal(_bits(y1.buf), _bits(y1_r.buf))
    else:
        assert torch.equal(_bits(y1), _bits(y1_r))
    if want_codes:
        assert torch.equal(codes, codes_r)
    else:
        assert codes is None
    assert torch.equal(c1, c1_r)
    # the stage-end flavour: codes without an fp32 output (the kernel's other compile-time form)
    _, codes_n, c1_n = K.conv2d_i8_recompute_chain(x, nxt, pa, pb, emit=e1, want_out=False, want_codes=True, emit2=e12, rows_per_tile=rows)
    if want_codes:
        assert torch.equal(codes_n, codes_r)
    assert torch.equal(c1_n, c1_r)


@pytest.mark.parametrize("rows", [0, 56])
@pytest.mark.parametrize("out_cm", [False, True])
def test_recompute_chain_matches_the_two_launches(rows, out_cm):
    K, *case = _case(11 + rows)
    assert K.recompute_chain_supported(C, C, C, K_, K2, 126)
    _compare(K, *case, rows=rows, out_cm=out_cm)
    _compare(K, *case, rows=rows, out_cm=out_cm, want_codes=False)


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("signed", [False, True])
def test_recompute_chain_zero_points_and_signed_codes(which, signed):
    """A non-zero integer zero point on each of the three inputs in turn, that input's codes unsigned or signed."""
    zps, sg = [None] * 3, [False] * 3
    zps[which], sg[which] = (7 if not signed else -5), signed
    K, *case = _case(23 + which, zps=tuple(zps), signed=tuple(sg))
    _compare(K, *case)
    K, *case = _case(29 + which, zps=(3, 2, 9), signed=(signed,) * 3)
    _compare(K, *case, out_cm=True)


@pytest.mark.parametrize("which", [0, 1, 2])
def test_recompute_chain_without_a_bias(which):
    K, *case = _case(31 + which, no_bias=which)
    _compare(K, *case)


def test_recompute_chain_less_than_one_tile():
    K, *case = _case(41, n=1, h=5, w=7, zps=(1, None, 4))
    _compare(K, *case)
    _compare(K, *case, rows=56, out_cm=True)


def test_recompute_chain_shortcut_without_relu():
    """relu_shortcut = 0 recomputes what the first block stores when it has no ReLU (its run-time-flag form)."""
    K, x, pa, pb, c3, nxt, (e0, e03, e1, e12) = _case(43)
    y0, _, _ = K.conv2d_i8_dual_chain(pa, pb, c3, relu=False, emit=e0, want_out=True, relu3=True, emit3=e03)
    assert bool((y0 < 0).any())
    y1_r, _, c1_r = K.conv2d_i8_chain(x, nxt, y0, emit=e1, want_out=True, emit2=e12)
    y1, _, c1 = K.conv2d_i8_recompute_chain(x, nxt, pa, pb, relu_shortcut=False, emit=e1, want_out=True, emit2=e12)
    assert torch.equal(_bits(y1), _bits(y1_r)) and torch.equal(c1, c1_r)


def test_recompute_chain_refuses_bad_arguments():
    from dlmc import _native as N
    K, x, pa, pb, c3, nxt, (e0, e03, e1, e12) = _case(47)
    n, _, h, w = x["codes"].shape
    out = torch.empty((n, K_, h, w), device=DEV).contiguous(memory_format=torch.channels_last)
    codes2 = torch.empty((n, K2, h, w), dtype=torch.uint8, device=DEV).contiguous(memory_format=torch.channels_last)
    keep = [t[k].contiguous() for t in (x, pa, pb, nxt) for k in ("w_scale",)]

    def op(t, ws):
        return [N.ptr(t["codes"]), N.ptr(t["wq"]), N.ptr(t["bias"]), N.ptr(t["wsum"]), N.ptr(t["in_scale"]), None, N.ptr(ws)]
    hx = op(x, keep[0])
    args = [hx[0], hx[1], N.ptr(out), *hx[2:], n, h, w, C, K_, 1, *op(pa, keep[1]), C, 1, *op(pb, keep[2]), h, w, C, 1, 1,
            1, 1, None, N.ptr(e1.scale), None, 0, 255, e1.form, 0.0,
            N.ptr(nxt["wq"]), N.ptr(nxt["bias"]), N.ptr(nxt["wsum"]), N.ptr(keep[3]), K2, 1, N.ptr(codes2), N.ptr(e12.scale), None, 0, 255,
            e12.form, 0.0, 0, N.stream_ptr()]
    X, W_, OUT, XA, WA, XB, WB, RELU_SC, RELU, Q_SCALE, Q_HI, W2, RELU2, CODES2, Q2_SCALE, Q2_FORM = 0, 1, 2, 14, 15, 23, 24, 35, 36, 38, 41, 44, 49, 50, 51, 55

    def call(**changes):
        a = list(args)
        for i, v in changes.items():
            a[int(i[1:])] = v
        return N.lib.dlmcq_conv2d_i8_nhwc_recompute_chain(*a)

    def off(i, by=4):
        return ctypes.c_void_p(args[i].value + by)
    assert call() == 0
    torch.cuda.synchronize()
    for i in (X, W_, XA, WA, XB, WB, W2, CODES2, Q_SCALE, Q2_SCALE, 4, 17, 26, 46):      # (4, 17, 26, 46: the four weight-sum tables)
        assert call(**{f"i{i}": None}) == -1, i                                           # DLMCQ_EINVAL
    for i in (X, W_, OUT, XA, WA, XB, WB, W2, CODES2):
        assert call(**{f"i{i}": off(i)}) == -4, i                                         # DLMCQ_EALIGN
    for i in (RELU_SC, RELU, RELU2):
        assert call(**{f"i{i}": N.ACT_RELU6}) == -1, i
    assert call(**{f"i{Q_HI}": 127}) == -1                                                # the second reduction reads unsigned bytes
    assert call(**{f"i{RELU}": 0}) == -1                                                  # no run-time-flag form of this kernel
    assert call(**{f"i{Q2_FORM}": e12.form | N.FORCE_TILED}) == -1
    assert call(**{f"i{Q2_FORM}": e12.form | N.FP32_OUT_CHUNK_MAJOR}) == 0                # the chunk-major out bit is taken
    assert call(i12=200) == -1                                                            # K % 64
    assert call(i30=h + 1) == -1                                                          # the recomputed block gives another height
    assert call(i8=0) == 0                                                                # an empty batch: nothing to do
    torch.cuda.synchronize()
    assert not K.recompute_chain_supported(128, 128, 256, 512, 128, 126)
