"""The quantising epilogue of every int8 kernel family against an exact reference (tests/exact_layers.py): layers whose fp32 result is
exact carry rounding ties on even and odd integers, values one ulp from a tie, v = s (k + 1/2) at the awkward consumer scales 3 and 6,
NaN, +-inf, saturating values and degenerate scales, and every kernel must give the float64 reference's fp32 values bit for bit and
the oracle's codes byte for byte - no tolerance, no off-by-one rate.  Each case first asserts which kernel the library's dispatch
picks for it (DLMCQ_ROUTE_ONLY through the profile tags), so a shape that falls back to the tiled kernel fails instead of passing."""
import pytest
import torch

import exact_layers as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL = -1


def gen(seed):
    return torch.Generator().manual_seed(9100 + seed)


def same(got, want, what, errs=None):
    """fp32: bit equality with +0 == -0 (NaN where NaN); codes: byte equality.  With `errs` the mismatch is recorded there (a case
    reports every quantiser and activation that fails, not just the first) - end the case with `settle(errs)`."""
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if want.dtype == torch.float32:
        a, b = got + 0.0, want + 0.0
        bad = a.view(torch.int32) != b.view(torch.int32)
    else:
        bad = got != want
    if bool(bad.any()):
        idx = bad.nonzero()[:4].tolist()
        ex = [(i, got[tuple(i)].item(), want[tuple(i)].item()) for i in idx]
        msg = f"{what}: {int(bad.sum())} of {want.numel()} differ, e.g. (index, got, want) {ex}"
        if errs is None:
            raise AssertionError(msg)
        errs.append(msg)


def settle(errs):
    assert not errs, f"{len(errs)} mismatches:\n" + "\n".join(errs)


def tagged(K, fn):
    """fn() with the launch profile on: (result, tags of the launches it made - the library's own routing answer)."""
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        r = fn()
    finally:
        K.PROFILE.enabled = False
    tags = [rec[0] for rec in K.PROFILE.records]
    K.PROFILE.reset()
    return r, tags


def t1(v):
    return torch.tensor([float(v)], dtype=torch.float32, device=DEV)


def emit_of(K, q):
    return K.EmitCodes(t1(q.scale), None if q.zp is None else t1(q.zp), q.lo, q.hi, q.form, q.g, q.shift128)


_PINNED = set()


def expect_codes(K, v32, q):
    """The reference's codes of v32 under q; once per quantiser also checked against dlmcq_fake_quant_f32 (DLMCQ_CODES_I8) on the same
    tensor, which the golden vectors pin - so the reference cannot drift from the oracle the rest of the suite trusts."""
    want = X.quantise(v32, q)
    key = q.tag()
    if key not in _PINNED:
        plain_q = X.Quant(q.scale, q.zp, q.lo, q.hi, q.form, q.g)
        _, kc = K.fake_quant(v32.to(DEV), t1(q.scale), None if q.zp is None else t1(q.zp), q.lo, q.hi, q.form, g=q.g, codes="i8",
                             want_y=False)
        same(kc.cpu().view(torch.uint8), X.quantise(v32, plain_q).view(torch.uint8), f"reference vs dlmcq_fake_quant_f32 {key}")
        _PINNED.add(key)
    return want


def cl(t):
    return t.to(DEV).contiguous(memory_format=torch.channels_last)


def dev_weights(K, lay):
    k = lay.wq.shape[0]
    wq, wsum = K.quantize_weight_krsc(lay.wq.float().to(DEV), torch.ones(k, device=DEV), -127, 127)
    return wq, wsum


ALL_Q = X.plain_quants() + X.nonplain_quants()
SHIFTED = [X.Quant(1.0, None, 0, 255, X.FORM_ZEROPOINT, shift128=True), X.Quant(3.0, 3.0, 0, 255, X.FORM_ZEROPOINT, shift128=True)]


# ------------------------------------------------------------------------------------------------ dlmcq_conv2d_i8_nhwc_fused family
CONV_CASES = {
    # name: (N, C, H, W, K, R, stride, pad, options, route)
    "tiled_vector": (2, 64, 9, 9, 128, 3, 1, 1, dict(force_tiled=True, want_out=True), "conv_i8"),
    "tiled_swapped": (2, 64, 9, 9, 64, 1, 1, 0, dict(force_tiled=True, want_out=False), "conv_i8"),
    "tiled_scalar_k42": (2, 64, 9, 9, 42, 3, 1, 1, dict(force_tiled=True, want_out=True), "conv_i8"),
    "tiled_scalar_k42_codes": (2, 64, 9, 9, 42, 3, 1, 1, dict(force_tiled=True, want_out=False), "conv_i8"),
    "tiled_asym192": (2, 64, 8, 8, 192, 1, 1, 0, dict(asym=True, want_out=False), "conv_i8"),
    "tiled_asym_signed": (2, 64, 9, 9, 128, 3, 2, 1, dict(asym=True, signed=True, want_out=True), "conv_i8"),
    "tiled_residual": (2, 64, 8, 8, 128, 1, 1, 0, dict(force_tiled=True, residual=True, want_out=True, zp=2.0), "conv_i8"),
    "tiled_observed": (2, 64, 8, 8, 128, 1, 1, 0, dict(observe=True, want_out=True), "conv_i8"),
    "pw_64_128": (4, 64, 32, 32, 128, 1, 1, 0, dict(want_out=False, plain_only=True), "conv_pw"),
    "pw_128_192_asym": (4, 128, 32, 32, 192, 1, 1, 0, dict(want_out=False, plain_only=True, asym=True, zp=2.0), "conv_pw"),
    "pwr_codes": (4, 256, 32, 32, 128, 1, 1, 0, dict(residual=True, want_out=False, plain_only=True, relu_only=True), "conv_pwr"),
    "pwr_out_codes": (4, 512, 32, 32, 256, 1, 1, 0, dict(residual=True, want_out=True, plain_only=True, relu_only=True, signed=True),
                      "conv_pwr"),
    "halo_s1": (2, 64, 16, 16, 128, 3, 1, 1, dict(want_out=False, no_relu6=True), "conv3x3_halo"),
    "halo_s2": (2, 128, 16, 16, 64, 3, 2, 1, dict(want_out=False, no_relu6=True, zp=2.0), "conv3x3_halo"),
    "halo_pipe": (18, 128, 60, 60, 256, 3, 1, 1, dict(want_out=False, plain_only=True, relu_only=True, pipelined=True, few_q=True),
                  "conv3x3_pipe"),
}


def _acts(opt):
    return [1] if opt.get("relu_only") else ([0, 1] if opt.get("no_relu6") else [0, 1, 2])


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_conv_family_epilogue_is_exact(name):
    from dlmc.quantization.scalar import kernels as K
    n, c, h, w, k, r, stride, pad, opt, route = CONV_CASES[name]
    gg = gen(list(CONV_CASES).index(name))
    lay = X.make_layer(gg, n, c, h, w, k, r, signed_in=opt.get("signed", False), zp=opt.get("zp", 0.0), asym=opt.get("asym", False))
    p, q_ = (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1
    res = None
    if opt.get("residual"):
        lay.bias[:lay.nz] = 0.0
        res = X.edge_residual((n, k, p, q_), lay.nz, gg)
    base = X.conv_ref(lay, stride, pad, residual=res)          # (act 0; the activations below act on these exact values)
    codes, (wq, wsum) = cl(lay.codes), dev_weights(K, lay)
    kw = dict(stride=stride, padding=pad, residual=None if res is None else cl(res),
              w_offset=None if lay.w_off is None else lay.w_off.to(DEV), force_tiled=opt.get("force_tiled", False),
              pipelined=opt.get("pipelined", False), observe=opt.get("observe", False))
    quants = X.plain_quants() if opt.get("plain_only") else ALL_Q + SHIFTED
    if opt.get("few_q"):
        quants = [q for q in quants if q.scale in (1.0, 0.5, 3.0, 6.0, 7.0, 15.0, 1e-41)]
    want_out = opt["want_out"]
    errs = []
    for act in _acts(opt):
        want = X.exact_f32(X.activation(base.double(), act))
        for q in quants:
            what = f"{name} act={act} {q.tag()}"

            def run():
                return K.conv2d_i8(codes, wq, wsum, lay.bias.to(DEV), t1(1.0), t1(lay.zp), torch.ones(k, device=DEV), act=act,
                                   emit=emit_of(K, q), want_out=want_out, **kw)
            (out, got), tags = tagged(K, run)
            assert tags == [route], (what, tags)
            if want_out:
                same(out, want, what + " fp32", errs)
            same(got, expect_codes(K, want, q), what + " codes", errs)
    settle(errs)


# ------------------------------------------------------------------------------------------------ dlmcq_conv2d_i8_nhwc_dual
def test_dual_block_end_epilogue_is_exact():
    """conv1x1(256) + conv1x1(512, stride 2) + ReLU -> fp32 + plain codes: the block-end kernel's dual form."""
    from dlmc.quantization.scalar import kernels as K
    gg = gen(40)
    n, h, w, k = 4, 32, 32, 128
    la = X.make_layer(gg, n, 256, h, w, k, 1)
    lb = X.make_layer(gg, n, 512, 2 * h, 2 * w, k, 1, nz=la.nz)
    lb.bias = torch.randint(-2, 3, (k,), generator=gg).float()
    lb.bias[:lb.nz] = 0.0
    base = X.exact_f32(X.conv_ref(la).double() + X.conv_ref(lb, stride=2).double())    # (integer + a dyadic bias, or an edge value + 0)
    want = X.exact_f32(X.activation(base.double(), 1))

    def dev(lay, stride):
        wq, wsum = dev_weights(K, lay)
        return dict(codes=cl(lay.codes), wq=wq, wsum=wsum, bias=lay.bias.to(DEV), in_scale=t1(1.0), in_zp=t1(lay.zp),
                    w_scale=torch.ones(k, device=DEV), stride=stride)
    a, b = dev(la, 1), dev(lb, 2)
    errs = []
    for q in X.plain_quants():
        what = f"dual {q.tag()}"
        (out, got), tags = tagged(K, lambda: K.conv2d_i8_dual(a, b, relu=True, emit=emit_of(K, q)))
        assert tags == ["conv_pwr"], (what, tags)
        same(out, want, what + " fp32", errs)
        same(got, expect_codes(K, want, q), what + " codes", errs)
    settle(errs)


# ------------------------------------------------------------------------------------------------ depthwise
DW_CASES = {
    # name: (N, C, H, W, R, stride, pad, asym, force_tiled, want_out, route)   FAST: 2 = plain + symmetric, 1 = plain + asym, 0 otherwise
    "dwm": (4, 64, 32, 32, 3, 1, 1, False, False, False, "conv_dwm"),
    "dwm_asym": (4, 128, 32, 32, 3, 1, 1, True, False, False, "conv_dwm"),
    "dw3p2_codes": (2, 64, 15, 15, 3, 1, 1, False, True, False, "conv_dw"),
    "dw3p2_codes_asym": (2, 64, 15, 15, 3, 1, 1, True, True, False, "conv_dw"),
    "dw3p2_out": (2, 64, 15, 15, 3, 1, 1, True, True, True, "conv_dw"),
    "dw3_s2_codes": (2, 96, 16, 16, 3, 2, 1, False, False, False, "conv_dw"),
    "dw3_s2_asym_out": (2, 96, 16, 16, 3, 2, 1, True, False, True, "conv_dw"),
    "dw_generic_r5": (2, 84, 9, 9, 5, 1, 2, True, False, False, "conv_dw"),
}


@pytest.mark.parametrize("name", list(DW_CASES))
def test_depthwise_epilogue_is_exact(name):
    from dlmc.quantization.scalar import kernels as K
    n, c, h, w, r, stride, pad, asym, force, want_out, route = DW_CASES[name]
    gg = gen(500 + list(DW_CASES).index(name))
    lay = X.make_layer(gg, n, c, h, w, c, r, depthwise=True, asym=asym, zp=2.0 if asym else 0.0)
    base = X.conv_ref(lay, stride, pad)
    wq = lay.wq.reshape(c, r, r).permute(1, 2, 0).contiguous().to(DEV)        # [R, S, C]
    codes = cl(lay.codes)
    kw = dict(w_offset=None if lay.w_off is None else lay.w_off.to(DEV), stride=stride, padding=pad, force_tiled=force)
    quants = X.plain_quants() if route == "conv_dwm" else ALL_Q
    errs = []
    for act in (0, 1, 2):
        want = X.exact_f32(X.activation(base.double(), act))
        for q in quants:
            what = f"{name} act={act} {q.tag()}"
            (res_, tags) = tagged(K, lambda: K.conv2d_dw_i8(codes, wq, lay.bias.to(DEV), t1(1.0), t1(lay.zp), torch.ones(c, device=DEV),
                                                           act=act, emit=emit_of(K, q), want_out=want_out, **kw))
            out, got = res_
            assert tags == [route], (what, tags)
            if want_out:
                same(out, want, what + " fp32", errs)
            same(got, expect_codes(K, want, q), what + " codes", errs)
    settle(errs)


# ------------------------------------------------------------------------------------------------ chain, dual chain
# the first quantiser's scale and zero point are the second GEMM's input scale and zero point: powers of two keep that GEMM exact
FIRST_Q = [X.Quant(1.0), X.Quant(0.5, form=X.FORM_SYMMETRIC), X.Quant(1.0, 3.0), X.Quant(0.5, 3.0)]
LAST_Q = X.plain_quants() + X.nonplain_quants() + SHIFTED


def _second(gg, k, k2):
    wq2, b2 = X.identity_pw(k2, k, 24, gg)
    return wq2, b2


@pytest.mark.parametrize("shape", [(64, 128, 64), (128, 128, 128), (256, 64, 256)], ids=lambda s: "x".join(map(str, s)))
def test_chain_epilogues_are_exact(shape):
    from dlmc.quantization.scalar import kernels as K
    c, k, k2 = shape
    gg = gen(600 + c + k2)
    n, h, w = 2, 8, 8
    assert K.chain_supported(c, k, k2, n * h * w)
    lay = X.make_layer(gg, n, c, h, w, k, 1)
    lay.bias[:lay.nz] = 0.0
    res = X.edge_residual((n, k, h, w), lay.nz, gg)
    wq2, b2 = _second(gg, k, k2)
    base = X.conv_ref(lay, residual=res)
    wq1d, ws1 = dev_weights(K, lay)
    wq2d, ws2 = K.quantize_weight_krsc(wq2.float().to(DEV), torch.ones(k2, device=DEV), -127, 127)
    a = dict(codes=cl(lay.codes), wq=wq1d, wsum=ws1, bias=lay.bias.to(DEV), in_scale=t1(1.0), in_zp=t1(lay.zp), w_scale=torch.ones(k, device=DEV))
    b = dict(wq=wq2d, wsum=ws2, bias=b2.to(DEV), w_scale=torch.ones(k2, device=DEV))
    errs = []
    for relu, relu2 in ((1, 1), (0, 0)):
        mid = X.exact_f32(X.activation(base.double(), relu))
        for q1 in FIRST_Q:
            c1 = expect_codes(K, mid, q1)
            v2 = X.second_gemm_ref(c1, q1, wq2, b2, act2=relu2)
            for q2 in LAST_Q:
                what = f"chain {shape} relu={relu}/{relu2} {q1.tag()} -> {q2.tag()}"
                (out, got1, got2), tags = tagged(K, lambda: K.conv2d_i8_chain(a, b, cl(res), relu=bool(relu), emit=emit_of(K, q1),
                                                                             want_out=True, want_codes=True, relu2=bool(relu2),
                                                                             emit2=emit_of(K, q2)))
                assert tags == ["conv_chain"], (what, tags)
                same(out, mid, what + " fp32", errs)
                same(got1, c1, what + " first codes", errs)
                same(got2, expect_codes(K, v2, q2), what + " second codes", errs)
    settle(errs)


@pytest.mark.parametrize("shape", [(64, 64, 128, 64), (128, 256, 128, 128)], ids=lambda s: "x".join(map(str, s)))
def test_dual_chain_epilogues_are_exact(shape):
    from dlmc.quantization.scalar import kernels as K
    c, c2, k, k3 = shape
    gg = gen(700 + c + c2)
    n, h, w = 2, 8, 8
    assert K.dual_chain_supported(c, c2, k, k3, n * h * w)
    la = X.make_layer(gg, n, c, h, w, k, 1)
    lb = X.make_layer(gg, n, c2, 2 * h, 2 * w, k, 1, nz=la.nz)
    lb.bias = torch.randint(-2, 3, (k,), generator=gg).float()
    lb.bias[:lb.nz] = 0.0
    base = X.exact_f32(X.conv_ref(la).double() + X.conv_ref(lb, stride=2).double())
    wq3, b3 = _second(gg, k, k3)

    def dev(lay, stride):
        wq, wsum = dev_weights(K, lay)
        return dict(codes=cl(lay.codes), wq=wq, wsum=wsum, bias=lay.bias.to(DEV), in_scale=t1(1.0), in_zp=t1(lay.zp),
                    w_scale=torch.ones(k, device=DEV), stride=stride)
    a, b = dev(la, 1), dev(lb, 2)
    wq3d, ws3 = K.quantize_weight_krsc(wq3.float().to(DEV), torch.ones(k3, device=DEV), -127, 127)
    c3 = dict(wq=wq3d, wsum=ws3, bias=b3.to(DEV), w_scale=torch.ones(k3, device=DEV))
    mid = X.exact_f32(X.activation(base.double(), 1))
    errs = []
    for q1 in FIRST_Q:
        c1 = expect_codes(K, mid, q1)
        v3 = X.second_gemm_ref(c1, q1, wq3, b3, act2=1)
        for q3 in LAST_Q:
            what = f"dual chain {shape} {q1.tag()} -> {q3.tag()}"
            (out, got1, got3), tags = tagged(K, lambda: K.conv2d_i8_dual_chain(a, b, c3, relu=True, emit=emit_of(K, q1), want_out=True,
                                                                              want_codes=True, relu3=True, emit3=emit_of(K, q3)))
            assert tags == ["conv_chain"], (what, tags)
            same(out, mid, what + " fp32", errs)
            same(got1, c1, what + " first codes", errs)
            same(got3, expect_codes(K, v3, q3), what + " last codes", errs)
    settle(errs)


# ------------------------------------------------------------------------------------------------ dwpw
@pytest.mark.parametrize("k", [128, 192, 512])
def test_dwpw_epilogues_are_exact(k):
    from dlmc.quantization.scalar import kernels as K
    gg = gen(800 + k)
    n, c, h, w = 2, 64, 12, 12
    assert K.dwpw_supported(c, k, h, w, 1, 1, 3)
    errs = []
    for asym in (False, True):
        lay = X.make_layer(gg, n, c, h, w, c, 3, depthwise=True, asym=asym, zp=2.0 if asym else 0.0)
        base = X.conv_ref(lay, 1, 1)
        wq_dw = lay.wq.reshape(c, 3, 3).permute(1, 2, 0).contiguous().to(DEV)
        table = K.dwpw_table(wq_dw, lay.bias.to(DEV), t1(1.0), t1(lay.zp), torch.ones(c, device=DEV),
                             None if lay.w_off is None else lay.w_off.to(DEV), x_unsigned=True)
        wq2, b2 = X.identity_pw(k, c, 24, gg)
        wq2d, ws2 = K.quantize_weight_krsc(wq2.float().to(DEV), torch.ones(k, device=DEV), -127, 127)
        codes = cl(lay.codes)
        for dw_relu in (1, 0):
            mid = X.exact_f32(X.activation(base.double(), dw_relu))
            for q1 in FIRST_Q:
                c1 = X.quantise(mid, q1)
                v2 = X.second_gemm_ref(c1, q1, wq2, b2, act2=1)
                pw = dict(wq=wq2d, wsum=ws2, bias=b2.to(DEV), w_scale=torch.ones(k, device=DEV), in_scale=t1(q1.scale))
                for q2 in X.plain_quants() + X.nonplain_quants():
                    what = f"dwpw k={k} asym={asym} dw_relu={dw_relu} {q1.tag()} -> {q2.tag()}"
                    got, tags = tagged(K, lambda: K.conv2d_dwpw_i8(codes, table, asym, True, bool(dw_relu), t1(lay.zp), emit_of(K, q1), pw,
                                                                  relu=True, emit2=emit_of(K, q2)))
                    assert tags == ["conv_dwpw"], (what, tags)
                    same(got, expect_codes(K, v2, q2), what + " codes", errs)
    settle(errs)


# ------------------------------------------------------------------------------------------------ first layer (stem)
def edge_image(gg, n, c, h, w):
    """fp32 image with the edge values and exact ties placed per pixel."""
    img = torch.randint(-8, 9, (n, c, h, w), generator=gg).float() * 0.5
    ev = torch.tensor(X.EDGE_VALUES, dtype=torch.float32)
    flat = img.view(-1)
    pos = torch.randperm(flat.numel(), generator=gg)[:4 * len(X.EDGE_VALUES)]
    flat[pos] = ev.repeat(4)
    return img


@pytest.mark.parametrize("layout", ["contiguous", "channels_last"])
def test_quantize_pad_is_exact(layout):
    from dlmc.quantization.scalar import kernels as K
    gg = gen(900)
    n, c, h, w, pad = 2, 3, 16, 20, 2
    img = edge_image(gg, n, c, h, w)
    x = img.to(DEV) if layout == "contiguous" else cl(img)
    padded = torch.nn.functional.pad(img, (pad, pad, pad, pad), value=0.0).permute(0, 2, 3, 1).contiguous()    # (N, Hp, Wp, C)
    errs = []
    for q in ALL_Q + SHIFTED:
        what = f"quantize_pad {layout} {q.tag()}"
        got, tags = tagged(K, lambda: K.quantize_pad_nhwc4(x, t1(q.scale), None if q.zp is None else t1(q.zp), q.lo, q.hi, q.form, pad,
                                                          g=q.g, shift128=q.shift128))
        assert tags == ["fq_image"], (what, tags)
        want = expect_codes(K, padded, q)
        same(got[..., :c].contiguous(), want, what, errs)
    settle(errs)


STEM_CASES = {
    # name: (N, H, W, K, R, stride, pad, asym, pool, want_out, expect the in-register 7x7 pooling kernel)
    "r3_codes_swapped": (2, 32, 32, 64, 3, 2, 1, False, False, False, False),
    "r3_out": (2, 32, 32, 64, 3, 2, 1, False, False, True, False),
    "r7_asym": (2, 32, 32, 96, 7, 2, 3, True, False, False, False),
    "r3_asym_out": (3, 17, 23, 96, 3, 2, 1, True, False, True, False),
    "pool_generic": (2, 30, 30, 64, 3, 2, 1, False, True, False, False),
    "pool7": (2, 32, 32, 64, 7, 2, 3, False, True, False, True),
}


@pytest.mark.parametrize("name", list(STEM_CASES))
def test_stem_epilogue_is_exact(name):
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    n, h, w, k, r, stride, pad, asym, pool, want_out, pool7 = STEM_CASES[name]
    gg = gen(1000 + list(STEM_CASES).index(name))
    c = 3
    zp = 2.0
    lay = X.make_layer(gg, n, c, h, w, k, r, asym=asym, zp=zp)
    img = lay.codes.float() - zp                                # the image whose codes (scale 1, zero point 2) are lay.codes
    xpad = K.quantize_pad_nhwc4(img.to(DEV), t1(1.0), t1(zp), 0, 255, N.FORM_ZEROPOINT, pad)
    wq, wsum = K.quantize_weight_stem(lay.wq.float().to(DEV), torch.ones(k, device=DEV), -127, 127)
    hp, wp = h + 2 * pad, w + 2 * pad
    if pool7:       # stem_pool7_applies (csrc/conv_stem_pool7_i8.hip): codes only, 7x7 / 2, K = 64, an even convolution output
        P, Q = (hp - r) // stride + 1, (wp - r) // stride + 1
        assert (r, stride, k, want_out, P % 2, Q % 2) == (7, 2, 64, False, 0, 0)
    acts = [1] if pool else [0, 1, 2]
    base = X.conv_ref(lay, stride, pad)
    quants = ALL_Q
    kw = dict(stride=stride, pool=pool, w_offset=None if lay.w_off is None else lay.w_off.to(DEV), channels=c)
    errs = []
    for act in acts:
        want = X.exact_f32(X.activation(base.double(), act))
        if pool:
            want = X.exact_f32(torch.nn.functional.max_pool2d(want.double(), 3, 2, 1))
        for q in quants:
            what = f"stem {name} act={act} {q.tag()}"
            res_, tags = tagged(K, lambda: K.conv2d_i8_stem(xpad, wq, wsum, lay.bias.to(DEV), t1(1.0), t1(zp), torch.ones(k, device=DEV), r,
                                                           act=act, emit=emit_of(K, q), want_out=want_out, **kw))
            out, got = res_
            assert tags == ["conv_stem"], (what, tags)
            if want_out:
                same(out, want, what + " fp32", errs)
            same(got, expect_codes(K, want, q), what + " codes", errs)
    settle(errs)


# ------------------------------------------------------------------------------------------------ control bits (include/dlmcq.h)
def _sentinel(t):
    t.view(torch.uint8).fill_(0xA5)
    return t


def _untouched(t, what):
    assert bool((t.view(torch.uint8) == 0xA5).all()), f"{what}: the call wrote to its output"


CTL_BITS = ("FORCE_TILED", "ROUTE_ONLY", "PIPELINED")


def test_chain_entry_points_refuse_control_bits():
    """DLMCQ_FORCE_TILED / ROUTE_ONLY / PIPELINED in the last form argument of the chain entry points: DLMCQ_EINVAL, nothing written (real,
    correctly sized buffers: a library that launched anyway would write only inside them)."""
    import ctypes
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    gg = gen(1100)
    n, h, w, c, k, k2 = 2, 8, 8, 64, 128, 64
    lay = X.make_layer(gg, n, c, h, w, k, 1)
    wq1, ws1 = dev_weights(K, lay)
    wq2, ws2 = K.quantize_weight_krsc(X.identity_pw(k2, k, 8, gg)[0].float().to(DEV), torch.ones(k2, device=DEV), -127, 127)
    x, res = cl(lay.codes), cl(torch.zeros(n, k, h, w))
    out, codes, codes2 = (_sentinel(torch.empty(n * h * w * k, device=DEV)), _sentinel(torch.empty(n * h * w * k, dtype=torch.uint8, device=DEV)),
                          _sentinel(torch.empty(n * h * w * k2, dtype=torch.uint8, device=DEV)))
    one, ones_k, ones_k2, bias, bias2 = t1(1.0), torch.ones(k, device=DEV), torch.ones(k2, device=DEV), lay.bias.to(DEV), torch.zeros(k2, device=DEV)
    P = N.ptr
    for bit in CTL_BITS:
        rc = N.lib.dlmcq_conv2d_i8_nhwc_chain(
            P(x), P(wq1), P(out), P(bias), P(ws1), P(one), None, P(ones_k), n * h * w, c, k, 1, P(res), 1, P(codes), P(one), None, 0, 255,
            N.FORM_ZEROPOINT, 0.0, P(wq2), P(bias2), P(ws2), P(ones_k2), k2, 1, P(codes2), P(one), None, 0, 255,
            N.FORM_ZEROPOINT | getattr(N, bit), 0.0, 0, N.stream_ptr())
        torch.cuda.synchronize()
        assert rc == EINVAL, (bit, rc)
        for t, nm in ((out, "out"), (codes, "codes"), (codes2, "codes2")):
            _untouched(t, f"chain {bit} {nm}")
    # dual chain: the same bits in q3_form
    xb = cl(X.make_layer(gg, n, c, 2 * h, 2 * w, k, 1).codes)
    for bit in CTL_BITS:
        rc = N.lib.dlmcq_conv2d_i8_nhwc_dual_chain(
            P(x), P(wq1), P(out), P(bias), P(ws1), P(one), None, P(ones_k), n, h, w, c, k, 1, P(xb), P(wq1), P(bias), P(ws1), P(one), None,
            P(ones_k), 2 * h, 2 * w, c, 2, 1, 1, P(codes), P(one), None, 0, 255, N.FORM_ZEROPOINT, 0.0, P(wq2), P(bias2), P(ws2), P(ones_k2),
            k2, 1, P(codes2), P(one), None, 0, 255, N.FORM_ZEROPOINT | getattr(N, bit), 0.0, 0, N.stream_ptr())
        torch.cuda.synchronize()
        assert rc == EINVAL, (bit, rc)
        for t, nm in ((out, "out"), (codes, "codes"), (codes2, "codes3")):
            _untouched(t, f"dual chain {bit} {nm}")


def test_dwpw_and_quantize_pad_refuse_flag_bits():
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    gg = gen(1200)
    n, c, h, w, k = 2, 64, 12, 12, 128
    lay = X.make_layer(gg, n, c, h, w, c, 3, depthwise=True)
    wq_dw = lay.wq.reshape(c, 3, 3).permute(1, 2, 0).contiguous().to(DEV)
    table = K.dwpw_table(wq_dw, lay.bias.to(DEV), t1(1.0), t1(0.0), torch.ones(c, device=DEV), None)
    wq2, ws2 = K.quantize_weight_krsc(X.identity_pw(k, c, 8, gg)[0].float().to(DEV), torch.ones(k, device=DEV), -127, 127)
    x = cl(lay.codes)
    out = _sentinel(torch.empty(n * h * w * k, dtype=torch.uint8, device=DEV))
    one, zero, ones_k = t1(1.0), t1(0.0), torch.ones(k, device=DEV)
    P = N.ptr
    for bit in CTL_BITS + ("EMIT_SHIFT128",):
        rc = N.lib.dlmcq_conv2d_dwpw_i8_nhwc(P(x), P(table), 0, 1, 1, P(zero), n, h, w, c, 1, P(one), None, 0, 255, N.FORM_ZEROPOINT, 0.0,
                                             P(wq2), None, P(ws2), P(one), P(ones_k), None, k, 1, P(out), P(one), None, 0, 255,
                                             N.FORM_ZEROPOINT | getattr(N, bit), 0.0, N.stream_ptr())
        torch.cuda.synchronize()
        assert rc == EINVAL, (bit, rc)
        _untouched(out, f"dwpw {bit}")
    img = torch.rand(2, 3, 8, 8, generator=gg).to(DEV)
    pad = 1
    buf = _sentinel(torch.empty(2 * 10 * 10 * 4 + 32, dtype=torch.uint8, device=DEV))
    s_img = t1(1 / 255)
    for bit in CTL_BITS:
        rc = N.lib.dlmcq_quantize_pad_nhwc4(P(img), P(buf), P(s_img), None, 2, 3, 8, 8, *img.stride(), pad, 0, 255,
                                            N.FORM_ZEROPOINT | getattr(N, bit), 0.0, N.stream_ptr())
        torch.cuda.synchronize()
        assert rc == EINVAL, (bit, rc)
        _untouched(buf, f"quantize_pad {bit}")
