"""LayerNorm rows on the GPU (include/dlmcq.h: dlmcq_layernorm_rows_f32; K.layernorm_quant).

Accuracy: against float64 from the same fp32 inputs - n = (x - mean) / sqrt(var + eps), ref = n * gamma + beta - with
        u = 2^-23 (|n gamma| + |beta| + |gamma| max_row|x| / sqrt(var + eps)):  |out - ref| <= 2 u, element by element.  The first two
        terms are the roundings of d * r * gamma + beta, the third the rounding of the mean carried through d; the factor 2 is the margin
        for second-order terms.  (A float32 emulation of the kernel's step sequence on the CPU stays within 0.85 u over these cases.)  The largest ratio seen on the device is printed (DESIGN.md 5.23 records it).
Codes:  for every quantiser the plan can emit, the codes of a launch are K.fake_quant of that launch's own fp32 output, bit for bit; a
        codes-only launch returns the same bytes; guard bytes and unrequested buffers untouched.
Independence: a row's result is that of the row launched alone.
Special values, refusals, the wrapper."""
import ctypes
import functools

import pytest
import torch

from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from test_gpu_gate import CODE_SENTINEL, DEV, SENTINEL, bits, tagged

pytestmark = pytest.mark.gpu
EPS = 1e-5
SHAPES = [(1, 4), (5, 8), (7, 260), (3, 768), (9, 2048), (1030, 64)]      # (7, 260): lanes with one and two quads; (1030, 64): more workgroups than CUs, a row tail
FAMILIES = {"n01": lambda r: r, "3_3n": lambda r: 3 + 3 * r, "100_n": lambda r: 100 + r, "1e-3n": lambda r: 1e-3 * r,
            "const_100": lambda r: torch.full_like(r, 100.0), "const_0.1": lambda r: torch.full_like(r, 0.1)}
WORST = {}


def quantisers():
    """name -> (scale, zero point / offset, lo, hi, form, g): FSPTQ's ZEROPOINT u8 with a non-zero integer zero point; QBase without and
    with needs_g (g = 0 / g > 0), s8 and u8 - what an _ActSpec of the plan's Linear layers can be."""
    t = lambda v: torch.tensor([v], device=DEV)  # noqa: E731
    return {"fsptq_zeropoint_u8": (t(0.03), t(120.0), 0, 255, N.FORM_ZEROPOINT, 0.0),
            "qbase_s8": (t(0.04), None, -128, 127, N.FORM_QBASE, 0.0), "qbase_s8_g": (t(0.04), None, -128, 127, N.FORM_QBASE, 0.02),
            "qbase_u8": (t(0.02), None, 0, 255, N.FORM_QBASE, 0.0), "qbase_u8_g": (t(0.02), None, 0, 255, N.FORM_QBASE, 0.01)}


def own_codes(out, qz):
    s, z, lo, hi, form, gq = qz
    return K.fake_quant(out, s, z, lo, hi, form, g=gq, codes="i8", want_y=False)[1].view(torch.uint8)


def raw(x, gamma, beta, qz, want_out, want_codes, eps=EPS):
    """One call of the entry point on guarded buffers: (out [M, C] or None, code bytes [M, C] or None)."""
    m, c = x.shape
    assert x.is_contiguous()
    n = m * c
    obuf = torch.full((n + 1024,), SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full((n + 1024,), CODE_SENTINEL, dtype=torch.uint8, device=DEV)
    sc, z, lo, hi, form, gq = qz if want_codes else (None, None, 0, 0, 0, 0.0)
    rc = N.lib.dlmcq_layernorm_rows_f32(N.ptr(x), N.ptr(gamma), N.ptr(beta), N.ptr(obuf) if want_out else None,
                                        N.ptr(cbuf) if want_codes else None, m, c, eps, N.ptr(sc), N.ptr(z), lo, hi, form, gq, N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    assert bool((obuf[n:] == SENTINEL).all()) and bool((cbuf[n:] == CODE_SENTINEL).all()), "guard bytes behind an output were written"
    if not want_out:
        assert bool((obuf == SENTINEL).all())
    if not want_codes:
        assert bool((cbuf == CODE_SENTINEL).all())
    return (obuf[:n].view(torch.float32).view(m, c) if want_out else None, cbuf[:n].view(m, c) if want_codes else None)


def all_calls(x, gamma, beta, names=None):
    """Every quantiser, the three calls: the codes are fake_quant of the launch's own output, the codes-only call returns the same bytes,
    the fp32 output is the same from every call.  Returns it."""
    first, none = raw(x, gamma, beta, None, True, False)
    assert none is None
    for name, qz in quantisers().items():
        if names is not None and name not in names:
            continue
        out, codes = raw(x, gamma, beta, qz, True, True)
        assert torch.equal(bits(out), bits(first)), name
        want = own_codes(out, qz)
        assert torch.equal(codes, want), f"{name}: {int((codes != want).sum())} of {codes.numel()} code bytes differ from fake_quant of the launch's own output"
        none, only = raw(x, gamma, beta, qz, False, True)
        assert none is None and torch.equal(only, codes), f"{name}: the codes-only call returns other bytes"
    return first


def reference(x, gamma, beta, eps=EPS):
    """(ref, u) in float64 from the fp32 inputs."""
    x64 = x.double()
    e64 = float(torch.tensor(eps, dtype=torch.float32).double())
    mean = x64.mean(-1, keepdim=True)
    var = ((x64 - mean) ** 2).mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + e64)
    n = (x64 - mean) * rs
    g64 = torch.ones_like(x64[0]) if gamma is None else gamma.double()
    b64 = torch.zeros_like(x64[0]) if beta is None else beta.double()
    ref = n * g64 + b64
    u = 2.0 ** -23 * ((n * g64).abs() + b64.abs() + g64.abs() * x64.abs().amax(-1, keepdim=True) * rs)
    return ref, u


def check_accuracy(x, gamma, beta, out, what):
    ref, u = reference(x, gamma, beta)
    ratio = float(((out.double() - ref).abs() / u.clamp_min(1e-300)).max())
    WORST[what] = ratio
    print(f"{what}: max |out - ref| / u = {ratio:.3f}")
    assert bool(((out.double() - ref).abs() <= 2 * u).all()), f"{what}: {ratio:.3f} u"
    return ratio


@functools.lru_cache(maxsize=None)
def case(shape, family):
    """(x, gamma, beta) on the device for one shape and row family: made once, shared, never written."""
    m, c = shape
    g = torch.Generator().manual_seed(1000 * m + c + sorted(FAMILIES).index(family))
    x = FAMILIES[family](torch.randn(m, c, generator=g)).to(torch.float32)
    return x.to(DEV), torch.randn(c, generator=g).to(DEV), torch.randn(c, generator=g).to(DEV)


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_kernel(shape, family):
    """The constant 0.1 rows are what a running sum inside the lane misses the bound on (2.500 u at 9x2048: 32 copies of 0.1f added one by
    one leave the mean 4 ulp low; 1.250 u at 3x768); the kernel's balanced tree adds them exactly."""
    x, gamma, beta = case(shape, family)
    names = None if family in ("n01", "100_n") else ("fsptq_zeropoint_u8", "qbase_s8_g")
    out = all_calls(x, gamma, beta, names)
    if family == "const_100":
        assert torch.equal(out, beta.expand_as(out)), "a constant row whose sum is exact: d = 0, out = beta"
    check_accuracy(x, gamma, beta, out, f"{shape[0]}x{shape[1]} {family}")


@pytest.mark.parametrize("shape", [(5, 8), (7, 260), (3, 768)], ids=["5x8", "7x260", "3x768"])
def test_without_gamma_and_beta(shape):
    x, gamma, beta = case(shape, "3_3n")
    for g_, b_ in ((None, None), (gamma, None), (None, beta)):
        out = all_calls(x, g_, b_, ("fsptq_zeropoint_u8", "qbase_s8_g"))
        check_accuracy(x, g_, b_, out, f"{shape} gamma={g_ is not None} beta={b_ is not None}")
    out = raw(x, None, None, None, True, False)[0]
    both = raw(x, torch.ones_like(gamma), None, None, True, False)[0]
    assert torch.equal(bits(out), bits(both)), "no gamma is gamma = 1"


def test_worst_ratio_over_all_cases():
    """The figure for DESIGN.md 5.23, printed; the bound is asserted case by case in test_kernel."""
    for shape in SHAPES:
        for family in FAMILIES:
            what = f"{shape[0]}x{shape[1]} {family}"
            if what not in WORST:
                x, gamma, beta = case(shape, family)
                ref, u = reference(x, gamma, beta)
                WORST[what] = float(((raw(x, gamma, beta, None, True, False)[0].double() - ref).abs() / u).max())
    ranked = sorted(WORST, key=WORST.get, reverse=True)
    print("LAYERNORM: largest |out - ref| / u: " + "; ".join(f"{k}: {WORST[k]:.3f}" for k in ranked[:4]) + f" (of {len(WORST)} cases)")
    assert len([k for k in WORST if k.split()[1] in FAMILIES]) == len(SHAPES) * len(FAMILIES)


@pytest.mark.parametrize("shape, row", [((7, 260), 5), ((9, 2048), 5), ((1030, 64), 1029)], ids=["7x260", "9x2048", "1030x64"])
def test_a_row_does_not_depend_on_the_launch(shape, row):
    x, gamma, beta = case(shape, "n01")
    qz = quantisers()["fsptq_zeropoint_u8"]
    out, codes = raw(x, gamma, beta, qz, True, True)
    one = x[row:row + 1].clone()
    o1, c1 = raw(one, gamma, beta, qz, True, True)
    assert torch.equal(o1, out[row:row + 1]) and torch.equal(c1, codes[row:row + 1])
    assert torch.equal(bits(o1), bits(out[row:row + 1]))


def test_nan_and_inf_rows():
    x, gamma, beta = (t.clone() for t in case((7, 260), "n01"))
    x[1, 37] = float("nan")
    x[3, 259] = float("inf")
    x[5, 0] = float("-inf")
    out = all_calls(x, gamma, beta)
    for r in (1, 3, 5):
        assert bool(torch.isnan(out[r]).all()), f"row {r}"
    clean, _ = raw(case((7, 260), "n01")[0], gamma, beta, None, True, False)
    for r in (0, 2, 4, 6):
        assert torch.equal(bits(out[r]), bits(clean[r])), "the other rows are what they were"


def test_every_refusal_leaves_the_outputs_untouched():
    x = torch.zeros(5, 64, device=DEV)
    gb = torch.ones(2, 64, device=DEV)
    obuf = torch.full((4096,), SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full((16384,), CODE_SENTINEL, dtype=torch.uint8, device=DEV)
    sc = torch.tensor([0.01], device=DEV)
    base = dict(x=x.data_ptr(), gamma=gb[0].data_ptr(), beta=gb[1].data_ptr(), out=obuf.data_ptr(), codes=cbuf.data_ptr(), m=5, c=64, eps=EPS,
                scale=sc.data_ptr(), lo=0, hi=255, form=N.FORM_ZEROPOINT)
    cases = {
        "M < 0": (dict(m=-1), -1), "C < 4": (dict(c=0), -1), "C % 4": (dict(c=62), -1), "C > 2048": (dict(c=2052), -1),
        "eps 0": (dict(eps=0.0), -1), "eps < 0": (dict(eps=-1.0), -1), "eps inf": (dict(eps=float("inf")), -1), "eps NaN": (dict(eps=float("nan")), -1),
        "both outputs NULL": (dict(out=None, codes=None), -1), "x NULL": (dict(x=None), -1), "codes without a scale": (dict(scale=None), -1),
        "lo > hi": (dict(lo=9, hi=3), -1), "unknown form": (dict(form=9), -1), "shifted emission": (dict(form=N.FORM_ZEROPOINT | N.EMIT_SHIFT128), -1),
        "FORCE_TILED": (dict(form=N.FORM_ZEROPOINT | N.FORCE_TILED), -1), "ROUTE_ONLY": (dict(form=N.FORM_ZEROPOINT | N.ROUTE_ONLY), -1),
        "PIPELINED": (dict(form=N.FORM_ZEROPOINT | N.PIPELINED), -1), "IN_CHUNK_MAJOR": (dict(form=N.FORM_ZEROPOINT | N.FP32_IN_CHUNK_MAJOR), -1),
        "OUT_CHUNK_MAJOR": (dict(form=N.FORM_ZEROPOINT | N.FP32_OUT_CHUNK_MAJOR), -1),
        "x not 16-byte aligned": (dict(x=x.data_ptr() + 4), -4), "gamma not 16-byte aligned": (dict(gamma=gb.data_ptr() + 8), -4),
        "beta not 16-byte aligned": (dict(beta=gb.data_ptr() + 4), -4), "out not 16-byte aligned": (dict(out=obuf.data_ptr() + 8), -4),
        "codes not 4-byte aligned": (dict(codes=cbuf.data_ptr() + 2), -4),
        "rows past 2^31": (dict(m=1 << 31, c=4), -2), "quads past 2^31": (dict(m=1 << 22, c=2048), -2),
    }
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731

    def call(a):
        return N.lib.dlmcq_layernorm_rows_f32(p(a["x"]), p(a["gamma"]), p(a["beta"]), p(a["out"]), p(a["codes"]), a["m"], a["c"], a["eps"],
                                              p(a["scale"]), None, a["lo"], a["hi"], a["form"], 0.0, N.stream_ptr())
    for what, (kw, rc) in cases.items():
        assert call(dict(base, **kw)) == rc, what
    assert call(dict(base, m=0)) == 0                                          # M == 0: nothing to do
    torch.cuda.synchronize()
    assert bool((obuf == SENTINEL).all()) and bool((cbuf == CODE_SENTINEL).all())


def test_wrapper():
    """K.layernorm_quant: shapes and dtypes of what it returns, the profile record, its own refusals."""
    x, gamma, beta = case((9, 2048), "n01")
    x3 = x.view(3, 3, 2048)
    ref = raw(x, gamma, beta, None, True, False)[0]
    (out, none), tags = tagged(lambda: K.layernorm_quant(x3, gamma, beta, EPS))
    assert tags == ["layernorm"] and none is None and tuple(out.shape) == (3, 3, 2048) and torch.equal(bits(out.view(9, 2048)), bits(ref))
    assert torch.equal(K.layernorm_quant(x3.transpose(0, 1), gamma, beta, EPS)[0], out.transpose(0, 1))      # a strided view: copied
    for name, qz in quantisers().items():
        sc, z, lo, hi, form, gq = qz
        em = K.EmitCodes(sc, z, lo, hi, form, gq)
        o2, codes = K.layernorm_quant(x3, gamma, beta, EPS, emit=em)
        assert codes.dtype == em.dtype and tuple(codes.shape) == (3, 3, 2048) and torch.equal(o2, out)
        assert torch.equal(codes.view(torch.uint8).view(9, 2048), own_codes(ref, qz)), name
        none, only = K.layernorm_quant(x3, gamma, beta, EPS, emit=em, want_out=False)
        assert none is None and torch.equal(only, codes)
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        K.layernorm_quant(x3, gamma, None, EPS, emit=em)
        assert K.PROFILE.records[0][:2] == ("layernorm", 9 * 2048 * (4 + 4 + 1) + 4 * 2048)
    finally:
        K.PROFILE.enabled = False
        K.PROFILE.reset()
    with pytest.raises(ValueError):
        K.layernorm_quant(x3, gamma, beta, EPS, want_out=False)
    with pytest.raises(ValueError):
        K.layernorm_quant(x3, gamma[:64], beta, EPS)
    with pytest.raises(ValueError):
        K.layernorm_quant(x3.double(), gamma, beta, EPS)
    with pytest.raises(ValueError):
        K.layernorm_quant(x3, gamma, beta, EPS, emit=K.EmitCodes(sc, None, 0, 255, N.FORM_ZEROPOINT, shift128=True))
    with pytest.raises(N.DlmcqError):
        K.layernorm_quant(torch.zeros(2, 2052, device=DEV), None, None, EPS)
    with pytest.raises(N.DlmcqError, match="no CPU fallback"):
        K.layernorm_quant(x3.cpu(), gamma, beta, EPS)


def test_the_plan_node_takes_the_torch_path_for_another_width():
    from torch import nn
    from dlmc.utils.fuse import LayerNormLayer, _ActSpec
    x, gamma, beta = case((7, 260), "n01")
    norm = nn.LayerNorm(260).to(DEV)
    with torch.no_grad():
        norm.weight.copy_(gamma)
        norm.bias.copy_(beta)
    spec = _ActSpec(torch.tensor([0.03], device=DEV), torch.tensor([120.0], device=DEV), 0, 255, N.FORM_ZEROPOINT, False)
    qz = (spec.scale, spec.zp, 0, 255, N.FORM_ZEROPOINT, 0.0)
    node = LayerNormLayer(norm, spec, True, 260)
    (out, codes), tags = tagged(lambda: node(x.view(7, 1, 260)))
    assert tags == ["layernorm"] and tuple(out.shape) == tuple(codes.shape) == (7, 1, 260) and codes.dtype == torch.uint8
    assert torch.equal(codes.view(7, 260), own_codes(out.view(7, 260), qz))
    other = LayerNormLayer(nn.LayerNorm(130).to(DEV), spec, False, 260)      # (planned for another width than it is given)
    y = x.view(14, 130)
    (out, codes), tags = tagged(lambda: other(y))
    ref = torch.nn.functional.layer_norm(y, (130,), other.norm.weight, other.norm.bias, 1e-5)
    assert "layernorm" not in tags and out is None and tuple(codes.shape) == (14, 130) and torch.equal(codes, own_codes(ref, qz))
