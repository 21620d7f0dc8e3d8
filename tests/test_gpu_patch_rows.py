"""A vision transformer's patch rows on the GPU (include/dlmcq.h: dlmcq_patch_rows_f32; K.patch_rows_quant).

The kernel moves and quantises, nothing else, so everything is exact: the fp32 rows are the bits of torch's reshape / permute / reshape,
the codes are K.fake_quant of that tensor, byte for byte, for the five quantisers of test_gpu_layernorm.py - at the shapes at which each
index computation can go wrong (one and several patches per line and per image, gh != gw, 4 channels, one real strip of 224 / 16 / 3:
10.5 KiB of LDS, 16-byte pieces; 768-byte strips that are copied out in 16-byte pieces and one of 64), with ordinary values, with NaN,
infinities, -0 and quantiser ties, and read through the strides of a view of a NaN-filled parent.  The outputs are views of
pattern-filled parents whose fill must be intact outside.  Then: a call with one output alone, every refusal of the entry point, the
wrapper and its torch restatement."""
import ctypes
import functools

import pytest
import torch

from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from test_gpu_gate import CODE_SENTINEL, DEV, SENTINEL, bits, tagged
from test_gpu_layernorm import own_codes, quantisers

pytestmark = pytest.mark.gpu
SHAPES = [(2, 3, 32, 32, 8), (3, 3, 32, 32, 16), (2, 4, 16, 48, 4), (1, 3, 224, 224, 16), (5, 1, 8, 8, 8)]      # (B, C, H, W, p)
IDS = ["x".join(map(str, s)) for s in SHAPES]
GUARD = 1024      # elements of fill in front of and behind an output (a multiple of 16 bytes: the view stays aligned)


def rearranged(img, p):
    """torch's rearrangement, dense: [B gh gw, p p C]."""
    rows = K.patch_rows_torch(img, p)
    return rows.reshape(-1, rows.shape[-1]).contiguous()


@functools.lru_cache(maxsize=None)
def image(shape, kind):
    """The image batch of one case on the device: made once, shared, never written.  `special`: NaN, infinities, -0 and, for every
    quantiser, values on its rounding ties ((k + 0.5) * scale) sprinkled over randn * 3.  `strided`: the same values as `randn` seen
    through `parent[1:, 1:1 + C]` of a NaN-filled parent with one image and two channels more (batch and channel strides that are not
    a dense tensor's)."""
    b, c, h, w, p = shape
    g = torch.Generator().manual_seed(17 * b + c + h + w + p)
    x = (torch.randn(b, c, h, w, generator=g) * 3).to(torch.float32)
    if kind == "special":
        flat = x.view(-1)
        n = flat.numel()
        scales = sorted({float(q[0]) for q in quantisers().values()})
        for i, s in enumerate(scales):
            idx = torch.arange(3 + i, n, 11)
            k = torch.randint(-140, 140, (idx.numel(),), generator=g).float()
            flat[idx] = ((k + 0.5) * s).to(torch.float32)
        for i, v in enumerate((float("nan"), float("inf"), float("-inf"), -0.0, 1e30, -1e30, 1e-40)):
            flat[torch.arange(i, n, 29 + i)] = v
    x = x.to(DEV)
    if kind == "strided":
        parent = torch.full((b + 1, c + 2, h, w), float("nan"), device=DEV)
        view = parent[1:, 1:1 + c]
        view.copy_(x)
        assert view.stride() == ((c + 2) * h * w, h * w, w, 1) and view.data_ptr() != parent.data_ptr()
        return view
    return x


def raw(img, p, qz, want_out, want_codes):
    """One call of the entry point, the outputs views (at element GUARD) of pattern-filled parents whose fill is checked everywhere
    outside: (rows [M, K] or None, code bytes [M, K] or None)."""
    b, c, h, w = img.shape
    gh, gw = h // p, w // p
    m, k = b * gh * gw, p * p * c
    n = m * k
    obuf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full((n + 2 * GUARD,), CODE_SENTINEL, dtype=torch.uint8, device=DEV)
    out, codes = obuf[GUARD:GUARD + n], cbuf[GUARD:GUARD + n]
    sc, z, lo, hi, form, gq = qz if want_codes else (None, None, 0, 0, 0, 0.0)
    rc = N.lib.dlmcq_patch_rows_f32(N.ptr(img), N.ptr(out) if want_out else None, N.ptr(codes) if want_codes else None, b, c, gh, gw, p,
                                    *img.stride()[:3], N.ptr(sc), N.ptr(z), lo, hi, form, gq, N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    for buf, fill in ((obuf, SENTINEL), (cbuf, CODE_SENTINEL)):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), "the fill around an output was written"
    if not want_out:
        assert bool((obuf == SENTINEL).all())
    if not want_codes:
        assert bool((cbuf == CODE_SENTINEL).all())
    return (out.view(torch.float32).view(m, k) if want_out else None, codes.view(m, k) if want_codes else None)


@pytest.mark.parametrize("kind", ["randn", "special", "strided"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kernel(shape, kind):
    img, p = image(shape, kind), shape[4]
    ref = rearranged(img, p)
    first, none = raw(img, p, None, True, False)                      # codes = NULL
    assert none is None and torch.equal(bits(first), bits(ref)), f"{int((bits(first) != bits(ref)).sum())} of {ref.numel()} fp32 words differ"
    for name, qz in quantisers().items():
        want = own_codes(ref, qz)
        out, codes = raw(img, p, qz, True, True)
        assert torch.equal(bits(out), bits(ref)), name
        assert torch.equal(codes, want), f"{name}: {int((codes != want).sum())} of {codes.numel()} code bytes differ from fake_quant of the rearrangement"
        none, only = raw(img, p, qz, False, True)                     # out = NULL
        assert none is None and torch.equal(only, want), f"{name}: the codes-only call returns other bytes"


def test_special_values_are_where_they_belong():
    """(the special image really holds them, and the rows hold them at the rearranged places: NaN compares by its bits)"""
    img = image(SHAPES[0], "special")
    assert bool(torch.isnan(img).any()) and bool(torch.isinf(img).any()) and bool(((img == 0) & torch.signbit(img)).any())
    out = raw(img, 8, None, True, False)[0]
    assert int(torch.isnan(out).sum()) == int(torch.isnan(img).sum()) and int(torch.signbit(out).sum()) == int(torch.signbit(img).sum())


def test_a_row_is_its_patch():
    """One element, by the header's formula, without torch's permute: row (b gh + gy) gw + gx, column (py p + px) C + c."""
    b, c, h, w, p = SHAPES[2]
    img = image(SHAPES[2], "randn")
    out = raw(img, p, None, True, False)[0]
    gh, gw = h // p, w // p
    for (bi, ci, y, x) in ((0, 0, 0, 0), (1, 3, 15, 47), (1, 2, 5, 22), (0, 1, 12, 3)):
        gy, py, gx, px = y // p, y % p, x // p, x % p
        assert float(out[(bi * gh + gy) * gw + gx, (py * p + px) * c + ci]) == float(img[bi, ci, y, x])


def test_every_refusal_leaves_the_outputs_untouched():
    img = torch.zeros(2, 3, 32, 32, device=DEV)
    obuf = torch.full((8192,), SENTINEL, dtype=torch.int32, device=DEV)
    cbuf = torch.full((8192,), CODE_SENTINEL, dtype=torch.uint8, device=DEV)
    sc = torch.tensor([0.01], device=DEV)
    base = dict(img=img.data_ptr(), out=obuf.data_ptr(), codes=cbuf.data_ptr(), b=2, c=3, gh=4, gw=4, p=8, sb=3072, sc=1024, sh=32,
                scale=sc.data_ptr(), lo=0, hi=255, form=N.FORM_ZEROPOINT)
    cases = {
        "B < 0": (dict(b=-1), -1), "C < 1": (dict(c=0), -1), "gh < 1": (dict(gh=0), -1), "gw < 1": (dict(gw=0), -1), "p < 1": (dict(p=0), -1),
        "p % 4": (dict(p=6), -1), "sb % 4": (dict(sb=3074), -1), "sc % 4": (dict(sc=1022), -1), "sh % 4": (dict(sh=34), -1),
        "a strip past the LDS": (dict(gw=86, p=16), -1), "both outputs NULL": (dict(out=None, codes=None), -1), "img NULL": (dict(img=None), -1),
        "codes without a scale": (dict(scale=None), -1), "lo > hi": (dict(lo=9, hi=3), -1), "unknown form": (dict(form=9), -1),
        "shifted emission": (dict(form=N.FORM_ZEROPOINT | N.EMIT_SHIFT128), -1), "FORCE_TILED": (dict(form=N.FORM_ZEROPOINT | N.FORCE_TILED), -1),
        "ROUTE_ONLY": (dict(form=N.FORM_ZEROPOINT | N.ROUTE_ONLY), -1), "PIPELINED": (dict(form=N.FORM_ZEROPOINT | N.PIPELINED), -1),
        "IN_CHUNK_MAJOR": (dict(form=N.FORM_ZEROPOINT | N.FP32_IN_CHUNK_MAJOR), -1),
        "OUT_CHUNK_MAJOR": (dict(form=N.FORM_ZEROPOINT | N.FP32_OUT_CHUNK_MAJOR), -1),
        "img not 16-byte aligned": (dict(img=img.data_ptr() + 4), -4), "out not 16-byte aligned": (dict(out=obuf.data_ptr() + 8), -4),
        "codes not 16-byte aligned": (dict(codes=cbuf.data_ptr() + 4), -4),
        "B past 2^31": (dict(b=1 << 31), -2), "strips past 2^31": (dict(b=1 << 16, gh=1 << 15), -2), "rows past 2^31": (dict(b=1 << 16, gh=1 << 14, gw=2), -2),
    }
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731

    def call(a):
        return N.lib.dlmcq_patch_rows_f32(p(a["img"]), p(a["out"]), p(a["codes"]), a["b"], a["c"], a["gh"], a["gw"], a["p"], a["sb"], a["sc"],
                                          a["sh"], p(a["scale"]), None, a["lo"], a["hi"], a["form"], 0.0, N.stream_ptr())
    for what, (kw, rc) in cases.items():
        assert call(dict(base, **kw)) == rc, what
    assert call(dict(base, b=0)) == 0                                          # B == 0: nothing to do
    torch.cuda.synchronize()
    assert bool((obuf == SENTINEL).all()) and bool((cbuf == CODE_SENTINEL).all())


def test_wrapper():
    """K.patch_rows_quant: shapes and dtypes of what it returns, the profile record, the torch restatement, its own refusals."""
    shape = SHAPES[0]
    b, c, h, w, p = shape
    img = image(shape, "randn")
    ref = rearranged(img, p)
    (out, none), tags = tagged(lambda: K.patch_rows_quant(img, p))
    assert tags == ["patch_rows"] and none is None and tuple(out.shape) == (b, 16, 192) and torch.equal(out.view(-1, 192), ref)
    strided = image(shape, "strided")
    cl = img.contiguous(memory_format=torch.channels_last)
    assert K.patch_rows_view(img, p) and K.patch_rows_view(strided, p) and not K.patch_rows_view(cl, p) and not K.patch_rows_view(img, 2)
    assert not K.patch_rows_view(img.double(), p) and not K.patch_rows_view(img.cpu(), p) and not K.patch_rows_view(img[:, :, :, 1:], p)
    for name, qz in quantisers().items():
        sc, z, lo, hi, form, gq = qz
        em = K.EmitCodes(sc, z, lo, hi, form, gq)
        o2, codes = K.patch_rows_quant(img, p, emit=em)
        assert codes.dtype == em.dtype and tuple(codes.shape) == (b, 16, 192) and torch.equal(o2, out)
        assert torch.equal(codes.view(torch.uint8).view(-1, 192), own_codes(ref, qz)), name
        none, only = K.patch_rows_quant(img, p, emit=em, want_out=False)
        assert none is None and torch.equal(only, codes)
        (o3, c3), tags = tagged(lambda: K.patch_rows_quant(strided, p, emit=em))
        assert tags == ["patch_rows"] and torch.equal(o3, out) and torch.equal(c3, codes)
        # a channels_last batch (unit stride along the channels, not along a line): the torch restatement, the same values
        (o4, c4), tags = tagged(lambda: K.patch_rows_quant(cl, p, emit=em))
        assert "patch_rows" not in tags and tags.count("fq_tensor") == 1 and torch.equal(o4, out) and torch.equal(c4, codes) and c4.dtype == em.dtype
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        K.patch_rows_quant(img, p, emit=em, want_out=False)
        assert K.PROFILE.records[0][:2] == ("patch_rows", img.numel() * 5)
    finally:
        K.PROFILE.enabled = False
        K.PROFILE.reset()
    with pytest.raises(ValueError):
        K.patch_rows_quant(img, p, want_out=False)
    with pytest.raises(ValueError):
        K.patch_rows_quant(img, 12)
    with pytest.raises(ValueError):
        K.patch_rows_quant(img[0], p)
    with pytest.raises(ValueError):
        K.patch_rows_quant(img, p, emit=K.EmitCodes(sc, None, 0, 255, N.FORM_ZEROPOINT, shift128=True))


def test_the_plan_node_takes_the_torch_path_for_another_shape():
    from dlmc.utils.fuse import PatchRowsLayer, _ActSpec, _PatchRows
    import torch.fx as fx
    spec = _ActSpec(torch.tensor([0.03], device=DEV), torch.tensor([120.0], device=DEV), 0, 255, N.FORM_ZEROPOINT, False)
    qz = (spec.scale, spec.zp, 0, 255, N.FORM_ZEROPOINT, 0.0)
    g = fx.Graph()
    nd = g.placeholder("img")
    node = PatchRowsLayer(_PatchRows(nd, (nd,), 3, 4, 4, 8, spec, (), True))
    img = image(SHAPES[0], "randn")
    ref = rearranged(img, 8)
    (out, codes), tags = tagged(lambda: node(img))
    assert tags == ["patch_rows"] and tuple(out.shape) == tuple(codes.shape) == (2, 16, 192) and codes.dtype == torch.uint8
    assert torch.equal(out.view(-1, 192), ref) and torch.equal(codes.view(-1, 192), own_codes(ref, qz))
    flat = img.reshape(2 * 3, 32 * 32)      # the same elements in another shape: the graph's own ops
    (o2, c2), tags = tagged(lambda: node(flat))
    assert "patch_rows" not in tags and torch.equal(o2, out) and torch.equal(c2, codes)
