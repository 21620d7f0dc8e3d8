"""A transformer's token tensor on the GPU (include/dlmcq.h: dlmcq_tokens_assemble_f32; K.assemble_tokens).

One IEEE add per element, so everything is exact: the result is torch.equal (and equal in its bits where NaN occurs) to
`torch.cat((cls.expand(B, -1, -1), e), 1) + pos` on the device - at one token of one quad, at an odd row count, at ViT-S/16's 196 x 384
and at rows of 2048 (more than one workgroup per row pair); `e` read through a row stride; `out` written through its own strides into a
pattern-filled parent whose fill must be intact outside; NaN and infinite rows as torch's.  Then every refusal and the wrapper."""
import ctypes
import functools

import pytest
import torch

from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from test_gpu_gate import DEV, SENTINEL, bits, tagged

pytestmark = pytest.mark.gpu
SHAPES = [(1, 1, 4), (3, 16, 64), (2, 196, 384), (2, 5, 2048)]      # (B, T, C)
IDS = ["x".join(map(str, s)) for s in SHAPES]
GUARD = 1024


def torch_tokens(e, cls, pos):
    return torch.cat((cls.expand(e.shape[0], -1, -1), e), 1) + pos


@functools.lru_cache(maxsize=None)
def case(shape, special=False):
    """(e, cls, pos) on the device: made once, shared, never written.  `e` is a column slice of a wider NaN-filled parent: its rows
    are C + 8 floats apart.  `special`: NaN and infinite rows (and an inf + -inf pair, a NaN of the add's own making)."""
    b, t, c = shape
    g = torch.Generator().manual_seed(31 * b + t + c)
    parent = torch.full((b, t, c + 8), float("nan"))
    parent[:, :, :c] = torch.randn(b, t, c, generator=g)
    cls, pos = torch.randn(1, 1, c, generator=g), torch.randn(1, t + 1, c, generator=g)
    if special:
        parent[0, 0, :c] = float("nan")
        parent[b - 1, t - 1, :c] = float("inf")
        parent[0, t // 2, 0] = float("-inf")
        pos[0, 1 + t // 2, 0] = float("inf")
        pos[0, 0, c - 1] = float("nan")
        cls[0, 0, 0] = -0.0
        pos[0, 0, 0] = -0.0
    parent = parent.to(DEV)
    return parent[:, :, :c], cls.to(DEV), pos.to(DEV)


def raw(e, cls, pos, o_pad=0, b_pad=0):
    """One call of the entry point, `out` a view (rows C + o_pad apart, images b_pad further apart) of a pattern-filled parent whose
    fill is checked everywhere outside the rows."""
    b, t, c = e.shape
    ost = c + o_pad
    osb = (t + 1) * ost + b_pad
    buf = torch.full((b * osb + 2 * GUARD,), SENTINEL, dtype=torch.int32, device=DEV)
    view = buf[GUARD:GUARD + b * osb].view(b, osb)[:, :(t + 1) * ost].view(b, t + 1, ost)
    rc = N.lib.dlmcq_tokens_assemble_f32(N.ptr(e), N.ptr(cls), N.ptr(pos), ctypes.c_void_p(view.data_ptr()), b, t, c, e.stride(1), osb, ost,
                                         N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    out = view[:, :, :c].contiguous().view(torch.float32)
    touched = torch.zeros_like(buf, dtype=torch.bool)
    touched[GUARD:GUARD + b * osb].view(b, osb)[:, :(t + 1) * ost].view(b, t + 1, ost)[:, :, :c] = True
    assert bool((buf[~touched] == SENTINEL).all()), "the fill outside the rows was written"
    return out


@pytest.mark.parametrize("special", [False, True], ids=["randn", "nan_inf"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kernel(shape, special):
    e, cls, pos = case(shape, special)
    assert e.stride(1) == shape[2] + 8 and not (e.is_contiguous() and shape[1] > 1)
    ref = torch_tokens(e, cls, pos)
    dense = raw(e, cls, pos)
    assert torch.equal(bits(dense), bits(ref)), f"{int((bits(dense) != bits(ref)).sum())} of {ref.numel()} words differ"
    assert torch.equal(bits(dense), bits(pos + torch.cat((cls.expand(shape[0], -1, -1), e), 1))), "the other operand order"
    strided = raw(e, cls, pos, o_pad=4, b_pad=12)
    assert torch.equal(bits(strided), bits(ref))
    if special:
        assert bool(torch.isnan(ref).any()) and bool(torch.isinf(ref).any())
    else:
        assert torch.equal(dense, ref)
    assert torch.equal(bits(raw(e.contiguous(), cls, pos)), bits(ref))      # dense rows of e


def test_every_refusal_leaves_the_output_untouched():
    e, cls, pos = (t.contiguous() for t in case((3, 16, 64)))
    obuf = torch.full((8192,), SENTINEL, dtype=torch.int32, device=DEV)
    base = dict(e=e.data_ptr(), cls=cls.data_ptr(), pos=pos.data_ptr(), out=obuf.data_ptr(), b=3, t=16, c=64, es=64, osb=17 * 64, ost=64)
    cases = {
        "B < 0": (dict(b=-1), -1), "T < 1": (dict(t=0), -1), "C < 4": (dict(c=0), -1), "C % 4": (dict(c=62), -1), "e stride < C": (dict(es=60), -1),
        "e stride % 4": (dict(es=66), -1), "out row stride < C": (dict(ost=60), -1), "out row stride % 4": (dict(ost=66, osb=17 * 66), -1),
        "out image stride % 4": (dict(osb=17 * 64 + 2), -1), "images overlap": (dict(osb=16 * 64), -1),
        "e NULL": (dict(e=None), -1), "cls NULL": (dict(cls=None), -1), "pos NULL": (dict(pos=None), -1), "out NULL": (dict(out=None), -1),
        "e not 16-byte aligned": (dict(e=e.data_ptr() + 4), -4), "cls not 16-byte aligned": (dict(cls=cls.data_ptr() + 8), -4),
        "pos not 16-byte aligned": (dict(pos=pos.data_ptr() + 4), -4), "out not 16-byte aligned": (dict(out=obuf.data_ptr() + 8), -4),
        "B past 2^31": (dict(b=1 << 31), -2), "rows past 2^31": (dict(b=1 << 27), -2), "quads past 2^31": (dict(b=1 << 23), -2),
    }
    p = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731

    def call(a):
        return N.lib.dlmcq_tokens_assemble_f32(p(a["e"]), p(a["cls"]), p(a["pos"]), p(a["out"]), a["b"], a["t"], a["c"], a["es"], a["osb"],
                                               a["ost"], N.stream_ptr())
    for what, (kw, rc) in cases.items():
        assert call(dict(base, **kw)) == rc, what
    assert call(dict(base, b=0)) == 0                                          # B == 0: nothing to do
    torch.cuda.synchronize()
    assert bool((obuf == SENTINEL).all())


def test_wrapper():
    """K.assemble_tokens: what it returns, the profile record, the inputs that take the torch expression."""
    e, cls, pos = case((2, 196, 384))
    ref = torch_tokens(e, cls, pos)
    out, tags = tagged(lambda: K.assemble_tokens(e, cls, pos))
    assert tags == ["tokens"] and tuple(out.shape) == (2, 197, 384) and out.is_contiguous() and torch.equal(out, ref)
    assert torch.equal(K.assemble_tokens(e.contiguous(), cls, pos), ref)
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        K.assemble_tokens(e, cls, pos)
        assert K.PROFILE.records[0][:2] == ("tokens", 4 * 384 * (2 * 196 + 197 + 1 + 2 * 197))
    finally:
        K.PROFILE.enabled = False
        K.PROFILE.reset()
    # not taken by the kernel: the torch expression itself, the same values
    longer = torch.cat((pos, pos), 1)
    others = {"a transposed e": (e.transpose(0, 1).contiguous().transpose(0, 1), cls, pos), "float64": (e.double(), cls.double(), pos.double()),
              "a sliced pos of a longer one is dense and taken": None, "C % 4": (e[:, :, :382], cls[:, :, :382], pos[:, :, :382]),
              "e misaligned": (e.contiguous()[:, :, 1:373], cls[:, :, :372], pos[:, :, :372])}
    for what, args in others.items():
        if args is None:
            got, tags = tagged(lambda: K.assemble_tokens(e, cls, longer[:, :197]))
            assert tags == ["tokens"] and torch.equal(got, ref), what
            continue
        assert not K.tokens_view(*args), what
        got, tags = tagged(lambda: K.assemble_tokens(*args))
        assert tags == [] and torch.equal(got, torch_tokens(*args)), what
    assert torch.equal(K.assemble_tokens(e.cpu(), cls.cpu(), pos.cpu()), ref.cpu())
