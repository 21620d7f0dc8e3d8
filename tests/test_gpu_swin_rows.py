"""Swin's row geometry on the GPU (csrc/swin_rows.hip; K.layernorm_window_quant, K.layernorm_merge_quant, K.window_reverse_add): rows
gathered from the token map against the same rows gathered with torch ops.  The inputs are seeded randn, independent per pixel and
channel, so a wrong pixel cannot pass.
(a) the fp32 output has the bits of K.layernorm_quant on the materialised rows; (b) |out - ref| <= 2 u against float64 from the same
fp32 inputs, u as test_gpu_layernorm.reference defines it; (c) the codes are K.fake_quant of the launch's own output
for an FSPTQ zero-point u8 and a QBase s8 quantiser; (d) a codes-only launch returns the same codes.  The reverse add is torch.equal to
`shortcut + roll(reverse(yw))` computed by torch on the device."""
import functools

import pytest
import torch

from dlmc.quantization.scalar import kernels as K
from test_gpu_layernorm import DEV, EPS, own_codes, quantisers, reference

pytestmark = pytest.mark.gpu
QUANTISERS = ("fsptq_zeropoint_u8", "qbase_s8")
# (B, Hm, Wm, ws, sy, sx, C): a non-square map with unequal shifts and a partial quad column; two quads per lane with a tail; eight
# quads per lane; Swin's own geometry
WINDOWS = [(2, 6, 9, 3, 1, 2, 8), (1, 6, 9, 3, 0, 0, 260), (2, 4, 4, 2, 1, 1, 2048), (1, 14, 14, 7, 3, 3, 128)]
# (B, Hm, Wm, C): the smallest row; 17 quads per segment (segment boundaries inside a lane stride); W = 2048
MERGES = [(2, 4, 6, 4), (1, 2, 2, 68), (1, 4, 2, 512)]
ids = lambda cases: ["x".join(map(str, c)) for c in cases]  # noqa: E731


@functools.lru_cache(maxsize=None)
def token_map(b, hm, wm, c, width, padded=False):
    """(map [B, Hm, Wm, C] - a view of rows C + 4 floats apart with `padded` -, gamma, beta [width]) on the device: made once, never written."""
    g = torch.Generator().manual_seed(b + 10 * hm + 100 * wm + 1000 * c + padded)
    buf = torch.randn(b, hm, wm, c + 4 * padded, generator=g).to(DEV)
    return buf[..., :c], torch.randn(width, generator=g).to(DEV), torch.randn(width, generator=g).to(DEV)


def check_rows(launch, rows, gamma, beta):
    """(a) - (d) of the module's docstring for `launch(emit=, want_out=)` against the materialised `rows`."""
    rows = rows.contiguous()
    out, none = launch()
    assert none is None and out.shape == rows.shape
    assert torch.equal(out, K.layernorm_quant(rows, gamma, beta, EPS)[0])
    ref, u = reference(rows, gamma, beta)
    err = (out.double() - ref).abs()
    print(f"max |out - ref| / u = {float((err / u).max()):.3f}")
    assert bool((err <= 2 * u).all())
    for name in QUANTISERS:
        qz = quantisers()[name]
        emit = K.EmitCodes(qz[0], qz[1], qz[2], qz[3], qz[4], g=qz[5])
        both, codes = launch(emit=emit)
        assert torch.equal(both, out) and torch.equal(codes.view(torch.uint8), own_codes(both, qz)), name
        none, only = launch(emit=emit, want_out=False)
        assert none is None and torch.equal(only, codes), name


@pytest.mark.parametrize("case,padded", [(c, False) for c in WINDOWS] + [(WINDOWS[0], True)], ids=ids(WINDOWS) + ["padded"])
def test_window_rows(case, padded):
    b, hm, wm, ws, sy, sx, c = case
    x, gamma, beta = token_map(b, hm, wm, c, c, padded)
    assert x.is_contiguous() != padded
    rows = torch.roll(x, (-sy, -sx), (1, 2)).reshape(b, hm // ws, ws, wm // ws, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, c)
    check_rows(lambda **kw: K.layernorm_window_quant(x, gamma, beta, EPS, ws, (sy, sx), **kw), rows, gamma, beta)


@pytest.mark.parametrize("case", MERGES, ids=ids(MERGES))
def test_merge_rows(case):
    b, hm, wm, c = case
    x, gamma, beta = token_map(b, hm, wm, c, 4 * c)
    rows = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).view(b, hm * wm // 4, 4 * c)
    check_rows(lambda **kw: K.layernorm_merge_quant(x, gamma, beta, EPS, **kw), rows, gamma, beta)


@pytest.mark.parametrize("case", WINDOWS, ids=ids(WINDOWS))
def test_reverse_add(case):
    b, hm, wm, ws, sy, sx, c = case
    shortcut = token_map(b, hm, wm, c, c)[0]
    yw = torch.randn(b * hm * wm // (ws * ws), ws * ws, c, generator=torch.Generator().manual_seed(c + sy)).to(DEV)
    back = yw.reshape(b, hm // ws, wm // ws, ws, ws, c).permute(0, 1, 3, 2, 4, 5).reshape(b, hm, wm, c)
    want = shortcut + torch.roll(back, (sy, sx), (1, 2))
    assert torch.equal(K.window_reverse_add(yw, shortcut, ws, (sy, sx)), want)


def test_reverse_add_on_padded_views():
    """A row-padded shortcut is read in place, and a row-padded `out` keeps its pad floats (the entry point itself: the wrapper allocates
    a dense `out`)."""
    from dlmc import _native as N
    b, hm, wm, ws, sy, sx, c = WINDOWS[0]
    shortcut = token_map(b, hm, wm, c, c, True)[0]
    yw = torch.randn(b * hm * wm // (ws * ws), ws * ws, c, generator=torch.Generator().manual_seed(5)).to(DEV)
    want = shortcut + K.window_reverse_torch(yw, shortcut.shape, ws, (sy, sx))
    assert torch.equal(K.window_reverse_add(yw, shortcut, ws, (sy, sx)), want)
    buf = torch.full((b, hm, wm, c + 4), 7.0, device=DEV)
    rc = N.lib.dlmcq_window_reverse_add_f32(N.ptr(yw), N.ptr(shortcut), N.ptr(buf), b, hm, wm, c, *shortcut.stride()[:3], *buf.stride()[:3],
                                            ws, sy, sx, N.stream_ptr())
    assert rc == 0 and torch.equal(buf[..., :c], want) and bool((buf[..., c:] == 7.0).all())
