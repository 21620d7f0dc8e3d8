"""The dense row mapping of the halo-tile 3x3 kernel (csrc/conv3x3_i8.hip, DENSE: a tile's 256 rows are consecutive REAL pixels, the frame's
junk positions are skipped) against the generic tiled kernel (DLMCQ_FORCE_TILED) on the whole tensor, byte for byte, on full-range codes and
weights (uint8 0 .. 255 / int8 -128 .. 127, weights -127 .. 127).  Both kernels add the same exact int32 sums into the same rounding chain.

Every case first asks the library which mapping its launch takes (DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_HALO_VARIANT | DLMCQ_ROUTE_HALO_ROWS, flag 8)
and must get the one written here: the dense mapping where the longer halo span fits the 24-piece buffers, the frame mapping elsewhere
(one-pixel-wide and 119-wide rows, stride 2) - those cases pin the fallback.  Shapes: the smallest that put an image seam, a row end and the
tile tail where the mapping can go wrong."""
import pytest
import torch

import test_conv_dispatch_host as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS = 0x200000      # DLMCQ_ROUTE_HALO_ROWS
DENSE = 8

# (N, C, H, W, K, stride, dense)
CASES = [
    (3, 64, 7, 7, 64, 1, True),        # 147 pixels: one partial tile across three images, 23 % junk skipped; the 64-wide single-buffer form
    (3, 128, 7, 7, 192, 1, True),      # two chunks, three 64-wide column blocks
    (11, 64, 7, 7, 128, 1, True),      # 539 pixels: three tiles, each across five or six images (six seams: the worst span)
    (5, 256, 14, 14, 256, 1, True),    # 980 pixels: a 256-row tile spans more than one image; four chunks, two column blocks
    (2, 64, 6, 10, 128, 1, True),      # H != W
    (1, 64, 15, 17, 128, 1, True),     # M = 255: one below the tile height
    (1, 64, 27, 19, 128, 1, True),     # M = 513: one above twice the tile height - a last tile of one row
    (3, 128, 11, 31, 128, 1, True),    # M = 1023: one below four tiles
    (2, 64, 28, 28, 64, 1, True),      # 28^2: the widest ResNet size that takes the mapping (23 pieces)
    (2, 64, 56, 56, 128, 1, False),    # 56^2: 28 pieces - the frame mapping
    (4, 64, 9, 1, 128, 1, False),      # one-pixel-wide rows: every other frame position is junk, the span does not fit
    (1, 64, 3, 119, 128, 1, False),    # 119-wide rows, one image, tiles inside a row: the 32-piece buffers keep the frame mapping
    (3, 128, 14, 14, 128, 2, False),   # stride 2, 14^2 -> 7^2
    (3, 64, 8, 12, 64, 2, False),      # stride 2, 8 x 12 -> 4 x 6
]


def _ids(c):
    return f"n{c[0]}_c{c[1]}_{c[2]}x{c[3]}_k{c[4]}_s{c[5]}"


@pytest.mark.parametrize("unsigned", [True, False], ids=["u8", "i8"])
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_dense_rows_are_the_tiled_kernel_byte_for_byte(case, unsigned):
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    n, c, h, w, k, stride, dense = case
    # which mapping the launch takes, asked of the library's own dispatch (placeholder pointers, nothing launched)
    q = dict(N=n, H=h, W=w, C=c, K=k, R=3, S=3, stride=stride, pad=1, uns=int(unsigned))
    if not unsigned:
        q.update(q_zp=D.P, q_lo=-128, q_hi=127)
    rc = D.call(N.lib, "fused", dict(q, ctl=D.HALO_VARIANT | ROWS))
    assert rc >> 25 == 1 and bool(rc & DENSE) == dense, hex(rc)
    assert D.call(N.lib, "fused", dict(q, ctl=D.HALO_VARIANT)) == rc & ~DENSE          # without the bit: the record as it always was
    g = torch.Generator(device=DEV).manual_seed(1000 * n + 10 * h + w + k + c + stride)
    lo, hi = (0, 256) if unsigned else (-128, 128)
    codes = torch.randint(lo, hi, (n, c, h, w), generator=g, device=DEV, dtype=torch.int16).to(torch.uint8 if unsigned else torch.int8)
    codes = codes.contiguous(memory_format=torch.channels_last)
    wq = torch.randint(-127, 128, (k, 3, 3, c), generator=g, device=DEV, dtype=torch.int8)
    wq[0, 0, 0, 0], wq[-1, -1, -1, -1] = -127, 127
    wsum = wq.to(torch.int32).sum(dim=(1, 2, 3)).to(torch.int32).contiguous()
    s_w = (torch.rand(k, generator=g, device=DEV) * 2e-4 + 5e-5).contiguous()
    bias = (torch.randn(k, generator=g, device=DEV) * 0.5).contiguous()
    zp = 131.0 if unsigned else -3.0          # a border that is not the zero byte
    s_in, in_zp = torch.full((1,), 0.021, device=DEV), torch.full((1,), zp, device=DEV)
    if unsigned:      # the plain unsigned-byte quantiser (the PLAIN instantiations)
        emit = K.EmitCodes(torch.full((1,), 0.004, device=DEV), None, 0, 255, N.FORM_ZEROPOINT)
    else:             # a signed range with a zero point
        emit = K.EmitCodes(torch.full((1,), 0.004, device=DEV), torch.full((1,), -40.0, device=DEV), -128, 127, N.FORM_ZEROPOINT)
    relu = unsigned

    def run(**kw):
        K.PROFILE.reset()
        K.PROFILE.enabled = True
        try:
            _, got = K.conv2d_i8(codes, wq, wsum, bias, s_in, in_zp, s_w, stride=stride, padding=1, relu=relu, emit=emit, want_out=False, **kw)
        finally:
            K.PROFILE.enabled = False
        tag = K.PROFILE.records[-1][0]
        K.PROFILE.reset()
        return got, tag
    got, tag = run()
    assert tag == "conv3x3_halo", tag
    tiled, tag = run(force_tiled=True)
    assert tag == "conv_i8", tag
    assert got.shape == (n, k, h // stride, w // stride)
    bad = got != tiled
    assert not bool(bad.any()), f"{int(bad.sum())} of {got.numel()} codes differ; first pixel (n, k, y, x) {bad.nonzero()[0].tolist()}"
    # the comparison means something: both ends of the code range and the values between occur
    v = got.to(torch.int16) if unsigned else got.view(torch.int8).to(torch.int16)
    assert int(v.min()) == emit.lo and int(v.max()) == emit.hi and v.unique().numel() > 100
