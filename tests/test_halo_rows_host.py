"""Which ROW MAPPING a conv3x3_halo_i8_kernel launch takes, asked from outside (no GPU): DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_HALO_VARIANT |
DLMCQ_ROUTE_HALO_ROWS adds flag 8 (DENSE: a tile's rows are real pixels only) to the halo answer.  Without the new bit every answer is what it
was; the bit alone, or without DLMCQ_ROUTE_HALO_VARIANT, is refused; the dense instantiations are a subset of the 40 records.  The expected
mapping is computed here from the sizing rule of DESIGN.md 5.5 (worst span of 256 consecutive pixels), not read back from the library."""
import ctypes

import halo_variant_cases as H
import test_conv_dispatch_host as D

ROWS, DENSE = 0x200000, 8


def _pieces_dense(h, w):
    return (256 + -(-255 // w) + (w + 1) * -(-255 // (h * w)) + 2 * (w + 1) + 2 + 15) // 16


def _want_dense(h, w, stride):
    return stride == 1 and H.pieces(1, w) <= 24 and _pieces_dense(h, w) <= 24


def test_the_sizing_rule_is_the_worst_span_over_every_tile_start():
    for h, w in ((7, 7), (14, 14), (28, 28), (56, 56), (6, 10), (7, 9), (1, 1), (9, 1), (3, 62)):
        q = lambda p: p + p // w + (p // (h * w)) * (w + 1)
        worst = max(q(p0 + 255) - q(p0) + 2 * (w + 1) + 3 for p0 in range(2 * h * w + 256))
        assert (worst + 15) // 16 <= _pieces_dense(h, w), (h, w)
    assert [_pieces_dense(s, s) for s in (7, 14, 28, 56)] == [23, 22, 23, 28]


def test_the_answer_names_the_mapping_and_nothing_else_changes():
    from dlmc import _native as N
    assert (N.ROUTE_HALO_ROWS, N.HV_DENSE) == (ROWS, DENSE)
    # ResNet-50's 3x3 sizes: 28^2, 14^2, 7^2 dense; 56^2 and every stride-2 layer on the frame mapping
    for c, hw, stride in ((64, 56, 1), (128, 56, 2), (128, 28, 1), (256, 28, 2), (256, 14, 1), (512, 14, 2), (512, 7, 1)):
        a = dict(N=2, H=hw, W=hw, C=c, K=c, R=3, S=3, stride=stride, pad=1)
        plain = D.call(N.lib, "fused", dict(a, ctl=D.HALO_VARIANT))
        rows = D.call(N.lib, "fused", dict(a, ctl=D.HALO_VARIANT | ROWS))
        assert plain >> 25 == 1 and not plain & DENSE and rows & ~DENSE == plain, (c, hw, stride)
        assert bool(rows & DENSE) == (stride == 1 and hw <= 28) == _want_dense(hw // stride, hw // stride, stride), (c, hw, stride)
    # every case of the variant tests: the record is untouched by the bit, the flag follows the sizing rule
    for c in H.CASES:
        a = c.route_args()
        rc = D.call(N.lib, "fused", dict(a, ctl=a["ctl"] | ROWS))
        assert rc & ~DENSE == D.call(N.lib, "fused", a), c.cid
        p, q = c.out_hw()
        assert bool(rc & DENSE) == (not c.pipelined and _want_dense(p, q, c.geo["stride"])), c.cid
    # the bit is a question about the halo kernel's launch: alone, without the variant query or without DLMCQ_ROUTE_ONLY it is refused
    geo = dict(N=2, H=14, W=14, C=64, K=128, R=3, S=3, pad=1)
    assert D.call(N.lib, "fused", dict(geo, ctl=ROWS)) == D.EINVAL
    assert H.launch(N.lib, "fused", dict(geo, N=0, ctl=ROWS)) == D.EINVAL and H.launch(N.lib, "fused", dict(geo, N=0, ctl=ROWS | D.HALO_VARIANT)) == D.EINVAL
    # another kernel's answer is what it is without the bit
    assert D.call(N.lib, "fused", dict(geo, ctl=D.HALO_VARIANT | ROWS | D.FORCE_TILED)) == D.ROUTES["tiled"]
    assert D.call(N.lib, "fused", dict(geo, R=1, S=1, pad=0, ctl=D.HALO_VARIANT | ROWS)) == D.call(N.lib, "fused", dict(geo, R=1, S=1, pad=0))


def test_the_dense_instantiations_are_twelve_of_the_forty():
    from dlmc import _native as N
    fn = N.experimental("dlmcq_x_conv3x3_variant_table", [ctypes.c_int, ctypes.POINTER(ctypes.c_int32), ctypes.c_int])
    n = fn(0x100, None, 0)
    answers = (ctypes.c_int32 * n)()
    assert n == 12 and fn(0x100, answers, n) == n
    assert all(int(a) & DENSE for a in answers)
    recs = [N.decode_halo_variant(int(a) & ~DENSE) for a in answers]
    assert len(set(recs)) == 12 and set(recs) <= set(H.HALO_RECORDS)
    assert {r[1:5] for r in recs} == {(128, False, 24, 2), (64, False, 24, 1), (64, False, 24, 2)}
