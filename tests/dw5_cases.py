"""The calls that reach every instantiation of the 5 x 5 depthwise kernel - csrc/conv_dw5_i8.hip (DW5_TABLE, 6: FAST 0 / 1 / 2 x R6): ONE table
for tests/test_dw5_host.py (which record does the entry point pick: DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_DW_VARIANT on placeholder pointers, no GPU)
and tests/test_gpu_dw5.py (the same calls launched; compared with the generic kernel and with an exact float64 reference).  TEST
INFRASTRUCTURE ONLY.

A record is ("dw5", FAST, R6), as dlmc._native.decode_dw5_variant answers.  The cases are tests/dw_variant_cases.py's `Case` records and
walk their operands the way that module does, by case index i: the input codes and zero point (uint8 / 0, uint8 above 128, int8 not 0,
uint8 below 128, int8 / 0), plain quantisers for FAST 1 / 2 and the open ones (zero point, signed range, with fp32, fp32 alone) for FAST 0,
ReLU6 on the R6 records and ReLU / none in turn elsewhere, a null bias in case 1, symmetric and asymmetric weights in turn where FAST does
not fix them, case 0 of every record at the consumer scale 2^-5 where the upper clamp occurs.

Geometries - the kernel handles ONE output pixel per thread, 16 channels wide, the filter's rows in a loop:
  * maps smaller than, equal to and just larger than the filter: 1x1 (only the centre tap inside), 2x3, 4x4, 5x5, 6x7, 9x9;
  * stride 2 on 7, 8 and 9 in either axis: the last output pixel's window ends inside, on and past the border;
  * output widths 1, 2, 3 and 5 (one pixel per thread: no run length to straddle);
  * channels 16 (one group), 48 (C % 64 != 0), 64, and 2048 on a 3x3 map (the full LDS table, above 64 KB); batch 1 and 3 (the 1x1 map at batch 3
    and 64 channels: enough values for the reference's own conditions);
  * one grid-stride case just past the grid cap of 2048 workgroups of 256 threads;
  * one full-range case per record (FULL_RANGE): every code at an end of the byte range against weights of +-127 / -128 in all 25 taps."""
from dw_variant_cases import _INPUT, _OPEN, _PLAIN, Case, _act, _geo

import test_dw_stem_refusals_host as D
from dlmc._native import ROUTE_DW_VARIANT, ROUTE_ONLY, decode_dw5_variant      # include/dlmcq.h

RECORDS = [("dw5", 0, False), ("dw5", 1, False), ("dw5", 2, False), ("dw5", 0, True), ("dw5", 1, True), ("dw5", 2, True)]     # by hand
assert len(RECORDS) == len(set(RECORDS)) == 6
GRID_CAP, BLOCK = 2048, 256          # csrc/conv_dw5_i8.hip: DW5_GRID, DLMCQ_BLOCK

_DW5 = "x w out bias s_in zp_in s_w w_off N H W C stride pad uns".split()
ENTRY = _DW5 + D._Q + ["stream"]     # dlmcq_conv2d_dw5_i8_nhwc: every argument by name, in the ABI's order
BASE = dict(D._QB, x=D.P, w=D.P, out=0, bias=0, s_in=D.P, zp_in=0, s_w=D.P, w_off=0, N=1, H=16, W=16, C=64, stride=1, pad=2, uns=1)


def call(lib, case):
    """D.call for the new entry point (`case`: overrides of BASE; R, S of a depthwise case are dropped)."""
    import ctypes
    a = dict(BASE, **{k: v for k, v in case.items() if k not in ("R", "S")})
    fn = lib.dlmcq_conv2d_dw5_i8_nhwc
    assert len(ENTRY) == len(fn.argtypes)
    return int(fn(*[(a[name] or None) if typ is ctypes.c_void_p else a[name] for name, typ in zip(ENTRY, fn.argtypes)]))


def decode(rc):
    r = decode_dw5_variant(rc)
    return rc if r is None else r


def record_name(r):
    return f"dw5_fast{r[1]}" + ("_r6" if r[2] else "")


def _g(n, h, w, c, stride=1):
    return _geo(n, h, w, c, 5, stride=stride, pad=2)


SMALL = [_g(3, 1, 1, 64), _g(3, 2, 3, 48), _g(1, 4, 4, 64), _g(3, 5, 5, 16), _g(1, 6, 7, 48), _g(3, 9, 9, 16)]
STRIDE2 = [_g(1, 7, 8, 16, 2), _g(3, 8, 9, 48, 2), _g(1, 9, 7, 64, 2), _g(3, 9, 8, 16, 2)]
WIDTHS = [_g(3, 3, 1, 16), _g(1, 5, 2, 48), _g(3, 4, 3, 16, 2), _g(1, 3, 5, 64), _g(1, 5, 9, 16, 2)]      # output widths 1, 2, 2, 5, 5 ...
WIDE = _g(1, 3, 3, 2048)
GEOS = SMALL + STRIDE2 + WIDTHS + [WIDE]
# (the 1x1 map - one tap, small values - at the index only a ReLU record's case reaches, and the 9x9 map at the index of the ReLU6 case
#  without a bias: that case needs reference values above 6, which few taps without a bias do not give)
GEOS[0], GEOS[10] = GEOS[10], GEOS[0]
GEOS[0], GEOS[5] = GEOS[5], GEOS[0]
GRID_STRIDE = _g(3, 58, 57, 1024)    # 3 x 58 x 57 pixels x 64 groups = 634 752 > 2048 x 256 = 524 288
PER_RECORD = 5


def cases():
    out = []
    for ri, r in enumerate(RECORDS):
        _, fast, r6 = r
        for i in range(PER_RECORD):
            uns, zp = _INPUT[i]
            quant, want_out = (_PLAIN[i], False) if fast else _OPEN[i]
            # every record walks the whole geometry list between its cases and its neighbours': 6 x 5 = 30 >= 2 x 16 is not needed - the
            # stride is 3 (coprime to 16), so the 30 cases cover all 16 geometries (asserted in tests/test_dw5_host.py)
            out.append(Case(f"{record_name(r)}/{i}", r, GEOS[(3 * (PER_RECORD * ri + i)) % len(GEOS)], uns, zp,
                            asym=(fast == 1) or (fast == 0 and i % 2 == 0), act=_act(r6, i), quant=quant, out=want_out, bias=i != 1, seed=9000 + 100 * ri + i))
    out.append(Case("dw5_fast2/grid_stride", ("dw5", 2, False), GRID_STRIDE, True, 200, quant="plain", seed=9901))
    return out


CASES = cases()
BY_RECORD = {r: [c for c in CASES if c.record == r] for r in RECORDS}


def route_args(case, ptr=None):
    """Case.route_args without R, S and the force bit: the arguments of the route query (and, the control bits cleared, of the launch)."""
    a = case.route_args(ptr=ptr)
    return {k: v for k, v in a.items() if k not in ("R", "S")}


# The full-range case of a record: (uint8 codes, zero point, sign pattern of the weights).  Codes 0 / 255 (int8: -128 / 127) against weights
# of -128 / +127 in all 25 taps: |S1| reaches 25 * 255 * 128 = 816 000 and 25 * 255 * 127 with both signs - what a wrong re-centring (xor
# 0x80, the (128 - zp) * SUM w constant) or a wrapped byte product would break.
FULL_RANGE = {r: dict(uns=(i % 2 == 0), zp=(0, -128, 255, 127, 0, 0)[i], asym=r[1] == 1 or (r[1] == 0 and i == 0), out=r[1] == 0,
                      quant="plain_hi" if r[1] else ("uzp_hi", "signed_hi")[i // 3], act=2 if r[2] else 1) for i, r in enumerate(RECORDS)}
FULL_GEO = _g(2, 6, 5, 32, 1)
