"""The calls that reach every instantiation of the two 3x3 kernels - conv3x3_halo_i8_kernel (csrc/conv3x3_i8.hip: DLMCQ_HALO_TABLE, 40) and
conv3x3_pipe_i8_kernel (csrc/conv3x3_pipe_i8.hip: DLMCQ_PIPE_TABLE, 6) - through dlmcq_conv2d_i8_nhwc_fused: ONE table for
tests/test_halo_variants_host.py (which record does the dispatch pick: DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_HALO_VARIANT on placeholder pointers, no
GPU) and tests/test_gpu_halo_variants.py (the same calls launched and compared with an exact float64 reference).  TEST INFRASTRUCTURE ONLY.

A halo record is ("halo", column width, stride 2, halo pieces per buffer, halo buffers, XS, PLAIN); a pipelined one ("pipe", chunks, XS).
Every (width, stride, pieces, buffers) tuple has a list of geometries below; each of its four records (XS: uint8 codes, else int8; PLAIN:
the plain quantiser or its DLMCQ_EMIT_SHIFT128 form, else a quantiser with a zero point) runs all of them.  The halo kernel has no minimum
size, so the shapes are the smallest that exercise what it gets wrong:
  * piece-count boundaries, both sides: stride 1 needs ceil((258 + 2 (W + 1)) / 16) pieces - 24 up to W = 62, 32 from W = 63 to the widest
    image taken, W = 119; a stride-2 phase tile ceil((258 + Q + 1) / 16) - 18 up to Q = 29, 20 from Q = 30 to Q = 61 (input width 2 Q).
    Wide images are 2 to 5 rows high; every record that takes narrow images also has a small one (7 x 9; 12 x 16 under stride 2);
  * frame tiles of 256 rows of N (H + 1)(W + 1): every case has more than one tile, a partial last tile, N >= 2 and (H + 1)(W + 1) no
    multiple of 256, so an image seam lies inside a tile.  One case per narrow tuple has a single output pixel per image (1 x 1 input;
    2 x 2 under stride 2: every tap but the centre is border), 70 images of it;
  * chunks of 64 input channels: two halo buffers C = 128 and 192 (an even and an odd count), the single buffer C = 64; stride 2's
    three-buffer ring takes four phase tiles per chunk: C = 64, 128, 192 (64-wide) / 128, 192, 256 (128-wide) give 4 C / 64 = 1, 2, 0 /
    2, 0, 1 mod 3.  (The weight ring runs 9 steps per chunk: always a multiple of 3);
  * column blocks: K = 256 for the 128-wide kernels (the second block reads its constants at n0 = 128).  The 64-wide kernels take
    K = 192, three blocks: the launcher gives every K % 128 == 0 the 128-wide kernel, so K = 2 x 64 cannot reach them.  Stride 2 with C = 64
    is taken for K = 64 only (conv3x3_halo_applies), one block; the same records' C = 128 / 192 calls have three;
  * input types: XS records uint8 codes with a zero point above 128 (`zp` "high") and below ("low"); the others int8 codes with zero
    points 37, 0, -100, 64 - the border line is then not the zero byte;
  * quantisers: PLAIN records `plain` and `shift` (DLMCQ_EMIT_SHIFT128), the others `uzp` (unsigned range, zero point 16) and `signed`
    (signed range, a zero point); the first call of every record at the consumer scale 2^-5, where the upper clamp occurs
    (tests/test_gpu_halo_variants.py asserts it), the others at 2^-2 / 2^-1;
  * ReLU on calls 0 and 2, none on 1 and 3; call 1 of every record passes a null bias.
The pipelined kernel needs two tiles per compute unit: N is computed from the device's CU count (`Case.geo_for`; 256 without a GPU) so that the
tile count lies strictly between 2 x and 3 x the CU count and is no multiple of the grid - workgroups own unequal numbers of tiles.  Odd
images below 62 wide (13 x 11, 7 x 9), K = 512 at C = 128 and 256, K = 512 and 256 at C = 512."""
from dataclasses import dataclass, field

import test_conv_dispatch_host as D
from tiled_variant_cases import launch      # noqa: F401  (the real call; re-exported for the GPU test)

from dlmc._native import ROUTE_HALO_VARIANT, decode_halo_variant      # include/dlmcq.h

TM = 256

# THE 40 + 6 records, by hand: the launchers' tables must hold exactly these (an instantiation dropped or added is a diff here)
TUPLES = [(128, False, 24, 2), (128, False, 32, 2), (64, False, 24, 1), (64, False, 32, 1), (64, False, 24, 2), (64, False, 32, 2),
          (128, True, 18, 3), (128, True, 20, 3), (64, True, 18, 3), (64, True, 20, 3)]
HALO_RECORDS = [("halo", bn, s2, hp, nhb, xs, plain) for xs in (True, False) for plain in (True, False) for bn, s2, hp, nhb in TUPLES]
PIPE_RECORDS = [("pipe", nch, xs) for nch in (2, 4, 8) for xs in (True, False)]
RECORDS = HALO_RECORDS + PIPE_RECORDS
assert len(HALO_RECORDS) == len(set(HALO_RECORDS)) == 40 and len(PIPE_RECORDS) == len(set(PIPE_RECORDS)) == 6


def record_name(r):
    if r[0] == "pipe":
        return f"pipe_{r[1]}" + ("_xs" if r[2] else "")
    return f"halo_{r[1]}_s{2 if r[2] else 1}_{r[3]}x{r[4]}" + ("_xs" if r[5] else "") + ("_plain" if r[6] else "")


def decode(rc):
    """A ROUTE_ONLY | ROUTE_HALO_VARIANT answer -> the record, or the integer itself when it names no 3x3 instantiation."""
    r = decode_halo_variant(rc)
    return rc if r is None else r


def pieces(stride, q):
    """Halo pieces of 16 frame positions a chunk's tile needs for an OUTPUT width q (csrc/conv3x3_i8.hip: halo_pieces)."""
    return (TM + (1 if stride == 2 else 2) * (q + 1) + 2 + 15) // 16


def pipe_n(cus, fs, nblk_n):
    """Images for the pipelined kernel: about 2.5 tiles per compute unit, the last row block partial."""
    row_blocks = (5 * cus // 2) // nblk_n
    return (row_blocks * TM - TM // 2) // fs


@dataclass(frozen=True)
class Case:
    cid: str
    record: tuple
    key: tuple                    # what the operands and the pre-activation reference depend on: shared by a tuple's PLAIN and other records
    geo: dict = field(hash=False, compare=False)      # BASE's vocabulary: N H W C K R S stride pad dil uns (N: None for a pipelined case - geo_for)
    relu: int = 1
    quant: str = "plain"          # tests/test_gpu_halo_variants.py: QUANTS
    bias: bool = True
    zp: object = None             # uint8 codes: "high" / "low" (a zero point above / below 128); int8 codes: the zero point

    @property
    def pipelined(self):
        return self.record[0] == "pipe"

    def geo_for(self, cus=256):
        g = dict(D.BASE, **self.geo)
        if g["N"] is None:
            g["N"] = pipe_n(cus, (g["H"] + 1) * (g["W"] + 1), g["K"] // 128)
        return g

    def out_hw(self):
        s = self.geo["stride"]
        return self.geo["H"] // s, self.geo["W"] // s       # 3 x 3 / pad 1; stride 2 on even sizes

    def frame(self, cus=256):
        """(rows of the linear frame space N (P + 1)(Q + 1), rows of one image's frame)."""
        p, q = self.out_hw()
        return self.geo_for(cus)["N"] * (p + 1) * (q + 1), (p + 1) * (q + 1)

    def route_args(self, ptr=None, cus=256, pipelined=None):
        """Overrides of BASE for the route query (`ptr` maps an argument name to a real address; placeholders otherwise)."""
        p = (lambda name: D.P) if ptr is None else ptr
        a = {k: v for k, v in self.geo_for(cus).items() if k in self.geo}
        pipe = self.pipelined if pipelined is None else pipelined
        a.update(out=0, res=0, codes=p("codes"), relu=self.relu, zp_in=p("zp_in"), bias=p("bias") if self.bias else 0,
                 ctl=(D.PIPELINED if pipe else 0) | ROUTE_HALO_VARIANT)
        if self.quant.startswith("signed"):
            a.update(q_zp=p("q_zp"), q_lo=-128, q_hi=127)
        elif self.quant.startswith("uzp"):
            a.update(q_zp=p("q_zp"))
        elif self.quant.startswith("shift"):
            a.update(form=D.FORM_ZEROPOINT | D.SHIFT128)
        if ptr is not None:
            for name in ("x", "w", "wsum", "s_in", "s_w", "q_scale"):
                a[name] = p(name)
        return a


def _geo(n, h, w, c, k, stride=1):
    return dict(N=n, H=h, W=w, C=c, K=k, R=3, S=3, stride=stride, pad=1, dil=1)


# tuple -> [geometry]; stride 2: H, W are the INPUT's (even), the frame is the output's
_GEOS = {
    (128, False, 24, 2): [_geo(4, 7, 9, 128, 256), _geo(2, 3, 62, 192, 256), _geo(70, 1, 1, 128, 256)],
    (128, False, 32, 2): [_geo(2, 2, 63, 128, 256), _geo(2, 5, 119, 192, 256)],
    (64, False, 24, 1): [_geo(4, 7, 9, 64, 192), _geo(2, 3, 62, 64, 192), _geo(70, 1, 1, 64, 192)],
    (64, False, 32, 1): [_geo(2, 2, 63, 64, 192), _geo(2, 5, 119, 64, 192)],
    (64, False, 24, 2): [_geo(4, 7, 9, 128, 192), _geo(2, 3, 62, 192, 192), _geo(70, 1, 1, 128, 192)],
    (64, False, 32, 2): [_geo(2, 2, 63, 128, 192), _geo(2, 5, 119, 192, 192)],
    (128, True, 18, 3): [_geo(5, 12, 16, 128, 256, 2), _geo(3, 6, 58, 192, 256, 2), _geo(5, 12, 16, 256, 256, 2), _geo(70, 2, 2, 128, 256, 2)],
    (128, True, 20, 3): [_geo(3, 6, 60, 128, 256, 2), _geo(2, 4, 122, 192, 256, 2), _geo(3, 4, 60, 256, 256, 2)],
    (64, True, 18, 3): [_geo(5, 12, 16, 64, 64, 2), _geo(3, 6, 58, 128, 192, 2), _geo(5, 12, 16, 192, 192, 2), _geo(70, 2, 2, 64, 64, 2)],
    (64, True, 20, 3): [_geo(3, 6, 60, 64, 64, 2), _geo(2, 4, 122, 128, 192, 2), _geo(3, 4, 60, 192, 192, 2)],
}
_PIPE_GEOS = {2: [_geo(None, 13, 11, 128, 512), _geo(None, 7, 9, 128, 512)], 4: [_geo(None, 13, 11, 256, 512), _geo(None, 7, 9, 256, 512)],
              8: [_geo(None, 13, 11, 512, 512), _geo(None, 7, 9, 512, 256)]}
_RELU = (1, 0, 1, 0)
_QUANT = {True: ("plain_hi", "shift", "plain", "shift_hi"), False: ("uzp_hi", "signed", "uzp", "signed_hi")}
_ZP = {True: ("high", "low", "high", "low"), False: (37, 0, -100, 64)}


def cases():
    out = []
    for r in HALO_RECORDS:
        _, bn, s2, hp, nhb, xs, plain = r
        for i, geo in enumerate(_GEOS[(bn, s2, hp, nhb)]):
            out.append(Case(f"{record_name(r)}/{i}", r, (TUPLES.index((bn, s2, hp, nhb)), xs, i), dict(geo, uns=int(xs)), _RELU[i], _QUANT[plain][i],
                            bias=i != 1, zp=_ZP[xs][i]))
    for r in PIPE_RECORDS:
        _, nch, xs = r
        for i, geo in enumerate(_PIPE_GEOS[nch]):
            out.append(Case(f"{record_name(r)}/{i}", r, (100 + nch, xs, i), dict(geo, uns=int(xs)), _RELU[i], _QUANT[True][i], bias=i != 1,
                            zp=_ZP[xs][i]))
    return out


CASES = cases()
BY_RECORD = {r: [c for c in CASES if c.record == r] for r in RECORDS}
