"""The calls that reach every instantiation of conv_i8_mfma_kernel (csrc/conv_i8.hip: DLMCQ_CV_TABLE) through the public entry points -
ONE table for tests/test_tiled_variants_host.py (which pair does the dispatch pick: DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_VARIANT on placeholder
pointers, no GPU) and tests/test_gpu_tiled_variants.py (the same calls launched and compared with an exact float64 reference).
TEST INFRASTRUCTURE ONLY.

A case carries the (tile width, flags) pair it is meant to reach.  The shapes are the smallest the dispatch rules (conv_plan, conv_launch,
swap_ok) admit, chosen pair by pair for what a tiled kernel gets wrong:
  * K steps (64 reduction bytes each; the LDS ring has 3 slots, two steps in flight): the smallest reduction that reaches the pair, and a
    call of >= 7 steps whose step count differs mod 3 from it.  The ring-fed (!ADIR) pairs start at 4 steps (C = 256 -> K = 64), the
    128-wide ones at C = 1024, the 256-wide one at C = 2048; (256, ADIR | SWAP) needs a filter larger than 1 x 1 over >= 512 channels, and
    a 2 x 2 filter gives it 32 steps beside the 72 of 3 x 3;
  * row tiles of 128 pixels: N = 3 images of 7 x 9 (189 rows), 13 x 16 under 3 x 3 / stride 2 / pad 1 (7 x 8 = 56 per image, 168 rows) -
    more than one tile, the last one partial, image seams inside a tile;
  * column tiles: K = 2 x width (the second tile reads its per-channel constants at n0 != 0) wherever the dispatch rules leave a pair
    such a K; where they do not, the nearest: (64, ADIR ...) K = 192 / 320 (K = 128 moves to 128-wide tiles), 192-wide K = 192 and 576.
    The unswapped A-direct 64-wide pairs add ragged last tiles, K = 72 (col < K guard of the vector path) and K = 42 (K % 4 != 0: the
    scalar store path).  The ring-fed unswapped (64, 0) pair cannot have one: conv_plan sends only K % 64 == 0 through the ring;
  * borders (every ADIR pair, the DUAL ones with such a first pair): 3 x 3 / stride 2 / pad 1 on an odd height and an even width, and a
    3 x 3 / dilation 2 / pad 2 call, both on uint8 codes whose zero point is neither 0 nor 128 (tests/test_gpu_tiled_variants.py: above
    128 for the strided call, below for the dilated one), so a padded tap reads a non-trivial pad-table line with either high bit.  (The
    XOFF construction fixes the zero point at 0; NARROW / PADRES sources are 13 x 15: odd both ways);
  * both input types, uint8 (shift 128) and int8, per pair.
NARROW / PADRES: the widths of tests/test_gpu_narrow_rows.py ((24, 64), (96, 128), (160, 192)) and tests/test_gpu_pad_shortcut.py (the
CIFAR 16 -> 32 pair, 48 -> 96 across two column tiles) on odd sources; DUAL: second pair 1 x 1 / stride 2.
Every ReLU6 twin runs its sibling's calls with DLMCQ_ACT_RELU6."""
from dataclasses import dataclass, field

import test_conv_dispatch_host as D

from dlmc._native import (CV_ADIR, CV_ASYM, CV_DUAL, CV_NARROW, CV_PADRES, CV_R6, CV_SWAP, CV_XOFF, ROUTE_VARIANT,      # include/dlmcq.h
                          decode_variant)

FLAG_NAMES = ((CV_DUAL, "DUAL"), (CV_ADIR, "ADIR"), (CV_ASYM, "ASYM"), (CV_SWAP, "SWAP"), (CV_R6, "R6"), (CV_XOFF, "XOFF"),
              (CV_NARROW, "NARROW"), (CV_PADRES, "PADRES"))

_R6_TOO = [(64, 0), (128, 0), (64, CV_ADIR), (128, CV_ADIR), (64, CV_SWAP), (128, CV_SWAP), (256, CV_SWAP),
           (64, CV_ADIR | CV_SWAP), (128, CV_ADIR | CV_SWAP), (256, CV_ADIR | CV_SWAP),
           (64, CV_ADIR | CV_ASYM), (128, CV_ADIR | CV_ASYM),
           (64, CV_ADIR | CV_ASYM | CV_SWAP), (128, CV_ADIR | CV_ASYM | CV_SWAP), (192, CV_ADIR | CV_ASYM | CV_SWAP),
           (64, CV_ADIR | CV_XOFF), (128, CV_ADIR | CV_XOFF), (64, CV_ADIR | CV_ASYM | CV_XOFF), (128, CV_ADIR | CV_ASYM | CV_XOFF),
           (64, CV_ADIR | CV_NARROW), (64, CV_ADIR | CV_ASYM | CV_NARROW),
           (64, CV_ADIR | CV_NARROW | CV_PADRES), (64, CV_ADIR | CV_ASYM | CV_NARROW | CV_PADRES)]
# THE 48 pairs, by hand: csrc/conv_i8.hip's DLMCQ_CV_TABLE must hold exactly these (an instantiation dropped or added is a diff here)
PAIRS = [p for bn, f in _R6_TOO for p in ((bn, f), (bn, f | CV_R6))] + [(64, CV_DUAL | CV_ADIR), (128, CV_DUAL | CV_ADIR)]
assert len(PAIRS) == 48 and len(set(PAIRS)) == 48


def pair_name(pair):
    return f"{pair[0]}_" + ("+".join(n for b, n in FLAG_NAMES if pair[1] & b) or "ring")


def decode(rc):
    """A ROUTE_ONLY | ROUTE_VARIANT answer -> (width, flags), or the integer itself when it is no variant."""
    pair = decode_variant(rc)
    return rc if pair is None else pair


@dataclass(frozen=True)
class Case:
    cid: str
    pair: tuple
    entry: str
    geo: dict = field(hash=False, compare=False)      # BASE's vocabulary: N H W C K R S stride pad dil uns (+ Kf, res_*, the second pair's)
    mode: str = "codes"           # "codes" | "out_codes" | "res_out_codes" (the fp32 shortcut: a tensor, or padres' source)
    relu: int = 1
    quant: str = "plain"          # "plain" | "signed" | "shift" (tests/test_gpu_tiled_variants.py: QUANTS)
    forced: bool = True

    @property
    def asym(self):
        return bool(self.pair[1] & CV_ASYM)

    @property
    def steps(self):
        g = dict(D.BASE, **self.geo)
        n = g["R"] * g["S"] * g["C"] // 64
        return n + (g["R2"] * g["S2"] * g["C2"] // 64 if self.entry == "dual" else 0)

    def route_args(self, ptr=None):
        """Overrides of BASE for the route query (`ptr` maps an argument name to a real address; placeholders otherwise)."""
        p = (lambda name: D.P) if ptr is None else ptr
        a = dict(self.geo)
        a.update(out=p("out") if self.mode != "codes" else 0, codes=p("codes"), res=p("res") if self.mode == "res_out_codes" else 0,
                 w_off=p("w_off") if self.asym else 0, relu=self.relu, zp_in=p("zp_in"),
                 ctl=(D.FORCE_TILED if self.forced else 0) | ROUTE_VARIANT)
        if self.quant == "signed":
            a.update(q_zp=p("q_zp"), q_lo=-128, q_hi=127)
        elif self.quant == "shift":
            a.update(form=D.FORM_ZEROPOINT | D.SHIFT128)
        if ptr is not None:
            for name in ("x", "w", "bias", "wsum", "s_in", "s_w", "q_scale"):
                a[name] = p(name)
            if self.entry == "xoff":
                a.update(x_off=p("x_off"), x_tap=p("x_tap"))
            if self.entry == "dual":
                a.update({n: p(n) for n in ("x2", "w2", "bias2", "wsum2", "s_in2", "zp_in2", "s_w2")})
        return a


def launch(lib, entry, args):
    """D.call without DLMCQ_ROUTE_ONLY: the real call (`args` as D.call takes them)."""
    import ctypes
    a = dict(D.BASE, **args)
    a["q_form"] = a["form"] | a["ctl"]
    a["stream"] = a.get("stream", 0)
    a["count"] = None
    fn = getattr(lib, "dlmcq_conv2d_i8_nhwc_" + entry)
    assert len(D.ENTRIES[entry]) == len(fn.argtypes), entry
    vals = []
    for name, typ in zip(D.ENTRIES[entry], fn.argtypes):
        v = a[name]
        vals.append((v or None) if typ is ctypes.c_void_p and not isinstance(v, ctypes.c_void_p) else v)
    return int(fn(*vals))


def _geo(n, h, w, c, k, r=1, stride=1, pad=0, dil=1, uns=1, s=None, **extra):
    return dict(N=n, H=h, W=w, C=c, K=k, R=r, S=r if s is None else s, stride=stride, pad=pad, dil=dil, uns=uns, **extra)


def _pw(c, k, uns=1, **extra):          # 1 x 1 on 3 images of 7 x 9: 189 rows
    return _geo(3, 7, 9, c, k, uns=uns, **extra)


def _border(c, k, uns=1, **extra):      # 3 x 3 / stride 2 / pad 1 on 13 x 16: 168 rows, 9 C / 64 steps
    return _geo(3, 13, 16, c, k, 3, 2, 1, uns=uns, **extra)


def _dil2(c, k, uns=1, **extra):        # 3 x 3 / dilation 2 / pad 2 on 7 x 9: 189 rows
    return _geo(3, 7, 9, c, k, 3, 1, 2, 2, uns=uns, **extra)


def _second(c2, h=13, w=17):            # the dual form's second pair: 1 x 1 / stride 2 on 13 x 17 -> 7 x 9
    return dict(H2=h, W2=w, C2=c2, R2=1, S2=1, stride2=2, pad2=0, dil2=1, uns2=1)


def _narrow_three(k1, kf1, k2, kf2, k3, kf3):
    # (odd sources: 7 x 9; 13 x 15 under stride 2)
    return [("narrow", _pw(64, k1, uns=0, Kf=kf1), "out_codes"), ("narrow", _geo(3, 13, 15, 64, k2, 3, 2, 1, Kf=kf2), "res_out_codes"),
            ("narrow", _dil2(128, k3, uns=1, Kf=kf3), "res_out_codes")]


def _padres_three():
    src = dict(res_h=13, res_w=15, res_stride=2)
    return [("padres", _geo(3, 13, 15, 64, 64, 1, 2, 0, uns=0, Kf=32, res_c=16, res_clo=8, **src), "res_out_codes"),        # the CIFAR 16 -> 32 pair
            ("padres", _geo(3, 13, 15, 64, 128, 3, 2, 1, Kf=96, res_c=48, res_clo=24, **src), "res_out_codes"),  # two column tiles
            ("padres", _dil2(128, 64, uns=1, Kf=64, res_c=32, res_clo=16, res_h=7, res_w=9, res_stride=1), "res_out_codes")]


def _xoff_three(k1, k2, k3):
    # (the entry point carries the offset only for pad > 0: the 1-step call is a 1 x 1 filter with pad 1, whose border pixels are all padding)
    return [("xoff", _geo(3, 7, 9, 64, k1, 1, 1, 1), "out_codes"), ("xoff", _border(64, k2, uns=0), "res_out_codes"),
            ("xoff", _dil2(128, k3, uns=1), "out_codes")]


# pair without R6 -> [(entry, geometry, mode)]
_CALLS = {
    # ---- both operands through the ring: 1 x 1, K % 64 == 0, (C >= 512 and K <= 512) or (C >= 256 and K <= 64)
    (64, 0): [("fused", _pw(256, 64), "out_codes"), ("fused", _pw(512, 128, uns=0), "res_out_codes")],                       # 4, 8 steps
    (64, CV_SWAP): [("fused", _pw(256, 64), "codes"), ("fused", _pw(512, 128, uns=0), "codes")],
    (128, 0): [("fused", _pw(1024, 128), "out_codes"), ("fused", _pw(1088, 256, uns=0), "res_out_codes"),                    # 16, 17 steps
               ("fused", _pw(2048, 256), "out_codes")],                                   # (a 256-wide plan narrowed: fp32 output)
    (128, CV_SWAP): [("fused", _pw(1024, 128), "codes"), ("fused", _pw(1088, 256, uns=0), "codes")],
    (256, CV_SWAP): [("fused", _pw(2048, 256), "codes"), ("fused", _pw(2112, 512, uns=0), "codes")],                         # 32, 33 steps
    # ---- activations straight to registers
    (64, CV_ADIR): [("fused", _pw(64, 72, uns=0), "out_codes"), ("fused", _border(64, 42), "res_out_codes"), ("fused", _dil2(128, 192), "out_codes")],
    (128, CV_ADIR): [("fused", _pw(64, 128, uns=0), "out_codes"), ("fused", _border(64, 256), "res_out_codes"),
                     ("fused", _dil2(128, 128), "out_codes")],
    (64, CV_ADIR | CV_SWAP): [("fused", _pw(64, 64, uns=0), "codes"), ("fused", _border(64, 192), "codes"), ("fused", _dil2(128, 64), "codes")],
    (128, CV_ADIR | CV_SWAP): [("fused", _pw(64, 128, uns=0), "codes"), ("fused", _border(64, 256), "codes"), ("fused", _dil2(128, 128), "codes")],
    (256, CV_ADIR | CV_SWAP): [("fused", _geo(3, 7, 9, 512, 512, 2, 1, 1, uns=0), "codes"),             # 2 x 2 / pad 1: 32 steps, 240 rows
                               ("fused", _border(512, 256), "codes"), ("fused", _dil2(512, 256), "codes")],                  # 72 steps
    # ---- asymmetric weights (always A-direct; deep 1 x 1 reductions move from conv_plan's 64-wide ring choice to 128)
    (64, CV_ADIR | CV_ASYM): [("asym", _pw(64, 72, uns=0), "out_codes"), ("asym", _border(64, 42), "res_out_codes"), ("asym", _dil2(128, 192), "out_codes")],
    (128, CV_ADIR | CV_ASYM): [("asym", _pw(64, 128, uns=0), "out_codes"), ("asym", _border(64, 256), "res_out_codes"),
                               ("asym", _dil2(128, 128), "out_codes"), ("asym", _pw(512, 128), "out_codes")],               # 8 steps
    (64, CV_ADIR | CV_ASYM | CV_SWAP): [("asym", _pw(64, 64, uns=0), "codes"), ("asym", _border(64, 320), "codes"), ("asym", _dil2(128, 64), "codes")],
    (128, CV_ADIR | CV_ASYM | CV_SWAP): [("asym", _pw(64, 128, uns=0), "codes"), ("asym", _border(64, 256), "codes"),
                                         ("asym", _dil2(128, 128), "codes"), ("asym", _pw(512, 256), "codes")],
    (192, CV_ADIR | CV_ASYM | CV_SWAP): [("asym", _pw(64, 192, uns=0), "codes"), ("asym", _border(64, 576), "codes"), ("asym", _dil2(128, 192), "codes")],
    # ---- float activation offset, narrow fp32 rows, pad shortcuts
    (64, CV_ADIR | CV_XOFF): _xoff_three(72, 42, 192),
    (128, CV_ADIR | CV_XOFF): _xoff_three(128, 256, 128),
    (64, CV_ADIR | CV_ASYM | CV_XOFF): _xoff_three(72, 42, 192),
    (128, CV_ADIR | CV_ASYM | CV_XOFF): _xoff_three(128, 256, 128),
    (64, CV_ADIR | CV_NARROW): _narrow_three(64, 24, 128, 96, 192, 160),
    (64, CV_ADIR | CV_ASYM | CV_NARROW): _narrow_three(64, 24, 128, 96, 192, 160),
    (64, CV_ADIR | CV_NARROW | CV_PADRES): _padres_three(),
    (64, CV_ADIR | CV_ASYM | CV_NARROW | CV_PADRES): _padres_three(),
    # ---- two operand pairs: 64-wide for K <= 256 on a short reduction (or K % 128 != 0), else 128-wide
    (64, CV_DUAL | CV_ADIR): [("dual", _pw(64, 128, **_second(64)), "out_codes"), ("dual", _pw(256, 192, uns=0, **_second(192)), "out_codes"),   # 2, 7 steps
                              ("dual", _pw(256, 256, **_second(128)), "codes"),
                              ("dual", _border(64, 192, **_second(64, 13, 15)), "out_codes"), ("dual", _dil2(64, 192, **_second(128)), "codes")],
    (128, CV_DUAL | CV_ADIR): [("dual", _pw(64, 384, **_second(64)), "out_codes"), ("dual", _pw(320, 256, uns=0, **_second(128)), "out_codes"),     # 2, 7 steps
                               ("dual", _border(64, 256, **_second(64, 13, 15)), "out_codes"), ("dual", _dil2(64, 256, **_second(128)), "codes")],
}
_ROTA = ((1, "plain"), (0, "signed"), (1, "shift"), (0, "plain"), (1, "signed"))
_ROTA_R6 = ("plain", "shift", "signed", "plain", "shift")


def cases():
    out = []
    for pair in PAIRS:
        calls = _CALLS[(pair[0], pair[1] & ~CV_R6)]
        for i, (entry, geo, mode) in enumerate(calls):
            relu, quant = (2, _ROTA_R6[i]) if pair[1] & CV_R6 else _ROTA[i]
            out.append(Case(f"{pair_name(pair)}/{i}", pair, entry, geo, mode, relu, quant, forced=entry in ("fused", "asym", "dual")))
    return out


CASES = cases()
BY_PAIR = {pair: [c for c in CASES if c.pair == pair] for pair in PAIRS}
