"""The int8 convolution's host dispatch (csrc/conv_i8.hip: conv_launch and the entry points in front of it), pinned from outside: the
integer every `dlmcq_conv2d_i8_nhwc_*` entry point returns for a sweep of calls - the route it picks (asked with DLMCQ_ROUTE_ONLY on
placeholder pointers: nothing is launched, no GPU is needed) or the code it refuses the call with - must equal
tests/golden/conv_dispatch_routes.json exactly, case for case.  The fixture was written by this file's own generator
(`python tests/test_conv_dispatch_host.py --write LIBRARY`) against the library built from the commit BEFORE the dispatch was
rewritten around one call record; its `header` says so.  A rewrite of the dispatch that changes a route, a refusal code or the order
two refusals are checked in fails here.

The cases: ResNet-50's (C, K, R, stride) set, MobileOne-S1's asymmetric 192 -> 192 and 512 -> 512 pointwise layers, MobileNetV2's narrow
widths, the CIFAR option-A pad-shortcut pairs, each through every entry point that can carry it and every output mode (codes only,
fp32 only, both, with a shortcut, ReLU / ReLU6 / none, plain and zero-point quantisers, FORCE_TILED, PIPELINED), plus one case per
refusal of conv_launch, make_seg2 and the entry points.  Two refusals of conv_launch cannot be reached through the ABI and are not
here: a float offset or narrow rows together with a second operand pair (no entry point builds that call).

dlmcq_conv2d_i8_nhwc_f32 has no q_form, hence no ROUTE_ONLY: only its calls that are answered before any launch are here (refusals,
and the empty problem).  The pipelined route asks the device's compute-unit count; without a GPU the library answers 256, which is
the MI355X's count, so DLMCQ_ROUTE_HALO3X3_PIPE cases give the same answer on both machines."""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_dispatch_routes.json")

EINVAL, ERANGE, ESCRATCH, EALIGN = -1, -2, -3, -4
FORM_ZEROPOINT, SHIFT128, FORCE_TILED, ROUTE_ONLY, PIPELINED, IN_CM, OUT_CM = 2, 0x100, 0x400, 0x800, 0x1000, 0x2000, 0x4000
HALO_VARIANT = 0x20000      # DLMCQ_ROUTE_HALO_VARIANT
ROUTES = {"tiled": 1, "halo3x3": 2, "pw": 3, "pwr": 4, "halo3x3_pipe": 7}
P = 4096            # a placeholder pointer: non-null, 16-byte aligned, never dereferenced
P4, P2 = P + 4, P + 2   # 4-byte aligned only; 2-byte aligned only

# every argument of every entry point by name; an entry point marshals the ones it has
BASE = dict(x=P, w=P, out=0, bias=P, wsum=P, s_in=P, zp_in=0, s_w=P, w_off=P, N=1, H=14, W=14, C=64, K=64, R=1, S=1, stride=1, pad=0, dil=1,
            uns=1, res=0, relu=1, codes=P, q_scale=P, q_zp=0, q_lo=0, q_hi=255, form=FORM_ZEROPOINT, ctl=0, g=0.0,
            partials=P, cap=1 << 40, count=True, x_off=P, x_tap=P, Kf=0, res_h=0, res_w=0, res_c=0, res_stride=1, res_clo=0,
            x2=P, w2=P, bias2=0, wsum2=P, s_in2=P, zp_in2=0, s_w2=P, H2=14, W2=14, C2=64, R2=1, S2=1, stride2=1, pad2=0, dil2=1, uns2=1)
_PROBLEM = "N H W C K R S stride pad dil uns".split()
_QUANT = "relu codes q_scale q_zp q_lo q_hi q_form g".split()
ENTRIES = {
    "f32": "x w out bias wsum s_in zp_in s_w".split() + _PROBLEM + ["stream"],
    "fused": "x w out bias wsum s_in zp_in s_w".split() + _PROBLEM + ["res"] + _QUANT + ["stream"],
    "fused_observed": "x w out bias wsum s_in zp_in s_w".split() + _PROBLEM + ["res"] + _QUANT + ["partials", "cap", "count", "stream"],
    "asym": "x w out bias wsum s_in zp_in s_w w_off".split() + _PROBLEM + ["res"] + _QUANT + ["stream"],
    "xoff": "x w out bias wsum s_in zp_in s_w w_off".split() + _PROBLEM + ["res"] + _QUANT + ["x_off", "x_tap", "stream"],
    "narrow": "x w out bias wsum s_in zp_in s_w w_off".split() + _PROBLEM + ["res"] + _QUANT + ["Kf", "stream"],
    "padres": "x w out bias wsum s_in zp_in s_w w_off".split() + _PROBLEM + "res res_h res_w res_c res_stride res_clo".split() + _QUANT
              + ["Kf", "stream"],
    "dual": "x w out bias wsum s_in zp_in s_w".split() + _PROBLEM
            + "x2 w2 bias2 wsum2 s_in2 zp_in2 s_w2 H2 W2 C2 R2 S2 stride2 pad2 dil2 uns2".split() + _QUANT + ["stream"],
}


def call(lib, entry, case):
    """One call; DLMCQ_ROUTE_ONLY rides in every q_form there is, whatever the case says: a case can be refused, never launched."""
    a = dict(BASE, **case)
    a["q_form"] = a["form"] | a["ctl"] | ROUTE_ONLY
    a["stream"] = 0
    count = ctypes.c_int64(-1)
    a["count"] = ctypes.cast(ctypes.byref(count), ctypes.c_void_p) if a["count"] else None
    fn = getattr(lib, "dlmcq_conv2d_i8_nhwc_" + entry)
    args = []
    assert len(ENTRIES[entry]) == len(fn.argtypes), entry
    for name, typ in zip(ENTRIES[entry], fn.argtypes):
        v = a[name]
        args.append((v or None) if typ is ctypes.c_void_p and not isinstance(v, ctypes.c_void_p) else v)
    return int(fn(*args))


def cases():
    """[(id, entry, overrides of BASE)], deterministic.  The ids are the fixture's keys."""
    out = []

    def add(name, entry, **kw):
        out.append((f"{entry}:{name}", entry, kw))

    # ---- the sweep: shape x size x output mode x control bits, through every entry point that takes the call ----
    shapes = [  # (tag, C, K, R, stride, pad)
        ("r50_64-64_3x3", 64, 64, 3, 1, 1), ("r50_64-256", 64, 256, 1, 1, 0), ("r50_256-64", 256, 64, 1, 1, 0),
        ("r50_256-128_3x3s2", 256, 128, 3, 2, 1), ("r50_128-128_3x3", 128, 128, 3, 1, 1), ("r50_256-256_3x3", 256, 256, 3, 1, 1),
        ("r50_512-512_3x3", 512, 512, 3, 1, 1), ("r50_512-512_3x3s2", 512, 512, 3, 2, 1), ("r50_256-512", 256, 512, 1, 1, 0),
        ("r50_512-128", 512, 128, 1, 1, 0), ("r50_1024-256", 1024, 256, 1, 1, 0), ("r50_256-1024", 256, 1024, 1, 1, 0),
        ("r50_2048-512", 2048, 512, 1, 1, 0), ("r50_512-2048", 512, 2048, 1, 1, 0), ("r50_64-128_3x3s2", 64, 128, 3, 2, 1),
        ("m1_192-192", 192, 192, 1, 1, 0), ("m1_512-512", 512, 512, 1, 1, 0), ("m1_192-576", 192, 576, 1, 1, 0),
        ("m1_64-64", 64, 64, 1, 1, 0), ("mnv2_64-384", 64, 384, 1, 1, 0), ("k320", 64, 320, 1, 1, 0), ("dil2_3x3", 64, 128, 3, 1, 2),
    ]
    sizes = [("n2_48", 2, 48, 48), ("n1_14", 1, 14, 14), ("n1_7", 1, 7, 7)]       # 4 608 pixels (the LDS-resident kernels' floor is 4 096), 196, 49
    modes = [  # (tag, fields)
        ("codes", dict()), ("codes_r6", dict(relu=2)), ("codes_norelu", dict(relu=0)), ("codes_zp", dict(q_zp=P, q_lo=-128, q_hi=127)),
        ("codes_shift", dict(form=FORM_ZEROPOINT | SHIFT128)), ("codes_c4", dict(codes=P4)),
        ("out", dict(out=P, codes=0)), ("out_codes", dict(out=P)), ("res_codes", dict(res=P)), ("res_out_codes", dict(res=P, out=P)),
        ("res_out_codes_r6", dict(res=P, out=P, relu=2)), ("res_out", dict(res=P, out=P, codes=0)),
    ]
    for stag, C, K, R, stride, pad in shapes:
        dil = 2 if stag.startswith("dil2") else 1
        for ztag, N, H, W in sizes:
            geo = dict(N=N, H=H, W=W, C=C, K=K, R=R, S=R, stride=stride, pad=pad, dil=dil)
            for mtag, m in modes:
                for ctag, ctl in (("", 0), ("+tiled", FORCE_TILED), ("+pipe", PIPELINED)):
                    if ctl and (mtag not in ("codes", "res_out_codes") or ztag == "n1_7"):
                        continue
                    name = f"{stag}/{ztag}/{mtag}{ctag}"
                    add(name, "fused", ctl=ctl, **geo, **m)
                    if not ctl and mtag in ("codes", "codes_r6", "out_codes", "res_codes", "res_out_codes", "codes_c4"):
                        add(name, "asym", **geo, **m)
                    if not ctl and m.get("out") and ztag != "n2_48":
                        add(name, "fused_observed", **geo, **m)
                    if not ctl and mtag in ("codes", "codes_r6", "out_codes", "res_out_codes") and ztag != "n1_7":
                        add(name, "xoff", **geo, **m)
                        add(name + "/sym", "xoff", w_off=0, **geo, **m)
    # the pipelined 3x3 kernel needs two tiles per compute unit: a batch that gives it 612
    for C in (128, 256, 512):
        geo = dict(N=12, H=56, W=56, C=C, K=512, R=3, S=3, pad=1)
        add(f"pipe_{C}-512/n12_56", "fused", ctl=PIPELINED, **geo)
        add(f"pipe_{C}-512/n12_56/no_bit", "fused", **geo)
        add(f"pipe_{C}-512/n12_56/r6", "fused", ctl=PIPELINED, relu=2, **geo)
        add(f"pipe_{C}-512/n12_56/zp", "fused", ctl=PIPELINED, q_zp=P, **geo)
    add("pipe_512-1024/n12_56", "fused", ctl=PIPELINED, N=12, H=56, W=56, C=512, K=1024, R=3, S=3, pad=1)       # K > the pipelined kernel's 512
    add("pipe_256-512/n2_56", "fused", ctl=PIPELINED, N=2, H=56, W=56, C=256, K=512, R=3, S=3, pad=1)           # too few tiles
    add("pipe_64-64/n12_56", "fused", ctl=PIPELINED, N=12, H=56, W=56, C=64, K=64, R=3, S=3, pad=1)
    # DLMCQ_ROUTE_HALO_VARIANT: which instantiation of the 3x3 kernels (the only entries not recorded from the parent library, which did not
    # know the bit: they were added by the commit that introduced it, from its own library; every other entry is unchanged)
    for stag, C, K, stride in (("r50_64-64_3x3", 64, 64, 1), ("r50_128-128_3x3", 128, 128, 1), ("r50_256-128_3x3s2", 256, 128, 2), ("64-192_3x3s2", 128, 192, 2)):
        for ztag, N, H, W in (("n2_48", 2, 48, 48), ("n1_14", 1, 14, 14), ("n1_4x100", 1, 4, 100)):
            geo = dict(N=N, H=H, W=W, C=C, K=K, R=3, S=3, stride=stride, pad=1)
            for mtag, m in (("codes", dict()), ("codes_zp", dict(q_zp=P, q_lo=-128, q_hi=127)), ("codes_int8", dict(uns=0)), ("codes_r6", dict(relu=2)),
                            ("out_codes", dict(out=P))):
                add(f"{stag}/{ztag}/{mtag}+which", "fused", ctl=HALO_VARIANT, **geo, **m)
            add(f"{stag}/{ztag}/codes+which+tiled", "fused", ctl=HALO_VARIANT | FORCE_TILED, **geo)
    for C in (128, 256, 512):
        add(f"pipe_{C}-512/n12_56+which", "fused", ctl=PIPELINED | HALO_VARIANT, N=12, H=56, W=56, C=C, K=512, R=3, S=3, pad=1)
        add(f"pipe_{C}-512/n12_56/int8+which", "fused", ctl=PIPELINED | HALO_VARIANT, uns=0, N=12, H=56, W=56, C=C, K=512, R=3, S=3, pad=1)
    add("pipe_256-512/n2_56+which", "fused", ctl=PIPELINED | HALO_VARIANT, N=2, H=56, W=56, C=256, K=512, R=3, S=3, pad=1)      # too few tiles: the halo kernel's record
    add("r50_64-256/n2_48/codes+which", "fused", ctl=HALO_VARIANT, N=2, H=48, W=48, C=64, K=256)                              # (pointwise: unchanged)
    add("r50_64-64_3x3/n2_48/codes+which", "asym", ctl=HALO_VARIANT, N=2, H=48, W=48, C=64, K=64, R=3, S=3, pad=1)
    # chunk-major fp32 tensors: only a call that lands on the block-end kernel may carry the bits
    blk = dict(N=2, H=48, W=48, C=512, K=2048, res=P, out=P)
    for tag, ctl in (("in", IN_CM), ("out", OUT_CM), ("both", IN_CM | OUT_CM)):
        add(f"cm_{tag}/pwr", "fused", ctl=ctl, **blk)
        add(f"cm_{tag}/pwr_codes_only", "fused", ctl=ctl, **dict(blk, out=0))
        add(f"cm_{tag}/pwr_out_only", "fused", ctl=ctl, **dict(blk, codes=0))
        add(f"cm_{tag}/forced_tiled", "fused", ctl=ctl | FORCE_TILED, **blk)
        add(f"cm_{tag}/small", "fused", ctl=ctl, **dict(blk, N=1, H=7, W=7))
        add(f"cm_{tag}/3x3", "fused", ctl=ctl, N=1, H=14, W=14, C=64, K=64, R=3, S=3, pad=1)
        add(f"cm_{tag}/asym", "asym", ctl=ctl, **blk)
        add(f"cm_{tag}/dual", "dual", ctl=ctl, N=2, H=48, W=48, C=256, K=1024, out=P, H2=96, W2=96, C2=512, stride2=2)
    # narrow fp32 rows (MobileNetV2's projection widths zero-padded to the K step) and their refusals
    for K, Kf in ((64, 24), (64, 32), (64, 64), (128, 96), (192, 160), (384, 320)):
        for ztag, N, H, W in sizes:
            geo = dict(N=N, H=H, W=W, C=192, K=K, Kf=Kf, out=P)
            add(f"{K}_{Kf}/{ztag}", "narrow", relu=0, **geo)
            add(f"{K}_{Kf}/{ztag}/sym_res_r6", "narrow", w_off=0, res=P, relu=2, **geo)
            add(f"{K}_{Kf}/{ztag}/out_only", "narrow", relu=0, codes=0, **geo)
        add(f"{K}_{Kf}/3x3s2", "narrow", N=1, H=14, W=14, C=64, K=K, Kf=Kf, R=3, S=3, stride=2, pad=1, out=P)
    nar = dict(N=1, H=14, W=14, C=64, K=128, out=P)
    for tag, kw in (("K_below_64", dict(K=32, Kf=32)), ("K_not_x64", dict(K=96, Kf=96)), ("Kf_not_x4", dict(Kf=126)), ("Kf_above_K", dict(Kf=132)),
                    ("Kf_in_earlier_block", dict(Kf=64)), ("Kf_0", dict(Kf=0)), ("Kf_negative", dict(Kf=-4)), ("pipelined", dict(Kf=96, ctl=PIPELINED)),
                    ("forced_tiled", dict(Kf=96, ctl=FORCE_TILED)), ("codes_4_aligned", dict(Kf=96, codes=P4)), ("codes_2_aligned", dict(Kf=96, codes=P2)),
                    ("chunk_major", dict(Kf=96, ctl=OUT_CM)), ("no_output", dict(Kf=96, out=0, codes=0)), ("C_not_x64", dict(Kf=96, C=32))):
        add("refuse/" + tag, "narrow", **dict(nar, **kw))
    # pad shortcuts: CIFAR option A, pairs (stride 2, 8 / 16 zero channels in front)
    for tag, C, K, Kf, res_c, clo in (("16-32", 64, 64, 32, 16, 8), ("32-64", 64, 64, 64, 32, 16)):
        pr = dict(N=2, H=32, W=32, C=C, K=K, Kf=Kf, R=3, S=3, stride=2, pad=1, out=P, res=P, res_h=32, res_w=32, res_c=res_c, res_stride=2,
                  res_clo=clo)
        add(tag, "padres", **pr)
        add(tag + "/sym_r6", "padres", w_off=0, relu=2, **pr)
        add(tag + "/odd_source", "padres", **dict(pr, H=31, W=31, res_h=31, res_w=31))
        for rtag, kw in (("no_source", dict(res=0)), ("h_0", dict(res_h=0)), ("w_0", dict(res_w=0)), ("stride_0", dict(res_stride=0)),
                         ("c_below_4", dict(res_c=2)), ("c_not_x4", dict(res_c=res_c + 2)), ("clo_negative", dict(res_clo=-4)),
                         ("clo_not_x4", dict(res_clo=clo + 2)), ("past_Kf", dict(res_clo=Kf - res_c + 4)), ("P_differs", dict(res_h=30)),
                         ("Q_differs", dict(res_w=34)), ("h_2^30", dict(res_h=1 << 30)), ("w_2^30", dict(res_w=1 << 30)), ("c_2^30", dict(res_c=1 << 30)),
                         ("clo_2^30", dict(res_clo=1 << 30)), ("source_2^40", dict(res_h=1 << 20, res_w=1 << 20, res_stride=1 << 16)),
                         ("Kf_rule", dict(Kf=Kf + 2)), ("pipelined", dict(ctl=PIPELINED)), ("source_misaligned", dict(res=P4)),
                         ("codes_misaligned", dict(codes=P4))):
            add(f"{tag}/refuse/{rtag}", "padres", **dict(pr, **kw))
    # the dual form: ResNet-50's first blocks (the block's last 1x1 + the 1x1 / stride-s convolution on the shortcut)
    for tag, C, K, C2, s2 in (("s1_64+64-256", 64, 256, 64, 1), ("s2_128+256-512", 128, 512, 256, 2), ("s3_256+512-1024", 256, 1024, 512, 2),
                              ("s4_512+1024-2048", 512, 2048, 1024, 2), ("s3_swapped_512+256-1024", 512, 1024, 256, 2)):
        for ztag, N, H in (("n2_48", 2, 48), ("n1_14", 1, 14), ("n1_7", 1, 7)):
            sw = "swapped" in tag
            d = dict(N=N, C=C, K=K, C2=C2, H=H * (s2 if sw else 1), W=H * (s2 if sw else 1), stride=s2 if sw else 1,
                     H2=H * (1 if sw else s2), W2=H * (1 if sw else s2), stride2=1 if sw else s2)
            add(f"{tag}/{ztag}/out_codes", "dual", out=P, **d)
            add(f"{tag}/{ztag}/codes", "dual", **d)
            add(f"{tag}/{ztag}/out", "dual", out=P, codes=0, **d)
            add(f"{tag}/{ztag}/out_codes+tiled", "dual", out=P, ctl=FORCE_TILED, **d)
            add(f"{tag}/{ztag}/out_codes_zp", "dual", out=P, q_zp=P, **d)
    dd = dict(N=1, H=14, W=14, C=64, K=256, out=P, H2=28, W2=28, C2=64, stride2=2)
    for tag, kw in (("relu6", dict(relu=2)), ("P_differs", dict(H2=26)), ("Q_differs", dict(W2=30)), ("PQ_transposed", dict(H=7, W=28, H2=56, W2=14)),
                    ("C2_not_x64", dict(C2=96)), ("x2_null", dict(x2=0)), ("w2_null", dict(w2=0)), ("wsum2_null", dict(wsum2=0)),
                    ("s_in2_null", dict(s_in2=0)), ("s_w2_null", dict(s_w2=0)), ("x2_misaligned", dict(x2=P4)), ("w2_misaligned", dict(w2=P4)),
                    ("stride2_0", dict(stride2=0)), ("pad2_negative", dict(pad2=-1)), ("dil2_0", dict(dil2=0)), ("H2_0", dict(H2=0)),
                    ("P2_below_1", dict(H2=1, R2=3)), ("second_2^40", dict(H2=1 << 17, W2=1 << 17, stride2=1 << 14)),
                    ("empty_null_second", dict(N=0, x2=0, w2=0)), ("x_null", dict(x=0)), ("C_not_x64", dict(C=32)), ("chunk_major", dict(ctl=IN_CM)),
                    ("pipelined", dict(ctl=PIPELINED))):
        add("refuse/" + tag, "dual", **dict(dd, **kw))
    # ---- conv_launch's refusals, one by one, through the fused entry point; the same few through every other one ----
    ok = dict(N=1, H=14, W=14, C=64, K=128, R=3, S=3, pad=1, out=P)
    refusals = [
        ("N_negative", dict(N=-1)), ("H_0", dict(H=0)), ("W_0", dict(W=0)), ("C_0", dict(C=0)), ("K_0", dict(K=0)), ("R_0", dict(R=0)), ("S_0", dict(S=0)),
        ("stride_0", dict(stride=0)), ("stride_negative", dict(stride=-2)), ("pad_negative", dict(pad=-1)), ("dil_0", dict(dil=0)),
        ("C_not_x64", dict(C=32)), ("C_96", dict(C=96)), ("P_below_1", dict(H=1, pad=0)), ("Q_below_1", dict(W=2, pad=0, dil=2)),
        ("empty", dict(N=0)), ("empty_all_null", dict(N=0, x=0, w=0, out=0, codes=0, wsum=0, s_in=0, s_w=0)), ("empty_bad_C", dict(N=0, C=32)),
        ("x_null", dict(x=0)), ("w_null", dict(w=0)), ("wsum_null", dict(wsum=0)), ("s_in_null", dict(s_in=0)), ("s_w_null", dict(s_w=0)),
        ("no_output", dict(out=0, codes=0)), ("bias_zp_null", dict(bias=0, zp_in=0)),
        ("q_scale_null", dict(q_scale=0)), ("q_scale_null_no_codes", dict(q_scale=0, codes=0)), ("lo_above_hi", dict(q_lo=5, q_hi=-5)),
        ("lo_below_-128", dict(q_lo=-129, q_hi=0)), ("hi_above_255", dict(q_hi=256)), ("range_above_255", dict(q_lo=-128, q_hi=255)),
        ("form_5", dict(form=5)), ("form_rootq", dict(form=4)), ("form_255", dict(form=255)), ("shifted_signed", dict(form=FORM_ZEROPOINT | SHIFT128, q_lo=-5, q_hi=5)),
        ("bad_form_no_codes", dict(form=5, codes=0)),
        ("x_misaligned", dict(x=P4)), ("w_misaligned", dict(w=P4)), ("out_misaligned", dict(out=P4)), ("res_misaligned", dict(res=P4)),
        ("codes_2_aligned", dict(codes=P2)), ("codes_4_aligned", dict(codes=P4)), ("null_before_align", dict(x=P4, wsum=0)),
        ("align_before_range", dict(x=P4, K=1 << 24)),
        ("K_2^24", dict(K=1 << 24)), ("K_2^24-64", dict(K=(1 << 24) - 64)), ("M_2^31", dict(H=46341, W=46341)), ("M_below_2^31", dict(H=46340, W=46340)),
        ("input_2^40", dict(H=1 << 17, W=1 << 17, stride=1 << 4)), ("grid_2^31", dict(N=2, H=46340, W=46340, stride=2, K=(1 << 24) - 64, pad=0, R=1, S=1)),
    ]
    for tag, kw in refusals:
        add("refuse/" + tag, "fused", **dict(ok, **kw))
    for entry in ("asym", "xoff", "fused_observed", "narrow", "padres", "dual", "f32"):
        extra = dict(narrow=dict(Kf=96), padres=dict(Kf=96, res=P, res_h=14, res_w=14, res_c=16), dual=dict(H2=14, W2=14, R2=1)).get(entry, {})
        for tag, kw in refusals:
            if tag in ("stride_0", "C_not_x64", "empty", "x_null", "no_output", "x_misaligned", "K_2^24", "M_2^31", "lo_above_hi", "form_5", "P_below_1",
                       "wsum_null", "out_misaligned", "empty_all_null", "N_negative", "dil_0"):
                if entry == "f32" and tag in ("lo_above_hi", "form_5"):
                    continue
                add("launch/" + tag, entry, **dict(ok, **extra, **kw))
    add("refuse/w_off_null", "asym", **dict(ok, w_off=0))
    add("refuse/w_off_null_first", "asym", **dict(ok, w_off=0, x=P4))
    for tag, kw in (("x_off_null", dict(x_off=0)), ("x_tap_null", dict(x_tap=0)), ("x_tap_misaligned", dict(x_tap=P4)), ("x_tap_misaligned_pad0", dict(x_tap=P4, pad=0, R=1, S=1)),
                    ("forced_tiled", dict(ctl=FORCE_TILED)), ("pipelined", dict(ctl=PIPELINED)), ("chunk_major", dict(ctl=IN_CM, res=P))):
        add("refuse/" + tag, "xoff", **dict(ok, **kw))
    # the observed entry point: its own refusals come first, then the capacity of three planes, then conv_launch's
    obs = dict(N=4, H=32, W=32, C=64, K=128, out=P)
    cap = ((4 * 32 * 32 + 127) // 128) * ((128 + 63) // 64)
    for tag, kw in (("cap_one_plane", dict(cap=cap)), ("cap_3_planes-1", dict(cap=3 * cap - 1)), ("cap_3_planes", dict(cap=3 * cap)), ("cap_negative", dict(cap=-1)),
                    ("partials_null", dict(partials=0)), ("count_null", dict(count=False)), ("out_null", dict(out=0)), ("K_0", dict(K=0)), ("empty", dict(N=0)),
                    ("stride_0_small_cap", dict(stride=0, cap=3 * cap - 1)), ("stride_0", dict(stride=0, cap=3 * cap)), ("stride_negative", dict(stride=-1, cap=3 * cap)),
                    ("stride_2_cap_of_stride_1", dict(stride=2, cap=3 * cap)), ("stride_2_small_cap", dict(stride=2, cap=3 * cap // 4 - 1)),
                    ("scratch_before_null_x", dict(x=0, cap=0)), ("scratch_before_C", dict(C=32, cap=0)), ("3x3_pad1", dict(R=3, S=3, pad=1, cap=3 * cap)),
                    ("3x3_pad0_small_cap", dict(R=3, S=3, cap=3 * cap - 1)), ("P_below_1", dict(H=1, R=3, S=3, cap=3 * cap)),
                    ("pwr", dict(N=8, H=32, W=32, C=256, K=256, res=P, cap=1 << 30)), ("r6_codes", dict(relu=2, cap=3 * cap))):
        add("observed/" + tag, "fused_observed", **dict(obs, **kw))
    assert len({c[0] for c in out}) == len(out), "duplicate case id"
    return out


def run(lib):
    return {cid: call(lib, entry, kw) for cid, entry, kw in cases()}


def _lib():
    from dlmc import _native as N
    return N.lib


def test_every_case_answers_as_the_fixture_records():
    """Exact: no tolerance, no case left out, none added without regenerating."""
    with open(FIXTURE) as f:
        want = json.load(f)["results"]
    got = run(_lib())
    assert sorted(got) == sorted(want), "the case generator and the fixture disagree on the cases: regenerate with the PARENT library"
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} of {len(want)} calls answer differently (got, fixture): {dict(list(wrong.items())[:12])}"


def test_the_fixture_reaches_every_route_and_every_refusal():
    """What the sweep must have covered (checked on the fixture, so a generator that drifts away from a route or a refusal fails)."""
    with open(FIXTURE) as f:
        want = json.load(f)["results"]
    assert len(want) >= 300
    seen = set(want.values())
    assert set(ROUTES.values()) <= seen and {0, EINVAL, EALIGN, ESCRATCH, ERANGE} <= seen
    per_entry = {}
    for k, v in want.items():
        per_entry.setdefault(k.split(":")[0], set()).add(v)
    assert set(per_entry) == set(ENTRIES)
    assert per_entry["f32"] <= {0, EINVAL, EALIGN, ERANGE}, "a dlmcq_conv2d_i8_nhwc_f32 case would launch"
    for entry in ("fused", "asym"):
        assert {ROUTES["tiled"], ROUTES["pw"]} <= per_entry[entry]
    assert {ROUTES["tiled"], ROUTES["pwr"], ROUTES["halo3x3"], ROUTES["halo3x3_pipe"]} <= per_entry["fused"]
    assert {ROUTES["tiled"], ROUTES["pwr"]} <= per_entry["dual"] and ROUTES["tiled"] in per_entry["narrow"] and ROUTES["tiled"] in per_entry["padres"]
    assert {ROUTES["tiled"], ROUTES["pw"]} <= per_entry["xoff"]         # (an unpadded xoff call carries no offset: every kernel may take it)
    named = {  # the refusals the dispatch is known by, each at its code
        "fused:refuse/x_null": EINVAL, "fused:refuse/x_misaligned": EALIGN, "fused:refuse/C_not_x64": EINVAL, "fused:refuse/lo_above_hi": EINVAL,
        "fused:refuse/form_5": EINVAL, "fused:refuse/empty": 0, "fused:refuse/K_2^24": ERANGE, "fused:refuse/M_2^31": ERANGE,
        "fused:cm_in/3x3": EINVAL, "fused:cm_both/pwr": ROUTES["pwr"], "narrow:refuse/pipelined": EINVAL, "narrow:refuse/Kf_not_x4": EINVAL,
        "narrow:refuse/Kf_above_K": EINVAL, "narrow:refuse/Kf_in_earlier_block": EINVAL, "narrow:refuse/K_below_64": EINVAL,
        "narrow:refuse/codes_4_aligned": EALIGN, "padres:16-32": ROUTES["tiled"], "padres:16-32/refuse/c_not_x4": EINVAL,
        "padres:16-32/refuse/clo_not_x4": EINVAL, "padres:16-32/refuse/past_Kf": EINVAL, "padres:16-32/refuse/P_differs": EINVAL,
        "padres:16-32/refuse/Q_differs": EINVAL, "padres:16-32/refuse/source_2^40": ERANGE, "dual:refuse/P_differs": EINVAL,
        "dual:refuse/Q_differs": EINVAL, "dual:refuse/PQ_transposed": EINVAL, "dual:refuse/relu6": EINVAL,
        "fused_observed:observed/cap_3_planes-1": ESCRATCH, "fused_observed:observed/cap_3_planes": ROUTES["tiled"],
        "fused_observed:observed/stride_0_small_cap": ESCRATCH, "fused_observed:observed/stride_0": EINVAL,
    }
    assert {k: want[k] for k in named} == named


if __name__ == "__main__":      # python tests/test_conv_dispatch_host.py --write LIBRARY [COMMIT]: the fixture, from that library
    assert sys.argv[1] == "--write"
    sys.path.insert(0, os.path.join(ROOT, "dlmc-quant_amd"))
    from dlmc import _native as N
    lib = ctypes.CDLL(os.path.abspath(sys.argv[2]))
    for name in ENTRIES:
        fn = getattr(lib, "dlmcq_conv2d_i8_nhwc_" + name)
        fn.restype, fn.argtypes = N.SIGNATURES["dlmcq_conv2d_i8_nhwc_" + name]
    results = run(lib)
    header = ("Return values of the dlmcq_conv2d_i8_nhwc_* entry points for the cases of tests/test_conv_dispatch_host.py, recorded from the "
              "library built at commit %s - the parent of the commit that rewrote the host dispatch around one call record - by "
              "`python tests/test_conv_dispatch_host.py --write LIBRARY`.  Positive: a DLMCQ_ROUTE_*; 0: DLMCQ_OK; negative: a refusal."
              % (sys.argv[3] if len(sys.argv) > 3 else "?"))
    with open(FIXTURE, "w") as f:
        json.dump({"header": header, "results": results}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(len(results), "cases;", {v: list(results.values()).count(v) for v in sorted(set(results.values()))})
