"""The host side of the first-layer, depthwise, depthwise + pointwise and pooled-head int8 entry points, pinned from outside: the integer
`dlmcq_conv2d_i8_stem_fused` / `_stem_asym` / `_stem_xoff`, `dlmcq_conv2d_i8_stem_pool_fused`, `dlmcq_conv2d_dw_i8_nhwc` / `_dw_i8_nhwc_xoff`,
`dlmcq_conv2d_dwpw_i8_nhwc` and `dlmcq_conv2d_i8_nhwc_gap` return for a sweep of calls on placeholder pointers must equal
tests/golden/dw_stem_refusals.json exactly, case for case.  The fixture was written by this file's own generator
(`python tests/test_dw_stem_refusals_host.py --write LIBRARY COMMIT`) against the library built from the commit BEFORE these hosts were
rewritten around one call record and one kernel table per family; its `header` names that commit.  A rewrite that changes a refusal's
code, the order two refusals are checked in, which bits of `q_form` an entry point takes, or where the depthwise dispatch hands a layer
to the matrix-core kernel, fails here.

The sweep holds ONLY calls that are answered without a launch: every refusal, the empty problem (N == 0), and - for the depthwise and
pooled-head entry points, which have a route query - accepted calls made with DLMCQ_ROUTE_ONLY.  The first-layer and dwpw entry points
have no route query, so no accepted call of theirs is in it: a property of an accepted call (an optional pointer given, a `q_form` bit
passed through because `codes` is null) is pinned by a later fault, a 4-byte-aligned pointer where 16 are required (`then_align`:
DLMCQ_EALIGN says the earlier checks let the call through) or a size past the 32-bit bound (`then_erange`).  The generator asserts that
every recorded value is negative, 0 for a case with no rows, or a route code for a case that carries DLMCQ_ROUTE_ONLY; and the calls are
made in a child process that hides the GPUs (HIP_VISIBLE_DEVICES=-1) and first asks the HIP runtime for its device count: it makes no
library call unless the answer is zero or an error.

The `return` statements of the recorded commit's host code that answer without a launch, all reached (file:line of that commit, csrc/):
  conv_stem_i8.hip    stem_launch 707 708 (EINVAL) 711 (OK) 712 715 (EINVAL) 716 (EALIGN) 717 (ERANGE); _stem_asym 799; _stem_xoff 810 811
                      (EINVAL) 812 (EALIGN); _stem_pool_fused 851 853 854 (EINVAL) 858 (OK) 859 862 (EINVAL) 863 (EALIGN) 870 (ERANGE)
  conv_dw_i8.hip      dw_launch 537 539 (EINVAL) 542 (OK) 543 546 (EINVAL) 549 (EALIGN) 550 (ERANGE) 573 (ROUTE_DWM) 578 (EINVAL) 579 (ROUTE_DW);
                      _dw_i8_nhwc_xoff 657 (EINVAL) 658 (EALIGN)
  conv_dwm_i8.hip     conv_dwm_applies 238 239 240 241 (no) 242 (yes and no), each seen as ROUTE_DW / ROUTE_DWM of a depthwise route query
  conv_dwpw_i8.hip    366 367 (EINVAL) 368 (OK) 369 370 (EINVAL) 371 (EALIGN) 375 (EINVAL) 380 (ERANGE) 382 (EINVAL)
  conv_gap_i8.hip     156 157 158 161 162 (EINVAL) 165 (OK) 166 (EINVAL) 168 (EALIGN) 169 (ERANGE) 170 (ROUTE_GAP)
  conv_gap.h          gap_set_quantiser 28 29 (EINVAL) 30 (OK)
Not reachable without a launch, hence not in the sweep: conv_stem_i8.hip 857 (a pooled size below 1 needs a convolution output below 1,
refused at 854); the three returns of stem_pool7_applies (conv_stem_pool7_i8.hip 351 353 354: nothing is refused after the question is
asked, either answer launches) and the range check of stem_pool7_launch (370: weaker than the entry point's own at 870).

Many refusals share DLMCQ_EINVAL, so the order of the checks is pinned where two codes differ: the `order/` cases carry two faults."""
import ctypes
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "dw_stem_refusals.json")

OK, EINVAL, ERANGE, EALIGN = 0, -1, -2, -4
ROUTE_DW, ROUTE_DWM, ROUTE_GAP = 5, 6, 8
ZP, ROOTQ = 2, 4
BITS = dict(SHIFT128=0x100, W2_CHUNK_MAJOR=0x200, FORCE_TILED=0x400, ROUTE_ONLY=0x800, PIPELINED=0x1000, FP32_IN_CHUNK_MAJOR=0x2000,
            FP32_OUT_CHUNK_MAJOR=0x4000, ROUTE_VARIANT=0x10000, ROUTE_HALO_VARIANT=0x20000)      # every bit of `q_form` include/dlmcq.h names
FORCE_TILED, ROUTE_ONLY = BITS["FORCE_TILED"], BITS["ROUTE_ONLY"]
P = 4096            # a placeholder pointer: non-null, 16-byte aligned, never dereferenced
P4 = P + 4          # 4-byte aligned only

_Q = "relu codes q_scale q_zp q_lo q_hi q_form g".split()
_STEM = "x w out bias wsum s_in zp_in s_w".split()
_DW = "x w out bias s_in zp_in s_w w_off N H W C R S stride pad uns".split()
ENTRIES = {     # every argument by name, in the ABI's order
    "i8_stem_fused": _STEM + "N H W K R S stride uns".split() + _Q + ["stream"],
    "i8_stem_asym": _STEM + "w_off C N H W K R S stride uns".split() + _Q + ["stream"],
    "i8_stem_xoff": _STEM + "w_off C N H W K R S stride pad uns".split() + _Q + ["x_off", "x_tap", "stream"],
    "i8_stem_pool_fused": _STEM + "N H W K R S stride uns".split() + _Q + ["stream"],
    "dw_i8_nhwc": _DW + _Q + ["stream"],
    "dw_i8_nhwc_xoff": _DW + _Q + ["x_off", "x_tap", "stream"],
    "dwpw_i8_nhwc": ("x table dw_asym dw_bias dw_relu zp_in N H W C uns q_scale q_zp q_lo q_hi q_form g w bias wsum s_in s_w w_off K relu codes "
                     "q2_scale q2_zp q2_lo q2_hi q2_form g2 stream").split(),
    "i8_nhwc_gap": "x w out bias wsum s_in zp_in s_w N H W C K uns res relu".split() + _Q[1:] + ["stream"],
}
STEMS = ("i8_stem_fused", "i8_stem_asym", "i8_stem_xoff", "i8_stem_pool_fused")
DWS = ("dw_i8_nhwc", "dw_i8_nhwc_xoff")
_QB = dict(relu=1, codes=P, q_scale=P, q_zp=0, q_lo=0, q_hi=255, q_form=ZP, g=0.0, stream=0)
# a call every entry point accepts (H, W of the first layers: the padded buffer's Hp, Wp): each case adds a reason to refuse it, takes its rows
# away, or asks for its route
BASE = {
    "i8_stem_fused": dict(_QB, x=P, w=P, out=0, bias=0, wsum=P, s_in=P, zp_in=0, s_w=P, N=1, H=14, W=14, K=64, R=3, S=3, stride=2, uns=1),
    "i8_stem_asym": dict(_QB, x=P, w=P, out=0, bias=0, wsum=P, s_in=P, zp_in=0, s_w=P, w_off=P, C=3, N=1, H=14, W=14, K=64, R=3, S=3, stride=2, uns=1),
    "i8_stem_xoff": dict(_QB, x=P, w=P, out=0, bias=0, wsum=P, s_in=P, zp_in=0, s_w=P, w_off=0, C=3, N=1, H=14, W=14, K=64, R=3, S=3, stride=2, pad=1,
                         uns=1, x_off=P, x_tap=P),
    "i8_stem_pool_fused": dict(_QB, x=P, w=P, out=0, bias=0, wsum=P, s_in=P, zp_in=0, s_w=P, N=1, H=38, W=38, K=64, R=7, S=7, stride=2, uns=1),
    "dw_i8_nhwc": dict(_QB, x=P, w=P, out=0, bias=0, s_in=P, zp_in=0, s_w=P, w_off=0, N=1, H=16, W=16, C=64, R=3, S=3, stride=1, pad=1, uns=1),
    "dw_i8_nhwc_xoff": dict(_QB, x=P, w=P, out=0, bias=0, s_in=P, zp_in=0, s_w=P, w_off=0, N=1, H=16, W=16, C=64, R=3, S=3, stride=1, pad=1, uns=1,
                            x_off=P, x_tap=P),
    "dwpw_i8_nhwc": dict(x=P, table=P, dw_asym=0, dw_bias=0, dw_relu=1, zp_in=0, N=1, H=14, W=14, C=64, uns=1, q_scale=P, q_zp=0, q_lo=0, q_hi=255,
                         q_form=ZP, g=0.0, w=P, bias=0, wsum=P, s_in=P, s_w=P, w_off=0, K=128, relu=1, codes=P, q2_scale=P, q2_zp=0, q2_lo=0,
                         q2_hi=255, q2_form=ZP, g2=0.0, stream=0),
    "i8_nhwc_gap": dict(_QB, x=P, w=P, out=P, bias=0, wsum=P, s_in=P, zp_in=0, s_w=P, N=2, H=7, W=7, C=64, K=64, uns=1, res=0),
}
POINTERS = {e: [k for k in names if k in ("x w out bias wsum s_in zp_in s_w w_off codes q_scale q_zp x_off x_tap table q2_scale q2_zp res").split()]
            for e, names in ENTRIES.items()}
# ... the ones an accepted call may leave null, and the ones read 16 bytes at a time (the others: 4, or never through a vector access)
OPTIONAL = {e: [k for k in POINTERS[e] if k in ("out", "codes", "bias", "zp_in", "q_zp", "q2_zp", "w_off", "res")] for e in ENTRIES}
OPTIONAL["i8_stem_asym"].remove("w_off")
OPTIONAL["dwpw_i8_nhwc"].remove("codes")
ALIGN16 = dict({e: ["w", "out"] for e in STEMS}, dw_i8_nhwc=["s_w", "w_off", "bias", "out"], dw_i8_nhwc_xoff=["s_w", "w_off", "bias", "out", "x_tap"],
               dwpw_i8_nhwc=["x", "table", "w", "codes"], i8_nhwc_gap=["x", "w", "out", "res"])
ALIGN16["i8_stem_xoff"] = ["w", "out", "x_tap"]
# one more fault for a call that is otherwise accepted: a 16-byte pointer at P + 4, a size past the 32-bit bound
THEN_ALIGN = dict({e: dict(w=P4) for e in STEMS}, dw_i8_nhwc=dict(s_w=P4), dw_i8_nhwc_xoff=dict(s_w=P4), dwpw_i8_nhwc=dict(w=P4), i8_nhwc_gap=dict(w=P4))
THEN_ERANGE = dict({e: dict(H=46344, W=46344, stride=1) for e in STEMS}, dw_i8_nhwc=dict(N=1 << 20, H=64, W=64),
                   dw_i8_nhwc_xoff=dict(N=1 << 20, H=64, W=64), dwpw_i8_nhwc=dict(N=1 << 20, H=61, W=61), i8_nhwc_gap=dict(N=1 << 26))
ROUTES = {"dw_i8_nhwc": (ROUTE_DW, ROUTE_DWM), "dw_i8_nhwc_xoff": (ROUTE_DW, ROUTE_DWM), "i8_nhwc_gap": (ROUTE_GAP,)}


def call(lib, entry, case):
    a = dict(BASE[entry], **case)
    fn = getattr(lib, "dlmcq_conv2d_" + entry)
    assert len(ENTRIES[entry]) == len(fn.argtypes), entry
    return int(fn(*[(a[name] or None) if typ is ctypes.c_void_p else a[name] for name, typ in zip(ENTRIES[entry], fn.argtypes)]))


def answered_without_launch(entry, case, v):
    """What the sweep may hold: a refusal, DLMCQ_OK for a case with no rows, a route code for a case that asks for the route."""
    a = dict(BASE[entry], **case)
    return v < 0 or (v == OK and a["N"] == 0) or (v in ROUTES.get(entry, ()) and bool(a["q_form"] & ROUTE_ONLY))


def cases():
    """[(id, entry, overrides of BASE[entry])], deterministic.  The ids are the fixture's keys."""
    out = []

    def add(name, entry, *dicts, **kw):
        c = {}
        for d in dicts:
            c.update(d)
        c.update(kw)
        assert all(k in BASE[entry] for k in c), (entry, name, c)
        out.append((f"{entry}:{name}", entry, c))

    bad_q = (("scale_null", dict(q_scale=0)), ("lo_above_hi", dict(q_lo=5, q_hi=-5)), ("lo_below_-128", dict(q_lo=-129, q_hi=0)),
             ("hi_above_255", dict(q_hi=256)), ("span_above_255", dict(q_lo=-128, q_hi=255)), ("span_256", dict(q_lo=-1, q_hi=255)),
             ("form_below_emulate", dict(q_form=-1)), ("form_rootq", dict(q_form=ROOTQ)), ("form_5", dict(q_form=5)), ("form_255", dict(q_form=255)))
    good_q = (("signed", dict(q_lo=-128, q_hi=127)), ("span_255", dict(q_lo=-100, q_hi=155)), ("narrow", dict(q_lo=0, q_hi=15)),
              ("emulate", dict(q_form=0)), ("symmetric", dict(q_form=3)), ("zero_point", dict(q_zp=P)))
    for e in ENTRIES:
        then_align, then_erange = THEN_ALIGN[e], THEN_ERANGE[e]
        routed = e in ROUTES
        nulls = {k: 0 for k in POINTERS[e]}
        given = {k: P for k in POINTERS[e]}
        # ---- the empty problem, and what is looked at before it ----
        add("empty", e, N=0)
        add("empty/all_null", e, nulls, N=0)
        add("empty/all_misaligned", e, {k: P4 for k in POINTERS[e] if k != "x_tap"}, N=0)
        add("empty/bad_quantiser", e, N=0, q_lo=5, q_hi=-5, q_form=77)
        add("empty/relu6", e, N=0, relu=2)
        if e != "i8_nhwc_gap":
            add("empty/no_outputs", e, N=0, **({"codes": 0} if e == "dwpw_i8_nhwc" else {"out": 0, "codes": 0}))
        # ---- every required pointer null in turn; the optional ones given ----
        for k in POINTERS[e]:
            if k not in OPTIONAL[e]:
                add(f"null/{k}", e, **{k: 0})
        if e != "dwpw_i8_nhwc":
            add("null/out_and_codes", e, out=0, codes=0)
            add("null/codes/then_align", e, then_align, out=P, codes=0)
            add("null/codes_and_q_scale/then_align", e, then_align, out=P, codes=0, q_scale=0)
            add("given/out_and_codes/then_align", e, then_align, out=P)
        add("given/every_pointer/then_align", e, given, then_align)
        add("given/every_pointer/then_erange", e, given, then_erange)
        for k in OPTIONAL[e]:
            if k not in ("out", "codes"):
                add(f"given/{k}/then_align", e, then_align, **{k: P})
        # ---- the pointers read 16 bytes at a time at P + 4; the others get past the check, onto the size bound ----
        for k in POINTERS[e]:
            if k in ALIGN16[e]:
                add(f"align/{k}", e, **{k: P4})
            else:
                add(f"align/{k}_is_free/then_erange", e, then_erange, **{k: P4})
        # ---- the quantiser's arguments: refused with `codes`, not looked at without (the pooled head: its form always) ----
        q = "q2_" if e == "dwpw_i8_nhwc" else "q_"
        ren = (lambda d: {k.replace("q_", q): v for k, v in d.items()})
        for tag, kw in bad_q:
            add(f"quant/{tag}", e, ren(kw))
            add(f"quant/{tag}/before_align", e, ren(kw), then_align)
            add(f"quant/{tag}/before_erange", e, ren(kw), then_erange)
            if e != "dwpw_i8_nhwc":
                add(f"quant/{tag}/no_codes/then_align", e, kw, then_align, out=P, codes=0)
        for tag, kw in good_q:
            add(f"quant/{tag}/then_align", e, ren(kw), then_align)
            if routed:
                add(f"quant/{tag}/route", e, kw, q_form=kw.get("q_form", ZP) | ROUTE_ONLY)
        # ---- every bit of `q_form` alone, with `codes` and without ----
        for bit, b in BITS.items():
            for form in ("q_form", "q2_form") if e == "dwpw_i8_nhwc" else ("q_form",):
                launches = e in DWS and bit == "FORCE_TILED"      # (taken, and the call then runs)
                if not launches and not (e == "i8_nhwc_gap" and bit == "SHIFT128"):
                    add(f"bit/{form}/{bit}", e, **{form: ZP | b})
                add(f"bit/{form}/{bit}/then_align", e, then_align, **{form: ZP | b})
                add(f"bit/{form}/{bit}/then_erange", e, then_erange, **{form: ZP | b})
                if e != "dwpw_i8_nhwc":
                    add(f"bit/{form}/{bit}/no_codes/then_align", e, then_align, out=P, codes=0, **{form: ZP | b})
                    add(f"bit/{form}/{bit}/no_codes/then_erange", e, then_erange, out=P, codes=0, **{form: ZP | b})
                else:
                    add(f"bit/{form}/{bit}/no_codes", e, codes=0, **{form: ZP | b})
                if routed and bit != "ROUTE_ONLY":
                    add(f"bit/{form}/{bit}/route", e, **{form: ZP | b | ROUTE_ONLY})
                    add(f"bit/{form}/{bit}/no_codes/route", e, out=P, codes=0, **{form: ZP | b | ROUTE_ONLY})
        add("bit/q_form/SHIFT128/signed_range/then_align", e, then_align, q_form=ZP | BITS["SHIFT128"], q_lo=-5, q_hi=5)
        if e != "dwpw_i8_nhwc":
            add("bit/q_form/SHIFT128/signed_range/no_codes/then_align", e, then_align, out=P, codes=0, q_form=ZP | BITS["SHIFT128"], q_lo=-5, q_hi=5)
        # ---- the order of the checks, where two codes tell ----
        first_required = [k for k in POINTERS[e] if k not in OPTIONAL[e]][-1]
        add("order/null_before_align", e, then_align, **{first_required: 0})
        add("order/null_before_erange", e, then_erange, **{first_required: 0})
        add("order/align_before_erange", e, then_align, then_erange)
        add("order/empty_before_erange", e, then_erange, N=0)
        if routed:
            add("route", e, q_form=ZP | ROUTE_ONLY)
            add("route/no_codes", e, out=P, codes=0, q_form=ZP | ROUTE_ONLY)
            add("route/empty", e, N=0, q_form=ZP | ROUTE_ONLY)
            add("order/null_before_route", e, q_form=ZP | ROUTE_ONLY, **{first_required: 0})
            add("order/align_before_route", e, then_align, q_form=ZP | ROUTE_ONLY)
            add("order/erange_before_route", e, then_erange, q_form=ZP | ROUTE_ONLY)
            add("order/bad_quantiser_before_route", e, q_form=ZP | ROUTE_ONLY, q_lo=5, q_hi=-5)

    # ---- the first layers: geometry ----
    for e in STEMS:
        for tag, kw in (("N_negative", dict(N=-1)), ("Hp_0", dict(H=0)), ("Wp_0", dict(W=0)), ("K_0", dict(K=0)), ("K_negative", dict(K=-4)),
                        ("R_0", dict(R=0)), ("R_8", dict(R=8)), ("S_0", dict(S=0)), ("S_9", dict(S=9)), ("stride_0", dict(stride=0)),
                        ("stride_negative", dict(stride=-1)), ("Hp_below_R", dict(H=6, R=7)), ("Wp_below_S", dict(W=6, S=7)), ("K_6", dict(K=6)),
                        ("K_66", dict(K=66))):
            add("range/" + tag, e, kw)
            add("range/" + tag + "/empty", e, kw, N=0 if "N" not in kw else kw["N"])
            add("range/" + tag + "/before_align", e, kw, THEN_ALIGN[e])
        for tag, kw in (("R_1_S_1", dict(R=1, S=1)), ("R_7_S_8", dict(R=7, S=8)), ("K_4", dict(K=4)), ("K_68", dict(K=68)), ("K_128", dict(K=128)),
                        ("Hp_equals_R", dict(H=7, R=7, S=7, W=38)), ("relu_none", dict(relu=0)), ("relu6", dict(relu=2)), ("signed_input", dict(uns=0))):
            if not (e == "i8_stem_xoff" and tag == "R_1_S_1") and not (e == "i8_stem_pool_fused" and tag in ("K_68", "K_128", "relu6")):   # (their own refusals, below)
                add("shape/" + tag + "/then_align", e, kw, THEN_ALIGN[e])
        add("erange/M_2^31", e, H=46344, W=46344, stride=1)
        add("erange/buffer_2^31", e, H=46344, W=46344, stride=2)
        add("erange/just_below/then_nothing_but_align", e, THEN_ALIGN[e], H=46340, W=46340, stride=1)
        add("erange/N_2^31", e, N=1 << 31)
    for e in ("i8_stem_asym", "i8_stem_xoff"):
        for tag, kw in (("C_0", dict(C=0)), ("C_5", dict(C=5)), ("C_negative", dict(C=-1))):
            add("range/" + tag, e, kw)
            add("range/" + tag + "/empty", e, kw, N=0)
        add("shape/C_1/then_align", e, THEN_ALIGN[e], C=1)
        add("shape/C_4/then_align", e, THEN_ALIGN[e], C=4)
    add("null/w_off/empty", "i8_stem_asym", w_off=0, N=0)
    add("null/w_off/before_align", "i8_stem_asym", THEN_ALIGN["i8_stem_asym"], w_off=0)
    e = "i8_stem_xoff"
    for tag, kw in (("pad_negative", dict(pad=-1)), ("pad_half_of_Hp", dict(pad=7)), ("pad_half_of_Wp", dict(pad=5, W=10)), ("R_5_padded", dict(R=5, S=5)),
                    ("R_1_padded", dict(R=1, S=1)), ("x_off_null/unpadded", dict(x_off=0, pad=0)), ("x_tap_null/unpadded", dict(x_tap=0, pad=0))):
        add("range/" + tag, e, kw)
        add("range/" + tag + "/empty", e, kw, N=0)
        add("range/" + tag + "/tap_sums_misaligned", e, kw, x_tap=kw.get("x_tap", P4))
    add("shape/R_5_unpadded/then_align", e, THEN_ALIGN[e], R=5, S=5, pad=0)
    add("shape/R_7_padded/then_align", e, THEN_ALIGN[e], R=7, S=7, pad=3, H=38, W=38)
    add("shape/asymmetric/then_align", e, THEN_ALIGN[e], w_off=P)
    add("order/tap_sums_misaligned/before_empty", e, x_tap=P4, N=0)
    add("order/tap_sums_misaligned/before_range", e, x_tap=P4, K=6)
    add("order/tap_sums_misaligned/before_null", e, x_tap=P4, wsum=0)
    add("order/tap_sums_misaligned/unpadded", e, x_tap=P4, pad=0)
    add("order/offset_null/before_tap_sums_misaligned", e, x_tap=P4, x_off=0)
    e = "i8_stem_pool_fused"
    add("range/relu6", e, relu=2)
    add("range/relu6/before_align", e, THEN_ALIGN[e], relu=2)
    add("range/relu6/before_erange", e, THEN_ERANGE[e], relu=2)
    add("range/K_68/before_align", e, THEN_ALIGN[e], K=68)
    add("range/K_128", e, K=128)
    add("range/K_128/empty", e, K=128, N=0)
    for tag, kw in (("not_pool7/R_3", dict(R=3, S=3, H=14, W=14)), ("not_pool7/K_32", dict(K=32)), ("not_pool7/stride_1", dict(stride=1)),
                    ("not_pool7/odd_P", dict(H=40, W=40)), ("not_pool7/out", dict(out=P)), ("pool7", dict())):
        add("shape/" + tag + "/then_align", e, kw, THEN_ALIGN[e])
        add("shape/" + tag + "/then_erange", e, kw, N=1 << 24)

    # ---- depthwise: geometry, then the dispatch through route queries ----
    R_ = dict(q_form=ZP | ROUTE_ONLY)
    for e in DWS:
        for tag, kw in (("N_negative", dict(N=-1)), ("H_0", dict(H=0)), ("W_0", dict(W=0)), ("C_0", dict(C=0)), ("C_2", dict(C=2)), ("C_6", dict(C=6)),
                        ("R_0", dict(R=0)), ("S_0", dict(S=0)), ("R_8", dict(R=8)), ("S_8", dict(S=8)), ("stride_0", dict(stride=0)),
                        ("pad_negative", dict(pad=-1)), ("P_0", dict(H=1, R=3, pad=0)), ("Q_0", dict(W=2, S=5, pad=1))):
            add("range/" + tag, e, kw)
            add("range/" + tag + "/empty", e, kw, N=0 if "N" not in kw else kw["N"])
            add("range/" + tag + "/route", e, kw, R_)
            add("range/" + tag + "/before_align", e, kw, THEN_ALIGN[e])
        add("erange/output", e, N=1 << 20, H=64, W=64)
        add("erange/input_only", e, N=1 << 17, H=64, W=64, stride=4)
        add("erange/input_only/route", e, R_, N=1 << 17, H=64, W=64, stride=4)
        add("erange/just_below/route", e, R_, N=(1 << 15) - 1, H=64, W=64)
        xoff = e.endswith("xoff")
        dwm = dict(R_, N=16, H=16, W=16)           # the matrix-core kernel's layer: 3 x 3 / 1 / 1, codes only, plain quantiser, 4096 positions
        for tag, kw in (("base", {}), ("W_13", dict(N=1, H=316, W=13)), ("W_14", dict(N=1, H=293, W=14)), ("positions_4095", dict(N=13, H=21, W=15)),
                        ("positions_4096", dict(N=4, H=32, W=32)), ("C_32", dict(C=32)), ("C_64", dict(C=64)), ("C_96", dict(C=96)), ("C_128", dict(C=128)),
                        ("C_2112", dict(C=2112)), ("halo_20_pieces", dict(N=2, H=64, W=62)), ("halo_21_pieces", dict(N=2, H=64, W=63)),
                        ("out_given", dict(out=P)), ("out_only", dict(out=P, codes=0)), ("zero_point", dict(q_zp=P)), ("narrowed_range", dict(q_hi=127)),
                        ("signed_range", dict(q_lo=-128, q_hi=127)), ("codes_4_aligned", dict(codes=P4)), ("x_4_aligned", dict(x=P4)),
                        ("force_tiled", dict(q_form=ZP | ROUTE_ONLY | FORCE_TILED)), ("5x5", dict(R=5, S=5, pad=2)), ("3x5", dict(S=5)),
                        ("stride_2", dict(stride=2)), ("pad_0", dict(pad=0)), ("pad_2", dict(pad=2)), ("relu6", dict(relu=2)), ("relu_none", dict(relu=0)),
                        ("asymmetric", dict(w_off=P)), ("bias", dict(bias=P)), ("input_zero_point", dict(zp_in=P)), ("signed_input", dict(uns=0)),
                        ("emulate", dict(q_form=0 | ROUTE_ONLY)), ("offsets_below_bound", dict(N=32766, H=32, W=32)),
                        ("offsets_at_bound", dict(N=32767, H=32, W=32))):
            add("dwm/" + tag, e, dwm, kw)
        # `wide` (the 3 x 3 kernels) shows only where a float offset needs it: the _xoff entry point with padding refuses anything else
        for tag, kw in (("C_16", dict(C=16)), ("C_24", dict(C=24)), ("C_2048", dict(C=2048)), ("C_2064", dict(C=2064)), ("x_4_aligned", dict(x=P4)),
                        ("codes_4_aligned", dict(codes=P4)), ("out_only", dict(out=P, codes=0)), ("out_only_codes_null_x_4_aligned", dict(out=P, codes=0, x=P4)),
                        ("5x5", dict(R=5, S=5, pad=2)), ("3x5", dict(S=5)), ("5x3", dict(R=5)), ("stride_2", dict(stride=2)), ("pad_2", dict(pad=2)),
                        ("unpadded_C_24", dict(C=24, pad=0, H=18, W=18)), ("unpadded_5x5", dict(R=5, S=5, pad=0))):
            add("wide/" + tag + "/route", e, R_, kw)
            if xoff:
                add("wide/" + tag + "/then_align", e, kw, THEN_ALIGN[e])
                add("wide/" + tag + "/then_erange", e, kw, N=1 << 24)
    e = "dw_i8_nhwc_xoff"
    for tag, kw in (("x_off_null", dict(x_off=0)), ("x_tap_null", dict(x_tap=0)), ("x_off_null/unpadded", dict(x_off=0, pad=0, H=18, W=18))):
        add("range/" + tag, e, kw)
        add("range/" + tag + "/empty", e, kw, N=0)
        add("range/" + tag + "/route", e, kw, R_)
        add("range/" + tag + "/tap_sums_misaligned", e, kw, x_tap=kw.get("x_tap", P4))
    add("order/tap_sums_misaligned/before_empty", e, x_tap=P4, N=0)
    add("order/tap_sums_misaligned/before_range", e, x_tap=P4, C=6)
    add("order/tap_sums_misaligned/before_route", e, R_, x_tap=P4)
    add("order/tap_sums_misaligned/unpadded", e, x_tap=P4, pad=0, H=18, W=18)
    add("order/not_wide/after_erange", e, C=24, N=1 << 24)
    add("order/not_wide/after_align", e, THEN_ALIGN[e], C=24)
    add("order/not_wide/before_route", e, R_, C=24)
    add("order/dwm_never_with_offset/route", e, R_, N=16, H=16, W=16)
    add("order/dwm_with_unpadded_offset_is_not_dwm/route", e, R_, N=16, H=18, W=18, pad=0)

    # ---- depthwise + pointwise ----
    e = "dwpw_i8_nhwc"
    for tag, kw in (("dw_relu6", dict(dw_relu=2)), ("relu6", dict(relu=2)), ("N_negative", dict(N=-1)), ("H_0", dict(H=0)), ("W_0", dict(W=0)), ("C_0", dict(C=0)),
                    ("C_32", dict(C=32)), ("C_96", dict(C=96)), ("K_0", dict(K=0)), ("K_64", dict(K=64)), ("K_256", dict(K=256)), ("K_130", dict(K=130))):
        add("range/" + tag, e, kw)
        add("range/" + tag + "/empty", e, kw, N=0 if "N" not in kw else kw["N"])
        add("range/" + tag + "/before_align", e, kw, THEN_ALIGN[e])
    for tag, kw in (("K_192", dict(K=192)), ("K_512", dict(K=512)), ("C_128", dict(C=128)), ("relu_none", dict(relu=0, dw_relu=0)), ("dw_flags", dict(dw_asym=1, dw_bias=1)),
                    ("signed_input", dict(uns=0)), ("W_62", dict(W=62))):
        add("shape/" + tag + "/then_align", e, kw, THEN_ALIGN[e])
    for tag, kw in (("lo_1", dict(q_lo=1)), ("hi_254", dict(q_hi=254)), ("signed", dict(q_lo=-128, q_hi=127)), ("lo_above_hi", dict(q_lo=5, q_hi=-5))):
        add("first_quantiser/" + tag, e, kw)
        add("first_quantiser/" + tag + "/before_align", e, kw, THEN_ALIGN[e])
        add("first_quantiser/" + tag + "/empty", e, kw, N=0)
    for tag, kw in (("form_below_emulate", dict(q_form=-1)), ("form_rootq", dict(q_form=ROOTQ)), ("form_5", dict(q_form=5))):
        add("first_quantiser/" + tag, e, kw)
        add("first_quantiser/" + tag + "/after_align", e, kw, THEN_ALIGN[e])
        add("first_quantiser/" + tag + "/before_erange", e, kw, THEN_ERANGE[e])
    for tag, kw in (("emulate", dict(q_form=0)), ("symmetric", dict(q_form=3))):
        add("first_quantiser/" + tag + "/then_erange", e, kw, THEN_ERANGE[e])
    add("order/align_before_second_quantiser", e, THEN_ALIGN[e], q2_lo=5, q2_hi=-5)
    add("order/null_before_first_quantiser_range", e, q_lo=1, wsum=0)
    add("erange/frame_2^31", e, N=1 << 20, H=61, W=61)
    add("erange/offsets_2^40", e, N=1024, H=32, W=32, C=1 << 20)
    add("range/W_63", e, W=63)
    add("range/W_63/after_align", e, THEN_ALIGN[e], W=63)
    add("order/erange_before_W_63", e, N=1 << 20, H=63, W=63)
    add("order/second_quantiser_before_W_63", e, W=63, q2_hi=256)

    # ---- the pooled head ----
    e = "i8_nhwc_gap"
    for tag, kw in (("N_negative", dict(N=-1)), ("H_0", dict(H=0)), ("W_0", dict(W=0)), ("C_0", dict(C=0)), ("K_0", dict(K=0)), ("HW_72", dict(H=9, W=8)),
                    ("H_65", dict(H=65, W=1)), ("W_65", dict(H=1, W=65)), ("C_32", dict(C=32)), ("C_2112", dict(C=2112)), ("K_32", dict(K=32)),
                    ("K_96", dict(K=96)), ("K_2^24", dict(K=1 << 24)), ("act_3", dict(relu=3)), ("act_negative", dict(relu=-1))):
        add("range/" + tag, e, kw)
        add("range/" + tag + "/empty", e, kw, N=0 if "N" not in kw else kw["N"])
        add("range/" + tag + "/route", e, kw, R_)
        add("range/" + tag + "/before_align", e, kw, THEN_ALIGN[e])
    for tag, kw in (("HW_64", dict(H=8, W=8)), ("HW_1", dict(H=1, W=1)), ("C_2048", dict(C=2048)), ("K_128", dict(K=128)), ("K_2^24-64", dict(K=(1 << 24) - 64)),
                    ("act_none", dict(relu=0)), ("relu6", dict(relu=2)), ("shortcut", dict(res=P)), ("codes_only", dict(out=0)), ("pooled_only", dict(codes=0)),
                    ("codes_4_aligned", dict(codes=P4)), ("shifted", dict(q_form=ZP | BITS["SHIFT128"])), ("signed_input", dict(uns=0))):
        add("shape/" + tag + "/route", e, kw, q_form=kw.get("q_form", ZP) | ROUTE_ONLY)
    for tag, kw in bad_q:
        add(f"quant/{tag}/empty", e, kw, N=0)
        add(f"quant/{tag}/no_codes/route", e, kw, out=P, codes=0, q_form=kw.get("q_form", ZP) | ROUTE_ONLY if kw.get("q_form", ZP) >= 0 else -1)
    add("quant/shifted_signed", e, q_form=ZP | BITS["SHIFT128"], q_lo=-5, q_hi=5)
    add("quant/shifted_signed/no_codes/route", e, out=P, codes=0, q_form=ZP | BITS["SHIFT128"] | ROUTE_ONLY, q_lo=-5, q_hi=5)
    add("quant/shifted_hi_256/no_codes/route", e, out=P, codes=0, q_form=ZP | BITS["SHIFT128"] | ROUTE_ONLY, q_hi=256)
    for bit in ("FORCE_TILED", "PIPELINED", "FP32_IN_CHUNK_MAJOR", "FP32_OUT_CHUNK_MAJOR", "ROUTE_VARIANT", "ROUTE_HALO_VARIANT", "W2_CHUNK_MAJOR"):
        add(f"bit/q_form/{bit}/empty", e, N=0, q_form=ZP | BITS[bit])
    add("bit/q_form/ROUTE_ONLY_and_SHIFT128/empty", e, N=0, q_form=ZP | ROUTE_ONLY | BITS["SHIFT128"])
    add("erange/N_2^26", e, N=1 << 26)
    add("erange/just_below/route", e, R_, N=(1 << 25) - 1, H=8, W=8)
    assert len({c[0] for c in out}) == len(out), "duplicate case id"
    return out


def hidden_gpu_count():
    """The HIP runtime's device count, or -1 when it answers with an error (the runtime torch ships: the one the library binds to)."""
    import torch
    rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    hip = ctypes.CDLL(rt if os.path.exists(rt) else "libamdhip64.so", mode=ctypes.RTLD_GLOBAL)
    n = ctypes.c_int(0)
    return n.value if hip.hipGetDeviceCount(ctypes.byref(n)) == 0 else -1


def child(path):
    """Runs in the child process: {"results": {id: value}} or {"skipped": why} as one JSON line on stdout."""
    got = cases()
    if os.environ.get("HIP_VISIBLE_DEVICES") != "-1" or hidden_gpu_count() > 0:
        print(json.dumps({"skipped": "the HIP runtime still sees a GPU: no call was made"}))
        return
    sys.path.insert(0, os.path.join(ROOT, "dlmc-quant_amd"))
    from dlmc import _native as N
    lib = N.lib
    if path:
        lib = ctypes.CDLL(os.path.abspath(path))
        for name in ENTRIES:
            fn = getattr(lib, "dlmcq_conv2d_" + name)
            fn.restype, fn.argtypes = N.SIGNATURES["dlmcq_conv2d_" + name]
    print(json.dumps({"results": {cid: call(lib, entry, kw) for cid, entry, kw in got}}))


def run(path=None):
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + ([path] if path else []), env=env, check=True,
                         capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def test_every_case_answers_as_the_fixture_records():
    """Exact: no tolerance, no case left out, none added without regenerating."""
    import pytest
    with open(FIXTURE) as f:
        want = json.load(f)["results"]
    got = run()
    if "skipped" in got:
        pytest.skip(got["skipped"])
    got = got["results"]
    assert sorted(got) == sorted(want), "the case generator and the fixture disagree on the cases: regenerate with the PARENT library"
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f"{len(wrong)} of {len(want)} calls answer differently (got, fixture): {dict(list(wrong.items())[:12])}"


def test_the_fixture_holds_no_launch_and_reaches_every_refusal():
    """Checked on the fixture, so a generator that drifts away from a refusal - or towards a launch - fails."""
    with open(FIXTURE) as f:
        want = json.load(f)["results"]
    all_cases = {cid: (entry, kw) for cid, entry, kw in cases()}
    assert sorted(all_cases) == sorted(want) and len(want) >= 1500
    for cid, v in want.items():
        assert answered_without_launch(*all_cases[cid], v), f"{cid} = {v}: an accepted call"
    per_entry = {}
    for k, v in want.items():
        per_entry.setdefault(k.split(":")[0], set()).add(v)
    every = {OK, EINVAL, ERANGE, EALIGN}
    # (a float offset never runs on the matrix-core kernel, and without padding - no offset term - the layer is not that kernel's)
    assert per_entry == {e: every | (set(ROUTES.get(e, ())) - ({ROUTE_DWM} if e == "dw_i8_nhwc_xoff" else set())) for e in ENTRIES}
    for cid, v in want.items():          # whole groups at one code
        e, name = cid.split(":", 1)
        name = name.split("/")
        if name[0] in ("range", "null") and name[-1] not in ("tap_sums_misaligned", "then_align", "after_align"):
            assert v == EINVAL, cid
        elif name[0] == "first_quantiser" and (len(name) == 2 or name[-1] in ("before_align", "before_erange")):
            assert v == EINVAL, cid
        elif name[0] == "align":
            assert v == (ERANGE if name[-1] == "then_erange" else EALIGN), cid
        elif name[0] == "erange":
            assert v == (ERANGE if name[-1] != "route" and "just_below" not in name else v), cid
            assert v in (ERANGE, EALIGN) + ROUTES.get(e, ()), cid
        elif name[0] == "given" or name[0] == "shape":
            assert v == (EALIGN if name[-1] == "then_align" else ERANGE if name[-1] == "then_erange" else ROUTES[e][0]), cid
        elif name[0] == "quant" and name[1] in ("signed", "span_255", "narrow", "emulate", "symmetric", "zero_point"):
            assert v == (EALIGN if name[-1] == "then_align" else ROUTES[e][0]), cid
        elif name[0] == "quant" and "no_codes" not in name and "shifted" not in name[1]:
            # (dwpw looks at its pointers' alignment before its second quantiser)
            assert v == (EALIGN if e == "dwpw_i8_nhwc" and name[-1] == "before_align" and name[1] != "scale_null" else EINVAL), cid
        elif name[0] == "dwm":       # (with a float offset: never the matrix cores, and a padded layer that is not 3 x 3 is refused)
            assert v in ((ROUTE_DW, ROUTE_DWM) if e == "dw_i8_nhwc" else (ROUTE_DW, EINVAL)), cid
    dwm = {k.split("dwm/")[1] for k, v in want.items() if k.startswith("dw_i8_nhwc:dwm/") and v == ROUTE_DWM}
    assert dwm == {"base", "W_14", "positions_4096", "C_64", "C_128", "C_2112", "halo_20_pieces", "relu6", "relu_none", "asymmetric", "bias",
                   "input_zero_point", "signed_input", "emulate", "offsets_below_bound"}
    assert not [k for k, v in want.items() if k.startswith("dw_i8_nhwc_xoff:") and v == ROUTE_DWM]       # a float offset never runs there
    named = {  # the order of the checks, where two codes tell; and which `q_form` bits an entry point takes
        "i8_stem_fused:order/null_before_align": EINVAL, "i8_stem_fused:order/align_before_erange": EALIGN, "i8_stem_fused:order/empty_before_erange": OK,
        "i8_stem_fused:quant/lo_above_hi/before_align": EINVAL, "i8_stem_fused:quant/lo_above_hi/no_codes/then_align": EALIGN,
        "i8_stem_xoff:order/tap_sums_misaligned/before_empty": EALIGN, "i8_stem_xoff:order/tap_sums_misaligned/before_range": EALIGN,
        "i8_stem_xoff:order/offset_null/before_tap_sums_misaligned": EINVAL, "i8_stem_xoff:shape/R_5_unpadded/then_align": EALIGN,
        "i8_stem_pool_fused:range/relu6/before_erange": EINVAL, "i8_stem_pool_fused:order/align_before_erange": EALIGN,
        "i8_stem_fused:bit/q_form/SHIFT128/then_align": EINVAL, "i8_stem_fused:bit/q_form/ROUTE_ONLY/then_align": EINVAL,
        "i8_stem_pool_fused:bit/q_form/FORCE_TILED/then_align": EINVAL,
        "dw_i8_nhwc:bit/q_form/SHIFT128/then_align": EINVAL, "dw_i8_nhwc:bit/q_form/PIPELINED/route": EINVAL,
        "dw_i8_nhwc:bit/q_form/FORCE_TILED/then_align": EALIGN, "dw_i8_nhwc:bit/q_form/FORCE_TILED/route": ROUTE_DW, "dw_i8_nhwc:route": ROUTE_DW,
        "dw_i8_nhwc:order/erange_before_route": ERANGE, "dw_i8_nhwc:order/align_before_route": EALIGN, "dw_i8_nhwc:route/empty": OK,
        "dw_i8_nhwc_xoff:order/not_wide/before_route": EINVAL, "dw_i8_nhwc_xoff:order/not_wide/after_erange": ERANGE,
        "dw_i8_nhwc_xoff:order/not_wide/after_align": EALIGN, "dw_i8_nhwc_xoff:wide/C_2048/route": ROUTE_DW, "dw_i8_nhwc_xoff:wide/C_2064/route": EINVAL,
        "dw_i8_nhwc_xoff:wide/C_24/route": EINVAL, "dw_i8_nhwc_xoff:wide/x_4_aligned/route": EINVAL, "dw_i8_nhwc_xoff:wide/codes_4_aligned/route": EINVAL,
        "dw_i8_nhwc_xoff:wide/out_only_codes_null_x_4_aligned/route": EINVAL, "dw_i8_nhwc_xoff:wide/out_only/route": ROUTE_DW,
        "dw_i8_nhwc_xoff:wide/unpadded_C_24/route": ROUTE_DW, "dw_i8_nhwc:wide/C_24/route": ROUTE_DW,
        "dwpw_i8_nhwc:bit/q_form/SHIFT128/then_erange": EINVAL, "dwpw_i8_nhwc:bit/q2_form/SHIFT128/then_erange": EINVAL,
        "dwpw_i8_nhwc:bit/q2_form/ROUTE_ONLY": EINVAL, "dwpw_i8_nhwc:order/align_before_second_quantiser": EALIGN,
        "dwpw_i8_nhwc:first_quantiser/lo_1/before_align": EINVAL, "dwpw_i8_nhwc:first_quantiser/form_5/after_align": EALIGN,
        "dwpw_i8_nhwc:order/erange_before_W_63": ERANGE, "dwpw_i8_nhwc:range/W_63/after_align": EALIGN,
        "i8_nhwc_gap:bit/q_form/SHIFT128/route": ROUTE_GAP, "i8_nhwc_gap:bit/q_form/FORCE_TILED/route": EINVAL, "i8_nhwc_gap:route": ROUTE_GAP,
        "i8_nhwc_gap:quant/lo_above_hi/empty": EINVAL, "i8_nhwc_gap:quant/lo_above_hi/no_codes/route": ROUTE_GAP,
        "i8_nhwc_gap:quant/form_5/no_codes/route": EINVAL, "i8_nhwc_gap:quant/shifted_signed/no_codes/route": EINVAL,
        "i8_nhwc_gap:order/erange_before_route": ERANGE, "i8_nhwc_gap:bit/q_form/PIPELINED/empty": EINVAL,
    }
    assert {k: want[k] for k in named} == named


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2] if len(sys.argv) > 2 else None)
    else:           # python tests/test_dw_stem_refusals_host.py --write LIBRARY [COMMIT]: the fixture, from that library
        assert sys.argv[1] == "--write"
        results = run(sys.argv[2])["results"]
        all_cases = {cid: (entry, kw) for cid, entry, kw in cases()}
        for cid, v in results.items():
            assert answered_without_launch(*all_cases[cid], v), f"{cid} = {v}: the library accepted the call - it does not belong in this sweep"
        header = ("Return values of dlmcq_conv2d_i8_stem_fused / _stem_asym / _stem_xoff / _stem_pool_fused, dlmcq_conv2d_dw_i8_nhwc / _xoff, "
                  "dlmcq_conv2d_dwpw_i8_nhwc and dlmcq_conv2d_i8_nhwc_gap for the cases of tests/test_dw_stem_refusals_host.py, recorded from the "
                  "library built at commit %s - the parent of the commit that rewrote these hosts around one call record and one kernel table per "
                  "family - by `python tests/test_dw_stem_refusals_host.py --write LIBRARY COMMIT`.  0: DLMCQ_OK (an empty problem); negative: a "
                  "refusal; 5 / 6 / 8: the answer of a DLMCQ_ROUTE_ONLY query.  No call in it launches." % (sys.argv[3] if len(sys.argv) > 3 else "?"))
        with open(FIXTURE, "w") as f:
            json.dump({"header": header, "results": results}, f, indent=0, sort_keys=True)
            f.write("\n")
        print(len(results), "cases;", {v: list(results.values()).count(v) for v in sorted(set(results.values()))})
