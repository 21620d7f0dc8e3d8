"""The chain kernels' host side (csrc/conv_chain_i8.hip: chain_launch and the three entry points in front of it), pinned from outside:
the integer `dlmcq_conv2d_i8_nhwc_chain`, `..._dual_chain` and `..._recompute_chain` return for a sweep of calls on placeholder pointers
must equal tests/golden/chain_refusals.json exactly, case for case.  The fixture was written by this file's own generator
(`python tests/test_chain_refusals_host.py --write LIBRARY COMMIT`) against the library built from the commit BEFORE the host side was
rewritten around one call record (ChainCall); its `header` names that commit.  A rewrite that changes a refusal's code, or the order two
refusals are checked in, fails here.

The sweep makes no route query (DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_CHAIN_VARIANT: tests/test_chain_variants_host.py; either bit alone is a refusal, and
ROUTE_ONLY alone is in it), so it holds ONLY calls that are answered without a launch: every refusal, and the
empty problem (DLMCQ_OK before any pointer is looked at).  No accepted call is in it - the generator asserts that every recorded value
is negative or belongs to a case with no rows - and the calls are made in a child process that hides the GPUs (HIP_VISIBLE_DEVICES=-1)
and first asks the HIP runtime for its device count: it makes no library call unless the answer is zero or an error.  A regression that
accepts a refused call therefore shows up as a wrong status code, never as a launch on a placeholder address.

Many refusals share DLMCQ_EINVAL, so the order of the checks is pinned where two codes differ: the `order/` cases carry two faults at
once (null and misaligned, misaligned and ReLU6, the multi-operand forms' range bounds and a later refusal, a later refusal and the
32-bit offset bound, that bound and the tile height / an unsupported shape).

The shapes expected to be refused as unsupported are the complement of kernels.CHAIN_SHAPES / DUAL_CHAIN_SHAPES / RECOMPUTE_CHAIN_SHAPES:
the fixture answering DLMCQ_EINVAL for exactly those ties the Python sets to the library's table of instantiations."""
import ctypes
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "chain_refusals.json")

OK, EINVAL, ERANGE, EALIGN = 0, -1, -2, -4
ZP, ROOTQ, SHIFT128, W2_CM, FORCE_TILED, ROUTE_ONLY, PIPELINED, IN_CM, OUT_CM = 2, 4, 0x100, 0x200, 0x400, 0x800, 0x1000, 0x2000, 0x4000
P = 4096            # a placeholder pointer: non-null, 16-byte aligned, never dereferenced
P4 = P + 4          # 4-byte aligned only

# every argument of the three entry points by name (operand `a`: the recomputed block's unit-stride one, `b`: the sampled one of
# both multi-operand forms, `2`: the second layer); an entry point marshals the ones it has.  The plain form's M is N * H * W.
BASE = dict(x=P, w=P, out=P, bias=0, wsum=P, s_in=P, zp_in=0, s_w=P, N=1, H=7, W=7, C=64, K=64, uns=1, res=P,
            xa=P, wa=P, biasa=0, wsuma=P, s_ina=P, zp_ina=0, s_wa=P, Ca=64, unsa=1,
            xb=P, wb=P, biasb=0, wsumb=P, s_inb=P, zp_inb=0, s_wb=P, Hb=7, Wb=7, Cb=64, strideb=1, unsb=1, relu_sc=1,
            relu=1, codes=P, q_scale=P, q_zp=0, q_lo=0, q_hi=255, q_form=ZP, g=0.0,
            w2=P, bias2=0, wsum2=P, s_w2=P, K2=64, relu2=1, codes2=P, q2_scale=P, q2_zp=0, q2_lo=0, q2_hi=255, q2_form=ZP, g2=0.0,
            rpt=0, stream=0)
_OWN = "x w out bias wsum s_in zp_in s_w".split()
_B = "xb wb biasb wsumb s_inb zp_inb s_wb Hb Wb Cb strideb unsb".split()
_TAIL = ("relu codes q_scale q_zp q_lo q_hi q_form g w2 bias2 wsum2 s_w2 K2 relu2 codes2 q2_scale q2_zp q2_lo q2_hi q2_form g2 "
         "rpt stream").split()
ENTRIES = {
    "chain": _OWN + "M C K uns res".split() + _TAIL,
    "dual_chain": _OWN + "N H W C K uns".split() + _B + _TAIL,
    "recompute_chain": _OWN + "N H W C K uns".split() + "xa wa biasa wsuma s_ina zp_ina s_wa Ca unsa".split() + _B + ["relu_sc"] + _TAIL,
}
MULTI = ("dual_chain", "recompute_chain")


def rows(case):
    a = dict(BASE, **case)
    return a["N"] * a["H"] * a["W"]


def call(lib, entry, case):
    a = dict(BASE, **case)
    a["M"] = a["N"] * a["H"] * a["W"]
    fn = getattr(lib, "dlmcq_conv2d_i8_nhwc_" + entry)
    assert len(ENTRIES[entry]) == len(fn.argtypes), entry
    return int(fn(*[(a[name] or None) if typ is ctypes.c_void_p else a[name] for name, typ in zip(ENTRIES[entry], fn.argtypes)]))


def cases():
    """[(id, entry, overrides of BASE)], deterministic.  The ids are the fixture's keys.  BASE itself is a call every entry point
    accepts: each case adds at least one reason to refuse it, or takes its rows away."""
    sys.path.insert(0, os.path.join(ROOT, "dlmc-quant_amd"))
    from dlmc.quantization.scalar import kernels as K
    out = []

    def add(name, entry, **kw):
        out.append((f"{entry}:{name}", entry, kw))

    big = dict(H=2048, W=1024, Hb=2048, Wb=1024, K=256)       # M * K * 4 = 2^31 > 0x7fff0000, at a shape every form is built for
    for e in ENTRIES:
        multi = e in MULTI
        # ---- the range checks, and the empty problem behind them ----
        for tag, kw in (("M_negative", dict(N=-1)), ("C_0", dict(C=0)), ("K_0", dict(K=0)), ("K2_0", dict(K2=0)), ("K_96", dict(K=96)),
                        ("K_32", dict(K=32)), ("C_negative", dict(C=-64))):
            add("range/" + tag, e, **kw)
        if multi:
            for tag, kw in (("H_0", dict(H=0)), ("W_0", dict(W=0)), ("Hb_0", dict(Hb=0)), ("Wb_0", dict(Wb=0)), ("Cb_0", dict(Cb=0)),
                            ("strideb_0", dict(strideb=0)), ("strideb_negative", dict(strideb=-1)), ("H_differs", dict(Hb=9)),
                            ("W_differs", dict(Wb=5)), ("H_differs_strided", dict(Hb=16, Wb=13, strideb=2)),
                            ("W_differs_strided", dict(Hb=13, Wb=16, strideb=2))):
                add("range/" + tag, e, **kw)
        if e == "recompute_chain":
            add("range/Ca_0", e, Ca=0)
            add("range/relu_shortcut_relu6", e, relu_sc=2)
            add("empty/relu_shortcut_relu6", e, N=0, relu_sc=2)
        nulls = {k: 0 for k in ENTRIES[e] if BASE.get(k) == P}
        add("empty", e, N=0)
        add("empty/all_null", e, N=0, **nulls)
        add("empty/all_misaligned", e, N=0, **{k: P4 for k in nulls})
        add("empty/bad_C", e, N=0, C=0)
        add("empty/K_96", e, N=0, K=96)
        add("empty/relu6_and_bad_ranges", e, N=0, relu=2, q_lo=5, q2_lo=9, q2_hi=-9, q_form=77, rpt=65)
        if multi:
            add("empty/H_differs", e, N=0, Hb=9)
        # ---- every required pointer null in turn; the optional ones null (BASE) or given ----
        optional = ("out", "codes")
        for k in nulls:
            if k not in optional:
                add(f"null/{k}", e, **{k: 0})
        for k in ("out", "codes"):
            add(f"null/{k}/then_rows_65", e, rpt=65, **{k: 0})
        add("null/out_and_codes/then_rows_65", e, out=0, codes=0, rpt=65)
        add("given/bias_and_zero_points/then_rows_65", e, rpt=65, **{k: P for k in ENTRIES[e] if k.startswith(("bias", "zp_in")) or k in ("q_zp", "q2_zp")})
        # ---- every pointer the kernel reads 16 bytes at a time, at P + 4 ----
        al = ["x", "w", "w2", "out", "codes", "codes2"] + (["res"] if e == "chain" else ["xb", "wb"]) + (["xa", "wa"] if e == "recompute_chain" else [])
        for k in al:
            add(f"align/{k}", e, **{k: P4})
        for k in nulls:           # ... and the ones it does not: they get past the check, onto a later refusal
            if k not in al:
                add(f"align/{k}_is_free/then_rows_65", e, rpt=65, **{k: P4})
        # ---- the multi-operand forms' own range bounds ----
        if multi:
            add("erange/M_2^31", e, H=46341, W=46341, Hb=46341, Wb=46341)
            add("erange/sampled_2^40", e, H=8, W=8, Hb=1 << 17, Wb=1 << 17, strideb=1 << 14)
        # ---- chain_launch ----
        add("erange/MK4", e, **big)
        add("erange/MK4_K_2^24", e, K=1 << 24, H=32, W=1, Hb=32, Wb=1)
        for tag, kw in (("relu6", dict(relu=2)), ("relu2_relu6", dict(relu2=2)), ("q_lo_1", dict(q_lo=1)), ("q_hi_254", dict(q_hi=254)),
                        ("q_signed", dict(q_lo=-128, q_hi=127)), ("q_hi_127", dict(q_hi=127)),
                        ("ctl/force_tiled", dict(q2_form=ZP | FORCE_TILED)), ("ctl/route_only", dict(q2_form=ZP | ROUTE_ONLY)),
                        ("ctl/pipelined", dict(q2_form=ZP | PIPELINED)), ("ctl/all_with_layout", dict(q2_form=ZP | W2_CM | OUT_CM | FORCE_TILED | ROUTE_ONLY | PIPELINED)),
                        ("q2/lo_above_hi", dict(q2_lo=5, q2_hi=-5)), ("q2/lo_below_-128", dict(q2_lo=-129, q2_hi=0)), ("q2/hi_above_255", dict(q2_hi=256)),
                        ("q2/span_above_255", dict(q2_lo=-128, q2_hi=255)), ("q_form/below_emulate", dict(q_form=-1)), ("q_form/rootq", dict(q_form=ROOTQ)),
                        ("q_form/shifted", dict(q_form=ZP | SHIFT128)), ("q_form/control_bit", dict(q_form=ZP | FORCE_TILED)),
                        ("q_form/layout_bit", dict(q_form=ZP | W2_CM)), ("q2_form/rootq", dict(q2_form=ROOTQ)), ("q2_form/5", dict(q2_form=5)),
                        ("q2_form/255", dict(q2_form=255)), ("q2_form/shifted_signed", dict(q2_form=ZP | SHIFT128, q2_lo=-5, q2_hi=5)),
                        ("q2_form/rootq_chunk_major", dict(q2_form=ROOTQ | W2_CM | OUT_CM)),
                        ("rows_65", dict(rpt=65)), ("rows_2^30", dict(rpt=1 << 30))):
            add("launch/" + tag, e, **kw)
            # a second fault behind it - the 32-bit offset bound, which answers DLMCQ_ERANGE once a call reaches it
            if tag not in ("rows_65", "rows_2^30"):
                add("order/" + tag + "/before_MK4", e, **dict(big, **kw))
        add("order/MK4/before_rows_65", e, rpt=65, **big)
        add("order/MK4/before_unsupported_shape", e, **dict(big, K2=512))
        add("order/MK4/before_mixed_layouts_elsewhere", e, q2_form=ZP | IN_CM, **big)
        add("order/null_before_align", e, x=P4, wsum=0)
        add("order/null_second_layer_before_align", e, w2=P4, s_w2=0)
        add("order/align_before_relu6", e, x=P4, relu=2)
        add("order/align_before_MK4", e, codes2=P4, **big)
        add("order/align_before_unsupported_shape", e, w=P4, K2=512)
        add("order/range_before_null", e, K=96, x=0)
        add("order/ctl_and_bad_range", e, q2_form=ZP | ROUTE_ONLY, q2_lo=5, q2_hi=-5)
        add("order/bad_range_and_rows_65", e, q2_lo=5, q2_hi=-5, rpt=65)
        if multi:
            add("order/align_before_M_2^31", e, xb=P4, H=46341, W=46341, Hb=46341, Wb=46341)
            add("order/null_before_sampled_2^40", e, wb=0, H=8, W=8, Hb=1 << 17, Wb=1 << 17, strideb=1 << 14)
            add("order/M_2^31_before_relu6", e, relu=2, H=46341, W=46341, Hb=46341, Wb=46341)
            add("order/sampled_2^40_before_q_range", e, q_lo=1, H=8, W=8, Hb=1 << 17, Wb=1 << 17, strideb=1 << 14)
            add("order/sampled_2^40_before_rows_65", e, rpt=65, H=8, W=8, Hb=1 << 17, Wb=1 << 17, strideb=1 << 14)
        else:
            add("order/relu6_before_M_2^31", e, relu=2, H=46341, W=46341)      # (the plain form has no bound of its own: M * K * 4 catches it, later)
            add("order/M_2^31", e, H=46341, W=46341)
    # ---- the fp32 tensors' layouts: the 128 -> K -> 128 instantiation keeps both in one ----
    for tag, bits in (("in", IN_CM), ("out", OUT_CM)):
        add(f"mixed_layouts/{tag}/128_128", "chain", C=128, K2=128, q2_form=ZP | bits)
        add(f"mixed_layouts/{tag}/128_128/weights_chunk_major", "chain", C=128, K2=128, q2_form=ZP | bits | W2_CM)
        add(f"mixed_layouts/{tag}/128_128/before_MK4", "chain", C=128, K2=128, q2_form=ZP | bits, **big)
        add(f"mixed_layouts/{tag}/64_64/then_rows_65", "chain", q2_form=ZP | bits, rpt=65)
        add(f"mixed_layouts/{tag}/64_64/then_MK4", "chain", q2_form=ZP | bits, **big)
    add("mixed_layouts/in/128_128/no_out/then_rows_65", "chain", C=128, K2=128, out=0, q2_form=ZP | IN_CM, rpt=65)       # one fp32 tensor: its layout is the call's
    add("mixed_layouts/in/128_128/no_out/then_MK4", "chain", C=128, K2=128, out=0, q2_form=ZP | IN_CM, **big)
    add("mixed_layouts/both/128_128/then_MK4", "chain", C=128, K2=128, q2_form=ZP | IN_CM | OUT_CM, **big)
    for e in MULTI:               # no shortcut tensor: the input bit says nothing
        add("mixed_layouts/in/then_MK4", e, q2_form=ZP | IN_CM, **big)
    add("mixed_layouts/in/128_256_128/then_MK4", "dual_chain", C=128, Cb=256, K2=128, q2_form=ZP | IN_CM, **big)
    # ---- shapes no kernel is built for: the complement of the wrappers' sets ----
    widths = (64, 128, 192, 256, 512)
    for c, k2 in itertools.product(widths, widths):
        if (c, k2) not in K.CHAIN_SHAPES:
            add(f"shape/{c}_{k2}", "chain", C=c, K2=k2)
    for c, cb, k3 in itertools.product((64, 128, 256), repeat=3):
        if (c, cb, k3) not in K.DUAL_CHAIN_SHAPES:
            add(f"shape/{c}_{cb}_{k3}", "dual_chain", C=c, Cb=cb, K2=k3)
    for c, ca, cb, k2 in itertools.product((64, 128, 256), repeat=4):
        if (c, ca, cb, k2) not in K.RECOMPUTE_CHAIN_SHAPES:
            add(f"shape/{c}_{ca}_{cb}_{k2}", "recompute_chain", C=c, Ca=ca, Cb=cb, K2=k2)
    for c, ca, cb, k2 in K.RECOMPUTE_CHAIN_SHAPES:     # ... and the one it is built for, with anything but the plan's epilogue
        sh = dict(C=c, Ca=ca, Cb=cb, K2=k2)
        for tag, kw in (("no_relu", dict(relu=0)), ("zero_point", dict(q_zp=P)), ("second_zero_point", dict(q2_zp=P)),
                        ("second_signed", dict(q2_lo=-128, q2_hi=127)), ("second_narrow", dict(q2_hi=127))):
            add(f"shape/{c}_{ca}_{cb}_{k2}/{tag}", "recompute_chain", **sh, **kw)
        add(f"order/MK4/before_no_relu_{c}_{ca}_{cb}_{k2}", "recompute_chain", relu=0, **dict(big, **sh))
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
    from dlmc import _native as N
    lib = N.lib
    if path:
        lib = ctypes.CDLL(os.path.abspath(path))
        for name in ENTRIES:
            fn = getattr(lib, "dlmcq_conv2d_i8_nhwc_" + name)
            fn.restype, fn.argtypes = N.SIGNATURES["dlmcq_conv2d_i8_nhwc_" + name]
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


def test_the_fixture_holds_no_accepted_call_and_reaches_every_refusal():
    """Checked on the fixture, so a generator that drifts away from a refusal - or towards a launch - fails."""
    with open(FIXTURE) as f:
        want = json.load(f)["results"]
    all_cases = {cid: (entry, kw) for cid, entry, kw in cases()}
    assert sorted(all_cases) == sorted(want) and len(want) >= 300
    for cid, v in want.items():
        assert v < 0 or (v == OK and rows(all_cases[cid][1]) == 0), f"{cid} = {v}: an accepted call"
    per_entry = {}
    for k, v in want.items():
        per_entry.setdefault(k.split(":")[0], set()).add(v)
    assert per_entry == {"chain": {OK, EINVAL, ERANGE, EALIGN}, "dual_chain": {OK, EINVAL, ERANGE, EALIGN}, "recompute_chain": {OK, EINVAL, ERANGE, EALIGN}}
    for cid, v in want.items():          # whole groups at one code
        name = cid.split(":", 1)[1].split("/")
        group = name[0]
        if group in ("range", "null", "launch", "shape"):
            assert v == EINVAL, cid
        elif group in ("align", "erange"):
            assert v == (EINVAL if "then_rows_65" in cid else EALIGN if group == "align" else ERANGE), cid
        elif group == "empty":
            assert v == (OK if name[-1] in ("empty", "all_null", "all_misaligned", "relu6_and_bad_ranges") else EINVAL), cid
    named = {  # the order of the checks, where two codes tell
        "chain:order/null_before_align": EINVAL, "chain:order/align_before_relu6": EALIGN, "chain:order/align_before_MK4": EALIGN,
        "chain:order/relu6_before_M_2^31": EINVAL, "chain:order/M_2^31": ERANGE, "dual_chain:order/M_2^31_before_relu6": ERANGE,
        "dual_chain:order/align_before_M_2^31": EALIGN, "recompute_chain:order/sampled_2^40_before_rows_65": ERANGE,
        "chain:order/relu6/before_MK4": EINVAL, "chain:order/q2/lo_above_hi/before_MK4": EINVAL,
        "chain:order/ctl/route_only/before_MK4": EINVAL, "chain:order/MK4/before_rows_65": ERANGE,
        "chain:order/MK4/before_unsupported_shape": ERANGE, "recompute_chain:order/MK4/before_no_relu_64_64_64_64": ERANGE,
        "chain:mixed_layouts/in/128_128": EINVAL, "chain:mixed_layouts/out/128_128/before_MK4": EINVAL,
        "chain:mixed_layouts/in/64_64/then_MK4": ERANGE, "chain:mixed_layouts/both/128_128/then_MK4": ERANGE,
        "chain:mixed_layouts/in/128_128/no_out/then_MK4": ERANGE, "dual_chain:mixed_layouts/in/128_256_128/then_MK4": ERANGE,
    }
    assert {k: want[k] for k in named} == named


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2] if len(sys.argv) > 2 else None)
    else:           # python tests/test_chain_refusals_host.py --write LIBRARY [COMMIT]: the fixture, from that library
        assert sys.argv[1] == "--write"
        results = run(sys.argv[2])["results"]
        all_cases = {cid: kw for cid, _, kw in cases()}
        for cid, v in results.items():
            assert v < 0 or (v == OK and rows(all_cases[cid]) == 0), f"{cid} = {v}: the library accepted the call - it does not belong in this sweep"
        header = ("Return values of dlmcq_conv2d_i8_nhwc_chain / _dual_chain / _recompute_chain for the cases of tests/test_chain_refusals_host.py, "
                  "recorded from the library built at commit %s - the parent of the commit that rewrote the chain kernels' host side around "
                  "one call record - by `python tests/test_chain_refusals_host.py --write LIBRARY COMMIT`.  0: DLMCQ_OK (an empty problem); "
                  "negative: a refusal.  No call in it is accepted." % (sys.argv[3] if len(sys.argv) > 3 else "?"))
        with open(FIXTURE, "w") as f:
            json.dump({"header": header, "results": results}, f, indent=0, sort_keys=True)
            f.write("\n")
        print(len(results), "cases;", {v: list(results.values()).count(v) for v in sorted(set(results.values()))})
