"""Which instantiation of the first-layer, pointwise and block-end kernels a call runs, pinned from outside (no GPU): every case of
tests/stem_pw_variant_cases.py is asked with DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_PW_VARIANT on placeholder pointers and must answer the record it
was written for; together the cases reach the library's own tables (dlmcq_x_stem_variant_table, dlmcq_x_pw_variant_table: listed by the
launchers) and nothing else; and the tables are the 93 records written out by hand in the case module.  Every case's exactness conditions
(tests/test_gpu_stem_pw_variants.py: `reference`) are asserted here on the CPU, with what keeps a case from proving nothing: ReLU6 cases leave
at least 10 % of the live outputs strictly inside (0, 6) with both bounds hit, plain-quantiser cases reach the upper clamp.  The launchers'
group formulas restated in the case module are proved for 256 CUs: in every `loops` case some wave owns 3 blocks or tiles and another 2 -
and those cases, sized for 256 CUs, meet the conditions here like every other.  The bit alone, and on every entry point that does not take
it, is DLMCQ_EINVAL: the first-layer, depthwise and tiled entry points in this process on empty problems, the chain, map, row, attention
and pooling entry points - whose shared form parser knows the bit - in a child process that hides the GPUs, next to the same call without it."""
import json
import os
import subprocess
import sys

if __name__ == "__main__":          # the child process of the refusal sweep below: no conftest has set the paths
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "dlmc-quant_amd")]

import pytest

import stem_pw_variant_cases as W
import test_conv_dispatch_host as T
import test_dw_stem_refusals_host as D
import tiled_variant_cases as V_

CUS = 256
V, R = W.ROUTE_PW_VARIANT, W.ROUTE_ONLY


def _lib():
    from dlmc import _native as N
    return N


def test_the_tables_are_the_93_records():
    N = _lib()
    stem, (pw, pwr) = N.stem_variant_table(), N.pw_variant_tables()
    assert sorted(stem) == sorted(W.STEM_RECORDS + W.POOL_RECORDS + W.POOL7_RECORDS) and len(stem) == 49
    assert sorted(pw) == sorted(W.PW_RECORDS) and sorted(pwr) == sorted(W.PWR_RECORDS) and len(pw) == 36 and len(pwr) == 8
    assert N.ROUTE_PW_VARIANT == 0x100000 and (N.ROUTE_STEM_VARIANT_TAG, N.ROUTE_PW_VARIANT_TAG, N.ROUTE_PWR_VARIANT_TAG) == (1 << 21, 1 << 22, 1 << 23)
    # the header's encoding, spelt out; the other decoders reject these answers, and these theirs
    assert N.decode_stem_variant((1 << 21) | (7 << 4) | 8 | 2 | 1) == ("stem", 7, True, False, True, True)
    assert N.decode_stem_variant((1 << 21) | (1 << 12) | (5 << 4)) == ("pool", 5) and N.decode_stem_variant((1 << 21) | (2 << 12) | 1) == ("pool7", True)
    assert N.decode_pw_variant((1 << 22) | (16 << 8) | (2 << 4) | 2) == ("pw", 1024, 128, True, False)
    assert N.decode_pw_variant((1 << 23) | (1 << 4) | 8 | 4 | 2 | 1) == ("pwr", 256, True, True, True, True)
    for rc in ((1 << 21) | (3 << 4), (1 << 22) | (1 << 8) | (1 << 4), (1 << 23) | (2 << 4) | 1):
        assert N.decode_variant(rc) is None and N.decode_halo_variant(rc) is None and N.decode_dw_variant(rc) is None and N.decode_dw5_variant(rc) is None
        assert N.decode_chain_variant(rc) is None and sum(d(rc) is not None for d in (N.decode_stem_variant, N.decode_pw_variant)) == 1
    for rc in (0, -1, 3, 4, 8, (1 << 24) | (128 << 8) | 10, (1 << 27) | (1 << 8), 1 << 29, 1 << 30, (1 << 21) | (1 << 22), (1 << 22) | (1 << 23), (1 << 21) | (8 << 4)):
        assert N.decode_stem_variant(rc) is None and N.decode_pw_variant(rc) is None, rc


def test_every_case_reaches_the_record_it_names_and_the_cases_reach_the_93():
    N = _lib()
    got = {c.cid: c.ask(N.lib, c.route_args(cus=CUS)) for c in W.CASES}
    wrong = {cid: (got[cid], W.BY_ID[cid].record) for cid in got if got[cid] != W.BY_ID[cid].record}
    assert not wrong, f"(answer, meant) {wrong}"
    assert set(got.values()) == set(W.RECORDS) and len(W.RECORDS) == 93
    for r in W.RECORDS:
        assert len(W.BY_RECORD[r]) >= (2 if r[0] in ("stem", "pw") and r[4] else 3), r
    assert len({c.cid for c in W.CASES}) == len(W.CASES)
    for c in W.CASES:       # without the variant bit: the family's route, as ever (the first-layer entry points take no lone DLMCQ_ROUTE_ONLY)
        a = c.route_args(cus=CUS)
        if c.family == "stem":
            if not c.quant:         # (without `codes` the form is not looked at: DLMCQ_ROUTE_ONLY alone would be a REAL call - never made here)
                continue
            assert D.call(N.lib, c.entry, dict(a, q_form=a["q_form"] & ~V)) == D.EINVAL, c.cid
        else:
            assert T.call(N.lib, c.entry, dict(a, ctl=a["ctl"] & ~V)) == T.ROUTES[c.record[0]], c.cid


def test_the_fallbacks_answer_the_other_record():
    N = _lib()
    for cid, change, record in W.FALLBACKS:
        c = W.BY_ID[cid]
        a = c.route_args(cus=CUS)
        if change.get("pad0"):
            a.update(pad=0)
        else:
            a["codes" if "codes_off" in change else "x"] += 4
        assert c.ask(N.lib, a) == record, (cid, change)


def test_the_bit_alone_and_elsewhere_is_refused():
    N = _lib()
    for e in D.STEMS:
        # (real calls on placeholder pointers, so the problem is EMPTY: a library that lost the check answers DLMCQ_OK and launches nothing)
        for extra in (dict(), dict(out=D.P, codes=0)):
            assert D.call(N.lib, e, dict(extra, N=0, q_form=D.ZP | V)) == D.EINVAL, (e, extra)
        assert D.call(N.lib, e, dict(q_form=D.ZP | R)) == D.EINVAL and D.call(N.lib, e, dict(q_form=D.ZP | R | V | D.FORCE_TILED)) == D.EINVAL, e
        assert D.call(N.lib, e, dict(N=0, q_form=D.ZP | R | V)) == 0, e                       # an empty problem stays DLMCQ_OK
        assert D.call(N.lib, e, dict(w=D.P4, q_form=D.ZP | R | V)) == D.EALIGN, e            # validated exactly as the real call
    for e in D.ENTRIES:
        if e in D.STEMS:
            continue
        for form in ("q_form", "q2_form") if e == "dwpw_i8_nhwc" else ("q_form",):
            assert D.call(N.lib, e, {form: D.ZP | V}) == D.EINVAL and D.call(N.lib, e, {form: D.ZP | V | R}) == D.EINVAL, (e, form)
    geo = dict(N=2, H=48, W=48, C=64, K=128)
    for e in T.ENTRIES:
        if e == "f32":
            continue
        args = dict(geo, out=T.P) if e == "fused_observed" else geo
        # alone: refused before anything is looked at (real calls on placeholder pointers: the problem is EMPTY, as above)
        assert V_.launch(N.lib, e, dict(args, N=0, ctl=V)) == T.EINVAL, e
        assert V_.launch(N.lib, e, dict(args, N=0, ctl=V, out=T.P, codes=0)) == T.EINVAL, e
    # the tiled route, an empty problem and a refusal are what they are without the bit
    assert T.call(N.lib, "fused", dict(geo, ctl=V | T.FORCE_TILED)) == T.ROUTES["tiled"] and T.call(N.lib, "fused", dict(geo, N=0, ctl=V)) == 0
    assert T.call(N.lib, "fused", dict(geo, C=32, ctl=V)) == T.EINVAL


def _elsewhere():
    """In the child process (GPUs hidden): the bit on the entry points that read their control bits out of `q_form` with epi_set_form - which
    knows the bit since the tiled dispatch takes it - and do not take it: the three chain entry points (any form argument) and the map, row,
    attention and pooling entry points.  Each is paired with the same call without the bit: that one gets PAST the argument checks (a record
    for the chain route query; for the others, which have no query, whatever the runtime answers a launch without a device - never
    DLMCQ_EINVAL), so the refusal is the bit's."""
    import ctypes
    import test_attention_host as A
    import test_avgpool_host as AP
    import test_chain_refusals_host as C
    import test_gate_host as G
    import test_swish_host as SW
    import test_transformer_host as TR
    from dlmc import _native as N
    if os.environ.get("HIP_VISIBLE_DEVICES") != "-1" or C.hidden_gpu_count() > 0:
        return {"skipped": "the HIP runtime still sees a GPU: no call was made"}
    Q = N.ROUTE_CHAIN_VARIANT
    out = {}
    for e in C.ENTRIES:
        out[f"{e}/accepted"] = C.call(N.lib, e, dict(q2_form=C.ZP | R | Q))
        for tag, kw in (("q2_form/alone", dict(q2_form=C.ZP | V)), ("q2_form/route_only", dict(q2_form=C.ZP | V | R)),
                        ("q2_form/chain_variant", dict(q2_form=C.ZP | V | Q)), ("q2_form/both_query_bits", dict(q2_form=C.ZP | V | R | Q)),
                        ("q2_form/layout", dict(q2_form=C.ZP | V | C.OUT_CM)), ("q_form/alone", dict(q_form=C.ZP | V)),
                        ("q_form/route_only", dict(q_form=C.ZP | V | R)), ("q_form/in_a_query", dict(q_form=C.ZP | V, q2_form=C.ZP | R | Q))):
            out[f"{e}/{tag}"] = C.call(N.lib, e, kw)
    p = ctypes.c_void_p(4096)
    others = {"swish": lambda f: SW._call(form=f), "gate": lambda f: G._call(form=f), "avgpool": lambda f: AP._call(form=f),
              "gelu": lambda f: TR._gelu(form=f), "layernorm": lambda f: TR._ln(form=f), "attention": lambda f: A._at(form=f),
              "gap": lambda f: N.lib.dlmcq_gap_nhwc_f32(p, None, p, 2, 49, 64, p, None, 0, 255, f, 0.0, None)}
    for name, fn in others.items():
        out[f"{name}/accepted"] = fn(N.FORM_ZEROPOINT)
        out[f"{name}/alone"] = fn(N.FORM_ZEROPOINT | V)
        out[f"{name}/route_only"] = fn(N.FORM_ZEROPOINT | V | R)
    return {"results": out}


def test_the_bit_is_refused_by_the_chain_and_the_other_epilogue_entry_points():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    got = json.loads(subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True, capture_output=True,
                                    text=True).stdout.strip().splitlines()[-1])
    if "skipped" in got:
        pytest.skip(got["skipped"])
    got = got["results"]
    assert len(got) == 3 * 9 + 7 * 3
    for key, v in got.items():
        if key.endswith("/accepted"):
            name = key.split("/")[0]
            assert (v >= (1 << 30)) if name.endswith("chain") else (v != D.EINVAL), (key, v)     # a chain record / past the argument checks
        else:
            assert v == D.EINVAL, (key, v)


@pytest.mark.parametrize("template", ["stem", "pool", "pw", "pwr"])
def test_the_loop_cases_give_waves_unequal_shares_at_256_cus(template):
    (c,) = [c for c in W.CASES if c.loops == template]
    g = c.geo_for(CUS)
    if template in ("pw", "pwr"):
        nblk = -(-g["N"] * g["H"] * g["W"] // 32)
        ngroups, nw = (W.pw_groups(CUS, g["C"], c.record[2], g["K"], nblk) if template == "pw" else W.pwr_groups(CUS, g["C"], g["K"], nblk))
        waves, items = ngroups * nw, nblk
        assert g["N"] * g["H"] * g["W"] >= 4096 and (template == "pw" or (g["N"] * g["H"] * g["W"]) % 32 == 0)
    elif template == "stem":
        p, q = c.out_hw(g)
        items = -(-g["N"] * p * q // 32)
        waves = 4 * W.stem_workgroups(items)
    else:
        p, q = c.out_hw(g)
        items = g["N"] * -(-((p - 1) // 2 + 1) // 3) * -(-((q - 1) // 2 + 1) // 8)
        waves = min(items, W.POOL_WORKGROUPS)
    assert 2 * waves < items < 3 * waves, (c.cid, items, waves)


@pytest.mark.parametrize("record", W.RECORDS, ids=W.record_name)
def test_every_case_meets_the_exactness_conditions_on_the_cpu(record):
    import exact_layers as X
    import test_gpu_stem_pw_variants as G
    for c in W.BY_RECORD[record]:
        _, _, _, facts = G.reference(c, CUS, X.quantise)
        G.assert_facts(c, facts)


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    print(json.dumps(_elsewhere()))
