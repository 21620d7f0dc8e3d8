"""Which instantiation of conv_chain_i8_kernel, which tile height and which fp32 layouts does chain_launch (csrc/conv_chain_i8.hip) pick for
each call of tests/chain_variant_cases.py - asked with DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_CHAIN_VARIANT on placeholder pointers, in a child process
that hides the GPUs (as tests/test_chain_refusals_host.py makes its calls; both bits are ALWAYS set here, so nothing can launch): every call
is answered with the record, FL slot, tile height and layouts the table says; every table row x existing FL slot is reached by at least three
calls; the table the library lists (dlmcq_x_chain_variant_table) is the 7 x 3 + 2 kernels written down by hand and agrees with the wrappers'
shape sets; the recomputing form refuses what would need FL = -1; the 128 -> K -> 128 row refuses mixed fp32 layouts; the automatic 56-row
rule picks what its comment says on either side of each of its bounds.

`reference` is the float64 reference tests/test_gpu_chain_variants.py compares the kernels with, computed here on the CPU for every call:
the staged exactness conditions (tests/exact_stages.py: chain_stages; exact_layers.second_gemm_full_ref) and the conditions that keep a
call from proving nothing are asserted WITHOUT a GPU, from the reference alone -
  * on the live channels at least 10 % of the reference codes of EACH quantiser lie strictly between its bounds (under ReLU the lower
    bound is the code of 0);
  * the lower clamp occurs in every ReLU case, for the quantiser behind that ReLU;
  * every instantiation has a call with reference codes at the first quantiser's upper bound, and one at the second's."""
import functools
import json
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@functools.lru_cache(maxsize=None)
def reference(cid):
    """The operands of a call and its exact reference, conditions asserted: dict with the layers (`own`, `sampled`, `unit`, `second`), the
    shortcut tensor `res` (N, K, H, W), the quantisers `q1`, `q2`, `mid` (the block's fp32 output), `c1` (first codes), `v2` (the second
    layer's fp32 value after its activation), `c2` (second codes; the bytes the kernel stores), all (N, channels, H, W) CPU tensors."""
    import chain_variant_cases as V
    import exact_layers as X
    import exact_stages as S
    from test_gpu_halo_variants import QUANTS
    case = next(c for c in V.CASES if c.cid == cid)
    c1, kb, c2, ca, cb, _ = case.row
    n, h, w = case.geo
    gen = torch.Generator().manual_seed(case.seed)

    def layer(c, hh, ww, which, extra):
        uns, side = V.INPUTS[case.inputs[which]]
        lay = X.make_full_range_layer(gen, n, c, hh, ww, case.kd, 1, signed_in=not uns, zp=None if uns else V.SIGNED_ZP, zp_side=side,
                                      edge_bias=not extra and case.entry != "chain")
        if extra:                              # the edge channels belong to the own operand: zero weights (they are) and zero biases here
            lay.bias[:lay.nz] = 0.0
        if case.null_bias == ("own", "sampled", "unit")[which]:
            lay.bias = torch.zeros(case.kd)
        return lay
    r = dict(own=layer(c1, h, w, 0, False), q1=X.Quant(*V.Q1[case.q1]), q2=QUANTS[case.q2])
    own = r["own"]
    shift = lambda lay, which: 128 if V.INPUTS[case.inputs[which]][0] else 0
    if case.entry == "chain":
        r["res"] = X.edge_residual((n, case.kd, h, w), own.nz, gen)
        true = S.chain_stages(own, shift(own, 0), residual=r["res"])
    else:
        hb, wb = case.sampled_hw()
        r["sampled"] = layer(c2 or cb, hb, wb, 1, True)
        if case.entry == "recompute_chain":
            r["unit"] = layer(ca, h, w, 2, True)
        true = S.chain_stages(own, shift(own, 0), sampled=r["sampled"], shift_s=shift(None, 1), stride=case.stride, unit=r.get("unit"),
                              shift_u=shift(None, 2), relu_shortcut=case.relu_sc)
    r["mid"] = X.exact_f32(X.activation(true, case.relu), "first activation")
    r["c1"] = X.quantise(r["mid"], r["q1"])
    sec = X.make_full_range_second(gen, r["c1"], r["q1"], kb)
    if case.null_bias == "second":
        sec.bias = torch.zeros(kb)
    r["second"] = sec
    r["v2"] = X.second_gemm_full_ref(r["c1"], r["q1"], sec.wq, sec.s_w, sec.bias, act2=case.relu2)
    r["c2"] = X.quantise(r["v2"], r["q2"])
    # ---- the conditions that keep the call from proving nothing
    r["facts"] = (clamp_facts(r["mid"], r["q1"], case.relu, own.nz), clamp_facts(r["v2"], r["q2"], case.relu2, sec.nz))
    for (inside, lower, _), relu, what in zip(r["facts"], (case.relu, case.relu2), ("first", "second")):
        assert inside >= 0.10 and (lower or not relu), (cid, what, inside, lower)
    return r


def clamp_facts(v, q, relu, nz):
    """(share of the live channels' reference codes strictly inside the bounds, the lower clamp occurs, the upper clamp occurs)."""
    import exact_layers as X
    c = X.oracle_codes(v, q)[:, nz:]
    lo = float(q.lo)
    if relu:
        lo = max(lo, float(X.oracle_codes(torch.zeros(1), q)))
    return float(((c > lo) & (c < q.hi)).float().mean()), bool((c == lo).any()), bool((c == q.hi).any())


def child():
    """Runs in the child process: every query's answer as one JSON line on stdout, or {"skipped": why}."""
    import chain_variant_cases as V
    import test_chain_refusals_host as R
    if os.environ.get("HIP_VISIBLE_DEVICES") != "-1" or R.hidden_gpu_count() > 0:
        print(json.dumps({"skipped": "the HIP runtime still sees a GPU: no call was made"}))
        return
    from dlmc import _native as N
    both = N.ROUTE_ONLY | N.ROUTE_CHAIN_VARIANT

    def ask(entry, kw):
        assert kw["q2_form"] & both == both, "a call without both query bits could launch"
        return R.call(N.lib, entry, kw)
    out = {"cases": {c.cid: ask(c.entry, c.route_args()) for c in V.CASES},
           "auto": {cid: ask(entry, kw) for cid, entry, kw, _ in V.auto_rule_cases()},
           "mixed": [ask("chain", kw) for kw in V.REFUSED_MIXED],
           "rows_65": [ask(c.entry, dict(c.route_args(), rpt=65)) for c in (V.CASES[0], V.CASES[10], V.CASES[-1])],
           "table": N.chain_variant_table()}
    # the recomputing form with anything that would need FL = -1: no such kernel
    rc0 = V.BY_RECORD[(0, 3)][0]
    out["recompute_flx"] = {tag: ask("recompute_chain", dict(rc0.route_args(), **kw)) for tag, kw in (
        ("no_relu", dict(relu=0)), ("zero_point", dict(q_zp=R.P)), ("second_zero_point", dict(q2_zp=R.P)),
        ("second_signed", dict(q2_lo=-128, q2_hi=127)))}
    out["recompute_ok"] = ask("recompute_chain", rc0.route_args())
    # either bit alone stays a refusal, with no other fault in the call (as the fixture of test_chain_refusals_host.py asks ROUTE_ONLY alone: this
    # process sees no GPU, so a regression that accepted the call would answer with a launch error, not run on the placeholder addresses)
    alone = {}
    for c in (V.CASES[0], V.CASES[10], V.CASES[-1]):
        for tag, bits in (("route_only", N.ROUTE_ONLY), ("chain_variant", N.ROUTE_CHAIN_VARIANT)):
            kw = c.call_args()
            kw["q2_form"] |= bits
            alone[f"{c.entry}/{tag}"] = R.call(N.lib, c.entry, kw)
    out["alone"] = alone
    print(json.dumps(out))


@functools.lru_cache(maxsize=None)
def answers():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, check=True, capture_output=True, text=True).stdout
    got = json.loads(out.strip().splitlines()[-1])
    if "skipped" in got:
        import pytest
        pytest.skip(got["skipped"])
    return got


def test_every_case_is_answered_with_the_record_the_table_says():
    import chain_variant_cases as V
    got = answers()["cases"]
    wrong = {c.cid: (V.decode(got[c.cid]), c.expected()) for c in V.CASES if V.decode(got[c.cid]) != c.expected()}
    assert not wrong, f"{len(wrong)} of {len(V.CASES)} calls answer differently (got, table): {dict(list(wrong.items())[:8])}"


def test_every_instantiation_is_reached_three_times_and_the_table_is_the_23_kernels():
    import chain_variant_cases as V
    from dlmc.quantization.scalar import kernels as K
    got = answers()
    table = [tuple(r[:5]) + (tuple(r[5]),) for r in got["table"]]
    assert table == V.ROWS and sum(len(r[5]) for r in table) == 7 * 3 + 2 == len(V.RECORDS)
    reached = {}
    for c in V.CASES:
        kind, ri, fl = V.decode(got["cases"][c.cid])[:3]
        reached[(ri, fl)] = reached.get((ri, fl), 0) + 1
    assert sorted(reached) == sorted(V.RECORDS) and min(reached.values()) >= 3, reached
    # the wrappers' shape sets are the table's rows, entry point by entry point
    assert K.CHAIN_SHAPES == {(r[0], r[1]) for r in table if not r[2] and not r[3]}
    assert K.DUAL_CHAIN_SHAPES == {(r[0], r[2], r[1]) for r in table if r[2]}
    assert K.RECOMPUTE_CHAIN_SHAPES == {(r[0], r[3], r[4], r[1]) for r in table if r[3]}
    assert K.CHAIN_ONE_LAYOUT == {(table[i][0], table[i][1]) for i in V.ONE_LAYOUT_ROWS}
    assert all(r[5] == ((3, 1) if r[3] else (3, 1, -1)) for r in table)


def test_the_table_covers_what_the_issue_of_each_row_needs():
    """The spread of the case table itself, row by row: every tile height, both W3 layouts, every block width per record, a call below one
    tile, every output combination, every input type on the own operand, a null bias on every operand; both strides and both shortcut
    activations where they exist; one high-address call per entry point."""
    import chain_variant_cases as V
    for ri, row in enumerate(V.ROWS):
        cs = [c for c in V.CASES if c.record[0] == ri]
        entry = V.entry_of(ri)
        assert {c.rpt for c in cs} == {0, 64, 56, 49} and {c.w3cm for c in cs} == {False, True}, ri
        assert sum(c.m == 35 for c in cs) == 1 and all(c.m in (35, 126) for c in cs), ri
        for fl in row[5]:
            assert {c.kd for c in V.BY_RECORD[(ri, fl)]} == {64, 192, 256}, (ri, fl)
        assert {(c.out, c.codes) for c in cs} == {(True, True), (False, True), (True, False), (False, False)}, ri
        assert {c.inputs[0] for c in cs} == {0, 1, 2}, ri
        want_nulls = {"chain": {"own", "second"}, "dual_chain": {"own", "sampled", "second"}, "recompute_chain": {"own", "sampled", "unit", "second"}}[entry]
        assert {c.null_bias for c in cs} == want_nulls | {None}, ri
        lay = {c.layouts() for c in cs if c.out and entry == "chain"}
        if entry == "chain":
            assert lay == ({(False, False), (True, True)} if ri in V.ONE_LAYOUT_ROWS else {(False, False), (True, True), (True, False), (False, True)}), (ri, lay)
        else:
            assert {c.stride for c in cs} == {1, 2} and {c.layouts() for c in cs} == {(False, False), (True, True)}, ri
        if entry == "recompute_chain":
            assert {c.relu_sc for c in cs} == {0, 1}
        for fl in row[5]:            # the FL slot is reached on purpose
            for c in V.BY_RECORD[(ri, fl)]:
                plain = V.Q1[c.q1][1] is None and not c.q2.startswith(("signed", "uzp"))
                assert fl == ((3 if c.out else 1) if c.relu and plain else -1), c.cid
        if -1 in row[5]:
            flx = V.BY_RECORD[(ri, -1)]
            assert any(not c.relu and c.q1 == "zp100" for c in flx) and any(c.relu and V.Q1[c.q1][1] is not None for c in flx)
            assert any(c.relu and V.Q1[c.q1][1] is None and c.q2.startswith("signed") for c in flx)
    assert sorted(c.entry for c in V.CASES if c.high) == ["chain", "dual_chain", "recompute_chain"]


def test_recompute_refuses_what_would_need_the_run_time_form():
    got = answers()
    assert got["recompute_flx"] == dict(no_relu=EINVAL, zero_point=EINVAL, second_zero_point=EINVAL, second_signed=EINVAL)
    assert got["recompute_ok"] > 0


def test_the_one_layout_row_refuses_mixed_layouts_and_either_bit_alone_is_refused():
    got = answers()
    assert got["mixed"] == [EINVAL, EINVAL]
    assert len(got["alone"]) == 6 and set(got["alone"].values()) == {EINVAL}, got["alone"]
    assert got["rows_65"] == [EINVAL] * 3


def test_the_56_row_rule_picks_what_its_comment_says():
    import chain_variant_cases as V
    got = answers()["auto"]
    cases = V.auto_rule_cases()
    assert {want for *_, want in cases} >= {56, 64, 49, 1}
    wrong = {}
    for cid, entry, kw, want in cases:
        ri = next(i for i, r in enumerate(V.ROWS) if V.record_name((i, 3)) == cid.split("/")[0])
        if V.decode(got[cid]) != ("chain", ri, 3, want, False, False):
            wrong[cid] = (V.decode(got[cid]), want)
    assert not wrong, wrong


def test_every_case_keeps_its_proving_conditions():
    """The reference of every call, on the CPU: `reference` asserts the staged conditions and the per-call clamp conditions; here the
    per-instantiation ones."""
    import chain_variant_cases as V
    for rec in V.RECORDS:
        facts = [reference(c.cid)["facts"] for c in V.BY_RECORD[rec]]
        assert any(f[0][2] for f in facts), f"{V.record_name(rec)}: no call has reference codes at the first quantiser's upper bound"
        assert any(f[1][2] for f in facts), f"{V.record_name(rec)}: no call has reference codes at the second quantiser's upper bound"


if __name__ == "__main__":
    assert sys.argv[1] == "--child"
    sys.path.insert(0, os.path.join(ROOT, "dlmc-quant_amd"))
    child()
