"""Which instantiation of the depthwise kernels a call runs, pinned from outside (no GPU): every depthwise case of tests/dw_variant_cases.py is
asked with DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_DW_VARIANT on placeholder pointers and must answer the record it was written for; together the cases
reach the library's two tables (dlmcq_x_dw_variant_table: listed from the launchers' own DW_TABLE / DWM_TABLE) and nothing else; and the tables
are the 26 + 8 records written out by hand in the case module.  A change to dw_variant, conv_dwm_plan or conv_dwm_applies that stops reaching
a record, or routes a shape to another one, fails here.  dlmcq_conv2d_dwpw_i8_nhwc has no route query (it refuses every control bit, the new
one included): the record of each of its cases is proved from dwpw_launch's formula, and its shapes from the geometry.

The structural assertions are computed from the geometry: the case module's promises (every family's shapes, grid-stride sizes, piece-count
boundaries on both sides, partial last tiles, unequal tile counts per workgroup, both input types, zero points on either side of 128 and
exactly 0 for the FAST records, quantisers, activations, a null bias) are proved here, not assumed."""
import dw_variant_cases as W
import test_dw_stem_refusals_host as D

CUS = 256
V = W.ROUTE_DW_VARIANT


def _lib():
    from dlmc import _native as N
    return N


def _dw_cases():
    return [c for c in W.CASES if c.record[0] != "dwpw"]


def test_the_tables_are_the_26_and_8_records():
    N = _lib()
    dw, dwm = N.dw_variant_tables()
    assert len(dw) == len(set(dw)) == 26 and len(dwm) == len(set(dwm)) == 8
    assert sorted(dw) == sorted(W.DW_RECORDS), (sorted(set(dw) - set(W.DW_RECORDS)), sorted(set(W.DW_RECORDS) - set(dw)))
    assert sorted(dwm) == sorted(W.DWM_RECORDS)
    assert N.ROUTE_DW_VARIANT == 0x40000 and (N.ROUTE_DW_VARIANT_TAG, N.ROUTE_DWM_VARIANT_TAG) == (1 << 27, 1 << 28)      # include/dlmcq.h
    # the other decoders reject these answers, and this one theirs
    for rc in ((1 << 27) | (1 << 8) | (2 << 4) | 3, (1 << 28) | (5 << 8) | 3):
        assert N.decode_variant(rc) is None and N.decode_halo_variant(rc) is None and N.decode_dw_variant(rc) is not None
    for rc in ((1 << 24) | (128 << 8) | 10, (1 << 25) | (128 << 16) | (24 << 8) | (2 << 4) | 3, (1 << 26) | (4 << 8), D.ROUTE_DW, D.ROUTE_DWM, 0,
               D.EINVAL, (1 << 27) | (3 << 8), (1 << 27) | (1 << 28), 1 << 29):
        assert N.decode_dw_variant(rc) is None, rc
    # the answers are above every DLMCQ_ROUTE_*, every tiled variant's and every 3x3 variant's
    assert (1 << 27) > (1 << 26) | (0xff << 8) | 0xff


def test_every_case_reaches_the_record_it_names_and_the_cases_reach_both_tables():
    N = _lib()
    got = {c.cid: W.decode(D.call(N.lib, c.entry, c.route_args(cus=CUS))) for c in _dw_cases()}
    wrong = {c.cid: (got[c.cid], c.record) for c in _dw_cases() if got[c.cid] != c.record}
    assert not wrong, f"(answer, meant) {wrong}"
    for c in _dw_cases():                                        # the header's encoding, spelt out
        r = c.record
        want = ((1 << 28) | (r[1] << 8) | (2 if r[2] else 0) | (1 if r[3] else 0)) if r[0] == "dwm" else \
            ((1 << 27) | (("p2", "dw3", "generic").index(r[1]) << 8) | (r[2] << 4) | (2 if r[4] else 0) | (1 if r[3] else 0))
        a = c.route_args(cus=CUS)
        assert D.call(N.lib, c.entry, a) == want, c.cid
        # without the bit: the family, as ever
        assert D.call(N.lib, c.entry, dict(a, q_form=a["q_form"] & ~V)) == (D.ROUTE_DWM if r[0] == "dwm" else D.ROUTE_DW), c.cid
    dw, dwm = N.dw_variant_tables()
    assert set(got.values()) == set(dw) | set(dwm)
    for r in W.RECORDS:
        assert len(W.BY_RECORD[r]) >= 2, r
    assert sum(len(v) for v in W.BY_RECORD.values()) == len(W.CASES) and len({c.cid for c in W.CASES}) == len(W.CASES)


def _zps(cs):
    return {(c.uns, c.zp) for c in cs}


def test_the_cases_cover_what_the_case_module_promises():
    geo_key = lambda g: tuple(sorted(g.items(), key=str))        # noqa: E731
    for r in W.DW_RECORDS:
        _, family, fast, r6, xoff = r
        cs = W.BY_RECORD[r]
        for c in cs:
            g = c.geo
            wide = (g["R"], g["S"]) == (3, 3) and g["C"] % 16 == 0 and g["C"] <= 2048
            p2 = wide and (g["stride"], g["pad"]) == (1, 1) and g["C"] <= 1024
            assert family == ("generic" if not wide else "p2" if p2 else "dw3"), c.cid
            assert g["N"] >= 2 and (c.act == 2) == r6 and c.xoff == xoff and (not xoff or g["pad"] > 0), c.cid
            plain = c.quant is not None and c.quant.startswith("plain")
            assert fast == ((1 if c.asym else 2) if (wide and not c.out and plain) else 0), c.cid
            # the matrix-core kernel would take a plain codes-only 3x3 / 1 / 1 layer of whole 64-channel chunks from 4096 pixels on
            dwm_takes = p2 and plain and not c.out and not xoff and g["C"] % 64 == 0 and g["W"] >= 14 and g["N"] * g["H"] * g["W"] >= 4096
            assert c.force == dwm_takes, c.cid
        # zero points: exactly 0 (the FAST kernels' out-of-range buffer loads) and not 0; uint8 above 128; int8 not 0
        zps = _zps(cs)
        assert (True, 0) in zps and any(u and z > 128 for u, z in zps) and any(not u and z != 0 for u, z in zps), r
        assert cs[0].quant.endswith("_hi") and sum(not c.bias for c in cs) == 1, r
        if not r6:
            assert {c.act for c in cs} == {0, 1}, r
        if fast:
            assert all(c.quant in ("plain", "plain_hi") and not c.out for c in cs), r
        else:
            assert {c.quant.split("_")[0] for c in cs if c.quant} >= {"uzp", "signed"} and any(c.out and c.quant for c in cs), r
            assert any(c.out and c.quant is None for c in cs) and {c.asym for c in cs} == {True, False}, r
    # every family's geometries are all used, and are what the kernels can get wrong
    used = lambda fam: {geo_key(c.geo) for c in W.CASES if c.record[0] == "dw" and c.record[1] == fam}        # noqa: E731
    assert used("p2") == {geo_key(g) for g in W.P2_GEOS + [W.P2_GRID_STRIDE]}
    assert used("dw3") == {geo_key(g) for g in W.DW3_PADDED + W.DW3_UNPADDED + [W.DW3_GRID_STRIDE]}
    assert used("generic") == {geo_key(g) for g in W.GENERIC_GEOS}
    for xoff in (False, True):          # ... the padded ones also under a float offset
        assert {geo_key(c.geo) for c in W.CASES if c.record[:2] == ("dw", "dw3") and c.record[4] == xoff} >= {geo_key(g) for g in W.DW3_PADDED}
        assert {geo_key(c.geo) for c in W.CASES if c.record[:2] == ("dw", "p2") and c.record[4] == xoff} >= {geo_key(g) for g in W.P2_GEOS}
    p2 = W.P2_GEOS
    assert {g["W"] % 2 for g in p2} == {0, 1} and any(g["W"] == 1 for g in p2) and any(g["H"] == 1 for g in p2)
    assert {16, 48, 1024} <= {g["C"] for g in p2} and all(g["N"] * g["H"] * g["W"] < 4096 for g in p2)
    d3 = W.DW3_PADDED + W.DW3_UNPADDED
    assert any((g["stride"], g["pad"], g["H"] % 2, g["W"] % 2) == (2, 1, 1, 0) for g in d3)
    assert {(g["stride"], g["pad"]) for g in d3} == {(2, 1), (1, 1), (1, 0), (2, 0)}
    assert any(g["C"] == 1040 and (g["stride"], g["pad"]) == (1, 1) for g in d3) and any(g["C"] == 2048 and (g["H"], g["W"]) == (3, 3) for g in d3)
    assert 2048 * 32 == 64 * 1024                                 # conv_dw3_i8_kernel's FAST 0 table at C = 2048: sizeof(DwTab) per channel
    assert any(c.record == ("dw", "dw3", 0, r6, x) and c.geo["C"] == 2048 for c in W.CASES for r6 in (False,) for x in (False, True))
    ge = W.GENERIC_GEOS
    assert {12, 84} <= {g["C"] for g in ge} and all(g["C"] % 16 for g in ge)
    assert {(g["R"], g["S"], g["stride"], g["pad"]) for g in ge} >= {(5, 5, 1, 2), (7, 7, 2, 3), (1, 1, 1, 0), (3, 5, 1, 1)}
    assert any(2 * g["pad"] > max(g["R"], g["S"]) - 1 for g in ge)          # more padding than the filter needs
    # grid-stride loops: more work items than 4096 workgroups of 256 threads, by less than a second full pass (an unequal second pass)
    threads = 4096 * 256
    g = W.P2_GRID_STRIDE
    assert threads < g["N"] * g["H"] * ((g["W"] + 1) // 2) * (g["C"] // 16) < 2 * threads
    g = W.DW3_GRID_STRIDE
    assert threads < g["N"] * (g["H"] - 2) * (g["W"] - 2) * (g["C"] // 16) < 2 * threads and g["pad"] == 0
    assert sum(c.geo is W.P2_GRID_STRIDE for c in W.CASES) == 1 and sum(c.geo is W.DW3_GRID_STRIDE for c in W.CASES) == 1

    # ---- the matrix-core kernel
    assert (W.dwm_pieces(14), W.dwm_pieces(30), W.dwm_pieces(31), W.dwm_pieces(62), W.dwm_pieces(63)) == (14, 16, 17, 20, 21)
    for r in W.DWM_RECORDS:
        _, hpw, xs, r6 = r
        cs = W.BY_RECORD[r]
        widths = set()
        for c in cs:
            g = c.geo_for(CUS)
            widths.add(g["W"])
            assert (4 if -(-W.dwm_pieces(g["W"]) // 4) <= 4 else 5) == hpw and c.uns != xs and (c.act == 2) == r6, c.cid
            assert g["C"] % 64 == 0 and g["N"] * g["H"] * g["W"] >= 4096 and c.quant.startswith("plain") and not c.out and not c.force, c.cid
            assert (g["N"] * (g["H"] + 1) * (g["W"] + 1)) % W.DWM_TP, c.cid                       # a partial last tile
            if c.geo["N"] is None:
                ntiles, groups = -(-g["N"] * (g["H"] + 1) * (g["W"] + 1) // W.DWM_TP), W.dwm_groups(CUS, g["C"] // 64)
                assert groups < ntiles < 2 * groups, (c.cid, ntiles, groups)
        assert widths >= ({14, 30} if hpw == 4 else {31, 62}), r
        assert {c.geo["C"] for c in cs} >= {64, 192} and any(c.geo["H"] % 2 for c in cs), r
        assert cs[0].quant == "plain_hi" and sum(not c.bias for c in cs) == 1 and {c.asym for c in cs} == {True, False}, r
        assert any(z != 0 for _, z in _zps(cs)), r
    assert any(4096 <= c.geo["N"] * c.geo["H"] * c.geo["W"] < 4096 + c.geo["H"] * c.geo["W"] for c in W.CASES if c.record[0] == "dwm" and c.geo["N"])
    assert {c.record[1] for c in W.CASES if c.record[0] == "dwm" and c.geo["N"] is None} == {4, 5}
    zps = _zps([c for c in W.CASES if c.record[0] == "dwm"])
    assert any(u and z > 128 for u, z in zps) and any(u and 0 < z < 128 for u, z in zps) and any(not u and z != 0 for u, z in zps)
    # the widest image taken: one pixel more and the call is the vector kernels'
    N = _lib()
    wide = dict(N=4, H=40, C=64, q_form=D.ZP | W.ROUTE_ONLY | V)
    assert W.decode(D.call(N.lib, "dw_i8_nhwc", dict(wide, W=62))) == ("dwm", 5, False, False)
    assert D.call(N.lib, "dw_i8_nhwc", dict(wide, W=63, q_form=D.ZP | W.ROUTE_ONLY)) == D.ROUTE_DW
    assert W.decode(D.call(N.lib, "dw_i8_nhwc", dict(wide, W=63))) == ("dw", "p2", 2, False, False)
    assert W.decode(D.call(N.lib, "dw_i8_nhwc", dict(wide, W=30))) == ("dwm", 4, False, False)
    assert W.decode(D.call(N.lib, "dw_i8_nhwc", dict(wide, W=31))) == ("dwm", 5, False, False)

    # ---- depthwise + pointwise: the record from dwpw_launch's formula; the shapes
    assert (W.dwpw_pieces(30), W.dwpw_pieces(31), W.dwpw_pieces(61), W.dwpw_pieces(62), W.dwpw_pieces(63)) == (8, 9, 12, 12, 13)      # (12: the most taken)
    for r in W.DWPW_RECORDS:
        _, k, hpw = r
        cs = W.BY_RECORD[r]
        for c in cs:
            g = c.geo
            hp = W.dwpw_pieces(g["W"])
            assert hp <= 12 and (2 if -(-hp // 4) <= 2 else 3) == hpw and c.k == k and g["C"] % 64 == 0, c.cid
            assert (g["R"], g["S"], g["stride"], g["pad"]) == (3, 3, 1, 1) and c.quant.split("_")[0] in ("plain", "uzp", "signed") and c.q1 in W.Q1, c.cid
            mq, fs = g["N"] * (g["H"] + 1) * (g["W"] + 1), (g["H"] + 1) * (g["W"] + 1)
            assert mq > W.DWPW_TP and mq % W.DWPW_TP and fs % W.DWPW_TP and g["N"] >= 2, c.cid        # > 1 tile, a partial one, tiles cross images
        assert {c.geo["W"] for c in cs} >= ({30} if hpw == 2 else {31, 61}), r
        assert {c.geo["C"] for c in cs} == {64, 128} and {c.asym for c in cs} == {c.asym2 for c in cs} == {c.dw_relu for c in cs} == {0, 1}, r
        if hpw == 2:
            assert any((c.geo["H"] + 1) * (c.geo["W"] + 1) < W.DWPW_TP for c in cs), r          # an image smaller than a tile
    dp = [c for c in W.CASES if c.record[0] == "dwpw"]
    assert {c.q1 for c in dp} == set(W.Q1) and {c.act for c in dp} == {0, 1} and {c.bias for c in dp} == {True, False}
    assert {c.uns for c in dp} == {True, False}
    # the entry point takes the shapes (answered without a launch: a 4-byte-aligned weight pointer is refused AFTER the shape is looked at),
    # and refuses the new bit like every other
    for c in dp:
        g = c.geo
        args = dict(N=g["N"], H=g["H"], W=g["W"], C=g["C"], K=c.k, uns=int(c.uns), w=D.P4)
        assert D.call(N.lib, "dwpw_i8_nhwc", args) == D.EALIGN, c.cid
        args["w"] = D.P             # (the forms are looked at after the alignment, and before anything is launched)
        assert D.call(N.lib, "dwpw_i8_nhwc", dict(args, q2_form=D.ZP | V)) == D.EINVAL and D.call(N.lib, "dwpw_i8_nhwc", dict(args, q_form=D.ZP | V)) == D.EINVAL
        assert D.call(N.lib, "dwpw_i8_nhwc", dict(args, q2_form=D.ZP | V | W.ROUTE_ONLY)) == D.EINVAL, c.cid


def test_the_bit_changes_no_other_answer_and_is_refused_without_route_only():
    N = _lib()
    R = W.ROUTE_ONLY
    # every route query of the refusal sweep (tests/golden/dw_stem_refusals.json) that does not answer ROUTE_DW / ROUTE_DWM answers the same
    # with the bit; those that do answer a record of the right table
    n = 0
    for cid, entry, kw in D.cases():
        a = dict(D.BASE[entry], **kw)
        if entry not in D.DWS or not (a["q_form"] & R) or a["q_form"] < 0:
            continue
        plain, asked = D.call(N.lib, entry, kw), D.call(N.lib, entry, dict(kw, q_form=a["q_form"] | V))
        if plain == D.ROUTE_DW:
            assert W.decode(asked) in W.DW_RECORDS, (cid, asked)
        elif plain == D.ROUTE_DWM:
            assert W.decode(asked) in W.DWM_RECORDS, (cid, asked)
        else:
            assert asked == plain, (cid, plain, asked)
        n += 1
    assert n > 200
    # alone, the bit is refused before anything else is looked at.  These are real calls on placeholder pointers, so the problem is EMPTY
    # (N = 0): a library that lost the check answers DLMCQ_OK for it - this test fails and nothing can be launched either way
    for entry in D.DWS:
        assert D.call(N.lib, entry, dict(N=0)) == 0, entry
        assert D.call(N.lib, entry, dict(N=0, q_form=D.ZP | V)) == D.EINVAL, entry
        assert D.call(N.lib, entry, dict(N=0, q_form=D.ZP | V | D.FORCE_TILED)) == D.EINVAL, entry
        assert D.call(N.lib, entry, dict(N=0, q_form=D.ZP | V, out=D.P, codes=0)) == D.EINVAL, entry          # (with no quantiser to check either)
        assert D.call(N.lib, entry, dict(N=0, q_form=D.ZP | V | R)) == 0, entry                               # with ROUTE_ONLY: answered as without the bit
        assert W.decode(D.call(N.lib, entry, dict(q_form=D.ZP | V | R | D.FORCE_TILED))) == ("dw", "p2", 2, False, entry.endswith("xoff")), entry
    # every entry point that takes no route query refuses it, with `codes`, as it refuses any bit it does not know
    for entry in D.ENTRIES:
        if entry in D.DWS:
            continue
        for form in ("q_form", "q2_form") if entry == "dwpw_i8_nhwc" else ("q_form",):
            assert D.call(N.lib, entry, {form: D.ZP | V}) == D.EINVAL, (entry, form)
            assert D.call(N.lib, entry, {form: D.ZP | V | R}) == D.EINVAL, (entry, form)
    import test_conv_dispatch_host as T
    for entry in T.ENTRIES:
        if entry != "f32":
            assert T.call(N.lib, entry, dict(N=2, H=14, W=14, C=64, K=128, ctl=V)) == T.EINVAL, entry        # (ROUTE_ONLY | the bit)
