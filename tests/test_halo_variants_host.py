"""Which instantiation of conv3x3_halo_i8_kernel / conv3x3_pipe_i8_kernel a call runs, pinned from outside (no GPU): every case of
tests/halo_variant_cases.py is asked with DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_HALO_VARIANT on placeholder pointers and must answer the record it
was written for; together the cases reach the library's two tables (dlmcq_x_conv3x3_variant_table: expanded from the launchers' own
DLMCQ_HALO_TABLE / DLMCQ_PIPE_TABLE) and nothing else; and the tables are the 40 + 6 records written out by hand in the case module.  A change
to halo_variant, conv3x3_halo_applies or conv3x3_pipe_applies that stops reaching a record, or routes a shape to another one, fails here.
Without a GPU the library answers 256 compute units for the pipelined route.

The structural assertions are computed from the geometry: the case module's promises (piece-count boundaries on both sides, chunk-count
residues, more than one frame tile with a partial last one and an image seam inside, a column block at n0 != 0, both input types, zero
points, quantisers, ReLU, a null bias) are proved here, not assumed."""
import halo_variant_cases as H
import test_conv_dispatch_host as D

CUS = 256


def _lib():
    from dlmc import _native as N
    return N


def test_the_tables_are_the_40_and_6_records():
    N = _lib()
    halo, pipe = N.conv3x3_variant_tables()
    assert len(halo) == len(set(halo)) == 40 and len(pipe) == len(set(pipe)) == 6
    assert sorted(halo) == sorted(H.HALO_RECORDS), (sorted(set(halo) - set(H.HALO_RECORDS)), sorted(set(H.HALO_RECORDS) - set(halo)))
    assert sorted(pipe) == sorted(H.PIPE_RECORDS)
    assert N.ROUTE_HALO_VARIANT == 0x20000 and (N.ROUTE_HALO_VARIANT_TAG, N.ROUTE_PIPE_VARIANT_TAG) == (1 << 25, 1 << 26)      # include/dlmcq.h
    assert (N.HV_PLAIN, N.HV_XS, N.HV_S2) == (1, 2, 4)
    # the tiled kernel's decoder rejects these answers, and this one the tiled kernel's
    assert N.decode_variant((1 << 25) | (128 << 16) | (24 << 8) | (2 << 4) | 3) is None and N.decode_variant((1 << 26) | (4 << 8)) is None
    assert N.decode_halo_variant((1 << 24) | (128 << 8) | 10) is None and N.decode_halo_variant(D.ROUTES["halo3x3"]) is None
    assert N.decode_halo_variant(0) is None and N.decode_halo_variant(D.EINVAL) is None


def test_every_case_reaches_the_record_it_names_and_the_cases_reach_both_tables():
    N = _lib()
    got = {c.cid: H.decode(D.call(N.lib, "fused", c.route_args(cus=CUS))) for c in H.CASES}
    wrong = {c.cid: (got[c.cid], c.record) for c in H.CASES if got[c.cid] != c.record}
    assert not wrong, f"(answer, meant) {wrong}"
    for c in H.CASES:                                        # the header's encoding, spelt out
        r = c.record
        want = ((1 << 26) | (r[1] << 8) | (2 if r[2] else 0)) if r[0] == "pipe" else \
            ((1 << 25) | (r[1] << 16) | (r[3] << 8) | (r[4] << 4) | (4 if r[2] else 0) | (2 if r[5] else 0) | (1 if r[6] else 0))
        assert D.call(N.lib, "fused", c.route_args(cus=CUS)) == want, c.cid
        # without the bit: the family, as ever (DLMCQ_ROUTE_VARIANT's meaning is untouched: it changes no 3x3 answer either)
        a = c.route_args(cus=CUS)
        family = D.ROUTES["halo3x3_pipe" if c.pipelined else "halo3x3"]
        assert D.call(N.lib, "fused", dict(a, ctl=a["ctl"] & ~H.ROUTE_HALO_VARIANT)) == family, c.cid
        assert D.call(N.lib, "fused", dict(a, ctl=(a["ctl"] & ~H.ROUTE_HALO_VARIANT) | N.ROUTE_VARIANT)) == family, c.cid
        assert D.call(N.lib, "fused", dict(a, ctl=a["ctl"] | N.ROUTE_VARIANT)) == want, c.cid
    halo, pipe = N.conv3x3_variant_tables()
    assert set(got.values()) == set(halo) | set(pipe)
    for r in H.RECORDS:
        assert len(H.BY_RECORD[r]) >= 2, r
    # a pipelined case without DLMCQ_PIPELINED is the plain halo kernel's PLAIN 128-wide two-buffer record: the GPU test's whole-tensor anchor
    for c in H.CASES:
        if c.pipelined:
            assert H.decode(D.call(N.lib, "fused", c.route_args(cus=CUS, pipelined=False))) == ("halo", 128, False, 24, 2, c.record[2], True), c.cid


def test_the_cases_cover_what_the_case_module_promises():
    narrow_small = {False: (7, 9), True: (12, 16)}
    for r in H.HALO_RECORDS:
        _, bn, s2, hp, nhb, xs, plain = r
        cs = H.BY_RECORD[r]
        stride = 2 if s2 else 1
        widths = set()
        for c in cs:
            g = c.geo
            assert g["stride"] == stride and g["uns"] == int(xs) and (g["R"], g["S"], g["pad"], g["dil"]) == (3, 3, 1, 1), c.cid
            assert stride == 1 or (g["H"] % 2 == 0 and g["W"] % 2 == 0), c.cid
            p, q = c.out_hw()
            widths.add(q)
            need = H.pieces(stride, q)
            assert (need <= hp) and (hp in (24, 18) or need > (24 if hp == 32 else 18)), (c.cid, need)        # the tuple's side of its split
            mq, fs = c.frame()
            assert mq > H.TM and mq % H.TM and g["N"] >= 2 and fs % H.TM, (c.cid, mq, fs)       # > 1 tile, a partial one, a seam inside a tile
            assert (g["K"] % 128 == 0) == (bn == 128), c.cid
            assert nhb == (3 if s2 else (1 if bn == 64 and g["C"] == 64 else 2)), c.cid
        # piece-count boundaries, proved from the formula: the last width on this side of the split, the first on the other, the widest taken
        if not s2:
            assert H.pieces(1, 62) == 24 and H.pieces(1, 63) == 25 and H.pieces(1, 119) == 32      # (W = 120 is conv3x3_halo_applies' limit: below)
            assert (62 in widths) if hp == 24 else ({63, 119} <= widths), (r, widths)
        else:
            assert H.pieces(2, 29) == 18 and H.pieces(2, 30) == 19 and H.pieces(2, 61) == 20 and H.pieces(2, 62) == 21
            assert (29 in widths) if hp == 18 else ({30, 61} <= widths), (r, widths)
        if hp in (24, 18):
            assert any((c.geo["H"], c.geo["W"]) == narrow_small[s2] for c in cs), r                   # a small image
            assert any(c.out_hw() == (1, 1) for c in cs), r                                          # a single output pixel per image
        else:
            assert all(2 <= c.out_hw()[0] <= 5 for c in cs), r
        # chunks
        chunks = [c.geo["C"] // 64 for c in cs]
        if s2:
            assert {4 * n % 3 for n in chunks} == {0, 1, 2}, (r, chunks)
        elif nhb == 2:
            assert {n % 2 for n in chunks} == {0, 1} and min(chunks) >= 2, (r, chunks)
        else:
            assert set(chunks) == {1}, (r, chunks)
        assert any(c.geo["K"] > bn for c in cs), r                                                   # a column block at n0 != 0
        # input zero points, quantisers, activation, bias
        if xs:
            assert {c.zp for c in cs} == {"high", "low"}, r
        else:
            assert any(isinstance(c.zp, int) and c.zp != 0 and abs(c.zp) <= 100 for c in cs), r
        kinds = {c.quant.split("_")[0] for c in cs}
        assert kinds == ({"plain", "shift"} if plain else {"uzp", "signed"}), (r, kinds)
        assert cs[0].quant.endswith("_hi") and {c.relu for c in cs} == {0, 1} and sum(not c.bias for c in cs) == 1, r
    # the widest images taken: one pixel more and the call leaves the halo kernel
    N = _lib()
    wide = dict(N=2, H=4, C=128, K=256, R=3, S=3, pad=1, ctl=H.ROUTE_HALO_VARIANT)
    assert H.decode(D.call(N.lib, "fused", dict(wide, W=119)))[:5] == ("halo", 128, False, 32, 2)
    assert D.call(N.lib, "fused", dict(wide, W=120)) == D.ROUTES["tiled"]
    assert H.decode(D.call(N.lib, "fused", dict(wide, W=122, stride=2)))[:5] == ("halo", 128, True, 20, 3)
    assert D.call(N.lib, "fused", dict(wide, W=124, stride=2)) == D.ROUTES["tiled"]
    for xs in (True, False):                                  # both input types for every tuple
        assert {r[1:5] for r in H.HALO_RECORDS if r[5] == xs} == set(H.TUPLES)
    for r in H.PIPE_RECORDS:
        cs = H.BY_RECORD[r]
        for c in cs:
            g = c.geo_for(CUS)
            assert g["C"] == 64 * r[1] and g["uns"] == int(r[2]) and g["H"] % 2 and g["W"] % 2 and g["W"] < 62 and g["stride"] == 1, c.cid
            mq, fs = c.frame(CUS)
            tiles = -(-mq // H.TM) * (g["K"] // 128)
            grid = min(CUS & ~7, tiles & ~7)
            assert 2 * CUS < tiles < 3 * CUS and tiles % grid and mq % H.TM and fs % H.TM, (c.cid, tiles, grid)
            assert c.quant.split("_")[0] in ("plain", "shift")
        assert {c.relu for c in cs} == {0, 1} and sum(not c.bias for c in cs) == 1 and cs[0].quant.endswith("_hi"), r
    assert {(c.geo["C"], c.geo["K"]) for c in H.CASES if c.pipelined} == {(128, 512), (256, 512), (512, 512), (512, 256)}


def test_the_bit_changes_no_other_answer_and_is_refused_without_route_only():
    N = _lib()
    P = D.P
    V = H.ROUTE_HALO_VARIANT
    geo = dict(N=2, H=48, W=48, C=64, K=128, R=3, S=3, pad=1)
    assert D.call(N.lib, "fused", dict(geo)) == D.ROUTES["halo3x3"]
    assert H.decode(D.call(N.lib, "fused", dict(geo, ctl=V))) == ("halo", 128, False, 24, 2, True, True)
    for ctl in (0, N.ROUTE_VARIANT):
        assert D.call(N.lib, "fused", dict(geo, ctl=ctl | D.FORCE_TILED)) == D.call(N.lib, "fused", dict(geo, ctl=ctl | D.FORCE_TILED | V))
    assert D.call(N.lib, "fused", dict(geo, ctl=D.FORCE_TILED | V)) == D.ROUTES["tiled"]
    assert D.call(N.lib, "fused", dict(N=2, H=48, W=48, C=64, K=128, ctl=V)) == D.ROUTES["pw"]
    assert D.call(N.lib, "fused", dict(geo, N=0, ctl=V)) == 0                                      # an empty problem
    assert D.call(N.lib, "fused", dict(geo, C=32, ctl=V)) == D.EINVAL
    assert D.call(N.lib, "fused", dict(geo, x=D.P4, ctl=V)) == D.EALIGN
    assert D.call(N.lib, "fused", dict(geo, relu=2, ctl=V)) == D.ROUTES["tiled"]                   # (ReLU6: the 3x3 kernels decline it)
    # without DLMCQ_ROUTE_ONLY the bit is refused by every entry point before anything else is looked at.  These are real calls on
    # placeholder pointers, so the problem is EMPTY (N = 0): a library that lost the check answers DLMCQ_OK for it - this test fails and
    # nothing can be launched either way
    for entry in D.ENTRIES:
        if entry in ("f32", "fused_observed"):
            continue        # (f32 has no q_form; the observed entry point refuses an empty problem itself, before conv_launch)
        extra = dict(narrow=dict(Kf=96, out=P), padres=dict(Kf=96, out=P, res=P, res_h=14, res_w=14, res_c=16), dual=dict(out=P)).get(entry, {})
        args = dict(N=0, H=14, W=14, C=64, K=128, R=3, S=3, pad=1, **extra)
        assert H.launch(N.lib, entry, dict(args, ctl=0)) == 0, entry                                      # (the empty problem itself is fine)
        assert H.launch(N.lib, entry, dict(args, ctl=V)) == D.EINVAL, entry
        assert H.launch(N.lib, entry, dict(args, ctl=V | D.FORCE_TILED)) == D.EINVAL, entry
        assert H.launch(N.lib, entry, dict(args, ctl=V | D.PIPELINED)) == D.EINVAL, entry
        assert D.call(N.lib, entry, dict(args, ctl=V)) == 0, entry                                        # with ROUTE_ONLY: answered as without the bit
    # the answers are above every DLMCQ_ROUTE_* and every tiled variant's
    assert (1 << 25) > (1 << 24) | (0xffff << 8) | 0xff
