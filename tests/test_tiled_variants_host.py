"""Which instantiation of conv_i8_mfma_kernel a call runs, pinned from outside (no GPU): every case of tests/tiled_variant_cases.py is
asked with DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_VARIANT on placeholder pointers and must answer the (tile width, flags) pair it was written
for; together the cases reach the library's whole table (dlmcq_x_conv_variant_table: expanded from the launcher's own DLMCQ_CV_TABLE) and
nothing else; and the table is the 48 pairs written out by hand in the case module.  A change to conv_plan, swap_ok or the 192- / 256-wide
adjustments that stops reaching a pair, or routes a shape to another one, fails here.

UNREACHABLE: pairs of the table no call through the ABI reaches - each an asserted exception with its reason.  None is known."""
import test_conv_dispatch_host as D
import tiled_variant_cases as V

UNREACHABLE = {}        # pair -> the reason, from csrc/conv_i8.hip


def _lib():
    from dlmc import _native as N
    return N


def test_the_table_is_the_48_pairs():
    N = _lib()
    table = N.conv_variant_table()
    assert len(table) == len(set(table)) == 48
    assert table == V.PAIRS, (sorted(set(table) - set(V.PAIRS)), sorted(set(V.PAIRS) - set(table)))
    assert (N.CV_DUAL, N.CV_ADIR, N.CV_ASYM, N.CV_SWAP, N.CV_R6, N.CV_XOFF, N.CV_NARROW, N.CV_PADRES) == (1, 2, 4, 8, 16, 32, 64, 128)
    assert N.ROUTE_VARIANT == 0x10000 and N.ROUTE_VARIANT_TAG == 1 << 24                      # include/dlmcq.h


def test_every_case_reaches_the_pair_it_names_and_the_cases_reach_the_whole_table():
    N = _lib()
    got = {c.cid: V.decode(D.call(N.lib, c.entry, c.route_args())) for c in V.CASES}
    wrong = {c.cid: (got[c.cid], c.pair) for c in V.CASES if got[c.cid] != c.pair}
    assert not wrong, f"(answer, meant) {wrong}"
    for c in V.CASES:                                        # the header's encoding, spelt out: tag | width << 8 | flags
        assert D.call(N.lib, c.entry, c.route_args()) == (1 << 24) | (c.pair[0] << 8) | c.pair[1], c.cid
    assert set(got.values()) | set(UNREACHABLE) == set(N.conv_variant_table()) and not set(got.values()) & set(UNREACHABLE)
    assert len(UNREACHABLE) == 0
    for pair in V.PAIRS:
        assert len(V.BY_PAIR[pair]) >= 2, pair


def test_the_cases_cover_what_the_case_module_promises():
    for pair, cs in V.BY_PAIR.items():
        steps = [c.steps for c in cs]
        assert any(s >= 7 and s % 3 != min(steps) % 3 for s in steps), (pair, steps)       # the ring wraps at another phase
        assert {c.geo["uns"] for c in cs} == {0, 1}, pair
        for c in cs:
            g = dict(D.BASE, **c.geo)
            p = (g["H"] + 2 * g["pad"] - g["dil"] * (g["R"] - 1) - 1) // g["stride"] + 1
            q = (g["W"] + 2 * g["pad"] - g["dil"] * (g["S"] - 1) - 1) // g["stride"] + 1
            m = g["N"] * p * q
            assert m > 128 and m % 128 and (p * q) % 128 and g["N"] >= 2, (c.cid, m)         # > 1 row tile, a partial one, a seam inside a tile
        if pair[1] & V.CV_ADIR:
            assert any((c.geo["R"], c.geo["stride"], c.geo["pad"], c.geo["H"] % 2, c.geo["W"] % 2) in ((3, 2, 1, 1, 0), (3, 2, 1, 1, 1)) for c in cs), pair
            assert any(c.geo["dil"] == 2 for c in cs), pair
        if not pair[1] & (V.CV_NARROW | V.CV_PADRES):
            assert any(c.geo["K"] > pair[0] for c in cs), pair                                # a column tile at n0 != 0
    ragged = {k for c in V.CASES if c.pair in ((64, V.CV_ADIR), (64, V.CV_ADIR | V.CV_ASYM)) for k in (c.geo["K"],)}
    assert {72, 42} <= ragged


def test_the_bit_changes_no_other_answer_and_is_refused_without_route_only():
    N = _lib()
    P = D.P
    geo = dict(N=2, H=48, W=48, C=64, K=128, R=3, S=3, pad=1)
    for ctl, want in ((0, D.ROUTES["halo3x3"]), (D.FORCE_TILED, None)):
        plain = D.call(N.lib, "fused", dict(geo, ctl=ctl))
        asked = D.call(N.lib, "fused", dict(geo, ctl=ctl | V.ROUTE_VARIANT))
        if want is None:
            assert plain == D.ROUTES["tiled"] and V.decode(asked) == (128, V.CV_ADIR | V.CV_SWAP)
        else:
            assert plain == asked == want
    assert D.call(N.lib, "fused", dict(N=2, H=48, W=48, C=64, K=128, ctl=V.ROUTE_VARIANT)) == D.ROUTES["pw"]
    assert D.call(N.lib, "fused", dict(geo, N=0, ctl=V.ROUTE_VARIANT)) == 0                                      # an empty problem
    assert D.call(N.lib, "fused", dict(geo, C=32, ctl=V.ROUTE_VARIANT | D.FORCE_TILED)) == D.EINVAL
    assert D.call(N.lib, "fused", dict(geo, x=D.P4, ctl=V.ROUTE_VARIANT | D.FORCE_TILED)) == D.EALIGN
    # without DLMCQ_ROUTE_ONLY the bit is refused by every entry point before anything else is looked at.  These are real calls on
    # placeholder pointers, so the problem is EMPTY (N = 0): a library that lost the check answers DLMCQ_OK for it - this test fails and
    # nothing can be launched either way
    for entry in D.ENTRIES:
        if entry in ("f32", "fused_observed"):
            continue        # (f32 has no q_form; the observed entry point refuses an empty problem itself, before conv_launch)
        extra = dict(narrow=dict(Kf=96, out=P), padres=dict(Kf=96, out=P, res=P, res_h=14, res_w=14, res_c=16), dual=dict(out=P)).get(entry, {})
        args = dict(N=0, H=14, W=14, C=64, K=128, R=3, S=3, pad=1, **extra)
        assert V.launch(N.lib, entry, dict(args, ctl=0)) == 0, entry                                      # (the empty problem itself is fine)
        assert V.launch(N.lib, entry, dict(args, ctl=V.ROUTE_VARIANT)) == D.EINVAL, entry
        assert V.launch(N.lib, entry, dict(args, ctl=V.ROUTE_VARIANT | D.FORCE_TILED)) == D.EINVAL, entry
        assert D.call(N.lib, entry, dict(args, ctl=V.ROUTE_VARIANT)) == 0, entry                          # with ROUTE_ONLY: answered as without the bit
    # the answers are above every DLMCQ_ROUTE_*
    assert all(((1 << 24) | bn << 8 | f) > max(D.ROUTES.values()) + 8 for bn, f in V.PAIRS)
