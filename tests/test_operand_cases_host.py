"""The cases of tests/operand_cases.py on the host (no GPU): every fact a case states is present in its own operands and reference (both clamp
ends, ties on both sides of zero and at the bounds, NaN -> code 0, the all-hi / all-lo sums, zero-filled positions, both image routes for every
C, P == 1, 2 pad == kernel, the minimum-only map, n odd and even on both sides of 16), the float64 and the oracle weight references agree on
every dyadic position, the layout restatements match examples written out by hand, every grid-cap size exceeds the launcher's cap, and the
refusals answer what the table says before anything is launched (placeholder pointers: a refused call touches none)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import exact_layers as X
import operand_cases as W
import test_gpu_epilogue_exact as E
from dlmc import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dlmc-quant_amd", "csrc")
P = ctypes.c_void_p(4096)                   # a 16-byte aligned placeholder: refused calls never touch it


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ weights
@pytest.mark.parametrize("cid", list(W.KRSC_SHAPES))
def test_weight_cases_hold_their_facts_and_both_references_agree(cid):
    shape = W.KRSC_SHAPES[cid][0]
    union = set()
    for lo, hi in W.RANGES:
        for layout in W.SCALE_LAYOUTS:
            wt = W.edge_weights(shape, lo, hi, layout)
            assert tuple(wt.w.shape) == shape and wt.scale.numel() == (1 if layout == "tensor" else shape[0])
            assert layout == "tensor" or wt.scale.dim() == len(shape)
            codes = W.oracle_weight_codes(wt, lo, hi)
            c = codes.reshape(shape[0], -1).numpy().astype(np.float64)
            f64 = W.float64_weight_codes(wt, lo, hi)
            assert (c[wt.dyadic] == f64[wt.dyadic]).all(), (cid, lo, hi, layout)
            assert int(codes.min()) >= lo and int(codes.max()) <= hi
            present = W.weight_facts(wt, codes, lo, hi)
            stated = W.stated_facts(cid, shape, lo, hi, layout)
            assert stated <= present, (cid, lo, hi, layout, stated - present)
            union |= present
            if cid in W.GAUSS_SHAPES:
                g = W.gauss_weights(shape, lo, hi, layout, 2 * (lo + 200) + (layout == "channel"))
                gc = W.oracle_weight_codes(g, lo, hi)
                s = g.s_k.astype(np.float64)
                assert not ((np.log2(s) % 1) == 0).any(), "a Gaussian row's scale is a power of two"
                assert hi == lo or gc.unique().numel() >= min(hi - lo, 12), (cid, lo, hi)
    if cid not in W.SMALL:
        assert W.EDGE_FACTS <= union
    if cid == "linear":
        assert W.CHANNEL_FACTS | {"every_tie"} <= union


def test_dyadic_scales_differ_and_the_special_channels_exist():
    s, kinds = W.channel_scales(10, "channel")
    assert kinds[:5] == ["normal", "normal", "negative", "tiny", "zero"] and s[2] < 0 and s[4] == 0
    with np.errstate(over="ignore"):
        assert np.float32(1e30) / s[3] == np.inf and len({float(v) for v in s}) >= 5
    m, e = np.frexp(np.abs(s[s != 0]))
    assert (m == 0.5).all()                                         # powers of two
    assert len(set(W.channel_scales(10, "tensor")[0].tolist())) == 1


def test_ladder_holds_every_tie_and_reaches_both_ends_first():
    for lo, hi in W.RANGES:
        lad = W.ladder(lo, hi)
        assert sorted(lad.tolist()) == [v / 2 for v in range(2 * lo - 5, 2 * hi + 6)]
        assert lad[0] == hi + 2.5 and lad[1] == lo - 2.5
        assert {hi - 0.5, hi + 0.5, lo - 0.5, lo + 0.5} <= set(lad[:14].tolist())


def test_wsum_rows_sum_to_what_they_claim():
    shape = W.KRSC_SHAPES[W.WSUM_SHAPE][0]
    n = int(np.prod(shape[1:]))
    assert n == 4608
    seen = set()
    for lo, hi in W.RANGES:
        for layout in W.SCALE_LAYOUTS:
            for first in (0, 2):
                wt, roles = W.wsum_weights(shape, lo, hi, layout, first)
                assert wt.dyadic.all()
                codes = W.oracle_weight_codes(wt, lo, hi).reshape(shape[0], -1)
                sums = W.wsum_of(codes)
                for k, role in enumerate(roles):
                    seen.add(int(role))
                    if role == 0:
                        assert bool((codes[k] == hi).all()) and int(sums[k]) == n * hi
                    elif role == 1:
                        assert bool((codes[k] == lo).all()) and int(sums[k]) == n * lo
                    else:
                        assert codes[k, :4].tolist() == [hi, lo, hi, lo] and int(sums[k]) == (n // 2) * (hi + lo)
    assert seen == {0, 1, 2}
    wt, roles = W.wsum_weights(shape, -128, 127, "tensor", 0)
    assert W.wsum_of(W.oracle_weight_codes(wt, -128, 127)).tolist() == [4608 * 127, 4608 * -128] == [585216, -589824]


def test_layouts_match_examples_written_out_by_hand():
    # KRSC: [K = 1][C = 2][R = 1][S = 3] holds 0 1 2 | 3 4 5 (c, s); the (r, s, c) order is 0 3 1 4 2 5
    codes = torch.arange(6, dtype=torch.int8).reshape(1, 2, 1, 3)
    assert W.krsc_layout(codes).reshape(-1).tolist() == [0, 3, 1, 4, 2, 5]
    # [K = 2][C = 2][R = 2][S = 1]: k0 = (c0: 0 1, c1: 2 3), k1 = (c0: 4 5, c1: 6 7) -> k0: r0 (0 2) r1 (1 3), k1: r0 (4 6) r1 (5 7)
    codes = torch.arange(8, dtype=torch.int8).reshape(2, 2, 2, 1)
    assert W.krsc_layout(codes).reshape(-1).tolist() == [0, 2, 1, 3, 4, 6, 5, 7]
    assert W.krsc_layout(torch.arange(6, dtype=torch.int8).reshape(2, 3)).shape == (2, 1, 1, 3)
    for shape in ((5, 7, 1, 3), (5, 7, 3, 1), (2, 3, 3, 3)):
        k_out, c, r, s = shape
        codes = torch.arange(int(np.prod(shape)), dtype=torch.int32).reshape(shape)
        flat = W.krsc_layout(codes).reshape(-1)
        st = W.stem_layout(codes.to(torch.int8)).reshape(-1) if c <= 4 else None
        for (k, ci, ri, si) in ((0, 0, 0, 0), (k_out - 1, c - 1, r - 1, s - 1), (1, 2, r - 1, 0), (1, 1, 0, s - 1)):
            assert int(flat[W.krsc_index(k, ci, ri, si, c, r, s)]) == int(codes[k, ci, ri, si])
            if st is not None:
                assert int(st[W.stem_index(k, ci, ri, si, r)]) == int(codes.to(torch.int8)[k, ci, ri, si])
    # the first layer: [1][1][8][4], tap s and channel c at byte 4 s + c; everything else zero
    codes = torch.tensor([1, 2, 3, 4, 5, 6], dtype=torch.int8).reshape(1, 2, 1, 3)
    assert W.stem_layout(codes).reshape(-1).tolist() == [1, 4, 0, 0, 2, 5, 0, 0, 3, 6, 0, 0] + [0] * 20
    # the dw+pw table: channel -> (chunk, slot)
    assert [W.table_slot(c) for c in (0, 1, 15, 16, 17, 48, 63, 64, 100, 319)] == \
        [(0, 0), (0, 4), (0, 60), (0, 1), (0, 5), (0, 3), (0, 63), (1, 0), (1, 18), (4, 63)]
    assert sorted(W.table_slot(c)[1] for c in range(64)) == list(range(64))
    # ... and one record by hand: taps 1 .. 9, uint8 codes with zero point 3, s_in = 2, s_w = 0.25, o_w = -1, bias = -0
    w = torch.zeros((3, 3, 64), dtype=torch.int8)
    w[:, :, 17] = torch.arange(1, 10, dtype=torch.int8).reshape(3, 3)
    w[:, :, 16] = -1
    bias = torch.zeros(64)
    bias[17] = -0.0
    t = W.table_expected(w, bias, torch.tensor([2.0]), 3.0, torch.full((64,), 0.25), torch.full((64,), -1.0), True)
    as_u32 = lambda v: int(np.array([v], np.float32).view(np.uint32)[0])
    assert [int(v) & 0xffffffff for v in t[0, 5]] == [0x04030201, 0x08070605, 0x00000009, (128 - 3) * 45, as_u32(0.5), as_u32(-2.0), 0x80000000, 0]
    assert [int(v) & 0xffffffff for v in t[0, 1][:4]] == [0xffffffff, 0xffffffff, 0x000000ff, ((128 - 3) * -9) & 0xffffffff]
    t = W.table_expected(w, None, torch.tensor([2.0]), -5.0, torch.full((64,), 0.25), None, False)
    assert [int(v) for v in t[0, 5][3:]] == [5 * 45, as_u32(0.5), 0, 0, 0]


@pytest.mark.parametrize("k_out", W.STEM_K)
def test_stem_cases_have_zero_filled_positions_and_real_sums(k_out):
    combos = [(c, r, s) for c in W.STEM_C for r in W.STEM_R for s in W.STEM_S]
    assert len(combos) == 48 and sum(1 for c, r, s in combos if s < 8 or c < 4) == 45
    for i, (c, r, s) in enumerate(combos):
        lo, hi = W.RANGES[i % len(W.RANGES)]
        shape = (k_out, c, r, s)
        wt = W.edge_weights(shape, lo, hi, W.SCALE_LAYOUTS[i % 2])
        codes = W.oracle_weight_codes(wt, lo, hi)
        lay = W.stem_layout(codes)
        assert lay.shape == (k_out, r, 8, 4)
        real = torch.zeros((r, 8, 4), dtype=torch.bool)
        real[:, :s, :c] = True
        assert int((~real).sum()) == r * (32 - s * c) and bool((lay[:, ~real] == 0).all())
        assert torch.equal(lay.reshape(k_out, -1).to(torch.int64).sum(1), W.wsum_of(codes))
        if r * s * c >= 8 and (lo, hi) != (0, 0):
            assert bool((lay[:, real] != 0).any())


# ------------------------------------------------------------------------------------------------ image
def test_the_image_quantisers_are_the_epilogue_suites():
    assert W.IMAGE_QUANTS == E.ALL_Q + E.SHIFTED and len(W.IMAGE_QUANTS) == 22
    assert W.IMAGE_FILL not in X.EDGE_VALUES and N.PAD_CODE0 == 0x8000 and N.EMIT_SHIFT128 == 0x100
    header = open(os.path.join(ROOT, "include", "dlmcq.h")).read()
    assert "holds code 0 (with DLMCQ_EMIT_SHIFT128: the byte 0x80) instead of the code of x' = 0" in header
    for q in W.IMAGE_QUANTS:
        assert W.border_byte(q, True) == (0x80 if q.shift128 else 0)
        z = int(X.quantise(torch.zeros(1), q).view(torch.uint8))
        assert W.border_byte(q, False) == z
    assert any(W.border_byte(q, False) != W.border_byte(q, True) for q in W.IMAGE_QUANTS)      # (PAD_CODE0 changes a border)


def test_image_geometry_reaches_both_routes_for_every_channel_count():
    cases = list(W.IMAGE_CASES.values())
    for c in (1, 2, 3, 4):
        mine = [k for k in cases if k.c == c]
        assert {k.route for k in mine} == {"x4", "pixel"}
        assert {k.pad for k in mine} == {0, 1, 3} and {k.n for k in mine} == {1, 3} and {k.layout for k in mine} == set(W.IMAGE_LAYOUTS)
        assert {k.w for k in mine if k.layout == "contig" and k.route == "x4"} == {4, 8, 20}
        assert {k.w for k in mine if k.layout == "contig" and k.route == "pixel"} == {5, 18}
        assert any(k.w == 4 and k.route == "x4" and k.pad > 0 for k in mine)               # one group writes both borders
        assert {(k.route, k.pad == 0) for k in mine} >= {("x4", True), ("pixel", True), ("x4", False), ("pixel", False)}


@pytest.mark.parametrize("cid", list(W.IMAGE_CASES))
def test_image_case_takes_its_route_and_holds_its_edges(cid):
    case = W.IMAGE_CASES[cid]
    img = W.image_of(case)
    st, view = W.embed(img, case.layout)
    v = view(st)
    assert tuple(v.shape) == (case.n, case.c, case.h, case.w) and torch.equal(v.contiguous().view(torch.int32), img.view(torch.int32))
    base = v.storage_offset() * 4 % 16                                                # (device allocations are 16-byte aligned: asserted there)
    assert W.image_route(case.c, case.w, v.stride(), base) == case.route
    if case.layout == "wslice":
        assert base == 4 and case.w % 4 == 0                                          # only the base keeps it off the four-pixel route
        assert W.image_route(case.c, case.w, v.stride(), 0) == "x4"
    if case.layout == "hslice":
        assert v.storage_offset() > 0 and base == 0
    if case.twin:
        other = W.IMAGE_CASES[case.twin]
        assert other.twin == cid and other.route != case.route and torch.equal(W.image_of(other).view(torch.int32), img.view(torch.int32))
    ev = torch.tensor(X.EDGE_VALUES, dtype=torch.float32).view(torch.int32).tolist()
    ties = edges = 0
    for b in range(case.n):
        for ch in range(case.c):
            for (y, x) in W.corner_pixels(case.h, case.w):
                val = img[b, ch, y, x]
                is_tie = float(val) in W.CORNER_TIES
                ties += is_tie
                edges += int(val.view(torch.int32)) in ev
                assert is_tie or int(val.view(torch.int32)) in ev
    assert ties >= 2 and edges >= 2 and bool(img.isnan().any())
    q = W.IMAGE_QUANTS[0]
    for code0 in (False, True):
        want = W.image_expected(img, case.pad, q, code0)
        p, h, w = case.pad, case.h, case.w
        assert want.shape == (case.n, h + 2 * p, w + 2 * p, 4)
        inner = want[:, p:p + h, p:p + w]
        assert bool((inner[..., case.c:] == 0).all())
        assert torch.equal(inner[..., :case.c], X.quantise(img.permute(0, 2, 3, 1).contiguous(), q).view(torch.uint8))
        if p:
            assert bool((want[:, :p] == W.border_byte(q, code0)).all()) and bool((want[:, :, -p:] == W.border_byte(q, code0)).all())
            assert bool((want[:, -p:] == W.border_byte(q, code0)).all()) and bool((want[:, :, :p] == W.border_byte(q, code0)).all())


# ------------------------------------------------------------------------------------------------ pool
def test_pool_cases_reach_what_they_claim():
    cases = W.POOL_CASES
    assert cases["p1q1"].pq == (1, 1) and cases["p1q1"].route == "vec" and cases["p1q1"].c // 16 == 1
    assert 2 * cases["pad_half"].p == cases["pad_half"].k and cases["c4"].c // 4 == 1
    for cid, case in cases.items():
        assert case.c % 4 == 0 and 2 * case.p <= case.k and min(case.pq) >= 1
        if case.offset:
            twin = cases[cid[:-5]]
            assert case.offset % 16 == 4 and case.c % 16 == 0 and case.route == "dword" and twin.route == "vec"
            assert (twin.n, twin.c, twin.h, twin.w, twin.k, twin.s, twin.p) == (case.n, case.c, case.h, case.w, case.k, case.s, case.p)
    assert {c.c for c in cases.values() if c.offset} == {16, 64} and {c.route for c in cases.values() if c.c % 16} == {"dword"}
    for what, (n, h, w, c, k, s, p), offset, rc in W.POOL_REFUSALS:
        bad = [c % 4 != 0, 2 * p > k, (h + 2 * p - k) // s + 1 < 1 or (w + 2 * p - k) // s + 1 < 1, offset % 4 != 0]
        assert sum(bad) == 1, what                                                        # each refusal for one reason only
        fake = ctypes.c_void_p(4096 + offset)
        assert N.lib.dlmcq_maxpool_codes_nhwc(fake, fake, n, h, w, c, k, s, p, 1, None) == rc, what


@pytest.mark.parametrize("cid", list(W.POOL_CASES))
def test_pool_contents_hold_every_byte_the_minimum_and_single_maxima(cid):
    case = W.POOL_CASES[cid]
    for unsigned in (True, False):
        lowest = 0 if unsigned else -128
        x = W.pool_codes(case, "bytes", unsigned)
        assert x.dtype == (torch.uint8 if unsigned else torch.int8) and x.unique().numel() == min(256, x.numel())
        y = W.pool_expected(x, case)
        assert y.shape == (case.n, *case.pq, case.c) and y.dtype == x.dtype
        x = W.pool_codes(case, "minimum", unsigned)
        assert bool((x == lowest).all()) and bool((W.pool_expected(x, case) == lowest).all())         # never what padding would give
        x = W.pool_codes(case, "corners", unsigned)
        y = W.pool_expected(x, case).to(torch.int64)
        assert int((x.to(torch.int64) != lowest).sum()) == case.n * case.c * len(set(W.corner_pixels(case.h, case.w)))
        ch, cw = W.windows_covering(case.h, case.k, case.s, case.p, 0), W.windows_covering(case.w, case.k, case.s, case.p, 0)
        top_left = x[:, 0, 0, :].to(torch.int64)
        hits = (y == top_left[:, None, None, :]).sum(dim=(1, 2))
        if case.k - case.p < min(case.h, case.w):                                          # (the first window holds no second corner)
            assert bool((hits >= ch * cw).all()) and bool((y[:, 0, 0, :] == top_left).all())
        if cid != "k5s1":
            assert ch * cw == 1                                                            # exactly one window covers the corner
    assert W.windows_covering(7, 5, 1, 2, 0) == 3


# ------------------------------------------------------------------------------------------------ pack
def test_pack_sizes_and_contents():
    odd, even = [n for n in W.PACK_N if n % 2], [n for n in W.PACK_N if n % 2 == 0]
    assert any(n < 16 for n in odd) and any(n > 16 for n in odd) and any(n < 16 for n in even) and any(n > 16 for n in even)
    assert {15, 16, 17, 31, 32, 33} <= set(W.PACK_N) and 4111 % 16 == 15 and 4111 > 16 * 256
    for n in W.PACK_N:
        for signed in (True, False):
            c = W.nibble_codes(n, signed, n)
            lo = -8 if signed else 0
            assert int(c.min()) >= lo and int(c.max()) <= lo + 15
            if n >= 16:
                assert c.unique().numel() == 16 and int(c.min()) == lo
            p = W.pack_expected(c)
            assert p.numel() == (n + 1) // 2 and torch.equal(W.unpack_expected(p, n, signed), c)
            assert int(p[0]) == (int(c[0]) & 15) | ((int(c[1]) & 15) << 4 if n > 1 else 0)
            if n % 2:
                assert int(p[-1]) >> 4 == 0
                dirty = p.clone()
                dirty[-1] |= 0xF0
                assert torch.equal(W.unpack_expected(dirty, n, signed), c)
    assert W.pack_expected(torch.tensor([-8, 7, -1], dtype=torch.int8)).tolist() == [0x78, 0x0F]
    assert W.unpack_expected(torch.tensor([0x78, 0x0F], dtype=torch.uint8), 3, True).tolist() == [-8, 7, -1]
    assert W.unpack_expected(torch.tensor([0x78, 0x0F], dtype=torch.uint8), 3, False).tolist() == [8, 7, 15]
    assert {o % 16 for o in W.CODE_OFFSETS} == {0, 1, 4, 15} and {o % 8 for o in W.PACKED_OFFSETS} == {0, 1, 4}


# ------------------------------------------------------------------------------------------------ table
def test_table_operands_cover_the_byte_range_and_the_bias_bits():
    assert W.TABLE_C == (64, 128, 320) and (320 + 255) // 256 == 2                     # the last needs two workgroups
    for c in W.TABLE_C:
        w, s_w, o_w, bias, s_in = W.table_operands(c, c)
        assert w.unique().numel() == 256 and int(w.reshape(9, c).to(torch.int64).sum(0).max()) == 9 * 127
        assert int(w.reshape(9, c).to(torch.int64).sum(0).min()) == 9 * -128
        bits = set((bias.view(torch.int32).to(torch.int64) & 0xffffffff).tolist())
        assert set(W.BIAS_BITS) <= bits and bool(bias.isnan().any())
        t = W.table_expected(w, bias, s_in, 131.0, s_w, o_w, True)
        assert t.shape == (c // 64, 64, 8) and bool((t[..., 7] == 0).all())
        assert {int(v) & 0xffffffff for v in t[..., 6].reshape(-1)} >= set(W.BIAS_BITS)
        assert not torch.equal(t, W.table_expected(w, bias, s_in, 77.0, s_w, o_w, True))
    v = W.TABLE_VARIANTS
    assert {(b, o) for b, o, _, _ in v} == {(True, True), (True, False), (False, True), (False, False)}
    assert any(u and z > 128 for _, _, u, z in v) and any(u and z < 128 for _, _, u, z in v) and any(not u for _, _, u, _ in v)
    for what, c, offset, rc in W.TABLE_REFUSALS:
        assert N.lib.dlmcq_dwpw_pack_table(P, P, P, P, P, P, c, 1, ctypes.c_void_p(4096 + offset), None) == rc, what


# ------------------------------------------------------------------------------------------------ refusals and grid caps
@pytest.mark.parametrize("name", ["krsc", "stem"])
def test_weight_refusals_answer_before_anything_is_launched(name):
    entry = N.lib.dlmcq_quantize_weight_krsc_i8 if name == "krsc" else N.lib.dlmcq_quantize_weight_stem_i8
    for what, over, null, rc_krsc, rc_stem in W.WEIGHT_REFUSALS:
        rc_want = rc_krsc if name == "krsc" else rc_stem
        if rc_want is None:
            continue
        a = dict(W.REFUSAL_BASE, **over)
        ptrs = [P, P, P, P]
        if null is not None:
            ptrs[null] = None
        assert entry(*ptrs, a["K"], a["C"], a["R"], a["S"], a["lo"], a["hi"], None) == rc_want, (name, what)
    if name == "stem":
        a = W.REFUSAL_BASE
        assert entry(P, ctypes.c_void_p(4100), P, P, a["K"], a["C"], a["R"], a["S"], a["lo"], a["hi"], None) == W.EALIGN


def test_every_grid_cap_size_exceeds_its_cap():
    internal = source("dlmcq_internal.h")
    cus = int(re.search(r"#define DLMCQ_CUS (\d+)", internal).group(1))
    block = int(re.search(r"#define DLMCQ_BLOCK (\d+)", internal).group(1))
    assert not hasattr(N, "CUS")                                     # (the package exports neither constant: they are read from the source)
    assert "if (b > DLMCQ_CUS * 16) b = DLMCQ_CUS * 16;" in source("pack.hip")
    stem = source("conv_stem_i8.hip")
    assert stem.count("blocks < 65536 ? blocks : 65536") == 3 and stem.count("b4 < 65536 ? b4 : 65536") == 2
    n = W.GRID_CAP["pack"]["n"]
    assert ((n >> 4) + block - 1) // block > cus * 16 and n % 16 and n % 2          # a second vector trip, a scalar remainder, an odd n
    assert n == (1 << 24) + 4096 + 5 and n < 70e6
    g = W.GRID_CAP["image"]
    assert g["w"] % 4 and g["n"] * g["h"] * g["w"] > 65536 * block and g["n"] * g["h"] * g["w"] * 4 < 70e6
    g = W.GRID_CAP["pool"]
    assert g["k"] == 1 and g["n"] * g["h"] * g["w"] * (g["c"] // 4) > 65536 * block and g["n"] * g["h"] * g["w"] * g["c"] < 70e6
