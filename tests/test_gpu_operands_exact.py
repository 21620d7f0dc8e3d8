"""The operand-preparation kernels - weights to KRSC / first-layer codes, images to padded NHWC4 codes, max-pool on codes, 4-bit pack and
unpack, the dw+pw constant table - launched on the calls of tests/operand_cases.py and compared with its references byte for byte: no
tolerance anywhere.  Every output is written through the raw entry point into a buffer filled with a sentinel (both fills of
operand_cases.SENTINELS where it is cheap) with guard bytes behind it, and the WHOLE buffer is compared: a byte the kernel should have written
that still shows the fill fails, and so does a guard byte (or the image buffer's 32 bytes of slack) that changed.  The wrappers of
dlmc.quantization.scalar.kernels must return the same bytes.  tests/test_operand_cases_host.py proves on the CPU that the cases hold what
they claim."""
import time

import pytest
import torch

import exact_layers as X
import operand_cases as W
from test_gpu_epilogue_exact import expect_codes, tagged

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def lib():
    from dlmc import _native as N
    return N


def kernels():
    from dlmc.quantization.scalar import kernels as K
    return K


def dev(t):
    return None if t is None else t.to(DEV)


def guarded(nbytes, fill, offset=0, slack=0):
    """A uint8 device buffer of `fill`: `offset` bytes, the output's nbytes (+ slack), W.GUARD bytes.  Returns (buffer, the output's view)."""
    buf = torch.full((offset + nbytes + slack + W.GUARD,), fill, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[offset:offset + nbytes]


def whole(buf, want, fill, offset, what, errs):
    """The whole buffer against fill | want | fill."""
    got = buf.cpu()
    exp = torch.full_like(got, fill)
    wb = want.contiguous().view(-1).view(torch.uint8)
    exp[offset:offset + wb.numel()] = wb
    if not torch.equal(got, exp):
        bad = (got != exp).nonzero().flatten()
        where = [(int(i) - offset, int(got[i]), int(exp[i])) for i in bad[:4]]
        kept = int(((got != exp) & (got == fill))[offset:offset + wb.numel()].sum())
        outside = int((bad < offset).sum() + (bad >= offset + wb.numel()).sum())
        errs.append(f"{what}: {bad.numel()} bytes differ ({kept} never written, {outside} outside the output), e.g. (byte, got, want) {where}")


def settle(errs):
    assert not errs, f"{len(errs)} mismatches:\n" + "\n".join(errs[:20])


# ------------------------------------------------------------------------------------------------ weights
def raw_weights(entry, wt, shape4, lo, hi, out_bytes, fill):
    N = lib()
    k_out = shape4[0]
    w, scale = dev(wt.w).contiguous(), dev(torch.from_numpy(wt.s_k.copy()))
    qbuf, q = guarded(out_bytes, fill)
    sbuf, s = guarded(4 * k_out, fill)
    rc = entry(N.ptr(w), N.ptr(q), N.ptr(s), N.ptr(scale), *shape4, lo, hi, N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return qbuf, sbuf


def check_weights(name, wt, shape, lo, hi, layout_of, errs, what, wrapper=True, wsum_roles=None):
    """One weight tensor through the raw entry point (both fills) and the wrapper; `layout_of`: codes [K, C, R, S] -> the entry point's layout."""
    N, K = lib(), kernels()
    entry = N.lib.dlmcq_quantize_weight_krsc_i8 if name == "krsc" else N.lib.dlmcq_quantize_weight_stem_i8
    shape4 = tuple(shape) + (1, 1) * (len(shape) == 2)
    codes = W.oracle_weight_codes(wt, lo, hi).reshape(shape4)
    want_q, want_s = layout_of(codes), W.wsum_of(codes).to(torch.int32)
    if wsum_roles is not None:
        n = codes[0].numel()
        for k, role in enumerate(wsum_roles):
            assert int(want_s[k]) == (n * hi, n * lo, ((n + 1) // 2) * hi + (n // 2) * lo)[role]
    for fill in W.SENTINELS:
        qbuf, sbuf = raw_weights(entry, wt, shape4, lo, hi, want_q.numel(), fill)
        whole(qbuf, want_q, fill, 0, f"{what} codes (fill {fill:#x})", errs)
        whole(sbuf, want_s, fill, 0, f"{what} wsum (fill {fill:#x})", errs)
    if wrapper:
        fn = K.quantize_weight_krsc if name == "krsc" else K.quantize_weight_stem
        gq, gs = fn(dev(wt.w), dev(wt.scale), lo, hi)
        if not (torch.equal(gq.cpu(), want_q) and torch.equal(gs.cpu(), want_s)):
            errs.append(f"{what}: the wrapper's codes or sums differ")


@pytest.mark.parametrize("cid", list(W.KRSC_SHAPES))
def test_weight_krsc_codes_are_exact(cid):
    shape = W.KRSC_SHAPES[cid][0]
    errs = []
    for lo, hi in W.RANGES:
        for layout in W.SCALE_LAYOUTS:
            what = f"krsc {cid} [{lo}, {hi}] {layout}"
            check_weights("krsc", W.edge_weights(shape, lo, hi, layout), shape, lo, hi, W.krsc_layout, errs, what + " edge")
            if cid == W.WSUM_SHAPE:
                for first in (0, 2):
                    wt, roles = W.wsum_weights(shape, lo, hi, layout, first)
                    check_weights("krsc", wt, shape, lo, hi, W.krsc_layout, errs, what + f" wsum rows {first}", wsum_roles=roles)
            if cid in W.GAUSS_SHAPES:
                check_weights("krsc", W.gauss_weights(shape, lo, hi, layout, 2 * (lo + 200) + (layout == "channel")), shape, lo, hi, W.krsc_layout, errs, what + " gauss")
    settle(errs)


@pytest.mark.parametrize("k_out", W.STEM_K)
def test_weight_stem_codes_and_zero_fill_are_exact(k_out):
    errs, i = [], 0
    for c in W.STEM_C:
        for r in W.STEM_R:
            for s in W.STEM_S:
                for lo, hi in W.RANGES:
                    layout = W.SCALE_LAYOUTS[i % 2]
                    shape = (k_out, c, r, s)
                    what = f"stem {shape} [{lo}, {hi}] {layout}"
                    check_weights("stem", W.edge_weights(shape, lo, hi, layout), shape, lo, hi, W.stem_layout, errs, what + " edge",
                                  wrapper=i % 4 == 0)
                    i += 1
        wt, roles = W.wsum_weights((k_out, c, 7, 7), -128, 127, "channel", c)
        check_weights("stem", wt, (k_out, c, 7, 7), -128, 127, W.stem_layout, errs, f"stem K {k_out} C {c} wsum rows", wsum_roles=roles)
        check_weights("stem", W.gauss_weights((k_out, c, 7, 7), -127, 127, "channel", c), (k_out, c, 7, 7), -127, 127, W.stem_layout, errs,
                      f"stem K {k_out} C {c} gauss")
    settle(errs)


@pytest.mark.parametrize("name", ["krsc", "stem"])
def test_weight_refusals_write_nothing(name):
    N = lib()
    entry = N.lib.dlmcq_quantize_weight_krsc_i8 if name == "krsc" else N.lib.dlmcq_quantize_weight_stem_i8
    fill = W.SENTINELS[0]
    big = 1 << 16                                                 # (placeholders larger than anything a refused call would touch if it ran)
    w = torch.ones(big // 4, dtype=torch.float32, device=DEV)
    scale = torch.ones(64, dtype=torch.float32, device=DEV)
    cases = [(what, over, null, (rc_krsc if name == "krsc" else rc_stem)) for what, over, null, rc_krsc, rc_stem in W.WEIGHT_REFUSALS]
    cases = [c for c in cases if c[3] is not None]
    for what, over, null, rc_want in cases:
        a = dict(W.REFUSAL_BASE, **over)
        qbuf, q = guarded(big, fill)
        sbuf, s = guarded(256, fill)
        ptrs = [N.ptr(w), N.ptr(q), N.ptr(s), N.ptr(scale)]
        if null is not None:
            ptrs[null] = None
        rc = entry(*ptrs, a["K"], a["C"], a["R"], a["S"], a["lo"], a["hi"], N.stream_ptr())
        torch.cuda.synchronize()
        assert rc == rc_want, (name, what, rc)
        assert bool((qbuf == fill).all()) and bool((sbuf == fill).all()), (name, what, "an output was written")
    if name == "stem":                                            # wq 4 bytes past a 16-byte boundary
        qbuf, _ = guarded(big, fill, offset=4)
        sbuf, s = guarded(256, fill)
        a = W.REFUSAL_BASE
        rc = entry(N.ptr(w), N.ptr(qbuf[4:]), N.ptr(s), N.ptr(scale), a["K"], a["C"], a["R"], a["S"], a["lo"], a["hi"], N.stream_ptr())
        torch.cuda.synchronize()
        assert rc == W.EALIGN and bool((qbuf == fill).all()) and bool((sbuf == fill).all())


# ------------------------------------------------------------------------------------------------ image -> padded NHWC4 codes
def image_form(N, q, code0):
    return int(q.form) | (N.EMIT_SHIFT128 if q.shift128 else 0) | (N.PAD_CODE0 if code0 else 0)


def raw_image(x, pad, q, code0, fill):
    """dlmcq_quantize_pad_nhwc4 on the (N, C, H, W) device view x: (whole buffer, payload bytes)."""
    N = lib()
    n, c, h, w = x.shape
    nbytes = n * (h + 2 * pad) * (w + 2 * pad) * 4
    buf, out = guarded(nbytes, fill, slack=W.IMAGE_SLACK)
    scale = torch.tensor([q.scale], dtype=torch.float32, device=DEV)
    zp = None if q.zp is None else torch.tensor([q.zp], dtype=torch.float32, device=DEV)
    rc = N.lib.dlmcq_quantize_pad_nhwc4(N.ptr(x), N.ptr(out), N.ptr(scale), N.ptr(zp), n, c, h, w, *x.stride(), pad, q.lo, q.hi,
                                        image_form(N, q, code0), float(q.g), N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return buf, nbytes


def device_view(case):
    img = W.image_of(case)
    st, view = W.embed(img, case.layout)
    std = st.to(DEV)
    assert std.data_ptr() % 16 == 0
    x = view(std)
    route = W.image_route(case.c, case.w, x.stride(), x.data_ptr() % 16)
    assert route == case.route, (case.cid, route)
    return img, std, x


@pytest.mark.parametrize("cid", list(W.IMAGE_CASES))
def test_image_codes_borders_and_slack_are_exact(cid):
    K = kernels()
    case = W.IMAGE_CASES[cid]
    img, _keep, x = device_view(case)
    padded = W.padded_nhwc(img, case.pad)
    errs = []
    for qi, q in enumerate(W.IMAGE_QUANTS):
        codes = expect_codes(K, padded, q)
        for code0 in (False, True):
            want = W.image_expected(img, case.pad, q, code0, codes)
            for fill in (W.SENTINELS if not code0 else W.SENTINELS[qi % 2:qi % 2 + 1]):
                buf, _ = raw_image(x, case.pad, q, code0, fill)
                whole(buf, want, fill, 0, f"{cid} {q.tag()} code0={code0} (fill {fill:#x})", errs)
            if qi % 5 == 0:
                got, tags = tagged(K, lambda: K.quantize_pad_nhwc4(x, torch.tensor([q.scale], device=DEV),
                                                                    None if q.zp is None else torch.tensor([q.zp], device=DEV), q.lo, q.hi,
                                                                    q.form, case.pad, g=q.g, shift128=q.shift128, pad_code0=code0))
                assert tags == ["fq_image"], tags
                if not torch.equal(got.cpu().view(torch.uint8), want):
                    errs.append(f"{cid} {q.tag()} code0={code0}: the wrapper's bytes differ")
    settle(errs)


@pytest.mark.parametrize("cid", [c.cid for c in W.IMAGE_CASES.values() if c.twin and c.route == "x4"])
def test_both_image_routes_give_the_same_bytes(cid):
    a, b = W.IMAGE_CASES[cid], W.IMAGE_CASES[W.IMAGE_CASES[cid].twin]
    (_, _ka, xa), (_, _kb, xb) = device_view(a), device_view(b)
    assert {a.route, b.route} == {"x4", "pixel"} and torch.equal(xa.cpu().view(torch.int32), xb.cpu().view(torch.int32))
    for q in W.IMAGE_QUANTS:
        for code0 in (False, True):
            (ba, na), (bb, nb) = raw_image(xa, a.pad, q, code0, 0x5A), raw_image(xb, b.pad, q, code0, 0x5A)
            assert na == nb and torch.equal(ba, bb), (cid, q.tag(), code0)


# ------------------------------------------------------------------------------------------------ max-pool on codes
def raw_pool(x_nhwc, geom, unsigned, offset, fill, out_bytes):
    N = lib()
    n, h, w, c, k, s, p = geom
    xb = torch.full((offset + x_nhwc.numel() + 16,), fill, dtype=torch.uint8, device=DEV)
    xb[offset:offset + x_nhwc.numel()] = dev(x_nhwc.contiguous().view(-1).view(torch.uint8))
    ybuf, y = guarded(out_bytes, fill, offset=offset)
    rc = N.lib.dlmcq_maxpool_codes_nhwc(N.ptr(xb[offset:]), N.ptr(y), n, h, w, c, k, s, p, int(unsigned), N.stream_ptr())
    torch.cuda.synchronize()
    return rc, ybuf


@pytest.mark.parametrize("cid", list(W.POOL_CASES))
def test_pooled_codes_are_exact(cid):
    K = kernels()
    case = W.POOL_CASES[cid]
    errs = []
    for unsigned in (True, False):
        for content in W.POOL_CONTENTS:
            x = W.pool_codes(case, content, unsigned)
            want = W.pool_expected(x, case)
            if content == "minimum":
                assert bool((want == (0 if unsigned else -128)).all())
            for fill in W.SENTINELS:
                rc, ybuf = raw_pool(x, (case.n, case.h, case.w, case.c, case.k, case.s, case.p), unsigned, case.offset, fill, want.numel())
                assert rc == 0, rc
                whole(ybuf, want, fill, case.offset, f"{cid} {content} {'u8' if unsigned else 'i8'} (fill {fill:#x})", errs)
            if case.offset == 0:
                got = K.maxpool_codes(dev(x).permute(0, 3, 1, 2), case.k, case.s, case.p)
                if not torch.equal(got.permute(0, 2, 3, 1).cpu(), want):
                    errs.append(f"{cid} {content}: the wrapper's codes differ")
    settle(errs)


def test_pool_refusals_write_nothing():
    fill = W.SENTINELS[0]
    x = torch.zeros((1 << 14,), dtype=torch.uint8)
    for what, geom, offset, rc_want in W.POOL_REFUSALS:
        rc, ybuf = raw_pool(x, geom, True, offset, fill, 1 << 14)      # (placeholders larger than what the call would touch if it ran)
        assert rc == rc_want, (what, rc)
        assert bool((ybuf == fill).all()), (what, "the output was written")


# ------------------------------------------------------------------------------------------------ pack / unpack
def raw_pack(codes, code_off, packed_off, fill):
    N = lib()
    n = codes.numel()
    cb = torch.full((code_off + n + 16,), fill, dtype=torch.uint8, device=DEV)
    cb[code_off:code_off + n] = dev(codes.view(torch.uint8))
    pbuf, p = guarded((n + 1) // 2, fill, offset=packed_off)
    rc = N.lib.dlmcq_pack_int4(N.ptr(cb[code_off:]), N.ptr(p), n, N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return pbuf


def raw_unpack(packed, n, signed, code_off, packed_off, fill):
    N = lib()
    pb = torch.full((packed_off + packed.numel() + 16,), fill, dtype=torch.uint8, device=DEV)
    pb[packed_off:packed_off + packed.numel()] = dev(packed)
    cbuf, c = guarded(n, fill, offset=code_off)
    rc = N.lib.dlmcq_unpack_int4(N.ptr(pb[packed_off:]), N.ptr(c), n, int(signed), N.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return cbuf


@pytest.mark.parametrize("n", W.PACK_N)
def test_pack_and_unpack_are_exact_on_every_alignment(n):
    errs = []
    for signed in (True, False):
        codes = W.nibble_codes(n, signed, n)
        packed = W.pack_expected(codes)
        assert n % 2 == 0 or int(packed[-1]) >> 4 == 0
        dirty = packed.clone()
        if n % 2:
            dirty[-1] |= 0xF0                       # the nibble behind an odd n: unpack must not write it out as codes[n]
        for co in W.CODE_OFFSETS:
            for po in W.PACKED_OFFSETS:
                for fill in W.SENTINELS:
                    what = f"n={n} signed={signed} codes+{co} packed+{po} (fill {fill:#x})"
                    whole(raw_pack(codes, co, po, fill), packed, fill, po, "pack " + what, errs)
                    whole(raw_unpack(dirty, n, signed, co, po, fill), codes, fill, co, "unpack " + what, errs)
    settle(errs)


def test_pack_wrappers_on_offset_views():
    """kernels.pack_int4 on a misaligned view and kernels.unpack_int4(out=...) into an offset of a larger buffer, as PackedWeights4 expands
    its weights: the same bytes as on aligned tensors, nothing written around them."""
    K = kernels()
    for n in (33, 4111):
        for signed in (True, False):
            codes = W.nibble_codes(n, signed, n)
            packed = W.pack_expected(codes)
            base = torch.zeros(n + 32, dtype=torch.int8, device=DEV)
            for off in (0, 1, 4, 15):
                base[off:off + n] = dev(codes)
                assert torch.equal(K.pack_int4(base[off:off + n]).cpu(), packed), (n, signed, off)
                big = torch.full((off + n + 64,), 0x5A, dtype=torch.uint8, device=DEV)
                got = K.unpack_int4(dev(packed), n, signed, out=big[off:])
                assert got.data_ptr() == big.data_ptr() + off
                exp = torch.full((off + n + 64,), 0x5A, dtype=torch.uint8)
                exp[off:off + n] = codes.view(torch.uint8)
                assert torch.equal(big.cpu(), exp), (n, signed, off)


# ------------------------------------------------------------------------------------------------ the dw+pw constant table
@pytest.mark.parametrize("c", W.TABLE_C)
def test_dwpw_table_records_are_exact(c):
    N, K = lib(), kernels()
    errs = []
    for vi, (with_bias, with_off, unsigned, zp) in enumerate(W.TABLE_VARIANTS):
        w, s_w, o_w, bias, s_in = W.table_operands(c, 10 * c + vi)
        bias, o_w = (bias if with_bias else None), (o_w if with_off else None)
        want = W.table_expected(w, bias, s_in, zp, s_w, o_w, unsigned)
        zpt = None if zp is None else torch.tensor([zp], dtype=torch.float32)
        ops = [dev(t) for t in (w.reshape(9, c).contiguous(), bias, s_in, zpt, s_w, o_w)]
        for fill in W.SENTINELS:
            buf, table = guarded(c * 32, fill)
            rc = N.lib.dlmcq_dwpw_pack_table(*map(N.ptr, ops), c, int(unsigned), N.ptr(table), N.stream_ptr())
            torch.cuda.synchronize()
            assert rc == 0, rc
            whole(buf, want, fill, 0, f"table C={c} variant {vi} (fill {fill:#x})", errs)
        got = K.dwpw_table(dev(w), dev(bias), dev(s_in), dev(zpt), dev(s_w), dev(o_w), x_unsigned=unsigned)
        if not torch.equal(got.cpu(), want):
            errs.append(f"table C={c} variant {vi}: the wrapper's table differs")
    settle(errs)


def test_dwpw_table_refusals_write_nothing():
    N = lib()
    fill = W.SENTINELS[0]
    w, s_w, o_w, bias, s_in = W.table_operands(128, 0)
    ops = [dev(t) for t in (w.reshape(9, 128).contiguous(), bias, s_in, None, s_w, o_w)]
    for what, c, offset, rc_want in W.TABLE_REFUSALS:
        buf, table = guarded(128 * 32, fill, offset=offset)
        rc = N.lib.dlmcq_dwpw_pack_table(*map(N.ptr, ops), c, 1, N.ptr(table), N.stream_ptr())
        torch.cuda.synchronize()
        assert rc == rc_want, (what, rc)
        assert bool((buf == fill).all()), (what, "the table was written")


# ------------------------------------------------------------------------------------------------ the grid caps
def on_device_equal(buf, want, fill, what):
    """fill | want | fill against the whole buffer, compared on the device (the grid-cap tensors are tens of megabytes)."""
    wb = dev(want.contiguous().view(-1).view(torch.uint8))
    n = wb.numel()
    assert bool((buf[n:] == fill).all()), what + ": bytes behind the output were written"
    if not torch.equal(buf[:n], wb):
        bad = (buf[:n] != wb).nonzero().flatten()
        raise AssertionError(f"{what}: {bad.numel()} bytes differ, first at {int(bad[0])}, last at {int(bad[-1])}")


def test_grid_cap_pack_and_unpack():
    t0 = time.time()
    N = lib()
    n = W.GRID_CAP["pack"]["n"]
    gg = torch.Generator().manual_seed(1)
    codes = (torch.randint(0, 16, (n,), generator=gg, dtype=torch.int16) - 8).to(torch.int8)
    packed = W.pack_expected(codes)
    fill = W.SENTINELS[0]
    cd = dev(codes)
    pbuf, p = guarded((n + 1) // 2, fill)
    assert N.lib.dlmcq_pack_int4(N.ptr(cd), N.ptr(p), n, N.stream_ptr()) == 0
    torch.cuda.synchronize()
    on_device_equal(pbuf, packed, fill, "pack at the grid cap")
    dirty = packed.clone()
    dirty[-1] |= 0xF0
    cbuf, c = guarded(n, fill)
    assert N.lib.dlmcq_unpack_int4(N.ptr(dev(dirty)), N.ptr(c), n, 1, N.stream_ptr()) == 0
    torch.cuda.synchronize()
    on_device_equal(cbuf, codes, fill, "unpack at the grid cap")
    print(f"\ngrid cap, pack + unpack (n = {n}): {time.time() - t0:.2f} s")


def test_grid_cap_image_pixel_route():
    t0 = time.time()
    g = W.GRID_CAP["image"]
    img = W.big_image(g["h"], g["w"])
    x = dev(img)
    assert W.image_route(1, g["w"], x.stride(), x.data_ptr() % 16) == "pixel"
    fill = W.SENTINELS[0]
    for q, code0 in ((X.Quant(1.0, 3.0), False), (X.Quant(1.0, None, 0, 255, X.FORM_ZEROPOINT, shift128=True), True)):
        want = W.image_expected(img, 0, q, code0)
        buf, _ = raw_image(x, 0, q, code0, fill)
        on_device_equal(buf, want, fill, f"image at the grid cap {q.tag()}")
    print(f"\ngrid cap, image pixel route ({g['h']} x {g['w']}): {time.time() - t0:.2f} s")


def test_grid_cap_pool():
    t0 = time.time()
    g = W.GRID_CAP["pool"]
    case = W.PoolCase("cap", g["n"], g["c"], g["h"], g["w"], g["k"], g["s"], g["p"])
    gg = torch.Generator().manual_seed(2)
    x = torch.randint(-128, 128, (g["n"], g["h"], g["w"], g["c"]), generator=gg, dtype=torch.int16).to(torch.int8)
    want = W.pool_expected(x, case)
    fill = W.SENTINELS[0]
    rc, ybuf = raw_pool(x, (g["n"], g["h"], g["w"], g["c"], g["k"], g["s"], g["p"]), False, 0, fill, want.numel())
    assert rc == 0, rc
    on_device_equal(ybuf, want, fill, "pool at the grid cap")
    print(f"\ngrid cap, pool ({g['h']} x {g['w']} x {g['c']}): {time.time() - t0:.2f} s")
