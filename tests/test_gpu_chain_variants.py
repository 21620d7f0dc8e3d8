"""Every instantiation of conv_chain_i8_kernel (csrc/conv_chain_i8.hip: the 23 kernels of CHAIN_TABLE, through dlmcq_conv2d_i8_nhwc_chain,
_dual_chain and _recompute_chain) against an independent float64 reference, whole tensors, NO tolerance, on full-range operands
(tests/exact_layers.py: make_full_range_layer with a 1x1 filter for the block end and its extra operands, make_full_range_second for the
reduction behind the first quantiser): codes over all 256 byte values, weight codes in +-127, per-channel dyadic weight scales that differ
from channel to channel, dyadic input scales != 1, biases that are multiples of each channel's unit and carry tie fractions, an fp32
shortcut with the edge values per pixel (the plain form) or edge biases (the other two).  The calls are tests/chain_variant_cases.py's;
each is first asked with DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_CHAIN_VARIANT, for the very arguments and pointers about to be launched, which
instantiation, tile height and layouts it runs, and is launched once.

Reference (tests/test_chain_variants_host.py: `reference`, computed and its conditions asserted on the CPU - that file proves them for every
call without a GPU): the float64 convolution of the dequantised operands (+ shortcut; the recomputing form's shortcut relu?(conv(a) +
conv(b sampled)) rounded to fp32 as the dual form stores it), exact_f32, the activation, the oracle's codes for the first quantiser, the
second layer on THOSE reference codes, its activation, the oracle's codes for the second quantiser.  The kernel's values equal it bit for
bit under the staged conditions of tests/exact_stages.py (`chain_stages`) and exact_layers.second_gemm_full_ref.

The fp32 output, the first codes and the second codes are sentinel-filled buffers one 64-row tile longer than needed: nothing beyond row M
may be written (chunk-major tensors: nothing beyond the last plane); a buffer the call does not ask for is allocated all the same, passed as
null, and must stay untouched.  Chunk-major fp32 tensors [K / 64][M][64] are reindexed to rows here."""
import functools

import pytest
import torch

import chain_variant_cases as V
import exact_stages as S
import test_chain_refusals_host as R
from test_chain_variants_host import reference
from test_gpu_epilogue_exact import DEV, expect_codes, same, settle

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _room():
    """2 GiB + 16 MiB of device memory, never filled: it holds 16-byte-aligned addresses whose low 32 bits have bit 31 set."""
    return torch.empty((1 << 31) + (1 << 24), dtype=torch.uint8, device=DEV)


class _High:
    """Places tensors inside `_room` at addresses with bit 31 of the low half set, 1 MiB apart."""

    def __init__(self):
        room = _room()
        base = room.data_ptr()
        self.room, self.off = room, next(o for o in range(0, 1 << 31, 1 << 20) if ((base + o) & 0xffffffff) >> 31)

    def place(self, t):
        nbytes = t.numel() * t.element_size()
        assert nbytes <= (1 << 20) and self.off + (1 << 20) <= self.room.numel()
        view = self.room[self.off:self.off + nbytes].view(t.dtype).view(t.shape)
        view.copy_(t)
        assert (view.data_ptr() & 0xffffffff) >> 31 == 1 and ((view.data_ptr() + nbytes) & 0xffffffff) >> 31 == 1
        self.off += 1 << 20
        return view


def _chunk_major(rows):
    """fp32 rows [M][K] -> the chunk-major tensor [K / 64][M][64] (DLMCQ_FP32_*_CHUNK_MAJOR)."""
    m, k = rows.shape
    return rows.reshape(m, k // 64, 64).permute(1, 0, 2).contiguous()


def _rows(flat, m, k, cm):
    """The first M * K values of a buffer as rows [M][K], from either layout."""
    t = flat[:m * k]
    return t.reshape(k // 64, m, 64).permute(1, 0, 2).reshape(m, k).contiguous() if cm else t.reshape(m, k)


def run_case(case, errs):
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    r = reference(case.cid)
    c1, kb, c2, ca, cb, _ = case.row
    n, h, w = case.geo
    m, kd = case.m, case.kd
    q1, q2, sec = r["q1"], r["q2"], r["second"]
    icm, ocm = case.layouts()
    hi = _High() if case.high else None
    t = {}                                       # name -> device tensor (kept alive until the launch is done)

    def put(name, tensor):
        tensor = tensor.contiguous()
        t[name] = hi.place(tensor.to(DEV)) if name in case.high else tensor.to(DEV)

    def f1(v):
        return torch.tensor([float(v)], dtype=torch.float32)
    for sfx, key in (("", "own"), ("b", "sampled"), ("a", "unit")):
        if key in r:
            lay = r[key]
            put("x" + sfx, S.nhwc(lay.codes))
            put("w" + sfx, S.nhwc(lay.wq))
            put("wsum" + sfx, lay.wq.to(torch.int32).sum(dim=(1, 2, 3)).to(torch.int32))
            put("bias" + sfx, lay.bias)
            put("s_in" + sfx, f1(lay.s_in))
            put("zp_in" + sfx, f1(lay.zp))
            put("s_w" + sfx, lay.s_w)
    if "res" in r:
        rows = S.nhwc(r["res"]).reshape(m, kd)
        put("res", _chunk_major(rows) if icm else rows)
    w2 = S.nhwc(sec.wq)                          # [K2][1][1][KD]
    put("w2", K.chunk_major(w2) if case.w3cm else w2)
    put("wsum2", sec.wq.to(torch.int32).sum(dim=(1, 2, 3)).to(torch.int32))
    put("bias2", sec.bias)
    put("s_w2", sec.s_w)
    put("q_scale", f1(q1.scale))
    put("q_zp", f1(q1.zp or 0.0))
    put("q2_scale", f1(q2.scale))
    put("q2_zp", f1(q2.zp or 0.0))
    extra = 64                                   # one 64-row tile more than the call needs
    out = S.sentinel((m + extra) * kd, torch.float32)
    if "out" in case.high:
        out = hi.place(out)
    t["out"], t["codes"], t["codes2"] = out, S.sentinel((m + extra) * kd, torch.uint8), S.sentinel((m + extra) * kb, torch.uint8)
    ptr = lambda name: t[name].data_ptr()
    what = (f"{case.cid} {case.entry} M={m} KD={kd} rpt={case.rpt} w3cm={case.w3cm} layouts={(icm, ocm)} out={case.out} codes={case.codes} "
            f"relu={case.relu}/{case.relu2} {q1.tag()} -> {q2.tag()} stride={case.stride} null_bias={case.null_bias}")
    # ---- which instantiation, tile height and layouts: asked for these very arguments
    assert V.decode(R.call(N.lib, case.entry, case.route_args(ptr))) == case.expected(), what
    torch.cuda.synchronize()
    rc = R.call(N.lib, case.entry, dict(case.call_args(ptr), stream=torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)
    got_out, got_c1, got_c2 = t["out"].cpu(), t["codes"].cpu(), t["codes2"].cpu()
    # ---- nothing beyond row M (beyond the last plane), nothing into a buffer that was not asked for
    assert bool((got_c2[m * kb:] == 0xA5).all()), what + ": second codes written beyond row M"
    if case.out:
        assert bool((got_out[m * kd:].view(torch.uint8) == 0xA5).all()), what + ": fp32 values written beyond the rows"
        same(_rows(got_out, m, kd, ocm).reshape(n, h, w, kd), S.nhwc(r["mid"]), what + " fp32", errs)
    else:
        assert bool((got_out.view(torch.uint8) == 0xA5).all()), what + ": a call without an fp32 output wrote fp32 values"
    if case.codes:
        assert bool((got_c1[m * kd:] == 0xA5).all()), what + ": first codes written beyond row M"
        same(got_c1[:m * kd].reshape(n, h, w, kd), S.nhwc(expect_codes(K, r["mid"], q1)), what + " first codes", errs)
    else:
        assert bool((got_c1 == 0xA5).all()), what + ": a call without first codes wrote some"
    want2 = S.nhwc(expect_codes(K, r["v2"], q2))
    assert torch.equal(want2, S.nhwc(r["c2"]))
    same(got_c2[:m * kb].view(want2.dtype).reshape(n, h, w, kb), want2, what + " second codes", errs)
    return r["facts"]


@pytest.mark.parametrize("record", V.RECORDS, ids=V.record_name)
def test_chain_variant_is_exact_on_full_range_operands(record):
    cases = V.BY_RECORD[record]
    assert len(cases) >= 3
    errs, facts = [], []
    for case in cases:
        facts.append(run_case(case, errs))
    settle(errs)
    print(f"{V.record_name(record)}: (inside, lower, upper) of the first / second quantiser per call: {facts}")
    assert any(f[0][2] for f in facts) and any(f[1][2] for f in facts), "no call of this instantiation has reference codes at an upper bound"
