"""The pooled head's launch record and the cases of tests/gap_head_cases.py, on the host (no GPU): what dlmcq_x_gap_launch_record answers
for every case (the facts each case exists for, asserted from the record), the record against the launcher's rule restated in Python - the LDS
formula at C = 320 / 384 / 2048, ngroups never above N -, every case's exactness conditions and quantiser facts proven on the CPU (the
reference of tests/test_gpu_gap_head_exact.py is built here, conditions asserted inside), and the refusals that already hold."""
import ctypes
import os
import re

import pytest
import torch

import exact_layers as X
import gap_head_cases as W
from dlmc import _native as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(4096)


def cus():
    """The CU count the launcher uses in this process (256 without a device): read back from the record of a one-slice problem."""
    return N.gap_launch_record(1 << 30, 64, 64)[2] // 2


def test_the_query_is_exported_and_not_in_the_header():
    assert hasattr(ctypes.CDLL(N.LIB_PATH), "dlmcq_x_gap_launch_record")
    assert "dlmcq_x_gap_launch_record" not in open(os.path.join(ROOT, "include", "dlmcq.h")).read()
    assert N.gap_launch_record(512, 512, 2048) == W.launch_restated(512, 512, 2048, cus())
    if cus() == 256:
        assert N.gap_launch_record(512, 512, 2048) == (64, 32, 16, 51968) and N.gap_launch_record(69, 64, 2048) == (128, 16, 32, 45568)
    fn = N.experimental("dlmcq_x_gap_launch_record", [ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)])
    answer = (ctypes.c_int64 * 4)(-7, -7, -7, -7)
    for n, c, k in ((0, 64, 64), (-1, 64, 64), (2, 96, 64), (2, 0, 64), (2, 2112, 64), (2, 64, 96), (2, 64, 0), (2, 64, 1 << 24)):
        assert fn(n, c, k, answer) == -1 and list(answer) == [-7] * 4, (n, c, k)       # what the entry point refuses, refused and nothing written
    assert fn(2, 64, 64, None) == -1


@pytest.mark.parametrize("cid", sorted(W.BY_ID))
def test_the_record_of_every_case_and_its_facts(cid):
    case = W.BY_ID[cid]
    n = case.n_for(N.gap_launch_record)
    rec = W.launch_facts(case, n, N.gap_launch_record)
    assert rec == W.launch_restated(n, case.c, case.k, cus()), (cid, rec)
    assert n >= 2
    if case.loops:
        assert n == 2 * rec[2] + rec[2] // 2 and 0 < n - 2 * rec[2] < rec[2]
    if cus() == 256:                                   # the record at the CU count of a process without a device, written out
        want = {"loop128": (80, (128, 16, 32, 45568)), "loop64": (42, (64, 31, 17, 23296)), "edge320": (3, (128, 2, 3, 78336)),
                "edge384": (3, (64, 4, 3, 43776)), "k192": (4, (64, 3, 4, 23296)), "lds64": (10, (64, 1, 10, 23296)),
                "lds2048": (10, (64, 1, 10, 150272)), "hw1": (48, (128, 1, 48, 45568)), "hw32": (6, (128, 1, 6, 53760))}
        if cid in want:
            assert (n, rec) == want[cid]


def test_the_lds_formula_and_the_slice_width_edge():
    """gap_lds_bytes restated: BN (C + 16) weight bytes + 12 BN constants + 64 rows of (BN + 4) floats.  128-wide slices while the 128-wide
    form stays within 78 KiB - up to C = 320 - and K % 128 == 0; C = 2048 is the largest the entry point takes and fits the CU's 160 KiB."""
    assert W.lds_bytes(320, 128) == 78336 <= 78 * 1024 < W.lds_bytes(384, 128) == 86528
    assert W.lds_bytes(384, 64) == 43776 and W.lds_bytes(2048, 64) == 150272 <= 160 * 1024
    for c in range(64, 2048 + 1, 64):
        for k in (64, 128, 192, 256, 1984, 2048):
            width, nslice, ngroups, lds = N.gap_launch_record(1000, c, k)
            assert width == (128 if c <= 320 and k % 128 == 0 else 64) and nslice == k // width and lds == W.lds_bytes(c, width), (c, k)
            assert lds <= 160 * 1024
    assert N.gap_launch_record(2, 320, 256)[0] == 128 and N.gap_launch_record(2, 384, 256)[0] == 64 and N.gap_launch_record(2, 64, 192)[0] == 64


def test_ngroups_never_exceeds_the_batch():
    for c, k in ((64, 64), (64, 2048), (64, 1984), (2048, 64), (320, 1280)):
        top = N.gap_launch_record(1 << 30, c, k)[2]
        assert top == -(-2 * cus() // N.gap_launch_record(1 << 30, c, k)[1])
        for n in list(range(1, 70)) + [top - 1, top, top + 1, 2 * top + 1, 1 << 20]:
            if n >= 1:
                assert N.gap_launch_record(n, c, k)[2] == min(n, top), (c, k, n)


@pytest.mark.parametrize("cid", sorted(W.BY_ID))
def test_every_case_meets_the_exactness_conditions_on_the_cpu(cid):
    """`reference` asserts the staged conditions and the quantiser's facts; here also what the special cases promise."""
    case = W.BY_ID[cid]
    n, rec, ref = W.prepare(case, N.gap_launch_record)
    lay, pooled, q = ref["lay"], ref["pooled"], ref["quant"]
    assert tuple(pooled.shape) == (n, case.k) and pooled.dtype == torch.float32
    assert lay.s_in != 1.0 and len(set(lay.s_w.tolist())) == 5 and int(lay.wq.min()) == -127 and int(lay.wq.max()) == 127
    assert len(lay.codes.view(torch.uint8).unique()) == 256
    assert (lay.zp != 128 and 0 < lay.zp < 255) if case.uns else lay.zp != 0
    assert len({lay.codes[i].view(torch.uint8).sum().item() for i in range(n)}) > n // 2         # the images differ
    lo, hi, distinct = W.quant_facts(pooled, q)
    print(cid, "N", n, "record", rec, q.tag(), "g", q.g, "ends", lo, hi, "distinct codes", distinct)
    codes = X.quantise(pooled, q)
    assert codes.dtype == (torch.int8 if q.shift128 or q.lo < 0 else torch.uint8)
    finite = pooled.isfinite()
    if case.res:                                       # no edge values in the bias: what is not finite comes from the shortcut alone
        want = torch.zeros_like(finite)
        if case.special:
            for name in ("nan", "inf"):
                i, ch, _ = W.SPECIAL[name]
                want[i, ch] = True
            assert pooled[W.SPECIAL["nan"][:2]].isnan() and pooled[W.SPECIAL["inf"][:2]] == float("inf")
            assert bool((ref["res"][W.SPECIAL["negzero_image"]].view(torch.int32) == -2 ** 31).all())
        assert torch.equal(~finite, want), cid
    if case.zero_image:                                # the image of zero-point codes: its convolution is 0, its output the bias itself
        z = ref["zero_at"]
        assert z == 1 + rec[2] and z + rec[2] < n and bool((lay.codes[z] == case.zp).all())
        assert case.act == 0 and not case.res
        live = slice(W.NZ, None)
        assert torch.equal(pooled[z, live], lay.bias[live]) and float(lay.bias[live].abs().max()) > 0
        assert not torch.equal(pooled[z - rec[2], live], lay.bias[live]) and not torch.equal(pooled[z + rec[2], live], lay.bias[live])


def test_the_pool_kernels_cases():
    assert {hw % 8 for _, _, hw in W.POOL_SHAPES} >= {0, 1, 2} and {(hw - 1) % 8 for _, c, hw in W.POOL_SHAPES if c == 4} == {0, 1, 7}
    for n, c, hw in W.POOL_SHAPES:
        rows, pooled, q = W.pool_reference(n, c, hw)
        assert n * (c // 4) > 256 and tuple(pooled.shape) == (n, c)
        lo, hi, distinct = W.quant_facts(pooled, q)
        assert lo and hi and distinct > 100, (n, c, hw, lo, hi, distinct)


def test_the_refusals_that_already_hold():
    f = N.lib.dlmcq_conv2d_i8_nhwc_gap

    def call(n=2, h=7, w=7, c=64, k=64, form=N.ROUTE_ONLY):
        return f(P, P, P, None, P, P, None, P, n, h, w, c, k, 1, None, 0, None, None, None, 0, 0, form, 0.0, None)
    assert call() == N.ROUTE_GAP
    assert call(h=9, w=9) == -1 and call(k=96) == -1 and call(c=2112) == -1               # H W = 81, K = 96, C = 2112
    for bit in (N.FORCE_TILED, N.PIPELINED, N.FP32_IN_CHUNK_MAJOR, N.FP32_OUT_CHUNK_MAJOR, N.W2_CHUNK_MAJOR, N.PAD_CODE0, N.ROUTE_VARIANT,
                N.ROUTE_HALO_VARIANT, N.ROUTE_DW_VARIANT, N.ROUTE_CHAIN_VARIANT, N.ROUTE_PW_VARIANT, N.ROUTE_HALO_ROWS):
        assert call(form=N.ROUTE_ONLY | bit) == -1, hex(bit)
    for case in W.CASES:                               # every case is a call the entry point takes: DLMCQ_ROUTE_GAP, nothing launched
        assert call(n=case.n_for(N.gap_launch_record), h=case.h, w=case.w, c=case.c, k=case.k) == N.ROUTE_GAP, case.cid


def test_the_case_table_names_what_the_issue_lists():
    src = open(os.path.join(ROOT, "tests", "gap_head_cases.py")).read()
    assert len(W.CASES) == 14 and len(re.findall(r"^    Case\(", src, flags=re.M)) == 14
    assert [W.BY_ID[c].c for c in W.LDS_ORDER] == [64, 2048, 64]
    assert sum(c.loops for c in W.CASES) == 2 and {c.width for c in W.CASES if c.loops} == {64, 128}
    assert any(c.loops and (c.k // 64) % 2 == 1 for c in W.CASES) and sum(c.zero_image for c in W.CASES) == 1
