"""The pooled head kernel (csrc/conv_gap_i8.hip: conv_gap_i8_kernel<1> / <2>) and the pool kernel (csrc/gap.hip: gap_nhwc_kernel) against an
independent reference, whole `pooled` and `codes` tensors, NO tolerance, on the calls of tests/gap_head_cases.py: the image loop run two and
three times per workgroup, both sides of the slice-width rule, the LDS maximum behind a small launch and in front of one, every pixel count at
which a wave's rows change, full-range operands, five quantisers, special values through the shortcut.  Each case is first asked for its launch
record (dlmc._native.gap_launch_record: the launcher's own function, for this device's CU count) and the facts the case exists for are
asserted from it - the slice width; on the loop cases that every workgroup owns at least two images and not all the same number.

The reference is built in three steps (gap_head_cases.reference):
  1. the fp32 map before the pool - the float64 convolution of the dequantised operands + bias + shortcut, then the activation.  The kernel's
     chain, read from it: v = fma(float(acc + (shift - zp) SUM qw), s_in s_w[k], bias[k]) on the exact int32 sum; v = v + shortcut; relu_nan;
     cap6_nan.  Each is one rounding of an exact value, so v equals the float64 value bit for bit under the conditions asserted on the CPU
     before any launch (tests/exact_stages.py: pair_stages, assert_final_units): integer sums below 2^24, every scale a power of two, the bias
     a multiple of s_in s_w[k] and the fma's result below 2^24 units, the shortcut sum an fp32 number.
  2. the pool - csrc/gap.hip's three lines restated in numpy float32 (tests/test_gpu_gap.py: restate): s = v[0]; s = fl32(s + v[p]) in pixel
     order; pooled = fl32(s / fl32(H W)).  This step ROUNDS; it is a restatement of the kernel's definition, not an exact-value argument: a
     kernel that summed in another order, or multiplied by a reciprocal, fails it.
  3. the codes - the oracle's quantiser of the pooled reference, as bytes (expect_codes).
Every case is launched three times through the C ABI - fp32 + codes, codes alone, fp32 alone - into buffers filled with 0xA5 and longer than the
tensor: the three agree with the reference, nothing behind the tensor changes, and a buffer that was not asked for is not written.  On the loop
cases the older equality, fused head == conv2d_i8 then global_avgpool, is asserted as well: it ties the two paths together.

The pool kernel: H W in {2, 8, 9, 16, 17} (the remainders of its `unroll 8`), C = 4 with N = 300 (one thread per image, two workgroups) and
C = 12 (the image index changes inside a wave), against the same restatement, bitwise."""
import pytest
import torch

import exact_stages as S
import gap_head_cases as W
from test_gpu_epilogue_exact import DEV, expect_codes, same, settle

pytestmark = pytest.mark.gpu
TAIL = 256          # guard elements behind every output tensor


def _t(v):
    return torch.tensor([float(v)], dtype=torch.float32, device=DEV)


def _quant_args(q, codes):
    """The seven quantiser arguments of an entry point (codes buffer or None)."""
    from dlmc import _native as N
    if codes is None:
        return (None, None, None, 0, 0, 0, 0.0), ()
    keep = (_t(q.scale), None if q.zp is None else _t(q.zp))
    return (N.ptr(codes), N.ptr(keep[0]), N.ptr(keep[1]), q.lo, q.hi, q.form | (N.EMIT_SHIFT128 if q.shift128 else 0), q.g), keep


def _one_nan(t):
    """Every NaN as one bit pattern (where a NaN is, is compared; which NaN it is, is the hardware's business)."""
    return torch.where(t.isnan(), torch.full_like(t, float("nan")), t)


def _check_outputs(out, codes, numel, want, want_codes, want_out, want_q, what, errs):
    """The two sentinel-filled buffers after a call: the tensor against the reference where it was asked for, 0xA5 everywhere else."""
    out, codes = out.cpu(), codes.cpu()
    assert bool((out[numel:].view(torch.uint8) == 0xA5).all()), what + ": fp32 values written behind the tensor"
    assert bool((codes[numel:] == 0xA5).all()), what + ": code bytes written behind the tensor"
    if want_out:
        same(_one_nan(out[:numel].reshape(want.shape)), _one_nan(want), what + " pooled", errs)
    else:
        assert bool((out.view(torch.uint8) == 0xA5).all()), what + ": a call without an fp32 output wrote fp32 values"
    if want_q:
        same(codes[:numel].view(want_codes.dtype).reshape(want_codes.shape), want_codes, what + " codes", errs)
    else:
        assert bool((codes == 0xA5).all()), what + ": a call without a quantiser wrote codes"


def run_case(case, errs):
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    n, rec, ref = W.prepare(case, N.gap_launch_record)            # the record's facts and the exactness conditions: asserted here, on the CPU
    lay, q, want = ref["lay"], ref["quant"], ref["pooled"]
    want_codes = expect_codes(K, want, q)
    k, numel = case.k, n * case.k
    x = S.nhwc(lay.codes).to(DEV)
    w = S.nhwc(lay.wq).reshape(k, case.c).contiguous().to(DEV)
    wsum = lay.wq.to(torch.int32).sum(dim=(1, 2, 3)).to(torch.int32).to(DEV)
    bias = ref["bias"].to(DEV) if case.bias else None
    s_in, zp, s_w = _t(lay.s_in), _t(lay.zp), lay.s_w.to(DEV)
    res = S.nhwc(ref["res"]).to(DEV) if case.res else None
    what = f"{case.cid} N{n} C{case.c} K{k} {case.h}x{case.w} record={rec} {'u8' if case.uns else 'i8'} zp={lay.zp} act={case.act} {q.tag()}"
    for want_out, want_q in ((True, True), (False, True), (True, False)):
        out, codes = S.sentinel(numel + TAIL, torch.float32), S.sentinel(numel + TAIL, torch.uint8)
        qa, keep = _quant_args(q, codes if want_q else None)
        rc = N.lib.dlmcq_conv2d_i8_nhwc_gap(N.ptr(x), N.ptr(w), N.ptr(out) if want_out else None, N.ptr(bias), N.ptr(wsum), N.ptr(s_in), N.ptr(zp),
                                            N.ptr(s_w), n, case.h, case.w, case.c, k, int(case.uns), N.ptr(res), case.act, *qa, N.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, (what, rc)
        _check_outputs(out, codes, numel, want, want_codes, want_out, want_q, f"{what} [fp32={want_out} codes={want_q}]", errs)
    if case.loops:          # the two paths tied together: the same head as the tiled kernel's fp32 map pushed through the pool kernel
        cl = lambda t: t.to(DEV).contiguous(memory_format=torch.channels_last)      # noqa: E731
        wq4 = w.reshape(k, 1, 1, case.c)
        em = K.EmitCodes(_t(q.scale), None if q.zp is None else _t(q.zp), q.lo, q.hi, q.form, q.g, q.shift128)
        r4 = cl(ref["res"]) if case.res else None
        full = K.conv2d_i8(cl(lay.codes), wq4, wsum, bias, s_in, zp, s_w, residual=r4, act=case.act)
        two, two_codes = K.global_avgpool(full, emit=em)
        one, one_codes = K.conv2d_i8_gap(cl(lay.codes), wq4, wsum, bias, s_in, zp, s_w, residual=r4, act=case.act, emit=em)
        same(one, two.cpu(), what + ": fused head against conv2d_i8 then global_avgpool, pooled", errs)
        same(one_codes, two_codes.cpu(), what + ": fused head against conv2d_i8 then global_avgpool, codes", errs)
        same(one, want, what + ": the wrapper's pooled", errs)


@pytest.mark.parametrize("cid", [c.cid for c in W.CASES])
def test_head_is_exact_on_full_range_operands(cid):
    errs = []
    run_case(W.BY_ID[cid], errs)
    settle(errs)


def test_lds_attribute_small_large_small():
    """The kernel's dynamic-LDS allowance is raised by the first launch that needs more (150 272 bytes at C = 2048) and kept: a small launch,
    the largest, and the small one again, in this order in one process, each exact."""
    errs = []
    for cid in W.LDS_ORDER:
        run_case(W.BY_ID[cid], errs)
    settle(errs)


@pytest.mark.parametrize("shape", W.POOL_SHAPES, ids=lambda s: "N%d_C%d_HW%d" % s)
def test_pool_kernel_unroll_remainders_and_image_seams(shape):
    from dlmc import _native as N
    from dlmc.quantization.scalar import kernels as K
    n, c, hw = shape
    rows, want, q = W.pool_reference(n, c, hw)
    want_codes = expect_codes(K, want, q)
    x = rows.to(DEV)
    errs = []
    for want_out, want_q in ((True, True), (False, True), (True, False)):
        out, codes = S.sentinel(n * c + TAIL, torch.float32), S.sentinel(n * c + TAIL, torch.uint8)
        qa, keep = _quant_args(q, codes if want_q else None)
        rc = N.lib.dlmcq_gap_nhwc_f32(N.ptr(x), N.ptr(out) if want_out else None, qa[0], n, hw, c, *qa[1:], N.stream_ptr())
        torch.cuda.synchronize()
        assert rc == 0, (shape, rc)
        _check_outputs(out, codes, n * c, want, want_codes, want_out, want_q, f"pool N{n} C{c} HW{hw} [fp32={want_out} codes={want_q}]", errs)
    settle(errs)
