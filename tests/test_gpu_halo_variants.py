"""Every instantiation of the two 3x3 kernels - conv3x3_halo_i8_kernel (csrc/conv3x3_i8.hip: the 40 records of DLMCQ_HALO_TABLE) and
conv3x3_pipe_i8_kernel (csrc/conv3x3_pipe_i8.hip: the 6 of DLMCQ_PIPE_TABLE) - against an independent float64 reference, whole tensor, NO
tolerance, on full-range operands (tests/exact_layers.py: make_full_range_layer): codes over all 256 byte values, weight codes in +-127,
per-channel dyadic weight scales that differ from channel to channel, a dyadic input scale != 1, uint8 zero points on either side of 128,
int8 zero points that are not 0, biases that are multiples of each channel's s_in * s_w[k] (or a null bias).  The calls are
tests/halo_variant_cases.py's; each is first asked with DLMCQ_ROUTE_ONLY | DLMCQ_ROUTE_HALO_VARIANT, for the very arguments about to be
launched, which record it runs, and is launched once.

Reference: float64 convolution of the DEQUANTISED operands (zero padding) + bias, ReLU, exact_f32, then the oracle's quantiser
(expect_codes).  The kernels' fp32 value before the quantiser equals it bit for bit under the staged conditions of tests/exact_stages.py
(`pair_stages`, `assert_final_units`), asserted on the CPU before any launch; the 3x3 kernels write codes only, so the comparison is the
code bytes of the whole tensor.  The code buffer is sentinel-filled and one tile longer than M * K: nothing beyond M * K may be written; no
fp32 buffer is passed.

The pipelined kernel's tensors are two to three tiles per compute unit - too many pixels for a float64 reference of all of them.  Its
WHOLE-TENSOR anchor is the plain halo kernel on the same full-range operands, byte for byte - the 128-wide, 24-piece, two-buffer PLAIN
record, which this file anchors exactly - and the exact reference is compared on the first image, the last image and every eighth image
(the staged conditions are asserted on those images).

Conditions that keep a case from proving nothing, computed from the reference alone before the launch, on the live channels:
  * at least 10 % of the reference codes lie strictly between the quantiser's bounds (the threshold of the ReLU6 check in
    tests/test_gpu_tiled_variants.py); under ReLU the lower bound is the code of 0 where that lies above the range's lower end;
  * the lower clamp occurs in every ReLU case;
  * at least one case per record has reference codes at the upper bound (the `_hi` quantisers: consumer scale 2^-5 of
    exact_layers.TIE_SCALES); which cases carry it is printed."""
import dataclasses
import functools

import pytest
import torch

import exact_layers as X
import exact_stages as S
import halo_variant_cases as H
import test_conv_dispatch_host as D
from test_gpu_epilogue_exact import DEV, expect_codes, same, settle

pytestmark = pytest.mark.gpu

QUANTS = {"plain": X.Quant(0.25), "plain_hi": X.Quant(2.0 ** -5), "shift": X.Quant(0.25, shift128=True), "shift_hi": X.Quant(2.0 ** -5, shift128=True),
          "uzp": X.Quant(0.25, 16.0, 0, 255), "uzp_hi": X.Quant(2.0 ** -5, 16.0, 0, 255),
          "signed": X.Quant(0.5, 3.0, -128, 127), "signed_hi": X.Quant(2.0 ** -5, -100.0, -128, 127)}
assert all(q.scale in X.TIE_SCALES for q in QUANTS.values())


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _operands(case, g):
    """The layer of a case (operands depend on `case.key` alone: a tuple's PLAIN and other records share them)."""
    gen = torch.Generator().manual_seed(8800 + 1000 * case.key[0] + 10 * case.key[2] + int(case.key[1]))
    signed = not g["uns"]
    lay = X.make_full_range_layer(gen, g["N"], g["C"], g["H"], g["W"], g["K"], 3, signed_in=signed, zp=case.zp if signed else None,
                                  zp_side=None if signed else case.zp)
    if not case.bias:
        lay.bias = torch.zeros(g["K"])
    return lay


def _exact(lay, g):
    """The exact pre-activation reference of a layer, its staged conditions asserted."""
    true, _, _ = S.pair_stages(lay, g, 128 if g["uns"] else 0)
    S.assert_final_units(true, lay)
    return true


@functools.lru_cache(maxsize=None)
def reference(key):
    case = next(c for c in H.CASES if c.key == key)
    g = case.geo_for()
    lay = _operands(case, g)
    return lay, _exact(lay, g)


def clamp_facts(want, q, relu, lay):
    """(share of the live channels' reference codes strictly inside the bounds, the lower clamp occurs, the upper clamp occurs)."""
    c = X.oracle_codes(want, q)[:, lay.nz:lay.live]
    lo = float(q.lo)
    if relu:
        lo = max(lo, float(X.oracle_codes(torch.zeros(1), q)))
    return float(((c > lo) & (c < q.hi)).float().mean()), bool((c == lo).any()), bool((c == q.hi).any())


def _device_operands(case, lay, quant):
    t = dict(x=S.nhwc(lay.codes).to(DEV), w=S.nhwc(lay.wq).to(DEV), wsum=lay.wq.to(torch.int32).sum(dim=(1, 2, 3)).to(torch.int32).to(DEV),
             s_in=torch.tensor([lay.s_in], dtype=torch.float32, device=DEV), zp_in=torch.tensor([float(lay.zp)], dtype=torch.float32, device=DEV),
             s_w=lay.s_w.to(DEV), q_scale=torch.tensor([quant.scale], dtype=torch.float32, device=DEV))
    if case.bias:
        t["bias"] = lay.bias.to(DEV)
    if quant.zp is not None:
        t["q_zp"] = torch.tensor([quant.zp], dtype=torch.float32, device=DEV)
    return t


def _launch(case, t, m, k, record, cus, what, pipelined=None):
    """Ask the route for these very arguments, launch once into a fresh sentinel buffer one tile longer than M * K; the bytes of M * K."""
    from dlmc import _native as N
    t["codes"] = S.sentinel((m + H.TM) * k, torch.uint8)
    args = case.route_args(ptr=lambda name: t[name].data_ptr(), cus=cus, pipelined=pipelined)
    assert H.decode(D.call(N.lib, "fused", args)) == record, what
    torch.cuda.synchronize()
    rc = H.launch(N.lib, "fused", dict(args, ctl=args["ctl"] & ~H.ROUTE_HALO_VARIANT, stream=torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)
    codes = t["codes"].cpu()
    assert bool((codes[m * k:] == 0xA5).all()), what + ": code bytes written beyond row M"
    return codes[:m * k]


def run_halo_case(case, errs):
    from dlmc.quantization.scalar import kernels as K
    lay, base = reference(case.key)
    g = case.geo_for()
    quant = QUANTS[case.quant]
    want = X.exact_f32(X.activation(base, case.relu), "activation")
    inside, lower, upper = clamp_facts(want, quant, case.relu, lay)
    what = f"{case.cid} {g['N']}x{g['H']}x{g['W']} C{g['C']} K{g['K']} relu={case.relu} bias={case.bias} zp={lay.zp} {quant.tag()}"
    assert inside >= 0.10 and (lower or not case.relu), (what, inside, lower)
    n, k, p, q_ = want.shape
    m = n * p * q_
    t = _device_operands(case, lay, quant)
    codes = _launch(case, t, m, k, case.record, 256, what)
    want_codes = S.nhwc(expect_codes(K, want, quant))
    same(codes.view(want_codes.dtype).reshape(n, p, q_, k), want_codes, what + " codes", errs)
    return upper


def run_pipe_case(case, errs):
    from dlmc.quantization.scalar import kernels as K
    cus = _cus()
    g = case.geo_for(cus)
    quant = QUANTS[case.quant]
    lay = _operands(case, g)
    n, k, p, q_ = g["N"], g["K"], g["H"], g["W"]
    m = n * p * q_
    tiles = -(-case.frame(cus)[0] // H.TM) * (k // 128)
    grid = min(cus & ~7, tiles & ~7)
    what = f"{case.cid} {n}x{p}x{q_} C{g['C']} K{k} relu={case.relu} bias={case.bias} zp={lay.zp} {quant.tag()} tiles={tiles} grid={grid}"
    assert 2 * cus < tiles < 3 * cus and tiles % grid, what       # workgroups own unequal numbers of tiles
    idx = sorted(set(range(0, n, 8)) | {n - 1})                    # the first image, every eighth, the last
    sub = dataclasses.replace(lay, codes=lay.codes[idx])
    want = X.exact_f32(X.activation(_exact(sub, g), case.relu), "activation")
    inside, lower, upper = clamp_facts(want, quant, case.relu, sub)
    assert inside >= 0.10 and (lower or not case.relu), (what, inside, lower)
    t = _device_operands(case, lay, quant)
    got = _launch(case, t, m, k, case.record, cus, what)
    halo = _launch(case, t, m, k, ("halo", 128, False, 24, 2, case.record[2], True), cus, what + " (plain halo kernel)", pipelined=False)
    assert torch.equal(got, halo), f"{what}: {int((got != halo).sum())} of {got.numel()} codes differ from the plain halo kernel"
    want_codes = S.nhwc(expect_codes(K, want, quant))
    same(got.view(want_codes.dtype).reshape(n, p, q_, k)[idx], want_codes, what + " codes of the sampled images", errs)
    return upper


@pytest.mark.parametrize("record", H.RECORDS, ids=H.record_name)
def test_3x3_variant_is_exact_on_full_range_operands(record):
    cases = H.BY_RECORD[record]
    assert len(cases) >= 2
    errs, carriers = [], []
    for case in cases:
        if (run_pipe_case if case.pipelined else run_halo_case)(case, errs):
            carriers.append(case.cid)
    settle(errs)
    print(f"upper clamp of {H.record_name(record)}: {carriers}")
    assert carriers, "no case of this record has reference codes at the upper bound"
