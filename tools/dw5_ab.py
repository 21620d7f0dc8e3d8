#!/usr/bin/env python3
"""The 5x5 depthwise kernel (csrc/conv_dw5_i8.hip) against the route such a layer takes without it (dlmcq_conv2d_dw_i8_nhwc: the generic
kernel), two interleaved comparisons in one process:
  (a) stand-alone: K.conv2d_dw5_i8 and K.conv2d_dw_i8 on the same operands, at the five distinct 5x5 layers of EfficientNet-B0 at 224^2 by
      padded channel width, input map and stride - 192 / 56^2 / 2, 256 / 28^2 / 1, 512 / 14^2 / 1, 704 / 14^2 / 1 and / 2, 1152 / 7^2 / 1 -
      codes only with symmetric and with asymmetric weights (the plain quantiser: FAST 2 / FAST 1), and one case with the fp32 output
      (FAST 0); per case the median of `rounds` interleaved timings of 20 launches each, max - min as the run-to-run spread, whether the
      results are equal, and whether the new kernel is faster by more than the larger spread;
  (b) whole plan: workloads.efficientnet_b0() FSPTQ and QBase W8A8, gates=True and swish=True in both, dw5 off against on, ms per step.
Writes profiles/dw5_ab.json (or --out) and prints it.
usage: python tools/dw5_ab.py [--batch N] [--plan-batch N] [--rounds N] [--out FILE]"""
import argparse

import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import fuse_inference

SHAPES = [(192, 56, 2), (256, 28, 1), (512, 14, 1), (704, 14, 1), (704, 14, 2), (1152, 7, 1)]      # padded channels, input map, stride
VARIANTS = [("codes_sym", False, False), ("codes_asym", True, False), ("fp32_and_codes_sym", False, True)]
DEV = P.DEV


def operands(batch, c, hw, gen):
    x = torch.randint(0, 256, (batch, hw, hw, c), generator=gen, dtype=torch.uint8).to(DEV).permute(0, 3, 1, 2)      # NHWC memory
    wq = torch.randint(-127, 128, (5, 5, c), generator=gen, dtype=torch.int8).to(DEV)
    s_w = (torch.rand(c, generator=gen) * 0.01 + 0.001).to(DEV)
    w_off = ((torch.rand(c, generator=gen) - 0.5) * 0.01).to(DEV)
    bias = torch.randn(c, generator=gen).to(DEV)
    one = lambda v: torch.tensor([v], dtype=torch.float32, device=DEV)      # noqa: E731
    return x, wq, bias, one(0.05), one(0.0), s_w, w_off, K.EmitCodes(one(0.5), None, 0, 255, N.FORM_ZEROPOINT)


def stats(v):
    return {"ms_median": round(sorted(v)[len(v) // 2], 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}


def standalone(batch, rounds):
    rows = []
    gen = torch.Generator().manual_seed(2333)
    for c, hw, stride in SHAPES:
        x, wq, bias, s_in, zp, s_w, w_off, emit = operands(batch, c, hw, gen)
        for tag, asym, want_out in VARIANTS:
            if want_out and (c, hw, stride) != (704, 14, 1):
                continue
            kw = dict(w_offset=w_off if asym else None, stride=stride, relu=True, emit=emit, want_out=want_out)
            runs = {"dw5": lambda _: K.conv2d_dw5_i8(x, wq, bias, s_in, zp, s_w, **kw),
                    "generic": lambda _: K.conv2d_dw_i8(x, wq, bias, s_in, zp, s_w, padding=2, **kw)}
            res = {k: f(None) for k, f in runs.items()}
            equal = all(torch.equal(a, b) for a, b in zip(res["dw5"], res["generic"]) if a is not None)
            ms = {k: [] for k in runs}
            for f in runs.values():
                P.timed(f, None, 3)
            for _ in range(rounds):                         # interleaved: A, B, A, B, ...
                for k, f in runs.items():
                    ms[k].append(P.timed(f, None, 20))
            new, old = stats(ms["dw5"]), stats(ms["generic"])
            spread = max(new["ms_max"] - new["ms_min"], old["ms_max"] - old["ms_min"])
            elems = batch * c * ((hw - 1) // stride + 1) ** 2
            rows.append({"channels": c, "input": hw, "stride": stride, "variant": tag, "batch": batch, "equal": bool(equal), "dw5": new, "generic": old,
                         "spread_ms": round(spread, 4), "speedup_median": round(old["ms_median"] / new["ms_median"], 3),
                         "faster_beyond_spread": bool(old["ms_median"] - new["ms_median"] > spread),
                         "dw5_gelem_per_s": round(elems / (new["ms_median"] * 1e-3) / 1e9, 2)})
            print(rows[-1], flush=True)
        del x
        torch.cuda.empty_cache()
    return rows


def whole_plan(batch, rounds):
    out = {}
    for tag, fam in (("efficientnet_b0_fsptq_w8a8", "fsptq"), ("efficientnet_b0_qbase_w8a8", "qbase")):
        model = P.seeded_model(W.efficientnet_b0)
        x = P.relu_images(batch, 224)
        P.calibrated(model, fam, x)
        with torch.no_grad():
            plans = {"dw5": fuse_inference(model, gates=True, swish=True, dw5=True), "flag_off": fuse_inference(model, gates=True, swish=True)}
            logits = {k: p(x) for k, p in plans.items()}
            torch.cuda.synchronize()
            ms = P.interleaved(plans, x, 2, rounds, 3)
        res = {"batch": batch, "logits_equal": bool(torch.equal(logits["dw5"], logits["flag_off"])), "dw5_layers": plans["dw5"].fusion_report.dw5,
               "int8_layers": plans["dw5"].fusion_report.layers, "dw5": stats(ms["dw5"]), "flag_off": stats(ms["flag_off"])}
        res["spread_ms"] = round(max(res[k]["ms_max"] - res[k]["ms_min"] for k in ("dw5", "flag_off")), 4)
        res["speedup_median"] = round(res["flag_off"]["ms_median"] / res["dw5"]["ms_median"], 3)
        out[tag] = res
        print(tag, res, flush=True)
        del model, plans, x, logits
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--plan-batch", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out")
    a = ap.parse_args()
    out = {"standalone": standalone(a.batch, a.rounds), "whole_plan": whole_plan(a.plan_batch, a.rounds), "rounds": a.rounds}
    out["every_standalone_case_faster_beyond_spread"] = all(r["faster_beyond_spread"] for r in out["standalone"])
    out["every_result_equal"] = all(r["equal"] for r in out["standalone"]) and all(r["logits_equal"] for r in out["whole_plan"].values())
    P.write_profile("dw5_ab", out, a.out)


if __name__ == "__main__":
    main()
