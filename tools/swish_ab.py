#!/usr/bin/env python3
"""Swish activations on the int8 plan (fuse_inference(swish=True): every `x * sigmoid(x)` of a map one launch of csrc/swish.hip that
hands the plan convolutions behind it their activation codes and everybody else the activated fp32 map) against the plan that runs
torch's sigmoid and multiply and lets the consumer quantise - `gates=True` in both: both plans built from ONE calibrated model and timed
interleaved, step by step, in one process.
  cases: the MBConv-SE network (workloads.mobilenet_v2(se=True, act="swish"): 35 swishes on maps, 17 gates) at 224^2, FSPTQ W8A8 (zero
         points set to exactly 0 after calibration, as the tests do) and QBase W8A8.
Per case: median ms per step of either plan over `steps` single steps each (A, B, A, B, ...), the run-to-run spread = the interquartile
range of the flag-off plan's steps, whether the flag-on plan is faster by more than that, max |delta logit| and top-1 agreement between
the two plans, and per swish node the kernel's time, bytes per second (per pixel: 4 C read, 4 C written if the fp32 map is wanted, c_pad
code bytes written) and elements per second.  Writes profiles/swish_ab.json (and prints it).
usage: python tools/swish_ab.py [batch] [steps] [--out PATH]"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc.utils.fuse import SwishLayer, fuse_inference

CASES = [("mbconv_se_fsptq_w8a8", "fsptq"), ("mbconv_se_qbase_w8a8", "qbase")]


def swish_kernel_times(plan, x, reps=20):
    """Per SwishLayer node (node_times): the kernel's time, bytes and elements per second."""
    rows = []
    for name, m, (t,), ms in P.node_times(plan, x, SwishLayer, reps):
        n, c, h, w = t.shape
        codes = m.c_pad if m.emit is not None else 0
        nbytes = n * h * w * (c * (4 + 4 * m.want_out) + codes)
        rows.append({"node": name, "input": [n, c, h, w], "floats_per_input_pixel": int(t.stride(3)), "c_pad": m.c_pad,
                     "codes_written": m.emit is not None, "fp32_written": m.want_out, "us": round(ms * 1e3, 2), "bytes": nbytes,
                     "gb_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1), "gelem_per_s": round(t.numel() / (ms * 1e-3) / 1e9, 1)})
    return rows


def main():
    arg = P.arguments(__doc__, batch=1024, steps=24)
    out = {"model": "mobilenet_v2(se=True, act='swish')", "batch": arg.batch, "steps_per_plan": arg.steps, "resolution": 224}
    for tag, fam in CASES:
        model = P.seeded_model(lambda: W.mobilenet_v2(se=True, act="swish"))
        x = P.relu_images(arg.batch, 224)
        P.calibrated(model, fam, x)
        with torch.no_grad():
            plans = {"swish": fuse_inference(model, gates=True, swish=True), "flag_off": fuse_inference(model, gates=True)}
            logits = {k: p(x) for k, p in plans.items()}
            kernels = swish_kernel_times(plans["swish"], x)
            ms = P.interleaved(plans, x, 3, arg.steps, 1)
        total, elems = sum(r["bytes"] for r in kernels), sum(r["input"][0] * r["input"][1] * r["input"][2] * r["input"][3] for r in kernels)
        us = sum(r["us"] for r in kernels)
        a, b = logits["swish"].float(), logits["flag_off"].float()
        res = {"logits_equal": bool(torch.equal(a, b)), "max_abs_delta_logit": float((a - b).abs().max()),
               "top1_agreement": float((a.argmax(1) == b.argmax(1)).float().mean()), "swish_kernels": kernels,
               "swish_kernels_total": {"us": round(us, 1), "bytes": total, "gb_per_s": round(total / (us * 1e-6) / 1e9, 1),
                                       "gelem_per_s": round(elems / (us * 1e-6) / 1e9, 1)}}
        for k, v in ms.items():
            rep = plans[k].fusion_report
            res[k] = dict(P.arm_summary(v, P.QUARTILES), int8_layers=rep.layers, gates=rep.gates, swishes=rep.swishes,
                          fp32_outputs=rep.fp32_outputs, not_eligible=len(rep.skipped))
        res.update(P.verdict(res["swish"], res["flag_off"], "iqr_off", ("faster",)))
        out[tag] = res
        del model, plans, x, logits
        torch.cuda.empty_cache()
    P.write_profile("swish_ab", out, arg.out)


if __name__ == "__main__":
    main()
