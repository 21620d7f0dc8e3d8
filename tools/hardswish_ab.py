#!/usr/bin/env python3
"""Hard-swish activations on the int8 plan (fuse_inference(hardswish=True): every hard swish of a map one launch of csrc/hardswish.hip
that hands the plan convolutions behind it their activation codes and everybody else the activated fp32 map) against the plan that runs
torch's own hard swish and lets the consumer quantise - `gates=True, dw5=True` in both: both plans built from ONE calibrated model and
timed interleaved, step by step, in one process.
  cases: workloads.mobilenet_v3_large() (20 hard swishes on maps, 8 gates) and mobilenet_v3_small() (18, 9) at 224^2, FSPTQ W8A8 (zero
         points set to exactly 0 after calibration, as the tests do) and QBase W8A8.
Per case: median ms per step of either plan over `steps` single steps each (A, B, A, B, ...), the run-to-run spread = the interquartile
range of the flag-off plan's steps, whether the flag-on plan is faster - or slower - by more than that, how many logits differ between
the two plans, and from the launch profile of one flag-on step (K.PROFILE: the wrapper's own byte count - per pixel 4 C read, 4 C
written if the fp32 map is wanted, c_pad code bytes written - between two events per launch) the kernel's time, bytes and elements per
second over its launches.  Writes profiles/hardswish_ab.json (and prints it).
usage: python tools/hardswish_ab.py [batch] [steps] [--out PATH]"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc.utils.fuse import HardswishLayer, fuse_inference

NETS = {"mobilenet_v3_large": W.mobilenet_v3_large, "mobilenet_v3_small": W.mobilenet_v3_small}
FLAGS = dict(gates=True, dw5=True)


def main():
    arg = P.arguments(__doc__, batch=256, steps=24)
    out = {"batch": arg.batch, "steps_per_plan": arg.steps, "resolution": 224, "flags_in_both": FLAGS}
    for net, make in NETS.items():
        for fam in ("fsptq", "qbase"):
            model = P.seeded_model(make)
            x = P.relu_images(arg.batch, 224)
            P.calibrated(model, fam, x)
            with torch.no_grad():
                plans = {"hardswish": fuse_inference(model, hardswish=True, **FLAGS), "flag_off": fuse_inference(model, **FLAGS)}
                logits = {k: p(x) for k, p in plans.items()}
                for p in plans.values():                        # warm-up here: this tool profiles the warm plan
                    P.timed(p, x, 3)
                kernel = P.kernel_profile(plans["hardswish"], x, {"hardswish": HardswishLayer})["hardswish"]
                ms = P.interleaved(plans, x, 0, arg.steps, 1)
            a, b = logits["hardswish"].float(), logits["flag_off"].float()
            res = {"logits": a.numel(), "logits_that_differ": int((a != b).sum()), "max_abs_delta_logit": float((a - b).abs().max()),
                   "hardswish_kernel": kernel}
            for k, v in ms.items():
                rep = plans[k].fusion_report
                res[k] = dict(P.arm_summary(v, P.QUARTILES), int8_layers=rep.layers, gates=rep.gates, hardswishes=rep.hardswishes,
                              fp32_outputs=rep.fp32_outputs, not_eligible=len(rep.skipped))
            nodes = [m for m in plans["hardswish"].modules() if isinstance(m, HardswishLayer)]
            res["hardswish"]["nodes_handing_codes_on"] = sum(m.emit is not None for m in nodes)
            res.update(P.verdict(res["hardswish"], res["flag_off"], "iqr_off"))
            out[f"{net}_{fam}_w8a8"] = res
            del model, plans, x, logits
            torch.cuda.empty_cache()
    P.write_profile("hardswish_ab", out, arg.out)


if __name__ == "__main__":
    main()
