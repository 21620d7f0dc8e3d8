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
usage: python tools/hardswish_ab.py [batch] [steps]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dlmc-quant_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

import workloads as W  # noqa: E402
from dlmc.quantization.scalar import kernels as K  # noqa: E402
from dlmc.utils.fuse import HardswishLayer, fuse_inference  # noqa: E402
from dlmc.utils.merge_bn import merge_bn  # noqa: E402
from node_times import calibrated  # noqa: E402
from relu6_ab import timed  # noqa: E402
from swish_ab import quartiles  # noqa: E402

NETS = {"mobilenet_v3_large": W.mobilenet_v3_large, "mobilenet_v3_small": W.mobilenet_v3_small}
FLAGS = dict(gates=True, dw5=True)


def kernel_profile(plan, x):
    """One step of `plan` with the launch profile on: the hard-swish launches' time, bytes and elements (the fp32 elements read)."""
    elems = []
    hooks = [m.register_forward_pre_hook(lambda mod, a: elems.append(a[0].numel())) for m in plan.modules() if isinstance(m, HardswishLayer)]
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        plan(x)
        torch.cuda.synchronize()
        recs = [(r[1], r[2].elapsed_time(r[3])) for r in K.PROFILE.records if r[0] == "hardswish"]
    finally:
        K.PROFILE.enabled = False
        K.PROFILE.reset()
        for h in hooks:
            h.remove()
    us, nbytes = sum(ms for _, ms in recs) * 1e3, sum(b for b, _ in recs)
    return {"launches": len(recs), "us": round(us, 1), "bytes": nbytes, "elements": sum(elems), "gb_per_s": round(nbytes / (us * 1e-6) / 1e9, 1),
            "gelem_per_s": round(sum(elems) / (us * 1e-6) / 1e9, 1)}


def main():
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    dev = "cuda:0"
    out = {"batch": batch, "steps_per_plan": steps, "resolution": 224, "flags_in_both": FLAGS}
    for net, make in NETS.items():
        for fam in ("fsptq", "qbase"):
            torch.manual_seed(2333)
            model = merge_bn(make().to(dev).eval(), inplace=True, allow_missing=True)
            x = torch.relu(torch.randn(batch, 3, 224, 224, device=dev))
            calibrated(model, fam, x)
            with torch.no_grad():
                plans = {"hardswish": fuse_inference(model, hardswish=True, **FLAGS), "flag_off": fuse_inference(model, **FLAGS)}
                logits = {k: p(x) for k, p in plans.items()}
                for p in plans.values():                        # warm-up
                    timed(p, x, 3)
                kernel = kernel_profile(plans["hardswish"], x)
                ms = {k: [] for k in plans}
                for _ in range(steps):                          # interleaved: A, B, A, B, ...
                    for k, p in plans.items():
                        ms[k].append(timed(p, x, 1))
            a, b = logits["hardswish"].float(), logits["flag_off"].float()
            res = {"logits": a.numel(), "logits_that_differ": int((a != b).sum()), "max_abs_delta_logit": float((a - b).abs().max()),
                   "hardswish_kernel": kernel}
            for k, v in ms.items():
                rep = plans[k].fusion_report
                q1, med, q3 = quartiles(v)
                res[k] = {"ms_per_step_median": round(med, 3), "ms_per_step_q1": round(q1, 3), "ms_per_step_q3": round(q3, 3),
                          "ms_per_step_min": round(min(v), 3), "ms_per_step_max": round(max(v), 3), "all_ms": [round(t, 3) for t in v],
                          "int8_layers": rep.layers, "gates": rep.gates, "hardswishes": rep.hardswishes, "fp32_outputs": rep.fp32_outputs,
                          "not_eligible": len(rep.skipped)}
            nodes = [m for m in plans["hardswish"].modules() if isinstance(m, HardswishLayer)]
            res["hardswish"]["nodes_handing_codes_on"] = sum(m.emit is not None for m in nodes)
            on, off = res["hardswish"], res["flag_off"]
            spread = off["ms_per_step_q3"] - off["ms_per_step_q1"]
            res["run_to_run_spread_ms"] = round(spread, 3)      # (the interquartile range of the baseline's steps)
            res["speedup_median"] = round(off["ms_per_step_median"] / on["ms_per_step_median"], 3)
            res["flag_on_faster_beyond_spread"] = bool(off["ms_per_step_median"] - on["ms_per_step_median"] > spread)
            res["flag_on_slower_beyond_spread"] = bool(on["ms_per_step_median"] - off["ms_per_step_median"] > spread)
            out[f"{net}_{fam}_w8a8"] = res
            del model, plans, x, logits
            torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "hardswish_ab.json"), "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
