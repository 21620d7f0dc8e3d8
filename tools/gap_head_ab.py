#!/usr/bin/env python3
"""Global-average-pool heads on the int8 plan (fuse_inference(gap_head=...)): the plan without them (False: fp32 map -> torch's pool ->
the classifier's quantise pass) against the pool kernel behind the last layer ("separate", csrc/gap.hip), the default route of the
feature (True: the fused head only where it is not measured slower) and the fused head wherever it is built ("fused",
csrc/conv_gap_i8.hip), for ResNet-50 b512, MobileNetV2 b1024, RepVGG-A1 b512 and MobileOne-S1 b1024 at 224^2 under
bench.py's FSPTQ W8A8.  The four plans are built from ONE calibrated model and timed interleaved in one process; besides the step
times, the head's own launches (HIP events, K.PROFILE tags gap / conv_gap) of one profiled step each.  FSPTQ's zero points are set to 0
after calibration (the classifier reads a pooled tensor whose minimum is not 0: no integer zero point, no plan node otherwise).
Prints one JSON object and writes it to profiles/gap_head_ab.json.
usage: python tools/gap_head_ab.py [rounds] [scale]      (scale divides the batch sizes: a quick run)"""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dlmc-quant_amd")]
import torch  # noqa: E402

import workloads as W  # noqa: E402
from bench import QCFG  # noqa: E402
from dlmc.quantization.scalar import kernels as K  # noqa: E402
from dlmc.quantization.scalar.FSPTQuant import FSPTQBase  # noqa: E402
from dlmc.utils.fuse import fuse_inference  # noqa: E402
from dlmc.utils.merge_bn import merge_bn  # noqa: E402
from dlmc.utils.quantize import quantize_model  # noqa: E402

CASES = (("resnet50", 512), ("mobilenet_v2", 1024), ("repvgg_a1", 512), ("mobileone_s1", 1024))
FLAGS = (("off", False), ("separate", "separate"), ("true", True), ("fused", "fused"))


def timed(fn, x, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn(x)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def head_launches(plan, x):
    """HIP-event times (us) of the head's launches in one profiled step: tags gap / conv_gap, and the last launch in front of them."""
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        plan(x)
        torch.cuda.synchronize()
        recs = [(tag, nbytes, a.elapsed_time(b) * 1e3) for tag, nbytes, a, b, _ in K.PROFILE.records]
    finally:
        K.PROFILE.enabled = False
        K.PROFILE.reset()
    out = []
    for i, (tag, nbytes, us) in enumerate(recs):
        if tag in ("gap", "conv_gap"):
            if tag == "gap" and i:
                out.append({"tag": recs[i - 1][0] + " (producer)", "bytes": recs[i - 1][1], "us": round(recs[i - 1][2], 1)})
            out.append({"tag": tag, "bytes": nbytes, "us": round(us, 1)})
    return out or [{"tag": t, "bytes": nb, "us": round(us, 1)} for t, nb, us in recs[-2:]]


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    scale = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    dev = "cuda:0"
    out = {"resolution": 224, "rounds": rounds, "quantiser": "FSPTQ W8A8 (bench.py QCFG), zero points 0"}
    for name, batch in CASES:
        batch //= scale
        torch.manual_seed(2333)
        model = merge_bn(W.MODELS[name]().to(dev).eval(), inplace=True, allow_missing=True)
        quantize_model(model, copy.deepcopy(QCFG), None, quantization_type="FSPTQ", int8_gemm=True)
        x = torch.relu(torch.randn(batch, 3, 224, 224, device=dev))
        with torch.no_grad():
            model(x[:64])                                   # calibrate
            for m in model.modules():
                if isinstance(m, FSPTQBase):
                    m.in_offset.zero_()
                    m._zp_is_int = None
            plans = {k: fuse_inference(model, gap_head=flag) for k, flag in FLAGS}
            logits = {k: p(x) for k, p in plans.items()}
            for p in plans.values():                        # warm-up
                timed(p, x, 2)
            ms = {k: [] for k in plans}
            for _ in range(rounds):                         # interleaved: A, B, C, D, A, B, C, D, ...
                for k, p in plans.items():
                    ms[k].append(timed(p, x, 3))
            res = {"batch": batch, "fused_equals_separate": bool(torch.equal(logits["fused"], logits["separate"])),
                   "true_equals_separate": bool(torch.equal(logits["true"], logits["separate"])),
                   "max_abs_logit": float(logits["off"].abs().max()),
                   "max_abs_logit_difference_to_off": float((logits["fused"] - logits["off"]).abs().max()),
                   "heads": {k: plans[k].fusion_report.gap_heads for k in plans}}
            for k, v in ms.items():
                best, med = min(v), sorted(v)[len(v) // 2]
                res[k] = {"ms_per_step_median": round(med, 3), "ms_per_step_min": round(best, 3), "ms_per_step_max": round(max(v), 3),
                          "images_per_s": round(batch / med * 1e3, 1), "all_ms": [round(t, 3) for t in v],
                          "head_launches": head_launches(plans[k], x)}
        for k in ("separate", "true", "fused"):
            res[f"speedup_median_{k}_over_off"] = round(res["off"]["ms_per_step_median"] / res[k]["ms_per_step_median"], 4)
        out[name] = res
        del model, plans, x, logits
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "gap_head_ab.json"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
