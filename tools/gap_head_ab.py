#!/usr/bin/env python3
"""Global-average-pool heads on the int8 plan (fuse_inference(gap_head=...)): the plan without them (False: fp32 map -> torch's pool ->
the classifier's quantise pass) against the pool kernel behind the last layer ("separate", csrc/gap.hip), the default route of the
feature (True: the fused head only where it is not measured slower) and the fused head wherever it is built ("fused",
csrc/conv_gap_i8.hip), for ResNet-50 b512, MobileNetV2 b1024, RepVGG-A1 b512 and MobileOne-S1 b1024 at 224^2 under
bench.py's FSPTQ W8A8.  The four plans are built from ONE calibrated model and timed interleaved in one process; besides the step
times, the head's own launches (HIP events, K.PROFILE tags gap / conv_gap) of one profiled step each.  FSPTQ's zero points are set to 0
after calibration (the classifier reads a pooled tensor whose minimum is not 0: no integer zero point, no plan node otherwise).
Prints one JSON object and writes it to profiles/gap_head_ab.json.
usage: python tools/gap_head_ab.py [rounds] [scale] [--out PATH]      (scale divides the batch sizes: a quick run)"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc.utils.fuse import fuse_inference

CASES = (("resnet50", 512), ("mobilenet_v2", 1024), ("repvgg_a1", 512), ("mobileone_s1", 1024))
FLAGS = (("off", False), ("separate", "separate"), ("true", True), ("fused", "fused"))


def head_launches(plan, x):
    """HIP-event times (us) of the head's launches in one profiled step: tags gap / conv_gap, and the last launch in front of them."""
    recs = [(tag, nbytes, ms * 1e3) for tag, nbytes, ms, _ in P.profile_step(plan, x, warm=False)]
    out = []
    for i, (tag, nbytes, us) in enumerate(recs):
        if tag in ("gap", "conv_gap"):
            if tag == "gap" and i:
                out.append({"tag": recs[i - 1][0] + " (producer)", "bytes": recs[i - 1][1], "us": round(recs[i - 1][2], 1)})
            out.append({"tag": tag, "bytes": nbytes, "us": round(us, 1)})
    return out or [{"tag": t, "bytes": nb, "us": round(us, 1)} for t, nb, us in recs[-2:]]


def main():
    a = P.arguments(__doc__, rounds=5, scale=1)
    out = {"resolution": 224, "rounds": a.rounds, "quantiser": "FSPTQ W8A8 (bench.py QCFG), zero points 0"}
    for name, batch in CASES:
        batch //= a.scale
        model = P.seeded_model(W.MODELS[name])
        x = P.relu_images(batch, 224)
        P.calibrated(model, "fsptq", x)
        with torch.no_grad():
            plans = {k: fuse_inference(model, gap_head=flag) for k, flag in FLAGS}
            logits = {k: p(x) for k, p in plans.items()}
            ms = P.interleaved(plans, x, 2, a.rounds, 3)          # A, B, C, D, A, B, C, D, ...
            res = {"batch": batch, "fused_equals_separate": bool(torch.equal(logits["fused"], logits["separate"])),
                   "true_equals_separate": bool(torch.equal(logits["true"], logits["separate"])),
                   "max_abs_logit": float(logits["off"].abs().max()),
                   "max_abs_logit_difference_to_off": float((logits["fused"] - logits["off"]).abs().max()),
                   "heads": {k: plans[k].fusion_report.gap_heads for k in plans}}
            for k, v in ms.items():
                res[k] = dict(P.arm_summary(v, P.RANGE, batch), head_launches=head_launches(plans[k], x))
        for k in ("separate", "true", "fused"):
            res[f"speedup_median_{k}_over_off"] = P.speedup_median(res[k], res["off"], 4)
        out[name] = res
        del model, plans, x, logits
        torch.cuda.empty_cache()
    P.write_profile("gap_head_ab", out, a.out)


if __name__ == "__main__":
    main()
