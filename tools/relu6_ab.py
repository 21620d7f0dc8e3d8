#!/usr/bin/env python3
"""ReLU6 fused into the int8 plan's epilogues (fuse_inference(relu6=True)) against the plan that keeps every ReLU6 a separate op
(relu6=False), on MobileNetV2 at 224^2: both plans built from ONE calibrated model and timed interleaved in one process, for FSPTQ W8A8
(bench.py's QCFG) and QBase W4A8 with asymmetric per-channel weights (BASELINE config 5's quantiser).  Prints one JSON object.
usage: python tools/relu6_ab.py [batch] [rounds] [--out PATH]"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc.utils.fuse import fuse_inference


def main():
    a = P.arguments(__doc__, batch=1024, rounds=5)
    out = {"model": "mobilenet_v2", "batch": a.batch, "resolution": 224, "rounds": a.rounds}
    for tag, cfg, qtype in (("fsptq_w8a8", P.FSPTQ_W8A8, "FSPTQ"), ("qbase_w4a8_asym", P.QBASE_W4A8, None)):
        model = P.seeded_model(W.mobilenet_v2)
        P.quantized(model, cfg, qtype)
        x = P.relu_images(a.batch, 224)
        with torch.no_grad():
            model(x[:64])                                   # calibrate
            plans = {"relu6_fused": fuse_inference(model), "relu6_separate": fuse_inference(model, relu6=False)}
            same = torch.equal(plans["relu6_fused"](x), plans["relu6_separate"](x))
            ms = P.interleaved(plans, x, 2, a.rounds, 3)
        res = {"identical_logits": bool(same)}
        for k, v in ms.items():
            res[k] = P.arm_summary(v, ("median", "min"), a.batch)
        res["speedup_median"] = P.speedup_median(res["relu6_fused"], res["relu6_separate"])
        res["report_fused"] = repr(plans["relu6_fused"].fusion_report)
        out[tag] = res
        del model, plans, x
        torch.cuda.empty_cache()
    P.write_profile(None, out, a.out)


if __name__ == "__main__":
    main()
