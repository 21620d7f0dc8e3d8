#!/usr/bin/env python3
"""ReLU6 fused into the int8 plan's epilogues (fuse_inference(relu6=True)) against the plan that keeps every ReLU6 a separate op
(relu6=False), on MobileNetV2 at 224^2: both plans built from ONE calibrated model and timed interleaved in one process, for FSPTQ W8A8
(bench.py's QCFG) and QBase W4A8 with asymmetric per-channel weights (BASELINE config 5's quantiser).  Prints one JSON object.
usage: python tools/relu6_ab.py [batch] [rounds]"""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dlmc-quant_amd")]
import torch  # noqa: E402

import workloads as W  # noqa: E402
from bench import QCFG  # noqa: E402
from dlmc.utils.fuse import fuse_inference  # noqa: E402
from dlmc.utils.merge_bn import merge_bn  # noqa: E402
from dlmc.utils.quantize import quantize_model  # noqa: E402

QBASE_W4A8 = {"weight": {"enable": True, "type": "minmax_channel", "args": {"n_bits": 4, "signed": False}},
              "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
              "exclude_layers": [], "override_options": []}


def timed(fn, x, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn(x)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = "cuda:0"
    out = {"model": "mobilenet_v2", "batch": batch, "resolution": 224, "rounds": rounds}
    for tag, cfg, qtype in (("fsptq_w8a8", QCFG, "FSPTQ"), ("qbase_w4a8_asym", QBASE_W4A8, None)):
        torch.manual_seed(2333)
        model = merge_bn(W.mobilenet_v2().to(dev).eval(), inplace=True)
        kw = {"quantization_type": qtype, "int8_gemm": True} if qtype else {}
        quantize_model(model, copy.deepcopy(cfg), None, **kw)
        x = torch.relu(torch.randn(batch, 3, 224, 224, device=dev))
        with torch.no_grad():
            model(x[:64])                                   # calibrate
            plans = {"relu6_fused": fuse_inference(model), "relu6_separate": fuse_inference(model, relu6=False)}
            same = torch.equal(plans["relu6_fused"](x), plans["relu6_separate"](x))
            for p in plans.values():                        # warm-up
                timed(p, x, 2)
            ms = {k: [] for k in plans}
            for _ in range(rounds):                         # interleaved: A, B, A, B, ...
                for k, p in plans.items():
                    ms[k].append(timed(p, x, 3))
        res = {"identical_logits": bool(same)}
        for k, v in ms.items():
            best, med = min(v), sorted(v)[len(v) // 2]
            res[k] = {"ms_per_step_median": round(med, 3), "ms_per_step_min": round(best, 3), "images_per_s": round(batch / med * 1e3, 1),
                      "all_ms": [round(t, 3) for t in v]}
        res["speedup_median"] = round(res["relu6_separate"]["ms_per_step_median"] / res["relu6_fused"]["ms_per_step_median"], 3)
        res["report_fused"] = repr(plans["relu6_fused"].fusion_report)
        out[tag] = res
        del model, plans, x
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
