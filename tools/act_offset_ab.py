#!/usr/bin/env python3
"""Float activation offsets in the int8 plan (fuse_inference(act_offsets=True)) against the plan that leaves every layer with a float
offset on its wrapper (act_offsets=False): both plans built from ONE calibrated model and timed interleaved in one process.
  case 1: MobileNetV2, QBase W4A8 (tools/relu6_ab.py's QBASE_W4A8), relu(N(0,1)) images - the 17 layers that read shortcut sums;
  case 2: ResNet-50, QBase W8A8, ImageNet-normalised images - the first layer (its input minimum is about -2.1).
Prints one JSON object.  usage: python tools/act_offset_ab.py [batch] [rounds]"""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dlmc-quant_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

import workloads as W  # noqa: E402
from dlmc.utils.fuse import fuse_inference  # noqa: E402
from dlmc.utils.merge_bn import merge_bn  # noqa: E402
from dlmc.utils.quantize import quantize_model  # noqa: E402
from relu6_ab import QBASE_W4A8, timed  # noqa: E402

QBASE_W8A8 = {"weight": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": True}},
              "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
              "exclude_layers": [], "override_options": []}


def images(batch, normalised, dev):
    if not normalised:
        return torch.relu(torch.randn(batch, 3, 224, 224, device=dev))
    mean = torch.tensor([0.485, 0.456, 0.406], device=dev)[:, None, None]
    std = torch.tensor([0.229, 0.224, 0.225], device=dev)[:, None, None]
    return (torch.rand(batch, 3, 224, 224, device=dev) - mean) / std


def main():
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = "cuda:0"
    out = {"batch": batch, "resolution": 224, "rounds": rounds}
    for tag, name, cfg, normalised in (("mobilenet_v2_qbase_w4a8", "mobilenet_v2", QBASE_W4A8, False),
                                       ("resnet50_qbase_w8a8_normalised", "resnet50", QBASE_W8A8, True)):
        torch.manual_seed(2333)
        model = merge_bn(W.MODELS[name]().to(dev).eval(), inplace=True)
        quantize_model(model, copy.deepcopy(cfg), None)
        x = images(batch, normalised, dev)
        with torch.no_grad():
            model(x[:64])                                   # calibrate
            plans = {"offsets": fuse_inference(model, act_offsets=True), "no_offsets": fuse_inference(model)}
            first = {k: p(x) for k, p in plans.items()}
            again = {k: p(x) for k, p in plans.items()}
            want = model(x[:64])
            for p in plans.values():                        # warm-up
                timed(p, x, 2)
            ms = {k: [] for k in plans}
            for _ in range(rounds):                         # interleaved: A, B, A, B, ...
                for k, p in plans.items():
                    ms[k].append(timed(p, x, 3))
        res = {"identical_run_to_run": {k: bool(torch.equal(first[k], again[k])) for k in plans},
               "rel_l2_to_wrappers_first64": {k: round(float((first[k][:64] - want).norm() / want.norm()), 4) for k in plans}}
        for k, v in ms.items():
            med = sorted(v)[len(v) // 2]
            res[k] = {"ms_per_step_median": round(med, 3), "ms_per_step_min": round(min(v), 3), "images_per_s": round(batch / med * 1e3, 1),
                      "all_ms": [round(t, 3) for t in v], "act_offset_layers": plans[k].fusion_report.act_offset,
                      "int8_layers": plans[k].fusion_report.layers}
        res["speedup_median"] = round(res["no_offsets"]["ms_per_step_median"] / res["offsets"]["ms_per_step_median"], 3)
        out[tag] = res
        del model, plans, x, first, again
        torch.cuda.empty_cache()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
