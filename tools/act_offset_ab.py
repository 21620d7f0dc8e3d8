#!/usr/bin/env python3
"""Float activation offsets in the int8 plan (fuse_inference(act_offsets=True)) against the plan that leaves every layer with a float
offset on its wrapper (act_offsets=False): both plans built from ONE calibrated model and timed interleaved in one process.
  case 1: MobileNetV2, QBase W4A8 (tools/plan_ab.py's QBASE_W4A8), relu(N(0,1)) images - the 17 layers that read shortcut sums;
  case 2: ResNet-50, QBase W8A8, ImageNet-normalised images - the first layer (its input minimum is about -2.1).
Prints one JSON object.  usage: python tools/act_offset_ab.py [batch] [rounds] [--out PATH]"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc.utils.fuse import fuse_inference


def images(batch, normalised):
    if not normalised:
        return P.relu_images(batch, 224)
    mean = torch.tensor([0.485, 0.456, 0.406], device=P.DEV)[:, None, None]
    std = torch.tensor([0.229, 0.224, 0.225], device=P.DEV)[:, None, None]
    return (torch.rand(batch, 3, 224, 224, device=P.DEV) - mean) / std


def main():
    a = P.arguments(__doc__, batch=1024, rounds=5)
    out = {"batch": a.batch, "resolution": 224, "rounds": a.rounds}
    for tag, name, cfg, normalised in (("mobilenet_v2_qbase_w4a8", "mobilenet_v2", P.QBASE_W4A8, False),
                                       ("resnet50_qbase_w8a8_normalised", "resnet50", P.QBASE_W8A8, True)):
        model = P.seeded_model(W.MODELS[name])
        P.quantized(model, cfg)
        x = images(a.batch, normalised)
        with torch.no_grad():
            model(x[:64])                                   # calibrate
            plans = {"offsets": fuse_inference(model, act_offsets=True), "no_offsets": fuse_inference(model)}
            first = {k: p(x) for k, p in plans.items()}
            again = {k: p(x) for k, p in plans.items()}
            want = model(x[:64])
            ms = P.interleaved(plans, x, 2, a.rounds, 3)
        res = {"identical_run_to_run": {k: bool(torch.equal(first[k], again[k])) for k in plans},
               "rel_l2_to_wrappers_first64": {k: round(float((first[k][:64] - want).norm() / want.norm()), 4) for k in plans}}
        for k, v in ms.items():
            rep = plans[k].fusion_report
            res[k] = dict(P.arm_summary(v, ("median", "min"), a.batch), act_offset_layers=rep.act_offset, int8_layers=rep.layers)
        res["speedup_median"] = P.speedup_median(res["offsets"], res["no_offsets"])
        out[tag] = res
        del model, plans, x, first, again
        torch.cuda.empty_cache()
    P.write_profile(None, out, a.out)


if __name__ == "__main__":
    main()
