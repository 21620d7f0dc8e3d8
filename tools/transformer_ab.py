#!/usr/bin/env python3
"""LayerNorm and GELU nodes on the int8 plan (fuse_inference(layer_norms=True, gelu=True): every `LayerNorm -> Linear` one launch of
csrc/layernorm.hip and every `GELU -> Linear` one launch of csrc/gelu.hip, each handing the Linear layer behind it its activation codes)
against the plan that runs torch's LayerNorm and GELU and lets the consumer quantise: both plans built from ONE calibrated model and timed
interleaved, step by step, in one process.
  cases: workloads.vit_small() (ViT-S/16: 25 LayerNorms, 12 GELUs, 50 Linear layers) at 224^2, FSPTQ W8A8 (the calibrated zero points
         rounded to integers) and QBase W8A8 (float offsets set to 0).  Attention's products and softmax run in torch in both plans.
Per case: median ms per step of either plan over `steps` single steps each (A, B, A, B, ...), the run-to-run spread = the interquartile
range of the flag-off plan's steps, whether the flag-on plan is faster by more than that, how many logits differ between the two plans and
by how much, and per kernel - from the launch profile's records of one step (K.PROFILE: algorithmic bytes, event times) - launches, time,
bytes per second and elements per second.  Writes profiles/transformer_ab.json (and prints it).
usage: python tools/transformer_ab.py [batch] [steps] [--out PATH]"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc.utils.fuse import GeluLayer, LayerNormLayer, fuse_inference

TAGS = {"layernorm": LayerNormLayer, "gelu": GeluLayer}


def main():
    arg = P.arguments(__doc__, batch=256, steps=24)
    out = {"model": "vit_small()", "batch": arg.batch, "steps_per_plan": arg.steps, "resolution": 224}
    for tag, fam in P.CASES:
        model = P.seeded_model(W.vit_small, bn=False)
        x = torch.randn(arg.batch, 3, 224, 224, device=P.DEV)
        P.calibrate(model, fam, x)
        with torch.no_grad():
            plans = {"nodes": fuse_inference(model, layer_norms=True, gelu=True), "flag_off": fuse_inference(model)}
            logits = {k: p(x) for k, p in plans.items()}
            kernels = P.kernel_profile(plans["nodes"], x, TAGS, warm=True)
            ms = P.interleaved(plans, x, 3, arg.steps, 1)
        a, b = logits["nodes"].float(), logits["flag_off"].float()
        res = {"logits_equal": bool(torch.equal(a, b)), "logits": a.numel(), "logits_that_differ": int((a != b).sum()),
               "max_abs_delta_logit": float((a - b).abs().max()), "max_abs_logit": float(b.abs().max()),
               "top1_agreement": float((a.argmax(1) == b.argmax(1)).float().mean()), "kernels": kernels}
        for k, v in ms.items():
            rep = plans[k].fusion_report
            res[k] = dict(P.arm_summary(v, P.QUARTILES), int8_layers=rep.layers, layer_norms=rep.layer_norms, gelus=rep.gelus,
                          fp32_outputs=rep.fp32_outputs, not_eligible=len(rep.skipped))
        res.update(P.verdict(res["nodes"], res["flag_off"], "iqr_off"))
        out[tag] = res
        del model, plans, x, logits
        torch.cuda.empty_cache()
    P.write_profile("transformer_ab", out, arg.out)


if __name__ == "__main__":
    main()
