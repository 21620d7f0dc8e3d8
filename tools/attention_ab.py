#!/usr/bin/env python3
"""Attention nodes on the int8 plan (fuse_inference(attention=True): every `softmax(q k^T * c) v` + merge-heads tail one launch of
csrc/attention.hip that hands `to_out` its activation codes) against the plan that runs the two products and the softmax in torch and
lets `to_out` quantise: both plans built from ONE calibrated model, both with layer_norms=True and gelu=True, timed interleaved, step by
step, in one process.
  cases: workloads.vit_small() (ViT-S/16: 12 attention cores of 6 heads, T = 197, d = 64) at 224^2, FSPTQ W8A8 (the calibrated zero
         points rounded to integers) and QBase W8A8 (float offsets set to 0).
Per case: median ms per step of either plan over `steps` single steps each (A, B, A, B, ...), the run-to-run spread = the interquartile
range of the flag-off plan's steps, whether the flag-on plan is faster by more than that, how many logits differ between the two plans,
by how much, and the top-1 agreement; for the kernel - from the launch profile's records of one step (K.PROFILE: algorithmic bytes and
operations, event times) - launches, time, TFLOP/s and bytes per second; and what the flag-off plan spends on attention: the launch
profile has no record of torch's own kernels, so the same op sequence (the views, two products, multiply, softmax, permute + reshape)
is timed with events on a [batch, 197, 1152] projection output, and `to_out`'s quantise passes are read from the profile.
Writes profiles/attention_ab.json (and prints it).
usage: python tools/attention_ab.py [batch] [steps] [--out PATH]"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc.utils.fuse import fuse_inference

FLAGS = dict(layer_norms=True, gelu=True)


def unfused_attention_us(batch, heads, dim_head, tokens, runs=9):
    """Median time of one block's attention as the flag-off plan runs it, in torch, on a projection output of the real shape."""
    qkv = torch.randn(batch, tokens, 3 * heads * dim_head, device=P.DEV)

    def once(_):
        p = qkv.reshape(batch, tokens, 3, heads, dim_head).permute(2, 0, 3, 1, 4)
        q, k, v = p[0], p[1], p[2]
        attn = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * dim_head ** -0.5, dim=-1)
        return torch.matmul(attn, v).permute(0, 2, 1, 3).reshape(batch, tokens, heads * dim_head)
    for _ in range(2):
        once(None)
    return P.quartiles([P.timed(once, None, 1) * 1e3 for _ in range(runs)])[1]


def main():
    arg = P.arguments(__doc__, batch=256, steps=24)
    out = {"model": "vit_small()", "batch": arg.batch, "steps_per_plan": arg.steps, "resolution": 224, "both_plans": FLAGS}
    for tag, fam in P.CASES:
        model = P.seeded_model(W.vit_small, bn=False)
        x = torch.randn(arg.batch, 3, 224, 224, device=P.DEV)
        P.calibrate(model, fam, x)
        with torch.no_grad():
            plans = {"attention": fuse_inference(model, attention=True, **FLAGS), "flag_off": fuse_inference(model, **FLAGS)}
            logits = {k: p(x) for k, p in plans.items()}
            recs = {k: P.profile_step(p, x) for k, p in plans.items()}
            torch_us = unfused_attention_us(arg.batch, 6, 64, 197)
            ms = P.interleaved(plans, x, 3, arg.steps, 1)
        a, b = logits["attention"].float(), logits["flag_off"].float()
        mine = [r for r in recs["attention"] if r[0] == "attention"]
        t_ms, nbytes, ops = sum(r[2] for r in mine), sum(r[1] for r in mine), sum(r[3] for r in mine)
        fq = {k: [r[2] for r in v if r[0] == "fq_tensor"] for k, v in recs.items()}
        res = {"logits_equal": bool(torch.equal(a, b)), "logits": a.numel(), "logits_that_differ": int((a != b).sum()),
               "max_abs_delta_logit": float((a - b).abs().max()), "max_abs_logit": float(b.abs().max()),
               "top1_agreement": float((a.argmax(1) == b.argmax(1)).float().mean()),
               "kernel": {"launches": len(mine), "us": round(t_ms * 1e3, 1), "flop": ops, "bytes": nbytes,
                          "tflop_per_s": round(ops / (t_ms * 1e-3) / 1e12, 1) if t_ms else None,
                          "gb_per_s": round(nbytes / (t_ms * 1e-3) / 1e9, 1) if t_ms else None},
               "flag_off_attention": {"torch_ops_us_per_block": round(torch_us, 1), "blocks": 12, "torch_ops_us_per_step": round(12 * torch_us, 1),
                                      "quantise_launches_saved": len(fq["flag_off"]) - len(fq["attention"]),
                                      "quantise_us_flag_off": round(sum(fq["flag_off"]) * 1e3, 1),
                                      "quantise_us_flag_on": round(sum(fq["attention"]) * 1e3, 1)}}
        for k, v in ms.items():
            rep = plans[k].fusion_report
            res[k] = dict(P.arm_summary(v, P.QUARTILES), int8_layers=rep.layers, layer_norms=rep.layer_norms, gelus=rep.gelus,
                          attentions=rep.attentions, fp32_outputs=rep.fp32_outputs, not_eligible=len(rep.skipped))
        res["flag_off_attention"]["share_of_step"] = round(12 * torch_us * 1e-3 / res["flag_off"]["ms_per_step_median"], 3)
        res.update(P.verdict(res["attention"], res["flag_off"], "iqr_off"))
        out[tag] = res
        del model, plans, x, logits
        torch.cuda.empty_cache()
    P.write_profile("attention_ab", out, arg.out)


if __name__ == "__main__":
    main()
