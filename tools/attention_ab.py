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
usage: python tools/attention_ab.py [batch] [steps]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dlmc-quant_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

import workloads as W  # noqa: E402
from dlmc.quantization.scalar import kernels as K  # noqa: E402
from dlmc.utils.fuse import fuse_inference  # noqa: E402
from relu6_ab import timed  # noqa: E402
from swish_ab import quartiles  # noqa: E402
from transformer_ab import CASES, calibrate  # noqa: E402

FLAGS = dict(layer_norms=True, gelu=True)


def profile_step(plan, x):
    plan(x)                                             # (warm)
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        plan(x)
        torch.cuda.synchronize()
        return [(r[0], r[1], r[2].elapsed_time(r[3]), r[4]) for r in K.PROFILE.records]
    finally:
        K.PROFILE.enabled = False
        K.PROFILE.reset()


def unfused_attention_us(batch, heads, dim_head, tokens, dev, runs=9):
    """Median time of one block's attention as the flag-off plan runs it, in torch, on a projection output of the real shape."""
    qkv = torch.randn(batch, tokens, 3 * heads * dim_head, device=dev)

    def once():
        p = qkv.reshape(batch, tokens, 3, heads, dim_head).permute(2, 0, 3, 1, 4)
        q, k, v = p[0], p[1], p[2]
        attn = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * dim_head ** -0.5, dim=-1)
        return torch.matmul(attn, v).permute(0, 2, 1, 3).reshape(batch, tokens, heads * dim_head)
    for _ in range(2):
        once()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        once()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return quartiles(ts)[1]


def main():
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    dev = "cuda:0"
    out = {"model": "vit_small()", "batch": batch, "steps_per_plan": steps, "resolution": 224, "both_plans": FLAGS}
    for tag, fam in CASES:
        torch.manual_seed(2333)
        model = W.vit_small().to(dev).eval()
        x = torch.randn(batch, 3, 224, 224, device=dev)
        calibrate(model, fam, x)
        with torch.no_grad():
            plans = {"attention": fuse_inference(model, attention=True, **FLAGS), "flag_off": fuse_inference(model, **FLAGS)}
            logits = {k: p(x) for k, p in plans.items()}
            recs = {k: profile_step(p, x) for k, p in plans.items()}
            torch_us = unfused_attention_us(batch, 6, 64, 197, dev)
            for p in plans.values():                        # warm-up
                timed(p, x, 3)
            ms = {k: [] for k in plans}
            for _ in range(steps):                          # interleaved: A, B, A, B, ...
                for k, p in plans.items():
                    ms[k].append(timed(p, x, 1))
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
            q1, med, q3 = quartiles(v)
            res[k] = {"ms_per_step_median": round(med, 3), "ms_per_step_q1": round(q1, 3), "ms_per_step_q3": round(q3, 3),
                      "ms_per_step_min": round(min(v), 3), "ms_per_step_max": round(max(v), 3), "all_ms": [round(t, 3) for t in v],
                      "int8_layers": rep.layers, "layer_norms": rep.layer_norms, "gelus": rep.gelus, "attentions": rep.attentions,
                      "fp32_outputs": rep.fp32_outputs, "not_eligible": len(rep.skipped)}
        on, off = res["attention"], res["flag_off"]
        res["flag_off_attention"]["share_of_step"] = round(12 * torch_us * 1e-3 / off["ms_per_step_median"], 3)
        spread = off["ms_per_step_q3"] - off["ms_per_step_q1"]
        res["run_to_run_spread_ms"] = round(spread, 3)      # (the interquartile range of the baseline's steps)
        res["speedup_median"] = round(off["ms_per_step_median"] / on["ms_per_step_median"], 3)
        res["flag_on_faster_beyond_spread"] = bool(off["ms_per_step_median"] - on["ms_per_step_median"] > spread)
        res["flag_on_slower_beyond_spread"] = bool(on["ms_per_step_median"] - off["ms_per_step_median"] > spread)
        out[tag] = res
        del model, plans, x, logits
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    with open(os.path.join(ROOT, "profiles", "attention_ab.json"), "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
