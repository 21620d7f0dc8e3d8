#!/usr/bin/env python3
"""Attention on the f16 matrix cores (fuse_inference(attention="f16"), csrc/attention_f16.hip) against the fp32 kernel
(attention=True, csrc/attention.hip), three measurements in one process, the fp32 arm measured in the same run on the same build, every
timing interleaved (A, B, A, B, ...), median and interquartile range per arm, the spread = the fp32 arm's interquartile range:
  (i)   the plan: workloads.vit_small(), FSPTQ and QBase W8A8, both arms with layer_norms=True and gelu=True, single steps; the attention
        launches' time, TFLOP/s and bytes per second of one step from the launch profile (K.PROFILE: algorithmic bytes and operations);
  (ii)  the kernel alone: K.attention_quant(operands="f16") against operands="f32" on the three slices of one packed projection, fp32
        out, at B H = 1536, T = 197, D = 64 (ViT-S/16 at batch 256) and at B = 4096, H = 3, T = 49, D = 32 (Swin-T's stage-1 windows);
  (iii) the logits of the f16 plan against the fp32-attention plan and against the attention-off plan: how many differ, the largest
        difference at what largest logit, top-1 agreement.
Writes profiles/attention_f16_compare.json (and prints it).  (Not named *_ab.py: tests/test_plan_ab_host.py pins how many such tools
there are, so its hygiene rules - no imports between tools, shared helpers from plan_ab.py alone - are kept here by hand.)
usage: python tools/attention_f16_compare.py [batch] [steps] [--out PATH]"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import fuse_inference

FLAGS = dict(layer_norms=True, gelu=True)
SHAPES = {"vit_small_b256": (256, 6, 197, 64), "swin_t_stage1_windows": (4096, 3, 49, 32)}      # (B, H, T, D)


def two_arms(arms, steps, reps):
    """{arm: summary} and the verdict of arms "f16" / "f32" = callables of no argument, `steps` timings of `reps` calls each, interleaved."""
    ms = P.interleaved({k: (lambda _, f=f: f()) for k, f in arms.items()}, None, 3, steps, reps)
    res = {k: P.arm_summary(v, P.QUARTILES) for k, v in ms.items()}
    v = P.verdict(res["f16"], res["f32"], "iqr_off")
    res.update(fp32_arm_iqr_ms=v["run_to_run_spread_ms"], speedup_median=v["speedup_median"], f16_faster_beyond_spread=v["flag_on_faster_beyond_spread"])
    return res


def kernel_alone(b, h, t, d, steps):
    p = torch.randn(b, t, 3 * h * d, device=P.DEV).reshape(b, t, 3, h, d).permute(2, 0, 3, 1, 4)
    q, k, v = p[0], p[1], p[2]
    run = {o: (lambda o=o: K.attention_quant(q, k, v, d ** -0.5, operands=o)) for o in ("f16", "f32")}
    res = two_arms(run, steps, 10)
    flop, nbytes = 4 * b * h * t * t * d, 4 * b * h * t * d * 4
    for arm in run:
        s = res[arm]["ms_per_step_median"] * 1e-3
        res[arm].update(tflop_per_s=round(flop / s / 1e12, 2), gb_per_s=round(nbytes / s / 1e9, 1))
    return dict(res, shape=dict(B=b, H=h, T=t, D=d), flop=flop, bytes=nbytes, max_abs_difference=float((run["f16"]()[0] - run["f32"]()[0]).abs().max()))


def against(a, b):
    return dict(logits=a.numel(), logits_that_differ=int((a != b).sum()), max_abs_delta_logit=float((a - b).abs().max()),
                max_abs_logit=float(b.abs().max()), top1_agreement=float((a.argmax(-1) == b.argmax(-1)).float().mean()))


def main():
    arg = P.arguments(__doc__, batch=256, steps=24)
    out = {"model": "vit_small", "batch": arg.batch, "steps_per_arm": arg.steps, "both_plans": FLAGS}
    for tag, fam in P.CASES:
        model = P.seeded_model(W.vit_small, bn=False)
        x = torch.randn(arg.batch, 3, 224, 224, device=P.DEV)
        P.calibrate(model, fam, x)
        with torch.no_grad():
            plans = {"f16": fuse_inference(model, attention="f16", **FLAGS), "f32": fuse_inference(model, attention=True, **FLAGS),
                     "off": fuse_inference(model, **FLAGS)}
            logits = {k: p(x).float() for k, p in plans.items()}
            res = two_arms({k: (lambda p=plans[k]: p(x)) for k in ("f16", "f32")}, arg.steps, 1)
            for arm, name in (("f16", "attention_f16"), ("f32", "attention")):
                mine = [r for r in P.profile_step(plans[arm], x) if r[0] == name]
                t_ms, nbytes, ops = sum(r[2] for r in mine), sum(r[1] for r in mine), sum(r[3] for r in mine)
                res[arm]["kernel"] = {"launches": len(mine), "us": round(t_ms * 1e3, 1), "flop": ops, "bytes": nbytes,
                                      "tflop_per_s": round(ops / (t_ms * 1e-3) / 1e12, 2) if t_ms else None,
                                      "gb_per_s": round(nbytes / (t_ms * 1e-3) / 1e9, 1) if t_ms else None}
        res.update(attentions=plans["f16"].fusion_report.attentions, operands=plans["f16"].fusion_report.attention_operands,
                   against_fp32_attention=against(logits["f16"], logits["f32"]), against_attention_off=against(logits["f16"], logits["off"]))
        out[tag] = res
        del model, plans, x, logits
        torch.cuda.empty_cache()
    out["kernel_alone"] = {name: kernel_alone(*shape, arg.steps) for name, shape in SHAPES.items()}
    P.write_profile("attention_f16_compare", out, arg.out)


if __name__ == "__main__":
    main()
