#!/usr/bin/env python3
"""Window attention on the f16 matrix cores (fuse_inference(window_attention="f16"), csrc/window_attention_f16.hip) against the fp32
window kernel (window_attention=True, csrc/window_attention.hip), three comparisons in one process, both arms on the same build, every
timing interleaved (A, B, A, B, ...), median and interquartile range per arm, the spread = the fp32 arm's interquartile range:
  (i)   the plan: workloads.window_vit(grid=8) (a 56^2 map of 128 channels: 64 windows of T = 49 per image, 4 heads of 32, 4 blocks, every
        second one masked), FSPTQ and QBase W8A8, both arms with layer_norms=True and gelu=True, single steps; the window attention
        launches' time, TFLOP/s and bytes per second of one step from the launch profile (K.PROFILE: algorithmic bytes and operations);
        the logits of the f16 plan against the fp32 arm's: how many differ, the largest difference at what largest logit, top-1 agreement;
  (ii)  the kernel alone: K.window_attention_quant(operands="f16") against operands="f32" on the three slices of one packed projection,
        fp32 out, with no term, with bias, and with bias and mask (both padded views read in place), at B = 4096, H = 3, T = 49, D = 32
        (Swin-T's stage-1 windows) and at B = 2048, H = 4, T = 64, D = 64; the largest output difference;
  (iii) against the streaming kernel on the same instruction: no term, the first shape, K.attention_quant(operands="f16") as the other arm.
Writes profiles/window_attention_f16_compare.json (and prints it).  (Not named *_ab.py: tests/test_plan_ab_host.py pins how many such
tools there are, so its hygiene rules - no imports between tools, shared helpers from plan_ab.py alone - are kept here by hand.)
usage: python tools/window_attention_f16_compare.py [batch] [steps] [--out PATH]"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import fuse_inference

FLAGS = dict(layer_norms=True, gelu=True)
CASES = [("window_vit_fsptq_w8a8", "fsptq"), ("window_vit_qbase_w8a8", "qbase")]
SHAPES = {"swin_t_stage1_windows": (4096, 3, 49, 32, 64), "t64_d64": (2048, 4, 64, 64, 64)}      # (B, H, T, D, nW)


def two_arms(arms, steps, reps, other="f32"):
    """{arm: summary} and the verdict of arm "f16" against arm `other`: `steps` timings of `reps` calls each, interleaved."""
    ms = P.interleaved({k: (lambda _, f=f: f()) for k, f in arms.items()}, None, 3, steps, reps)
    res = {k: P.arm_summary(v, P.QUARTILES) for k, v in ms.items()}
    v = P.verdict(res["f16"], res[other], "iqr_off")
    res.update({f"{other}_arm_iqr_ms": v["run_to_run_spread_ms"], "speedup_median": v["speedup_median"],
                "f16_faster_beyond_spread": v["flag_on_faster_beyond_spread"], "f16_slower_beyond_spread": v["flag_on_slower_beyond_spread"]})
    return res


def kernel_alone(b, h, t, d, nw, steps, streaming):
    p = torch.randn(b, t, 3 * h * d, device=P.DEV).reshape(b, t, 3, h, d).permute(2, 0, 3, 1, 4)
    q, k, v = p[0], p[1], p[2]
    pad = (t + 3) // 4 * 4
    bias = torch.randn(h, t, pad, device=P.DEV)[:, :, :t]
    mask = torch.where(torch.rand(nw, t, pad, device=P.DEV) < 0.4, -100.0, 0.0)[:, :, :t]
    out = {"shape": dict(B=b, H=h, T=t, D=d, nW=nw), "flop": 4 * b * h * t * t * d, "bytes": 4 * b * h * t * d * 4}
    for name, kw in (("no_term", {}), ("bias", dict(bias=bias)), ("bias_and_mask", dict(bias=bias, mask=mask))):
        run = {o: (lambda o=o, kw=kw: K.window_attention_quant(q, k, v, d ** -0.5, operands=o, **kw)) for o in ("f16", "f32")}
        res = two_arms(run, steps, 10)
        for arm in run:
            s = res[arm]["ms_per_step_median"] * 1e-3
            res[arm].update(tflop_per_s=round(out["flop"] / s / 1e12, 2), gb_per_s=round(out["bytes"] / s / 1e9, 1))
        out[name] = dict(res, max_abs_difference=float((run["f16"]()[0] - run["f32"]()[0]).abs().max()))
    if streaming:      # (iii): the window split against the streaming split, both on v_mfma_f32_32x32x16_f16
        run = {"f16": lambda: K.window_attention_quant(q, k, v, d ** -0.5, operands="f16"),
               "streaming_f16": lambda: K.attention_quant(q, k, v, d ** -0.5, operands="f16")}
        out["against_attention_f16"] = dict(two_arms(run, steps, 10, other="streaming_f16"),
                                            max_abs_difference=float((run["f16"]()[0] - run["streaming_f16"]()[0]).abs().max()))
    return out


def main():
    arg = P.arguments(__doc__, batch=32, steps=24)
    out = {"model": "window_vit(grid=8)", "batch": arg.batch, "steps_per_arm": arg.steps, "map": [128, 56, 56], "both_plans": FLAGS}
    for tag, fam in CASES:
        model = P.seeded_model(lambda: W.window_vit(grid=8), bn=False)
        x = torch.randn(arg.batch, 128, 56, 56, device=P.DEV)
        P.calibrate(model, fam, x)
        with torch.no_grad():
            plans = {"f16": fuse_inference(model, window_attention="f16", **FLAGS), "f32": fuse_inference(model, window_attention=True, **FLAGS)}
            a, b = (plans[k](x).float() for k in ("f16", "f32"))
            res = two_arms({k: (lambda p=p: p(x)) for k, p in plans.items()}, arg.steps, 1)
            for arm, name in (("f16", "window_attention_f16"), ("f32", "window_attention")):
                mine = [r for r in P.profile_step(plans[arm], x) if r[0] == name]
                t_ms, nbytes, ops = sum(r[2] for r in mine), sum(r[1] for r in mine), sum(r[3] for r in mine)
                res[arm]["kernel"] = {"launches": len(mine), "us": round(t_ms * 1e3, 1), "flop": ops, "bytes": nbytes,
                                      "tflop_per_s": round(ops / (t_ms * 1e-3) / 1e12, 2) if t_ms else None,
                                      "gb_per_s": round(nbytes / (t_ms * 1e-3) / 1e9, 1) if t_ms else None}
        res.update(window_attentions=plans["f16"].fusion_report.window_attentions, operands=plans["f16"].fusion_report.window_attention_operands,
                   against_fp32_window_attention=dict(logits=a.numel(), logits_that_differ=int((a != b).sum()),
                                                      max_abs_delta_logit=float((a - b).abs().max()), max_abs_logit=float(b.abs().max()),
                                                      top1_agreement=float((a.argmax(-1) == b.argmax(-1)).float().mean())))
        out[tag] = res
        del model, plans, x, a, b
        torch.cuda.empty_cache()
    out["kernel_alone"] = {name: kernel_alone(*shape, arg.steps, streaming=name == "swin_t_stage1_windows") for name, shape in SHAPES.items()}
    P.write_profile("window_attention_f16_compare", out, arg.out)


if __name__ == "__main__":
    main()
