#!/usr/bin/env python3
"""Window attention past 64 tokens on the int8 plan (fuse_inference(window_attention=True) where a window has 65 .. 256 tokens: every
`softmax(q k^T * c + bias + mask) v` + merge-heads tail one launch of csrc/window_attention_stream.hip that hands `to_out` its activation
codes), three comparisons in one process, each interleaved (A, B, A, B, ...), median and interquartile range:
  (i)   the plan: workloads.window_vit(window=12, grid=4) (a 48^2 map of 128 channels: 16 windows of T = 144 per image, 4 heads of 32, 4
        blocks, every second one masked) and the same with window=16 (T = 256, a 64^2 map), FSPTQ W8A8, flag on against flag off, both
        with layer_norms=True and gelu=True; the spread is the flag-off arm's interquartile range; how many logits differ; the kernel's
        launches, TFLOP/s and bytes per second from the launch profile of one step (K.PROFILE: algorithmic bytes and operations);
  (ii)  the kernel against torch: every WindowAttentionLayer node of the step alone on the tensors the step handed it - the launch (the
        terms' padded copies included) against the node's torch restatement (the graph's own ops and `to_out`'s quantise pass).  This is
        the comparison that decides the route: the kernel's median has to beat the torch arm's by more than the torch arm's
        interquartile range at T = 144 and at T = 256;
  (iii) the kernel against the existing streaming one: dlmcq_window_attention_stream_f32 with bias = mask = NULL against
        dlmcq_attention_f32 on the same packed q / k / v at T = 144, D = 32 (4 heads, 16 windows per image), fp32 out; the largest
        difference between the two outputs is reported.  Information, not a gate.
Writes profiles/window_attention_stream.json (and prints it).  (Not named *_ab.py: tests/test_plan_ab_host.py pins how many such tools
there are, so its hygiene checks - no imports between tools, shared helpers defined in plan_ab.py alone - are kept here by hand.)
usage: python tools/window_attention_stream_compare.py [batch] [steps] [--out PATH]"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import WindowAttentionLayer, fuse_inference

FLAGS = dict(layer_norms=True, gelu=True)
TAG = "window_attention_stream"


def two_arms(arms, steps, reps):
    """{arm: summary} and the verdict of arms "on" / "off" = callables of no argument, `steps` timings of `reps` calls each, interleaved."""
    ms = P.interleaved({k: (lambda _, f=f: f()) for k, f in arms.items()}, None, 3, steps, reps)
    res = {k: P.arm_summary(v, P.QUARTILES) for k, v in ms.items()}
    res.update(P.verdict(res["on"], res["off"], "iqr_off"))
    return res


def kernels_alone(images, steps):
    b, h, t, d = images * 16, 4, 144, 32
    p = torch.randn(b, t, 3 * h * d, device=P.DEV).reshape(b, t, 3, h, d).permute(2, 0, 3, 1, 4)
    q, k, v = p[0], p[1], p[2]
    new, old = K.window_attention_quant(q, k, v, d ** -0.5)[0], K.attention_quant(q, k, v, d ** -0.5)[0]
    res = two_arms({"on": lambda: K.window_attention_quant(q, k, v, d ** -0.5), "off": lambda: K.attention_quant(q, k, v, d ** -0.5)}, steps, 10)
    flop, nbytes = 4 * b * h * t * t * d, 4 * b * h * t * d * 4
    for arm in ("on", "off"):
        s = res[arm]["ms_per_step_median"] * 1e-3
        res[arm].update(tflop_per_s=round(flop / s / 1e12, 2), gb_per_s=round(nbytes / s / 1e9, 1))
    return dict(res, shape=dict(B=b, H=h, T=t, D=d), arms=dict(on="dlmcq_window_attention_stream_f32, bias = mask = NULL", off="dlmcq_attention_f32"),
                max_abs_difference=float((new - old).abs().max()))


def plan_case(window, batch, steps):
    model = P.seeded_model(lambda: W.window_vit(window=window, grid=4), bn=False)
    x = torch.randn(batch, 128, 4 * window, 4 * window, device=P.DEV)
    P.calibrate(model, "fsptq", x)
    with torch.no_grad():
        plans = {"on": fuse_inference(model, window_attention=True, **FLAGS), "off": fuse_inference(model, **FLAGS)}
        logits = {k: p(x).float() for k, p in plans.items()}
        recs = P.profile_step(plans["on"], x)
        res = two_arms({k: (lambda p=p: p(x)) for k, p in plans.items()}, steps, 1)
        nodes = {}
        for name, m, a, _ in P.node_times(plans["on"], x, WindowAttentionLayer, reps=1):
            at = 3 + m.has_bias      # (behind q, k, v: the bias, then the mask and the graph's nW, then the reshape's sizes)
            bias, (mask, windows) = (a[3] if m.has_bias else None), (a[at:at + 2] if m.has_mask else (None, None))
            off = lambda m=m, a=a, r=(bias, mask, windows, a[at + 2 * m.has_mask:]): m._torch(*a[:3], *r)  # noqa: E731
            nodes[name] = dict(two_arms({"on": lambda m=m, a=a: m(*a), "off": off}, steps, 5), terms=m.has_bias + m.has_mask,
                               q_shape=list(a[0].shape))
    mine = [r for r in recs if r[0] == TAG]
    t_ms, nbytes, ops = sum(r[2] for r in mine), sum(r[1] for r in mine), sum(r[3] for r in mine)
    a, b = logits["on"], logits["off"]
    res.update(model=f"window_vit(window={window}, grid=4)", tokens=window * window, map=[128, 4 * window, 4 * window], logits=a.numel(),
               logits_that_differ=int((a != b).sum()), max_abs_delta_logit=float((a - b).abs().max()), max_abs_logit=float(b.abs().max()),
               window_attentions=plans["on"].fusion_report.window_attentions,
               kernel={"launches": len(mine), "us": round(t_ms * 1e3, 1), "flop": ops, "bytes": nbytes,
                       "tflop_per_s": round(ops / (t_ms * 1e-3) / 1e12, 2) if t_ms else None,
                       "gb_per_s": round(nbytes / (t_ms * 1e-3) / 1e9, 1) if t_ms else None},
               nodes_against_torch=nodes,
               kernel_kept=bool(nodes) and all(n["flag_on_faster_beyond_spread"] for n in nodes.values()))
    return res


def main():
    arg = P.arguments(__doc__, batch=32, steps=24)
    out = {"batch": arg.batch, "steps_per_arm": arg.steps, "both_plans": FLAGS, "quantiser": "fsptq_w8a8"}
    for window in (12, 16):
        out[f"window_vit_t{window * window}"] = plan_case(window, arg.batch, arg.steps)
        torch.cuda.empty_cache()
    out["kernel_against_attention_kernel"] = kernels_alone(arg.batch, arg.steps)
    P.write_profile(TAG, out, arg.out)


if __name__ == "__main__":
    main()
