#!/usr/bin/env python3
"""A Swin stage's row geometry on the plan (fuse_inference(swin_geometry=True), csrc/swin_rows.hip: the LayerNorm that gathers shifted-window
and 2 x 2 merge rows from the token map, the window reverse + roll back + residual add) against the plan that runs the roll, the
partition / reverse copies, the concatenation and the add in torch, both arms on the same build in one process:
  (i)   the plan: workloads.swin() (Swin-B's widths, 224^2 images: 24 blocks on maps of 56 / 28 / 14 / 7 tokens a side, 3 merges), FSPTQ and
        QBase W8A8, both arms with layer_norms=True, gelu=True and window_attention="f16", interleaved single steps (A, B, A, B, ...), median
        and interquartile range per arm, the spread = the flag-off arm's interquartile range; how many logits differ and by how much;
  (ii)  per node kind, on the tensors the step handed the node: the node's launch against the torch ops it replaces (its own restatement:
        LayerNorm, roll, partition copy and the consumer's quantise pass; slices, cat, LayerNorm, quantise; reverse copy, roll, add), summed
        over the step's nodes;
  (iii) the two kernels' algorithmic bytes per second over one step's launches, from the launch profile (K.PROFILE).
Writes profiles/swin_geometry_compare.json (and prints it).  (Not named *_ab.py: tests/test_plan_ab_host.py pins how many such tools there
are, so its hygiene rules - no imports between tools, shared helpers from plan_ab.py alone - are kept here by hand.)
usage: python tools/swin_geometry_compare.py [batch] [steps] [--out PATH]"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import torch.nn.functional as F
import workloads as W
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import MergeNormLayer, WindowAddLayer, WindowNormLayer, fuse_inference

FLAGS = dict(layer_norms=True, gelu=True, window_attention="f16")
CASES = [("swin_fsptq_w8a8", "fsptq"), ("swin_qbase_w8a8", "qbase")]


def restated(m, args):
    """The torch ops node `m` replaces, on its inputs `args`."""
    if isinstance(m, WindowAddLayer):
        yw, x = args
        return K.window_reverse_torch(yw, (x.shape[0], *m.hw, m.c), m.window, m.shift).reshape(x.shape) + x
    n, x = m.norm, args[0]
    if isinstance(m, MergeNormLayer):
        return m._torch_rows(F.layer_norm(K.merge_rows_torch(x), n.normalized_shape, n.weight, n.bias, n.eps))
    v = F.layer_norm(x, n.normalized_shape, n.weight, n.bias, n.eps).view(-1, *m.hw, m.c)
    return m._torch_rows(K.window_rows_torch(v, m.window, m.shift))


def nodes_against_torch(plan, x, cls, reps=10):
    """The step's `cls` nodes, each timed alone on the inputs the step gave it, against `restated`: summed ms of both, and their ratio."""
    rows = P.node_times(plan, x, cls, reps=reps)
    torch_ms = []
    for _, m, a, _ in rows:
        run = lambda _, m=m, a=a: restated(m, a)  # noqa: E731
        P.timed(run, None, 3)
        torch_ms.append(P.timed(run, None, reps))
    node, ops = sum(r[3] for r in rows), sum(torch_ms)
    return {"nodes": len(rows), "node_ms": round(node, 4), "torch_ops_ms": round(ops, 4), "torch_over_node": round(ops / node, 2) if node else None}


def main():
    arg = P.arguments(__doc__, batch=32, steps=24)
    out = {"model": "swin()", "batch": arg.batch, "steps_per_arm": arg.steps, "image": [3, 224, 224], "both_plans": FLAGS}
    for tag, fam in CASES:
        model = P.seeded_model(W.swin, bn=False)
        x = torch.randn(arg.batch, 3, 224, 224, device=P.DEV)
        P.calibrate(model, fam, x)
        with torch.no_grad():
            plans = {"on": fuse_inference(model, swin_geometry=True, **FLAGS), "off": fuse_inference(model, **FLAGS)}
            a, b = (plans[k](x).float() for k in ("on", "off"))
            ms = P.interleaved(plans, x, 3, arg.steps, 1)
            res = {k: P.arm_summary(v, P.QUARTILES, arg.batch) for k, v in ms.items()}
            res.update(P.verdict(res["on"], res["off"], "iqr_off"))
            res["nodes_against_torch_ops"] = {name: nodes_against_torch(plans["on"], x, cls) for name, cls in
                                              (("window_norm", WindowNormLayer), ("merge_norm", MergeNormLayer), ("window_add", WindowAddLayer))}
            recs = P.profile_step(plans["on"], x)
            res["kernels"] = {t: P.launch_sum(recs, t) for t in ("layernorm_gather", "window_reverse_add")}
        rep = plans["on"].fusion_report
        res.update(window_norms=rep.window_norms, merge_norms=rep.merge_norms, window_adds=rep.window_adds,
                   against_flag_off=dict(logits=a.numel(), logits_that_differ=int((a != b).sum()), max_abs_delta_logit=float((a - b).abs().max()),
                                         max_abs_logit=float(b.abs().max()), top1_agreement=float((a.argmax(-1) == b.argmax(-1)).float().mean())))
        out[tag] = res
        del model, plans, x, a, b
        torch.cuda.empty_cache()
    P.write_profile("swin_geometry_compare", out, arg.out)


if __name__ == "__main__":
    main()
