#!/usr/bin/env python3
"""Squeeze paths on the int8 plan (fuse_inference(squeezes=True): the pool kernel hands the first small layer its codes, one launch of
csrc/squeeze_i8.hip takes them to the gate) against the plan that runs the squeeze in torch and fake-quant wrappers - both plans built
from ONE calibrated model and timed interleaved, step by step, in one process.
  cases: workloads.efficientnet_b0() with gates, swish and dw5 on, and workloads.mobilenet_v2(se=True) with gates on, at 224^2, under
         FSPTQ W8A8 (zero points set to exactly 0 after calibration, as the tests do) and QBase W8A8.
Per case: median and interquartile range of the ms per step of either plan over `steps` single steps each (A, B, A, B, ...), whether
the flag-on plan is faster or slower by more than the flag-off plan's interquartile range, how many logits differ between the two plans
and by how much; from the launch profile of one flag-on step the squeeze kernel's time per launch; per squeeze node the node alone (pool
kernel + squeeze kernel) and the torch op sequence it replaces - the model's own squeeze-excite module without its last multiply - both
between two events on the tensor the step hands the node.  Writes profiles/squeeze_ab.json (and prints it).
usage: python tools/squeeze_ab.py [batch] [steps] [--out PATH]"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import torch.nn.functional as F
import workloads as W
from dlmc.utils.fuse import SqueezeLayer, fuse_inference

NETS = {"efficientnet_b0": (W.efficientnet_b0, dict(gates=True, swish=True, dw5=True)),
        "mobilenet_v2_se": (lambda: W.mobilenet_v2(se=True), dict(gates=True))}


def torch_squeeze(se, x):
    """workloads.SqueezeExcite.forward without its last multiply: the ops a SqueezeLayer node replaces."""
    v = se.pool(x)
    if se.squeeze == "linear":
        v = se.reduce(v.view(x.size(0), -1))
        v = se.expand(v * torch.sigmoid(v)).view(x.size(0), x.size(1), 1, 1)
    else:
        v = se.expand(F.relu(se.reduce(v)))
    return torch.sigmoid(v) if se.gate == "sigmoid" else F.relu6(v + 3.) / 6.


def node_rows(model, plan, x, reps=20):
    rows = []
    for name, m, (t,), ms in P.node_times(plan, x, SqueezeLayer, reps):
        se = model.get_submodule(m.decision.layer1.rsplit(".", 1)[0])
        run = lambda _, se=se, t=t: torch_squeeze(se, t)  # noqa: E731
        P.timed(run, None, 3)
        rows.append({"node": name, "input": list(t.shape), "hidden": m.r, "node_us": round(ms * 1e3, 2),
                     "torch_ops_us": round(P.timed(run, None, reps) * 1e3, 2)})
    return rows


def main():
    arg = P.arguments(__doc__, batch=256, steps=24)
    steps = max(24, arg.steps)
    out = {"batch": arg.batch, "steps_per_plan": steps, "resolution": 224}
    for net, (make, flags) in NETS.items():
        for fam in ("fsptq", "qbase"):
            model = P.seeded_model(make)
            x = P.relu_images(arg.batch, 224)
            P.calibrated(model, fam, x)
            with torch.no_grad():
                plans = {"squeezes": fuse_inference(model, squeezes=True, **flags), "flag_off": fuse_inference(model, **flags)}
                logits = {k: p(x).float() for k, p in plans.items()}
                nodes = node_rows(model, plans["squeezes"], x)
                # the `squeeze` launches of one step, from the launch profile: microseconds each
                launches = [round(r[2] * 1e3, 2) for r in P.profile_step(plans["squeezes"], x, warm=False) if r[0] == "squeeze"]
                ms = P.interleaved(plans, x, 3, steps, 1)
            a, b = logits["squeezes"], logits["flag_off"]
            res = {"logits": a.numel(), "logits_differing": int((a != b).sum()), "max_abs_delta_logit": float((a - b).abs().max()),
                   "largest_logit": float(b.abs().max()), "top1_agreement": float((a.argmax(1) == b.argmax(1)).float().mean()),
                   "squeeze_nodes": nodes, "squeeze_kernel_us_per_launch": launches,
                   "squeeze_kernel_us_median": P.quartiles(launches)[1] if launches else None,
                   "nodes_total_us": round(sum(r["node_us"] for r in nodes), 1), "torch_ops_total_us": round(sum(r["torch_ops_us"] for r in nodes), 1)}
            for k, v in ms.items():
                rep = plans[k].fusion_report
                res[k] = dict(P.arm_summary(v, ("median", "iqr", "q1", "q3")), int8_layers=rep.layers, gates=rep.gates, squeezes=rep.squeezes,
                              not_eligible=len(rep.skipped))
            on, off = res["squeezes"], res["flag_off"]
            res["ratio_off_over_on"] = P.speedup_median(on, off)
            res["flag_on_faster_beyond_iqr"] = bool(off["ms_per_step_median"] - on["ms_per_step_median"] > off["ms_per_step_iqr"])
            res["flag_on_slower_beyond_iqr"] = bool(on["ms_per_step_median"] - off["ms_per_step_median"] > off["ms_per_step_iqr"])
            out[f"{net}_{fam}_w8a8"] = res
            del model, plans, x, logits
            torch.cuda.empty_cache()
    P.write_profile("squeeze_ab", out, arg.out)


if __name__ == "__main__":
    main()
