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
usage: python tools/squeeze_ab.py [batch] [steps]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dlmc-quant_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import workloads as W  # noqa: E402
from dlmc.quantization.scalar import kernels as K  # noqa: E402
from dlmc.utils.fuse import SqueezeLayer, fuse_inference  # noqa: E402
from dlmc.utils.merge_bn import merge_bn  # noqa: E402
from node_times import calibrated, node_times  # noqa: E402
from relu6_ab import timed  # noqa: E402
from swish_ab import quartiles  # noqa: E402

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
    for name, m, (t,), ms in node_times(plan, x, SqueezeLayer, reps):
        se = model.get_submodule(m.decision.layer1.rsplit(".", 1)[0])
        run = lambda _, se=se, t=t: torch_squeeze(se, t)  # noqa: E731
        timed(run, None, 3)
        rows.append({"node": name, "input": list(t.shape), "hidden": m.r, "node_us": round(ms * 1e3, 2),
                     "torch_ops_us": round(timed(run, None, reps) * 1e3, 2)})
    return rows


def squeeze_launch_us(plan, x):
    """The `squeeze` launches of one step, from the launch profile: microseconds each."""
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        plan(x)
        torch.cuda.synchronize()
        return [round(a.elapsed_time(b) * 1e3, 2) for tag, _, a, b, _ in K.PROFILE.records if tag == "squeeze"]
    finally:
        K.PROFILE.enabled = False
        K.PROFILE.reset()


def main():
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    steps = max(24, int(sys.argv[2])) if len(sys.argv) > 2 else 24
    dev = "cuda:0"
    out = {"batch": batch, "steps_per_plan": steps, "resolution": 224}
    for net, (make, flags) in NETS.items():
        for fam in ("fsptq", "qbase"):
            torch.manual_seed(2333)
            model = merge_bn(make().to(dev).eval(), inplace=True, allow_missing=True)
            x = torch.relu(torch.randn(batch, 3, 224, 224, device=dev))
            calibrated(model, fam, x)
            with torch.no_grad():
                plans = {"squeezes": fuse_inference(model, squeezes=True, **flags), "flag_off": fuse_inference(model, **flags)}
                logits = {k: p(x).float() for k, p in plans.items()}
                nodes = node_rows(model, plans["squeezes"], x)
                launches = squeeze_launch_us(plans["squeezes"], x)
                for p in plans.values():                        # warm-up
                    timed(p, x, 3)
                ms = {k: [] for k in plans}
                for _ in range(steps):                          # interleaved: A, B, A, B, ...
                    for k, p in plans.items():
                        ms[k].append(timed(p, x, 1))
            a, b = logits["squeezes"], logits["flag_off"]
            res = {"logits": a.numel(), "logits_differing": int((a != b).sum()), "max_abs_delta_logit": float((a - b).abs().max()),
                   "largest_logit": float(b.abs().max()), "top1_agreement": float((a.argmax(1) == b.argmax(1)).float().mean()),
                   "squeeze_nodes": nodes, "squeeze_kernel_us_per_launch": launches,
                   "squeeze_kernel_us_median": sorted(launches)[len(launches) // 2] if launches else None,
                   "nodes_total_us": round(sum(r["node_us"] for r in nodes), 1), "torch_ops_total_us": round(sum(r["torch_ops_us"] for r in nodes), 1)}
            for k, v in ms.items():
                rep = plans[k].fusion_report
                q1, med, q3 = quartiles(v)
                res[k] = {"ms_per_step_median": round(med, 3), "ms_per_step_iqr": round(q3 - q1, 3), "ms_per_step_q1": round(q1, 3),
                          "ms_per_step_q3": round(q3, 3), "all_ms": [round(t, 3) for t in v], "int8_layers": rep.layers, "gates": rep.gates,
                          "squeezes": rep.squeezes, "not_eligible": len(rep.skipped)}
            on, off = res["squeezes"], res["flag_off"]
            res["ratio_off_over_on"] = round(off["ms_per_step_median"] / on["ms_per_step_median"], 3)
            res["flag_on_faster_beyond_iqr"] = bool(off["ms_per_step_median"] - on["ms_per_step_median"] > off["ms_per_step_iqr"])
            res["flag_on_slower_beyond_iqr"] = bool(on["ms_per_step_median"] - off["ms_per_step_median"] > off["ms_per_step_iqr"])
            out[f"{net}_{fam}_w8a8"] = res
            del model, plans, x, logits
            torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    with open(os.path.join(ROOT, "profiles", "squeeze_ab.json"), "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
