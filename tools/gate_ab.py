#!/usr/bin/env python3
"""Squeeze-excite gates on the int8 plan (fuse_inference(gates=True): the `x * gate` between every block's depthwise and projection
layer handing the projection its activation codes - csrc/gate.hip - instead of an fp32 tensor the projection quantises itself) against
the plan without `gates`: both plans built from ONE calibrated model and timed interleaved in one process.
  cases: MobileNetV2-SE (workloads.mobilenet_v2(se=True): 17 gates) at 224^2, FSPTQ W8A8 (zero points set to exactly 0 after
         calibration, as the tests do: every tensor a planned layer reads is a ReLU / ReLU6 output, a gated one or their pool) and
         QBase W8A8.
Per case: median / min / max ms per step of either plan, whether the flag-on plan is slower by more than the run-to-run spread, whether
the logits are equal, and per gate node the kernel's time and achieved bytes per second (per pixel: 4 C read, 4 C written if the fp32
tensor is wanted, c_pad code bytes written; the N x C gate once).  Writes profiles/gate_ab.json (and prints it).
usage: python tools/gate_ab.py [batch] [rounds] [--out PATH]"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc.utils.fuse import GateLayer, fuse_inference

CASES = [("mobilenet_v2_se_fsptq_w8a8", "fsptq"), ("mobilenet_v2_se_qbase_w8a8", "qbase")]


def gate_kernel_times(plan, x, reps=20):
    """Per GateLayer node (node_times): the kernel's time and bytes per second."""
    rows = []
    for name, m, (t, g), ms in P.node_times(plan, x, GateLayer, reps):
        n, c, h, w = t.shape
        nbytes = n * h * w * (c * (4 + 4 * m.want_out) + m.c_pad) + n * c * 4
        rows.append({"node": name, "input": [n, c, h, w], "floats_per_input_pixel": int(t.stride(3)), "c_pad": m.c_pad, "act": m.act,
                     "fp32_written": m.want_out, "us": round(ms * 1e3, 2), "bytes": nbytes, "gb_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1)})
    return rows


def main():
    a = P.arguments(__doc__, batch=1024, rounds=7)
    out = {"model": "mobilenet_v2(se=True)", "batch": a.batch, "rounds": a.rounds, "steps_per_round": 3, "resolution": 224}
    for tag, fam in CASES:
        model = P.seeded_model(lambda: W.mobilenet_v2(se=True))
        x = P.relu_images(a.batch, 224)
        P.calibrated(model, fam, x)
        with torch.no_grad():
            plans = {"gates": fuse_inference(model, gates=True), "flag_off": fuse_inference(model)}
            logits = {k: p(x) for k, p in plans.items()}
            kernels = gate_kernel_times(plans["gates"], x)
            ms = P.interleaved(plans, x, 2, a.rounds, 3)
        total = sum(r["bytes"] for r in kernels)
        us = sum(r["us"] for r in kernels)
        res = {"logits_equal": bool(torch.equal(logits["gates"], logits["flag_off"])), "gate_kernels": kernels,
               "gate_kernels_total": {"us": round(us, 1), "bytes": total, "gb_per_s": round(total / (us * 1e-6) / 1e9, 1)}}
        for k, v in ms.items():
            rep = plans[k].fusion_report
            res[k] = dict(P.arm_summary(v), int8_layers=rep.layers, gates=rep.gates, fp32_outputs=rep.fp32_outputs, not_eligible=len(rep.skipped))
        res.update(P.verdict(res["gates"], res["flag_off"], "range", ("slower",)))
        out[tag] = res
        del model, plans, x, logits
        torch.cuda.empty_cache()
    P.write_profile("gate_ab", out, a.out)


if __name__ == "__main__":
    main()
