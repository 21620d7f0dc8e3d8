#!/usr/bin/env python3
"""Average-pooled shortcuts on the int8 plan (fuse_inference(avg_pools=True): the `nn.AvgPool2d(2, 2)` in front of every transition
block's shortcut convolution handing that convolution its activation codes - csrc/avgpool.hip - instead of an fp32 tensor it quantises
itself) against the plan without `avg_pools`: both plans built from ONE calibrated model and timed interleaved in one process.
  cases: the CIFAR ResNet-20 and ResNet-56 with option-C and option-D shortcuts (workloads.CifarResNet(3, option="C")), FSPTQ W8A8 (zero
         points set to exactly 0 after calibration, as the tests do: every tensor is a ReLU output or an average of ReLU outputs) and
         QBase W8A8 (act_offsets=True in both plans: a pooled map's minimum is rarely exactly 0), 32^2.
Per case: median / min / max ms per step of either plan, whether the flag-on plan is slower by more than the run-to-run spread, whether
the logits are equal, and per pool node the kernel's time and achieved bytes per second (bytes per output pixel and channel: 4 s^2 read,
4 written if the fp32 tensor is wanted, 1 written per padded code).  Writes profiles/avgpool_shortcut_ab.json (and prints it).
usage: python tools/avgpool_shortcut_ab.py [batch] [rounds] [--out PATH]"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc.utils.fuse import AvgPoolLayer, fuse_inference

CASES = [(f"cifar_resnet{depth}_option_{opt.lower()}_{fam}", depth, opt, fam)
         for depth in (20, 56) for opt in ("C", "D") for fam in ("fsptq_w8a8", "qbase_w8a8")]


def pool_kernel_times(plan, x, reps=20):
    """Per AvgPoolLayer node (node_times): the kernel's time and bytes per second."""
    rows = []
    for name, m, (t,), ms in P.node_times(plan, x, AvgPoolLayer, reps):
        n, c, h, w = t.shape
        s = m.window
        pix = n * (h // s) * (w // s)
        nbytes = pix * (c * (4 * s * s + 4 * m.want_out) + m.c_pad)
        rows.append({"node": name, "input": [n, c, h, w], "floats_per_input_pixel": int(t.stride(3)), "window": s, "c_pad": m.c_pad,
                     "fp32_written": m.want_out, "us": round(ms * 1e3, 2), "bytes": nbytes, "gb_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1)})
    return rows


def main():
    a = P.arguments(__doc__, batch=512, rounds=7)
    out = {"batch": a.batch, "rounds": a.rounds, "steps_per_round": 3, "resolution": 32}
    for tag, depth, opt, fam in CASES:
        model = P.seeded_model(lambda: W.CifarResNet((depth - 2) // 6, option=opt))
        kw = {} if fam.startswith("fsptq") else dict(act_offsets=True)
        x = P.relu_images(a.batch, 32)
        P.calibrated(model, fam, x, zero_qbase=False)
        with torch.no_grad():
            plans = {"avg_pools": fuse_inference(model, avg_pools=True, **kw), "flag_off": fuse_inference(model, **kw)}
            logits = {k: p(x) for k, p in plans.items()}
            kernels = pool_kernel_times(plans["avg_pools"], x)
            ms = P.interleaved(plans, x, 2, a.rounds, 3)
        res = {"logits_equal": bool(torch.equal(logits["avg_pools"], logits["flag_off"])), "pool_kernels": kernels}
        for k, v in ms.items():
            rep = plans[k].fusion_report
            res[k] = dict(P.arm_summary(v), int8_layers=rep.layers, avg_pools=rep.avg_pools, dual=rep.dual, fp32_outputs=rep.fp32_outputs,
                          not_eligible=len(rep.skipped))
        res.update(P.verdict(res["avg_pools"], res["flag_off"], "range", ("slower",)))
        out[tag] = res
        del model, plans, x, logits
        torch.cuda.empty_cache()
    P.write_profile("avgpool_shortcut_ab", out, a.out)


if __name__ == "__main__":
    main()
