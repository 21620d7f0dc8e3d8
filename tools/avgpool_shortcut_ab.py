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
usage: python tools/avgpool_shortcut_ab.py [batch] [rounds]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dlmc-quant_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

import workloads as W  # noqa: E402
from dlmc.utils.fuse import AvgPoolLayer, fuse_inference  # noqa: E402
from dlmc.utils.merge_bn import merge_bn  # noqa: E402
from node_times import calibrated, node_times  # noqa: E402
from relu6_ab import timed  # noqa: E402

CASES = [(f"cifar_resnet{depth}_option_{opt.lower()}_{fam}", depth, opt, fam)
         for depth in (20, 56) for opt in ("C", "D") for fam in ("fsptq_w8a8", "qbase_w8a8")]


def pool_kernel_times(plan, x, reps=20):
    """Per AvgPoolLayer node (node_times): the kernel's time and bytes per second."""
    rows = []
    for name, m, (t,), ms in node_times(plan, x, AvgPoolLayer, reps):
        n, c, h, w = t.shape
        s = m.window
        pix = n * (h // s) * (w // s)
        nbytes = pix * (c * (4 * s * s + 4 * m.want_out) + m.c_pad)
        rows.append({"node": name, "input": [n, c, h, w], "floats_per_input_pixel": int(t.stride(3)), "window": s, "c_pad": m.c_pad,
                     "fp32_written": m.want_out, "us": round(ms * 1e3, 2), "bytes": nbytes, "gb_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1)})
    return rows


def main():
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    dev = "cuda:0"
    out = {"batch": batch, "rounds": rounds, "steps_per_round": 3, "resolution": 32}
    for tag, depth, opt, fam in CASES:
        torch.manual_seed(2333)
        model = merge_bn(W.CifarResNet((depth - 2) // 6, option=opt).to(dev).eval(), inplace=True, allow_missing=True)
        kw = {} if fam.startswith("fsptq") else dict(act_offsets=True)
        x = torch.relu(torch.randn(batch, 3, 32, 32, device=dev))
        calibrated(model, fam, x, zero_qbase=False)
        with torch.no_grad():
            plans = {"avg_pools": fuse_inference(model, avg_pools=True, **kw), "flag_off": fuse_inference(model, **kw)}
            logits = {k: p(x) for k, p in plans.items()}
            kernels = pool_kernel_times(plans["avg_pools"], x)
            for p in plans.values():                        # warm-up
                timed(p, x, 2)
            ms = {k: [] for k in plans}
            for _ in range(rounds):                         # interleaved: A, B, A, B, ...
                for k, p in plans.items():
                    ms[k].append(timed(p, x, 3))
        res = {"logits_equal": bool(torch.equal(logits["avg_pools"], logits["flag_off"])), "pool_kernels": kernels}
        for k, v in ms.items():
            rep = plans[k].fusion_report
            res[k] = {"ms_per_step_median": round(sorted(v)[len(v) // 2], 3), "ms_per_step_min": round(min(v), 3),
                      "ms_per_step_max": round(max(v), 3), "all_ms": [round(t, 3) for t in v], "int8_layers": rep.layers,
                      "avg_pools": rep.avg_pools, "dual": rep.dual, "fp32_outputs": rep.fp32_outputs, "not_eligible": len(rep.skipped)}
        on, off = res["avg_pools"], res["flag_off"]
        spread = max(on["ms_per_step_max"] - on["ms_per_step_min"], off["ms_per_step_max"] - off["ms_per_step_min"])
        res["run_to_run_spread_ms"] = round(spread, 3)
        res["speedup_median"] = round(off["ms_per_step_median"] / on["ms_per_step_median"], 3)
        res["flag_on_slower_beyond_spread"] = bool(on["ms_per_step_median"] - off["ms_per_step_median"] > spread)
        out[tag] = res
        del model, plans, x, logits
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    with open(os.path.join(ROOT, "profiles", "avgpool_shortcut_ab.json"), "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
