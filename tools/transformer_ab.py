#!/usr/bin/env python3
"""LayerNorm and GELU nodes on the int8 plan (fuse_inference(layer_norms=True, gelu=True): every `LayerNorm -> Linear` one launch of
csrc/layernorm.hip and every `GELU -> Linear` one launch of csrc/gelu.hip, each handing the Linear layer behind it its activation codes)
against the plan that runs torch's LayerNorm and GELU and lets the consumer quantise: both plans built from ONE calibrated model and timed
interleaved, step by step, in one process.
  cases: workloads.vit_small() (ViT-S/16: 25 LayerNorms, 12 GELUs, 50 Linear layers) at 224^2, FSPTQ W8A8 (the calibrated zero points
         rounded to integers) and QBase W8A8 (float offsets set to 0).  Attention's products and softmax run in torch in both plans.
Per case: median ms per step of either plan over `steps` single steps each (A, B, A, B, ...), the run-to-run spread = the interquartile
range of the flag-off plan's steps, whether the flag-on plan is faster by more than that, how many logits differ between the two plans and
by how much, and per kernel - from the launch profile's records of one step (K.PROFILE: algorithmic bytes, event times) - launches, time,
bytes per second and elements per second.  Writes profiles/transformer_ab.json (and prints it).
usage: python tools/transformer_ab.py [batch] [steps]"""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dlmc-quant_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

import workloads as W  # noqa: E402
from act_offset_ab import QBASE_W8A8  # noqa: E402
from dlmc.quantization.scalar import kernels as K  # noqa: E402
from dlmc.quantization.scalar.FSPTQuant import FSPTQBase  # noqa: E402
from dlmc.quantization.scalar.modules.base import QBase  # noqa: E402
from dlmc.utils.fuse import GeluLayer, LayerNormLayer, fuse_inference  # noqa: E402
from dlmc.utils.quantize import quantize_model  # noqa: E402
from relu6_ab import QCFG as FSPTQ_W8A8, timed  # noqa: E402
from swish_ab import quartiles  # noqa: E402

CASES = [("vit_small_fsptq_w8a8", "fsptq"), ("vit_small_qbase_w8a8", "qbase")]
TAGS = {"layernorm": LayerNormLayer, "gelu": GeluLayer}


def calibrate(model, fam, x):
    if fam == "fsptq":
        quantize_model(model, copy.deepcopy(FSPTQ_W8A8), None, "FSPTQ", int8_gemm=True)
    else:
        quantize_model(model, copy.deepcopy(QBASE_W8A8), None)
    with torch.no_grad():
        model(x[:32])
        for m in model.modules():
            if isinstance(m, FSPTQBase):
                m.in_offset.round_().clamp_(m.in_min_val, m.in_max_val)
                m._zp_is_int = None
            elif isinstance(m, QBase) and m.in_offset is not None:
                m.in_offset.zero_()


def kernel_rates(plan, x):
    """Per kernel tag: launches, elements (the nodes' inputs), and the profile records' bytes and event times of one step."""
    elems = {t: 0 for t in TAGS}
    hooks = [m.register_forward_pre_hook(lambda mod, a, t=t: elems.__setitem__(t, elems[t] + a[0].numel()))
             for m in plan.modules() for t, cls in TAGS.items() if isinstance(m, cls)]
    plan(x)                                             # (warm)
    for t in elems:
        elems[t] = 0
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        plan(x)
        torch.cuda.synchronize()
        recs = list(K.PROFILE.records)
    finally:
        K.PROFILE.enabled = False
        K.PROFILE.reset()
        for h in hooks:
            h.remove()
    out = {}
    for t in TAGS:
        mine = [(r[1], r[2].elapsed_time(r[3])) for r in recs if r[0] == t]
        nbytes, ms = sum(b for b, _ in mine), sum(m for _, m in mine)
        out[t] = {"launches": len(mine), "us": round(ms * 1e3, 1), "bytes": nbytes, "elements": elems[t],
                  "gb_per_s": round(nbytes / (ms * 1e-3) / 1e9, 1) if ms else None,
                  "gelem_per_s": round(elems[t] / (ms * 1e-3) / 1e9, 1) if ms else None}
    return out


def main():
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    dev = "cuda:0"
    out = {"model": "vit_small()", "batch": batch, "steps_per_plan": steps, "resolution": 224}
    for tag, fam in CASES:
        torch.manual_seed(2333)
        model = W.vit_small().to(dev).eval()
        x = torch.randn(batch, 3, 224, 224, device=dev)
        calibrate(model, fam, x)
        with torch.no_grad():
            plans = {"nodes": fuse_inference(model, layer_norms=True, gelu=True), "flag_off": fuse_inference(model)}
            logits = {k: p(x) for k, p in plans.items()}
            kernels = kernel_rates(plans["nodes"], x)
            for p in plans.values():                        # warm-up
                timed(p, x, 3)
            ms = {k: [] for k in plans}
            for _ in range(steps):                          # interleaved: A, B, A, B, ...
                for k, p in plans.items():
                    ms[k].append(timed(p, x, 1))
        a, b = logits["nodes"].float(), logits["flag_off"].float()
        res = {"logits_equal": bool(torch.equal(a, b)), "logits": a.numel(), "logits_that_differ": int((a != b).sum()),
               "max_abs_delta_logit": float((a - b).abs().max()), "max_abs_logit": float(b.abs().max()),
               "top1_agreement": float((a.argmax(1) == b.argmax(1)).float().mean()), "kernels": kernels}
        for k, v in ms.items():
            rep = plans[k].fusion_report
            q1, med, q3 = quartiles(v)
            res[k] = {"ms_per_step_median": round(med, 3), "ms_per_step_q1": round(q1, 3), "ms_per_step_q3": round(q3, 3),
                      "ms_per_step_min": round(min(v), 3), "ms_per_step_max": round(max(v), 3), "all_ms": [round(t, 3) for t in v],
                      "int8_layers": rep.layers, "layer_norms": rep.layer_norms, "gelus": rep.gelus, "fp32_outputs": rep.fp32_outputs,
                      "not_eligible": len(rep.skipped)}
        on, off = res["nodes"], res["flag_off"]
        spread = off["ms_per_step_q3"] - off["ms_per_step_q1"]
        res["run_to_run_spread_ms"] = round(spread, 3)      # (the interquartile range of the baseline's steps)
        res["speedup_median"] = round(off["ms_per_step_median"] / on["ms_per_step_median"], 3)
        res["flag_on_faster_beyond_spread"] = bool(off["ms_per_step_median"] - on["ms_per_step_median"] > spread)
        res["flag_on_slower_beyond_spread"] = bool(on["ms_per_step_median"] - off["ms_per_step_median"] > spread)
        out[tag] = res
        del model, plans, x, logits
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    with open(os.path.join(ROOT, "profiles", "transformer_ab.json"), "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
