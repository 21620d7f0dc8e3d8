#!/usr/bin/env python3
"""What avgpool_shortcut_ab.py, gate_ab.py and swish_ab.py share: the calibrated W8A8 model and the time of every plan node of one class
alone - its inputs as the plan hands them over, then the node by itself between two events.
As a program: the AvgPoolLayer, GateLayer and SwishLayer nodes of those tools' workloads, each 20 launches between two events after 3
warm-ups, five times: the median, and max - min of the five as the node's run-to-run spread.  It uses no name younger than the three
node classes, so the same file runs in a checkout of an earlier commit for an A/B of the kernels.
usage: python tools/node_times.py out.json [cifar batch] [mobilenet batch]"""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dlmc-quant_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

import workloads as W  # noqa: E402
from act_offset_ab import QBASE_W8A8  # noqa: E402
from dlmc.quantization.scalar.FSPTQuant import FSPTQBase  # noqa: E402
from dlmc.quantization.scalar.modules.base import QBase  # noqa: E402
from dlmc.utils.fuse import AvgPoolLayer, GateLayer, SwishLayer, fuse_inference  # noqa: E402
from dlmc.utils.merge_bn import merge_bn  # noqa: E402
from dlmc.utils.quantize import quantize_model  # noqa: E402
from relu6_ab import QCFG as FSPTQ_W8A8, timed  # noqa: E402


def calibrated(model, fam, x, zero_qbase=True):
    """Quantise `model` W8A8 in place (`fam`: "fsptq..." or "qbase..."), calibrate on x[:64], then set the activation zero points to
    exactly 0, as the tests do (FSPTQ always, QBase with `zero_qbase`)."""
    if fam.startswith("fsptq"):
        quantize_model(model, copy.deepcopy(FSPTQ_W8A8), None, "FSPTQ", int8_gemm=True)
    else:
        quantize_model(model, copy.deepcopy(QBASE_W8A8), None)
    with torch.no_grad():
        model(x[:64])
        for m in model.modules():
            if isinstance(m, FSPTQBase):
                m.in_offset.zero_()
                m._zp_is_int = None
            elif zero_qbase and isinstance(m, QBase) and m.in_offset is not None:
                m.in_offset.zero_()


def node_times(plan, x, cls, reps=20, repeats=1):
    """[(name, module, its positional inputs, ms per launch)] per `cls` node of `plan`: the inputs caught in one run of `plan(x)`, then
    `reps` launches of the node alone between two events after 3 warm-ups (`repeats` > 1: a list of that many such times)."""
    seen, hooks, rows = {}, [], []
    for name, m in plan.named_modules():
        if isinstance(m, cls):
            hooks.append(m.register_forward_pre_hook(lambda mod, a, name=name: seen.__setitem__(name, a)))
    plan(x)
    for h in hooks:
        h.remove()
    mods = dict(plan.named_modules())
    for name, a in seen.items():
        run = lambda _, m=mods[name], a=a: m(*a)  # noqa: E731
        timed(run, None, 3)
        ms = [timed(run, None, reps) for _ in range(repeats)]
        rows.append((name, mods[name], a, ms if repeats > 1 else ms[0]))
    return rows


def main():
    b_cifar, b_mbv2 = (int(sys.argv[i]) if len(sys.argv) > i else d for i, d in ((2, 512), (3, 1024)))
    # (tag, the model, input size, batch, fuse_inference's flags by family) - as the three tools build them
    cases = [(f"cifar_resnet{d}_option_{o.lower()}", lambda d=d, o=o: W.CifarResNet((d - 2) // 6, option=o), 32, b_cifar,
              lambda fam: dict(avg_pools=True, act_offsets=fam == "qbase")) for d in (20, 56) for o in ("C", "D")]
    cases += [("mobilenet_v2_se", lambda: W.mobilenet_v2(se=True), 224, b_mbv2, lambda fam: dict(gates=True)),
              ("mbconv_se", lambda: W.mobilenet_v2(se=True, act="swish"), 224, b_mbv2, lambda fam: dict(gates=True, swish=True))]
    out = {}
    for tag, make, res, batch, flags in cases:
        for fam in ("fsptq", "qbase"):
            torch.manual_seed(2333)
            model = merge_bn(make().to("cuda:0").eval(), inplace=True, allow_missing=True)
            x = torch.relu(torch.randn(batch, 3, res, res, device="cuda:0"))
            calibrated(model, fam, x, zero_qbase="avg_pools" not in flags(fam))
            with torch.no_grad():
                rows = node_times(fuse_inference(model, **flags(fam)), x, (AvgPoolLayer, GateLayer, SwishLayer), 20, repeats=5)
            for name, m, a, ms in rows:
                us = [round(t * 1e3, 2) for t in ms]
                out[f"{tag}_{fam}_w8a8/{name}"] = {"class": type(m).__name__, "input": list(a[0].shape), "us_median": sorted(us)[2],
                                                   "us_spread": round(max(us) - min(us), 2), "us_all": us}
            print(tag, fam, len(rows), "nodes", flush=True)
            del model, rows, x
            torch.cuda.empty_cache()
    with open(sys.argv[1], "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
