#!/usr/bin/env python3
"""The time of every plan node of one class alone (tools/plan_ab.py's node_times: its inputs as the plan hands them over, then the node
by itself between two events), as a program: the AvgPoolLayer, GateLayer and SwishLayer nodes of the workloads of avgpool_shortcut_ab.py,
gate_ab.py and swish_ab.py, each 20 launches between two events after 3 warm-ups, five times: the median, and max - min of the five as
the node's run-to-run spread.
usage: python tools/node_times.py out.json [cifar batch] [mobilenet batch]"""
import sys

import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc.utils.fuse import AvgPoolLayer, GateLayer, SwishLayer, fuse_inference


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
            model = P.seeded_model(make)
            x = P.relu_images(batch, res)
            P.calibrated(model, fam, x, zero_qbase="avg_pools" not in flags(fam))
            with torch.no_grad():
                rows = P.node_times(fuse_inference(model, **flags(fam)), x, (AvgPoolLayer, GateLayer, SwishLayer), 20, repeats=5)
            for name, m, a, ms in rows:
                us = [round(t * 1e3, 2) for t in ms]
                out[f"{tag}_{fam}_w8a8/{name}"] = {"class": type(m).__name__, "input": list(a[0].shape), "us_median": P.quartiles(us)[1],
                                                   "us_spread": round(max(us) - min(us), 2), "us_all": us}
            print(tag, fam, len(rows), "nodes", flush=True)
            del model, rows, x
            torch.cuda.empty_cache()
    P.write_profile(None, out, sys.argv[1], quiet=True)


if __name__ == "__main__":
    main()
