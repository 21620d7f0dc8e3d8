#!/usr/bin/env python3
"""A/B of the one-launch weight fake-quant (csrc/fake_quant_multi.hip) against the per-layer launches, in ONE process:

  * stand-alone: the weight tensors of a model (default ResNet-50's 54) as one launch per tensor against one `fq_multi`
    launch, and the same for the backward (per tensor: fq_bwd + finalize; batched: fq_multi_bwd + finalize) - HIP events
    around a loop of launches after a warm-up, GB/s against the 8 TB/s roofline (8 B per element forward, 12 backward);
  * QAT step (forward + backward + SGD, tools/qat_step.py's loop) of the QBase and FSPTQ families with and without
    WeightQuantBatch, the two alternated `--rounds` times on the same model and data.

    python tools/fq_multi_ab.py [--steps resnet18:256,resnet50:128] [--rounds 3] [--json profiles/fq_multi_ab.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dlmc-quant_amd")]
import torch  # noqa: E402

import workloads as W  # noqa: E402
from dlmc import _native as N  # noqa: E402
from dlmc.quantization.scalar import kernels as K  # noqa: E402
from dlmc.utils.quantize import WeightQuantBatch, quantize_model  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", default="resnet18:256,resnet50:128")
ap.add_argument("--standalone", default="resnet50")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--json", default=None)
args = ap.parse_args()
dev = "cuda:0"


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def standalone(name):
    torch.manual_seed(2333)
    net = W.MODELS[name]()
    ws = [m.weight.detach().to(dev) for m in net.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear))]
    segs, gys = [], []
    for w in ws:      # FSPTQ's weight quantiser: per output channel, symmetric, 4 bit
        scale = (w.abs().amax(dim=tuple(range(1, w.dim())), keepdim=True) / 7 + 1e-6).contiguous()
        segs.append(K.Segment(w, scale, None, -8, 7, N.FORM_SYMMETRIC))
        gys.append(torch.randn_like(w))
    n = sum(w.numel() for w in ws)
    plan = K.FqMultiPlan(segs)

    def each_fwd():
        for s in segs:
            K.fake_quant(s.x, s.scale, None, s.lo, s.hi, s.form)

    def each_bwd():
        for s, g in zip(segs, gys):
            K.fake_quant_backward(s.x, g, s.scale, None, s.lo, s.hi, 0.0, form=s.form)
    rec = {"model": name, "tensors": len(ws), "elements": n}
    for what, fn, nbytes, launches in (("fwd_per_tensor", each_fwd, 8 * n, len(ws)), ("fwd_fq_multi", plan.forward, 8 * n, 1),
                                       ("bwd_per_tensor", each_bwd, 12 * n, 2 * len(ws)),
                                       ("bwd_fq_multi", lambda: plan.backward(gys), 12 * n, 2)):
        ms = min(timed(fn, 20) for _ in range(3))
        rec[what] = {"ms": round(ms, 4), "launches": launches, "GBps": round(nbytes / ms / 1e6, 1),
                     "frac_of_8TBps": round(nbytes / ms / 1e6 / 8000, 4)}
        print(f"{name} {what:16s} {ms:8.4f} ms  {nbytes / ms / 1e6:8.1f} GB/s  x{launches}", flush=True)
    return rec


def qat(name, batch):
    out = {}
    for family, qtype, wtype, asigned in (("QBase", None, "minmax_tensor", True), ("FSPTQ", "FSPTQ", "minmax_channel", False)):
        torch.manual_seed(2333)
        net = W.MODELS[name]().to(dev).train()
        cfg = {"weight": {"enable": True, "type": wtype, "args": {"n_bits": 4, "signed": True}},
               "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 4, "signed": asigned}},
               "momentum": 0.1, "exclude_layers": [], "override_options": []}
        quantize_model(net, cfg, None, qtype)
        opt = torch.optim.SGD(net.parameters(), lr=1e-4)
        x = torch.randn(batch, 3, 224, 224, device=dev)
        y = torch.randint(0, 1000, (batch,), device=dev)
        with torch.no_grad():
            net(x)
        wqb = WeightQuantBatch(net)

        def step(batched):
            opt.zero_grad(set_to_none=True)
            if batched:
                with wqb.step():
                    loss = torch.nn.functional.cross_entropy(net(x), y)
            else:
                loss = torch.nn.functional.cross_entropy(net(x), y)
            loss.backward()
            opt.step()
        runs = {"per_layer": [], "batched": []}
        for _ in range(args.rounds):
            for key, flag in (("per_layer", False), ("batched", True)):
                runs[key].append(round(timed(lambda: step(flag), args.iters, warm=3), 3))
        K.PROFILE.reset()
        K.PROFILE.enabled = True
        step(True)
        torch.cuda.synchronize()
        K.PROFILE.enabled = False
        kern = {}
        for tag, nbytes, e0, e1, _ in K.PROFILE.records:
            if tag.startswith("fq_multi"):
                ms = e0.elapsed_time(e1)
                kern[tag] = {"ms": round(ms, 4), "GBps": round(nbytes / ms / 1e6, 1), "frac_of_8TBps": round(nbytes / ms / 1e6 / 8000, 4)}
        K.PROFILE.reset()
        out[family] = {"ms_per_step": runs, "median_per_layer": sorted(runs["per_layer"])[len(runs["per_layer"]) // 2],
                       "median_batched": sorted(runs["batched"])[len(runs["batched"]) // 2], "members": len(wqb.members),
                       "skipped": len(wqb.skipped), "in_step_events": kern}
        print(f"{name} b{batch} {family:6s} per-layer {runs['per_layer']}  batched {runs['batched']} ms/step  {kern}", flush=True)
    return out


record = {"what": "one-launch weight fake-quant (fq_multi) against per-layer launches, same process; W4A4, synthetic 224^2 batch",
          "device": torch.cuda.get_device_name(0), "standalone": standalone(args.standalone), "qat_step": {}}
for item in [s for s in args.steps.split(",") if s]:
    name, batch = item.split(":")
    record["qat_step"][f"{name}_b{batch}"] = qat(name, int(batch))
if args.json:
    with open(args.json, "w") as fh:
        json.dump(record, fh, indent=1)
