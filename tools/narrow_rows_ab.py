#!/usr/bin/env python3
"""Narrow fp32 rows in the int8 plan (fuse_inference(narrow_rows=True): shortcut adds folded behind channel-padded layers, their fp32
tensors at the real width) against the plan without the flag: both plans built from ONE calibrated model and timed interleaved in one
process.
  case 1: MobileNetV2, FSPTQ W8A8, relu(N(0,1)) images, 224^2;
  case 2: MobileNetV2, QBase W4A8 (tools/plan_ab.py's QBASE_W4A8) with act_offsets=True, 224^2 - the plan of
          profiles/plan_profile_mobilenet_v2_qbase_act_offsets_b1024.txt;
  case 3: the CIFAR ResNet-20 (workloads.cifar_resnet20), QBase W8A8, 32^2.
Per case: median / min / max ms per step of either plan, the route DLMCQ_ROUTE_ONLY reports for every narrow node, and whether the
logits of the two plans are equal.  Writes profiles/narrow_rows_ab.json (and prints it).
usage: python tools/narrow_rows_ab.py [batch] [rounds] [--out PATH]"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import Int8Layer, fuse_inference

CASES = (  # tag, model, config, quantization type, fuse_inference arguments, resolution
    ("mobilenet_v2_fsptq_w8a8", W.mobilenet_v2, P.FSPTQ_W8A8, "FSPTQ", {}, 224),
    ("mobilenet_v2_qbase_w4a8_act_offsets", W.mobilenet_v2, P.QBASE_W4A8, None, {"act_offsets": True}, 224),
    ("cifar_resnet20_qbase_w8a8", W.cifar_resnet20, P.QBASE_W8A8, None, {}, 32),
)


def narrow_routes(plan, x):
    """(layer, its route as the library's dispatch reports it) of every narrow node, asked with the node's own operands in a forward."""
    routes, hooks = [], []

    def ask(mod, args):
        codes = mod._codes(args[0])
        o = K._operand(dict(mod.operand(args[0], codes), bias=mod._bias()))
        emit = mod._emit_for(codes.shape[0], mod.k, *mod._out_hw(codes)) or K.EmitCodes(torch.ones(1, device=codes.device), None, 0, 255, N.FORM_ZEROPOINT)
        n, kpad = o.shape[:2]
        rc = N.lib.dlmcq_conv2d_i8_nhwc_narrow(*K._head(o, None), N.ptr(mod.w_off), n, *o.geom[:3], kpad, *o.geom[3:], None, mod._act_arg(),
                                               N.ptr(codes), N.ptr(emit.scale), N.ptr(emit.zero_point), emit.lo, emit.hi,
                                               emit.form_arg | N.ROUTE_ONLY, emit.g, mod.k, N.stream_ptr())
        w = mod.layer.weight
        routes.append({"layer": f"{w.shape[1]}->{w.shape[0]} {w.shape[2]}x{w.shape[3]} at {codes.shape[2]}x{codes.shape[3]}",
                       "shortcut": len(args) > 1, "route": N.ROUTE_TAG.get(rc, rc)})
    for m in plan.modules():
        if isinstance(m, Int8Layer) and m.narrow:
            hooks.append(m.register_forward_pre_hook(ask))
    plan(x)
    for h in hooks:
        h.remove()
    return routes


def main():
    a = P.arguments(__doc__, batch=1024, rounds=7)
    out = {"batch": a.batch, "rounds": a.rounds, "steps_per_round": 3}
    for tag, make, cfg, qtype, kw, side in CASES:
        model = P.seeded_model(make)
        P.quantized(model, cfg, qtype)
        x = P.relu_images(a.batch, side)
        with torch.no_grad():
            model(x[:64])                                   # calibrate
            plans = {"narrow_rows": fuse_inference(model, narrow_rows=True, **kw), "flag_off": fuse_inference(model, **kw)}
            logits = {k: p(x) for k, p in plans.items()}
            routes = narrow_routes(plans["narrow_rows"], x[:8])
            ms = P.interleaved(plans, x, 2, a.rounds, 3)
        res = {"resolution": side, "logits_equal": bool(torch.equal(logits["narrow_rows"], logits["flag_off"])), "narrow_node_routes": routes}
        for k, v in ms.items():
            rep = plans[k].fusion_report
            res[k] = dict(P.arm_summary(v), int8_layers=rep.layers, residual_fused=rep.residual, narrow_nodes=rep.narrow,
                          fp32_outputs=rep.fp32_outputs)
        res["speedup_median"] = P.speedup_median(res["narrow_rows"], res["flag_off"])
        out[tag] = res
        del model, plans, x, logits
        torch.cuda.empty_cache()
    P.write_profile("narrow_rows_ab", out, a.out)


if __name__ == "__main__":
    main()
