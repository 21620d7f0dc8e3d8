#!/usr/bin/env python3
"""Option-A shortcuts read in place by the int8 epilogue (fuse_inference(narrow_rows=True, pad_shortcuts=True): the `x[:, :, ::2, ::2]`
slice and the `F.pad` of every transition block gone, the block's last convolution reading x itself) against the plan without
`pad_shortcuts`: both plans built from ONE calibrated model and timed interleaved in one process.
  case 1: the CIFAR ResNet-20 with option-A shortcuts (workloads.cifar_resnet20(option="A")), QBase W8A8, 32^2;
  case 2: the CIFAR ResNet-56 likewise.
Per case: median / min / max ms per step of either plan, the route DLMCQ_ROUTE_ONLY reports for every node with a pad shortcut, and
whether the logits of the two plans are equal.  Writes profiles/pad_shortcut_ab.json (and prints it).
usage: python tools/pad_shortcut_ab.py [batch] [rounds] [--out PATH]"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import Int8Layer, fuse_inference

CASES = (  # tag, model
    ("cifar_resnet20_option_a_qbase_w8a8", lambda: W.cifar_resnet20(option="A")),
    ("cifar_resnet56_option_a_qbase_w8a8", lambda: W.cifar_resnet56(option="A")),
)


def pad_shortcut_routes(plan, x):
    """(layer, shortcut, route as the library's dispatch reports it) of every node with a pad shortcut, asked with the node's own operands."""
    routes, hooks = [], []

    def ask(mod, args):
        codes = mod._codes(args[0])
        o = K._operand(dict(mod.operand(args[0], codes), bias=mod._bias()))
        emit = mod._emit_for(codes.shape[0], mod.k, *mod._out_hw(codes)) or K.EmitCodes(torch.ones(1, device=codes.device), None, 0, 255, N.FORM_ZEROPOINT)
        src, (stride, lo) = K._nhwc(args[1]), mod.pad_shortcut
        n, kpad = o.shape[:2]
        rc = N.lib.dlmcq_conv2d_i8_nhwc_padres(*K._head(o, None), N.ptr(mod.w_off), n, *o.geom[:3], kpad, *o.geom[3:], N.ptr(src), src.shape[2],
                                               src.shape[3], src.shape[1], stride, lo, mod._act_arg(), N.ptr(codes), N.ptr(emit.scale),
                                               N.ptr(emit.zero_point), emit.lo, emit.hi, emit.form_arg | N.ROUTE_ONLY, emit.g, mod.k, N.stream_ptr())
        w = mod.layer.weight
        routes.append({"layer": f"{w.shape[1]}->{w.shape[0]} {w.shape[2]}x{w.shape[3]} at {codes.shape[2]}x{codes.shape[3]}",
                       "shortcut": f"{src.shape[1]} channels at {src.shape[2]}x{src.shape[3]}, stride {stride}, {lo} zero channels in front",
                       "route": N.ROUTE_TAG.get(rc, rc)})
    for m in plan.modules():
        if isinstance(m, Int8Layer) and m.pad_shortcut is not None:
            hooks.append(m.register_forward_pre_hook(ask))
    plan(x)
    for h in hooks:
        h.remove()
    return routes


def main():
    a = P.arguments(__doc__, batch=1024, rounds=7)
    out = {"batch": a.batch, "rounds": a.rounds, "steps_per_round": 3, "resolution": 32}
    for tag, make in CASES:
        model = P.seeded_model(make)
        P.quantized(model, P.QBASE_W8A8)
        x = P.relu_images(a.batch, 32)
        with torch.no_grad():
            model(x[:64])                                   # calibrate
            plans = {"pad_shortcuts": fuse_inference(model, narrow_rows=True, pad_shortcuts=True), "flag_off": fuse_inference(model, narrow_rows=True)}
            logits = {k: p(x) for k, p in plans.items()}
            routes = pad_shortcut_routes(plans["pad_shortcuts"], x[:8])
            ms = P.interleaved(plans, x, 2, a.rounds, 3)
        res = {"logits_equal": bool(torch.equal(logits["pad_shortcuts"], logits["flag_off"])), "pad_shortcut_node_routes": routes}
        for k, v in ms.items():
            rep = plans[k].fusion_report
            res[k] = dict(P.arm_summary(v), int8_layers=rep.layers, residual_fused=rep.residual, narrow_nodes=rep.narrow,
                          pad_shortcuts=rep.pad_shortcuts, fp32_outputs=rep.fp32_outputs)
        res["speedup_median"] = P.speedup_median(res["pad_shortcuts"], res["flag_off"])
        out[tag] = res
        del model, plans, x, logits
        torch.cuda.empty_cache()
    P.write_profile("pad_shortcut_ab", out, a.out)


if __name__ == "__main__":
    main()
