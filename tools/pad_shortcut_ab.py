#!/usr/bin/env python3
"""Option-A shortcuts read in place by the int8 epilogue (fuse_inference(narrow_rows=True, pad_shortcuts=True): the `x[:, :, ::2, ::2]`
slice and the `F.pad` of every transition block gone, the block's last convolution reading x itself) against the plan without
`pad_shortcuts`: both plans built from ONE calibrated model and timed interleaved in one process.
  case 1: the CIFAR ResNet-20 with option-A shortcuts (workloads.cifar_resnet20(option="A")), QBase W8A8, 32^2;
  case 2: the CIFAR ResNet-56 likewise.
Per case: median / min / max ms per step of either plan, the route DLMCQ_ROUTE_ONLY reports for every node with a pad shortcut, and
whether the logits of the two plans are equal.  Writes profiles/pad_shortcut_ab.json (and prints it).
usage: python tools/pad_shortcut_ab.py [batch] [rounds]"""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dlmc-quant_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

import workloads as W  # noqa: E402
from act_offset_ab import QBASE_W8A8  # noqa: E402
from dlmc import _native as N  # noqa: E402
from dlmc.quantization.scalar import kernels as K  # noqa: E402
from dlmc.utils.fuse import Int8Layer, fuse_inference  # noqa: E402
from dlmc.utils.merge_bn import merge_bn  # noqa: E402
from dlmc.utils.quantize import quantize_model  # noqa: E402
from relu6_ab import timed  # noqa: E402

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
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    dev = "cuda:0"
    out = {"batch": batch, "rounds": rounds, "steps_per_round": 3, "resolution": 32}
    for tag, make in CASES:
        torch.manual_seed(2333)
        model = merge_bn(make().to(dev).eval(), inplace=True, allow_missing=True)
        quantize_model(model, copy.deepcopy(QBASE_W8A8), None)
        x = torch.relu(torch.randn(batch, 3, 32, 32, device=dev))
        with torch.no_grad():
            model(x[:64])                                   # calibrate
            plans = {"pad_shortcuts": fuse_inference(model, narrow_rows=True, pad_shortcuts=True), "flag_off": fuse_inference(model, narrow_rows=True)}
            logits = {k: p(x) for k, p in plans.items()}
            routes = pad_shortcut_routes(plans["pad_shortcuts"], x[:8])
            for p in plans.values():                        # warm-up
                timed(p, x, 2)
            ms = {k: [] for k in plans}
            for _ in range(rounds):                         # interleaved: A, B, A, B, ...
                for k, p in plans.items():
                    ms[k].append(timed(p, x, 3))
        res = {"logits_equal": bool(torch.equal(logits["pad_shortcuts"], logits["flag_off"])), "pad_shortcut_node_routes": routes}
        for k, v in ms.items():
            rep = plans[k].fusion_report
            res[k] = {"ms_per_step_median": round(sorted(v)[len(v) // 2], 3), "ms_per_step_min": round(min(v), 3),
                      "ms_per_step_max": round(max(v), 3), "all_ms": [round(t, 3) for t in v], "int8_layers": rep.layers,
                      "residual_fused": rep.residual, "narrow_nodes": rep.narrow, "pad_shortcuts": rep.pad_shortcuts,
                      "fp32_outputs": rep.fp32_outputs}
        res["speedup_median"] = round(res["flag_off"]["ms_per_step_median"] / res["pad_shortcuts"]["ms_per_step_median"], 3)
        out[tag] = res
        del model, plans, x, logits
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    with open(os.path.join(ROOT, "profiles", "pad_shortcut_ab.json"), "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
