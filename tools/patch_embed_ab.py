#!/usr/bin/env python3
"""The front of a vision transformer on the int8 plan (fuse_inference(patch_embed=True): the patch rearrangement one launch of
csrc/patch_rows.hip that hands the embedding its activation codes, the class-token concatenation + position embedding one launch of
csrc/tokens.hip) against the plan that runs the reshape / permute / reshape, the concatenation and the add in torch and lets the
embedding quantise: both plans built from ONE calibrated model, both with layer_norms=True, gelu=True and attention=True, timed
interleaved, step by step, in one process.
  cases: workloads.vit_small() (ViT-S/16: 196 patches of 768 features, width 384) at 224^2, FSPTQ W8A8 (the calibrated zero points
         rounded to integers) and QBase W8A8 (float offsets set to 0).
Per case: median ms per step of either plan over `steps` single steps each (A, B, A, B, ...), the run-to-run spread = the interquartile
range of the flag-off plan's steps, whether the logits are equal; per node, on the step's own tensors and interleaved launch by launch
(`steps` of each): the kernel's launch against the torch ops it replaces as the flag-off plan runs them - the strided copy and the
embedding's K.fake_quant for the patch rows, torch.cat and the add for the tokens - timed with events, medians and the interquartile
range of the torch ops, and whether the kernel is faster by more than that; and from the launch profile's records of one step
(K.PROFILE: algorithmic bytes, event times) each kernel's bytes per second.
Writes profiles/patch_embed_ab.json (and prints it).
usage: python tools/patch_embed_ab.py [batch] [steps]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dlmc-quant_amd"), os.path.join(ROOT, "tools")]
import torch  # noqa: E402

import workloads as W  # noqa: E402
from attention_ab import profile_step  # noqa: E402
from dlmc.quantization.scalar import kernels as K  # noqa: E402
from dlmc.utils.fuse import PatchRowsLayer, fuse_inference  # noqa: E402
from relu6_ab import timed  # noqa: E402
from swish_ab import quartiles  # noqa: E402
from transformer_ab import CASES, calibrate  # noqa: E402

FLAGS = dict(layer_norms=True, gelu=True, attention=True)


def event_us(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3


def interleaved(pairs, steps):
    """{name: [us per call]} of the callables in `pairs`, called in turn, `steps` rounds after two warm rounds."""
    for _ in range(2):
        for fn in pairs.values():
            fn()
    us = {k: [] for k in pairs}
    for _ in range(steps):
        for k, fn in pairs.items():
            us[k].append(event_us(fn))
    return us


def node_report(us, kernel, torch_ops):
    (kq1, kmed, kq3), (tq1, tmed, tq3) = quartiles(us[kernel]), quartiles(us[torch_ops])
    iqr = max(tq3 - tq1, kq3 - kq1)
    return {"kernel_us_median": round(kmed, 2), "kernel_us_q1_q3": [round(kq1, 2), round(kq3, 2)], "torch_ops_us_median": round(tmed, 2),
            "torch_ops_us_q1_q3": [round(tq1, 2), round(tq3, 2)], "iqr_us": round(iqr, 2), "ratio_torch_over_kernel": round(tmed / kmed, 2),
            "kernel_faster_beyond_iqr": bool(tmed - kmed > iqr)}


def main():
    batch = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 24
    dev = "cuda:0"
    out = {"model": "vit_small()", "batch": batch, "steps_per_plan": steps, "resolution": 224, "both_plans": FLAGS}
    for tag, fam in CASES:
        torch.manual_seed(2333)
        model = W.vit_small().to(dev).eval()
        x = torch.randn(batch, 3, 224, 224, device=dev)
        calibrate(model, fam, x)
        with torch.no_grad():
            plans = {"patch_embed": fuse_inference(model, patch_embed=True, **FLAGS), "flag_off": fuse_inference(model, **FLAGS)}
            logits = {k: p(x) for k, p in plans.items()}
            recs = {k: profile_step(p, x) for k, p in plans.items()}
            # the two nodes against the torch ops they replace, on the step's own tensors
            node = next(m for m in plans["patch_embed"].modules() if isinstance(m, PatchRowsLayer))
            p, emit = node.patch, node.emit.emit(x.numel())
            e = torch.randn(batch, node.tokens, model.cls_token.shape[2], device=dev)
            cls, pos = model.cls_token.detach(), model.pos_embedding.detach()

            def torch_rows():
                rows = K.patch_rows_torch(x, p)      # (the last reshape is the strided copy)
                return K.fake_quant(rows, emit.scale, emit.zero_point, emit.lo, emit.hi, emit.form, g=emit.g, codes="i8", want_y=False)[1]
            us = interleaved({"patch_rows_kernel": lambda: K.patch_rows_quant(x, p, emit=emit, want_out=False), "patch_rows_torch": torch_rows,
                              "tokens_kernel": lambda: K.assemble_tokens(e, cls, pos),
                              "tokens_torch": lambda: torch.cat((cls.expand(batch, -1, -1), e), dim=1) + pos}, steps)
            same = (torch.equal(K.patch_rows_quant(x, p, emit=emit, want_out=False)[1], torch_rows()) and
                    torch.equal(K.assemble_tokens(e, cls, pos), torch.cat((cls.expand(batch, -1, -1), e), dim=1) + pos))
            for pl in plans.values():                       # warm-up
                timed(pl, x, 3)
            ms = {k: [] for k in plans}
            for _ in range(steps):                          # interleaved: A, B, A, B, ...
                for k, pl in plans.items():
                    ms[k].append(timed(pl, x, 1))
        a, b = logits["patch_embed"].float(), logits["flag_off"].float()
        res = {"logits_equal": bool(torch.equal(a, b)), "logits": a.numel(), "nodes_equal_torch": bool(same),
               "patch_rows": node_report(us, "patch_rows_kernel", "patch_rows_torch"), "tokens": node_report(us, "tokens_kernel", "tokens_torch"),
               "kernels_in_one_step": {}}
        for name in ("patch_rows", "tokens", "gelu"):       # (gelu: the map-to-codes yardstick of DESIGN.md 5.23)
            mine = [r for r in recs["patch_embed"] if r[0] == name]
            t_ms, nbytes = sum(r[2] for r in mine), sum(r[1] for r in mine)
            res["kernels_in_one_step"][name] = {"launches": len(mine), "us": round(t_ms * 1e3, 1), "bytes": nbytes,
                                                "gb_per_s": round(nbytes / (t_ms * 1e-3) / 1e9, 1) if t_ms else None}
        fq = {k: [r[2] for r in v if r[0] == "fq_tensor"] for k, v in recs.items()}
        res["quantise_launches_saved"] = len(fq["flag_off"]) - len(fq["patch_embed"])
        res["launches_recorded"] = {k: len(v) for k, v in recs.items()}
        for k, v in ms.items():
            rep = plans[k].fusion_report
            q1, med, q3 = quartiles(v)
            res[k] = {"ms_per_step_median": round(med, 3), "ms_per_step_q1": round(q1, 3), "ms_per_step_q3": round(q3, 3),
                      "ms_per_step_min": round(min(v), 3), "ms_per_step_max": round(max(v), 3), "all_ms": [round(t, 3) for t in v],
                      "int8_layers": rep.layers, "patch_rows": rep.patch_rows, "token_assemblies": rep.token_assemblies,
                      "layer_norms": rep.layer_norms, "gelus": rep.gelus, "attentions": rep.attentions, "not_eligible": len(rep.skipped)}
        on, off = res["patch_embed"], res["flag_off"]
        spread = off["ms_per_step_q3"] - off["ms_per_step_q1"]
        res["run_to_run_spread_ms"] = round(spread, 3)      # (the interquartile range of the baseline's steps)
        res["speedup_median"] = round(off["ms_per_step_median"] / on["ms_per_step_median"], 3)
        res["flag_on_faster_beyond_spread"] = bool(off["ms_per_step_median"] - on["ms_per_step_median"] > spread)
        res["flag_on_slower_beyond_spread"] = bool(on["ms_per_step_median"] - off["ms_per_step_median"] > spread)
        out[tag] = res
        del model, plans, x, logits
        torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    with open(os.path.join(ROOT, "profiles", "patch_embed_ab.json"), "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
