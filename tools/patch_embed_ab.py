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
usage: python tools/patch_embed_ab.py [batch] [steps] [--out PATH]"""
import plan_ab as P  # (first: it puts the repository on the import path)
import torch
import workloads as W
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import PatchRowsLayer, fuse_inference

FLAGS = dict(layer_norms=True, gelu=True, attention=True)


def node_report(us, kernel, torch_ops):
    (kq1, kmed, kq3), (tq1, tmed, tq3) = P.quartiles(us[kernel]), P.quartiles(us[torch_ops])
    iqr = max(tq3 - tq1, kq3 - kq1)
    return {"kernel_us_median": round(kmed, 2), "kernel_us_q1_q3": [round(kq1, 2), round(kq3, 2)], "torch_ops_us_median": round(tmed, 2),
            "torch_ops_us_q1_q3": [round(tq1, 2), round(tq3, 2)], "iqr_us": round(iqr, 2), "ratio_torch_over_kernel": round(tmed / kmed, 2),
            "kernel_faster_beyond_iqr": bool(tmed - kmed > iqr)}


def main():
    arg = P.arguments(__doc__, batch=256, steps=24)
    batch = arg.batch
    out = {"model": "vit_small()", "batch": batch, "steps_per_plan": arg.steps, "resolution": 224, "both_plans": FLAGS}
    for tag, fam in P.CASES:
        model = P.seeded_model(W.vit_small, bn=False)
        x = torch.randn(batch, 3, 224, 224, device=P.DEV)
        P.calibrate(model, fam, x)
        with torch.no_grad():
            plans = {"patch_embed": fuse_inference(model, patch_embed=True, **FLAGS), "flag_off": fuse_inference(model, **FLAGS)}
            logits = {k: p(x) for k, p in plans.items()}
            recs = {k: P.profile_step(p, x) for k, p in plans.items()}
            # the two nodes against the torch ops they replace, on the step's own tensors
            node = next(m for m in plans["patch_embed"].modules() if isinstance(m, PatchRowsLayer))
            p, emit = node.patch, node.emit.emit(x.numel())
            e = torch.randn(batch, node.tokens, model.cls_token.shape[2], device=P.DEV)
            cls, pos = model.cls_token.detach(), model.pos_embedding.detach()

            def torch_rows(_=None):
                rows = K.patch_rows_torch(x, p)      # (the last reshape is the strided copy)
                return K.fake_quant(rows, emit.scale, emit.zero_point, emit.lo, emit.hi, emit.form, g=emit.g, codes="i8", want_y=False)[1]
            calls = {"patch_rows_kernel": lambda _: K.patch_rows_quant(x, p, emit=emit, want_out=False), "patch_rows_torch": torch_rows,
                     "tokens_kernel": lambda _: K.assemble_tokens(e, cls, pos),
                     "tokens_torch": lambda _: torch.cat((cls.expand(batch, -1, -1), e), dim=1) + pos}
            for _ in range(2):                              # two warm rounds of the four calls in turn, then `steps` rounds: us per call
                for fn in calls.values():
                    fn(None)
            us = {k: [t * 1e3 for t in v] for k, v in P.interleaved(calls, None, 0, arg.steps, 1).items()}
            same = (torch.equal(K.patch_rows_quant(x, p, emit=emit, want_out=False)[1], torch_rows()) and
                    torch.equal(K.assemble_tokens(e, cls, pos), torch.cat((cls.expand(batch, -1, -1), e), dim=1) + pos))
            ms = P.interleaved(plans, x, 3, arg.steps, 1)
        a, b = logits["patch_embed"].float(), logits["flag_off"].float()
        res = {"logits_equal": bool(torch.equal(a, b)), "logits": a.numel(), "nodes_equal_torch": bool(same),
               "patch_rows": node_report(us, "patch_rows_kernel", "patch_rows_torch"), "tokens": node_report(us, "tokens_kernel", "tokens_torch"),
               "kernels_in_one_step": {name: P.launch_sum(recs["patch_embed"], name)      # (gelu: the map-to-codes yardstick of DESIGN.md 5.23)
                                       for name in ("patch_rows", "tokens", "gelu")}}
        fq = {k: [r[2] for r in v if r[0] == "fq_tensor"] for k, v in recs.items()}
        res["quantise_launches_saved"] = len(fq["flag_off"]) - len(fq["patch_embed"])
        res["launches_recorded"] = {k: len(v) for k, v in recs.items()}
        for k, v in ms.items():
            rep = plans[k].fusion_report
            res[k] = dict(P.arm_summary(v, P.QUARTILES), int8_layers=rep.layers, patch_rows=rep.patch_rows,
                          token_assemblies=rep.token_assemblies, layer_norms=rep.layer_norms, gelus=rep.gelus, attentions=rep.attentions,
                          not_eligible=len(rep.skipped))
        res.update(P.verdict(res["patch_embed"], res["flag_off"], "iqr_off"))
        out[tag] = res
        del model, plans, x, logits
        torch.cuda.empty_cache()
    P.write_profile("patch_embed_ab", out, arg.out)


if __name__ == "__main__":
    main()
