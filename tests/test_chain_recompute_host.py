"""The plan pass that lets a chain recompute its shortcut instead of reading it (dlmc.utils.fuse._recompute_pass), on CPU models whose
wrappers are marked calibrated by hand: structure only (`dry_run="chains"`: the chain-level decisions on stand-ins of the plan layers)."""
import operator

import torch


def _resnet50():
    import workloads as W
    from dlmc.quantization.scalar.FSPTQuant import FSPTQBase
    from dlmc.utils.quantize import quantize_model
    cfg = {"weight": {"enable": True, "type": "minmax_channel", "args": {"n_bits": 8, "signed": True}},
           "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
           "exclude_layers": [], "override_options": []}
    net = W.resnet50()
    for m in net.modules():                      # BatchNorm folded by hand: the pass treats Identity as a wire
        for name, child in list(m.named_children()):
            if isinstance(child, torch.nn.BatchNorm2d):
                setattr(m, name, torch.nn.Identity())
    quantize_model(net, cfg, None, "FSPTQ")
    for m in net.modules():
        if isinstance(m, FSPTQBase):
            m.in_init_state.fill_(1)
            m.wt_init_state.fill_(1)
            m.in_offset = torch.tensor(0.0)
    return net.eval()


def _chains(gm):
    from dlmc.utils.fuse import ChainInt8Layer
    mods = dict(gm.named_modules())
    return [(n, mods[n.target]) for n in gm.graph.nodes if n.op == "call_module" and isinstance(mods.get(n.target), ChainInt8Layer)]


def test_the_pass_rewrites_exactly_the_stage_1_pair_of_resnet50():
    from dlmc.utils.fuse import fuse_inference
    gm = fuse_inference(_resnet50(), dry_run="chains", recompute_shortcuts=True)
    rep = gm.fusion_report
    assert rep.chained == 11 and rep.recomputed == 1, rep
    chains = _chains(gm)
    duals = [(n, m) for n, m in chains if m.short is not None]
    assert len(chains) == 11 and len(duals) == 2
    (n0, m0), (n2, m2) = duals                         # stage 1's and stage 2's first blocks, in graph order
    took = [(n, m) for n, m in chains if m.recompute]
    assert len(took) == 1 and [m for _, m in chains if m.defer_out] == [m0]
    n1, m1 = took[0]
    # stage 1: 64 | 64, 64 -> 256 -> 64; the first launch hands its fp32 output on unstored, the second - its only reader - recomputes it.
    # The graph's edges are as they were: the deferred value travels where the tensor did
    assert (m1.main.c, m0.main.c, m0.short.c, m1.a.k, m1.b.k) == (64, 64, 64, 256, 64)
    assert m0.a.want_out and m1.a.want_out and m1.short is None
    y0 = [u for u in n0.users if u.op == "call_function" and u.target is operator.getitem and u.args[1] == 0]
    assert len(y0) == 1 and list(y0[0].users) == [n1] and len(n1.args) == 2 and n1.args[1] is y0[0]
    # stage 2's first block (128 | 128, 256 at 28^2: not enabled) keeps writing its tensor, read by the next chain as before
    assert m2.a.want_out and not m2.defer_out and not m2.recompute
    out2 = [u for u in n2.users if u.op == "call_function" and u.target is operator.getitem and u.args[1] == 0]
    assert len(out2) == 1 and len(out2[0].users) == 1
    gm.graph.lint()


def test_the_pass_is_off_with_the_keyword_and_keeps_todays_graph():
    from dlmc.utils.fuse import fuse_inference
    gm = fuse_inference(_resnet50(), dry_run="chains", recompute_shortcuts=False)
    assert gm.fusion_report.chained == 11 and gm.fusion_report.recomputed == 0
    chains = _chains(gm)
    assert all(not m.recompute and not m.defer_out and len(n.args) == 2 for n, m in chains)
    assert all(m.a.want_out for n, m in chains if m.short is not None)
    # (the plain dry run takes no chain-level decisions at all, as before)
    assert fuse_inference(_resnet50(), dry_run=True).fusion_report.chained == 0


def test_the_pass_leaves_a_tensor_with_a_second_reader_alone():
    from dlmc.utils.fuse import RECOMPUTE_ENABLED, FusionReport, _recompute_pass, fuse_inference
    gm = fuse_inference(_resnet50(), dry_run="chains", recompute_shortcuts=False)
    n0 = next(n for n, m in _chains(gm) if m.short is not None)
    y0 = next(u for u in n0.users if u.op == "call_function" and u.target is operator.getitem and u.args[1] == 0)
    with gm.graph.inserting_after(y0):
        gm.graph.call_function(torch.sum, (y0,))        # another reader of the stage's first block tensor
    before = [(n.name, tuple(a.name for a in n.args if hasattr(a, "name"))) for n in gm.graph.nodes]
    rep = FusionReport()
    _recompute_pass(gm, rep, RECOMPUTE_ENABLED)
    assert rep.recomputed == 0
    assert before == [(n.name, tuple(a.name for a in n.args if hasattr(a, "name"))) for n in gm.graph.nodes]
    assert not any(m.recompute or m.defer_out for _, m in _chains(gm))
    # ... and a shape outside the list, likewise
    rep = FusionReport()
    _recompute_pass(fuse_inference(_resnet50(), dry_run="chains", recompute_shortcuts=False), rep, set())
    assert rep.recomputed == 0
