"""The plans fuse_inference(squeezes=True) builds for the three squeeze-excite networks, node for node, against recorded texts
(tests/plan_dump.py as it is; dry run, models marked calibrated by hand).  The texts lie in tests/golden/squeeze_plans/, a directory of
their own: tests/test_plan_snapshot_host.py requires tests/golden/plans/ to hold its own cases and nothing else.  What plan_dump does not
print of a SqueezeLayer is asserted here.  Regenerate with `python tests/test_squeeze_plan_snapshot_host.py` and review the difference."""
import functools
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "squeeze_plans")
CASES = {
    "efficientnet_b0-dw5_True-gates_True-squeezes_True-swish_True-dry": ("efficientnet_b0", {}, dict(gates=True, swish=True, dw5=True)),
    "mobilenet_v2_se-gates_True-squeezes_True-dry": ("mobilenet_v2", dict(se=True), dict(gates=True)),
    "mobilenet_v2_se_swish-gates_True-squeezes_True-swish_True-dry": ("mobilenet_v2", dict(se=True, act="swish"), dict(gates=True, swish=True)),
}


@functools.lru_cache(maxsize=None)
def plan(case):
    import workloads as W
    from dlmc.utils.fuse import fuse_inference
    from test_gap_host import calibrated
    name, net_kw, kw = CASES[case]
    return fuse_inference(calibrated(getattr(W, name)(**net_kw)), dry_run=True, squeezes=True, **kw)


@pytest.mark.parametrize("case", sorted(CASES))
def test_plan_is_the_recorded_plan(case):
    from plan_dump import plan_text
    with open(os.path.join(GOLDEN, case + ".txt")) as f:
        assert plan_text(plan(case)) == f.read()


@pytest.mark.parametrize("case", sorted(CASES))
def test_what_the_dump_does_not_print(case):
    from dlmc.utils.fuse import SqueezeLayer
    gm = plan(case)
    nodes = {n.target: n for n in gm.graph.nodes if n.op == "call_module" and n.target.startswith("_int8_squeeze_")}
    mods = dict(gm.named_modules())
    assert len(nodes) == gm.fusion_report.squeezes == (16 if case.startswith("efficientnet") else 17)
    swish = "swish_True" in case
    for name, node in nodes.items():
        m, d = mods[name], mods[name].decision
        assert isinstance(m, SqueezeLayer) and type(m).__name__ == "_DrySqueezeLayer"
        assert (m.r, m.r4, m.inner, m.gate_fn, m.rank4) == (d.r, d.r4, d.inner, d.gate_fn, d.rank4) and m.c == d.c and m.r4 % 4 == 0 and 0 <= m.r4 - m.r < 4
        assert (m.inner, m.gate_fn) == (("swish", "sigmoid") if swish else ("relu", "hardsigmoid"))
        assert m.act1 is d.q1 and m.act2 is d.q2 and m.act1.lo == 0 and m.act1.hi == 255
        # one argument, the map the pool read; the gate node multiplies that very map with this node's value
        assert len(node.args) == 1 and node.args[0].name == d.x
        (gate,) = node.users
        assert gate.target.startswith("_int8_gate_") and gate.args == (node.args[0], node)
    assert sorted(os.listdir(GOLDEN)) == sorted(c + ".txt" for c in CASES)


if __name__ == "__main__":
    here = os.path.dirname(GOLDEN)
    sys.path[:0] = [os.path.join(here, ".."), os.path.join(here, "..", ".."), os.path.join(here, "..", "..", "dlmc-quant_amd")]
    from plan_dump import plan_text
    os.makedirs(GOLDEN, exist_ok=True)
    for case in sorted(CASES):
        with open(os.path.join(GOLDEN, case + ".txt"), "w") as f:
            f.write(plan_text(plan(case)))
        print(case)
