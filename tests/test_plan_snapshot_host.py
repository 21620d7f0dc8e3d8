"""The plan `fuse_inference` builds, node for node, against recorded texts (tests/plan_dump.py, tests/golden/plans/): models marked
calibrated by hand on the CPU, every case under `dry_run=True` (the main pass's decisions) and `dry_run="chains"` (the chain-level passes
on stand-ins of the plan layers); the passes that put code-emitting nodes behind the main pass (_node_pass_cases) under `dry_run=True`
alone.  A change to the plan builder that is meant to keep the plans keeps these texts; one that is meant to
change a plan regenerates the files it changes (`python tests/test_plan_snapshot_host.py`) and shows the difference for review.
One file per case: the plan's text, or - first line `= <case>` - its difference (difflib.unified_diff, no context) from the text of that
other case, which has its own file and test: most cases differ from a neighbour in a few lines, many in none."""
import difflib
import functools
import os
import sys

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "plans")
CIFAR_FLAGS = [dict(narrow_rows=n, pad_shortcuts=p) for n in (False, True) for p in (False, True)]
GAP = [dict(), dict(gap_head=True), dict(gap_head="separate"), dict(gap_head="fused")]


@functools.lru_cache(maxsize=None)
def model(name):
    """The hand-calibrated model `name`, built once: neither dry run changes the model it reads."""
    import workloads as W
    from test_act_offset_host import calibrated as qbase_mobilenet
    from test_chain_recompute_host import _resnet50
    from test_gap_host import calibrated
    if name == "resnet50":
        return _resnet50()
    if name == "mobilenet_v2_qbase":
        return qbase_mobilenet(first_offset=True)[0]
    if name.startswith("cifar_resnet20_"):
        return calibrated(W.CifarResNet(3, option=name[-1]))
    if name == "small_vit":
        from transformer_nets import small_vit
        return calibrated(small_vit())
    if name == "mobilenet_v2_se_swish":
        return calibrated(W.mobilenet_v2(se=True, act="swish"))
    if name.startswith("left_"):
        return _left_alone(name[len("left_"):])
    return calibrated(getattr(W, name)())


def _left_alone(name):
    """One model per code-emitting pass that the pass leaves as it is, from the LEFT_ALONE tables of the passes' host tests."""
    import attention_nets
    import test_avgpool_host
    import test_gate_host
    import test_patch_embed_host
    import test_swish_host
    import test_transformer_host
    from test_gap_host import calibrated
    kind, _, case = name.partition("_")
    if kind == "swish":
        return calibrated(test_swish_host.Toy(test_swish_host.LEFT_ALONE[case]))
    if kind == "gate":
        return calibrated(test_gate_host.Toy(test_gate_host.LEFT_ALONE[case]))
    if kind == "avgpool":
        pool, tail = test_avgpool_host.LEFT_ALONE[case]
        return calibrated(test_avgpool_host.Toy(pool(), tail))
    if kind == "rows":
        return test_transformer_host.LEFT_ALONE[case]()
    if kind == "attention":
        return calibrated(attention_nets.LEFT_ALONE[case]())
    return calibrated(test_patch_embed_host.LEFT[case][0]())


def _cases():
    out = []
    for name in ("resnet18", "resnet50", "repvgg_a1_deploy", "mobileone_s1_deploy"):
        out += [(name, kw) for kw in GAP]
    out.append(("mobileone_s1_deploy", dict(dwpw=True)))
    out += [("mobilenet_v2", kw) for kw in (dict(), dict(narrow_rows=True), dict(relu6=False))]
    out += [("mobilenet_v2_qbase", kw) for kw in (dict(act_offsets=True), dict(act_offsets=True, narrow_rows=True))]
    for option in "ABCD":
        out += [(f"cifar_resnet20_{option}", kw) for kw in CIFAR_FLAGS]
        if option in "CD":
            out += [(f"cifar_resnet20_{option}", dict(kw, avg_pools=True)) for kw in CIFAR_FLAGS]
    out = [(name, kw, dry) for name, kw in out for dry in (True, "chains")]
    # (ResNet-50's chain-level flags decide nothing without the chain passes: under "chains" only)
    out += [("resnet50", kw, "chains") for kw in (dict(recompute_shortcuts=True), dict(recompute_shortcuts=False), dict(block_layout=True),
                                                  dict(block_layout=False), dict(chain_pairs=False))]
    return out + [(name, kw, True) for name, kw in _node_pass_cases()]


TRANSFORMER = dict(patch_embed=True, layer_norms=True, gelu=True, attention=True)


def _node_pass_cases():
    """The passes that put a code-emitting node behind the main pass's plan (swish, gate, average pool, patch embedding, LayerNorm, GELU,
    attention), under `dry_run=True` only: each transformer flag alone and all four, the squeeze-excite / swish networks, and per pass one
    model it leaves alone (a matcher that starts taking more shows up here)."""
    out = [("small_vit", {flag: True}) for flag in TRANSFORMER] + [("small_vit", TRANSFORMER), ("vit_small", TRANSFORMER)]
    out += [("mobilenet_v2_se_swish", dict(gates=True)), ("mobilenet_v2_se_swish", dict(gates=True, swish=True)),
            ("efficientnet_b0", dict(gates=True, swish=True, dw5=True))]
    return out + [("left_swish_sigmoid_read_twice", dict(swish=True)), ("left_gate_spatial_gate", dict(gates=True)),
                  ("left_avgpool_kernel_3_stride_2", dict(avg_pools=True)), ("left_rows_c_66", dict(layer_norms=True)),
                  ("left_rows_tanh_gelu", dict(gelu=True)), ("left_attention_scores_read_twice", dict(attention=True)),
                  ("left_patch_p_mod_4", dict(patch_embed=True)), ("left_patch_pos_of_the_wrong_length", dict(patch_embed=True))]


def case_id(name, kw, dry):
    flags = "".join(f"-{k}_{v}" for k, v in sorted(kw.items())) or "-default"
    return f"{name}{flags}-{'chains' if dry == 'chains' else 'dry'}"


CASES = _cases()
IDS = [case_id(*c) for c in CASES]


def build(name, kw, dry):
    from dlmc.utils import fuse
    default = fuse.RECOMPUTE_DEFAULT
    fuse.RECOMPUTE_DEFAULT = True        # (the flag's default is read from the environment: the recorded plans are those of an unset one)
    try:
        return fuse.fuse_inference(model(name), dry_run=dry, **kw)
    finally:
        fuse.RECOMPUTE_DEFAULT = default


def standins(gm):
    """The Int8Layer stand-ins of a `dry_run="chains"` plan, those inside dual and chain nodes included, each once."""
    from dlmc.utils.fuse import Int8Layer
    seen = {}
    for m in gm.modules():
        for p in [m] + [getattr(m, part, None) for part in ("a", "b", "short", "main")]:
            if isinstance(p, Int8Layer):
                seen[id(p)] = p
    return list(seen.values())


@functools.lru_cache(maxsize=None)
def text(case):
    from plan_dump import plan_text
    return plan_text(build(*CASES[IDS.index(case)]))


def record(case, base):
    """What the file of `case` holds: its text, or the difference of its text from that of case `base`."""
    if base is None:
        return text(case)
    diff = difflib.unified_diff(text(base).splitlines(), text(case).splitlines(), lineterm="", n=0)
    return "".join(line + "\n" for line in [f"= {base}"] + list(diff)[2:])


@pytest.mark.parametrize("case", IDS)
def test_plan_is_the_recorded_plan(case):
    with open(os.path.join(GOLDEN, case + ".txt")) as f:
        want = f.read()
    base = want.split("\n", 1)[0][2:] if want.startswith("= ") else None
    assert record(case, base) == want


def test_standins_carry_the_pad_shortcuts_of_the_plan():
    """CIFAR ResNet-20, option A: the two option-A shortcuts the report counts are on the stand-ins, as on the real plan's nodes."""
    gm = build("cifar_resnet20_A", dict(narrow_rows=True, pad_shortcuts=True), "chains")
    rep = gm.fusion_report
    nodes = standins(gm)
    assert rep.pad_shortcuts == 2 and rep.narrow > 0
    assert sum(m.pad_shortcut is not None for m in nodes) == rep.pad_shortcuts
    assert sorted(m.pad_shortcut for m in nodes if m.pad_shortcut is not None) == [(2, 8), (2, 16)]
    assert sum(bool(m.narrow) for m in nodes) == rep.narrow
    assert all(m.narrow for m in nodes if m.pad_shortcut is not None and m.k_pad != m.k)


def test_standins_carry_the_narrow_rows_of_the_plan():
    """MobileNetV2 (FSPTQ): the 11 narrow nodes the report counts (tests/test_narrow_rows_host.py) are narrow stand-ins."""
    gm = build("mobilenet_v2", dict(narrow_rows=True), "chains")
    assert gm.fusion_report.narrow == 11
    assert sum(bool(m.narrow) for m in standins(gm)) == 11


def test_no_recorded_plan_is_left_over():
    assert sorted(os.listdir(GOLDEN)) == sorted(i + ".txt" for i in IDS)


if __name__ == "__main__":      # regenerate the recorded plans, each against the earlier case that leaves the least to write down
    sys.path[:0] = [os.path.join(os.path.dirname(GOLDEN), "..", ".."), os.path.join(os.path.dirname(GOLDEN), "..", "..", "dlmc-quant_amd")]
    sys.path[:0] = sys.argv[2:]       # (another tree's package directory: the plans as that tree builds them)
    os.makedirs(sys.argv[1] if sys.argv[1:] else GOLDEN, exist_ok=True)
    for n, case in enumerate(IDS):
        best = min([record(case, base) for base in [None] + IDS[:n]], key=len)
        with open(os.path.join(sys.argv[1] if sys.argv[1:] else GOLDEN, case + ".txt"), "w") as f:
            f.write(best)
        print(len(best), case)
