"""tools/plan_ab.py, the module the plan A/B tools share, on the host: its statistics and verdicts reproduce every two-arm case recorded
under profiles/ (22 cases of seven tools, under that tool's spread rule), `quartiles` follows the index rule written out here, and - read
with `ast`, nothing imported - no tool imports another tool and every shared helper has one definition."""
import ast
import glob
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")

RULES = {"avgpool_shortcut_ab": ("range", 8), "gate_ab": ("range", 2), "swish_ab": ("iqr_off", 2), "hardswish_ab": ("iqr_off", 4),
         "transformer_ab": ("iqr_off", 2), "attention_ab": ("iqr_off", 2), "patch_embed_ab": ("iqr_off", 2)}      # tool: its rule, its cases
STATS = ("median", "q1", "q3", "min", "max")


@pytest.fixture(scope="module")
def P():
    """tools/plan_ab.py, imported by the statistics tests alone (it imports torch and the package), tools/ on the path no longer than that."""
    sys.path.insert(0, TOOLS)
    try:
        import plan_ab
    finally:
        sys.path.remove(TOOLS)
    return plan_ab


def recorded(tool):
    with open(os.path.join(ROOT, "profiles", tool + ".json")) as f:
        return {tag: case for tag, case in json.load(f).items() if isinstance(case, dict) and "run_to_run_spread_ms" in case}


def test_every_recorded_case_is_found():
    assert {tool: len(recorded(tool)) for tool in RULES} == {tool: n for tool, (_, n) in RULES.items()}


@pytest.mark.parametrize("tool, tag", [(tool, tag) for tool in RULES for tag in recorded(tool)])
def test_recorded_statistics_reproduce(P, tool, tag):
    case = recorded(tool)[tag]
    arms = {k: v for k, v in case.items() if isinstance(v, dict) and "all_ms" in v}
    assert len(arms) == 2 and "flag_off" in arms
    summary = {}
    for k, rec in arms.items():
        stats = tuple(s for s in STATS if f"ms_per_step_{s}" in rec)
        assert {"median", "min", "max"} <= set(stats)
        summary[k] = P.arm_summary(rec["all_ms"], stats)
        assert summary[k] == {key: rec[key] for key in summary[k]}, (k, summary[k])      # median, min, max, q1, q3 and all_ms: exactly
    on = next(k for k in arms if k != "flag_off")
    flags = tuple(k for k in ("faster", "slower") if f"flag_on_{k}_beyond_spread" in case)
    assert flags
    got = P.verdict(summary[on], summary["flag_off"], RULES[tool][0], flags)
    assert list(got) == ["run_to_run_spread_ms", "speedup_median"] + [f"flag_on_{k}_beyond_spread" for k in flags]
    # the tools took spread and speed-up from the rounded summaries, as `verdict` does: the recorded all_ms give them back exactly
    assert got == {k: case[k] for k in got}


def test_the_two_rules_differ_and_others_are_refused(P):
    on = P.arm_summary([1.0, 1.1, 1.2, 5.0], P.QUARTILES)
    off = P.arm_summary([2.0, 2.1, 2.2, 2.3], P.QUARTILES)
    assert P.verdict(on, off, "range")["run_to_run_spread_ms"] == 4.0
    assert P.verdict(on, off, "iqr_off")["run_to_run_spread_ms"] == round(2.3 - 2.1, 3)
    with pytest.raises(ValueError):
        P.verdict(on, off, "iqr")


@pytest.mark.parametrize("n", [1, 2, 4, 7, 24])
def test_quartiles_index_rule(P, n):
    v = [((7 * i) % n) + 0.5 * (i % 2) for i in range(n)]      # distinct, not sorted
    s = sorted(v)
    assert P.quartiles(v) == tuple(s[min(n - 1, int(f * n))] for f in (0.25, 0.5, 0.75))
    assert P.arm_summary(v)["ms_per_step_median"] == round(s[n // 2], 3)


# ------------------------------------------------------------------------------------------- import hygiene, from the source text
AB_TOOLS = sorted(glob.glob(os.path.join(TOOLS, "*_ab.py")) + [os.path.join(TOOLS, "node_times.py")])
LAB_TOOLS = ("chain_ab.py", "halo_pipe_ab.py", "fq_multi_ab.py")      # raw entry points on lab builds: their own loop, left alone
IN_SCOPE = [p for p in AB_TOOLS if os.path.basename(p) not in LAB_TOOLS]      # plan_ab.py, its 13 tools, node_times.py, dw5_ab.py


def tree(path):
    with open(path) as f:
        return ast.parse(f.read())


def imported(path):
    names = set()
    for node in ast.walk(tree(path)):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom) and node.module and not node.level:
            names.add(node.module.split(".")[0])
    return names


def test_no_tool_imports_another_tool():
    siblings = {os.path.basename(p)[:-3] for p in glob.glob(os.path.join(TOOLS, "*.py"))}
    assert "plan_ab" in siblings and len(IN_SCOPE) == 16
    for path in AB_TOOLS:
        mine = imported(path) & siblings
        if os.path.basename(path) == "plan_ab.py" or path not in IN_SCOPE:
            assert mine == set(), (path, mine)
        else:
            assert mine == {"plan_ab"}, (path, mine)


def test_shared_helpers_are_defined_once():
    where = {}
    for path in IN_SCOPE:
        for node in tree(path).body:
            names = [node.name] if isinstance(node, ast.FunctionDef) else \
                [t.id for t in node.targets if isinstance(t, ast.Name)] if isinstance(node, ast.Assign) else []
            for name in names:
                where.setdefault(name, []).append(os.path.basename(path))
    for name in ("timed", "quartiles", "calibrated", "node_times", "profile_step", "QBASE_W8A8", "QBASE_W4A8"):
        assert where.get(name) == ["plan_ab.py"], (name, where.get(name))
