"""What the plan A/B tools (tools/*_ab.py, tools/node_times.py) share: the quantiser configs, calibration, the interleaved timing loop, the
statistics of an arm, the two run-to-run-spread rules and their verdicts, node and launch-profile times, the command line and the writer
of profiles/<name>.json.  A tool keeps its docstring, its case table, its node- or kernel-specific extras and the keys it adds to a
case's result; it imports this module and no other tool.  Not a program."""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "dlmc-quant_amd")) if p not in sys.path]
import torch  # noqa: E402

from bench import QCFG as FSPTQ_W8A8  # noqa: E402
from dlmc.quantization.scalar import kernels as K  # noqa: E402
from dlmc.quantization.scalar.FSPTQuant import FSPTQBase  # noqa: E402
from dlmc.quantization.scalar.modules.base import QBase  # noqa: E402
from dlmc.utils.merge_bn import merge_bn  # noqa: E402
from dlmc.utils.quantize import quantize_model  # noqa: E402

DEV = "cuda:0"
QBASE_W8A8 = {"weight": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": True}},
              "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
              "exclude_layers": [], "override_options": []}
QBASE_W4A8 = {"weight": {"enable": True, "type": "minmax_channel", "args": {"n_bits": 4, "signed": False}},
              "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
              "exclude_layers": [], "override_options": []}
CASES = [("vit_small_fsptq_w8a8", "fsptq"), ("vit_small_qbase_w8a8", "qbase")]      # the transformer tools' two cases
RANGE = ("median", "min", "max")                    # an arm's statistics where the spread is max - min ...
QUARTILES = ("median", "q1", "q3", "min", "max")    # ... and where it is the flag-off arm's interquartile range


# ------------------------------------------------------------------------------------------- the model, its input, calibration
def seeded_model(make, bn=True):
    """Seed 2333, then `make()` on the GPU in eval mode, its BatchNorms merged (`bn`)."""
    torch.manual_seed(2333)
    model = make().to(DEV).eval()
    return merge_bn(model, inplace=True, allow_missing=True) if bn else model


def relu_images(batch, side):
    return torch.relu(torch.randn(batch, 3, side, side, device=DEV))


def quantized(model, cfg, qtype=None):
    """Quantise `model` in place with `cfg`; `qtype` "FSPTQ": that family's wrappers on the int8 GEMM path, as bench.py takes them."""
    quantize_model(model, copy.deepcopy(cfg), None, **({"quantization_type": qtype, "int8_gemm": True} if qtype else {}))


def _quantized_w8a8(model, fsptq):
    quantized(model, *((FSPTQ_W8A8, "FSPTQ") if fsptq else (QBASE_W8A8,)))


def calibrated(model, fam, x, zero_qbase=True):
    """Quantise `model` W8A8 in place (`fam`: "fsptq..." or "qbase..."), calibrate on x[:64], then set the activation zero points to
    exactly 0, as the tests do (FSPTQ always, QBase with `zero_qbase`)."""
    _quantized_w8a8(model, fam.startswith("fsptq"))
    with torch.no_grad():
        model(x[:64])
        for m in model.modules():
            if isinstance(m, FSPTQBase):
                m.in_offset.zero_()
                m._zp_is_int = None
            elif zero_qbase and isinstance(m, QBase) and m.in_offset is not None:
                m.in_offset.zero_()


def calibrate(model, fam, x):
    """`calibrated` for the transformer tools - what differs: 32 calibration images, and FSPTQ's zero points are rounded to integers
    (a LayerNorm or GELU output is signed: no zero point of 0), not set to 0."""
    _quantized_w8a8(model, fam == "fsptq")
    with torch.no_grad():
        model(x[:32])
        for m in model.modules():
            if isinstance(m, FSPTQBase):
                m.in_offset.round_().clamp_(m.in_min_val, m.in_max_val)
                m._zp_is_int = None
            elif isinstance(m, QBase) and m.in_offset is not None:
                m.in_offset.zero_()


# ------------------------------------------------------------------------------------------- timing
def timed(fn, x, steps):
    """ms per call of `steps` calls of fn(x) between two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn(x)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def interleaved(plans, x, warm, rounds, steps_per_round):
    """{arm: [ms per step, ...]}: `warm` steps of every arm (0: the caller has warmed them), then `rounds` timings of `steps_per_round`
    steps each, the arms in turn - A, B, A, B, ... in dictionary order."""
    for p in plans.values() if warm else ():
        timed(p, x, warm)
    ms = {k: [] for k in plans}
    for _ in range(rounds):
        for k, p in plans.items():
            ms[k].append(timed(p, x, steps_per_round))
    return ms


# ------------------------------------------------------------------------------------------- statistics
def quartiles(v):
    s = sorted(v)
    q = lambda f: s[min(len(s) - 1, int(f * len(s)))]  # noqa: E731
    return q(0.25), q(0.5), q(0.75)


def arm_summary(v, stats=RANGE, batch=None):
    """One arm's record: the `stats` asked for (of median, iqr, q1, q3, min, max; in that order) as ms_per_step_<stat>, images_per_s of
    the median step with `batch`, and all_ms - everything rounded to three places."""
    q1, med, q3 = quartiles(v)
    have = {"median": med, "iqr": q3 - q1, "q1": q1, "q3": q3, "min": min(v), "max": max(v)}
    out = {f"ms_per_step_{k}": round(have[k], 3) for k in stats}
    if batch is not None:
        out["images_per_s"] = round(batch / med * 1e3, 1)
    out["all_ms"] = [round(t, 3) for t in v]
    return out


def speedup_median(on, off, places=3):
    return round(off["ms_per_step_median"] / on["ms_per_step_median"], places)


def verdict(on, off, rule, report=("faster", "slower")):
    """From two arm summaries: the run-to-run spread by `rule` - "range": the larger max - min of the two arms; "iqr_off": the
    interquartile range of the flag-off arm - the speed-up of the medians, and whether the flag-on arm's median is `report`ed faster /
    slower than the flag-off arm's by more than that spread."""
    if rule == "range":
        spread = max(on["ms_per_step_max"] - on["ms_per_step_min"], off["ms_per_step_max"] - off["ms_per_step_min"])
    elif rule == "iqr_off":
        spread = off["ms_per_step_q3"] - off["ms_per_step_q1"]
    else:
        raise ValueError(f"spread rule {rule!r}: 'range' or 'iqr_off'")
    gain = off["ms_per_step_median"] - on["ms_per_step_median"]
    out = {"run_to_run_spread_ms": round(spread, 3), "speedup_median": speedup_median(on, off)}
    out.update({f"flag_on_{k}_beyond_spread": bool((gain if k == "faster" else -gain) > spread) for k in report})
    return out


# ------------------------------------------------------------------------------------------- nodes and launches alone
def node_times(plan, x, cls, reps=20, repeats=1):
    """[(name, module, its positional inputs, ms per launch)] per `cls` node of `plan`: the inputs caught in one run of `plan(x)`, then
    `reps` launches of the node alone between two events after 3 warm-ups (`repeats` > 1: a list of that many such times)."""
    seen, hooks, rows = {}, [], []
    for name, m in plan.named_modules():
        if isinstance(m, cls):
            hooks.append(m.register_forward_pre_hook(lambda mod, a, name=name: seen.__setitem__(name, a)))
    plan(x)
    for h in hooks:
        h.remove()
    mods = dict(plan.named_modules())
    for name, a in seen.items():
        run = lambda _, m=mods[name], a=a: m(*a)  # noqa: E731
        timed(run, None, 3)
        ms = [timed(run, None, reps) for _ in range(repeats)]
        rows.append((name, mods[name], a, ms if repeats > 1 else ms[0]))
    return rows


def profile_step(plan, x, warm=True):
    """[(tag, algorithmic bytes, ms, operations)] of every launch of one step of `plan` with the launch profile (K.PROFILE) on, after one
    step without it (`warm`)."""
    if warm:
        plan(x)
    K.PROFILE.reset()
    K.PROFILE.enabled = True
    try:
        plan(x)
        torch.cuda.synchronize()
        return [(r[0], r[1], r[2].elapsed_time(r[3]), r[4]) for r in K.PROFILE.records]
    finally:
        K.PROFILE.enabled = False
        K.PROFILE.reset()


def launch_sum(recs, tag, elements=None):
    """The launches tagged `tag` among profile_step's records: how many, their time, bytes and bytes per second (with `elements`: those
    and elements per second)."""
    mine = [r for r in recs if r[0] == tag]
    ms, nbytes = sum(r[2] for r in mine), sum(r[1] for r in mine)
    rate = lambda n, unit: round(n / (ms * 1e-3) / unit, 1) if ms else None  # noqa: E731
    out = {"launches": len(mine), "us": round(ms * 1e3, 1), "bytes": nbytes}
    if elements is None:
        return dict(out, gb_per_s=rate(nbytes, 1e9))
    return dict(out, elements=elements, gb_per_s=rate(nbytes, 1e9), gelem_per_s=rate(elements, 1e9))


def kernel_profile(plan, x, tags, warm=False):
    """{tag: launch_sum} of one profiled step of `plan` for `tags` = {K.PROFILE tag: its node class}; the elements are the fp32 elements
    those nodes read in that step."""
    if warm:
        plan(x)
    elems = {t: 0 for t in tags}
    hooks = [m.register_forward_pre_hook(lambda mod, a, t=t: elems.__setitem__(t, elems[t] + a[0].numel()))
             for m in plan.modules() for t, cls in tags.items() if isinstance(m, cls)]
    try:
        recs = profile_step(plan, x, warm=False)
    finally:
        for h in hooks:
            h.remove()
    return {t: launch_sum(recs, t, elems[t]) for t in tags}


# ------------------------------------------------------------------------------------------- the command line and the record
def arguments(doc, **defaults):
    """The tools' command line: the optional positional integers named in `defaults`, in that order, and --out PATH."""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    for name, default in defaults.items():
        ap.add_argument(name, nargs="?", type=int, default=default)
    ap.add_argument("--out", metavar="PATH", help="write the JSON here instead of the tool's own place")
    return ap.parse_args()


def write_profile(name, out, path=None, quiet=False):
    """Print `out` as JSON (not with `quiet`) and write it to `path`, or to profiles/<name>.json; a tool that only prints passes no name."""
    text = json.dumps(out, indent=1)
    if path is None and name is not None:
        os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
        path = os.path.join(ROOT, "profiles", name + ".json")
    if path is not None:
        with open(path, "w") as f:
            f.write(text + "\n")
    if not quiet:
        print(text)
