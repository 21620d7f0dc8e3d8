"""Render the plan `fuse_inference` returns as text (a helper, not a test): per graph node its op, target and arguments, then per plan
module what the later passes and the kernels' wrappers read off it, and the fusion report.  Two plans with the same text launch the
same kernels with the same options in the same order.  Public attributes only: the same text comes out of any version of the plan
builder that builds the same plan.  tests/golden/plans/ holds one such text per case of tests/test_plan_snapshot_host.py."""
import torch.fx as fx

ATTRS = ("relu", "relu6", "want_out", "pool", "k", "c", "k_pad", "c_pad", "kind", "narrow", "pad_shortcut", "emit_shift", "out_cm",
         "want_codes", "swapped", "defer_out", "recompute", "window", "pad_code", "rows", "merged", "flatten", "scale", "sdpa", "channels",
         "grid", "patch", "tokens")
PARTS = ("a", "b", "short", "main", "dw", "pw")       # the plan layers a wrapper node (dual, chain, depthwise + pointwise, head) holds


def _target(t):
    return t if isinstance(t, str) else f"{getattr(t, '__module__', '')}.{getattr(t, '__qualname__', getattr(t, '__name__', repr(t)))}"


def _arg(a):
    if isinstance(a, fx.Node):
        return a.name
    if isinstance(a, (tuple, list)):
        return "(" + ", ".join(_arg(v) for v in a) + ")"
    if isinstance(a, slice):
        return f"slice({_arg(a.start)}, {_arg(a.stop)}, {_arg(a.step)})"
    return repr(a)


def _from_plan_builder(m):
    return type(m).__module__.startswith("dlmc.utils.fuse")


def module_text(m):
    """Class name and the attributes of ATTRS the module has (plus its quantisers' keys and whether its weights are symmetric)."""
    fields = [f"{name}={getattr(m, name, None)!r}" for name in ATTRS if hasattr(m, name)]
    for name in ("emit", "act"):
        if hasattr(m, name):
            q = getattr(m, name, None)
            fields.append(f"{name}.key={getattr(q, 'key', None)!r}")
    if hasattr(m, "w_off"):
        fields.append(f"w_off is None={getattr(m, 'w_off', None) is None}")
    if hasattr(m, "norm"):
        fields += [f"norm.{name}={getattr(m.norm, name)!r}" for name in ("normalized_shape", "eps")]
    if hasattr(m, "decision"):       # a pass's record (a namedtuple): node names and numbers; a quantiser by its key
        fields += [f"decision.{name}={getattr(v, 'key', v)!r}" for name, v in m.decision._asdict().items()]
    return f"{type(m).__name__}({', '.join(fields)})"


def plan_text(gm):
    mods = dict(gm.named_modules())
    lines, nodes_of = [], {}        # the text of a plan module (and of the plan layers it holds) -> the nodes that call one like it
    for n in gm.graph.nodes:
        kwargs = "".join(f", {k}={_arg(v)}" for k, v in n.kwargs.items())
        lines.append(f"{n.name} = {n.op} {_target(n.target)}({', '.join(_arg(a) for a in n.args)}{kwargs})")
        m = mods.get(n.target) if n.op == "call_module" else None
        if m is not None and _from_plan_builder(m):
            parts = [(part, getattr(m, part, None)) for part in PARTS]
            text = "".join(f"\n      .{part}: {module_text(p)}" for part, p in parts if p is not None and _from_plan_builder(p))
            nodes_of.setdefault(f"    {module_text(m)}{text}", []).append(n.name)
    for text, names in nodes_of.items():      # (modules that read the same are listed once, under the names of their nodes)
        lines += [" ".join(names) + ":", text]
    lines.append(repr(gm.fusion_report))
    return "\n".join(lines) + "\n"
