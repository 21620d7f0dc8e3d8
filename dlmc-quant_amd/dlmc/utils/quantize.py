"""`quantize_model`: swap nn.Conv2d / nn.Linear for the HIP-backed quant wrappers, in place
(reference: dlmc/utils/quantize.py:61-143 - same signature, same config schema, same swap mechanism:
`__new__` + `__dict__.update` + `initialize`, so parameters, hooks and buffers of the original layer
carry over and `state_dict` keys stay what the reference's checkpoints expect)."""
import contextlib
import copy
import math
from operator import attrgetter
from typing import Dict

import torch
from torch import nn

from ..quantization.scalar import FSPTQuant as FSPQ
from ..quantization.scalar import RootQ as RQ
from ..quantization.scalar import modules as qnn
from ..quantization.scalar import _wrapper as _W
from ..quantization.scalar import kernels as K
from .. import _native as N
from .access import attrsetter, get_layers

__all__ = ["quantize_model", "WeightQuantBatch"]

MODULE_MAPPING = {nn.Conv2d: qnn.QConv2d, nn.Linear: qnn.QLinear}
ROOTQ_MAPPING = {nn.Conv2d: RQ.RootQConv2d, nn.Linear: RQ.RootQLinear}
FSPTQUANT_MAPPING = {nn.Conv2d: FSPQ.FSPTQConv2d, nn.Linear: FSPQ.FSPTQLinear}
_FAMILIES = {None: MODULE_MAPPING, "RootQ": ROOTQ_MAPPING, "FSPTQ": FSPTQUANT_MAPPING}


def _override_options(dst_config: Dict, src_config: Dict = None) -> Dict:
    """Per-layer override of {type, enable, args} (reference: quantize.py:44-58)."""
    if src_config is None:
        return dst_config
    merged = copy.deepcopy(dst_config)
    for key in ("type", "enable"):
        if key in src_config:
            merged[key] = src_config[key]
    if "args" in src_config:
        merged["args"].update(src_config["args"])
    return merged


def quantize_model(model: nn.Module, config: Dict, logger=None, quantization_type: str = None, **kwargs) -> None:
    """Quantise `model` in place.

    :param config: the `quantization:` section of the YAML (weight / input / exclude_layers /
                   override_options [/ momentum])
    :param quantization_type: None (QBase family), "RootQ" or "FSPTQ".  "BitMixer" and "MetaQ" name
                   packages that are missing from the reference itself (quantize.py:10,12).
    """
    if quantization_type in ("BitMixer", "MetaQ"):
        raise NotImplementedError(f"quantization_type={quantization_type!r}: its package is absent from the reference")
    mapping = _FAMILIES.get(quantization_type, MODULE_MAPPING)
    momentum = config["momentum"] if quantization_type == "RootQ" else 0.1

    candidates = get_layers(model, filter_types=tuple(mapping.keys()))
    excluded = set()
    for regexp in config.get("exclude_layers") or []:
        excluded.update(get_layers(model, filter_regexp=regexp))

    overrides = {}
    for opt in config.get("override_options") or []:
        for regexp in opt.get("layers") or []:
            for name in get_layers(model, filter_regexp=regexp):
                assert name not in overrides, f"layer {name} is overridden twice"
                overrides[name] = opt["options"]

    for name in candidates:
        if name in excluded:
            continue
        layer = attrgetter(name)(model)
        if type(layer) not in mapping:     # an already-quantised subclass, or a foreign subclass
            continue
        weight_cfg, input_cfg = config["weight"], config["input"]
        if name in overrides:
            weight_cfg = _override_options(weight_cfg, overrides[name].get("weight"))
            input_cfg = _override_options(input_cfg, overrides[name].get("input"))
        layer_cfg = {"input": copy.deepcopy(input_cfg), "weight": copy.deepcopy(weight_cfg), "momentum": momentum}
        if "int8_gemm" in kwargs or "int8_gemm" in config:   # opt-in fused int8 conv/linear (FSPTQ family)
            layer_cfg["int8_gemm"] = bool(kwargs.get("int8_gemm", config.get("int8_gemm")))
        cls = mapping[type(layer)]
        wrapped = cls.__new__(cls)
        wrapped.__dict__.update(layer.__dict__)
        wrapped.initialize(layer_cfg)
        attrsetter(name)(model, wrapped)
        if logger is not None:
            logger.info("Quantize module {} with method <input: {}> <weight: {}>".format(
                name, layer_cfg["input"], layer_cfg["weight"]))


class WeightQuantBatch:
    """Fake-quantise ALL of a model's weights in one launch per step, and run all their backward passes in one more
    (csrc/fake_quant_multi.hip), instead of one launch per layer in the forward and two per layer in the backward:

        wqb = WeightQuantBatch(model)            # after the calibrating forward (or call wqb.refresh() after it)
        with wqb.step():
            loss = criterion(model(x), y)
        loss.backward(); optimizer.step()

    Members are the QBase / FSPTQBase wrappers whose weight quantiser is enabled and calibrated, is not AdaRound / dist_recon,
    and whose weight the segment table takes (fp32, contiguous, 16-byte aligned, at most 8 388 608 elements); every other
    wrapper is listed in `.skipped` (module name -> reason) and runs as it does without the handle.  Inside the step a member's
    forward takes its tensor from `wqb.outputs` where it would launch its own weight fake-quant - the same bits - unless its
    weight or scale was written to since the launch, or the layer takes its int8 route.  Outside a step nothing changes.

    The outputs live in an arena the handle owns and are overwritten by the next step: run a step's backward before opening
    the next one (autograd reports a graph that still holds overwritten outputs).  Optimisers update weights and scales in
    place, so the forward table is uploaded once; `refresh()` rebuilds it (new calibration, replaced parameters)."""

    def __init__(self, model):
        self.model = model
        self.outputs = {}
        self.refresh()

    # -------------------------------------------------------------------------- membership
    @staticmethod
    def _segment(mod):
        """(K.Segment, None) for a member, (None, reason) otherwise."""
        if isinstance(mod, RQ.base.RootQBase):
            return None, "RootQ: the weight transform has its own kernel and backward"
        if isinstance(mod, qnn.base.QBase):
            if not mod.qconfig["weight"]["enable"]:
                return None, "weight quantiser disabled"
            form, offset = N.FORM_QBASE, mod.wt_offset
            g = 1 / math.sqrt(mod.weight.numel() * mod.wt_max_val)
        else:
            if not mod.wt_quant:
                return None, "weight quantiser disabled"
            if mod.qconfig["weight"].get("recon_type") in ("adaround", "dist_recon"):
                return None, "AdaRound / dist_recon: the soft-rounding kernel, not a fake-quant"
            form, offset, g = N.FORM_SYMMETRIC, None, 0.0
        if not mod._init.ready(mod, "wt_init_state"):
            return None, "not calibrated yet (refresh() after the first forward)"
        try:
            seg = K.Segment(mod.weight, mod.wt_scale, offset, mod.wt_min_val, mod.wt_max_val, form, g)
        except ValueError as e:
            return None, f"not eligible: {e}"
        why = K.segment_refusal(seg)
        if why is not None:
            return None, f"not eligible: {why}"
        return seg, None

    def refresh(self):
        """Collect the members again (module order) and drop the cached tables."""
        self.members, self.skipped, self._segments = [], {}, {}
        for name, mod in self.model.named_modules():
            if not isinstance(mod, (qnn.base.QBase, FSPQ.base.FSPTQBase, RQ.base.RootQBase)):
                continue
            seg, why = self._segment(mod)
            if seg is None:
                self.skipped[name] = why
            else:
                self.members.append(mod)
                self._segments[mod] = seg
        self._plans = {}
        return self

    def _signature(self, mods):
        return tuple((m.weight.data_ptr(), m.wt_scale.data_ptr(), id(getattr(m, "wt_offset", None))) for m in mods)

    def _plan(self, mods):
        """The uploaded table of `mods`, rebuilt only when a weight, scale or offset moved."""
        key = tuple(id(m) for m in mods)
        sig = self._signature(mods)
        hit = self._plans.get(key)
        if hit is None or hit[0] != sig:
            for m in mods:
                self._segments[m] = self._segment(m)[0] or self._segments[m]
            hit = (sig, K.FqMultiPlan([self._segments[m] for m in mods]))
            self._plans[key] = hit
        return hit[1]

    # -------------------------------------------------------------------------------- step
    @contextlib.contextmanager
    def step(self):
        grad = torch.is_grad_enabled()
        # without autograd a layer on its int8 route never reads a fake-quantised weight: leave those out
        mods = [m for m in self.members if grad or not m.int8_gemm]
        if mods:
            plan = self._plan(mods)
            tensors = [m.weight for m in mods] + [m.wt_scale for m in mods]
            if grad and any(t.requires_grad for t in tensors):
                ys = _W.MultiFakeQuantFn.apply(plan, *tensors)
            else:
                ys = plan.forward()
            self.outputs = dict(zip(mods, ys))
            self._stamp = {m: (m.weight._version, m.wt_scale._version, m._init.marks) for m in mods}
        outer, _W.ACTIVE_WEIGHT_BATCH = _W.ACTIVE_WEIGHT_BATCH, self
        try:
            yield self
        finally:
            _W.ACTIVE_WEIGHT_BATCH = outer
            self.outputs = {}

    def take(self, mod):
        y = self.outputs.get(mod)
        if y is None or self._stamp[mod] != (mod.weight._version, mod.wt_scale._version, mod._init.marks):
            return None
        return y
