"""Swin's row geometry on the host: every refusal of dlmcq_layernorm_gather_rows_f32 and dlmcq_window_reverse_add_f32 returns its code
before anything is launched, the three wrappers refuse what they cannot read in place, and fuse_inference(swin_geometry=True) plans
the nodes of a small SwinNet (8 x 8 map, then 4 x 4) and nothing without the flag."""
import ctypes
import types

import pytest
import torch

import workloads as W
from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from dlmc.utils.fuse import MergeNormLayer, WindowAddLayer, WindowNormLayer, fuse_inference
from test_relu6_host import calibrated as fsptq

FLAGS = dict(dry_run=True, layer_norms=True, gelu=True, window_attention=True)
P = lambda v: None if v is None else ctypes.c_void_p(v)  # noqa: E731


def small_swin():
    return fsptq(W.SwinNet(10, 64, (2, 2), (2, 4), 4, 32, 4))


def gather(x=1 << 12, out=1 << 13, codes=1 << 14, mode=N.GATHER_WINDOW, b=2, hm=6, wm=9, c=8, sb=None, sy_=None, sx_=None, ws=3, sy=1, sx=2,
           eps=1e-5, scale=1 << 15, form=N.FORM_ZEROPOINT, gamma=1 << 16):
    sx_ = c if sx_ is None else sx_
    sy_ = wm * sx_ if sy_ is None else sy_
    sb = hm * sy_ if sb is None else sb
    return N.lib.dlmcq_layernorm_gather_rows_f32(P(x), P(gamma), None, P(out), P(codes), mode, b, hm, wm, c, sb, sy_, sx_, ws, sy, sx, eps,
                                                 P(scale), None, 0, 255, form, 0.0, None)


def reverse(yw=1 << 12, sc=1 << 16, out=1 << 20, b=2, hm=6, wm=9, c=8, s=None, o=None, ws=3, sy=1, sx=2):
    dense = (hm * wm * c, wm * c, c)
    return N.lib.dlmcq_window_reverse_add_f32(P(yw), P(sc), P(out), b, hm, wm, c, *(s or dense), *(o or dense), ws, sy, sx, None)


MERGE = dict(mode=N.GATHER_MERGE, hm=4, wm=6, ws=0, sy=0, sx=0)
GATHER_REFUSED = {
    "mode": (dict(mode=2), -1), "c_below_4": (dict(c=0), -1), "c_mod_4": (dict(c=6), -1), "row_too_wide": (dict(c=2052), -1),
    "merge_row_too_wide": (dict(MERGE, c=516), -1), "ws_0": (dict(ws=0), -1), "hm_mod_ws": (dict(hm=7), -1), "wm_mod_ws": (dict(wm=10), -1),
    "sy_out": (dict(sy=6), -1), "sx_out": (dict(sx=9), -1), "sy_negative": (dict(sy=-1), -1), "merge_odd_hm": (dict(MERGE, hm=5), -1),
    "merge_odd_wm": (dict(MERGE, wm=7), -1), "merge_shift": (dict(MERGE, sy=1), -1), "stride_mod_4": (dict(sx_=10), -1),
    "stride_short": (dict(sx_=4), -1), "line_stride_mod_4": (dict(sy_=74), -1), "eps_0": (dict(eps=0.0), -1), "eps_nan": (dict(eps=float("nan")), -1),
    "shifted_codes": (dict(form=N.FORM_ZEROPOINT | N.EMIT_SHIFT128), -1), "codes_without_scale": (dict(scale=None), -1),
    "null_x": (dict(x=None), -1), "nothing": (dict(out=None, codes=None), -1), "x_align": (dict(x=(1 << 12) + 4), -4),
    "gamma_align": (dict(gamma=(1 << 16) + 8), -4), "codes_align": (dict(codes=(1 << 14) + 2), -4),
    "m_2_31": (dict(b=1 << 31, hm=1, wm=1, ws=1, sy=0, sx=0), -2), "quads_2_31": (dict(b=1 << 22, hm=1, wm=1, ws=1, sy=0, sx=0, c=2048), -2),
}
REVERSE_REFUSED = {
    "c_mod_4": (dict(c=6), -1), "ws_0": (dict(ws=0), -1), "hm_mod_ws": (dict(hm=7), -1), "sy_out": (dict(sy=6), -1), "sx_out": (dict(sx=-1), -1),
    "shortcut_stride_mod_4": (dict(s=(6 * 9 * 10, 9 * 10, 10)), -1), "out_stride_short": (dict(o=(6 * 9 * 8, 9 * 8, 4)), -1),
    "null_yw": (dict(yw=None), -1), "null_out": (dict(out=None), -1), "out_align": (dict(out=(1 << 20) + 4), -4),
    "out_meets_yw": (dict(out=(1 << 12) + 64), -1), "out_is_the_shortcut": (dict(out=1 << 16), -1),
    "pixels_2_31": (dict(b=1 << 31, hm=1, wm=1, ws=1, sy=0, sx=0), -2),
}


@pytest.mark.parametrize("name", sorted(GATHER_REFUSED))
def test_gather_refusals(name):
    kw, code = GATHER_REFUSED[name]
    assert gather(**kw) == code


@pytest.mark.parametrize("name", sorted(REVERSE_REFUSED))
def test_reverse_add_refusals(name):
    kw, code = REVERSE_REFUSED[name]
    assert reverse(**kw) == code


def test_empty_problems_launch_nothing():
    assert gather(b=0) == gather(b=0, x=None, out=None, codes=None, scale=None) == gather(**dict(MERGE, b=0)) == 0
    assert reverse(b=0) == reverse(b=0, yw=None, sc=None, out=None) == 0
    assert gather(b=0, ws=0) == reverse(b=0, ws=0) == -1      # (the geometry is checked first)


def test_the_wrappers_refuse_what_they_cannot_read_in_place():
    x, w = torch.zeros(2, 6, 9, 8), torch.zeros(8)
    for bad in (x.double(), x[..., ::2], x[:, :, :, 1:5], torch.zeros(2, 54, 8), torch.zeros(2, 6, 9, 6)):
        for call in (lambda t: K.layernorm_window_quant(t, None, None, 1e-5, 3, 0), lambda t: K.layernorm_merge_quant(t, None, None, 1e-5),
                     lambda t: K.window_reverse_add(torch.zeros(12, 9, 8), t, 3, 0)):
            with pytest.raises(ValueError, match="read in place"):
                call(bad)
    with pytest.raises(ValueError, match="do not fit"):
        K.layernorm_window_quant(x, w, w, 1e-5, 4, 0)
    with pytest.raises(ValueError, match="do not fit"):
        K.window_reverse_add(torch.zeros(12, 9, 8), x, 3, (6, 0))
    with pytest.raises(ValueError, match="shift is an int or a pair"):
        K.layernorm_window_quant(x, w, w, 1e-5, 3, 1.5)
    with pytest.raises(ValueError, match="no 2 x 2 merge"):
        K.layernorm_merge_quant(x, None, None, 1e-5)
    with pytest.raises(ValueError, match=r"weight of shape \(32,\)"):
        K.layernorm_merge_quant(torch.zeros(2, 6, 8, 8), w, None, 1e-5)
    with pytest.raises(ValueError, match="at most 2048"):
        K.layernorm_merge_quant(torch.zeros(1, 2, 2, 516), None, None, 1e-5)
    with pytest.raises(ValueError, match="nothing to produce"):
        K.layernorm_window_quant(x, w, w, 1e-5, 3, 0, want_out=False)
    with pytest.raises(ValueError, match="window rows"):
        K.window_reverse_add(torch.zeros(12, 9, 4), x, 3, 0)
    with pytest.raises(N.DlmcqError, match="no CPU fallback"):      # (what is left for a well-formed call without a device)
        K.layernorm_window_quant(x, w, w, 1e-5, 3, (1, 2))


def test_the_plan_takes_a_swin_stage():
    plan = fuse_inference(small_swin(), swin_geometry=True, **FLAGS)
    rep = plan.fusion_report
    assert (rep.window_norms, rep.window_adds, rep.merge_norms, rep.window_attentions) == (4, 4, 1, 4)
    norms = [m for m in plan.modules() if isinstance(m, WindowNormLayer)]
    adds = [m for m in plan.modules() if isinstance(m, WindowAddLayer)]
    want = [((8, 8), 4, (0, 0), 64), ((8, 8), 4, (2, 2), 64), ((4, 4), 4, (0, 0), 128), ((4, 4), 4, (0, 0), 128)]
    assert [(m.hw, m.window, m.shift, m.c) for m in norms] == [(m.hw, m.window, m.shift, m.c) for m in adds] == want
    merge, = [m for m in plan.modules() if isinstance(m, MergeNormLayer)]
    assert (merge.hw, merge.c) == ((8, 8), 256) and not any(m.want_out for m in norms + [merge])
    assert "window norms on the plan=4" in repr(rep) and not any(n.op == "call_function" and n.target in (torch.roll, torch.cat) for n in plan.graph.nodes)


def test_flag_off_is_the_default_plan():
    plain, off = fuse_inference(small_swin(), **FLAGS), fuse_inference(small_swin(), swin_geometry=False, **FLAGS)
    assert repr(plain.fusion_report) == repr(off.fusion_report) and str(plain.graph) == str(off.graph)
    assert (off.fusion_report.window_norms, off.fusion_report.window_adds, off.fusion_report.merge_norms) == (0, 0, 0)


def test_another_permutation_is_not_taken():
    """A block whose partition and reverse permute (0, 3, 1, 2, 4, 5) - windows in column-major order - keeps its own ops; the other
    blocks and the merge are taken."""
    def forward(self, x):
        c, w, side = self.dim, self.window, self.side
        g = side // w
        h = self.norm1(x).view(-1, side, side, c).reshape(-1, g, w, g, w, c).permute(0, 3, 1, 2, 4, 5).reshape(-1, w * w, c)
        h = self.attn(h).reshape(-1, g, g, w, w, c).permute(0, 2, 3, 1, 4, 5).reshape(-1, side, side, c)
        x = h.view(-1, side * side, c) + x
        return self.fc2(self.act(self.fc1(self.norm2(x)))) + x
    net = small_swin()
    net.stages[0].forward = types.MethodType(forward, net.stages[0])
    rep = fuse_inference(net, swin_geometry=True, **FLAGS).fusion_report
    assert (rep.window_norms, rep.window_adds, rep.merge_norms) == (3, 3, 1)
