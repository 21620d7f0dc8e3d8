"""The host side of the 5 x 5 depthwise kernel (csrc/conv_dw5_i8.hip), no GPU: the header and the ctypes table carry
dlmcq_conv2d_dw5_i8_nhwc; its table holds the six records written out by hand in tests/dw5_cases.py and every one is reached by a route
query of that module's cases; its refusals on placeholder pointers, in dlmcq_conv2d_dw_i8_nhwc's order of precedence; the old entry point's
tables and its answer for a 5 x 5 layer are what they were; and the plan builder's decisions under fuse_inference(dw5=...) on
workloads.efficientnet_b0() and small MBConv networks (dry run, wrappers marked calibrated by hand as in test_relu6_host.py)."""
import os
import re

import torch
from torch import nn

import dw5_cases as W5
import dw_variant_cases as W
import test_dw_stem_refusals_host as D
import workloads as WL
from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from dlmc.quantization.scalar.modules.base import QBase
from dlmc.utils.fuse import fuse_inference
from dlmc.utils.quantize import quantize_model
from plan_dump import plan_text
from test_act_offset_host import QBASE_W4A8
from test_relu6_host import calibrated as fsptq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = W5.ROUTE_ONLY | W5.ROUTE_DW_VARIANT


def test_header_and_signatures_carry_the_symbol():
    text = open(os.path.join(ROOT, "include", "dlmcq.h")).read()
    m = re.search(r"int dlmcq_conv2d_dw5_i8_nhwc\(([^;]*)\);", text)
    assert m and "dlmcq_x_dw5_variant_table" not in text
    params = [p.strip() for p in m.group(1).split(",")]
    res, args = N.SIGNATURES["dlmcq_conv2d_dw5_i8_nhwc"]
    assert len(params) == len(args) == len(W5.ENTRY) == len(N.SIGNATURES["dlmcq_conv2d_dw_i8_nhwc"][1]) - 2      # ... minus R, S
    assert "DLMCQ_ROUTE_DW5_VARIANT_TAG (1 << 29)" in text and N.ROUTE_DW5_VARIANT_TAG == 1 << 29
    assert "conv_dw5_i8.hip" in open(os.path.join(ROOT, "dlmc-quant_amd", "csrc", "Makefile")).read()


def test_the_table_is_the_six_records_and_every_one_is_reached():
    table = N.dw5_variant_table()
    assert len(table) == len(set(table)) == 6 and sorted(table) == sorted(W5.RECORDS)
    got = {c.cid: W5.decode(W5.call(N.lib, W5.route_args(c))) for c in W5.CASES}
    assert not {k: (v, c.record) for (k, v), c in zip(got.items(), W5.CASES) if v != c.record}
    assert set(got.values()) == set(table)
    for c in W5.CASES:           # the header's encoding, spelt out; and the tag collides with no other decoder's
        rc = W5.call(N.lib, W5.route_args(c))
        assert rc == (1 << 29) | (c.record[1] << 4) | (1 if c.record[2] else 0)
        assert N.decode_dw_variant(rc) is None and N.decode_variant(rc) is None and N.decode_halo_variant(rc) is None
    for rc in (D.ROUTE_DW, D.ROUTE_DWM, 0, D.EINVAL, (1 << 27) | (2 << 8), (1 << 28) | (4 << 8), (1 << 29) | (3 << 4), (1 << 29) | 2, 1 << 30):
        assert N.decode_dw5_variant(rc) is None, rc


def test_the_cases_cover_what_the_case_module_promises():
    used = {tuple(sorted(c.geo.items())) for c in W5.CASES}
    assert used == {tuple(sorted(g.items())) for g in W5.GEOS + [W5.GRID_STRIDE]} and len(W5.GEOS) == 16
    geos = W5.GEOS
    assert {(g["H"], g["W"]) for g in geos} >= {(1, 1), (2, 3), (4, 4), (5, 5), (6, 7), (9, 9)}
    assert {(g["H"], g["W"]) for g in geos if g["stride"] == 2} >= {(7, 8), (8, 9), (9, 7), (9, 8)}
    out_w = {(g["W"] - 1) // g["stride"] + 1 for g in geos}
    assert out_w >= {1, 2, 3, 5} and {g["C"] for g in geos} == {16, 48, 64, 2048} and {g["N"] for g in geos} == {1, 3}
    assert all(K.dw5_supported(g["C"], g["stride"], g["pad"], g["R"]) for g in geos)
    g = W5.GRID_STRIDE
    threads = W5.GRID_CAP * W5.BLOCK
    assert threads < g["N"] * g["H"] * g["W"] * (g["C"] // 16) < 2 * threads and g["stride"] == 1
    for r in W5.RECORDS:
        cs = [c for c in W5.BY_RECORD[r] if "grid_stride" not in c.cid]
        zps = {(c.uns, c.zp) for c in cs}
        assert zps == {(True, 0), (True, 200), (False, -37), (True, 77), (False, 0)}, r
        assert sum(not c.bias for c in cs) == 1 and cs[0].quant.endswith("_hi") and all((c.act == 2) == r[2] for c in cs), r
        if r[1]:
            assert all(c.quant.startswith("plain") and not c.out and c.asym == (r[1] == 1) for c in cs), r
        else:
            assert {c.asym for c in cs} == {True, False} and any(c.out and c.quant is None for c in cs) and any(c.out and c.quant for c in cs), r
            assert {c.quant.split("_")[0] for c in cs if c.quant} >= {"uzp", "signed"}, r
        if not r[2]:
            assert {c.act for c in cs} == {0, 1}, r
        f = W5.FULL_RANGE[r]
        assert (f["act"] == 2) == r[2] and f["quant"].endswith("_hi") and (r[1] == 0) == f["out"], r


def test_refusals_on_placeholder_pointers():
    call = lambda **kw: W5.call(N.lib, kw)       # noqa: E731
    assert call(q_form=D.ZP | Q) == (1 << 29) | (2 << 4)          # the base call is accepted: FAST 2
    for kw in (dict(stride=3), dict(stride=0), dict(pad=1), dict(pad=3), dict(C=24), dict(C=2064), dict(C=8), dict(H=0), dict(W=0), dict(N=-1),
               dict(q_form=D.ZP | D.FORCE_TILED), dict(q_form=D.ZP | W5.ROUTE_ONLY), dict(q_form=D.ZP | W5.ROUTE_DW_VARIANT),
               dict(q_form=D.ZP | D.BITS["PIPELINED"]), dict(q_form=D.ZP | D.BITS["SHIFT128"]), dict(q_form=D.ZP | Q | D.FORCE_TILED),
               dict(q_scale=0), dict(x=0), dict(s_w=0), dict(out=0, codes=0), dict(q_lo=5, q_hi=-5)):
        assert call(**kw) == D.EINVAL, kw
        assert call(**dict(kw, x=kw.get("x", D.P4))) == D.EINVAL, kw                     # ... before the alignment
        assert call(**dict(kw, N=kw.get("N", 1 << 20), H=kw.get("H", 64), W=kw.get("W", 64))) == D.EINVAL, kw      # ... and before the size bound
    # P < 1 cannot be reached with padding 2 but through H < 1; an empty problem is answered before the pointers are looked at
    assert call(N=0) == D.OK and call(N=0, x=0, codes=0, q_form=D.ZP | Q) == D.OK and call(N=0, stride=3) == D.EINVAL and call(N=0, C=24) == D.EINVAL
    for kw in (dict(x=D.P4), dict(codes=D.P4), dict(s_w=D.P4), dict(bias=D.P4), dict(w_off=D.P4), dict(out=D.P4)):
        assert call(**kw) == D.EALIGN, kw
        assert call(**dict(kw, N=1 << 20, H=64, W=64)) == D.EALIGN, kw                   # alignment before the size bound
        assert call(**dict(kw, q_form=D.ZP | Q)) == D.EALIGN, kw                         # ... and before the route
    assert call(w=D.P4, N=1 << 20, H=64, W=64) == D.ERANGE                              # (the weights: bytes, read one at a time)
    assert call(N=1 << 20, H=64, W=64) == D.ERANGE and call(N=1 << 20, H=64, W=64, q_form=D.ZP | Q) == D.ERANGE      # 2^31 work items
    assert call(N=(1 << 15) - 1, H=64, W=64, q_form=D.ZP | Q) > 0
    assert call(C=2048, q_form=D.ZP | Q) > 0 and call(stride=2, q_form=D.ZP | Q) > 0


def test_the_old_entry_point_is_what_it_was():
    dw, dwm = N.dw_variant_tables()
    assert [len(dw), len(dwm)] == [26, 8]
    fn = N.experimental("dlmcq_x_dw_variant_table", [N.ctypes.c_int, N.ctypes.POINTER(N.ctypes.c_int32), N.ctypes.c_int])
    assert fn(2, None, 0) == -1
    for kw in (dict(), dict(stride=2), dict(C=2048), dict(out=D.P), dict(relu=2)):
        a = dict(kw, R=5, S=5, pad=2, q_form=D.ZP | Q)
        assert W.decode(D.call(N.lib, "dw_i8_nhwc", a))[:3] == ("dw", "generic", 0), kw
        assert D.call(N.lib, "dw_i8_nhwc", dict(a, q_form=D.ZP | W5.ROUTE_ONLY)) == D.ROUTE_DW, kw


def test_dw5_supported_restates_the_entry_point():
    for c in (16, 24, 64, 2048, 2064):
        for stride in (1, 2, 3):
            for pad in (1, 2, 3):
                rc = W5.call(N.lib, dict(C=c, stride=stride, pad=pad, q_form=D.ZP | Q))
                assert K.dw5_supported(c, stride, pad, 5) == (rc > 0), (c, stride, pad, rc)
    assert not K.dw5_supported(64, 1, 2, 3) and not K.dw5_supported(64, 1, 2, 7) and K.dw5_profitable(704, 14, 14, 1)


# ------------------------------------------------------------------------------------------- the plan builder
class _MBConvs(nn.Module):
    """Three MBConv blocks (workloads.InvertedResidual): 5x5 / 1 with squeeze-excite and swish, 5x5 / 2 with ReLU6, 3x3 with ReLU6."""

    def __init__(self):
        super().__init__()
        self.first = WL._conv_bn_act(8, 16, 3, act="swish")
        self.a = WL.InvertedResidual(16, 24, 1, 6, se=True, act="swish", k=5)
        self.b = WL.InvertedResidual(24, 32, 2, 6, se=False, act="relu6", k=5)
        self.c = WL.InvertedResidual(32, 32, 1, 6, se=False, act="relu6")

    def forward(self, x):
        return self.c(self.b(self.a(self.first(x))))


def test_inverted_residual_takes_a_5x5_filter_with_its_padding():
    net = _MBConvs()
    dws = [m for m in net.modules() if isinstance(m, nn.Conv2d) and m.groups == m.in_channels > 1]
    assert [(m.kernel_size, m.padding, m.stride) for m in dws] == [((5, 5), (2, 2), (1, 1)), ((5, 5), (2, 2), (2, 2)), ((3, 3), (1, 1), (1, 1))]
    assert WL.mobilenet_v2().features[3].conv[1][0].kernel_size == (3, 3)           # the default network is unchanged


def test_dw5_counts_the_layers_and_off_is_the_plan_as_it_was():
    make = _MBConvs
    on = fuse_inference(fsptq(make()), dry_run=True, gates=True, swish=True, dw5=True)
    off = fuse_inference(fsptq(make()), dry_run=True, gates=True, swish=True, dw5=False)
    plain = fuse_inference(fsptq(make()), dry_run=True, gates=True, swish=True)
    assert on.fusion_report.dw5 == 2 and "5x5 depthwise on the dot-product kernel=2" in repr(on.fusion_report)
    assert off.fusion_report.dw5 == 0 and "dot-product" not in repr(off.fusion_report)
    assert plan_text(off) == plan_text(plain)
    # the flag changes nothing but the kernel of those nodes: the same graph, the same options
    assert plan_text(on).replace("5x5 depthwise on the dot-product kernel=2, ", "") == plan_text(plain)
    assert on.fusion_report.layers == plain.fusion_report.layers and on.fusion_report.skipped == plain.fusion_report.skipped
    # MobileNetV2 has no 5x5 layer: nothing to take
    assert fuse_inference(fsptq(WL.mobilenet_v2()), dry_run=True, dw5=True).fusion_report.dw5 == 0


def test_efficientnet_b0_is_the_paper_network():
    net = WL.efficientnet_b0()
    dws = [m for m in net.modules() if isinstance(m, nn.Conv2d) and m.groups == m.in_channels > 1]
    assert len(dws) == 16 and sum(m.kernel_size == (5, 5) for m in dws) == 9
    assert all(m.padding == ((m.kernel_size[0] - 1) // 2,) * 2 for m in dws)
    five = [(m.in_channels, m.stride[0]) for m in dws if m.kernel_size == (5, 5)]
    assert five == [(144, 2), (240, 1), (480, 1), (672, 1), (672, 1), (672, 2), (1152, 1), (1152, 1), (1152, 1)]
    assert net.features[0][0].out_channels == 32 and net.features[0][0].stride == (2, 2) and net.features[-1][0].out_channels == 1280
    with torch.no_grad():
        assert net.eval()(torch.zeros(1, 3, 64, 64)).shape == (1, 1000)


def test_efficientnet_b0_dw5_counts_nine_and_off_is_the_plan_as_it_was():
    make = WL.efficientnet_b0
    on = fuse_inference(fsptq(make()), dry_run=True, gates=True, swish=True, dw5=True)
    off = fuse_inference(fsptq(make()), dry_run=True, gates=True, swish=True, dw5=False)
    plain = fuse_inference(fsptq(make()), dry_run=True, gates=True, swish=True)
    assert on.fusion_report.dw5 == 9 and off.fusion_report.dw5 == plain.fusion_report.dw5 == 0
    assert plan_text(off) == plan_text(plain)
    assert plan_text(on).replace("5x5 depthwise on the dot-product kernel=9, ", "") == plan_text(plain)


class _Net(nn.Module):
    def __init__(self, c, pad):
        super().__init__()
        self.a = nn.Conv2d(16, c, 1)
        self.dw = nn.Conv2d(c, c, 5, padding=pad, groups=c)
        self.b = nn.Conv2d(c, 64, 1)

    def forward(self, x):
        return self.b(torch.relu(self.dw(torch.relu(self.a(x)))))


def test_layers_left_on_todays_route():
    for c, pad, want in ((96, 2, 1), (96, 0, 0), (2048, 2, 1), (2064, 2, 0), (96, 1, 0)):
        rep = fuse_inference(fsptq(_Net(c, pad)), dry_run=True, dw5=True).fusion_report
        assert (rep.dw5, rep.layers, rep.skipped) == (want, 3, []), (c, pad, rep)
    # QBase, a float offset in front of the 5x5 layer, act_offsets=True: a padded one stays unplanned (no border term), an unpadded one
    # is planned - on today's kernel
    for pad, layers in ((2, 2), (0, 3)):
        net = _Net(96, pad)
        quantize_model(net, QBASE_W4A8, None)
        for m in net.modules():
            if isinstance(m, QBase):
                m.in_init_state.fill_(1)
                m.wt_init_state.fill_(1)
                m.in_offset = torch.tensor([-0.625 if m is net.dw else 0.0])
        rep = fuse_inference(net.eval(), dry_run=True, act_offsets=True, dw5=True).fusion_report
        assert (rep.dw5, rep.layers) == (0, layers), (pad, rep)
        net.dw.in_offset = torch.tensor([0.0])
        rep = fuse_inference(net.eval(), dry_run=True, act_offsets=True, dw5=True).fusion_report
        assert (rep.dw5, rep.layers) == (1 if pad == 2 else 0, 3), (pad, rep)
