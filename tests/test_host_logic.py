"""Host-side logic that needs no GPU: `quantize_model` (class swap, regex exclusion, per-layer
overrides, state_dict layout), the benchmark layer tables, and the refusal to run on CPU tensors."""
import copy
import os
import logging

import pytest
import torch
from torch import nn

import workloads as W
from dlmc._native import DlmcqError
from dlmc.quantization.scalar import FSPTQuant, RootQ, modules
from dlmc.utils.access import attrsetter, get_layers, mark_modules
from dlmc.utils.quantize import quantize_model

CFG = {
    "weight": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": True}},
    "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": True}},
    "exclude_layers": [],
    "override_options": [{"layers": []}],
}


def small_net():
    return nn.Sequential()  # placeholder replaced below


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 8, 3, padding=1)
        self.bn1 = nn.BatchNorm2d(8)
        self.layer1 = nn.Sequential(nn.Conv2d(8, 8, 3, padding=1, bias=False), nn.ReLU(), nn.Conv2d(8, 16, 1))
        self.fc = nn.Linear(16, 10)

    def forward(self, x):
        x = self.layer1(self.bn1(self.conv1(x)))
        return self.fc(x.mean(dim=(2, 3)))


def test_layer_tables_match_the_survey():
    want = {"resnet18": (21, 2183168, 11678912), "resnet50": (54, 10664448, 25502912),
            "repvgg_a1": (23, 2459904, 12783296)}
    for name, (layers, act, wt) in want.items():
        rows = W.layer_table(W.MODELS[name](), torch.zeros(1, 3, 224, 224))
        got = W.table_totals(rows)
        assert got[:3] == (layers, act, wt), name
    assert W.table_totals(W.layer_table(W.resnet50(), torch.zeros(1, 3, 224, 224)))[3] == 4089184256


def test_get_layers_and_attrsetter():
    net = Net()
    assert get_layers(net, filter_types=(nn.Conv2d, nn.Linear)) == ["conv1", "layer1.0", "layer1.2", "fc"]
    assert get_layers(net, filter_regexp="layer1") == ["layer1.0", "layer1.2"]
    assert get_layers(net, filter_regexp="conv") == ["conv1"]          # re.match: anchored at the start
    assert "bn1" in get_layers(net)                                     # every weight owner, like the reference
    attrsetter("layer1.2")(net, nn.Identity())
    assert isinstance(net.layer1[2], nn.Identity)
    mark_modules(net)
    assert net.layer1[0].name == "layer1.0"


def test_quantize_model_swaps_in_place_and_keeps_parameters():
    net = Net()
    w_before = net.conv1.weight
    quantize_model(net, copy.deepcopy(CFG), logging.getLogger("t"))
    assert isinstance(net.conv1, modules.QConv2d) and isinstance(net.conv1, modules.QBase)
    assert isinstance(net.layer1[0], modules.QConv2d) and isinstance(net.fc, modules.QLinear)
    assert net.conv1.weight is w_before                                  # __dict__ carried over, not copied
    assert isinstance(net.bn1, nn.BatchNorm2d)
    keys = set(net.state_dict().keys())
    for k in ("conv1.in_scale", "conv1.wt_scale", "conv1.in_init_state", "conv1.wt_init_state", "conv1.weight",
              "conv1.bias", "fc.in_scale"):
        assert k in keys
    assert "conv1.in_offset" not in keys                                 # None until the first forward, as the reference
    assert net.conv1.in_scale.shape == (1,) and net.conv1.in_init_state.shape == (1,)
    assert (net.conv1.wt_min_val, net.conv1.wt_max_val) == (-127, 127)
    assert hasattr(net.conv1, "reset_qparams") and hasattr(net.conv1, "_forward_func")
    names = [n for n, _ in net.named_parameters()]
    assert any(n.endswith("in_scale") for n in names) and any(n.endswith("wt_scale") for n in names)


def test_quantize_model_exclude_and_override():
    net = Net()
    cfg = copy.deepcopy(CFG)
    cfg["exclude_layers"] = ["conv1", "fc"]
    cfg["override_options"] = [{"layers": ["layer1.2"], "options": {"weight": {"args": {"n_bits": 4}},
                                                                      "input": {"type": "minmax_channel", "args": {"signed": False}}}}]
    quantize_model(net, cfg, None)
    assert type(net.conv1) is nn.Conv2d and type(net.fc) is nn.Linear
    assert isinstance(net.layer1[0], modules.QConv2d)
    q = net.layer1[2]
    assert (q.wt_min_val, q.wt_max_val) == (-7, 7) and (q.in_min_val, q.in_max_val) == (0, 255)
    assert q.qconfig["input"]["type"] == "minmax_channel" and q.qconfig["input"]["args"]["ch_axis"] == 1
    assert net.layer1[0].qconfig["weight"]["args"]["n_bits"] == 8          # the default was not mutated
    with pytest.raises(AssertionError):
        bad = copy.deepcopy(CFG)
        bad["override_options"] = [{"layers": ["fc"], "options": {}}, {"layers": ["fc"], "options": {}}]
        quantize_model(Net(), bad, None)


def test_families_and_state_dict_layout():
    net = Net()
    cfg = copy.deepcopy(CFG)
    cfg["weight"].update(type="minmax_channel", recon_type="adaround")
    quantize_model(net, cfg, None, quantization_type="FSPTQ")
    assert isinstance(net.conv1, FSPTQuant.FSPTQConv2d) and isinstance(net.fc, FSPTQuant.FSPTQBase)
    sd = net.state_dict()
    assert sd["conv1.wt_scale"].shape == (8, 1, 1, 1) and sd["fc.wt_scale"].shape == (10, 1)
    assert sd["conv1.wt_offset"].shape == (8, 1, 1, 1) and sd["conv1.in_offset"].shape == (1,)
    assert sd["conv1.org_weight"].shape == net.conv1.weight.shape and sd["conv1.alpha"].shape == net.conv1.weight.shape
    for m in ("change_quant_state", "reinit_parameters", "init_alpha", "get_soft_targets"):
        assert hasattr(net.conv1, m)
    net.conv1.change_quant_state(False, True)
    assert (net.conv1.wt_quant, net.conv1.act_quant) == (False, True)

    net = Net()
    cfg = copy.deepcopy(CFG)
    cfg["momentum"] = 0.05
    quantize_model(net, cfg, None, quantization_type="RootQ")
    assert isinstance(net.fc, RootQ.RootQLinear) and net.fc.momentum == 0.05
    sd = net.state_dict()
    for k in ("in_scale", "in_run_upper", "in_run_scale", "in_init_state", "wt_upper", "wt_lower", "wt_alpha",
              "wt_run_upper", "wt_run_lower", "wt_init_state"):
        assert sd["fc." + k].shape == ()
    assert float(sd["fc.wt_upper"]) == 3.0 and float(sd["fc.wt_lower"]) == -4.0 and float(sd["fc.wt_alpha"]) == 0.25
    with pytest.raises(NotImplementedError):
        quantize_model(Net(), copy.deepcopy(CFG), None, quantization_type="BitMixer")


def test_no_cpu_fallback_in_the_wrappers():
    net = Net()
    quantize_model(net, copy.deepcopy(CFG), None)
    with pytest.raises(DlmcqError, match="no CPU fallback"):
        net(torch.randn(2, 3, 8, 8))


def test_unknown_qtype_raises_keyerror_like_the_reference():
    from dlmc.quantization.scalar import ops
    with pytest.raises(KeyError):
        ops.get_qparams_tensor(torch.zeros(4), "no_such_estimator", n_bits=8, signed=True)


def test_mobileone_s1_matches_the_published_size():
    rows = W.layer_table(W.mobileone_s1_deploy(), torch.zeros(1, 3, 224, 224))
    layers, act, wt, macs = W.table_totals(rows)
    assert layers == 44 and 4.7e6 < wt < 4.8e6 and 8.2e8 < macs < 8.3e8   # 4.8 M parameters, 825 MFLOPs (paper)


def test_fusion_decisions_without_a_gpu():
    """The dataflow pass of dlmc.utils.fuse (which ReLU / shortcut add / max-pool / consumer quantiser folds into which
    int8 kernel) on CPU models whose wrappers are marked calibrated by hand: structure only (`dry_run`)."""
    import workloads as W
    from dlmc.quantization.scalar.FSPTQuant import FSPTQBase
    from dlmc.utils.fuse import fuse_inference
    from dlmc.utils.quantize import quantize_model
    cfg = {"weight": {"enable": True, "type": "minmax_channel", "args": {"n_bits": 8, "signed": True}},
           "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
           "exclude_layers": [], "override_options": []}

    def calibrated(net, first_layer_zp=0.0):
        for m in net.modules():                      # BatchNorm folded by hand: the pass treats Identity as a wire
            for name, child in list(m.named_children()):
                if isinstance(child, torch.nn.BatchNorm2d):
                    setattr(m, name, torch.nn.Identity())
        quantize_model(net, cfg, None, "FSPTQ")
        first = True
        for m in net.modules():
            if isinstance(m, FSPTQBase):
                m.in_init_state.fill_(1)
                m.wt_init_state.fill_(1)
                m.in_offset = torch.tensor(first_layer_zp if first else 0.0)
                first = False
        return net.eval()

    rep = fuse_inference(calibrated(W.resnet50()), dry_run=True).fusion_report
    assert (rep.layers, rep.stem, rep.pooled, rep.dual, rep.relu, rep.residual, rep.emit, rep.fp32_outputs, rep.skipped) == (
        54, 1, 1, 4, 49, 16, 48, 14, [])
    rep = fuse_inference(calibrated(W.resnet50(), first_layer_zp=-2.117), dry_run=True).fusion_report
    assert rep.stem == 0 and rep.skipped == ["conv1"] and rep.layers == 53       # non-integer zero point: fp32 first layer
    rep = fuse_inference(calibrated(W.resnet18()), dry_run=True).fusion_report
    assert (rep.layers, rep.stem, rep.pooled, rep.dual, rep.residual) == (21, 1, 1, 3, 8)   # the stem kernel pools in fp32: shortcut served too
    rep = fuse_inference(calibrated(W.repvgg_a1_deploy()), dry_run=True).fusion_report
    assert (rep.layers, rep.stem, rep.relu, rep.emit, rep.fp32_outputs, rep.dual) == (23, 1, 22, 21, 2, 0)
    rep = fuse_inference(calibrated(W.mobileone_s1_deploy()), dry_run=True).fusion_report
    assert (rep.stem, rep.layers, rep.skipped) == (1, 44, [])        # depthwise layers and 96-channel pointwise layers (padded) included
    with pytest.raises(RuntimeError):
        fuse_inference(calibrated(W.resnet18()).train(), dry_run=True)

    # a residual block whose width is no multiple of 64 (MobileNetV2-style 96-channel projection): the plan pads the layer's output
    # channels to 128, so its shortcut add is NOT absorbed into the kernel (the k-wide fp32 shortcut would not fit the padded tile)
    class Narrow(torch.nn.Module):
        def __init__(self, ch):
            super().__init__()
            self.stem = torch.nn.Conv2d(64, ch, 1)
            self.a = torch.nn.Conv2d(ch, 128, 1)
            self.b = torch.nn.Conv2d(128, ch, 1)
            self.head = torch.nn.Conv2d(ch, 64, 1)

        def forward(self, x):
            y = self.stem(x)
            return self.head(torch.relu(self.b(torch.relu(self.a(y))) + y))
    rep = fuse_inference(calibrated(Narrow(96)), dry_run=True).fusion_report
    assert (rep.layers, rep.residual) == (4, 0), rep
    rep = fuse_inference(calibrated(Narrow(128)), dry_run=True).fusion_report
    assert (rep.layers, rep.residual) == (4, 1), rep


def test_fuse_reports_untraceable_models():
    from dlmc.utils.fuse import fuse_inference

    class Dyn(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.c = torch.nn.Conv2d(64, 64, 1)

        def forward(self, x):
            return self.c(x) if x.sum() > 0 else x      # data-dependent branch: not a static dataflow

    with pytest.raises(RuntimeError, match="torch.fx"):
        fuse_inference(Dyn().eval(), dry_run=True)


def test_chain_kernel_listing_has_no_spill_in_its_loop_and_keeps_its_store_wait_states():
    """tools/lint_chain.py on the cross-compiled listing (hipcc, no GPU): the chain kernel keeps asm-loaded registers in flight
    across a chunk and counts its own waits, so a spill inside the loop or a missing wait state after an asm store is a bug."""
    import shutil
    import subprocess
    import sys
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "lint_chain.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


def test_first_layer_kernel_listing_leaves_in_flight_fragments_alone():
    """tools/lint_stem.py on the cross-compiled listing: conv_stem_pool_i8_kernel<7> loads its operand fragments by inline asm two
    items ahead; nothing may read, copy or spill them between issue and the counted wait."""
    import shutil
    import subprocess
    import sys
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "lint_stem.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


def test_pointwise_kernel_listing_leaves_in_flight_fragments_alone():
    """tools/lint_pw.py on the cross-compiled listing: conv_pw_i8_kernel requests a block's activation fragments (asm buffer loads) in
    the middle of the previous block's epilogue and waits for them with a counted s_waitcnt at the top of its loop; nothing reachable
    in between (control-flow walk) may read, copy or overwrite those registers, the kernel uses no scratch, every asm store has its
    wait states.  conv_pwr_i8_kernel (csrc/conv_pwr_i8.hip) keeps loads in flight ACROSS counted waits: the same script replays its
    whole vector-memory queue along every path of the listing."""
    import shutil
    import subprocess
    import sys
    if not shutil.which("hipcc") and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("no hipcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "lint_pw.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "residual-block kernels checked, 0 problem(s)" in r.stdout, r.stdout


def test_bench_refuses_counter_tails_that_are_not_the_step_s_launches(tmp_path):
    """bench.py:pmc_traffic (round 5; VERDICT r4: a TAIL that held the side networks' dispatches fed the headline's roofline objects): a tail
    is used only when its dispatch count is the step's launch count and its bytes are not below 0.9 x the algorithmic bytes; only the newest
    round's file is asked; a refusal carries its reason."""
    import json
    import bench
    tail = lambda n, f, w: {"FETCH_SIZE": {"dispatches": n, "mean_KiB": f}, "WRITE_SIZE": {"dispatches": n, "mean_KiB": w}}
    (tmp_path / "r04_pmc_bench_fused_plan.json").write_text(json.dumps({"TAIL last 16 dispatches of *conv3x3_halo_i8_kernel*": tail(16, 50000.0, 30000.0)}))
    (tmp_path / "r05_pmc_bench_fused_plan.json").write_text(json.dumps({
        "TAIL last 16 dispatches of *conv3x3_halo_i8_kernel*": tail(16, 17414.82, 28224.0),        # 64.6 MB: RepVGG's layers, not ResNet-50's 105.9 MB
        "TAIL last 11 dispatches of *conv_chain_i8_kernel*": tail(11, 366460.9, 780499.34),
        "TAIL last 6 dispatches of *conv_i8_mfma_kernel*": tail(6, 10651.0, 127565.09)}))
    got, src, why = bench.pmc_traffic("conv_chain_i8_kernel", 11, 1546270000, directory=str(tmp_path))
    assert src == "r05_pmc_bench_fused_plan.json" and why is None and abs(got / 1546270000 - 1.002) < 0.01
    got, src, why = bench.pmc_traffic("conv3x3_halo_i8_kernel", 16, 105900000, directory=str(tmp_path))
    assert got is None and src is None and "below 0.9" in why and "r05" in why            # (and NOT the older round's plausible-looking entry)
    got, src, why = bench.pmc_traffic("conv_i8_mfma_kernel", 4, 0, directory=str(tmp_path))
    assert got is None and "TAIL holds (6, 6) dispatches" in why
    got, src, why = bench.pmc_traffic("conv_pwr_i8_kernel", 4, 1, directory=str(tmp_path))
    assert got is None and "no profiles" in why


def test_bench_dump_outputs_float32_within_budget_and_seeded(tmp_path):
    """bench.py --dump-outputs: float32 .npy per output; one over its share of the byte budget keeps a fixed, seeded sample of its rows,
    the same from call to call (two builds dump the same elements), in their original order."""
    import numpy as np
    import bench
    y = torch.arange(512 * 1000, dtype=torch.float64).reshape(512, 1000)
    bench.dump_outputs(str(tmp_path / "all"), {"logits": y})
    a = np.load(tmp_path / "all" / "logits.npy")
    assert a.dtype == np.float32 and np.array_equal(a, y.float().numpy())
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), {"logits": y}, budget=100 * 1000 * 4 + 5)
    s1, s2 = np.load(tmp_path / "s1" / "logits.npy"), np.load(tmp_path / "s2" / "logits.npy")
    assert s1.shape == (100, 1000) and s1.nbytes <= 100 * 1000 * 4 + 5 and np.array_equal(s1, s2)
    rows = s1[:, 0] / 1000
    assert np.all(np.diff(rows) > 0) and np.array_equal(s1, y.float().numpy()[rows.astype(np.int64)])


def test_chunk_major_block_tensor_round_trip_on_the_host():
    """kernels.ChunkMajor (the fp32 block tensor between two chain kernels, DLMCQ_FP32_*_CHUNK_MAJOR): [K / 64][N H W][64] planes of the same
    values - conversions and windows are plain tensor arithmetic, checked here without a GPU; the kernels' side of it: tests/test_gpu_chain.py."""
    import torch
    from dlmc.quantization.scalar import kernels as K
    g = torch.Generator().manual_seed(4)
    t = torch.randn(3, 192, 5, 7, generator=g).contiguous(memory_format=torch.channels_last)
    cm = K.ChunkMajor.from_nhwc(t)
    assert cm.shape == (3, 192, 5, 7) and tuple(cm.buf.shape) == (3, 3 * 5 * 7, 64) and cm.dim() == 4 and cm.numel() == t.numel()
    # element (n, k, h, w) sits at plane k // 64, row (n H + h) W + w, column k % 64
    for n, k, h, w in ((0, 0, 0, 0), (2, 191, 4, 6), (1, 64, 2, 3), (2, 127, 0, 5)):
        assert cm.buf[k // 64, (n * 5 + h) * 7 + w, k % 64] == t[n, k, h, w]
    back = cm.to_nhwc()
    assert torch.equal(back, t) and back.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(cm.window(1, 1, 4, 2, 7), t[1:2, :, 1:4, 2:7])
    e = K.ChunkMajor.empty(2, 128, 4, 4, "cpu")
    assert tuple(e.buf.shape) == (2, 32, 64) and e.shape == (2, 128, 4, 4)
    with pytest.raises(ValueError):
        K.ChunkMajor.from_nhwc(torch.zeros(1, 96, 2, 2))          # K % 64 != 0
    with pytest.raises(ValueError):
        K.ChunkMajor.from_nhwc(torch.zeros(1, 64, 2, 2, dtype=torch.float16))


def test_wrapper_marshalling_helpers_on_the_host():
    """The pure helpers the int8 convolution wrappers marshal their operands with (kernels._flat, _out_hw, _as_chunk_major)."""
    import torch.nn.functional as F
    from dlmc.quantization.scalar import kernels as K
    like = torch.zeros(1)
    assert K._flat(None, like) is None and K._flat(None, like, 5) is None
    one = K._flat(0.25, like)
    assert one.dtype == torch.float32 and tuple(one.shape) == (1,) and float(one) == 0.25
    wide = K._flat(torch.tensor([[1.5]]), like, 5)
    assert tuple(wide.shape) == (5,) and wide.is_contiguous() and wide.stride() == (1,) and bool((wide == 1.5).all())
    assert tuple(K._flat(torch.tensor(1.5), like).shape) == (1,)                       # 0-d -> [1]; not broadcast without k
    five = torch.arange(5, dtype=torch.float32)
    for got in (K._flat(five, like), K._flat(five, like, 5), K._flat(five.reshape(1, 5, 1, 1), like, 5)):
        assert got.data_ptr() == five.data_ptr() and tuple(got.shape) == (5,)       # no copy
    assert torch.equal(K._flat(torch.arange(5, dtype=torch.float64), like, 5), five)  # other dtypes are converted
    for k in (None, 5):                                                                 # requires_grad does not leak
        assert not K._flat(torch.ones(1, requires_grad=True), like, k).requires_grad
        assert not K._flat(torch.ones(5, requires_grad=True), like, k).requires_grad
    for h, w, r, s, stride, pad, dil in ((5, 5, 3, 3, 1, 1, 1), (7, 9, 1, 1, 1, 0, 1), (10, 10, 1, 1, 2, 0, 1), (24, 24, 7, 7, 2, 0, 1),
                                         (9, 8, 3, 3, 2, 1, 1), (11, 13, 3, 3, 1, 2, 2), (12, 7, 3, 5, 3, 2, 2), (3, 3, 3, 3, 1, 0, 1)):
        want = F.conv2d(torch.zeros(1, 1, h, w), torch.zeros(1, 1, r, s), stride=stride, padding=pad, dilation=dil).shape[2:]
        assert K._out_hw(h, w, r, s, stride, pad, dil) == tuple(want), (h, w, r, s, stride, pad, dil)
    assert K._out_hw(9, 9, 3, 3, 2, 1) == tuple(F.max_pool2d(torch.zeros(1, 1, 9, 9), 3, 2, 1).shape[2:])
    # a channels_last tensor whose MEMORY holds chunk-major planes, re-read as the ChunkMajor it is
    t = torch.randn(2, 128, 3, 5, generator=torch.Generator().manual_seed(5)).contiguous(memory_format=torch.channels_last)
    cm = K._as_chunk_major(t)
    assert cm.shape == (2, 128, 3, 5) and tuple(cm.buf.shape) == (2, 30, 64) and cm.buf.data_ptr() == t.data_ptr()
    assert torch.equal(cm.buf.reshape(-1), t.permute(0, 2, 3, 1).reshape(-1))
