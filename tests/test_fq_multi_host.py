"""Host side of the one-launch fake-quant of many tensors (csrc/fake_quant_multi.hip): the segment struct's layout, the
table preparation (a host function: sizes in, prefixes and grids out) and WeightQuantBatch's membership - none of it
touches a GPU."""
import ctypes

import pytest
import torch

EINVAL, ERANGE, ESCRATCH, EALIGN = -1, -2, -3, -4
MAX_N = 8192 * 1024


@pytest.fixture(scope="module")
def N():
    from dlmc import _native
    return _native


def make(N, specs):
    """specs: dicts of dlmcq_fq_segment fields; pointers default to distinct 16-byte aligned integers (never dereferenced)."""
    t = (N.FqSegment * max(len(specs), 1))()
    for i, (rec, sp) in enumerate(zip(t, specs)):
        base = 0x10000 * (i + 1)
        d = dict(x=base, y=base + 0x1000, gy=base + 0x2000, gx=base + 0x3000, scale=base + 0x4000, offset=0, gscale=base + 0x5000,
                 n=0, channels=1, inner=0, lo=-7, hi=7, ste_g=0.0, form=N.FORM_SYMMETRIC)
        d.update(sp)
        for k, v in d.items():
            setattr(rec, k, v)
    return t


def prepare(N, t, nseg):
    f, b, z, sc = ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_int64(-1), ctypes.c_size_t(77)
    rc = N.lib.dlmcq_fq_multi_prepare(ctypes.byref(t), nseg, ctypes.byref(f), ctypes.byref(b), ctypes.byref(z), ctypes.byref(sc))
    return rc, f.value, b.value, z.value, sc.value


def restate(specs):
    """The documented grids, restated: forward = one 256-element chunk per workgroup (the 0-3 tail rides on the first), backward =
    one 1024-element chunk per workgroup per tensor or one row per workgroup per channel, one partial per backward workgroup."""
    fwd = bwd = 0
    rows = []
    for sp in specs:
        n, ch = sp.get("n", 0), sp.get("channels", 1)
        rows.append((fwd, bwd, bwd))
        if n > 0 and sp.get("y", 1):
            fwd += max(1, -(-(n // 4) // 64))
        if n > 0 and sp.get("gy", 1) and (sp.get("gx", 1) or sp.get("gscale", 1)):
            bwd += ch if ch > 1 else max(1, -(-(n // 4) // 256))
    return rows, fwd, bwd


def test_struct_mirror_has_the_library_size(N):
    assert ctypes.sizeof(N.FqSegment) == N.lib.dlmcq_fq_segment_bytes() == 17 * 8


def test_prepare_fills_prefixes_and_grids(N):
    specs = [dict(n=n) for n in (0, 1, 3, 4, 255, 256, 257, 1023, 1024, 1025, 4099, MAX_N)]
    specs += [dict(n=c * i, channels=c, inner=i) for c, i in ((8, 9), (3, 147), (16, 64), (64, 4), (5, 1030), (2048, 512))]
    specs += [dict(n=0, channels=4, inner=0), dict(n=600, y=0), dict(n=600, gy=0), dict(n=600, gx=0, gscale=0), dict(n=5000, gx=0),
              dict(n=0)]
    t = make(N, specs)
    rc, fwd, bwd, fin, scratch = prepare(N, t, len(specs))
    assert rc == 0
    rows, wfwd, wbwd = restate(specs)
    assert (fwd, bwd, fin, scratch) == (wfwd, wbwd, len(specs), 4 * wbwd)
    assert [(r.fwd_chunk0, r.bwd_wg0, r.part0) for r in t] == rows
    # empty segments get no workgroups: each starts where its successor does
    for i, sp in enumerate(specs[:-1]):
        if sp.get("n", 0) == 0:
            assert rows[i] == rows[i + 1]
    assert rows[-1] == (wfwd, wbwd, wbwd)
    # nobody wants a scale gradient: no finalize and no scratch
    t = make(N, [dict(n=5000, gscale=0), dict(n=64, channels=8, inner=8, gscale=0)])
    assert prepare(N, t, 2) == (0, 20 + 1, 5 + 8, 0, 0)      # 1250 float4: 20 chunks of 64, 5 of 256; 16 float4: 1 chunk, 8 rows
    # an empty table
    assert prepare(N, make(N, []), 0) == (0, 0, 0, 0, 0)


@pytest.mark.parametrize("spec,code", [
    (dict(n=MAX_N + 1), ERANGE),                                  # 8193 backward chunks: the one-tensor backward grid-strides there
    (dict(n=64, x=0x10004), EALIGN), (dict(n=64, y=0x11008), EALIGN), (dict(n=64, gy=0x12004), EALIGN), (dict(n=64, gx=0x1300c), EALIGN),
    (dict(n=64, lo=8, hi=7), EINVAL),
    (dict(n=64, form=0), EINVAL), (dict(n=64, form=4), EINVAL), (dict(n=64, form=5), EINVAL),     # EMULATE, ROOTQ_ACT, unknown
    (dict(n=65, channels=8, inner=8), EINVAL),
    (dict(n=64, channels=0), EINVAL), (dict(n=-1), EINVAL), (dict(n=64, x=0), EINVAL), (dict(n=64, scale=0), EINVAL),
    (dict(n=64, hi=2 ** 31), ERANGE),
])
def test_prepare_refuses(N, spec, code):
    good = dict(n=1000)
    for specs in ([spec], [good, spec], [spec, good]):
        assert prepare(N, make(N, specs), len(specs))[0] == code
    assert prepare(N, make(N, [good]), 1)[0] == 0


def test_launch_entry_points_validate_without_a_gpu(N):
    one = ctypes.c_void_p(4096)
    assert N.lib.dlmcq_fake_quant_multi_f32(None, 3, 0, None) == 0            # nothing to launch
    assert N.lib.dlmcq_fake_quant_multi_f32(None, 3, 5, None) == EINVAL
    assert N.lib.dlmcq_fake_quant_multi_f32(ctypes.c_void_p(4100), 3, 5, None) == EALIGN
    assert N.lib.dlmcq_fake_quant_multi_bwd_f32(one, 3, 10, 3, one, 39, None) == ESCRATCH
    assert N.lib.dlmcq_fake_quant_multi_bwd_f32(one, 3, 10, 3, None, 40, None) == ESCRATCH
    assert N.lib.dlmcq_fake_quant_multi_bwd_f32(one, 3, 10, 2, one, 40, None) == EINVAL   # the finalize is indexed by segment
    assert N.lib.dlmcq_fake_quant_multi_bwd_f32(None, 3, 0, 0, None, 0, None) == 0


# ------------------------------------------------------------------------------- WeightQuantBatch
def _cfg(wtype="minmax_tensor", enable=True, **extra):
    w = {"enable": enable, "type": wtype, "args": {"n_bits": 4, "signed": True}}
    w.update(extra)
    return {"weight": w, "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 4, "signed": False}},
            "momentum": 0.1, "exclude_layers": [], "override_options": []}


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Conv2d(3, 8, 3)
        self.b = torch.nn.Conv2d(8, 8, 3, groups=8)
        self.c = torch.nn.Conv2d(8, 16, 1)
        self.d = torch.nn.Linear(16, 10)


def _ready(model, skip=()):
    for name, m in model.named_children():
        if name not in skip:
            m._init.mark(m, "wt_init_state")


def test_weight_quant_batch_membership_on_cpu():
    from dlmc.utils.quantize import WeightQuantBatch, quantize_model
    # QBase family: one layer with its weight quantiser off, one left uncalibrated
    net = _Net()
    cfg = _cfg()
    cfg["override_options"] = [{"layers": ["^b$"], "options": {"weight": {"enable": False}}}]
    quantize_model(net, cfg)
    _ready(net, skip=("c",))
    wqb = WeightQuantBatch(net)
    assert wqb.members == [net.a, net.d]                      # module order
    assert set(wqb.skipped) == {"b", "c"}
    # FSPTQ family: AdaRound on one layer
    fs = _Net()
    cfg = _cfg("minmax_channel")
    cfg["override_options"] = [{"layers": ["^c$"], "options": {"weight": {"recon_type": "adaround"}}}]
    quantize_model(fs, cfg, quantization_type="FSPTQ")
    if "alpha" not in dict(fs.c.named_parameters()):          # (override_options carries type / enable / args only)
        fs.c.qconfig["weight"]["recon_type"] = "adaround"
    _ready(fs)
    wf = WeightQuantBatch(fs)
    assert wf.members == [fs.a, fs.b, fs.d] and set(wf.skipped) == {"c"}
    # RootQ: every layer is skipped
    rq = _Net()
    quantize_model(rq, _cfg(), quantization_type="RootQ")
    wr = WeightQuantBatch(rq)
    assert wr.members == [] and set(wr.skipped) == {"a", "b", "c", "d"}
    reasons = {wqb.skipped["b"], wqb.skipped["c"], wf.skipped["c"], wr.skipped["a"]}
    assert len(reasons) == 4, reasons                         # disabled, uncalibrated, AdaRound, RootQ: four distinct reasons
    # refresh() picks up a calibration that happened since, in module order again
    net.c._init.mark(net.c, "wt_init_state")
    assert wqb.refresh().members == [net.a, net.c, net.d] and set(wqb.skipped) == {"b"}
    # a weight the segment table does not take (not fp32) is skipped as not eligible and keeps its own launches
    net.d.weight.data = net.d.weight.data.double()
    assert wqb.refresh().members == [net.a, net.c] and wqb.skipped["d"].startswith("not eligible")
