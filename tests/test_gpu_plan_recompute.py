"""fuse_inference(recompute_shortcuts=...): ResNet-50's stage-1 pair with the first block's fp32 output dropped and recomputed by its
reader, against the plan that stores it - identical logits bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_resnet50_plan_with_the_recomputed_shortcut_is_bit_identical():
    import workloads as W
    from dlmc.quantization.scalar import kernels as K
    from dlmc.utils.fuse import ChainInt8Layer, fuse_inference
    from dlmc.utils.merge_bn import merge_bn
    from dlmc.utils.quantize import quantize_model
    cfg = {"weight": {"enable": True, "type": "minmax_channel", "args": {"n_bits": 8, "signed": True}},
           "input": {"enable": True, "type": "minmax_tensor", "args": {"n_bits": 8, "signed": False}},
           "exclude_layers": [], "override_options": []}
    torch.manual_seed(2333)
    net = W.MODELS["resnet50"]().to("cuda:0").eval()
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    net = merge_bn(net, inplace=True)
    quantize_model(net, cfg, None, "FSPTQ", int8_gemm=True)
    x = torch.relu(torch.randn(2, 3, 64, 64, device="cuda:0"))
    with torch.no_grad():
        net(x)                                  # calibrate
        off = fuse_inference(net, recompute_shortcuts=False)
        on = fuse_inference(net, recompute_shortcuts=True)
        assert off.fusion_report.recomputed == 0 and on.fusion_report.recomputed == 1, on.fusion_report      # the default shape list: stage 1 alone
        assert off.fusion_report.chained == on.fusion_report.chained == 11
        took = [m for m in on.modules() if isinstance(m, ChainInt8Layer) and m.recompute]
        first = [m for m in on.modules() if isinstance(m, ChainInt8Layer) and m.defer_out]
        assert len(took) == 1 and len(first) == 1 and first[0].short is not None
        seen = []
        first[0].register_forward_hook(lambda mod, args, out: seen.append(out[0]))
        took[0].register_forward_hook(lambda mod, args, out: seen.append(args[1]))
        y_off, y_on = off(x * 0.8), on(x * 0.8)
        torch.cuda.synchronize()
        # the first block's output travelled as its operands and was never stored; asked for, it is the tensor the other plan stores
        assert len(seen) == 2 and seen[0] is seen[1] and isinstance(seen[0], K.DeferredBlock) and seen[0]._buf is None
        want = []
        h = next(m for m in off.modules() if isinstance(m, ChainInt8Layer) and m.short is not None).register_forward_hook(
            lambda mod, args, out: want.append(out[0]))
        off(x * 0.8)
        h.remove()
        stored = want[0].to_nhwc() if isinstance(want[0], K.ChunkMajor) else want[0]
        assert torch.equal(seen[0].to_nhwc().view(torch.int32), stored.view(torch.int32))
    assert torch.equal(y_off.view(torch.int32), y_on.view(torch.int32))
    assert bool(torch.isfinite(y_on).all()) and float(y_on.abs().max()) > 0
