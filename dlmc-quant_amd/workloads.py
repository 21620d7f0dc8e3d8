"""Shape generators for the benchmark configurations (BASELINE.json `configs`).

The reference takes ResNet-18/50 from torchvision/timm (model/classification/__init__.py:2,4), which are
not installed here, and RepVGG-A1 from model/classification/repvgg.py:205-207.  These are independent
minimal definitions of the same public architectures - only the layer shapes matter to the fake-quantize
path - with random-init weights (Kaiming normal, as cifarresnet.py:46-48 initialises convs).

`layer_table(model, x)` lists every quantisable layer with its input-activation and weight element
counts; tests pin the totals to SURVEY.md section 8(d):
    ResNet-18 : 21 layers, 2 183 168 input elems/img, 11 678 912 weight elems
    ResNet-50 : 54 layers, 10 664 448 input elems/img, 25 502 912 weight elems (4.089 GMAC/img)
    RepVGG-A1 (deploy): 23 layers, 2 459 904 input elems/img, 12 783 296 weight elems
    MobileNetV2: 53 layers, 6 767 200 input elems/img, 3 469 760 weight elems (300 774 272 MAC/img)
"""
import torch
import torch.nn.functional as F
from torch import nn


def _conv(cin, cout, k, stride=1, groups=1):
    return nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, groups=groups, bias=False)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, cin, width, stride, option="B"):
        super().__init__()
        if option not in ("A", "B", "C", "D"):
            raise ValueError(f"BasicBlock: shortcut option 'A', 'B', 'C' or 'D', not {option!r}")
        self.conv1 = _conv(cin, width, 3, stride)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = _conv(width, width, 3)
        self.bn2 = nn.BatchNorm2d(width)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        # where the shape changes: a 1x1 convolution + BN on the shortcut ("option B"), or no parameters at all ("option A", He et al.
        # 2016, section 4.2): every stride-th pixel of x, the new channels zero, half of them in front and half behind
        self.subsample = None
        if (stride != 1 or cin != width) and option == "A":
            if width < cin or (width - cin) % 2:
                raise ValueError("BasicBlock: option A pads (width - cin) / 2 zero channels on either side")
            self.subsample = (stride, (width - cin) // 2)
        elif option == "D" or ((stride != 1 or cin != width) and option == "C"):
            # "option C": the stride moves from the 1x1 convolution into an average pool in front of it (nn.AvgPool2d(stride, stride), the
            # ResNet-D / "anti-aliased" downsample); "option D": the same, and a 1x1 convolution + BN on every stride-1 shortcut as well
            # (cifarresnet.py:57-87)
            pool = [nn.AvgPool2d(kernel_size=stride, stride=stride)] if stride != 1 else []
            self.downsample = nn.Sequential(*pool, _conv(cin, width, 1), nn.BatchNorm2d(width))
        elif stride != 1 or cin != width:
            self.downsample = nn.Sequential(_conv(cin, width, 1, stride), nn.BatchNorm2d(width))

    def forward(self, x):
        if self.subsample is not None:
            s, pad = self.subsample
            idt = F.pad(x[:, :, ::s, ::s], (0, 0, 0, 0, pad, pad), "constant", 0)
        else:
            idt = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        return self.relu(out + idt)


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, cin, width, stride):
        super().__init__()
        cout = width * 4
        self.conv1 = _conv(cin, width, 1)
        self.bn1 = nn.BatchNorm2d(width)
        self.conv2 = _conv(width, width, 3, stride)   # stride on the 3x3 (torchvision "v1.5")
        self.bn2 = nn.BatchNorm2d(width)
        self.conv3 = _conv(width, cout, 1)
        self.bn3 = nn.BatchNorm2d(cout)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = None
        if stride != 1 or cin != cout:
            self.downsample = nn.Sequential(_conv(cin, cout, 1, stride), nn.BatchNorm2d(cout))

    def forward(self, x):
        idt = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        return self.relu(out + idt)


class ResNet(nn.Module):
    def __init__(self, block, depths, num_classes=1000):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, stride=2, padding=1)
        cin, stages = 64, []
        for i, (width, depth) in enumerate(zip((64, 128, 256, 512), depths)):
            blocks = []
            for j in range(depth):
                blocks.append(block(cin, width, 2 if (j == 0 and i > 0) else 1))
                cin = width * block.expansion
            stages.append(nn.Sequential(*blocks))
        self.layer1, self.layer2, self.layer3, self.layer4 = stages
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(cin, num_classes)
        _init(self)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.fc(torch.flatten(self.avgpool(x), 1))


class RepVGGDeployBlock(nn.Module):
    """A RepVGG block after `switch_to_deploy` (repvgg.py:132-147): one 3x3 conv with bias + ReLU."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.rbr_reparam = nn.Conv2d(cin, cout, 3, stride=stride, padding=1, bias=True)
        self.nonlinearity = nn.ReLU()

    def forward(self, x):
        return self.nonlinearity(self.rbr_reparam(x))


class RepVGGTrainBlock(nn.Module):
    """A RepVGG block in its multi-branch training form (3x3+BN, 1x1+BN, identity BN), with the reference's
    attribute names (repvgg.py:22-60) so `dlmc.utils.reparam` converts it."""

    def __init__(self, cin, cout, stride, groups=1):
        super().__init__()
        self.in_channels, self.groups = cin, groups
        self.rbr_identity = nn.BatchNorm2d(cin) if (cin == cout and stride == 1) else None

        def conv_bn(k, pad):
            seq = nn.Sequential()
            seq.add_module("conv", nn.Conv2d(cin, cout, k, stride=stride, padding=pad, groups=groups, bias=False))
            seq.add_module("bn", nn.BatchNorm2d(cout))
            return seq
        self.rbr_dense = conv_bn(3, 1)
        self.rbr_1x1 = conv_bn(1, 0)
        self.nonlinearity = nn.ReLU()

    def forward(self, x):
        if hasattr(self, "rbr_reparam"):
            return self.nonlinearity(self.rbr_reparam(x))
        idt = 0 if self.rbr_identity is None else self.rbr_identity(x)
        return self.nonlinearity(self.rbr_dense(x) + self.rbr_1x1(x) + idt)


class RepVGGDeploy(nn.Module):
    def __init__(self, num_blocks, widths, num_classes=1000):
        super().__init__()
        self.stage0 = RepVGGDeployBlock(3, widths[0], 2)
        cin, stages = widths[0], []
        for n, w in zip(num_blocks, widths[1:]):
            stages.append(nn.Sequential(*[RepVGGDeployBlock(cin if j == 0 else w, w, 2 if j == 0 else 1)
                                          for j in range(n)]))
            cin = w
        self.stage1, self.stage2, self.stage3, self.stage4 = stages
        self.gap = nn.AdaptiveAvgPool2d(1)
        self.linear = nn.Linear(cin, num_classes)
        _init(self)

    def forward(self, x):
        x = self.stage4(self.stage3(self.stage2(self.stage1(self.stage0(x)))))
        return self.linear(torch.flatten(self.gap(x), 1))


class MobileOneDeployBlock(nn.Module):
    """A re-parameterised MobileOne unit: depthwise 3x3 (+bias, ReLU) then pointwise 1x1 (+bias, ReLU)."""

    def __init__(self, cin, cout, stride):
        super().__init__()
        self.dw = nn.Conv2d(cin, cin, 3, stride=stride, padding=1, groups=cin, bias=True)
        self.pw = nn.Conv2d(cin, cout, 1, bias=True)
        self.act = nn.ReLU()

    def forward(self, x):
        return self.act(self.pw(self.act(self.dw(x))))


class MobileOneDeploy(nn.Module):
    """MobileOne in inference form (public architecture, Vasu et al. 2022; NOT in the reference - BASELINE
    config 5 only borrows its layer shapes).  S1: width multipliers (1.5, 1.5, 2.0, 2.5), blocks (2, 8, 10, 1)."""

    def __init__(self, widths=(1.5, 1.5, 2.0, 2.5), blocks=(2, 8, 10, 1), num_classes=1000):
        super().__init__()
        cin = min(64, int(64 * widths[0]))
        self.stage0 = nn.Sequential(nn.Conv2d(3, cin, 3, stride=2, padding=1, bias=True), nn.ReLU())
        stages = []
        for base, mult, n in zip((64, 128, 256, 512), widths, blocks):
            cout = int(base * mult)
            stages.append(nn.Sequential(*[MobileOneDeployBlock(cin if j == 0 else cout, cout, 2 if j == 0 else 1)
                                          for j in range(n)]))
            cin = cout
        self.stage1, self.stage2, self.stage3, self.stage4 = stages
        self.gap = nn.AdaptiveAvgPool2d(1)
        self.linear = nn.Linear(cin, num_classes)
        _init(self)

    def forward(self, x):
        x = self.stage4(self.stage3(self.stage2(self.stage1(self.stage0(x)))))
        return self.linear(torch.flatten(self.gap(x), 1))


def _conv_bn_relu6(cin, cout, k, stride=1, groups=1):
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride=stride, padding=(k - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(cout),
                         nn.ReLU6(inplace=True))


class Swish(nn.Module):
    """x * sigmoid(x) as a module of its own (EfficientNet's activation, efficientnet_block.py:36-41): traced into the multiply."""

    def forward(self, x):
        return x * torch.sigmoid(x)


def _conv_bn_act(cin, cout, k, stride=1, groups=1, act="relu6"):
    """_conv_bn_relu6, the activation `act`: "relu6" (that very block), "swish", "relu" or "hardswish" (nn.Hardswish: MobileNetV3's)."""
    if act == "relu6":
        return _conv_bn_relu6(cin, cout, k, stride, groups)
    if act not in ("swish", "relu", "hardswish"):
        raise ValueError(f"activation 'relu6', 'swish', 'relu' or 'hardswish', not {act!r}")
    fn = Swish() if act == "swish" else (nn.ReLU(inplace=True) if act == "relu" else nn.Hardswish())
    return nn.Sequential(nn.Conv2d(cin, cout, k, stride=stride, padding=(k - 1) // 2, groups=groups, bias=False), nn.BatchNorm2d(cout), fn)


class SqueezeExcite(nn.Module):
    """A squeeze-and-excitation block (public architecture, Hu et al. 2018): x * gate(squeeze(x)), the gate one value per image and
    channel.  `squeeze="linear"`: global average pool, flatten, Linear(c, reduced), swish, Linear(reduced, c), back to (N, C, 1, 1) -
    EfficientNet's spelling (efficientnet_block.py:44-59); `squeeze="conv"`: the pool kept (N, C, 1, 1), two 1x1 convolutions with a ReLU
    between them - GhostNet's and MobileNetV3's (ghostnet.py:44-61).  `gate`: "sigmoid", or "hardsigmoid" = relu6(v + 3) / 6."""

    def __init__(self, c, reduced, gate="sigmoid", squeeze="linear"):
        super().__init__()
        if gate not in ("sigmoid", "hardsigmoid") or squeeze not in ("linear", "conv"):
            raise ValueError(f"SqueezeExcite: gate 'sigmoid' or 'hardsigmoid', squeeze 'linear' or 'conv', not {gate!r} / {squeeze!r}")
        self.gate, self.squeeze = gate, squeeze
        self.pool = nn.AdaptiveAvgPool2d(1)
        if squeeze == "linear":
            self.reduce, self.expand = nn.Linear(c, reduced), nn.Linear(reduced, c)
        else:
            self.reduce, self.expand = nn.Conv2d(c, reduced, 1, bias=True), nn.Conv2d(reduced, c, 1, bias=True)

    def forward(self, x):
        v = self.pool(x)
        if self.squeeze == "linear":
            v = self.reduce(v.view(x.size(0), -1))
            v = self.expand(v * torch.sigmoid(v)).view(x.size(0), x.size(1), 1, 1)
        else:
            v = self.expand(F.relu(self.reduce(v)))
        return x * (torch.sigmoid(v) if self.gate == "sigmoid" else F.relu6(v + 3.) / 6.)


class InvertedResidual(nn.Module):
    """MobileNetV2's unit: 1x1 expansion (t > 1) + depthwise 3x3 + linear 1x1 projection, BN after every convolution, ReLU6 after
    the first two; the identity shortcut where stride is 1 and the width is kept.  `se=True`: a squeeze-excite gate (MobileNetV3's:
    1x1 convolutions, a quarter of the expanded width rounded up to a multiple of 8, hard sigmoid) between the depthwise and the
    projection layer.  `act="swish"`: EfficientNet's MBConv (efficientnet_block.py:44-59, efficientnet.py:29-34) - swish where ReLU6
    was, and with `se` its squeeze-excite block: Linear layers on the flattened pool, a quarter of the block's INPUT width between them,
    a swish there too, a sigmoid gate.  `k`: the depthwise filter, 3 or 5 (EfficientNet's stages 3, 5 and 6 have 5), always with the symmetric
    padding (k - 1) / 2 carried by the convolution."""

    def __init__(self, cin, cout, stride, t, se=False, act="relu6", k=3):
        super().__init__()
        hidden = cin * t
        self.use_res = stride == 1 and cin == cout
        layers = [_conv_bn_act(cin, hidden, 1, act=act)] if t != 1 else []
        layers += [_conv_bn_act(hidden, hidden, k, stride, groups=hidden, act=act)]
        if se and act == "swish":
            layers += [SqueezeExcite(hidden, max(1, cin // 4), gate="sigmoid", squeeze="linear")]
        elif se:
            layers += [SqueezeExcite(hidden, (hidden // 4 + 7) // 8 * 8, gate="hardsigmoid", squeeze="conv")]
        layers += [nn.Conv2d(hidden, cout, 1, bias=False), nn.BatchNorm2d(cout)]
        self.conv = nn.Sequential(*layers)

    def forward(self, x):
        return x + self.conv(x) if self.use_res else self.conv(x)


class MobileNetV2(nn.Module):
    """MobileNetV2 (public architecture, Sandler et al. 2018) in torchvision's module layout - `features.N.0` convolutions with their
    BatchNorm at `features.N.1` (merge_bn's default mapping), `nn.ReLU6`, dropout + linear head.  Width 1.0: 3 504 872 parameters."""

    SETTINGS = ((1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1), (6, 160, 3, 2), (6, 320, 1, 1))   # t, c, n, s

    def __init__(self, num_classes=1000, dropout=0.2, se=False, act="relu6"):
        super().__init__()
        cin = 32
        feats = [_conv_bn_act(3, cin, 3, stride=2, act=act)]
        for t, c, n, s, *k in self.SETTINGS:       # (a fifth entry: the stage's depthwise filter)
            for j in range(n):
                feats.append(InvertedResidual(cin, c, s if j == 0 else 1, t, se, act, *k))
                cin = c
        feats.append(_conv_bn_act(cin, 1280, 1, act=act))
        self.features = nn.Sequential(*feats)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(nn.Dropout(dropout), nn.Linear(1280, num_classes))
        _init(self)

    def forward(self, x):
        return self.classifier(torch.flatten(self.pool(self.features(x)), 1))


class EfficientNetB0(MobileNetV2):
    """EfficientNet-B0 (public architecture, Tan & Le 2019, table 1) on MobileNetV2's frame: a 32-channel 3x3 / 2 first layer, seven MBConv
    stages (expansion, channels, repeats, stride, depthwise filter), a 1280-channel 1x1 head.  9 of its 16 depthwise layers are 5x5, with
    padding 2 carried by the convolution (torchvision's and timm's spelling; not the reference's F.pad in front of an unpadded one)."""

    SETTINGS = ((1, 16, 1, 1, 3), (6, 24, 2, 2, 3), (6, 40, 2, 2, 5), (6, 80, 3, 2, 3), (6, 112, 3, 1, 5), (6, 192, 4, 2, 5), (6, 320, 1, 1, 3))


class MobileNetV3Block(nn.Module):
    """MobileNetV3's unit (Howard et al. 2019): 1x1 expansion to `expanded` channels (omitted where that is the input width) + depthwise
    `k` x `k` + linear 1x1 projection, BN after every convolution, `act` ("relu" or "hardswish") after the first two; with `se` the
    squeeze-excite gate between the depthwise and the projection layer (1x1 convolutions, a quarter of the expanded width rounded up
    to a multiple of 8, ReLU, hard sigmoid); the identity shortcut where stride is 1 and the width is kept."""

    def __init__(self, cin, k, expanded, cout, se, act, stride):
        super().__init__()
        self.use_res = stride == 1 and cin == cout
        layers = [_conv_bn_act(cin, expanded, 1, act=act)] if expanded != cin else []
        layers += [_conv_bn_act(expanded, expanded, k, stride, groups=expanded, act=act)]
        if se:
            layers += [SqueezeExcite(expanded, (expanded // 4 + 7) // 8 * 8, gate="hardsigmoid", squeeze="conv")]
        layers += [nn.Sequential(nn.Conv2d(expanded, cout, 1, bias=False), nn.BatchNorm2d(cout))]
        self.block = nn.Sequential(*layers)

    def forward(self, x):
        return x + self.block(x) if self.use_res else self.block(x)


class MobileNetV3(nn.Module):
    """MobileNetV3 (public architecture, Howard et al. 2019, tables 1 and 2) in torchvision's module layout - `features.N` blocks whose
    convolutions stand in front of their BatchNorm (merge_bn's default mapping), `avgpool`, a Linear -> Hardswish -> Dropout -> Linear
    classifier.  `rows`: (depthwise filter, expanded, out, SE, activation "RE" | "HS", stride) per block; the first layer is 3x3 / 2 to
    16 channels, the last 1x1 to six times the last block's width, both with hard swish; `hidden`: the classifier's width.  Large:
    5 483 032 parameters, Small: 2 542 856."""

    LARGE = ((3, 16, 16, False, "RE", 1), (3, 64, 24, False, "RE", 2), (3, 72, 24, False, "RE", 1), (5, 72, 40, True, "RE", 2),
             (5, 120, 40, True, "RE", 1), (5, 120, 40, True, "RE", 1), (3, 240, 80, False, "HS", 2), (3, 200, 80, False, "HS", 1),
             (3, 184, 80, False, "HS", 1), (3, 184, 80, False, "HS", 1), (3, 480, 112, True, "HS", 1), (3, 672, 112, True, "HS", 1),
             (5, 672, 160, True, "HS", 2), (5, 960, 160, True, "HS", 1), (5, 960, 160, True, "HS", 1))
    SMALL = ((3, 16, 16, True, "RE", 2), (3, 72, 24, False, "RE", 2), (3, 88, 24, False, "RE", 1), (5, 96, 40, True, "HS", 2),
             (5, 240, 40, True, "HS", 1), (5, 240, 40, True, "HS", 1), (5, 120, 48, True, "HS", 1), (5, 144, 48, True, "HS", 1),
             (5, 288, 96, True, "HS", 2), (5, 576, 96, True, "HS", 1), (5, 576, 96, True, "HS", 1))

    def __init__(self, rows, hidden, num_classes=1000, dropout=0.2):
        super().__init__()
        cin = 16
        feats = [_conv_bn_act(3, cin, 3, stride=2, act="hardswish")]
        for k, expanded, cout, se, act, stride in rows:
            feats.append(MobileNetV3Block(cin, k, expanded, cout, se, {"RE": "relu", "HS": "hardswish"}[act], stride))
            cin = cout
        feats.append(_conv_bn_act(cin, 6 * cin, 1, act="hardswish"))
        self.features = nn.Sequential(*feats)
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.classifier = nn.Sequential(nn.Linear(6 * cin, hidden), nn.Hardswish(), nn.Dropout(dropout), nn.Linear(hidden, num_classes))
        _init(self)

    def forward(self, x):
        return self.classifier(torch.flatten(self.avgpool(self.features(x)), 1))


class CifarResNet(nn.Module):
    """The CIFAR ResNet of He et al. 2016, section 4.2 (public architecture): a 3x3 first layer of 16 channels on the 32 x 32 image, three
    stages of `depth` BasicBlocks at 16 / 32 / 64 channels (stride 2 into the second and third), global average pool, linear head.  Where
    the shape changes the shortcut is a 1x1 convolution + BN (BasicBlock's `downsample`; "option B") or, with `option="A"`, the paper's
    parameter-free one: x subsampled at the stride, its channels zero-padded on both sides (what its CIFAR experiments use).  `option="C"`:
    an average pool at the stride, then a 1x1 / stride 1 convolution + BN; `option="D"`: C, and a 1x1 convolution + BN on every stride-1
    shortcut too (cifarresnet.py:57-87)."""

    def __init__(self, depth, num_classes=10, option="B"):
        super().__init__()
        self.conv1 = _conv(3, 16, 3)
        self.bn1 = nn.BatchNorm2d(16)
        self.relu = nn.ReLU(inplace=True)
        cin, stages = 16, []
        for i, width in enumerate((16, 32, 64)):
            stages.append(nn.Sequential(*[BasicBlock(cin if j == 0 else width, width, 2 if (j == 0 and i > 0) else 1, option)
                                          for j in range(depth)]))
            cin = width
        self.layer1, self.layer2, self.layer3 = stages
        self.avgpool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(cin, num_classes)
        _init(self)

    def forward(self, x):
        x = self.relu(self.bn1(self.conv1(x)))
        x = self.layer3(self.layer2(self.layer1(x)))
        return self.fc(torch.flatten(self.avgpool(x), 1))


class ViTAttention(nn.Module):
    """Multi-head self-attention on tokens [B, T, dim]: one Linear to q, k and v (no bias), softmax(q k^T / sqrt(d)) v per head, one
    Linear back to `dim`.  The two Linear layers are the quantisable part; the products and the softmax run in torch."""

    def __init__(self, dim, heads, dim_head):
        super().__init__()
        self.heads, self.dim_head = heads, dim_head
        self.to_qkv = nn.Linear(dim, 3 * heads * dim_head, bias=False)
        self.to_out = nn.Linear(heads * dim_head, dim)

    def forward(self, x):
        qkv = self.to_qkv(x)
        b, t = qkv.shape[0], qkv.shape[1]      # (read off the projection, not off x: the plan may hand to_qkv codes and write no fp32 x)
        qkv = qkv.reshape(b, t, 3, self.heads, self.dim_head).permute(2, 0, 3, 1, 4)      # [3, B, heads, T, d]
        q, k, v = qkv[0], qkv[1], qkv[2]
        attn = torch.softmax(torch.matmul(q, k.transpose(-1, -2)) * self.dim_head ** -0.5, dim=-1)
        out = torch.matmul(attn, v).permute(0, 2, 1, 3).reshape(b, t, self.heads * self.dim_head)
        return self.to_out(out)


class ViTBlock(nn.Module):
    """A pre-norm encoder block: x = attn(norm(x)) + x; x = ff(norm(x)) + x, ff = Linear -> GELU -> Linear."""

    def __init__(self, dim, heads, dim_head, mlp_dim):
        super().__init__()
        self.norm1, self.attn = nn.LayerNorm(dim), ViTAttention(dim, heads, dim_head)
        self.norm2, self.fc1, self.act, self.fc2 = nn.LayerNorm(dim), nn.Linear(dim, mlp_dim), nn.GELU(), nn.Linear(mlp_dim, dim)

    def forward(self, x):
        x = self.attn(self.norm1(x)) + x
        return self.fc2(self.act(self.fc1(self.norm2(x)))) + x


class ViT(nn.Module):
    """The vision transformer (public architecture, Dosovitskiy et al. 2021; the reference's spelling of it, model/classification/vit.py:
    patches embedded by a Linear on the flattened patch, a cls token, a learned position embedding, pre-norm blocks, a LayerNorm -> Linear
    head on the cls token) in plain torch - reshape / permute only.  Every Linear's in-features must be a multiple of 64 for the int8
    plan to take it: patch_size^2 * channels, dim, heads * dim_head and mlp_dim."""

    def __init__(self, image_size=224, patch_size=16, num_classes=1000, dim=384, depth=12, heads=6, mlp_dim=1536, dim_head=64, channels=3):
        super().__init__()
        if image_size % patch_size:
            raise ValueError(f"ViT: image size {image_size} is no multiple of the patch size {patch_size}")
        self.patch, self.grid, self.channels = patch_size, image_size // patch_size, channels
        self.embed = nn.Linear(channels * patch_size * patch_size, dim)
        self.cls_token = nn.Parameter(torch.randn(1, 1, dim) * 0.02)
        self.pos_embedding = nn.Parameter(torch.randn(1, self.grid * self.grid + 1, dim) * 0.02)
        self.blocks = nn.Sequential(*[ViTBlock(dim, heads, dim_head, mlp_dim) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim)
        self.head = nn.Linear(dim, num_classes)

    def forward(self, img):
        p, g = self.patch, self.grid
        # [B, C, g p, g p] -> [B, g g, p p C]: one row per patch, its pixels row-major with the channels innermost
        x = img.reshape(-1, self.channels, g, p, g, p).permute(0, 2, 4, 3, 5, 1).reshape(-1, g * g, p * p * self.channels)
        x = self.embed(x)
        x = torch.cat((self.cls_token.expand(x.shape[0], -1, -1), x), dim=1) + self.pos_embedding
        x = self.blocks(x)
        return self.head(self.norm(x[:, 0]))


def _init(model):
    for m in model.modules():
        if isinstance(m, nn.Conv2d):
            nn.init.kaiming_normal_(m.weight, mode="fan_in", nonlinearity="relu")
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.Linear):
            nn.init.kaiming_normal_(m.weight, mode="fan_in", nonlinearity="relu")
            nn.init.zeros_(m.bias)


def resnet18(num_classes=1000):
    return ResNet(BasicBlock, (2, 2, 2, 2), num_classes)


def resnet50(num_classes=1000):
    return ResNet(Bottleneck, (3, 4, 6, 3), num_classes)


def repvgg_a1_deploy(num_classes=1000):
    """RepVGG-A1: num_blocks [2,4,14,1], width multipliers [1,1,1,2.5] (repvgg.py:205-207)."""
    return RepVGGDeploy((2, 4, 14, 1), (64, 64, 128, 256, 1280), num_classes)


def mobileone_s1_deploy(num_classes=1000):
    return MobileOneDeploy(num_classes=num_classes)


def mobilenet_v2(num_classes=1000, se=False, act="relu6"):
    """MobileNetV2; `se=True`: with a squeeze-excite gate in every inverted-residual block (17 gates; the default network is unchanged).
    `act="swish"`: x * sigmoid(x) where ReLU6 was (35 swishes on maps) and, with `se`, EfficientNet's squeeze-excite block - its MBConv
    at MobileNetV2's widths."""
    return MobileNetV2(num_classes=num_classes, se=se, act=act)


def efficientnet_b0(num_classes=1000, se=True, act="swish"):
    """EfficientNet-B0: MBConv blocks (`mobilenet_v2(se=True, act="swish")`'s) with the paper's stage table - 5x5 depthwise layers in
    stages 3, 5 and 6.  `se` / `act` as in mobilenet_v2."""
    return EfficientNetB0(num_classes=num_classes, se=se, act=act)


def mobilenet_v3_large(num_classes=1000):
    """MobileNetV3-Large: 15 blocks, a 960-channel last layer, a 1280-wide classifier; 20 hard swishes on maps, 8 squeeze-excite gates."""
    return MobileNetV3(MobileNetV3.LARGE, 1280, num_classes)


def mobilenet_v3_small(num_classes=1000):
    """MobileNetV3-Small: 11 blocks, a 576-channel last layer, a 1024-wide classifier; 18 hard swishes on maps, 9 squeeze-excite gates."""
    return MobileNetV3(MobileNetV3.SMALL, 1024, num_classes)


def vit_tiny(num_classes=1000):
    """ViT-Ti/16: dim 192, depth 12, 3 heads of 64, MLP 768, 224^2 images (197 tokens)."""
    return ViT(224, 16, num_classes, dim=192, depth=12, heads=3, mlp_dim=768)


def vit_small(num_classes=1000):
    """ViT-S/16: dim 384, depth 12, 6 heads of 64, MLP 1536, 224^2 images (197 tokens)."""
    return ViT(224, 16, num_classes, dim=384, depth=12, heads=6, mlp_dim=1536)


def _named_option(option):
    # the named CIFAR networks are the ones they were: options "A" and "B" (tests/test_pad_shortcut_host.py pins that anything else is
    # refused here); the average-pooled shortcuts "C" / "D" are built with CifarResNet(depth, option=...) itself
    if option not in ("A", "B"):
        raise ValueError(f"cifar_resnet20 / cifar_resnet56: shortcut option 'A' or 'B', not {option!r} (CifarResNet(depth, option=...) takes 'C' and 'D')")
    return option


def cifar_resnet20(num_classes=10, option="B"):
    """ResNet-20 for CIFAR: 6 * 3 + 2 layers, widths 16 / 32 / 64 - every block of its first two stages has channel-padded outputs.
    `option="A"`: parameter-free shortcuts (20 layers: no shortcut convolutions).  (Average-pooled shortcuts: CifarResNet(3, option="C" / "D"),
    22 / 29 layers.)"""
    return CifarResNet(3, num_classes, _named_option(option))


def cifar_resnet56(num_classes=10, option="B"):
    """ResNet-56 for CIFAR: 6 * 9 + 2 layers."""
    return CifarResNet(9, num_classes, _named_option(option))


MODELS = {"resnet18": resnet18, "resnet50": resnet50, "repvgg_a1": repvgg_a1_deploy, "mobileone_s1": mobileone_s1_deploy,
          "mobilenet_v2": mobilenet_v2}


def layer_table(model, x):
    """[(name, kind, input_shape, weight_shape, macs)] of every Conv2d / Linear, by a hooked forward."""
    rows, hooks = [], []

    def hook(name):
        def fn(mod, inp, out):
            w = mod.weight
            macs = out.numel() // out.shape[0] * (w.numel() // w.shape[0])
            rows.append((name, type(mod).__name__, tuple(inp[0].shape), tuple(w.shape), macs))
        return fn
    for name, m in model.named_modules():
        if isinstance(m, (nn.Conv2d, nn.Linear)):
            hooks.append(m.register_forward_hook(hook(name)))
    was = model.training
    model.eval()
    with torch.no_grad():
        model(x)
    model.train(was)
    for h in hooks:
        h.remove()
    return rows


def table_totals(rows):
    """(layers, input elems per image, weight elems, MACs per image)."""
    n = rows[0][2][0]
    act = sum(int(torch.tensor(r[2]).prod()) for r in rows) // n
    wt = sum(int(torch.tensor(r[3]).prod()) for r in rows)
    return len(rows), act, wt, sum(r[4] for r in rows)
