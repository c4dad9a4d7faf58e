"""Ego-pose decoder `ResNetLike` of the "sequence" branch -- counterpart of reference
model/modeling/pose_decoder/resnet_like_pose_decoder.py:7-72 (same module tree and state-dict names: `layer{1-4}.{0,1,2}`, `squeeze`,
`convs.pose_{0,1,2}`; channel counts hard-wired to the concatenated (previous, current) Swin-T features, :33-36).
Two paths, chosen by the module's mode.  `eval()`: every convolution is a HIP GEMM with the folded BatchNorm / bias / ReLU in its epilogue
(uenc/convnet.py, detached cached operands, no gradient).  `train()`: every conv + BatchNorm (+ shortcut add) (+ ReLU) is one
`ops.conv_bn_act` node on channels-last maps, the biased 1x1 / 3x3 convolutions are `LinearFn` / `Conv3x3Fn`; a BatchNorm child in
training mode normalises with batch statistics and updates its running ones, one put in `eval()` uses the running statistics."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ...convnet import conv, conv_bn_act


class ResidualBlock(nn.Module):
    def __init__(self, inchannel, outchannel, stride=1):
        super().__init__()
        self.left = nn.Sequential(nn.Conv2d(inchannel, outchannel, kernel_size=3, stride=stride, padding=1, bias=False),
                                  nn.BatchNorm2d(outchannel), nn.ReLU(inplace=True),
                                  nn.Conv2d(outchannel, outchannel, kernel_size=3, stride=1, padding=1, bias=False), nn.BatchNorm2d(outchannel))
        self.shortcut = nn.Sequential()
        if stride != 1 or inchannel != outchannel:
            self.shortcut = nn.Sequential(nn.Conv2d(inchannel, outchannel, kernel_size=1, stride=stride, bias=False), nn.BatchNorm2d(outchannel))
    act = staticmethod(F.relu)

    @staticmethod
    def _cba(x, c, bn, **kw):
        return ops.conv_bn_act(x, c.weight, bn, kind=c.kernel_size[0], stride=c.stride[0], train=bn.training, **kw)

    def forward_train(self, x):
        """x (B, H, W, C) channels-last -> (B, H', W', C') fp32."""
        out = self._cba(x, self.left[0], self.left[1], relu=True, out_dtype=ops.BF16)
        sc = self._cba(x, self.shortcut[0], self.shortcut[1]) if len(self.shortcut) else x
        return self._cba(out, self.left[3], self.left[4], residual=sc, relu=True)

    def forward(self, x):
        out = conv_bn_act(x, self.left[0], self.left[1], relu=True, out_dtype=torch.bfloat16)
        out = conv_bn_act(out, self.left[3], self.left[4])
        sc = conv_bn_act(x, self.shortcut[0], self.shortcut[1]) if len(self.shortcut) else x.float()
        return self.act(out + sc)


class ResNetLike(nn.Module):
    def __init__(self, ResidualBlock=ResidualBlock, num_input_features=1, num_frames_to_predict_for=2):
        super().__init__()
        self.layer1 = self.make_layer(ResidualBlock, 192, 64, 2, stride=2)
        self.layer2 = self.make_layer(ResidualBlock, 384 + 64, 128, 2, stride=2)
        self.layer3 = self.make_layer(ResidualBlock, 768 + 128, 256, 2, stride=2)
        self.layer4 = self.make_layer(ResidualBlock, 1536 + 256, 512, 2, stride=2)
        self.squeeze = nn.Conv2d(512, 256, 1)
        self.relu = nn.ReLU()
        self.convs = nn.ModuleDict({"pose_0": nn.Conv2d(num_input_features * 256, 256, 3, 1, 1), "pose_1": nn.Conv2d(256, 256, 3, 1, 1),
                                    "pose_2": nn.Conv2d(256, 6 * num_frames_to_predict_for, 1)})
        self.num_frames_to_predict_for = num_frames_to_predict_for

    def make_layer(self, block, in_channels, out_channels, num_blocks, stride):
        layers = [nn.Conv2d(in_channels, out_channels, 1)]
        for s in [stride] + [1] * (num_blocks - 1):
            layers.append(block(out_channels, out_channels, s))
        return nn.Sequential(*layers)

    @staticmethod
    def _run(seq, x):
        x = conv(x, seq[0])
        for blk in list(seq)[1:]:
            x = blk(x)
        return x

    @staticmethod
    def _run_train(seq, x):
        x = ops.linear(x, seq[0].weight, seq[0].bias, out_dtype=ops.F32)
        for blk in list(seq)[1:]:
            x = blk.forward_train(x)
        return x

    def _forward_train(self, features):
        """The differentiable path on channels-last maps; gradient reaches the (concatenated) backbone features."""
        res2, res3, res4, res5 = (features[k].permute(0, 2, 3, 1) for k in ("res2", "res3", "res4", "res5"))
        out = self._run_train(self.layer1, res2)
        out = self._run_train(self.layer2, torch.cat([out, res3.float()], dim=-1))
        out = self._run_train(self.layer3, torch.cat([out, res4.float()], dim=-1))
        out = self._run_train(self.layer4, torch.cat([out, res5.float()], dim=-1))
        B, H, W, _ = out.shape
        out = F.relu(ops.linear(out, self.squeeze.weight, self.squeeze.bias, out_dtype=ops.F32))
        out = F.relu(ops.conv3x3(out, self.convs["pose_0"].weight, self.convs["pose_0"].bias)).view(B, H, W, -1)
        out = F.relu(ops.conv3x3(out, self.convs["pose_1"].weight, self.convs["pose_1"].bias)).view(B, H, W, -1)
        out = ops.linear(out, self.convs["pose_2"].weight, self.convs["pose_2"].bias, out_dtype=ops.F32)
        out = out.float().mean(2).mean(1)
        out = 0.01 * out.view(-1, self.num_frames_to_predict_for, 1, 6)
        return out[..., :3], out[..., 3:]

    def forward(self, features):
        if self.training:
            with ops.ordered_wgrads():              # weight gradients summed in a fixed order
                return self._forward_train(features)
        res2, res3, res4, res5 = features["res2"], features["res3"], features["res4"], features["res5"]
        out = self._run(self.layer1, res2)
        out = self._run(self.layer2, torch.cat([out, res3.float()], dim=1))
        out = self._run(self.layer3, torch.cat([out, res4.float()], dim=1))
        out = self._run(self.layer4, torch.cat([out, res5.float()], dim=1))
        out = conv(out, self.squeeze, relu=True)
        out = conv(out, self.convs["pose_0"], relu=True)
        out = conv(out, self.convs["pose_1"], relu=True)
        out = conv(out, self.convs["pose_2"])
        out = out.mean(3).mean(2)
        out = 0.01 * out.view(-1, self.num_frames_to_predict_for, 1, 6)
        return out[..., :3], out[..., 3:]
