"""Depth-Anything-V2 DPT head + model (reference src/depth_anything_v2/dpt.py:38-184,
util/blocks.py). Returns (relative depth [B, H, W], the 64-channel output_conv1 feature) exactly
as the reference forward does; parameter names match (`depth_head.{projects,resize_layers,
scratch.{layer*_rn,refinenet*,output_conv*}}`)."""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn


from ... import kernels
from .dinov2 import DINOv2

# The token maps enter the DPT as channels-last views (permute of [B, N, C]); the whole conv chain
# then runs MIOpen's NHWC kernels, measured ~4% faster end-to-end than an NCHW copy up front. The
# conv weights are laid out channels-last once (first forward) so torch stops re-laying them out
# on every call. The convolutions stay on MIOpen with their epilogues (bias + ReLU, bias + residuals)
# fused after them: as the channels-last direct kernel (kernels.conv2d_nhwc) the latency-bound ones
# (ResidualConvUnits <= 36^2, out_convs) measured 2.0 % SLOWER end to end, the units alone 1.3 %: its
# pixel-per-lane B gathers touch 32 cache lines per load on a channels-last map.
# The reassemble branches run after the last ViT block: forked onto a side stream while the later
# blocks run they measured SLOWER end to end (profiles/r3/ab_r3c: C2 332 vs 356 views/s, C3 849 vs
# 887): the branches' MIOpen convolutions take CUs from the critical path (DINOv2 blocks and the
# backbone beside them) rather than filling idle ones. Round 6 (hand-written DINOv2 GEMMs): still
# slower, 444.7 vs 487.6 views/s same box (profiles/r6/ab_c2_dpt_hoist.txt).
# bf16x3 dense mode (kernels.dense_precision): the head runs on NCHW maps instead, so its 3x3
# convolutions take the bf16x3 Winograd kernel with the ResidualConvUnit glue fused (ReLU on load,
# bias, + x, + the fusion block's skip: two launches per unit) and the 1x1s the direct kernel. The projects'
# 1x1 reads the token rows where they lie and the transposed convolutions' 1x1 stores pixel-shuffled
# (kernels.conv1x1_rows, conv_transpose_direct): no layout copy is left in reassemble. The depth
# after output_conv1 (depth_tail) can be left to the caller, who needs it a whole matching stage later.


def _nchw3() -> bool:
    return kernels.split_mode()


def _resize(x, modifier: dict, align_corners: bool):
    """F.interpolate(x, **modifier, mode="bilinear", align_corners=...); the channels-last fp32 maps
    of the head go through one kernel (kernels.resize_bilinear_nhwc) instead of torch's NHWC
    interpolation kernel."""
    # (bilinear upsampling runs in fp32 under autocast: a bf16 map is widened first, as autocast
    # itself would, and then takes the kernel instead of torch's NHWC kernel, 88 us per call at C3)
    if (align_corners and x.is_cuda and x.dtype == torch.bfloat16 and x.shape[1] % 4 == 0
            and torch.is_autocast_enabled("cuda") and x.is_contiguous(memory_format=torch.channels_last)):
        x = x.float().contiguous(memory_format=torch.channels_last)
    if (align_corners and x.is_cuda and x.dtype == torch.float32 and x.shape[1] % 4 == 0
            and x.is_contiguous(memory_format=torch.channels_last)):
        if "size" in modifier:
            size = modifier["size"]
        else:
            sf = modifier["scale_factor"]
            size = (int(x.shape[-2] * sf), int(x.shape[-1] * sf))
        return kernels.resize_bilinear_nhwc(x, size)
    if align_corners and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous():
        # NCHW fp32 (the head's final resize; every config, fp32 included -- test_depth_anything_gpu
        # covers it in fp32): PyTorch's generic NCHW kernel took 0.87 ms per call at C3's batch 8
        if "size" in modifier:
            size = modifier["size"]
        else:
            sf = modifier["scale_factor"]
            size = (int(x.shape[-2] * sf), int(x.shape[-1] * sf))
        return kernels.interpolate_bilinear_ac(x, size)
    return F.interpolate(x, **modifier, mode="bilinear", align_corners=align_corners)


class ResidualConvUnit(nn.Module):
    def __init__(self, features, activation, bn):
        super().__init__()
        self.bn = bn
        self.conv1 = nn.Conv2d(features, features, kernel_size=3, stride=1, padding=1, bias=True)
        self.conv2 = nn.Conv2d(features, features, kernel_size=3, stride=1, padding=1, bias=True)
        if bn:
            self.bn1 = nn.BatchNorm2d(features)
            self.bn2 = nn.BatchNorm2d(features)
        self.activation = activation

    def _epilogue_ok(self, x) -> bool:
        return (not self.bn and isinstance(self.activation, nn.ReLU) and x.dtype == torch.float32
                and self.conv1.weight.dtype == torch.float32 and x.shape[1] % 4 == 0
                and not torch.is_autocast_enabled("cuda"))

    def forward(self, x, skip=None):
        """out(x) + x (+ skip: the FeatureFusionBlock's other input, added in the same pass)."""
        if (_nchw3() and not self.bn and isinstance(self.activation, nn.ReLU) and x.is_cuda and x.is_contiguous()
                and kernels.conv_route(kernels.conv_module_call(self.conv1, (x,)), kernels.SITE_FORWARD) == "wino"
                and (skip is None or skip.is_contiguous())):
            # bf16x3 mode, NCHW: relu -> conv1 + bias, relu -> conv2 + bias + x (+ skip), two launches
            out = kernels.conv3x3_wino(x, self.conv1.weight, self.conv1.bias, relu_in=True)
            return kernels.conv3x3_wino(out, self.conv2.weight, self.conv2.bias, relu_in=True, residual=x,
                                        residual2=skip)
        if self._epilogue_ok(x):
            # bias-free MIOpen convs with bias + ReLU / bias + residual(s) fused after each:
            # 3 glue launches per unit instead of 5 (6 with the fusion block's add)
            out = kernels.conv_nhwc_epilogue(self.conv1, self.activation(x), "relu")
            return kernels.conv_nhwc_epilogue(self.conv2, out, "none", x, skip)
        out = self.conv1(self.activation(x))
        if self.bn:
            out = self.bn1(out)
        out = self.conv2(self.activation(out))
        if self.bn:
            out = self.bn2(out)
        return out + x if skip is None else skip + (out + x)


class FeatureFusionBlock(nn.Module):
    def __init__(self, features, activation, bn=False, align_corners=True, size=None):
        super().__init__()
        self.align_corners = align_corners
        self.out_conv = nn.Conv2d(features, features, kernel_size=1, stride=1, padding=0, bias=True)
        self.resConfUnit1 = ResidualConvUnit(features, activation, bn)
        self.resConfUnit2 = ResidualConvUnit(features, activation, bn)
        self.size = size

    def forward(self, *xs, size=None):
        output = xs[0]
        if len(xs) == 2:
            output = self.resConfUnit1(xs[1], skip=output)  # xs[0] + unit(xs[1])
        output = self.resConfUnit2(output)
        if size is None and self.size is None:
            modifier = {"scale_factor": 2}
        elif size is None:
            modifier = {"size": self.size}
        else:
            modifier = {"size": size}
        output = _resize(output, modifier, self.align_corners)
        return self.out_conv(output)


class _Scratch(nn.Module):
    pass


class DPTHead(nn.Module):
    def __init__(self, in_channels, features=256, use_bn=False, out_channels=(256, 512, 1024, 1024),
                 use_clstoken=False):
        super().__init__()
        if use_clstoken:
            raise NotImplementedError("Depth-Anything-V2 ViT-B runs without the class-token readout")
        self.use_clstoken = use_clstoken
        self.projects = nn.ModuleList([nn.Conv2d(in_channels, oc, kernel_size=1, stride=1, padding=0)
                                       for oc in out_channels])
        self.resize_layers = nn.ModuleList([
            nn.ConvTranspose2d(out_channels[0], out_channels[0], kernel_size=4, stride=4, padding=0),
            nn.ConvTranspose2d(out_channels[1], out_channels[1], kernel_size=2, stride=2, padding=0),
            nn.Identity(),
            nn.Conv2d(out_channels[3], out_channels[3], kernel_size=3, stride=2, padding=1)])
        s = _Scratch()
        s.layer1_rn = nn.Conv2d(out_channels[0], features, 3, 1, 1, bias=False)
        s.layer2_rn = nn.Conv2d(out_channels[1], features, 3, 1, 1, bias=False)
        s.layer3_rn = nn.Conv2d(out_channels[2], features, 3, 1, 1, bias=False)
        s.layer4_rn = nn.Conv2d(out_channels[3], features, 3, 1, 1, bias=False)
        s.stem_transpose = None
        act = nn.ReLU(False)
        s.refinenet1 = FeatureFusionBlock(features, act, bn=use_bn)
        s.refinenet2 = FeatureFusionBlock(features, act, bn=use_bn)
        s.refinenet3 = FeatureFusionBlock(features, act, bn=use_bn)
        s.refinenet4 = FeatureFusionBlock(features, act, bn=use_bn)
        s.output_conv1 = nn.Conv2d(features, features // 2, kernel_size=3, stride=1, padding=1)
        s.output_conv2 = nn.Sequential(
            nn.Conv2d(features // 2, 32, kernel_size=3, stride=1, padding=1), nn.ReLU(True),
            nn.Conv2d(32, 1, kernel_size=1, stride=1, padding=0), nn.ReLU(True), nn.Identity())
        self.scratch = s

    def _channels_last_weights(self):
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.ConvTranspose2d)) and m.weight.dim() == 4:
                m.weight.data = m.weight.data.contiguous(memory_format=torch.channels_last)
        self._cl_done = True

    def prepare(self, is_cuda: bool):
        if not getattr(self, "_cl_done", False) and is_cuda and not _nchw3():
            self._channels_last_weights()

    def reassemble(self, i, x, patch_h, patch_w):
        """Branch i of the head up to layer{i+1}_rn (reference dpt.py:121-140): tokens [B, N, C] ->
        project (1x1) -> resize (convT / identity / strided conv) -> 3x3 layer_rn."""
        if _nchw3():  # NCHW maps for the bf16x3 kernels: the 1x1 reads the token rows, no permuted copy first
            x = self.resize_layers[i](kernels.conv1x1_rows(self.projects[i], x, patch_h, patch_w)).contiguous()
            return getattr(self.scratch, f"layer{i + 1}_rn")(x).contiguous()
        x = x.permute(0, 2, 1).reshape((x.shape[0], x.shape[-1], patch_h, patch_w))
        x = self.resize_layers[i](self.projects[i](x))
        return getattr(self.scratch, f"layer{i + 1}_rn")(x)

    def forward(self, out_features, patch_h, patch_w, raw_tail: bool = False, defer_tail: bool = False):
        """`raw_tail` (not in the reference): the depth may come back WITHOUT output_conv2's last
        ReLU (the bf16x3 NCHW route only); the caller applies ReLU either way. `defer_tail`: output_conv1's
        map comes back in the depth's place, for the caller to give to depth_tail later (nothing between
        output_conv1 and the depth's first reader needs the depth)."""
        self.prepare(out_features[0][0].is_cuda)
        layer_1_rn, layer_2_rn, layer_3_rn, layer_4_rn = [self.reassemble(i, x[0], patch_h, patch_w)
                                                          for i, x in enumerate(out_features)]
        s = self.scratch
        path_4 = s.refinenet4(layer_4_rn, size=layer_3_rn.shape[2:])
        path_3 = s.refinenet3(path_4, layer_3_rn, size=layer_2_rn.shape[2:])
        path_2 = s.refinenet2(path_3, layer_2_rn, size=layer_1_rn.shape[2:])
        path_1 = s.refinenet1(path_2, layer_1_rn)
        final_out = s.output_conv1(path_1)
        # nothing below writes final_out in place (_resize allocates its result): no copy needed
        out_feature = final_out.detach()
        if defer_tail:
            return final_out, out_feature
        return self.depth_tail(final_out, patch_h, patch_w, raw_tail), out_feature

    def depth_tail(self, final_out, patch_h, patch_w, raw_tail: bool = False):
        """The head after output_conv1 (reference dpt.py:150-153): resize to the image, output_conv2."""
        final_out = _resize(final_out, {"size": (int(patch_h * 14), int(patch_w * 14))}, True)
        oc = self.scratch.output_conv2
        if (_nchw3() and final_out.is_contiguous()
                and kernels.conv_route(kernels.conv_module_call(oc[0], (final_out,)), kernels.SITE_FORWARD) == "wino"):
            h = kernels.conv3x3_wino(final_out, oc[0].weight, oc[0].bias, act="relu")
            if raw_tail and isinstance(oc[3], nn.ReLU) and isinstance(oc[4], nn.Identity):
                return oc[2](h)  # the ReLUs are the caller's
            return oc[4](oc[3](oc[2](h)))
        if (final_out.dtype == torch.float32 and not torch.is_autocast_enabled("cuda")
                and final_out.is_cuda and final_out.is_contiguous(memory_format=torch.channels_last)):
            # conv -> ReLU as conv + (bias, ReLU) epilogue; the 1-channel tail stays on the modules
            h = kernels.conv_nhwc_epilogue(oc[0], final_out, "relu")
            return oc[4](oc[3](oc[2](h)))
        return oc(final_out)


class DepthAnythingV2(nn.Module):
    def __init__(self, encoder="vitl", features=256, out_channels=(256, 512, 1024, 1024), use_bn=False,
                 use_clstoken=False):
        super().__init__()
        self.intermediate_layer_idx = {"vits": [2, 5, 8, 11], "vitb": [2, 5, 8, 11], "vitl": [4, 11, 17, 23]}
        self.encoder = encoder
        self.pretrained = DINOv2(model_name=encoder)
        self.depth_head = DPTHead(self.pretrained.embed_dim, features, use_bn, out_channels=out_channels,
                                  use_clstoken=use_clstoken)

    def forward(self, x, patches=None, raw_depth: bool = False, defer_tail: bool = False):
        """x: the images [B, 3, H, W]. Not in the reference: `patches` = (patch matrix of
        kernels.da_patches, B, patch_h, patch_w) in place of x (x is then ignored); `raw_depth`: the
        depth comes back as the [B, 1, H, W] map with its trailing ReLUs possibly still to apply
        (kernels.depth_norm applies ReLU on load; it is idempotent); `defer_tail` (with raw_depth): in the
        depth's place comes the pair (fn, final_out), fn(final_out) being that depth (DPTHead.depth_tail
        on output_conv1's map), for a caller that runs it later."""
        if patches is not None:
            pm, n_img, patch_h, patch_w = patches
            tokens = self.pretrained.prepare_tokens_patches(pm, n_img, patch_h, patch_w)
            is_cuda = True
        else:
            patch_h, patch_w = x.shape[-2] // 14, x.shape[-1] // 14
            tokens = None
            is_cuda = x.is_cuda
        head = self.depth_head
        head.prepare(is_cuda)
        from ...misc.benchmarker import stage

        with stage(None, "da_dinov2"):  # diagnostic sub-stage marks (TSPLAT_MARKS / TSPLAT_ROCTX)
            features = self.pretrained.get_intermediate_layers(x, self.intermediate_layer_idx[self.encoder],
                                                               return_class_token=True, tokens=tokens)
        with stage(None, "da_dpt"):
            depth, out_features = head(features, patch_h, patch_w, raw_tail=raw_depth, defer_tail=defer_tail)
        if defer_tail:
            if not raw_depth:
                raise ValueError("defer_tail returns the raw depth's tail: raw_depth must be set")
            return (lambda final_out: head.depth_tail(final_out, patch_h, patch_w, True), depth), out_features
        if raw_depth:
            return depth, out_features
        return F.relu(depth).squeeze(1), out_features
