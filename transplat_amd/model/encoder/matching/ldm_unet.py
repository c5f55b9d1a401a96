"""LDM-style 2-D U-Net with cross-view self-attention, as configured by DepthPredictorTrans
(reference src/model/encoder/matching/ldm_unet/{unet.py:589-1144, util.py}).

Only the configuration the depth predictor instantiates is built: postnorm ResBlocks, conv
down/up-sampling, legacy QKV attention at the requested resolutions with views folded into the
token axis, middle block = ResBlock, Identity, ResBlock. Module indices and parameter names
follow the reference (`input_blocks.{i}.{j}`, `middle_block.{0,2}`, `output_blocks.{i}.{j}`,
`out.{0,1}`) so checkpoint keys load. Every convolution takes the route kernels.SITE_UNET gives it (the
HIP kernels read the skip concat / nearest upsample in place; the full-resolution fp32 1x1s are library
GEMMs; under bf16 autocast the shapes the bf16 kernel does not take stay on the library); every
GroupNorm runs as one fused gfx950 kernel pair together with the activation and residual add
that follow it in the reference's module chain (kernels.group_norm).
"""
from __future__ import annotations

import math

import torch
from einops import rearrange
from torch import nn

from .... import kernels

_ACT_OF = {nn.SiLU: "silu", nn.GELU: "gelu"}


def gn_act(norm: nn.GroupNorm, x, act: str = "none", residual=None, pre_bias=None):
    """act(norm(x + pre_bias)) [+ residual] in one fused kernel, computed in fp32 and returned in
    x's dtype (GroupNorm32 semantics: the reference normalises in float and casts back)."""
    y = kernels.group_norm(x, norm.num_groups, norm.weight, norm.bias, norm.eps, act, residual, pre_bias)
    return y.type(x.dtype)


def conv(conv: nn.Module, x, x2=None, upsample: bool = False, bias: bool = True, decided=None):
    """conv(cat([x, x2], 1) (nearest-upsampled 2x if upsample)) [+ bias] on the route of kernels.SITE_UNET
    (decided: the caller's (call, route)); the concat / upsample are read in place where the kernel can."""
    srcs = (x,) if x2 is None else (x, x2)
    call, route = decided or (kernels.conv_module_call(conv, srcs, upsample), None)
    route = route or kernels.conv_route(call, kernels.SITE_UNET)
    return kernels.conv_run(route, call, conv.weight, srcs, conv.bias if bias else None)


def conv_gn_act(conv_mod: nn.Module, norm: nn.GroupNorm, x, act: str = "none", residual=None, x2=None, decided=None):
    """conv -> GroupNorm -> act (-> + residual) with the conv bias folded into the norm kernel."""
    y = conv(conv_mod, x, x2, bias=False, decided=decided)
    return gn_act(norm, y, act, residual, pre_bias=conv_mod.bias)


def run_sequential(seq: nn.Sequential, x):
    """Run an nn.Sequential, fusing each GroupNorm with a SiLU / GELU that directly follows it."""
    mods = list(seq)
    i = 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, (nn.Conv1d, nn.Conv2d)) and i + 1 < len(mods) and isinstance(mods[i + 1], nn.GroupNorm):
            nxt = mods[i + 2] if i + 2 < len(mods) else None
            act = _ACT_OF.get(type(nxt)) if nxt is not None else None
            if isinstance(nxt, nn.GELU) and nxt.approximate != "none":
                act = None
            x = conv_gn_act(m, mods[i + 1], x, act or "none")
            i += 3 if act else 2
            continue
        if isinstance(m, nn.GroupNorm):
            nxt = mods[i + 1] if i + 1 < len(mods) else None
            act = _ACT_OF.get(type(nxt)) if nxt is not None else None
            if isinstance(nxt, nn.GELU) and nxt.approximate != "none":
                act = None
            x = gn_act(m, x, act or "none")
            i += 2 if act else 1
            continue
        x = m(x)
        i += 1
    return x


class GroupNorm32(nn.GroupNorm):
    def forward(self, x):
        return gn_act(self, x)


def normalization(channels):
    """GroupNorm8 when channels % 8 == 0 else GroupNorm4 (reference util.py:189-208)."""
    return GroupNorm32(8 if channels % 8 == 0 else 4, channels)


class ResBlock(nn.Module):
    """postnorm residual block (reference unet.py:177-300): conv-GN-SiLU, conv-GN-SiLU, skip."""

    def __init__(self, channels, out_channels=None, kernel_size=3):
        super().__init__()
        self.channels = channels
        self.out_channels = out_channels or channels
        pad = (kernel_size - 1) // 2
        self.in_layers = nn.Sequential(
            nn.Conv2d(channels, self.out_channels, kernel_size, padding=pad), normalization(self.out_channels),
            nn.SiLU())
        self.out_layers = nn.Sequential(
            nn.Conv2d(self.out_channels, self.out_channels, kernel_size, padding=pad),
            normalization(self.out_channels), nn.SiLU())
        self.skip_connection = (nn.Identity() if self.out_channels == channels
                                else nn.Conv2d(channels, self.out_channels, 1))

    def forward(self, x, x2=None):
        # skip + SiLU(GN(conv(SiLU(GN(conv(x)))))): both GN + SiLU pairs and the residual fused;
        # x2: the output blocks' skip input, x = cat([x, x2], 1) without materialising the concat
        # where the convolutions read it in place. Each convolution's route is decided once, here.
        c, sk = self.in_layers[0], self.skip_connection
        srcs = (x,) if x2 is None else (x, x2)
        call = kernels.conv_module_call(c, srcs)
        route = kernels.conv_route(call, kernels.SITE_UNET)
        sk_call = None if isinstance(sk, nn.Identity) else kernels.conv_module_call(sk, srcs)
        sk_route = sk_call and kernels.conv_route(sk_call, kernels.SITE_UNET)
        if x2 is not None and route != "direct":
            # bf16x3 mode, a Winograd / few-channel in_layers conv (the output blocks' skip concatenation,
            # round 6): both convolutions read cat([x, x2]) in place (the 3x3 as a two-source launch, a 1x1
            # skip on the two-source direct kernel whether or not it wins there)
            if kernels.split_mode() and route == "wino" and (sk_call is None or kernels.conv_can_direct(sk_call)):
                sk_route = "direct"
            else:
                # materialised once for both convolutions; the routes decided on the two sources run on it
                x, x2, call, sk_call = torch.cat(srcs, dim=1), None, call.joined(), sk_call and sk_call.joined()
        h = conv_gn_act(c, self.in_layers[1], x, "silu", x2=x2, decided=(call, route))
        if sk_call is None:
            skip = x if x2 is None else (x, x2)  # the concat read in place by the norm's residual add
        else:
            skip = conv(sk, x, x2, decided=(sk_call, sk_route))
        return conv_gn_act(self.out_layers[0], self.out_layers[1], h, "silu", residual=skip)


class QKVAttentionLegacy(nn.Module):
    """heads split before q/k/v; views folded into tokens ((v b) n t -> b n (v t))
    (reference unet.py:510-552)."""

    def __init__(self, n_heads, n_frames=2, use_cross_view_self_attn=False):
        super().__init__()
        self.n_heads = n_heads
        self.n_frames = n_frames
        self.use_cross_view_self_attn = use_cross_view_self_attn

    def forward(self, qkv):
        width = qkv.shape[1]
        if qkv.is_cuda and width // (3 * self.n_heads) == 32 and (
                qkv.dtype == torch.float32 or torch.is_autocast_enabled("cuda")):
            # one kernel reading / writing the (v b) layout in place (kernels.qkv_attention_cf); under
            # bf16 autocast the qkv projection's bf16 output is widened once and the attention runs in
            # fp32 (the reference's einsum path: bf16 products, fp32 softmax; 8 launches)
            return kernels.qkv_attention_cf(qkv.float(), self.n_heads,
                                            self.n_frames if self.use_cross_view_self_attn else 1)
        if self.use_cross_view_self_attn:
            qkv = rearrange(qkv, "(v b) n t -> b n (v t)", v=self.n_frames)
        bs, width, length = qkv.shape
        ch = width // (3 * self.n_heads)
        q, k, v = qkv.reshape(bs * self.n_heads, ch * 3, length).split(ch, dim=1)
        scale = 1 / math.sqrt(math.sqrt(ch))
        weight = torch.einsum("bct,bcs->bts", q * scale, k * scale)
        weight = torch.softmax(weight.float(), dim=-1).type(weight.dtype)
        a = torch.einsum("bts,bcs->bct", weight, v).reshape(bs, -1, length)
        if self.use_cross_view_self_attn:
            a = rearrange(a, "b n (v t) -> (v b) n t", v=self.n_frames)
        return a


class AttentionBlock(nn.Module):
    """postnorm self-attention block (reference unet.py:306-370)."""

    def __init__(self, channels, num_head_channels=32, num_frames=2, use_cross_view_self_attn=False):
        super().__init__()
        self.channels = channels
        self.num_heads = channels // num_head_channels
        self.qkv = nn.Conv1d(channels, channels * 3, 1)
        self.attention = QKVAttentionLegacy(self.num_heads, n_frames=num_frames,
                                            use_cross_view_self_attn=use_cross_view_self_attn)
        self.proj_out = nn.Conv1d(channels, channels, 1)
        self.norm = normalization(channels)

    def forward(self, x):
        b, c, *spatial = x.shape
        x = x.reshape(b, c, -1)
        h = self.attention(conv(self.qkv, x))
        return conv_gn_act(self.proj_out, self.norm, h, residual=x).reshape(b, c, *spatial)


class Downsample(nn.Module):
    def __init__(self, channels, out_channels=None):
        super().__init__()
        self.channels = channels
        self.op = nn.Conv2d(channels, out_channels or channels, 3, stride=2, padding=1)

    def forward(self, x):
        return conv(self.op, x)


class Upsample(nn.Module):
    def __init__(self, channels, out_channels=None):
        super().__init__()
        self.channels = channels
        self.conv = nn.Conv2d(channels, out_channels or channels, 3, padding=1)

    def forward(self, x):
        return conv(self.conv, x, upsample=True)


class UNetModel(nn.Module):
    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions,
                 dropout=0, channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, postnorm=False,
                 num_head_channels=-1, num_frames=2, use_cross_view_self_attn=False, **kwargs):
        super().__init__()
        if dims != 2 or not postnorm or not conv_resample or num_head_channels <= 0:
            raise NotImplementedError("only the DepthPredictorTrans configuration is built")
        self.in_channels = in_channels
        self.model_channels = model_channels
        self.out_channels = out_channels
        attn = lambda ch: AttentionBlock(ch, num_head_channels=num_head_channels, num_frames=num_frames,
                                         use_cross_view_self_attn=use_cross_view_self_attn)
        self.input_blocks = nn.ModuleList([nn.Sequential(nn.Conv2d(in_channels, model_channels, 3, padding=1))])
        input_block_chans = [model_channels]
        ch = model_channels
        ds = 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [ResBlock(ch, out_channels=mult * model_channels)]
                ch = mult * model_channels
                if ds in attention_resolutions:
                    layers.append(attn(ch))
                self.input_blocks.append(nn.Sequential(*layers))
                input_block_chans.append(ch)
            if level != len(channel_mult) - 1:
                self.input_blocks.append(nn.Sequential(Downsample(ch, out_channels=ch)))
                input_block_chans.append(ch)
                ds *= 2
        self.middle_block = nn.Sequential(ResBlock(ch), nn.Identity(), ResBlock(ch))
        self.output_blocks = nn.ModuleList([])
        for level, mult in list(enumerate(channel_mult))[::-1]:
            for i in range(num_res_blocks + 1):
                ich = input_block_chans.pop()
                layers = [ResBlock(ch + ich, out_channels=model_channels * mult)]
                ch = model_channels * mult
                if ds in attention_resolutions:
                    layers.append(attn(ch))
                if level and i == num_res_blocks:
                    layers.append(Upsample(ch, out_channels=ch))
                    ds //= 2
                self.output_blocks.append(nn.Sequential(*layers))
        self.out = nn.Sequential(nn.Conv2d(model_channels, out_channels, 3, padding=1), normalization(out_channels),
                                 nn.SiLU())

    def forward(self, x, timesteps=None, context=None, y=None, **kwargs):
        hs = []
        h = x
        for module in self.input_blocks:
            h = module(h)
            hs.append(h)
        h = self.middle_block(h)
        for module in self.output_blocks:
            # ResBlock(cat([h, skip])): the concat is read in place by its convolutions
            mods = list(module)
            h = mods[0](h, hs.pop())
            for m in mods[1:]:
                h = m(h)
        return run_sequential(self.out, h)
