"""The refinement U-Net's blocks restated in plain torch on the CPU, in one of four arithmetics, and
with the index mistakes a block-level test must catch (tests/test_unet_blocks.py).

Every restatement takes the module (transplat_amd.model.encoder.matching.ldm_unet: ResBlock,
AttentionBlock, Downsample, Upsample, UNetModel) for its parameters only and never calls its forward
(reference ldm_unet/unet.py: ResBlock :177-300, AttentionBlock :306-370, QKVAttentionLegacy :510-552,
Upsample :128-137, Downsample :160-170, UNetModel.forward :1084-1104).

Arithmetics (`Arith`):
  f64   everything in float64: the reference of every test
  f32   the same statement in plain torch fp32
  x3    float64, every convolution's product an ideal split-bf16 product of fp32-rounded operands
        (x3_ideal: hi = bf16(x), lo = bf16(x - hi), hi hi' + hi lo' + lo hi')
  bf16  fp32 parameters under torch.autocast("cpu", bfloat16); GroupNorm as GroupNorm32 (normalise
        x.float(), cast back), the softmax in float

Mutations (`mut`, a set of names; float64 only makes sense): see MUTANTS.
"""
from __future__ import annotations

import math

import torch

F = torch.nn.functional

MUTANTS = {
    "concat_swap": "cat([x2, x]) where the block computes cat([x, x2])",
    "no_bias1": "the first convolution's bias dropped (the norm kernel's pre_bias lost)",
    "no_bias2": "the second convolution's bias dropped",
    "skip_x_only": "the skip path sees x and zeros where x2 is",
    "gn_groups": "the 4-group GroupNorm run with the 8-group form's c // 8 channels per group (9 groups at c = 36)",
    "no_proj_bias": "proj_out's bias dropped (the attention block's pre_bias)",
    "vb_as_bv": "the batch read as (b v) where it is laid out (v b)",
    "no_fold": "views not folded into the tokens: every image attends to itself only",
    "stride_offset": "the stride-2 convolution sampled one pixel off",
    "zero_insert": "zero insertion where the upsample is nearest-neighbour",
}


def bf16_hi(t: torch.Tensor, truncate: bool = False) -> torch.Tensor:
    """The bf16 image of fp32 t (round to nearest even, or the biased truncation), as float64."""
    if truncate:
        return (t.float().contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).double()
    return t.float().bfloat16().double()


def x3_ideal(op, x, w, truncate: bool = False):
    """An ideal bf16x3 product in float64: hi = bf16(x), lo = bf16(x - hi), hi hi' + hi lo' + lo hi'."""
    xh, wh = bf16_hi(x, truncate), bf16_hi(w, truncate)
    xl, wl = (x.double() - xh).float().bfloat16().double(), (w.double() - wh).float().bfloat16().double()
    return op(xh, wh + wl) + op(xl, wh)


def rel_err(out, ref) -> float:
    """max |out - ref| / max |ref|, in float64."""
    ref = ref.double()
    return ((out.double() - ref).abs().max() / ref.abs().max()).item()


class Arith:
    """One arithmetic class: how convolutions, norms and the attention products are computed."""

    def __init__(self, kind: str):
        if kind not in ("f64", "f32", "x3", "bf16"):
            raise ValueError(kind)
        self.kind = kind
        self.dtype = torch.float64 if kind in ("f64", "x3") else torch.float32

    def cast(self, t):
        return None if t is None else t.detach().to(self.dtype)

    def conv(self, x, weight, bias, stride: int = 1, padding: int = 0):
        """conv2d / conv1d (by the weight's rank) of x with the module's parameters."""
        op = F.conv1d if weight.dim() == 3 else F.conv2d
        if self.kind == "x3":
            y = x3_ideal(lambda a, b: op(a, b, None, stride, padding), x.float(), weight.detach().float())
            if bias is not None:
                y = y + bias.detach().double().view(1, -1, *([1] * (weight.dim() - 2)))
            return y
        if self.kind == "bf16":
            with torch.autocast("cpu", dtype=torch.bfloat16):
                return op(x, weight.detach(), None if bias is None else bias.detach(), stride, padding)
        return op(x, self.cast(weight), self.cast(bias), stride, padding)

    def norm(self, x, norm, groups: int | None = None):
        """GroupNorm32: normalise in float (float64 for the f64 / x3 classes), cast back to x's dtype."""
        wide = x.float() if self.kind == "bf16" else x
        y = F.group_norm(wide, groups or norm.num_groups, self.cast(norm.weight), self.cast(norm.bias), norm.eps)
        return y.to(x.dtype)

    def attend(self, q, k, v):
        """softmax(q^T k) v over [b, c, t] operands; the softmax in float (float64: f64 / x3)."""
        if self.kind == "bf16":
            with torch.autocast("cpu", dtype=torch.bfloat16):
                w = torch.einsum("bct,bcs->bts", q, k)
                w = torch.softmax(w.float(), dim=-1).type(w.dtype)
                return torch.einsum("bts,bcs->bct", w, v)
        w = torch.softmax(torch.einsum("bct,bcs->bts", q, k), dim=-1)
        return torch.einsum("bts,bcs->bct", w, v)


F64 = Arith("f64")


def res_block(m, x, x2=None, ar: Arith = F64, mut=frozenset()):
    """skip(cat) + silu(gn(conv(silu(gn(conv(cat)))))), cat = cat([x, x2], 1)."""
    x = ar.cast(x)
    x2 = ar.cast(x2)
    if x2 is None:
        cat = skip_in = x
    else:
        cat = torch.cat([x2, x] if "concat_swap" in mut else [x, x2], dim=1)
        skip_in = torch.cat([x, torch.zeros_like(x2)], dim=1) if "skip_x_only" in mut else cat
    c1, n1 = m.in_layers[0], m.in_layers[1]
    c2, n2 = m.out_layers[0], m.out_layers[1]

    def groups(n):
        if "gn_groups" in mut and n.num_groups == 4:
            return n.num_channels // (n.num_channels // 8)
        return n.num_groups

    h = ar.conv(cat, c1.weight, None if "no_bias1" in mut else c1.bias, 1, c1.padding[0])
    h = F.silu(ar.norm(h, n1, groups(n1)))
    h = ar.conv(h, c2.weight, None if "no_bias2" in mut else c2.bias, 1, c2.padding[0])
    h = F.silu(ar.norm(h, n2, groups(n2)))
    sk = m.skip_connection
    skip = skip_in if isinstance(sk, torch.nn.Identity) else ar.conv(skip_in, sk.weight, sk.bias, 1, 0)
    return skip + h


def qkv_attention(qkv, heads: int, views: int, ar: Arith = F64, mut=frozenset()):
    """QKVAttentionLegacy: "(v b) n t -> b n (v t)" when views > 1, heads split before q / k / v,
    scale ch^-1/4 on q and on k, back to "(v b) n t"."""
    from einops import rearrange

    fold = views > 1 and "no_fold" not in mut
    layout = "(b v) n t" if "vb_as_bv" in mut else "(v b) n t"
    if fold:
        qkv = rearrange(qkv, f"{layout} -> b n (v t)", v=views)
    bs, width, length = qkv.shape
    ch = width // (3 * heads)
    q, k, v = qkv.reshape(bs * heads, ch * 3, length).split(ch, dim=1)
    scale = 1 / math.sqrt(math.sqrt(ch))
    a = ar.attend(q * scale, k * scale, v).reshape(bs, -1, length)
    return rearrange(a, f"b n (v t) -> {layout}", v=views) if fold else a


def attention_block(m, x, ar: Arith = F64, mut=frozenset()):
    """x + gn(proj_out(attention(qkv(x)))) over the flattened map."""
    x = ar.cast(x)
    b, c, *spatial = x.shape
    x = x.reshape(b, c, -1)
    att = m.attention
    views = att.n_frames if att.use_cross_view_self_attn else 1
    h = qkv_attention(ar.conv(x, m.qkv.weight, m.qkv.bias), m.num_heads, views, ar, mut)
    h = ar.conv(h, m.proj_out.weight, None if "no_proj_bias" in mut else m.proj_out.bias)
    return (x + ar.norm(h, m.norm)).reshape(b, c, *spatial)


def downsample(m, x, ar: Arith = F64, mut=frozenset()):
    """The stride-2 3x3 convolution, padding 1."""
    x = ar.cast(x)
    if "stride_offset" in mut:  # the taps centred on the odd pixels' upper-left neighbours
        x = F.pad(x, (1, 0, 1, 0))[..., :-1, :-1]
    return ar.conv(x, m.op.weight, m.op.bias, 2, 1)


def upsample(m, x, ar: Arith = F64, mut=frozenset()):
    """Nearest 2x upsample, then the 3x3 convolution."""
    x = ar.cast(x)
    if "zero_insert" in mut:
        up = x.new_zeros(x.shape[0], x.shape[1], 2 * x.shape[2], 2 * x.shape[3])
        up[..., ::2, ::2] = x
    else:
        up = F.interpolate(x, scale_factor=2, mode="nearest")
    return ar.conv(up, m.conv.weight, m.conv.bias, 1, 1)


def _step(mod, h, ar, mut):
    kind = type(mod).__name__
    if kind == "ResBlock":
        return res_block(mod, h, None, ar, mut)
    if kind == "AttentionBlock":
        return attention_block(mod, h, ar, mut)
    if kind == "Downsample":
        return downsample(mod, h, ar, mut)
    if kind == "Upsample":
        return upsample(mod, h, ar, mut)
    if kind == "Conv2d":
        return ar.conv(h, mod.weight, mod.bias, mod.stride[0], mod.padding[0])
    if kind == "Identity":
        return h
    raise TypeError(f"no restatement of {kind}")


def unet(m, x, ar: Arith = F64, mut=frozenset()):
    """UNetModel.forward: the input blocks, the middle block, the output blocks on
    cat([h, skip]), out = conv -> GroupNorm -> SiLU."""
    h = ar.cast(x)
    hs = []
    for block in m.input_blocks:
        for mod in block:
            h = _step(mod, h, ar, mut)
        hs.append(h)
    for mod in m.middle_block:
        h = _step(mod, h, ar, mut)
    for block in m.output_blocks:
        mods = list(block)
        h = res_block(mods[0], h, hs.pop(), ar, mut)
        for mod in mods[1:]:
            h = _step(mod, h, ar, mut)
    conv, norm = m.out[0], m.out[1]
    return F.silu(ar.norm(ar.conv(h, conv.weight, conv.bias, 1, conv.padding[0]), norm))
