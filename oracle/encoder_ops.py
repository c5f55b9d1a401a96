"""TEST INFRASTRUCTURE ONLY — CPU restatements of the encoder hot-path ops (torch fp32, CPU).

Each function has the exact signature of its gfx950 counterpart in transplat_amd/kernels.py so a
test can run the surrounding module code on the CPU with these in place (monkeypatched), and the
GPU tests compare the HIP ops with these on identical inputs. Pinned by tests/golden/*.npz
(generated from the reference modules, see tests/golden/gen_golden.py). The correlation ops
(calculate_grid, uv_coarse, uv_cross, msda) also run in float64 on the widened fp32 inputs
(dtype=torch.float64), the reference of tests/test_corr_shapes.py.
"""
from __future__ import annotations

import math

import torch


# --------------------------------------------------------------------- window attention (T2, T3)
def _window_pixel_index(h: int, w: int, splits: int, shift_h: int, shift_w: int) -> torch.Tensor:
    """[K*K, L] original pixel of every (window, in-window position) after the roll.

    Restates split_feature (reference unimatch/utils.py:34-59: windows ordered (row-split,
    col-split), positions row-major) applied to torch.roll(x, (-shift_h, -shift_w)) (reference
    multiview_transformer.py:91-98): rolled[y, x] = x_orig[(y + shift_h) % h, (x + shift_w) % w].
    """
    wh, ww = h // splits, w // splits
    idx = []
    for sy in range(splits):
        for sx in range(splits):
            yy = (torch.arange(wh) + sy * wh + shift_h) % h
            xx = (torch.arange(ww) + sx * ww + shift_w) % w
            idx.append((yy[:, None] * w + xx[None, :]).reshape(-1))
    return torch.stack(idx)


def _region_ids(h: int, w: int, splits: int) -> torch.Tensor:
    """[K*K, L] Swin region id of each in-window position (generate_shift_window_attn_mask,
    reference multiview_transformer.py:17-54): slices (0:-wsize), (-wsize:-shift), (-shift:)."""
    wh, ww = h // splits, w // splits
    sh, sw = wh // 2, ww // 2

    def band(coord, size, win, sft):
        return torch.where(coord < size - win, 0, torch.where(coord < size - sft, 1, 2))

    ids = []
    for sy in range(splits):
        for sx in range(splits):
            yy = torch.arange(wh) + sy * wh
            xx = torch.arange(ww) + sx * ww
            r = band(yy, h, wh, sh)[:, None] * 3 + band(xx, w, ww, sw)[None, :]
            ids.append(r.reshape(-1))
    return torch.stack(ids)


def window_attention(q, k, v, h: int, w: int, num_splits: int, with_shift: bool, kv_shift: int = 0):
    """softmax(Q K^T / sqrt(C) + mask) V over split windows (reference
    single_head_split_window_attention, multiview_transformer.py:57-206); kv_shift pairs query batch
    i with key batch (i + kv_shift) % B (batch_features' view swap, :495-515).

    q [B, L, C]; k, v [B, L, C] (two views) or [B, m, L, C] (m = V - 1 key views).
    Multi-view keys are ordered pixel-major / view-minor within a window and the shift mask is
    tiled view-major (`attn_mask.repeat(b, 1, m)`, :130), so key j takes mask column j mod L.
    """
    if kv_shift:
        k, v = torch.roll(k, -kv_shift, dims=0), torch.roll(v, -kv_shift, dims=0)
    q = q.float()
    b, _, c = q.shape
    if k.dim() == 3:
        k = k[:, None]
        v = v[:, None]
    m = k.shape[1]
    wh, ww = h // num_splits, w // num_splits
    # shift_size_h / _w = window // 2 per axis (reference :93-94)
    pix = _window_pixel_index(h, w, num_splits, wh // 2 if with_shift else 0, ww // 2 if with_shift else 0)
    k2, L = pix.shape
    out = torch.empty_like(q)
    if with_shift:
        reg = _region_ids(h, w, num_splits)  # [K2, L]
        kcol = torch.arange(L * m) % L
    for bi in range(b):
        for wi in range(k2):
            qi = q[bi, pix[wi]]  # [L, C]
            # keys: pixel-major, view-minor
            kw = k[bi][:, pix[wi]].permute(1, 0, 2).reshape(L * m, c).float()
            vw = v[bi][:, pix[wi]].permute(1, 0, 2).reshape(L * m, c).float()
            s = qi @ kw.T / math.sqrt(c)
            if with_shift:
                r = reg[wi]
                s = s + torch.where(r[:, None] == r[kcol][None, :], 0.0, -100.0)
            out[bi, pix[wi]] = torch.softmax(s, dim=-1) @ vw
    return out


# --------------------------------------------------------------------- correlation (C2-C9)
def calculate_grid(intr, pose, disp, h: int, w: int, dtype=None):
    """Projection grid (reference depth_predictor_trans.py:11-57): pixel (x, y) at depth 1/disp
    of camera n lands at uv in the other camera; normalised 2u/(W-1) - 1. -> [N, D, HW, 2].
    dtype (torch.float64): the inputs are widened before the first operation (the inverse of the
    intrinsics included) and everything runs in that type; None is the fp32 form."""
    n, d = disp.shape
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    pts = torch.stack([xs, ys, torch.ones_like(xs)], 0).float().reshape(3, -1)  # [3, HW]
    if dtype is not None:
        intr, pose, disp, pts = intr.to(dtype), pose.to(dtype), disp.to(dtype), pts.to(dtype)
    depth = 1.0 / disp  # [N, D]
    cam = torch.inverse(intr) @ pts  # [N, 3, HW]
    rot = pose[:, :3, :3] @ cam  # [N, 3, HW]
    p = rot[:, :, None, :] * depth[:, None, :, None] + pose[:, :3, 3][:, :, None, None]
    p = (intr @ p.reshape(n, 3, -1)).reshape(n, 3, d, h * w)
    uv = p[:, :2] / p[:, 2:].clamp(min=1e-3)
    gx = 2 * uv[:, 0] / (w - 1) - 1
    gy = 2 * uv[:, 1] / (h - 1) - 1
    return torch.stack([gx, gy], -1)


def bilinear_zero(img, x, y):
    """Sample img [HW... as H, W, C] at pixel coords (x, y) with zero padding (mmcv MSDA /
    grid_sample(align_corners=False) after loc * size - 0.5). x, y: [...] -> [..., C].

    Runs as F.grid_sample (bilinear, zeros, align_corners=False) -- the operator the reference's own
    CPU path calls for these samplings (mmcv's pytorch MSDA fallback and UVCoarseAttention) -- on
    grid = (pixel + 0.5) / size * 2 - 1; `bilinear_zero_corners` is the explicit four-corner form
    it is checked against (tests/test_encoder_ops.py)."""
    import torch.nn.functional as F

    hh, ww, c = img.shape
    grid = torch.stack(((x + 0.5) * (2.0 / ww) - 1.0, (y + 0.5) * (2.0 / hh) - 1.0), -1).reshape(1, -1, 1, 2)
    out = F.grid_sample(img.permute(2, 0, 1).unsqueeze(0), grid.to(img.dtype), mode="bilinear",
                        padding_mode="zeros", align_corners=False)  # [1, C, N, 1]
    return out[0, :, :, 0].t().reshape(*x.shape, c)


def bilinear_zero_corners(img, x, y):
    """bilinear_zero written out: the four corners' weights and zero padding per sample."""
    hh, ww, c = img.shape
    x0 = torch.floor(x)
    y0 = torch.floor(y)
    out = torch.zeros((*x.shape, c), dtype=img.dtype)
    for dy in (0, 1):
        for dx in (0, 1):
            xi = x0 + dx
            yi = y0 + dy
            wgt = (1 - (x - xi).abs()) * (1 - (y - yi).abs())
            ok = (xi >= 0) & (xi <= ww - 1) & (yi >= 0) & (yi <= hh - 1)
            xc = xi.clamp(0, ww - 1).long()
            yc = yi.clamp(0, hh - 1).long()
            val = img[yc, xc]
            out = out + torch.where(ok[..., None], wgt[..., None] * val, torch.zeros((), dtype=img.dtype))
    return out


def _sampler(dtype):
    """The bilinear sampler of a correlation op: grid_sample in the fp32 form, the explicit corners
    in a widened one."""
    return bilinear_zero if dtype is None else bilinear_zero_corners


def _ref3d(intr, pose, disp, h, w, b, dtype=None):
    """ref_3d of UVTransformerEncoder (reference utils/encoder.py:57-59) in (b v) order,
    normalised to [0, 1] as grid / 2 + 0.5 -> [B*2, HW, D, 2]."""
    grid = calculate_grid(intr, pose, disp, h, w, dtype)  # [(v b), D, HW, 2]
    d = disp.shape[1]
    r = grid.reshape(2, b, d, h * w, 2).permute(1, 0, 3, 2, 4).reshape(b * 2, h * w, d, 2)
    return r / 2 + 0.5


def uv_coarse(feat, intr, pose, disp, h: int, w: int, dtype=None):
    """UVCoarseAttention core (reference attention.py:468-551 with calculate_grid): for query
    (b, v) pixel p and depth d, sample the OTHER view's feature at ref_3d and dot with the own
    feature, / sqrt(C).  feat [B, 2, HW, C] -> [B*2, HW, D].
    dtype=torch.float64: the same operation on the widened fp32 inputs, sampled with the explicit
    four corners (no grid_sample), returned in float64; None is the fp32 form."""
    b, _, hw, c = feat.shape
    if dtype is not None:
        feat = feat.to(dtype)
    ref = _ref3d(intr, pose, disp, h, w, b, dtype)
    d = disp.shape[1]
    out = torch.empty((b * 2, hw, d), dtype=dtype or torch.float32)
    sample = _sampler(dtype)
    for bi in range(b):
        for vi in range(2):
            other = feat[bi, 1 - vi].reshape(h, w, c)
            r = ref[bi * 2 + vi]
            for q0 in range(0, hw, 512):
                sl = slice(q0, q0 + 512)
                s = sample(other, r[sl, :, 0] * w - 0.5, r[sl, :, 1] * h - 0.5)  # [q, D, C]
                out[bi * 2 + vi, sl] = (s * feat[bi, vi][sl, None, :]).sum(-1) / math.sqrt(c)
    return out


def uv_cross(value, key, intr, pose, disp, offsets, logits, h: int, w: int, dtype=None):
    """UVCrossAttention core (reference attention.py:329-416): per (query, depth) 4 points at
    ref_3d + offset / (W, H), softmax weights over the points, sampled from the OTHER view's
    value_proj output, then mean over channels of (sample * own key).
    value, key [B, 2, HW, C]; offsets [B*2, HW, D*P*2]; logits [B*2, HW, D*P] -> [B*2, HW, D].
    dtype=torch.float64: the same operation on the widened fp32 inputs (softmax included), sampled
    with the explicit four corners, returned in float64; None is the fp32 form."""
    b, _, hw, c = value.shape
    d = disp.shape[1]
    p = logits.shape[-1] // d
    if dtype is not None:
        value, key, offsets, logits = value.to(dtype), key.to(dtype), offsets.to(dtype), logits.to(dtype)
    ref = _ref3d(intr, pose, disp, h, w, b, dtype)
    off = offsets.reshape(b * 2, hw, d, p, 2)
    wts = torch.softmax(logits.reshape(b * 2, hw, d, p), -1)
    out = torch.empty((b * 2, hw, d), dtype=dtype or torch.float32)
    sample = _sampler(dtype)
    # [chunk, D, P, C] samples at a time: 256 queries in fp32; the corner form holds a few such
    # arrays at once, so its chunk keeps each near 64 MB
    chunk = 256 if dtype is None else max(1, 65536 // (d * p))
    for bi in range(b):
        for vi in range(2):
            n = bi * 2 + vi
            other = value[bi, 1 - vi].reshape(h, w, c)
            for q0 in range(0, hw, chunk):
                sl = slice(q0, q0 + chunk)
                loc = ref[n][sl, :, None, :] + off[n][sl] / torch.tensor([w, h], dtype=dtype or torch.float32)
                s = sample(other, loc[..., 0] * w - 0.5, loc[..., 1] * h - 0.5)  # [q, D, P, C]
                s = (s * wts[n][sl][..., None]).sum(2)
                out[n, sl] = (s * key[bi, vi][sl, None, :]).mean(-1)
    return out


def msda(value, loc, weights, h: int, w: int, dtype=None):
    """Single-level single-head MSDA (mmcv ms_deform_attn_forward semantics): value [N, HW, C],
    loc [N, Q, P, 2] in [0, 1], weights [N, Q, P] -> [N, Q, C].
    dtype=torch.float64: on the widened inputs with the explicit four corners; None: fp32."""
    n, hw, c = value.shape
    if dtype is not None:
        value, loc, weights = value.to(dtype), loc.to(dtype), weights.to(dtype)
    sample = _sampler(dtype)
    out = []
    for i in range(n):
        img = value[i].reshape(h, w, c)
        s = sample(img, loc[i, ..., 0] * w - 0.5, loc[i, ..., 1] * h - 0.5)  # [Q, P, C]
        out.append((s * weights[i][..., None]).sum(1))
    return torch.stack(out)


def msda_raw(value, ow, points: int, h: int, w: int):
    """kernels.msda_raw restated with the reference's operations (attention.py:232-262: offsets /
    (W, H) + the pixel-centre reference points, softmax over the points) and msda above."""
    n, hw, _ = value.shape
    off = ow[..., :2 * points].reshape(n, hw, points, 2)
    logits = ow[..., 2 * points:3 * points]
    ref_y, ref_x = torch.meshgrid(torch.linspace(0.5, h - 0.5, h, dtype=value.dtype),
                                  torch.linspace(0.5, w - 0.5, w, dtype=value.dtype), indexing="ij")
    ref = torch.stack((ref_x.reshape(-1) / w, ref_y.reshape(-1) / h), -1)[None].to(value.device)
    loc = ref[:, :, None, :] + off / torch.tensor([w, h], dtype=value.dtype, device=value.device)
    return msda(value, loc, logits.softmax(-1), h, w)


def depth_tail(fullres, head, near, far):
    """kernels.depth_tail restated with the reference's operations (depth_predictor_trans.py:480-491)."""
    from einops import rearrange

    b, v = near.shape
    delta, raw = head.split(1, dim=1)
    fine = (fullres + delta).clamp(1.0 / rearrange(far, "b v -> (v b) () () ()"),
                                   1.0 / rearrange(near, "b v -> (v b) () () ()"))
    depth = rearrange(1.0 / fine, "(v b) () h w -> b v (h w)", b=b, v=v)
    dens = rearrange(torch.sigmoid(raw), "(v b) () h w -> b v (h w)", b=b, v=v)
    return depth.contiguous(), dens.contiguous()


def resize_bilinear_nchw(x, size):
    """F.interpolate(x, size, mode="bilinear", align_corners=True) on NCHW maps (the PyTorch calls
    at the reference's encoder_trans.py / depth_predictor_trans.py resizes), on the CPU."""
    import torch.nn.functional as F

    return F.interpolate(x.float(), size=tuple(size), mode="bilinear", align_corners=True)


def ms_deform_attn(value, spatial_shapes, level_start_index, sampling_locations, attention_weights):
    """mmcv ms_deform_attn_forward, multi-level multi-head (the contract of the reference's
    MultiScaleDeformableAttnFunction_fp32, src/model/utils/multi_scale_deformable_attn_function.py:87-121;
    mmcv itself is absent here, its published im2col bilinear is restated): value
    [bs, keys, heads, hd] with level l's h x w map at keys [start_l, start_l + h w),
    sampling_locations [bs, nq, heads, L, P, 2] (x, y in [0, 1]), attention_weights
    [bs, nq, heads, L, P] -> [bs, nq, heads * hd]; bilinear at (x w - 1/2, y h - 1/2), zero padding."""
    bs, _, nh, hd = value.shape
    _, nq, _, nl, _, _ = sampling_locations.shape
    out = torch.zeros((bs, nq, nh, hd), dtype=torch.float32)
    for lvl in range(nl):
        h, w = int(spatial_shapes[lvl, 0]), int(spatial_shapes[lvl, 1])
        s = int(level_start_index[lvl])
        for b in range(bs):
            for m in range(nh):
                img = value[b, s:s + h * w, m].reshape(h, w, hd).float()
                loc = sampling_locations[b, :, m, lvl].float()  # [nq, P, 2]
                smp = bilinear_zero(img, loc[..., 0] * w - 0.5, loc[..., 1] * h - 0.5)  # [nq, P, hd]
                out[b, :, m] += (smp * attention_weights[b, :, m, lvl].float()[..., None]).sum(1)
    return out.reshape(bs, nq, nh * hd)


# --------------------------------------------------------------------- Gaussian adapter (A1-A4)
def gaussian_adapter(raw, depths, densities, extrinsics, intrinsics, image_shape, scale_min: float,
                     scale_max: float, opacity_exponent: float = 1.0, gaussians_per_pixel: int = 1,
                     camera_consts=None):
    """Encoder stage 5 (reference encoder_trans.py:294-353) + GaussianAdapter.forward
    (reference gaussian_adapter.py:48-96), restated with the reference's torch expressions.
    The SH rotation uses the e3nn construction restated in transplat_amd.misc.sh_rotation.
    camera_consts (the kernel path's precomputed per-camera inputs) is ignored: the restatement
    derives everything from the cameras itself."""
    from transplat_amd.misc.sh_rotation import rotate_sh

    b, v, hw, r = raw.shape
    h, w = image_shape
    d_sh = (r - 9) // 3
    ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    xy_ray = torch.stack([(xs + 0.5) / w, (ys + 0.5) / h], -1).reshape(hw, 2).float()
    pixel_size = 1 / torch.tensor((w, h), dtype=torch.float32)
    xy_ray = xy_ray + (raw[..., :2].sigmoid() - 0.5) * pixel_size  # [b, v, hw, 2]
    scales = scale_min + (scale_max - scale_min) * raw[..., 2:5].sigmoid()
    k = intrinsics[:, :, None]  # [b, v, 1, 3, 3]
    mult = 0.1 * (torch.inverse(k[..., :2, :2]) @ pixel_size[:, None])[..., 0].sum(-1)
    scales = scales * depths[..., None] * mult[..., None]
    rot = raw[..., 5:9]
    rot = rot / (rot.norm(dim=-1, keepdim=True) + 1e-8)
    i, j, kk, rr = rot.unbind(-1)
    two_s = 2 / ((rot * rot).sum(-1) + 1e-8)
    q = torch.stack((1 - two_s * (j * j + kk * kk), two_s * (i * j - kk * rr), two_s * (i * kk + j * rr),
                     two_s * (i * j + kk * rr), 1 - two_s * (i * i + kk * kk), two_s * (j * kk - i * rr),
                     two_s * (i * kk - j * rr), two_s * (j * kk + i * rr), 1 - two_s * (i * i + j * j)), -1)
    q = q.reshape(*q.shape[:-1], 3, 3)
    s = scales.diag_embed()
    cov = q @ s @ s.transpose(-1, -2) @ q.transpose(-1, -2)
    c2w = extrinsics[:, :, None, :3, :3]
    cov = c2w @ cov @ c2w.transpose(-1, -2)
    dirs = torch.cat([xy_ray, torch.ones_like(xy_ray[..., :1])], -1)
    dirs = (torch.inverse(k) @ dirs[..., None])[..., 0]
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    dirs = (c2w @ dirs[..., None])[..., 0]
    means = extrinsics[:, :, None, :3, 3] + dirs * depths[..., None]
    mask = torch.ones(d_sh)
    deg = int(round(d_sh**0.5)) - 1
    for l in range(1, deg + 1):
        mask[l * l:(l + 1) ** 2] = 0.1 * 0.25**l
    sh = raw[..., 9:].reshape(b, v, hw, 3, d_sh) * mask
    harm = rotate_sh(sh, extrinsics[:, :, None, None, :3, :3])
    e = float(opacity_exponent)
    opac = 0.5 * (1 - (1 - densities) ** e + densities ** (1 / e)) / gaussians_per_pixel
    flat = lambda t: t.reshape(b, v * hw, *t.shape[3:])
    return flat(means), flat(cov), flat(harm), flat(opac)


def group_norm(x, num_groups: int, weight, bias, eps: float, act: str = "none", residual=None, pre_bias=None):
    """torch.nn.GroupNorm followed by the module chain's activation and residual add (reference
    ldm_unet/unet.py:177-300 ResBlock: skip + SiLU(GN(conv)); :306-370 AttentionBlock:
    x + GN(proj); depth_predictor_trans.py:142-206: GN -> GELU). A residual pair (r1, r2) is the
    channel concatenation torch.cat([r1, r2], 1) (the output blocks' identity skip)."""
    if isinstance(residual, (tuple, list)):
        residual = torch.cat([residual[0], residual[1]], dim=1)
    x = x.float()
    if pre_bias is not None:  # the producing convolution's bias (reference: conv2d with bias)
        x = x + pre_bias.float().view(1, -1, *([1] * (x.dim() - 2)))
    y = torch.nn.functional.group_norm(x, num_groups, weight, bias, eps)
    if act == "silu":
        y = torch.nn.functional.silu(y)
    elif act == "gelu":
        y = torch.nn.functional.gelu(y)
    elif act == "relu":
        y = torch.relu(y)
    if residual is not None:
        y = residual.float() + y
        if act == "relu":  # UniMatch ResidualBlock: relu(x + relu(norm(conv(y))))
            y = torch.relu(y)
    return y


def conv_bias_act(conv, x, act: str = "none", residual=None, site: str = "", extra=()):
    """conv(cat([x, *extra], 1)) -> (GELU | ReLU) [-> + residual (-> ReLU)] as the reference module
    chains compute it (the reference materialises the concatenation with torch.cat)."""
    y = conv(torch.cat([x, *extra], dim=1) if extra else x)
    if act == "gelu":
        y = torch.nn.functional.gelu(y)
    elif act == "relu":
        y = torch.relu(y)
    if residual is not None:
        y = y + residual
        if act == "relu":
            y = torch.relu(y)
    return y


def conv2d_direct(x1, weight, bias=None, stride: int = 1, x2=None, upsample: bool = False):
    """nn.Conv2d(padding = k // 2) of cat([x1, x2], 1), nearest-upsampled 2x first if upsample:
    the reference ldm_unet chains ResBlock(cat([h, skip])) (unet.py:1096-1100), Upsample
    (unet.py:128-137: F.interpolate(nearest) -> conv), Downsample (unet.py:160-170)."""
    x = x1 if x2 is None else torch.cat([x1, x2], dim=1)
    if weight.dim() == 3:
        weight = weight.unsqueeze(-1)
    if upsample:
        x = torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest")
    return torch.nn.functional.conv2d(x, weight, bias, stride, weight.shape[-1] // 2)


def conv2d_nhwc_ok(x, weight) -> bool:
    """Every stride-1 conv the channels-last kernel takes (CPU model runs exercise its sites)."""
    return x.dim() == 4 and weight.shape[-1] in (1, 3) and x.shape[1] % 2 == 0 and x.shape[1] > 1


def conv2d_nhwc(x, weight, bias=None, residual=None, relu_in: bool = False):
    """DPT ResidualConvUnit step (reference util/blocks.py:73-99): conv(relu(x)) + bias (+ residual)."""
    y = torch.nn.functional.conv2d(torch.relu(x) if relu_in else x, weight, bias, 1, weight.shape[-1] // 2)
    return y if residual is None else y + residual


def upsample_bilinear_act(x, scale: int, bias=None, act: str = "none"):
    """depth predictor upsampler tail (reference depth_predictor_trans.py): conv bias -> bilinear
    upsample (align_corners=True) -> activation, in the reference's order."""
    if bias is not None:
        x = x + bias.reshape(1, -1, 1, 1)
    y = torch.nn.functional.interpolate(x, scale_factor=scale, mode="bilinear", align_corners=True)
    return {"none": y, "gelu": torch.nn.functional.gelu(y), "relu": torch.relu(y)}[act]


def qkv_attention_cf(qkv, heads: int, views: int = 1):
    """reference ldm_unet/unet.py QKVAttentionLegacy.forward (:510-552), with
    use_cross_view_self_attn when views > 1: "(v b) n t -> b n (v t)", heads split before q/k/v,
    softmax((q s)^T (k s)) v with s = ch^(-1/4), back to "(v b) n t"."""
    from einops import rearrange

    if views > 1:
        qkv = rearrange(qkv, "(v b) n t -> b n (v t)", v=views)
    bs, width, length = qkv.shape
    ch = width // (3 * heads)
    q, k, v = qkv.reshape(bs * heads, ch * 3, length).split(ch, dim=1)
    scale = 1 / math.sqrt(math.sqrt(ch))
    weight = torch.softmax(torch.einsum("bct,bcs->bts", q * scale, k * scale).float(), dim=-1)
    a = torch.einsum("bts,bcs->bct", weight, v).reshape(bs, -1, length)
    return rearrange(a, "b n (v t) -> (v b) n t", v=views) if views > 1 else a


def conv_nhwc_epilogue(conv, x, act: str = "none", res1=None, res2=None):
    """DPT unit chains (reference util/blocks.py): act(conv(x)) (+ res1) (+ res2)."""
    y = conv(x)
    y = {"none": y, "relu": torch.relu(y), "gelu": torch.nn.functional.gelu(y)}[act]
    if res1 is not None:
        y = y + res1
    if res2 is not None:
        y = y + res2
    return y


def resize_bilinear_nhwc(x, size):
    """reference DPT interpolations: F.interpolate(bilinear, align_corners=True)."""
    return torch.nn.functional.interpolate(x, size=tuple(int(v) for v in size), mode="bilinear", align_corners=True)


def mha(qkv, heads: int, scale: float):
    """DINOv2 Attention core (reference dinov2_layers/attention.py): reshape to heads, softmax
    attention (torch SDPA math), back to [B, N, heads * head_dim]."""
    b, n, c3 = qkv.shape
    d = c3 // (3 * heads)
    q, k, v = qkv.reshape(b, n, 3, heads, d).permute(2, 0, 3, 1, 4)
    x = torch.nn.functional.scaled_dot_product_attention(q, k, v, scale=scale)
    return x.transpose(1, 2).reshape(b, n, heads * d)


def depth_softmax(logits, disp):
    """reference depth_predictor_trans.py:170-180: pdf = softmax over depths, coarse disparity =
    sum(disp * pdf), pdf_max = max(pdf)."""
    pdf = torch.nn.functional.softmax(logits, dim=1)
    n, d = logits.shape[:2]
    coarse = (disp.reshape(n, d, 1, 1) * pdf).sum(dim=1, keepdim=True)
    return coarse, torch.max(pdf, dim=1, keepdim=True)[0]


def residual_ln(x, y, ls, norm, bf16_out: bool = False):
    """DINOv2 pre-norm residual step: x' = x + ls * y (LayerScale), LayerNorm(x') with the next norm
    (rounded to bf16 when `bf16_out`, as the kernel's bf16 output)."""
    if y is not None:
        x = x + (ls * y.float() if ls is not None else y.float())
    h = torch.nn.functional.layer_norm(x, (x.shape[-1],), norm.weight, norm.bias, norm.eps)
    return x, h.to(torch.bfloat16) if bf16_out else h


def instance_norm(x, eps: float, act: str = "none", residual=None):
    """nn.InstanceNorm2d (affine=False) [-> ReLU] [-> relu(residual + .)] (reference
    src/model/encoder/backbone/unimatch/backbone.py ResidualBlock / CNNEncoder)."""
    return group_norm(x, x.shape[1], None, None, eps, act, residual)


def sh_rotation(rotations, d_sh: int):
    """Per-camera block-diagonal real-SH rotation (the e3nn construction restated in
    transplat_amd.misc.sh_rotation, float64 matrix exponentials)."""
    from transplat_amd.misc.sh_rotation import sh_rotation_matrix

    return sh_rotation_matrix(rotations.reshape(-1, 3, 3).double(), d_sh).float()


# kernels.<name> -> oracle.<name>: what a CPU run of the module glue swaps in (tests, bench cpu leg)
def fused_linear(x1, weight, x2=None, bias=None, gelu: bool = False, ln=None, residual=None, split: bool = False,
                 gelu_in: bool = False, relu_in: bool = False, res_pre_ln: bool = False, out_dtype=torch.float32):
    """CPU restatement of kernels.fused_linear: the reference TransformerLayer's chain
    (multiview_transformer.py:327-407) torch.cat -> nn.Linear -> nn.GELU -> nn.LayerNorm -> + x, and
    the UV encoder layers' post-norm form LN(Linear(x) + identity) (utils/encoder.py:131-209); a bf16
    x1 is widened, out_dtype rounds the result (the bf16 attention's operands under autocast)."""
    x1 = x1.float()
    x = torch.cat([x1, x2], dim=-1) if x2 is not None else x1
    if gelu_in:
        x = torch.nn.functional.gelu(x)
    if relu_in:
        x = torch.relu(x)
    y = torch.nn.functional.linear(x, weight, bias)
    if gelu:
        y = torch.nn.functional.gelu(y)
    if residual is not None and res_pre_ln:
        y = y + residual
    if ln is not None:
        y = torch.nn.functional.layer_norm(y, (y.shape[-1],), ln[0], ln[1], ln[2])
    if residual is not None and not res_pre_ln:
        y = residual + y
    y = y.to(out_dtype)
    if split:
        return [t.contiguous() for t in y.split(128, dim=-1)]
    return y


def attention_merge(q, k, v, h: int, w: int, num_splits: int, with_shift: bool, merge_weight, ln, residual=None,
                    kv_shift: int = 0):
    """CPU restatement of kernels.attention_merge: window attention, merge Linear, LayerNorm,
    optional residual (reference multiview_transformer.py:327-407); kv_shift pairs query batch i
    with key batch (i + kv_shift) % B (batch_features' view swap, :495-515)."""
    if kv_shift:
        k, v = torch.roll(k, -kv_shift, dims=0), torch.roll(v, -kv_shift, dims=0)
    msg = window_attention(q, k, v, h, w, num_splits, with_shift)
    return fused_linear(msg, merge_weight, ln=ln, residual=residual)


KERNEL_RESTATEMENTS = ("window_attention", "uv_coarse", "uv_cross", "msda", "msda_raw", "ms_deform_attn", "gaussian_adapter", "group_norm",
                       "sh_rotation", "fused_linear", "attention_merge", "instance_norm",
                       "conv_bias_act", "mha", "residual_ln", "depth_softmax", "depth_tail", "conv2d_nhwc_ok",
                       "conv2d_nhwc", "upsample_bilinear_act", "qkv_attention_cf",
                       "conv_nhwc_epilogue", "resize_bilinear_nhwc")
