"""PSNR and SSIM as the reference computes them (reference src/evaluation/metrics.py:11-19, :36-52)."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from .lpips_vgg import MIN_SIZE as LPIPS_MIN_SIZE, SCALE, SHIFT, VGG_BLOCKS

SSIM_WIN = 11  # skimage win_size; = 2 int(3.5 * 1.5 + 0.5) + 1, the taps of gaussian_filter(sigma=1.5, truncate=3.5)


@torch.no_grad()
def compute_psnr(ground_truth: torch.Tensor, predicted: torch.Tensor) -> torch.Tensor:
    """[batch, 3, H, W] pairs -> per-image PSNR: clip to [0, 1], per-image MSE, -10 log10."""
    ground_truth = ground_truth.clip(min=0, max=1)
    predicted = predicted.clip(min=0, max=1)
    mse = ((ground_truth - predicted) ** 2).flatten(1).mean(dim=-1)
    return -10 * mse.log10()


def _ssim_weights() -> torch.Tensor:
    """The 11 float64 taps of scipy.ndimage.gaussian_filter(sigma=1.5, truncate=3.5)."""
    w = torch.tensor([math.exp(-0.5 / (1.5 * 1.5) * i * i) for i in range(-5, 6)], dtype=torch.float64)
    return w / w.sum()


@torch.no_grad()
def compute_ssim(ground_truth: torch.Tensor, predicted: torch.Tensor) -> torch.Tensor:
    """[batch, 3, H, W] pairs -> per-image SSIM, the reference's configuration of skimage's
    structural_similarity(gt, hat, win_size=11, gaussian_weights=True, channel_axis=0,
    data_range=1.0): per channel the 11-tap Gaussian (sigma 1.5) of x, y, xx, yy, xy, sample
    covariances (121 / 120), C1 = 0.01^2, C2 = 0.03^2, the mean of the map without its 5-pixel border
    over pixels and channels. Inputs are not clipped (the reference clips for PSNR only); H or W below
    11 raises, as skimage does. The result has predicted's dtype and device.

    Device tensors go to the HIP kernel (kernels.ssim: float64 inside, one fp32 per image, no host
    round trip). CPU tensors take a plain torch float64 restatement (a separable conv2d with the same
    weights): like compute_psnr, which runs anywhere, it is metric code for the CPU plumbing tests,
    not a fallback of the product path."""
    if ground_truth.shape != predicted.shape:
        raise ValueError(f"compute_ssim: ground truth {tuple(ground_truth.shape)} != prediction "
                         f"{tuple(predicted.shape)}")
    if predicted.dim() != 4:
        raise ValueError(f"compute_ssim: expected [batch, channel, H, W], got {tuple(predicted.shape)}")
    b, c, h, w = predicted.shape
    if h < SSIM_WIN or w < SSIM_WIN:
        raise ValueError(f"compute_ssim: win_size {SSIM_WIN} exceeds the {h} x {w} image")
    if predicted.is_cuda:
        from .. import kernels

        return kernels.ssim(ground_truth, predicted).to(predicted.dtype)
    x = ground_truth.to(torch.float64).reshape(b * c, 1, h, w)
    y = predicted.to(torch.float64).reshape(b * c, 1, h, w)
    wt = _ssim_weights()

    def filt(t):  # valid region only: the crop drops every pixel the boundary mode would touch
        return F.conv2d(F.conv2d(t, wt.reshape(1, 1, -1, 1)), wt.reshape(1, 1, 1, -1))

    ux, uy, uxx, uyy, uxy = filt(x), filt(y), filt(x * x), filt(y * y), filt(x * y)
    cov_norm = SSIM_WIN * SSIM_WIN / (SSIM_WIN * SSIM_WIN - 1)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux ** 2 + uy ** 2 + c1) * (vx + vy + c2))
    return s.reshape(b, -1).mean(dim=-1).to(predicted.dtype)


@torch.no_grad()
def compute_lpips(ground_truth: torch.Tensor, predicted: torch.Tensor, net, return_layers: bool = False):
    """[batch, 3, H, W] pairs -> per-image LPIPS as the reference's compute_lpips calls it:
    LPIPS(net="vgg") (version 0.1, linear layers on), forward(ground_truth, predicted, normalize=True),
    inputs not clipped. x <- ((2 x - 1) - shift) / scale; VGG16's thirteen 3x3 convolutions + ReLU with
    2x2 max-pools (floor mode) between the five blocks; after each block, per pixel, both feature
    vectors divided by (their norm + 1e-10), the squared difference weighted by the tap's 1x1 weights,
    the spatial mean; the five means summed. H or W below 16 raises (the fifth block's map would be
    empty). `net` is an evaluation.lpips_vgg.LpipsVGG -- the one deviation from the reference's
    signature, which downloads the weights on first use. The result has predicted's dtype and device;
    with `return_layers` also the five taps' contributions [batch, 5].

    Device tensors go to the HIP kernels (kernels.lpips: exact-fp32 Winograd convolutions, float64
    from the features on). CPU tensors take a plain torch float64 restatement: like compute_ssim's, it
    is metric code for the CPU plumbing tests, not a fallback of the product path."""
    if ground_truth.shape != predicted.shape:
        raise ValueError(f"compute_lpips: ground truth {tuple(ground_truth.shape)} != prediction "
                         f"{tuple(predicted.shape)}")
    if predicted.dim() != 4 or predicted.shape[1] != 3:
        raise ValueError(f"compute_lpips: expected [batch, 3, H, W], got {tuple(predicted.shape)}")
    b, _, h, w = predicted.shape
    if h < LPIPS_MIN_SIZE or w < LPIPS_MIN_SIZE:
        raise ValueError(f"compute_lpips: a {h} x {w} image leaves the fifth VGG block an empty map")
    if predicted.is_cuda:
        from .. import kernels

        got = kernels.lpips(ground_truth, predicted, net, return_layers=return_layers)
        return tuple(t.to(predicted.dtype) for t in got) if return_layers else got.to(predicted.dtype)
    x = torch.cat([ground_truth, predicted]).to(torch.float64) * 2 - 1
    x = (x - torch.tensor(SHIFT, dtype=torch.float64).reshape(1, 3, 1, 1)) / torch.tensor(
        SCALE, dtype=torch.float64).reshape(1, 3, 1, 1)
    layers, conv = [], 0
    for k, count in enumerate(VGG_BLOCKS):
        if k:
            x = F.max_pool2d(x, 2)
        for _ in range(count):
            weight, bias = net.convs[conv]
            x = F.relu(F.conv2d(x, weight.double(), bias.double(), padding=1))
            conv += 1
        unit = x / (x.square().sum(dim=1, keepdim=True).sqrt() + 1e-10)
        diff = (unit[:b] - unit[b:]).square() * net.lins[k].double().reshape(1, -1, 1, 1)
        layers.append(diff.sum(dim=1).mean(dim=(1, 2)))
    layers = torch.stack(layers, dim=1)
    value = layers.sum(dim=1).to(predicted.dtype)
    return (value, layers.to(predicted.dtype)) if return_layers else value
