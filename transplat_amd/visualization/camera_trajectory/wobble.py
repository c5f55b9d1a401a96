"""Wobble trajectories (reference src/visualization/camera_trajectory/wobble.py:7-32): the camera
circles in its own image plane. A handful of torch ops on the inputs' device, no host sync."""
from __future__ import annotations

import math

import torch
from torch import Tensor


@torch.no_grad()
def generate_wobble_transformation(radius: Tensor, t: Tensor, num_rotations: int = 1,
                                   scale_radius_with_t: bool = True) -> Tensor:
    """radius [*batch], t [T] -> [*batch, T, 4, 4] fp32: the identity whose translation is
    r (sin a, -cos a, 0) with a = 2 pi num_rotations t and r = radius t (or radius)."""
    steps = t.shape[0]
    angle = (2 * math.pi * num_rotations) * t
    r = radius.unsqueeze(-1) * t if scale_radius_with_t else radius.unsqueeze(-1).expand(*radius.shape, steps)
    out = torch.zeros((*radius.shape, steps, 4, 4), dtype=torch.float32, device=t.device)
    out.diagonal(dim1=-2, dim2=-1).fill_(1.0)
    out[..., 0, 3] = angle.sin() * r
    out[..., 1, 3] = -angle.cos() * r
    return out


@torch.no_grad()
def generate_wobble(extrinsics: Tensor, radius: Tensor, t: Tensor) -> Tensor:
    """extrinsics [*batch, 4, 4], radius [*batch], t [T] -> [*batch, T, 4, 4]: each pose times the
    wobble transformation of its step."""
    return extrinsics.unsqueeze(-3) @ generate_wobble_transformation(radius, t)
