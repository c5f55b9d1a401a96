"""Camera interpolation of the fly-through videos (reference
src/visualization/camera_trajectory/interpolation.py: interpolate_intrinsics :8-16,
interpolate_extrinsics :204-252).

The reference's interpolate_extrinsics goes through torch.linalg.lstsq, boolean-mask indexing and
scipy's Euler conversions on numpy: several host round trips per video. Device tensors here take
one launch (tsplat_trajectory_extrinsics, one thread per (pair, time step)); host tensors (CPU
tests, CPU baselines) take the same math on float64 torch ops. Both stay in float64 to the end and
round only the result to fp32; the reference rounds the interpolated parameters, the pivot frame
and the pivot point to fp32 before converting back, so it differs by a few fp32 roundings.
"""
from __future__ import annotations

import math

import torch
from torch import Tensor

from ... import kernels


def interpolate_intrinsics(initial: Tensor, final: Tensor, t: Tensor) -> Tensor:
    """initial, final [*batch, 3, 3], t [T] -> [*batch, T, 3, 3], linear."""
    initial = initial[..., None, :, :]
    final = final[..., None, :, :]
    return initial + (final - initial) * t[:, None, None]


def _cross(a: Tensor, b: Tensor) -> Tensor:
    return torch.linalg.cross(a, b, dim=-1)


def _dot(a: Tensor, b: Tensor) -> Tensor:
    return (a * b).sum(dim=-1)


def _frame(y: Tensor, z: Tensor) -> Tensor:
    """Columns (y x z, y, z): generate_coordinate_frame."""
    y, z = torch.broadcast_tensors(y, z)
    return torch.stack([_cross(y, z), y, z], dim=-1)


def _parallel(a: Tensor, b: Tensor, eps: float) -> Tensor:
    return (_dot(a, b).abs() - 1).abs() < eps


def _pivot_parameters(ext: Tensor, frame: Tensor, pivot: Tensor) -> Tensor:
    """extrinsics_to_pivot_parameters: 3 translations in the frame (axis x look, axis, look) and the
    first and third intrinsic YXZ Euler angle of frame^-1 R."""
    tf = _frame(frame[..., :, 1], ext[..., :3, 2])
    delta = pivot - ext[..., :3, 3]
    translation = (tf * delta[..., :, None]).sum(dim=-2)
    m = torch.linalg.inv(frame) @ ext[..., :3, :3]
    lock = torch.hypot(m[..., 0, 2], m[..., 2, 2]) < 1e-7  # gimbal lock: the third angle is zero
    first = torch.where(lock, torch.atan2(-m[..., 2, 0], m[..., 0, 0]), torch.atan2(m[..., 0, 2], m[..., 2, 2]))
    third = torch.where(lock, torch.zeros_like(first), torch.atan2(m[..., 1, 0], m[..., 1, 1]))
    return torch.cat([translation, first[..., None], third[..., None]], dim=-1)


def _lerp_circular(a: Tensor, b: Tensor, t: Tensor) -> Tensor:
    """interpolate_circular: from the nearest of a - 2 pi, a, a + 2 pi towards b."""
    tau = 2 * math.pi
    a, b = a % tau, b % tau
    d, d_left, d_right = (b - a).abs(), (b - (a - tau)).abs(), (b - (a + tau)).abs()
    use_d = (d < d_left) & (d < d_right)
    use_left = (d_left < d_right) & ~use_d
    a0 = torch.where(use_d, a, torch.where(use_left, a - tau, a + tau))
    return a0 + (b - a0) * t


def _interpolate_host(initial: Tensor, final: Tensor, t: Tensor, eps: float) -> Tensor:
    """[P, 4, 4] x 2, [T] -> [P, T, 4, 4] float64: the kernel's math on torch ops."""
    la, lb = initial[:, :3, 2], final[:, :3, 2]
    oa, ob = initial[:, :3, 3], final[:, :3, 3]
    par = _parallel(la, lb, eps)
    eye = torch.eye(3, dtype=torch.float64)
    na = la[:, :, None] * la[:, None, :] - eye
    nb = lb[:, :, None] * lb[:, None, :] - eye
    lhs = na + nb
    rhs = (na @ oa[:, :, None] + nb @ ob[:, :, None])[..., 0]
    lhs = torch.where(par[:, None, None], eye, lhs)  # unused rows stay solvable
    focus = (torch.linalg.inv(lhs) @ rhs[:, :, None])[..., 0]
    pivot = torch.where(par[:, None], 0.5 * (oa + ob), focus)

    b = lb.clone()
    b = torch.where(_parallel(la, b, eps)[:, None], torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64), b)
    b = torch.where(_parallel(la, b, eps)[:, None], torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), b)
    n = _cross(la, b)
    frame = _frame(n / n.norm(dim=-1, keepdim=True), la)

    pi = _pivot_parameters(initial, frame, pivot)[:, None]
    pf = _pivot_parameters(final, frame, pivot)[:, None]
    tt = t[None, :, None]
    trans = pi[..., :3] + (pf[..., :3] - pi[..., :3]) * tt
    ang = _lerp_circular(pi[..., 3:], pf[..., 3:], tt)

    ca, sa, cg, sg = ang[..., 0].cos(), ang[..., 0].sin(), ang[..., 1].cos(), ang[..., 1].sin()
    zero = torch.zeros_like(ca)
    euler = torch.stack([ca * cg, -ca * sg, sa, sg, cg, zero, -sa * cg, sa * sg, ca], dim=-1)
    rot = frame[:, None] @ euler.reshape(*euler.shape[:-1], 3, 3)
    tf = _frame(frame[:, None, :, 1], rot[..., :, 2])
    origin = pivot[:, None] - (tf @ trans[..., None])[..., 0]
    out = torch.zeros((*rot.shape[:2], 4, 4), dtype=torch.float64)
    out[..., :3, :3] = rot
    out[..., :3, 3] = origin
    out[..., 3, 3] = 1
    return out


@torch.no_grad()
def interpolate_extrinsics(initial: Tensor, final: Tensor, t: Tensor, eps: float = 1e-4) -> Tensor:
    """Interpolate camera-to-world poses by rotating about their focus point, the least-squares
    intersection of the two look rays (the origins' midpoint for parallel looks).
    initial, final [*batch, 4, 4], t [T] (outside [0, 1]: extrapolation) -> [*batch, T, 4, 4] fp32."""
    initial, final = torch.broadcast_tensors(initial, final)
    batch = initial.shape[:-2]
    a, b = initial.reshape(-1, 4, 4), final.reshape(-1, 4, 4)
    if a.is_cuda:
        out = kernels.trajectory_extrinsics(a, b, t, eps)
    else:
        out = _interpolate_host(a.double(), b.double(), t.double(), eps).float()
    return out.reshape(*batch, t.shape[0], 4, 4)
