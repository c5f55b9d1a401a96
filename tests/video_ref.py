"""Float64 numpy restatements of the video path, for the tests: the trajectory between two poses
(own intrinsic-YXZ Euler code, no scipy), exact quantiles (sort + linear interpolation) and the
frames (quantiles, tone map, turbo lookup, layout, uint8). Written from the contracts in
include/transplat_hip.h / DESIGN.md, one pose and one pixel array at a time."""
from __future__ import annotations

import math
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
GAP = 8
TAU = 2.0 * math.pi


# ----------------------------------------------------------------------------------- trajectory
def _frame(y, z):
    return np.stack([np.cross(y, z), y, z], axis=1)  # columns


def _is_parallel(a, b, eps):
    return abs(abs(float(a @ b)) - 1.0) < eps


def euler_yxz(m):
    """(first, middle, third) angle of m = Ry(first) Rx(middle) Rz(third); in gimbal lock third = 0."""
    if math.hypot(m[0, 2], m[2, 2]) < 1e-7:
        return math.atan2(-m[2, 0], m[0, 0]), math.asin(max(-1.0, min(1.0, -m[1, 2]))), 0.0
    return (math.atan2(m[0, 2], m[2, 2]), math.asin(max(-1.0, min(1.0, -m[1, 2]))),
            math.atan2(m[1, 0], m[1, 1]))


def rot_y(a):
    return np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])


def rot_x(a):
    return np.array([[1, 0, 0], [0, math.cos(a), -math.sin(a)], [0, math.sin(a), math.cos(a)]])


def rot_z(a):
    return np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])


def pivot_of(a, b, eps=1e-4):
    """Pivot point and pivot frame of the pose pair a, b [4, 4] float64."""
    la, lb, oa, ob = a[:3, 2], b[:3, 2], a[:3, 3], b[:3, 3]
    if _is_parallel(la, lb, eps):
        pivot = 0.5 * (oa + ob)
    else:
        na, nb = np.outer(la, la) - np.eye(3), np.outer(lb, lb) - np.eye(3)
        pivot = np.linalg.solve(na + nb, na @ oa + nb @ ob)
    other = lb
    if _is_parallel(la, other, eps):
        other = np.array([0.0, 0.0, 1.0])
    if _is_parallel(la, other, eps):
        other = np.array([0.0, 1.0, 0.0])
    n = np.cross(la, other)
    return pivot, _frame(n / np.linalg.norm(n), la)


def _parameters(e, frame, pivot):
    tf = _frame(frame[:, 1], e[:3, 2])
    first, _, third = euler_yxz(np.linalg.inv(frame) @ e[:3, :3])
    return np.concatenate([tf.T @ (pivot - e[:3, 3]), [first, third]])


def _circular(a, b, t):
    a, b = a % TAU, b % TAU
    d, dl, dr = abs(b - a), abs(b - (a - TAU)), abs(b - (a + TAU))
    if d < dl and d < dr:
        a0 = a
    elif dl < dr:
        a0 = a - TAU
    else:
        a0 = a + TAU
    return a0 + (b - a0) * t


def interpolate_extrinsics(initial, final, t, eps=1e-4):
    """initial, final [P, 4, 4], t [T] -> [P, T, 4, 4] float64 (inputs taken as float64)."""
    initial, final, t = (np.asarray(x, dtype=np.float64) for x in (initial, final, t))
    out = np.zeros((initial.shape[0], t.shape[0], 4, 4))
    for p, (a, b) in enumerate(zip(initial, final)):
        pivot, frame = pivot_of(a, b, eps)
        pa, pb = _parameters(a, frame, pivot), _parameters(b, frame, pivot)
        for i, ti in enumerate(t):
            trans = pa[:3] + (pb[:3] - pa[:3]) * ti
            rot = frame @ rot_y(_circular(pa[3], pb[3], ti)) @ rot_z(_circular(pa[4], pb[4], ti))
            out[p, i, :3, :3] = rot
            out[p, i, :3, 3] = pivot - _frame(frame[:, 1], rot[:, 2]) @ trans
            out[p, i, 3, 3] = 1.0
    return out


def trajectory_scale(initial, final, eps=1e-4):
    """[P] max(1, |pivot| + |origin|) per pair (the larger origin): the size the fp32 roundings of the
    reference's second half act on."""
    initial, final = np.asarray(initial, dtype=np.float64), np.asarray(final, dtype=np.float64)
    out = []
    for a, b in zip(initial, final):
        pivot, _ = pivot_of(a, b, eps)
        origin = max(np.linalg.norm(a[:3, 3]), np.linalg.norm(b[:3, 3]))
        out.append(max(1.0, float(np.linalg.norm(pivot)) + float(origin)))
    return np.array(out)


# ------------------------------------------------------------------------------------- quantile
def quantile(x, q, positive_only=False):
    """numpy.quantile(pop, q) with linear interpolation, evaluated in double, as the kernel states it:
    pos = q (m - 1), k = floor(pos), lo + (hi - lo) (pos - k); NaN for an empty population."""
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    pop = np.sort(x[x > 0] if positive_only else x).astype(np.float64)
    m = pop.shape[0]
    if m == 0:
        return float("nan")
    pos = q * (m - 1)
    k = int(math.floor(pos))
    lo, hi = pop[k], pop[min(k + 1, m - 1)]
    return float(lo + (hi - lo) * (pos - k))


# --------------------------------------------------------------------------------------- frames
def turbo_table():
    """The 256 x 3 table of transplat_amd/csrc/turbo_lut.h, as fp32 (what the kernel reads)."""
    text = (ROOT / "transplat_amd" / "csrc" / "turbo_lut.h").read_text()
    rows = re.findall(r"\{([0-9.e-]+)f, ([0-9.e-]+)f, ([0-9.e-]+)f\}", text)
    assert len(rows) == 256
    return np.array(rows, dtype=np.float64).astype(np.float32)


def tone(x):
    """uint8(clip(x, 0, 1) * 255): fp32 multiply, truncation."""
    return (np.clip(np.asarray(x, dtype=np.float32), 0, 1) * np.float32(255)).astype(np.uint8)


def depth_ratio(depth, max_values=16_000_000):
    """r = 1 - (log(depth) - near) / (far - near) in float64, unclipped (inf / NaN as IEEE gives)."""
    depth = np.asarray(depth, dtype=np.float32)
    flat = depth.reshape(-1)[:max_values]
    with np.errstate(all="ignore"):
        near = np.log(np.float64(quantile(flat, 0.01, True)))
        far = np.log(np.float64(quantile(flat, 0.99, False)))
        return 1.0 - (np.log(depth.astype(np.float64)) - near) / (far - near)


def frames(color, depth=None):
    """color [T, 3, H, W] (+ depth [T, H, W]) -> (uint8 [T, H_out, W, 3], r or None)."""
    color = np.asarray(color, dtype=np.float32)
    t, _, h, w = color.shape
    top = tone(color).transpose(0, 2, 3, 1)
    if depth is None:
        return top, None
    r = depth_ratio(depth)
    lut = tone(turbo_table())
    with np.errstate(all="ignore"):
        entry = np.minimum((np.clip(r, 0, 1) * 256).astype(np.int64), 255)
    entry = np.where(np.isnan(r), 0, entry)
    mapped = np.where(np.isnan(r)[..., None], np.uint8(0), lut[entry])
    gap = np.full((t, GAP, w, 3), 255, dtype=np.uint8)
    return np.concatenate([top, gap, mapped.astype(np.uint8)], axis=1), r


def flagged(r, tol):
    """Depth pixels whose colour-map entry is a rounding decision: unclipped r in (0, 1) and r * 256
    within tol of an integer 1..255."""
    with np.errstate(all="ignore"):
        s = r * 256
        near_int = np.abs(s - np.round(s)) <= tol
        return (r > 0) & (r < 1) & near_int & (np.round(s) >= 1) & (np.round(s) <= 255)
