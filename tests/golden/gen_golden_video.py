#!/usr/bin/env python3
"""Generate tests/golden/video.npz by running the REFERENCE's trajectory and layout modules.

Usage: python tests/golden/gen_golden_video.py --ref <reference checkout>

Trajectory goldens come from the reference's real interpolate_extrinsics, interpolate_intrinsics
and generate_wobble (src/visualization/camera_trajectory/). Frame goldens come from a float32 torch
restatement of the depth_map closure (src/model/model_wrapper.py:736-741: it is a closure, and
apply_color_map's cm.get_cmap no longer exists in current matplotlib, so neither can be imported;
the table is matplotlib.colormaps["turbo"]) followed by the reference's real vcat
(src/visualization/layout.py) and the uint8 conversion of model_wrapper.py:771. Only harness code
lives here (gen_golden.py's annotation stubs, namespace-package registration); no reference source
is written into the repo, only the inputs and the recorded outputs.
"""
from __future__ import annotations

import argparse
import importlib
import math
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(HERE))

import gen_golden  # noqa: E402  (install_shims: the jaxtyping annotation stub and friends)

from transplat_amd import synthetic as S  # noqa: E402


def _rot(yaw: float, pitch: float) -> torch.Tensor:
    cy, sy, cp, sp = math.cos(yaw), math.sin(yaw), math.cos(pitch), math.sin(pitch)
    ry = torch.tensor([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = torch.tensor([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    return (ry @ rx).float()


def _pose(yaw: float, pitch: float, origin) -> torch.Tensor:
    e = torch.eye(4)
    e[:3, :3] = _rot(yaw, pitch)
    e[:3, 3] = torch.tensor(origin, dtype=torch.float32)
    return e


def pose_pairs() -> tuple[torch.Tensor, torch.Tensor]:
    """[4, 4, 4] initial and final poses: the synthetic context pair; a pair yawed and pitched towards
    each other; parallel looks (same rotation, shifted origin); looks 0.02 rad apart (just outside
    eps = 1e-4: 1 - cos 0.02 = 2e-4)."""
    ctx = S.context_extrinsics(2)
    pairs = [
        (ctx[0], ctx[1]),
        (_pose(0.35, -0.12, (-1.5, 0.2, 0.1)), _pose(-0.4, 0.15, (1.7, -0.3, -0.2))),
        (_pose(0.2, 0.1, (0.0, 0.0, 0.0)), _pose(0.2, 0.1, (0.8, -0.1, 0.3))),
        (_pose(0.0, 0.0, (0.0, 0.0, 0.0)), _pose(0.02, 0.0, (0.5, 0.0, 0.0))),
    ]
    return torch.stack([a for a, _ in pairs]), torch.stack([b for _, b in pairs])


def time_sets() -> dict:
    t = torch.linspace(0, 1, 5, dtype=torch.float32)
    return {"smooth": (torch.cos(torch.pi * (t + 1)) + 1) / 2, "exaggerated": t * 5 - 2}


def frame_inputs(shape, seed: int, constant: bool = False):
    """colour U(-0.2, 1.2) [T, 3, H, W]; depth (1 + 9 u)^1.5 with a block of zeros, or constant 3."""
    t, h, w = shape
    gen = torch.Generator().manual_seed(seed)
    color = torch.rand((t, 3, h, w), generator=gen) * 1.4 - 0.2
    depth = (1 + 9 * torch.rand((t, h, w), generator=gen)) ** 1.5
    depth[:, 2:7, 3:11] = 0.0
    if constant:
        depth = torch.full((t, h, w), 3.0)
    return color, depth


def reference_frames(color: torch.Tensor, depth: torch.Tensor, vcat) -> np.ndarray:
    """model_wrapper.py:736-741 restated on float32 torch, then the reference's vcat and :771."""
    import matplotlib

    near = depth[depth > 0][:16_000_000].quantile(0.01).log()
    far = depth.view(-1)[:16_000_000].quantile(0.99).log()
    result = 1 - (depth.log() - near) / (far - near)
    mapped = matplotlib.colormaps["turbo"](result.clip(min=0, max=1).numpy())[..., :3]
    mapped = torch.tensor(mapped, dtype=torch.float32).permute(0, 3, 1, 2)
    video = torch.stack([vcat(rgb, d) for rgb, d in zip(color, mapped)])
    video = (video.clip(min=0, max=1) * 255).type(torch.uint8).numpy()
    return np.ascontiguousarray(video.transpose(0, 2, 3, 1))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="checkout of the reference project")
    ref = Path(ap.parse_args().ref)
    if not (ref / "src" / "visualization").is_dir():
        raise SystemExit(f"{ref} is not a reference checkout")
    gen_golden.install_shims(ref)
    for name in ("src.visualization", "src.visualization.camera_trajectory"):
        m = types.ModuleType(name)
        m.__path__ = [str(ref / name.replace(".", "/"))]
        sys.modules[name] = m
    interp = importlib.import_module("src.visualization.camera_trajectory.interpolation")
    wobble = importlib.import_module("src.visualization.camera_trajectory.wobble")
    layout = importlib.import_module("src.visualization.layout")

    out = {}
    initial, final = pose_pairs()
    out["traj_initial"], out["traj_final"] = initial.numpy(), final.numpy()
    k0, k1 = S.intrinsics(1)[0], S.intrinsics(1)[0] * torch.tensor([[1.2, 1, 0.9], [1, 0.8, 1.1], [1, 1, 1]])
    out["intr_initial"], out["intr_final"] = k0.numpy(), k1.numpy()
    radius = torch.tensor([0.25, 0.4, 0.1, 0.05])
    out["wobble_radius"] = radius.numpy()
    for name, t in time_sets().items():
        out[f"t_{name}"] = t.numpy()
        out[f"traj_{name}"] = interp.interpolate_extrinsics(initial, final, t).numpy()
        out[f"intr_{name}"] = interp.interpolate_intrinsics(k0, k1, t).numpy()
        out[f"wobble_{name}"] = wobble.generate_wobble(initial, radius, t).numpy()
    for name, shape, seed, constant in (("a", (3, 32, 48), 11, False), ("b", (2, 17, 23), 12, False),
                                        ("const", (2, 17, 23), 13, True)):
        color, depth = frame_inputs(shape, seed, constant)
        out[f"frames_{name}_color"], out[f"frames_{name}_depth"] = color.numpy(), depth.numpy()
        out[f"frames_{name}"] = reference_frames(color, depth, layout.vcat)
    np.savez_compressed(HERE / "video.npz", **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
