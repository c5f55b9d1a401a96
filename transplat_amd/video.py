"""Fly-through videos (reference ModelWrapper.render_video_generic, render_video_interpolation,
render_video_wobble and render_video_interpolation_exaggerated, src/model/model_wrapper.py:616-790):
frames along a camera path between the context views, colour above colour-mapped depth.

From the Gaussians to uint8 frames everything stays on the device: the trajectory cameras are one
launch, the decoder renders colour and depth in one pass per group of views, the depth colour map's
two quantiles come from a radix selection (no sort, no boolean-mask indexing), and one launch
writes every frame; one device-to-host copy ends it. Deviations from the reference: no "Softmax"
label and no 8-px border (they need a font file), both quantiles look at the first 16,000,000
depth values, and an empty positive depth population gives a black depth half instead of raising.

`python -m transplat_amd.video --index ... --trajectory wobble --output-dir out` writes
out/<scene>/<trajectory>/<frame:0>6>.png (no mp4: the PNG sequence is what an encoder is fed).
"""
from __future__ import annotations

import json
from pathlib import Path
from typing import Callable, Optional

import torch
from torch import Tensor

from . import kernels
from .visualization.camera_trajectory.interpolation import interpolate_extrinsics, interpolate_intrinsics
from .visualization.camera_trajectory.wobble import generate_wobble, generate_wobble_transformation

TrajectoryFn = Callable[[Tensor], tuple[Tensor, Tensor]]  # t [T] -> extrinsics [b, T, 4, 4], intrinsics [b, T, 3, 3]

# (q, positive_only) of the depth colour map: near = log(q01 of the positive depths), far = log(q99)
DEPTH_QUANTILES = ((0.01, True), (0.99, False))


def trajectory_times(num_frames: int, smooth: bool, device) -> Tensor:
    """linspace(0, 1, num_frames), cosine-smoothed (ease in, ease out) when `smooth`."""
    t = torch.linspace(0, 1, num_frames, dtype=torch.float32, device=device)
    if smooth:
        t = (torch.cos(torch.pi * (t + 1)) + 1) / 2
    return t


def loop_order(num_frames: int, loop_reverse: bool) -> list[int]:
    """Frame indices of the finished video: forward, then (loop_reverse) backward without the two end
    frames, the reference's pack([video, video[::-1][1:-1]])."""
    fwd = list(range(num_frames))
    return fwd + fwd[::-1][1:-1] if loop_reverse else fwd


def compose_frames(color: Tensor, depth: Tensor) -> Tensor:
    """color [T, 3, H, W], depth [T, H, W] on the device -> uint8 [T, 2H + 8, W, 3] on the device: one
    quantile call over the first 16,000,000 depth values, one frames launch."""
    flat = depth.reshape(-1)[:kernels.QUANTILE_MAX]
    return kernels.video_frames(color, depth, kernels.quantile(flat, DEPTH_QUANTILES))


@torch.no_grad()
def render_video_generic(model, batch: dict, trajectory_fn: TrajectoryFn, num_frames: int = 30,
                         smooth: bool = True, loop_reverse: bool = True) -> Tensor:
    """Encoder once, cameras from trajectory_fn(t), decoder with depth_mode="depth" (in groups of
    views when num_frames > 32), frames -> uint8 [F, 2H + 8, W, 3] on the host, F = num_frames or
    2 num_frames - 2 with loop_reverse. Scene 0 of the batch is rendered, as in the reference."""
    batch = model.data_shim(batch)
    ctx = batch["context"]
    device = ctx["image"].device
    gaussians = model.encoder(ctx, 0, deterministic=False)
    t = trajectory_times(num_frames, smooth, device)
    extrinsics, intrinsics = trajectory_fn(t)
    _, _, _, h, w = ctx["image"].shape
    near = ctx["near"][:, :1].expand(-1, num_frames)  # TODO of the reference too: planes not interpolated
    far = ctx["far"][:, :1].expand(-1, num_frames)
    out = model.decoder(gaussians, extrinsics, intrinsics, near, far, (h, w), depth_mode="depth")
    frames = compose_frames(out.color[0], out.depth[0])
    if loop_reverse:  # loop_order(num_frames, True), without an index tensor from the host
        frames = torch.cat([frames, frames.flip(0)[1:-1]])
    return frames.cpu()


def _pair(batch: dict, key: str) -> tuple[Tensor, Tensor]:
    """Scene 0's end points of the interpolation: context views 0 and 1, or (other than two context
    views) context view 0 and the first target view."""
    ctx = batch["context"][key]
    last = ctx[0, 1] if ctx.shape[1] == 2 else batch["target"][key][0, 0]
    return ctx[0, 0], last


def _baseline(batch: dict) -> Tensor:
    ext = batch["context"]["extrinsics"]
    return (ext[:, 0, :3, 3] - ext[:, 1, :3, 3]).norm(dim=-1)


def render_video_interpolation(model, batch: dict, num_frames: int = 30) -> Tensor:
    """Interpolate from context view 0 to context view 1 (30 frames, smoothed, looped back)."""
    batch = model.data_shim(batch)

    def trajectory_fn(t):
        extrinsics = interpolate_extrinsics(*_pair(batch, "extrinsics"), t)
        intrinsics = interpolate_intrinsics(*_pair(batch, "intrinsics"), t)
        return extrinsics[None], intrinsics[None]

    return render_video_generic(model, batch, trajectory_fn, num_frames=num_frames)


def render_video_wobble(model, batch: dict, num_frames: int = 60) -> Optional[Tensor]:
    """Context view 0 circling in its image plane with radius 0.25 |o_a - o_b| (60 frames). None
    unless there are exactly two context views (the radius needs them)."""
    batch = model.data_shim(batch)
    if batch["context"]["extrinsics"].shape[1] != 2:
        return None

    def trajectory_fn(t):
        extrinsics = generate_wobble(batch["context"]["extrinsics"][:, 0], _baseline(batch) * 0.25, t)
        intrinsics = batch["context"]["intrinsics"][:, :1].expand(-1, t.shape[0], -1, -1)
        return extrinsics, intrinsics

    return render_video_generic(model, batch, trajectory_fn, num_frames=num_frames)


def render_video_interpolation_exaggerated(model, batch: dict, num_frames: int = 300) -> Optional[Tensor]:
    """The interpolation run from t = -2 to 3 with a 5-turn wobble of radius 0.5 |o_a - o_b| on top
    (300 frames, not smoothed, not looped). None unless there are exactly two context views."""
    batch = model.data_shim(batch)
    if batch["context"]["extrinsics"].shape[1] != 2:
        return None

    def trajectory_fn(t):
        tf = generate_wobble_transformation(_baseline(batch) * 0.5, t, 5, scale_radius_with_t=False)
        extrinsics = interpolate_extrinsics(*_pair(batch, "extrinsics"), t * 5 - 2)
        intrinsics = interpolate_intrinsics(*_pair(batch, "intrinsics"), t * 5 - 2)
        return extrinsics @ tf, intrinsics[None]

    return render_video_generic(model, batch, trajectory_fn, num_frames=num_frames, smooth=False,
                                loop_reverse=False)


TRAJECTORIES = {"rgb": render_video_interpolation, "wobble": render_video_wobble,
                "exaggerated": render_video_interpolation_exaggerated}


def write_frames(frames: Tensor, directory: str | Path) -> Path:
    """uint8 [F, H, W, 3] host frames -> directory/<frame:0>6>.png."""
    from PIL import Image

    directory = Path(directory)
    directory.mkdir(parents=True, exist_ok=True)
    for i, frame in enumerate(frames.numpy()):
        Image.fromarray(frame).save(directory / f"{i:0>6}.png")
    return directory


def parse_args(argv=None):
    import argparse

    ap = argparse.ArgumentParser(prog="python -m transplat_amd.video", description=__doc__.split("\n\n")[0])
    ap.add_argument("--index", required=True, help="evaluation index (the scenes and their context views)")
    ap.add_argument("--data-root", action="append", default=None,
                    help="dataset root holding test/*.torch chunks (repeatable); real frames instead of synthetic")
    ap.add_argument("--checkpoint", default=None, help="reference Lightning checkpoint (loaded weights_only)")
    ap.add_argument("--experiment", choices=["re10k", "acid", "dtu"], default="re10k")
    ap.add_argument("--dense-dtype", choices=["fp32", "bf16x3", "bf16"], default="bf16x3")
    ap.add_argument("--scene", default=None, help="scene key of the index (default: its first scene)")
    ap.add_argument("--trajectory", choices=sorted(TRAJECTORIES), default="rgb")
    ap.add_argument("--output-dir", required=True, help="frames go to DIR/<scene>/<trajectory>/<frame:0>6>.png")
    return ap.parse_args(argv)


def _scene_batch(args, device) -> dict:
    """The batch (b = 1) of the chosen scene: from the chunks under --data-root, else synthetic
    frames at the index entry's frame positions."""
    from .evaluate import index_batch, load_index

    if args.data_root:
        from .dataset import EXPERIMENTS, ChunkDatasetCfg, ChunkTestDataset

        cfg = ChunkDatasetCfg(roots=tuple(args.data_root), **EXPERIMENTS[args.experiment])
        for example in ChunkTestDataset.from_index_file(cfg, args.index):
            if args.scene is None or example["scene"] == args.scene:
                return ChunkTestDataset.batch(example, device)
        raise SystemExit(f"scene {args.scene!r} is not in the chunks under {args.data_root}")
    scenes = load_index(args.index)
    for i, (key, entry) in enumerate(scenes):
        if args.scene is None or key == args.scene:
            batch = index_batch(i, key, entry, device=device)
            batch["scene"] = [key]
            return batch
    raise SystemExit(f"scene {args.scene!r} is not in {args.index}")


def main(argv=None) -> None:
    args = parse_args(argv)
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    from .e2e import build_model
    from .gemm_tuning import use_tuned_gemms

    torch.backends.cudnn.benchmark = True
    use_tuned_gemms(device, args.dense_dtype)
    model = build_model(device, args.dense_dtype)
    if args.checkpoint:
        model.load_checkpoint(args.checkpoint)
    batch = _scene_batch(args, device)
    frames = TRAJECTORIES[args.trajectory](model, batch)
    if frames is None:
        raise SystemExit(f"the {args.trajectory} video needs exactly two context views")
    out = write_frames(frames, Path(args.output_dir) / batch["scene"][0] / args.trajectory)
    print(json.dumps({"scene": batch["scene"][0], "trajectory": args.trajectory, "frames": frames.shape[0],
                      "shape": list(frames.shape), "output": str(out)}), flush=True)


if __name__ == "__main__":
    main()
