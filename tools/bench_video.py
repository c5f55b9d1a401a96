"""One 60-frame 256 x 256 wobble video of the synthetic scene, timed per phase on the MI355X: encoder,
trajectory cameras, the rasterizer groups (decoder, depth_mode="depth"), quantile, frames,
device-to-host copy -- HIP events around each phase after a warm-up, `--runs` repetitions, median
(min, max). The tail (quantile + frames + copy) is also timed as a composition of what the tree had
before those kernels: torch.quantile on the boolean-masked depth, the colour map through numpy on
the host, torch for the layout and the uint8 conversion, on the same colour and depth tensors (host
clock around a synchronise, since part of it runs on the host). The interpolation kernel, which the
wobble path does not use, is timed for 60 steps on the side.
Usage: PYTHONPATH=. python tools/bench_video.py [--frames 60] [--runs 20] [--dense-dtype bf16x3]"""
import argparse
import json
import statistics
import time

import torch
from matplotlib import colormaps  # the baseline tail's colour map only; the product path never imports it

from transplat_amd import kernels, video
from transplat_amd import synthetic as S
from transplat_amd.e2e import build_model
from transplat_amd.gemm_tuning import use_tuned_gemms
from transplat_amd.visualization.camera_trajectory.interpolation import interpolate_extrinsics
from transplat_amd.visualization.camera_trajectory.wobble import generate_wobble

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=60)
ap.add_argument("--runs", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--dense-dtype", default="bf16x3")
args = ap.parse_args()
dev = torch.device("cuda:0")
torch.backends.cudnn.benchmark = True
use_tuned_gemms(dev, args.dense_dtype)
model = build_model(dev, args.dense_dtype)
batch = model.data_shim(S.make_batch(1, device=dev))
ctx = batch["context"]
n = args.frames
h, w = ctx["image"].shape[-2:]
turbo = colormaps["turbo"]


def phases():
    """The video phase by phase: the state the phases hand on, and the (name, function) steps in order."""
    state = {}

    def encoder():
        state["g"] = model.encoder(ctx, 0, deterministic=False)

    def trajectory():
        t = video.trajectory_times(n, True, dev)
        radius = (ctx["extrinsics"][:, 0, :3, 3] - ctx["extrinsics"][:, 1, :3, 3]).norm(dim=-1) * 0.25
        state["ext"] = generate_wobble(ctx["extrinsics"][:, 0], radius, t)
        state["intr"] = ctx["intrinsics"][:, :1].expand(-1, n, -1, -1)

    def raster():
        out = model.decoder(state["g"], state["ext"], state["intr"], ctx["near"][:, :1].expand(-1, n),
                            ctx["far"][:, :1].expand(-1, n), (h, w), depth_mode="depth")
        state["color"], state["depth"] = out.color[0], out.depth[0]

    def quantile():
        state["q"] = kernels.quantile(state["depth"].reshape(-1)[:kernels.QUANTILE_MAX], video.DEPTH_QUANTILES)

    def frames():
        state["frames"] = kernels.video_frames(state["color"], state["depth"], state["q"])

    def copy():
        state["host"] = state["frames"].cpu()

    def interpolation_kernel():
        t = video.trajectory_times(n, True, dev)
        interpolate_extrinsics(ctx["extrinsics"][0, 0], ctx["extrinsics"][0, 1], t)

    def tail_before():
        depth, color = state["depth"], state["color"]
        near = depth[depth > 0][:16_000_000].quantile(0.01).log()
        far = depth.view(-1)[:16_000_000].quantile(0.99).log()
        r = 1 - (depth.log() - near) / (far - near)
        mapped = turbo(r.clip(min=0, max=1).cpu().numpy())[..., :3]
        mapped = torch.tensor(mapped, device=dev, dtype=torch.float32).permute(0, 3, 1, 2)
        gap = torch.ones((n, 3, 8, w), device=dev)
        frames = torch.cat([color, gap, mapped], dim=2)
        state["host_before"] = (frames.clip(min=0, max=1) * 255).type(torch.uint8).permute(0, 2, 3, 1).cpu()

    return state, [("encoder", encoder), ("trajectory (wobble, torch ops)", trajectory),
                   (f"rasterizer groups ({n} views)", raster), ("quantile", quantile), ("frames", frames),
                   ("device-to-host copy", copy), ("interpolation kernel (on the side)", interpolation_kernel),
                   ("tail before: torch.quantile + numpy colour map + copy", tail_before)]


state, steps = phases()
times = {name: {"event_ms": [], "wall_ms": []} for name, _ in steps}
with torch.no_grad():
    for it in range(args.warmup + args.runs):
        for name, fn in steps:
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[name]["event_ms"].append(a.elapsed_time(b))
                times[name]["wall_ms"].append((time.perf_counter() - t0) * 1e3)

same = (state["host"] == state["host_before"]).all(dim=-1).float().mean().item()
print(f"{n} frames of {h} x {w}, dense {args.dense_dtype}, {args.runs} runs after {args.warmup} warm-up; "
      f"frames {tuple(state['host'].shape)}; pixels equal to the fp32 torch / numpy tail: {same:.6f}")
result = {}
for name, _ in steps:
    ev, wall = times[name]["event_ms"], times[name]["wall_ms"]
    result[name] = {"event_ms_median": statistics.median(ev), "event_ms_min": min(ev), "event_ms_max": max(ev),
                    "wall_ms_median": statistics.median(wall)}
    print(f"{name:56s} events median {statistics.median(ev):9.3f} ms (min {min(ev):.3f}, max {max(ev):.3f})   "
          f"host clock median {statistics.median(wall):9.3f} ms", flush=True)
tail = sum(result[k]["event_ms_median"] for k in ("quantile", "frames", "device-to-host copy"))
print(f"tail now (quantile + frames + copy, events): {tail:.3f} ms")
print(json.dumps({"frames": n, "shape": [h, w], "dense_dtype": args.dense_dtype, "phases": result}))
