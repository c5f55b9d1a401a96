"""Rasterizer phase timing (HIP events around each kernel of tsplat_raster_fwd) on the bench's
raster-only workload (1 scene, G = 131,072, 3 target views at 256x256), optionally with the
render-kernel diagnostics of TSPLAT_RASTER_DIAG (2: key load + sort only, 3: key load
only, 4: no blending -- fetch + cull + compaction only; images are wrong in those modes, only
the times mean something).

--depth: what the depth render costs at the same shape, through the decoder: colour only, colour +
depth from the one fused pass (tsplat_raster_depth_fwd), colour + depth by the two-pass route
(TSPLAT_DEPTH_FUSED=0: a second rasterizer run over the Gaussians repeated per view), and the
depth-only call. HIP events around --iters eager calls per sample, the routes alternating inside
one process for --rounds samples each; prints the median, lowest and highest per-call time.

--backward: what the backward (tsplat_raster_bwd through rasterize_differentiable) costs at the same
shape beside the forward call of the same process, its two kernels separately, and the render-backward
kernel's atomic bytes over its time against the chip-wide float-atomic rate.

--backward --depth MODE: forward + backward of the depth routes in one process, the routes alternating:
the colour-only pair (rasterize_differentiable), the fused pairs (rasterize_with_depth_differentiable:
colour + depth, and colour + depth + alpha; tsplat_raster_depth_bwd) and the two-pass composition the
fused call retires (rasterize_differentiable on the colour, plus depth_fake_color under autograd and a
second rasterize_differentiable over the Gaussians repeated per view at sh_degree = 0). HIP events around
--iters eager pairs per sample; then the library's own events around the forward and backward launch
sequences and the two backward kernels of the colour-only and the fused route."""
import argparse
import os
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from bench import build_raster_workload  # noqa: E402
from transplat_amd import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=30)
ap.add_argument("--diag", default="0,2,3")
ap.add_argument("--waves", action="store_true", help="per-wave cost distribution (diag 5)")
ap.add_argument("--depth", default=None, metavar="MODE", help="time the depth routes (a DepthRenderingMode)")
ap.add_argument("--rounds", type=int, default=15, help="--depth, --backward: samples per route")
ap.add_argument("--backward", action="store_true", help="time tsplat_raster_bwd and its two kernels beside the forward")
args = ap.parse_args()
dev = torch.device("cuda:0")


def depth_routes(mode: str) -> None:
    from statistics import median

    from transplat_amd import synthetic as S
    from transplat_amd.model.decoder import DatasetCfgLite, DecoderSplattingHIP, DecoderSplattingHIPCfg
    from transplat_amd.model.types import Gaussians

    hw = (256, 256)
    g = S.make_gaussians(1, image_shape=hw, device=dev)
    t = S.make_batch(1, image_shape=hw, device=dev)["target"]
    gs = Gaussians(g["means"], g["covariances"], g["harmonics"], g["opacities"])
    cam = (t["extrinsics"], t["intrinsics"], t["near"], t["far"])
    dec = DecoderSplattingHIP(DecoderSplattingHIPCfg(check_overflow=False), DatasetCfgLite((0.0, 0.0, 0.0))).to(dev)

    def two_pass():
        os.environ["TSPLAT_DEPTH_FUSED"] = "0"
        try:
            return dec(gs, *cam, hw, depth_mode=mode)
        finally:
            del os.environ["TSPLAT_DEPTH_FUSED"]

    routes = {"colour only": lambda: dec(gs, *cam, hw),
              "fused colour + depth": lambda: dec(gs, *cam, hw, depth_mode=mode),
              "two-pass colour + depth": two_pass,
              "depth only": lambda: dec.render_depth(gs, *cam, hw, mode)}
    with torch.no_grad():
        for f in routes.values():  # warm up every route: code objects, workspace growth, allocator
            for _ in range(5):
                f()
        torch.cuda.synchronize()
        fused, two = routes["fused colour + depth"](), two_pass()
        scale = max(float(two.depth.abs().max()), 1.0)
        print(f"depth mode {mode}: fused vs two-pass colour equal {torch.equal(fused.color, two.color)}, depth max "
              f"diff {float((fused.depth - two.depth).abs().max()):.3e} (scale {scale:.3g})", flush=True)
        us = {k: [] for k in routes}
        for _ in range(args.rounds):
            for k, f in routes.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.iters):
                    f()
                b.record()
                b.synchronize()
                us[k].append(a.elapsed_time(b) / args.iters * 1e3)
    for k, v in us.items():
        print(f"{k:>24}: median {median(v):7.1f} us per call (min {min(v):.1f}, max {max(v):.1f}; {len(v)} samples x "
              f"{args.iters} eager decoder calls, 3 views, G = {g['means'].shape[1]}, 256x256)", flush=True)
    # the rasterizer launch sequences alone (events around them inside the library), without the
    # torch ops and the launch gaps of the eager decoder call around them
    with torch.no_grad():
        for k, f in routes.items():
            _lib.prof_enable("raster")
            for _ in range(args.iters):
                f()
            ms, n = _lib.prof_read()
            _lib.prof_enable(None)
            print(f"{k:>24}: rasterizer launches {ms / args.iters * 1e3:7.1f} us per decoder call ({n // args.iters} "
                  f"rasterizer call(s) each)", flush=True)


def backward_cost() -> None:
    """tsplat_raster_bwd beside tsplat_raster_fwd in one process: HIP events inside the library around
    the forward launch sequence, the backward launch sequence (zero fill included) and its two kernels,
    --rounds samples of --iters forward + backward pairs each; then the render-backward kernel's atomic
    bytes (entries reaching a wave, the forward's diag-5 counters of the same walk, x 9 floats: an upper
    bound, exact zeros are not added) over its time, against the chip-wide float-atomic rate."""
    from statistics import median

    from transplat_amd import synthetic as S
    from transplat_amd.model.decoder.hip_splatting import prepare_cameras, rasterize, rasterize_differentiable

    hw = (256, 256)
    g = S.make_gaussians(1, image_shape=hw, device=dev)
    tb = S.make_batch(1, image_shape=hw, device=dev)["target"]
    b, v = tb["near"].shape
    cams = prepare_cameras(tb["extrinsics"].reshape(b * v, 4, 4), tb["intrinsics"].reshape(b * v, 3, 3),
                           tb["near"].reshape(-1), tb["far"].reshape(-1), torch.zeros(b * v, 3, device=dev))
    leaves = [g[k].clone().requires_grad_() for k in ("means", "covariances", "harmonics", "opacities")]
    grad_color = torch.randn((b * v, 3, *hw), generator=torch.Generator(device=dev).manual_seed(1), device=dev)

    def pair():
        color, _ = rasterize_differentiable(*leaves, cams, hw, v, check=False)
        for t in leaves:
            t.grad = None
        color.backward(grad_color)

    for _ in range(3):
        pair()
    torch.cuda.synchronize()
    ids = ("raster", "raster_bwd", "raster_bwd_render", "raster_bwd_preprocess")
    us = {k: [] for k in ids}
    for _ in range(args.rounds):
        for k in ids:
            _lib.prof_enable(k)
            for _ in range(args.iters):
                pair()
            ms, n = _lib.prof_read()
            _lib.prof_enable(None)
            us[k].append(ms / n * 1e3)
    label = {"raster": "forward call", "raster_bwd": "backward call", "raster_bwd_render": "  render_bwd_kernel",
             "raster_bwd_preprocess": "  preprocess_bwd_kernel"}
    for k in ids:
        print(f"{label[k]:>24}: median {median(us[k]):8.1f} us (min {min(us[k]):.1f}, max {max(us[k]):.1f}; "
              f"{args.rounds} samples x {args.iters} calls, {b * v} views, G = {g['means'].shape[1]}, 256x256)", flush=True)
    os.environ["TSPLAT_RASTER_DIAG"] = "5"
    with torch.no_grad():
        counters = rasterize(*leaves, cams, hw, v, check=False)[0]
    torch.cuda.synchronize()
    os.environ["TSPLAT_RASTER_DIAG"] = "0"
    entries = float(counters.reshape(-1, 3, hw[0] // 8, 8, hw[1] // 8, 8)[:, 1, :, 0, :, 0].double().sum())
    nbytes = entries * 9 * 4
    t = median(us["raster_bwd_render"]) * 1e-6
    print(f"render_bwd_kernel atomics: {entries:.4g} (wave, entry) instances x 36 B = {nbytes / 1e6:.1f} MB per launch "
          f"(upper bound), / {t * 1e6:.1f} us = {nbytes / t / 1e12:.3f} TB/s against the chip-wide float-atomic rate "
          f"of about 1.3 TB/s (floor {nbytes / 1.3e12 * 1e6:.1f} us)", flush=True)


def backward_depth_routes(mode: str) -> None:
    from statistics import median

    from transplat_amd import synthetic as S
    from transplat_amd.model.decoder.decoder_splatting_hip import depth_fake_color
    from transplat_amd.model.decoder.hip_splatting import (prepare_cameras, rasterize_differentiable,
                                                           rasterize_with_depth_differentiable)

    hw = (256, 256)
    g = S.make_gaussians(1, image_shape=hw, device=dev)
    tb = S.make_batch(1, image_shape=hw, device=dev)["target"]
    b, v = tb["near"].shape
    ext, intr = tb["extrinsics"].reshape(b * v, 4, 4), tb["intrinsics"].reshape(b * v, 3, 3)
    near, far = tb["near"].reshape(-1), tb["far"].reshape(-1)
    black = torch.zeros(b * v, 3, device=dev)
    cams = prepare_cameras(ext, intr, near, far, black)
    leaves = [g[k].clone().requires_grad_() for k in ("means", "covariances", "harmonics", "opacities")]
    gen = torch.Generator(device=dev).manual_seed(1)
    grad_color = torch.randn((b * v, 3, *hw), generator=gen, device=dev)
    grad_depth = torch.randn((b * v, *hw), generator=gen, device=dev)
    grad_alpha = torch.randn((b * v, *hw), generator=gen, device=dev)

    def clear():
        for t in leaves:
            t.grad = None

    def colour_pair():
        clear()
        color, _ = rasterize_differentiable(*leaves, cams, hw, v, check=False)
        color.backward(grad_color)

    def fused_pair(alpha):
        clear()
        out = rasterize_with_depth_differentiable(*leaves, cams, hw, v, check=False, near=near, far=far,
                                                  depth_mode=mode, alpha=alpha)
        outs, grads = [out.color, out.depth], [grad_color, grad_depth]
        if alpha:
            outs.append(out.alpha)
            grads.append(grad_alpha)
        torch.autograd.backward(outs, grads)

    def two_pass_pair():
        clear()
        m, k, sh, o = leaves
        color, _ = rasterize_differentiable(m, k, sh, o, cams, hw, v, check=False)
        rep = lambda t: t.repeat_interleave(v, dim=0)
        means = rep(m)
        fake = depth_fake_color(ext, means, near, far, mode)
        fc, _ = rasterize_differentiable(means, rep(k), fake[:, :, None, None].expand(-1, -1, 3, 1).contiguous(), rep(o),
                                         cams, hw, 1, sh_degree=0, check=False)
        torch.autograd.backward([color, fc.mean(dim=1)], [grad_color, grad_depth])

    routes = {"colour only": colour_pair, "fused colour + depth": lambda: fused_pair(False),
              "fused colour + depth + alpha": lambda: fused_pair(True), "two-pass colour + depth": two_pass_pair}
    for f in routes.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    routes["fused colour + depth"]()
    fused = [t.grad.clone() for t in leaves]
    two_pass_pair()
    torch.cuda.synchronize()
    print(f"depth mode {mode}: fused vs two-pass gradients, max |diff| / max |two-pass|: " + ", ".join(
        f"{float((a - t.grad).abs().max() / t.grad.abs().max()):.2e}" for a, t in zip(fused, leaves)), flush=True)
    us = {k: [] for k in routes}
    for _ in range(args.rounds):
        for k, f in routes.items():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                f()
            e.record()
            e.synchronize()
            us[k].append(a.elapsed_time(e) / args.iters * 1e3)
    for k, t in us.items():
        print(f"{k:>30}: median {median(t):8.1f} us per forward + backward (min {min(t):.1f}, max {max(t):.1f}; {len(t)} "
              f"samples x {args.iters} eager pairs, {b * v} views, G = {g['means'].shape[1]}, 256x256)", flush=True)
    ids = ("raster", "raster_bwd", "raster_bwd_render", "raster_bwd_preprocess")
    label = {"raster": "forward call", "raster_bwd": "backward call", "raster_bwd_render": "  render_bwd_kernel",
             "raster_bwd_preprocess": "  preprocess_bwd_kernel"}
    timed = ("colour only", "fused colour + depth", "fused colour + depth + alpha")
    lib_us = {(r, k): [] for r in timed for k in ids}
    for _ in range(args.rounds):
        for r in timed:
            for k in ids:
                _lib.prof_enable(k)
                for _ in range(args.iters):
                    routes[r]()
                ms, n = _lib.prof_read()
                _lib.prof_enable(None)
                lib_us[(r, k)].append(ms / n * 1e3)
    for r in timed:
        for k in ids:
            t = lib_us[(r, k)]
            print(f"{r:>30} {label[k]:<24}: median {median(t):8.1f} us (min {min(t):.1f}, max {max(t):.1f}; "
                  f"{args.rounds} samples x {args.iters} calls)", flush=True)


if args.backward and args.depth:
    backward_depth_routes(args.depth)
    sys.exit(0)
if args.backward:
    backward_cost()
    sys.exit(0)
if args.depth:
    depth_routes(args.depth)
    sys.exit(0)
step, info, _ = build_raster_workload(1, dev, 0)
for _ in range(3):
    step()
torch.cuda.synchronize()
for d in args.diag.split(","):
    os.environ["TSPLAT_RASTER_DIAG"] = d
    row = []
    for k in ("raster_preprocess", "raster_scan", "raster_scatter", "raster_render", "raster"):
        step()
        torch.cuda.synchronize()
        _lib.prof_enable(k)
        for _ in range(args.iters):
            step()
        ms, n = _lib.prof_read()
        _lib.prof_enable(None)
        if n:  # (raster_scan: folded into the scatter kernel in round 5)
            row.append(f"{k}={ms / n * 1e3:.1f}us")
    print(f"diag={d}: " + " ".join(row), flush=True)
os.environ["TSPLAT_RASTER_DIAG"] = "0"
if args.waves:
    os.environ["TSPLAT_RASTER_DIAG"] = "5"
    color = step()[0]
    torch.cuda.synchronize()
    os.environ["TSPLAT_RASTER_DIAG"] = "0"
    # one value per 8x8 block (= wave): [views, 3, H/8, 8, W/8, 8] -> block corner
    c = color.reshape(-1, 3, color.shape[-2] // 8, 8, color.shape[-1] // 8, 8)[:, :, :, 0, :, 0]
    cyc, ent, chk = (c[:, i].flatten().double().cpu() for i in range(3))
    q = torch.tensor([0.0, 0.1, 0.5, 0.9, 0.99, 1.0], dtype=torch.float64)
    print("wave cycles   quantiles", [f"{x:.0f}" for x in torch.quantile(cyc, q)])
    print("entries blended       ", [f"{x:.0f}" for x in torch.quantile(ent, q)])
    print("chunks walked         ", [f"{x:.0f}" for x in torch.quantile(chk, q)])
    print("corr(cycles, entries) %.3f  corr(cycles, chunks) %.3f" % (
        torch.corrcoef(torch.stack([cyc, ent]))[0, 1], torch.corrcoef(torch.stack([cyc, chk]))[0, 1]))
