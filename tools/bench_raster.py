"""Rasterizer phase timing (HIP events around each kernel of tsplat_raster_fwd) on the bench's
raster-only workload (1 scene, G = 131,072, 3 target views at 256x256), optionally with the
render-kernel diagnostics of TSPLAT_RASTER_DIAG (2: key load + sort only, 3: key load
only, 4: no blending -- fetch + cull + compaction only; images are wrong in those modes, only
the times mean something).

--depth: what the depth render costs at the same shape, through the decoder: colour only, colour +
depth from the one fused pass (tsplat_raster_depth_fwd), colour + depth by the two-pass route
(TSPLAT_DEPTH_FUSED=0: a second rasterizer run over the Gaussians repeated per view), and the
depth-only call. HIP events around --iters eager calls per sample, the routes alternating inside
one process for --rounds samples each; prints the median, lowest and highest per-call time."""
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
ap.add_argument("--rounds", type=int, default=15, help="--depth: samples per route")
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
