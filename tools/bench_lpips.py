"""The evaluation's LPIPS at its shape (one scene: 3 target views of 3 x 256 x 256) with
LpipsVGG.seeded(0): kernels.lpips as a whole, then its parts -- the thirteen exact-fp32 Winograd
convolutions and the seven launches around them (tsplat_lpips_scale_fwd, five tsplat_lpips_tap_fwd,
tsplat_lpips_reduce_fwd) -- and per tap shape the bytes tsplat_lpips_tap_fwd must move (both images'
features once, the pooled map once) over its time, as a fraction of the HBM peak. HIP events around
`--calls` back-to-back calls after a warm-up; the median over `--runs` runs, per call, with min and max.
The parts run on maps kept from one pass, with their outputs allocated by the bindings as in the whole
call. Usage: python tools/bench_lpips.py [--n 3]"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from transplat_amd import _lib, kernels
from transplat_amd.evaluation.lpips_vgg import VGG_BLOCKS, LpipsVGG

HBM_PEAK = 8.0e12  # bytes / s, the MI355X's specified HBM3E rate

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=3)
ap.add_argument("--hw", type=int, nargs=2, default=(256, 256))
ap.add_argument("--runs", type=int, default=15)
ap.add_argument("--calls", type=int, default=10)
args = ap.parse_args()
dev = torch.device("cuda:0")
n, (h, w) = args.n, args.hw
gen = torch.Generator().manual_seed(0)
gt = torch.rand((n, 3, h, w), generator=gen).to(dev)
pred = (gt + 0.05 * torch.randn((n, 3, h, w), generator=gen).to(dev)).contiguous()
net = LpipsVGG.seeded(0).to(dev)
lib = _lib.load()


def timeit(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1000 / args.calls)
    return statistics.median(times), min(times), max(times)


def report(name, stat, extra=""):
    med, lo, hi = stat
    print(f"{name:44s} median {med:9.1f} us  (min {lo:.1f}, max {hi:.1f}){extra}", flush=True)


# one pass that keeps every convolution's input and every tap's input
x = kernels.lpips_scale(gt, pred)
conv_inputs, tap_inputs, conv = [], [], 0
for k, count in enumerate(VGG_BLOCKS):
    for _ in range(count):
        conv_inputs.append(x)
        x = kernels.conv3x3_wino(x, *net.convs[conv], act="relu", precision="fp32")
        conv += 1
    tap_inputs.append(x)
    if k + 1 < len(VGG_BLOCKS):
        x = torch.nn.functional.max_pool2d(x, 2)

value, layers = kernels.lpips(gt, pred, net, return_layers=True)
print(f"{n} x 3 x {h} x {w}, {args.runs} runs x {args.calls} calls: lpips {value.tolist()} taps {layers[0].tolist()}")
report("kernels.lpips (20 launches)", timeit(lambda: kernels.lpips(gt, pred, net)))


def convs():
    for i, xin in enumerate(conv_inputs):
        kernels.conv3x3_wino(xin, *net.convs[i], act="relu", precision="fp32")


report("13 convolutions (fp32 Winograd)", timeit(convs))
for i, xin in enumerate(conv_inputs):
    co, ci = net.convs[i][0].shape[:2]
    stat = timeit(lambda: kernels.conv3x3_wino(xin, *net.convs[i], act="relu", precision="fp32"))
    flop = 2.0 * xin.shape[0] * xin.shape[2] * xin.shape[3] * co * ci * 9
    report(f"  conv {i + 1:2d}: {ci:3d} -> {co:3d} at {xin.shape[2]} x {xin.shape[3]}", stat,
           f"  {flop / stat[0] / 1e6:6.1f} TFLOP/s (direct-form FLOPs)")

blocks = [int(lib.tsplat_lpips_tap_blocks(*t.shape[1:])) for t in tap_inputs]
ws = torch.empty(n * sum(blocks), dtype=torch.float64, device=dev)
out = torch.empty(n, device=dev)


def new_launches():
    kernels.lpips_scale(gt, pred)
    at = 0
    for k, t in enumerate(tap_inputs):
        kernels._lpips_tap_into(t, net.lins[k], ws[at:at + n * blocks[k]], pool=k + 1 < len(tap_inputs))
        at += n * blocks[k]
    kernels._lpips_reduce(ws, n, blocks, [t.shape[2] * t.shape[3] for t in tap_inputs], out, None)


new_launches()
assert torch.equal(out, value)
report("7 new launches (scale, 5 taps, reduce)", timeit(new_launches))
report("  tsplat_lpips_scale_fwd", timeit(lambda: kernels.lpips_scale(gt, pred)))
at = 0
for k, t in enumerate(tap_inputs):
    pool = k + 1 < len(tap_inputs)
    part = ws[at:at + n * blocks[k]]
    at += n * blocks[k]
    stat = timeit(lambda: kernels._lpips_tap_into(t, net.lins[k], part, pool=pool))
    nbytes = t.numel() * 4 + (t.shape[0] * t.shape[1] * (t.shape[2] // 2) * (t.shape[3] // 2) * 4 if pool else 0)
    report(f"  tsplat_lpips_tap_fwd {tuple(t.shape[1:])}", stat,
           f"  {nbytes / 1e6:6.1f} MB, {nbytes / stat[0] / 1e6:5.2f} TB/s = {100 * nbytes / stat[0] * 1e6 / HBM_PEAK:4.1f} % of HBM peak")
report("  tsplat_lpips_reduce_fwd", timeit(
    lambda: kernels._lpips_reduce(ws, n, blocks, [t.shape[2] * t.shape[3] for t in tap_inputs], out, None)))
