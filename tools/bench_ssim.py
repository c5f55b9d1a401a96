"""The evaluation's SSIM at its shape (one scene: 3 target views of 3 x 256 x 256): tsplat_ssim_fwd
against the compute_psnr torch sequence on the same tensors, the yardstick for "a metric's cost".
HIP events around `--calls` back-to-back calls, after a warm-up; the median over `--runs` runs, per
call. tsplat_ssim_fwd is called through the C-ABI with its workspace allocated once (the kernel pair
alone); kernels.ssim adds the binding's two allocations. Usage: python tools/bench_ssim.py [--n 3]"""
import argparse
import statistics

import torch

from transplat_amd import _lib, kernels
from transplat_amd.evaluation.metrics import compute_psnr

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=3)
ap.add_argument("--hw", type=int, nargs=2, default=(256, 256))
ap.add_argument("--runs", type=int, default=30)
ap.add_argument("--calls", type=int, default=50)
args = ap.parse_args()
dev = torch.device("cuda:0")
n, (h, w) = args.n, args.hw
gen = torch.Generator().manual_seed(0)
gt = torch.rand((n, 3, h, w), generator=gen).to(dev)
pred = (gt + 0.05 * torch.randn((n, 3, h, w), generator=gen).to(dev)).contiguous()
lib = _lib.load()
out = torch.empty(n, device=dev)
ws = torch.empty(int(lib.tsplat_ssim_workspace_bytes(n, h, w)), dtype=torch.uint8, device=dev)
stream = _lib.stream_ptr(dev)


def raw():
    _lib.check(lib.tsplat_ssim_fwd(gt.data_ptr(), pred.data_ptr(), out.data_ptr(), ws.data_ptr(), n, h, w, stream),
               "tsplat_ssim_fwd")


def timeit(fn):
    for _ in range(20):
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


raw()
assert torch.equal(out, kernels.ssim(gt, pred))
print(f"{n} x 3 x {h} x {w}: ssim {out.tolist()}  psnr {compute_psnr(gt, pred).tolist()}")
for name, fn in (("tsplat_ssim_fwd", raw), ("kernels.ssim", lambda: kernels.ssim(gt, pred)),
                 ("compute_psnr (torch)", lambda: compute_psnr(gt, pred))):
    med, lo, hi = timeit(fn)
    print(f"{name:22s} median {med:7.1f} us per call  (min {lo:.1f}, max {hi:.1f}; {args.runs} runs x {args.calls} calls)",
          flush=True)
