"""Bit comparison of attention_merge (window attention partials + merge projection) across builds of
the library: each build runs in a fresh child process (TSPLAT_LIB), which saves its outputs; the
parent compares them with torch.equal.

    python tools/ab_attn_merge.py tools/_bin/prev.so transplat_amd/libtransplat_hip.so"""
import math
import os
import subprocess
import sys
import tempfile

CASES = [(1, 64, 64), (2, 64, 64), (1, 32, 96)]  # batch, height, width; 2 x 2 windows, shifted


def child(out_path):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch

    from transplat_amd import kernels as K

    dev = torch.device("cuda:0")
    outs = {}
    for b, h, w in CASES:
        g = torch.Generator().manual_seed(b * 1000 + w)
        q, k, v, r = (torch.randn((b, h * w, 128), generator=g).to(dev) for _ in range(4))
        wm = (torch.randn((128, 128), generator=g) / math.sqrt(128)).to(dev)
        ln = ((torch.randn(128, generator=g) * 0.1 + 1).to(dev), (torch.randn(128, generator=g) * 0.1).to(dev), 1e-5)
        for dense in ("fp32", "bf16x3"):
            with K.dense_precision(dense):
                outs[f"{dense} b={b} {h}x{w}"] = K.attention_merge(q, k, v, h, w, 2, True, wm, ln, residual=r).cpu()
    torch.save(outs, out_path)


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
        sys.exit(0)
    import torch

    results = []
    with tempfile.TemporaryDirectory() as tmp:
        for i, lib in enumerate(sys.argv[1:]):
            path = os.path.join(tmp, f"out{i}.pt")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], check=True,
                           env={**os.environ, "TSPLAT_LIB": os.path.abspath(lib)})
            results.append(torch.load(path))
    bad = 0
    for name, ref in results[0].items():
        for lib, res in zip(sys.argv[2:], results[1:]):
            same = torch.equal(ref, res[name])
            bad += not same
            print(f"{name:22s} {lib}: {'bit-identical' if same else 'DIFFERS'} to {sys.argv[1]}"
                  f" (max diff {(ref - res[name]).abs().max().item():.2e})", flush=True)
    sys.exit(1 if bad else 0)
