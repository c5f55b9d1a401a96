"""Bands of the other view's map that each workgroup of tsplat_uv_cross_fused_fwd computes, and its
phase clocks, in one eager e2e step on the bench's synthetic cameras (diagnostic build: tools/build_var.sh
tools/var/uvx_diag.so uvfused.hip -DTSPLAT_UVX_DIAG=1; run with TSPLAT_LIB pointing at it).
A band is 512 consecutive pixels (8 rows at 64 x 64: 8 bands per map); the dense worst case computes
all of them. usage: uv_cross_bands.py [batch]"""
import ctypes
import sys

import torch

from transplat_amd import _lib
from transplat_amd import kernels as K
from transplat_amd import synthetic as S
from transplat_amd.e2e import build_model

batch = int(sys.argv[1]) if len(sys.argv) > 1 else 1
dev = torch.device("cuda:0")
lib = _lib.load()
diag = lib.tsplat_uv_cross_fused_diag
diag.argtypes = [ctypes.c_void_p]
diag.restype = ctypes.c_int
model = build_model(dev, "bf16x3")
data = S.make_batch(batch, image_shape=(256, 256), device=dev)
model.test_step(data)
torch.cuda.synchronize()

records = []
fused = K.uv_cross_fused


def counted(value, key, intr, pose, disp, offsets, logits, h, w):
    hw = h * w
    buf = torch.full((2 * value.shape[0] * -(-hw // 32), 8), -1, dtype=torch.int32, device=dev)
    assert diag(buf.data_ptr()) == 0
    out = fused(value, key, intr, pose, disp, offsets, logits, h, w)
    torch.cuda.synchronize()
    assert diag(None) == 0
    records.append((h, w, buf.cpu()))
    return out


K.uv_cross_fused = counted
model.test_step(data)
torch.cuda.synchronize()
K.uv_cross_fused = fused
for i, (h, w, rec) in enumerate(records):
    bands = -(-h * w // 512)
    cnt = rec[:, 0]
    hist = torch.bincount(cnt.clamp(min=0), minlength=bands + 1).tolist()
    print(f"layer {i}: {h}x{w}, {len(cnt)} workgroups, {bands} bands per map: mean {cnt.float().mean().item():.2f} "
          f"touched, max {cnt.max().item()}, workgroups by bands touched (0..{bands}) {hist}", flush=True)
    us = rec[:, 1:5].float() / 100.0  # 100-MHz clock
    for k, name in enumerate(["marking pass", "fills", "gathers", "whole workgroup"]):
        col = us[:, k].sort().values
        print(f"    {name:16s} median {col[len(col) // 2].item():6.2f} us, max {col[-1].item():6.2f} us", flush=True)
