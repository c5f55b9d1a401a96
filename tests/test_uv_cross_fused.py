"""The fused fine cross correlation (tsplat_uv_cross_pack_fwd + tsplat_uv_cross_fused_fwd): the table
route's split-bf16 products computed per 32-query block in LDS and gathered there, with the bands
of the other view's map that no sample of the block touches skipped.

Bound: the one the project uses for this operation (test_uv_cross_kernel), max |delta| < 1e-4
against oracle.encoder_ops.uv_cross on O(1) outputs, inside dense_precision("bf16x3").
"""
import ctypes
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_encoder_ops import _cams, seeded  # noqa: E402

from oracle import encoder_ops as E  # noqa: E402

# (H, W, B, D, offsets scale, points)
CASES = [
    (6, 10, 1, 5, 2.0, 4),      # HW = 60: less than one query-block pair, less than one band, odd D
    (12, 40, 1, 33, 2.0, 4),    # non-square, HW = 15 query blocks, partial last band
    (16, 16, 2, 128, 40.0, 4),  # most samples off-image, every band touched (dense path), B = 2 indexing
    (16, 16, 2, 128, 0.0, 4),   # few bands touched (skip path)
    (24, 24, 2, 128, 2.0, 4),   # the existing table case
    (6, 10, 1, 130, 2.0, 3),    # fewer points than the kernel's 4 slots; D above its 128 depths per pass
    (6, 10, 1, 70, 2.0, 8),     # the 8-point kernel, D above its 64 depths per pass
]
_REF: dict = {}


def _case(h, w, b, d, scale, pts):
    """Inputs and the CPU reference of one case, computed once and shared (never modified)."""
    k = (h, w, b, d, scale, pts)
    if k not in _REF:
        intr, pose, disp = _cams(b, max(h, w))  # the helper's square-image cameras at the longer side
        if d > disp.shape[1]:  # beyond the helper's 128: its first ones again, 10 % farther
            disp = torch.cat([disp, disp[:, :d - disp.shape[1]] * 0.9], dim=1)
        disp = disp[:, :d].contiguous()
        value = seeded((b, 2, h * w, 128), 41)
        key = seeded((b, 2, h * w, 128), 42)
        offsets = seeded((b * 2, h * w, d * pts * 2), 43, scale)
        logits = seeded((b * 2, h * w, d * pts), 44)
        ref = E.uv_cross(value, key, intr, pose, disp, offsets, logits, h, w)
        _REF[k] = ((value, key, intr, pose, disp, offsets, logits), ref)
    return _REF[k]


@pytest.mark.gpu
@pytest.mark.parametrize("h,w,b,d,scale,pts", CASES)
def test_uv_cross_fused(device, h, w, b, d, scale, pts):
    from transplat_amd import kernels as K

    args, ref = _case(h, w, b, d, scale, pts)
    nonzero = (ref != 0).float().mean().item()
    dev = [t.to(device) for t in args]
    with K.dense_precision("bf16x3"):
        routed = K.uv_cross(*dev, h, w).cpu()  # the default route of this mode
    out = K.uv_cross_fused(*dev, h, w).cpu()
    again = K.uv_cross_fused(*dev, h, w).cpu()
    # the table route of the same mode, called directly: K = 3C split-bf16 GEMM + table gather
    value, key, intr, pose, disp, offsets, logits = dev
    k3 = K.split_bf16x3(key.reshape(b * 2, h * w, 128))
    v3 = K.split_bf16x3(torch.flip(value, dims=[1]).reshape(b * 2, h * w, 128), weight_order=True)
    table = torch.bmm(k3, v3.transpose(1, 2), out_dtype=torch.float32)
    tab = torch.empty_like(out, device=device)
    lib = K._lib.load()
    K._lib.check(lib.tsplat_uv_cross_table_fwd(K._lib.ptr(table), K._lib.ptr(K.pack_cameras(intr, pose)),
                                               K._lib.ptr(disp), K._lib.ptr(offsets), K._lib.ptr(logits),
                                               K._lib.ptr(tab), b, h, w, 128, d, pts, K._lib.stream_ptr(device)),
                 "tsplat_uv_cross_table_fwd")
    tab = tab.cpu()
    d_ref, d_tab = (out - ref).abs().max().item(), (out - tab).abs().max().item()
    print(f"uv_cross_fused {h}x{w} b={b} D={d} P={pts} scale={scale}: vs oracle {d_ref:.2e}, vs table route {d_tab:.2e}, "
          f"reference non-zero in {nonzero:.2f} of the outputs")
    assert nonzero > 0.05
    assert K._UV_FUSED and torch.equal(routed, out)
    assert torch.equal(out, again)
    assert d_ref < 1e-4
    assert d_tab < 1e-4


def test_uv_cross_fused_rejects_bad_arguments():
    """Null pointers, C != 128 and P > 8 return TSPLAT_EINVAL before anything is launched (CPU host)."""
    from transplat_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16  # never dereferenced: every call is rejected
    einval = -1

    def fused(ptrs=None, c=128, pts=4):
        a = [p] * 7 if ptrs is None else ptrs
        return lib.tsplat_uv_cross_fused_fwd(*a, 1, 4, 4, c, 2, pts, None)

    for i in range(7):
        assert fused([None if j == i else p for j in range(7)]) == einval
    assert fused(c=64) == einval
    assert fused(pts=9) == einval
    assert fused(pts=0) == einval
    assert lib.tsplat_uv_cross_pack_fwd(None, p, 1, 4, 4, 128, None) == einval
    assert lib.tsplat_uv_cross_pack_fwd(p, None, 1, 4, 4, 128, None) == einval
    assert lib.tsplat_uv_cross_pack_fwd(p, p, 1, 4, 4, 64, None) == einval
    assert lib.tsplat_uv_cross_pack_bytes(1, 64, 64) == 2 * 4096 * 512
    assert lib.tsplat_uv_cross_pack_bytes(1, 6, 10) == 2 * 64 * 512


def test_conv3x3_few_rejects_misaligned_output_and_residuals():
    """tsplat_conv3x3_few_bf16x3_fwd moves y, residual and residual2 as float4: a pointer that is not
    16-byte aligned is TSPLAT_EINVAL before anything is launched (CPU host), on a shape the kernel
    takes (2 x 32 -> 32 at 256^2, form 41) with every other argument valid."""
    from transplat_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16  # never dereferenced: every call is rejected
    srcs = ctypes.cast((ctypes.c_void_p * 1)(p), ctypes.c_void_p)
    chans = ctypes.cast((ctypes.c_int32 * 1)(32), ctypes.c_void_p)
    assert lib.tsplat_conv3x3_few_form(2, 32, 256, 256, 32) == 41

    def few(y=p, residual=None, residual2=None):
        return lib.tsplat_conv3x3_few_bf16x3_fwd(srcs, chans, 1, p, p, residual, residual2, y, 2, 256, 256, 32, 0, 0,
                                                 None)

    for off in (4, 8, 12):
        assert few(y=p + off) == -1
        assert few(residual=p + off) == -1
        assert few(residual=p, residual2=p + off) == -1
