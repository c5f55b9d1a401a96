"""Operands read in place instead of through a copy: the gate multiply and the channel-last output inside
the camera-parameter encoder's 1x1 (tsplat_conv1x1_bf16x3_scaled_fwd) and [x1 | x2] rows in the split-bf16
GEMM (tsplat_gemm_x3_cat_fwd). Each runs the kernel of the materialised form on the same values in the
same order, so every comparison is bit for bit.
"""
import ctypes
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_encoder_ops import seeded  # noqa: E402


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(8, 8), (4, 12)])
def test_scaled_1x1_channel_last_bit_identical(device, h, w):
    from transplat_amd import kernels as K

    n, ci, co = 2, 128, 128
    x, g = seeded((n, ci, h, w), 801).to(device), seeded((n, ci), 802, 1.0, "rand").to(device)
    weight, bias = seeded((co, ci, 1, 1), 803, ci ** -0.5).to(device), seeded((co,), 804).to(device)
    with K.dense_precision("bf16x3"):
        assert K.conv1x1_scaled_ok(x, weight)
        ref = K.conv2d_direct(x * g.view(n, ci, 1, 1), weight, bias)  # what nn.Conv2d's dispatch runs for it
        nchw = K.conv1x1_scaled(x, g, weight, bias)
        rows = K.conv1x1_scaled(x, g, weight, bias, channel_last=True)
    assert torch.equal(nchw, ref)
    assert tuple(rows.shape) == (n, h * w, co)
    assert torch.equal(rows, ref.flatten(2).transpose(1, 2).contiguous())
    assert not K.conv1x1_scaled_ok(x, weight)  # outside the bf16x3 mode: the module path


@pytest.mark.gpu
def test_cam_param_encoder_channel_last(device):
    """forward(channel_last=True) in the bf16x3 mode returns the rows of forward()'s map, bit for bit."""
    from test_matching_prep import _encoder
    from transplat_amd import kernels as K
    from transplat_amd.model.utils import cam_param_encoder as C

    enc = _encoder(device)
    feat, cam = seeded((2, 128, 8, 12), 811).to(device), seeded((2, 16), 812, 2.0).to(device)
    with torch.no_grad(), K.dense_precision("bf16x3"):
        rows = enc(feat, cam, channel_last=True)
        C._FUSE_GATE_CONV = False
        try:
            nchw = enc(feat, cam, channel_last=True)  # multiply, convolution: an NCHW map
        finally:
            C._FUSE_GATE_CONV = True
    assert rows.dim() == 3 and nchw.dim() == 4
    assert torch.equal(rows, nchw.flatten(2).transpose(1, 2).contiguous())


_GEMM: dict = {}


def _gemm_case(k1, k2, n):
    if (k1, k2, n) not in _GEMM:
        _GEMM[(k1, k2, n)] = (seeded((130, k1), 820 + k1), seeded((130, k2), 821 + k2),
                              seeded((n, k1 + k2), 822 + n, (k1 + k2) ** -0.5), seeded((n,), 823))
    return _GEMM[(k1, k2, n)]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 132])
@pytest.mark.parametrize("k1,k2", [(64, 64), (128, 128), (64, 192)])
def test_gemm_x3_cat_bit_identical(device, k1, k2, n):
    from transplat_amd import kernels as K

    x1, x2, weight, bias = [t.to(device) for t in _gemm_case(k1, k2, n)]
    for m in (1, 63, 130):
        a, b = x1[:m].contiguous(), x2[:m].contiguous()
        for ksplit in (1, 2):
            seen = []
            prev, K._lib.ROUTE_HOOK = K._lib.ROUTE_HOOK, lambda what, route=None: seen.append(what)
            try:
                out = K.gemm_x3(a, weight, bias, ksplit=ksplit, x2=b)
            finally:
                K._lib.ROUTE_HOOK = prev
            ref = K.gemm_x3(torch.cat((a, b), dim=-1), weight, bias, ksplit=ksplit)
            assert seen[-1] == "tsplat_gemm_x3_cat_fwd" and "tsplat_gemm_x3_fwd" not in seen  # (+ the weight pack)
            assert out.shape == ref.shape and torch.equal(out, ref), (m, ksplit)
    act = K.gemm_x3(x1, weight, bias, act="gelu", x2=x2)
    assert torch.equal(act, K.gemm_x3(torch.cat((x1, x2), dim=-1), weight, bias, act="gelu"))


def test_gemm_x3_cat_rejects_unaligned_split():
    """k1 must be a multiple of the kernel's 64-deep chunk (TSPLAT_EINVAL before any launch, CPU host)."""
    from transplat_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16  # never dereferenced: every call is rejected
    for k1 in (32, 96, 100):
        assert lib.tsplat_gemm_x3_cat_fwd(p, k1, p, 64, p, None, p, 8, 8, 1, 0, None) == -1
    assert lib.tsplat_gemm_x3_cat_fwd(p, 64, None, 64, p, None, p, 8, 8, 1, 0, None) == -1
    assert lib.tsplat_gemm_x3_cat_fwd(p, 64, p, 6, p, None, p, 8, 8, 1, 0, None) == -1
    assert lib.tsplat_gemm_x3_cat_fwd(p, 64, p + 4, 64, p, None, p, 8, 8, 1, 0, None) == -1
    assert lib.tsplat_conv1x1_bf16x3_scaled_fwd(p, 16, p, p, None, p, 1, 4, 4, 32, 2, 1, 1, None, None, None) == -1
    assert lib.tsplat_conv1x1_bf16x3_scaled_fwd(None, 16, p, p, None, p, 1, 4, 4, 32, 1, 1, 1, None, None, None) == -1


@pytest.mark.gpu
def test_mvt_layer_reads_source_and_message_in_place(device):
    """A multi-view transformer layer with mlp[0] on [source | message] in place against the
    materialised concatenation (bf16x3 mode)."""
    from transplat_amd import kernels as K
    from transplat_amd.model.encoder.backbone.multiview_transformer import TransformerLayer

    torch.manual_seed(7)
    layer = TransformerLayer(d_model=128, nhead=1, attention_type="swin", no_ffn=False, ffn_dim_expansion=4,
                             with_shift=False).to(device).eval()
    src = seeded((2, 16 * 16, 128), 831).to(device)
    with torch.no_grad(), K.dense_precision("bf16x3"):
        inplace = layer(src, src, height=16, width=16, attn_num_splits=2)
        K._GEMM_CAT = False
        try:
            cat = layer(src, src, height=16, width=16, attn_num_splits=2)
        finally:
            K._GEMM_CAT = True
    assert torch.equal(inplace, cat)
