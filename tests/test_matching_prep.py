"""The matching stage's camera-only work done once (tsplat_cam_gate_fwd, tsplat_pack_cameras_fwd) and its
merged projections read in place (tsplat_uv_cross_fused_ld_fwd, tsplat_uv_cross_pack_ld_fwd).

Bounds: the gate kernel against the same chain in float64, within four times the error of PyTorch's own
fp32 evaluation of that chain on the same inputs (both are fp32 sums of the same products in another
order); everything else re-arranges launches around unchanged arithmetic and is compared bit for bit.
"""
import ctypes
import sys
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_encoder_ops import _cams, seeded  # noqa: E402

_GATE: dict = {}


def _gate_case(vb):
    """Camera rows, the four layers' weights and the float64 gate of one case (shared, never modified)."""
    if vb not in _GATE:
        cam = seeded((vb, 16), 700 + vb, 2.0)
        dims = [(128, 16), (128, 128), (128, 128), (128, 128)]
        ws = [seeded(d, 710 + i, d[1] ** -0.5) for i, d in enumerate(dims)]
        bs = [seeded((128,), 720 + i, 0.5) for i in range(4)]

        def chain(x, ws, bs):
            x = torch.relu(F.linear(x, ws[0], bs[0]))
            x = F.linear(x, ws[1], bs[1])
            x = torch.relu(F.linear(x, ws[2], bs[2]))
            return torch.sigmoid(F.linear(x, ws[3], bs[3]))

        ref = chain(cam.double(), [w.double() for w in ws], [b.double() for b in bs])
        _GATE[vb] = (cam, ws, bs, chain, ref)
    return _GATE[vb]


@pytest.mark.gpu
@pytest.mark.parametrize("vb", [1, 2, 5])
def test_cam_gate_kernel_vs_float64(device, vb):
    from transplat_amd import kernels as K

    cam, ws, bs, chain, ref = _gate_case(vb)
    dcam, dws, dbs = cam.to(device), [w.to(device) for w in ws], [b.to(device) for b in bs]
    out = K.cam_gate(dcam, dws[0], dbs[0], dws[1], dbs[1], dws[2], dbs[2], dws[3], dbs[3]).cpu().double()
    torch_fp32 = chain(dcam, dws, dbs).cpu().double()
    e_kernel, e_torch = (out - ref).abs().max().item(), (torch_fp32 - ref).abs().max().item()
    print(f"cam_gate vb={vb}: kernel vs float64 {e_kernel:.3e}, torch fp32 vs float64 {e_torch:.3e}, "
          f"gate in [{ref.min().item():.3f}, {ref.max().item():.3f}]")
    assert out.shape == ref.shape
    assert e_torch > 0
    assert e_kernel <= 4 * e_torch


def _encoder(device):
    """A cam_param_encoder in eval mode with non-trivial BatchNorm statistics."""
    from transplat_amd import kernels as K
    from transplat_amd.model.utils.cam_param_encoder import cam_param_encoder

    torch.manual_seed(5)
    enc = cam_param_encoder(in_channels=128, mid_channels=128, embed_dims=128)
    for bn, seed in ((enc.bn, 731), (enc.reduce_conv[1], 732)):
        n = bn.num_features
        bn.running_mean.copy_(seeded((n,), seed, 0.3))
        bn.running_var.copy_(seeded((n,), seed + 10, 1.0, "rand") + 0.5)
        bn.weight.data.copy_(seeded((n,), seed + 20, 0.2) + 1.0)
        bn.bias.data.copy_(seeded((n,), seed + 30, 0.2))
    enc = enc.to(device).eval()
    K.install_conv2d_dispatch(enc)
    K.install_linear_dispatch(enc)
    return enc


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["fp32", "bf16x3"])
def test_cam_param_encoder_gate_argument(device, mode):
    """forward(feat, cam, gate=gate(cam)) is forward(feat, cam): the gate computed ahead is the one the
    module computes in place, and it is the module chain's gate to fp32 rounding."""
    from transplat_amd import kernels as K

    enc = _encoder(device)
    feat, cam = seeded((2, 128, 8, 8), 741).to(device), seeded((2, 16), 742, 2.0).to(device)
    with torch.no_grad(), K.dense_precision(mode):
        g = enc.gate(cam)
        assert g is not None and tuple(g.shape) == (2, 128)
        ahead, inplace = enc(feat, cam, gate=g), enc(feat, cam)
        mlp, se = enc.context_mlp, enc.context_se
        x = mlp.fc2(torch.relu(mlp.fc1(enc.bn(cam))))
        chain = torch.sigmoid(F.conv2d(torch.relu(F.conv2d(x[..., None, None], se.conv_reduce.weight,
                                                           se.conv_reduce.bias)),
                                       se.conv_expand.weight, se.conv_expand.bias)).flatten(1)
    d = (g - chain).abs().max().item()
    print(f"gate kernel vs module chain ({mode}): {d:.3e}")
    assert torch.equal(ahead, inplace)
    assert d < 1e-5  # fp32 rounding of O(1) sums through a sigmoid (slope <= 1/4); a wrong layer is O(0.1)
    assert enc.gate(cam.cpu()) is None  # host tensors: the module chain


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 7])
def test_pack_cameras_kernel_bit_identical(device, n):
    from transplat_amd import kernels as K

    intr, pose, _ = _cams(4, 16)
    intr, pose = intr[:n].contiguous().to(device), pose[:n].contiguous().to(device)
    out = K.pack_cameras_fused(intr, pose)
    assert tuple(out.shape) == (n, 30)
    assert torch.equal(out, K.pack_cameras(intr, pose))


def _cross_case(h, w, b, d):
    intr, pose, disp = _cams(b, max(h, w), d)
    value, key = seeded((b, 2, h * w, 128), 41), seeded((b, 2, h * w, 128), 42)
    ow = seeded((b * 2, h * w, d * 4 * 3), 43, 2.0)
    return value, key, intr, pose, disp.contiguous(), ow


# the smallest map of test_uv_cross_fused.py and a non-square one (HW = 15 query blocks, partial band)
@pytest.mark.gpu
@pytest.mark.parametrize("h,w,b,d", [(6, 10, 1, 5), (12, 40, 1, 33), (8, 8, 2, 128)])
def test_uv_cross_fused_reads_column_ranges(device, h, w, b, d):
    """Offsets and logits as column ranges of one [M, D * 12] buffer, value as a column range of a
    [M, 256] buffer, and the packed cameras handed in: the same bits as the contiguous call."""
    from transplat_amd import kernels as K

    value, key, intr, pose, disp, ow = [t.to(device) for t in _cross_case(h, w, b, d)]
    offsets, logits = ow[..., :d * 8], ow[..., d * 8:]
    assert not offsets.is_contiguous() and not logits.is_contiguous()
    base = K.uv_cross_fused(value, key, intr, pose, disp, offsets.contiguous(), logits.contiguous(), h, w)
    packed = K.pack_cameras_fused(intr, pose)
    both = torch.cat((seeded(tuple(value.shape), 45).to(device), value), dim=-1)  # value = columns 128:256
    seen = []
    prev, K._lib.ROUTE_HOOK = K._lib.ROUTE_HOOK, lambda what, route=None: seen.append(what)
    try:
        out = K.uv_cross_fused(both[..., 128:], key, intr, pose, disp, offsets, logits, h, w, cams_packed=packed)
        with K.dense_precision("bf16x3"):
            routed = K.uv_cross(both[..., 128:], key, intr, pose, disp, offsets, logits, h, w, cams_packed=packed)
    finally:
        K._lib.ROUTE_HOOK = prev
    assert seen.count("tsplat_uv_cross_fused_ld_fwd") == 2 and seen.count("tsplat_uv_cross_pack_ld_fwd") == 2
    assert "tsplat_small_inverse" not in seen  # the packed cameras were not rebuilt
    assert torch.equal(out, base)
    assert torch.equal(routed, base)
    # the strided pack alone
    lib = K._lib.load()
    images = []
    for src, ld in ((value.contiguous(), 128), (both[..., 128:], 256)):
        img = torch.zeros(int(lib.tsplat_uv_cross_pack_bytes(b, h, w)), dtype=torch.uint8, device=device)
        K._lib.check(lib.tsplat_uv_cross_pack_ld_fwd(K._lib.ptr(src), ld, K._lib.ptr(img), b, h, w, 128,
                                                     K._lib.stream_ptr(device)), "tsplat_uv_cross_pack_ld_fwd")
        images.append(img)
    assert torch.equal(images[0], images[1])


@pytest.mark.gpu
def test_fine_layers_merged_projections_bit_identical(device):
    """The fine transformer with one GEMM for sampling_offsets | attention_weights and one for both
    layers' value_proj (bf16x3 mode) against the same modules run one by one."""
    from transplat_amd import kernels as K
    from transplat_amd.model.utils import uv_transformer as U

    h, w, b = 8, 12, 1
    torch.manual_seed(3)
    net = U.UVTransformer(embed_dims=128, mode="fine", num_layers=2).to(device).eval()
    K.install_linear_dispatch(net)
    intr, pose, disp = [t.to(device) for t in _cams(b, max(h, w))]
    feats = seeded((b, 2, 128, h, w), 51).to(device)
    query, pos = seeded((2 * b, h * w, 128), 52).to(device), seeded((2 * b, h * w, 128), 53).to(device)
    cams = (intr, pose, disp.contiguous())
    seen = []
    prev, K._lib.ROUTE_HOOK = K._lib.ROUTE_HOOK, lambda what, route=None: seen.append(what)
    try:
        with torch.no_grad(), K.dense_precision("bf16x3"):
            merged = net([feats], query, w, h, bev_pos=pos, cameras=cams + (K.pack_cameras_fused(intr, pose),))
            n_merged, U._MERGE_PROJ = len(seen), False  # the modules one by one (their own gemm_x3 calls)
            try:
                single = net([feats], query, w, h, bev_pos=pos, cameras=cams)
            finally:
                U._MERGE_PROJ = True
    finally:
        K._lib.ROUTE_HOOK = prev
    assert "tsplat_uv_cross_fused_ld_fwd" in seen[:n_merged] and "tsplat_uv_cross_fused_ld_fwd" not in seen[n_merged:]
    assert torch.equal(merged, single)


@pytest.mark.gpu
def test_coarse_layer_without_query(device):
    from transplat_amd import kernels as K
    from transplat_amd.model.utils import uv_transformer as U

    h, w, b = 6, 10, 1
    net = U.UVTransformer(embed_dims=128, mode="coarse", num_layers=1).to(device).eval()
    intr, pose, disp = [t.to(device) for t in _cams(b, max(h, w))]
    feats = seeded((b, 2, 128, h, w), 61).to(device)
    cams = (intr, pose, disp.contiguous())
    zero = torch.zeros((2 * b, h * w, disp.shape[1]), device=device)
    with torch.no_grad():
        with_zero = net([feats], zero, w, h, cameras=cams)
        without = net([feats], None, w, h, cameras=cams + (K.pack_cameras_fused(intr, pose),))
        layer = net.encoder.layers[0].attentions[0]
        direct = layer(None, feats.flatten(3).transpose(2, 3).contiguous(), cams, h, w)
    assert torch.equal(with_zero, without)
    assert torch.equal(direct, without)


def test_new_entry_points_reject_bad_arguments():
    """TSPLAT_EINVAL before anything is launched (CPU host): null pointers, the gate's fixed widths,
    row strides shorter than a row or off the float4 grid."""
    from transplat_amd import _lib

    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = (ctypes.cast(buf, ctypes.c_void_p).value + 15) // 16 * 16  # never dereferenced: every call is rejected
    assert lib.tsplat_pack_cameras_fwd(None, p, p, 1, None) == -1
    assert lib.tsplat_pack_cameras_fwd(p, p, p, -1, None) == -1
    assert lib.tsplat_pack_cameras_fwd(p, p, p, 0, None) == 0
    assert lib.tsplat_cam_gate_fwd(*([p] * 10), 1, 8, 128, None) == -1
    assert lib.tsplat_cam_gate_fwd(*([p] * 10), 1, 16, 64, None) == -1
    assert lib.tsplat_cam_gate_fwd(*([p] * 9), None, 1, 16, 128, None) == -1
    assert lib.tsplat_cam_gate_fwd(*([p] * 10), 0, 16, 128, None) == 0
    assert lib.tsplat_uv_cross_pack_ld_fwd(p, 64, p, 1, 4, 4, 128, None) == -1
    assert lib.tsplat_uv_cross_pack_ld_fwd(p, 130, p, 1, 4, 4, 128, None) == -1
    fused = lambda ldo, ldl: lib.tsplat_uv_cross_fused_ld_fwd(p, p, p, p, p, ldo, p, ldl, p, 1, 4, 4, 128, 2, 4, None)
    assert fused(15, 8) == -1 and fused(16, 7) == -1    # shorter than depths x points (x 2)
    assert fused(18, 8) == -1 and fused(16, 10) == -1   # 4 points: float4 rows
